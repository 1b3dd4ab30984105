"""CPU tests of tests/mixed_axis_scenes.py: at the sizes and frames tests/test_gpu_mixed_axis_groups.py renders, the scenes have the
squares the GPU tests rely on -- a frame pair whose shadow rays are mixed along exactly the scene's axis with the prescribed signs
along the other two (the walk's one-mixed-axis form of that scene), a pair with two mixed axes in the two-axis scene, and in the
penumbra scene a pixel of a mixed square that is lit in one frame of its pair and dark in the other."""
import numpy as np
import pytest

from lens_trace_amd import scene as sc
from oracle import pyoracle as po
from tests import mixed_axis_scenes as mx
from tests import octant_scenes as oc
from tests import penumbra_scenes as ps


@pytest.mark.parametrize("axis,k", mx.FORMS)
def test_the_light_lies_on_both_sides_along_the_axis_only(axis, k):
    s = mx.form_signs(axis, k)
    P, _, _, _, light = mx.triangles(s, mx.form_index(axis, k))
    assert light.sum() >= 2 and not light[0]
    lo, hi = mx.light_box(s)
    lp = P[light].reshape(-1, 3)
    assert (lp >= lo - 1e-6).all() and (lp <= hi + 1e-6).all()
    assert (np.abs(P[~light]) <= mx.BOX).all()
    assert lo[axis] < -mx.BOX and hi[axis] > mx.BOX                      # every point of B has the light on both sides
    assert (P[light][:, :, axis].min(axis=1) == np.float32(lo[axis])).all() and (P[light][:, :, axis].max(axis=1) == np.float32(hi[axis])).all()
    for a in range(3):
        if a != axis:                                                     # ... and wholly on the prescribed side elsewhere
            assert ((lo[a] - mx.BOX >= 5.0) if s[a] > 0 else (-mx.BOX - hi[a] >= 5.0)), a


@pytest.mark.parametrize("axis,k", mx.FORMS)
def test_every_call_has_a_square_of_the_scenes_form(axis, k):
    form = mx.form_index(axis, k)
    scene = mx.mixed_scene(axis, k)
    for W, H in mx.SIZES:
        hits = None
        for first in mx.FIRSTS:
            cam = mx.camera(form, first)
            seen = set()
            for pair in mx.call_pairs(first, max(mx.COUNTS)):
                forms, _, hits = mx.square_forms(scene, cam, W, H, pair, hits)
                got = set(f for f in forms if f is not None)
                # whatever the draws, a square is in the octants / forms the light's placement allows
                assert got <= {form} | {o for o in range(8) if all(((o >> a) & 1) == (mx.form_signs(axis, k)[a] < 0) for a in range(3) if a != axis)}, got
                if pair == first:
                    assert form in got, (W, H, first, forms)             # the one group of a call of 2 or 3 frames
                seen |= got
            assert form in seen


def test_the_two_axis_scene_has_squares_with_two_mixed_axes():
    scene = mx.two_axis_scene()
    for W, H in mx.SIZES:
        for first in mx.FIRSTS:
            forms, _, _ = mx.square_forms(scene, mx.camera(0, first), W, H, first)
            assert -2 in forms, (W, H, first, forms)


@pytest.mark.parametrize("name", sorted(mx.PENUMBRA_CASES))
def test_a_pixel_of_a_mixed_square_flips_between_the_frames_of_a_pair(name):
    c = mx.PENUMBRA_CASES[name]
    W, H = c["W"], c["H"]
    scene = mx.penumbra_scene(name)
    want = mx.form_index(*mx.PENUMBRA_FORM)
    hits = None
    for first in mx.FIRSTS:
        forms, lanes, hits = mx.square_forms(scene, sc.camera_with_frame(ps.CAM, first), W, H, first, hits)
        to_dark, to_lit = ps.flips(scene, ps.CAM, W, H, first)
        flipped = to_dark | to_lit
        assert any(f == want and flipped[ys, xs].any() for f, (ys, xs) in zip(forms, lanes)), (first, forms)
    # the last square of 17x9's first row has one column, its last square a single pixel
    if name == "17x9":
        assert [ys.size for ys, _ in lanes][-3:] == [8, 8, 1] and lanes[2][0].shape == (8, 1)


def test_shadow_directions_are_the_oracles():
    """The reconstruction agrees with the oracle's frame: a pixel whose shadow ray -- from the hit's position along the direction, as
    long as the distance less the shadow epsilon, past the primitive it starts on -- meets a triangle is black."""
    scene = mx.mixed_scene(0, 0)
    W, H, frame = 24, 16, 1
    cam = mx.camera(8, frame)
    hits = mx.camera_hits(scene, cam, W, H)
    d = mx.shadow_directions(scene, hits, frame)
    img = po.render(scene, cam, W, H, po.ACCUMULATOR)
    blocked = lit = 0
    for y, x in zip(*np.nonzero(hits[0])):
        n = np.linalg.norm(d[y, x])
        hit, _, _ = po.trace(scene, np.append(hits[1][y, x], np.float32(1)), np.append((d[y, x] / n).astype(np.float32), np.float32(0)),
                             tmax=float(n) - 0.01, ignore=int(hits[3][y, x]))
        if hit:
            assert img[y, x].max() == 0.0, (x, y)
            blocked += 1
        else:
            lit += int(img[y, x].max() > 0.0)
    assert blocked >= 10 and lit >= 10
