"""CPU tests of tests/penumbra_scenes.py: the scene and the calls of tests/test_gpu_penumbra.py have what the GPU tests rely on --
every shadow ray in one direction-sign octant (a square's frame groups walk together), and pixels that are lit in one frame of a
two-frame group and dark in the other, in both orders: where the frames' rays part at the occluder's box."""
import numpy as np
import pytest

from tests import penumbra_scenes as ps
from tests import octant_scenes as oc


def test_every_shadow_ray_has_one_octant():
    fp, _ = ps.floor_triangles()
    lp, _ = ps.light_triangles()
    rng = np.random.default_rng(3)

    def points(tris, k):
        uv = rng.uniform(0, 1, (k, 2))
        uv = np.where(uv.sum(axis=1, keepdims=True) > 1, 1 - uv, uv)
        w = np.concatenate([1 - uv.sum(axis=1, keepdims=True), uv], axis=1).astype(np.float32)
        return np.concatenate([np.einsum("kj,njc->nkc", w, tris).reshape(-1, 3), tris.reshape(-1, 3)]).astype(np.float32)

    d = points(lp, 64)[None, :, :] - points(fp, 256)[:, None, :]
    assert (oc.octant_of(d) == ps.OCTANT).all()
    assert np.abs(d).min() >= 2.0                       # far above any rounding
    assert np.allclose(lp.reshape(-1, 3).mean(axis=0), ps.LIGHT_CENTRE)


@pytest.mark.parametrize("name", sorted(ps.CASES))
def test_the_scene_is_five_triangles_with_the_occluder_between(name):
    c = ps.CASES[name]
    target = ps.floor_point(ps.CAM, c["W"], c["H"], *c["target"])
    P, _, M, m = ps.penumbra_triangles(target)
    assert P.shape == (5, 3, 3) and list(M) == [0, 0, 1, 2, 2] and m[2]["emission"][0] == 1.0
    (x0, x1), (y0, y1), (z0, z1) = ps.FLOOR_X, ps.FLOOR_Y, ps.FLOOR_Z
    assert x0 < target[0] < x1 and y0 < target[1] < y1 and z0 < target[2] < z1     # the pixel's ray meets the floor quad
    occ = P[2]
    # strictly between the floor point and the light on every axis, and small against the light's distance
    lo, hi = np.minimum(target, ps.LIGHT_CENTRE), np.maximum(target, ps.LIGHT_CENTRE)
    assert (occ > lo).all() and (occ < hi).all()
    assert np.ptp(occ, axis=0).max() < 1.5


@pytest.mark.parametrize("name", sorted(ps.CASES))
def test_pixels_flip_between_the_frames_of_a_group(name):
    c = ps.CASES[name]
    W, H = c["W"], c["H"]
    s = ps.case_scene(name)
    seen = [False, False]
    for first in c["firsts"]:
        to_dark, to_lit = ps.flips(s, ps.CAM, W, H, first)      # the group (first, first + 1) of a call of 2 or 3 frames
        seen[0] |= bool(to_dark.any())
        seen[1] |= bool(to_lit.any())
        assert to_dark.any() or to_lit.any(), first
        if c["watch"] is None:
            assert to_dark.any() and to_lit.any(), first        # both orders inside one group's image
    assert seen == [True, True]


@pytest.mark.parametrize("name", [n for n in sorted(ps.CASES) if ps.CASES[n]["watch"]])
def test_the_watched_pixel_flips_once_in_each_order(name):
    """The single valid pixel of the 9x9 corner square (the one valid column's pixel of 17x9): lit then dark in the first call's group,
    dark then lit in the second's."""
    c = ps.CASES[name]
    W, H = c["W"], c["H"]
    x, y = c["watch"]
    assert x == W - 1 and x % 8 == 0                            # the last square of its row: one valid column
    if name == "9x9":
        assert y == H - 1 and y % 8 == 0                        # ... and one valid row: a single pixel
    s = ps.case_scene(name)
    a, b = c["firsts"]
    assert ps.flips(s, ps.CAM, W, H, a)[0][y, x]                # lit in a, dark in a + 1
    assert ps.flips(s, ps.CAM, W, H, b)[1][y, x]                # dark in b, lit in b + 1
