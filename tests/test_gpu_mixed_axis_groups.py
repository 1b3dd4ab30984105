"""GPU tests (-m gpu) of the two-frame shadow walk's one-mixed-axis forms (lt_walk_asm.hpp: LT_NF_X0 .. LT_NF_Z3; lt_device.hpp:
traverse_shadow2): a square whose two frames' shadow rays have mixed direction signs along exactly one axis walks them together.
Not a bit may change: every call is compared with LT_SHADOW_FRAMES=1 (a work item per frame, each frame's own walk) in the default
and the portable flavour, and in the portable flavour with the CPU oracle's frames folded by its own running mean.

The scenes come from tests/mixed_axis_scenes.py, whose construction tests/test_mixed_axis_scenes_cpu.py checks: one scene per form,
every call of which has a square of that form (LT_DEBUG_SHADOW_FRAMES reports the together-walks per form); a scene with squares
of two mixed axes, which render apart; a penumbra under a light that straddles the floor.  17x9 ends in a one-column square and a
single-pixel square: the walk runs with lanes off and its stack register parked."""
import re

import numpy as np
import pytest

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, RenderPropertiesHIP
from oracle import pyoracle as po
from tests import mixed_axis_scenes as mx
from tests import penumbra_scenes as ps
from tests.conftest import oracle_props

pytestmark = pytest.mark.gpu

ACCUMULATOR = "examples/accumulator/resources/kernels/accumulator.cl"
LINE = re.compile(r"shadow-ray frame groups: (\d+) \(walk (\d+), (\d+) frames\)(?:: (\d+) waves walked both frames together, (\d+) apart; "
                  r"of those together, one mixed axis: x (\d+) (\d+) (\d+) (\d+), y (\d+) (\d+) (\d+) (\d+), z (\d+) (\d+) (\d+) (\d+))?")


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no calibration launches: the packet walk, frame groups
    monkeypatch.setenv("LT_DEBUG_SHADOW_FRAMES", "1")


def launches(capfd):
    """Of every render launch since the last look: (frames per work item, walk, frames, together, apart, [12 per-form counts])."""
    out = []
    for m in LINE.findall(capfd.readouterr().err):
        n = [int(v) if v else 0 for v in m]
        out.append((n[0], n[1], n[2], n[3], n[4], n[5:]))
    return out


def hip(renderer, s, W, H, cam, start, first, count, base, portable):
    out = start.copy()
    props = oracle_props if portable else RenderPropertiesHIP
    renderer.render(props(ACCUMULATOR, (W, H, 3), out, s, pCamera=cam, frameFirst=first, frameCount=count, accumulate=True, accumulateBase=base))
    return out


def assert_same(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), got.size)


def check_calls(renderer, monkeypatch, capfd, s, cam0, sizes, what, firsts=mx.FIRSTS, counts=mx.COUNTS):
    """Every call of the case -- size, first frame, frame count -- grouped against LT_SHADOW_FRAMES=1 (both flavours) and against the
    oracle's frames folded (portable); returns the grouped launches' lines."""
    seen = []
    rng = np.random.default_rng(len(what))
    for W, H in sizes:
        frames = {}
        start = rng.random((H, W, 3), dtype=np.float32)
        for first in firsts:
            cam = sc.camera_with_frame(cam0, first)
            base = 0 if first == firsts[0] else 3
            for count in counts:
                for portable in (True, False):
                    tag = "%s %dx%d frames %d..%d base %d %s" % (what, W, H, first, first + count - 1, base, "portable" if portable else "default")
                    launches(capfd)
                    got = hip(renderer, s, W, H, cam, start, first, count, base, portable)
                    g = launches(capfd)
                    assert g and all(x[:3] == (2, 1, count) for x in g), (tag, g)    # (a scene handed over anew is rendered again)
                    seen.append((W, H, first, count, portable) + g[-1][3:])
                    monkeypatch.setenv("LT_SHADOW_FRAMES", "1")
                    alone = hip(renderer, s, W, H, cam, start, first, count, base, portable)
                    assert all(x[0] == 1 for x in launches(capfd))
                    monkeypatch.delenv("LT_SHADOW_FRAMES")
                    assert_same(got, alone, tag + " vs LT_SHADOW_FRAMES=1")
                    if portable:
                        acc = start.copy()
                        for i in range(count):
                            f = first + i
                            if f not in frames:
                                frames[f] = po.render(s, sc.camera_with_frame(cam0, f), W, H, po.ACCUMULATOR)
                            po.accumulate(acc, frames[f], base + i)
                        assert_same(got, acc, tag + " vs the oracle's frames folded")
    return seen


@pytest.mark.parametrize("axis,k", mx.FORMS, ids=["%s%d" % ("xyz"[a], k) for a, k in mx.FORMS])
def test_one_mixed_axis_form(renderer, monkeypatch, capfd, axis, k):
    form = mx.form_index(axis, k)
    s = mx.mixed_scene(axis, k)
    seen = check_calls(renderer, monkeypatch, capfd, s, mx.camera(form, 0), mx.SIZES, "form %s%d" % ("xyz"[axis], k))
    for W, H, first, count, portable, together, apart, per_form in seen:
        # (tests/test_mixed_axis_scenes_cpu.py: the first group of every call has a square of this form, and no square of another)
        assert per_form[form - 8] > 0, (W, H, first, count, portable, per_form)
        assert sum(per_form) == per_form[form - 8] and together >= per_form[form - 8], (per_form, together)


def test_two_mixed_axes_render_apart(renderer, monkeypatch, capfd):
    seen = check_calls(renderer, monkeypatch, capfd, mx.two_axis_scene(), mx.camera(0, 0), mx.SIZES, "two axes")
    for W, H, first, count, portable, together, apart, per_form in seen:
        assert apart > 0, (W, H, first, count, portable, together, apart)


@pytest.mark.parametrize("name", sorted(mx.PENUMBRA_CASES))
def test_penumbra_under_a_straddling_light(renderer, monkeypatch, capfd, name):
    c = mx.PENUMBRA_CASES[name]
    seen = check_calls(renderer, monkeypatch, capfd, mx.penumbra_scene(name), ps.CAM, ((c["W"], c["H"]),), "penumbra " + name)
    form = mx.form_index(*mx.PENUMBRA_FORM)
    for W, H, first, count, portable, together, apart, per_form in seen:
        assert per_form[form - 8] > 0, (first, count, portable, per_form)


def test_per_wavefront_packets(renderer, monkeypatch, capfd):
    """LT_SHADOW_PACKETS=2 (a wave walks as a packet where its rays pass the spread test): bit equality only."""
    monkeypatch.setenv("LT_SHADOW_PACKETS", "2")
    monkeypatch.setenv("LT_SHADOW_SPREAD", "100")
    axis, k = 2, 1
    s = mx.mixed_scene(axis, k)
    cam0 = mx.camera(mx.form_index(axis, k), 0)
    rng = np.random.default_rng(5)
    for W, H in mx.SIZES:
        start = rng.random((H, W, 3), dtype=np.float32)
        for first, count, base in ((1, 5, 0), (4, 3, 3)):
            cam = sc.camera_with_frame(cam0, first)
            got = hip(renderer, s, W, H, cam, start, first, count, base, True)
            assert any(x[:3] == (2, 2, count) for x in launches(capfd))
            monkeypatch.setenv("LT_SHADOW_FRAMES", "1")
            alone = hip(renderer, s, W, H, cam, start, first, count, base, True)
            monkeypatch.delenv("LT_SHADOW_FRAMES")
            assert_same(got, alone, "walk 2 %dx%d first %d count %d vs LT_SHADOW_FRAMES=1" % (W, H, first, count))
            acc = start.copy()
            for i in range(count):
                po.accumulate(acc, po.render(s, sc.camera_with_frame(cam0, first + i), W, H, po.ACCUMULATOR), base + i)
            assert_same(got, acc, "walk 2 %dx%d first %d count %d vs the oracle" % (W, H, first, count))
