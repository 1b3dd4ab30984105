"""GPU tests (-m gpu) of the two-frame walk's leaf (lt_walk_asm.hpp: LT_ASM_TRI2_TVEC / LT_ASM_TRI2_PART1 / LT_ASM_TRI2_PART2;
lt_device.hpp: leaf2_frame), which computes tvec once per leaf record for both frames, under the union of their lane masks, and
leaves out the four terms that restate dot4's zero `a.w * b.w` product.  Not a bit may change: every call is compared with
LT_SHADOW_FRAMES=1 (each frame's own one-frame walk, whose leaf computes everything per frame and keeps the four terms) in the
default and the portable flavour, and in the portable flavour with the CPU oracle's frames folded by its own running mean.
LT_DEBUG_SHADOW_FRAMES must report waves that walked both frames together in every call, so that the new leaf really ran.

The checks are tests/test_gpu_mixed_axis_groups.py's check_calls; the scenes come from tests/mixed_axis_scenes.py's builders and, for
the wall kind that bench.py measures, lens_trace_amd.synth.heightfield_wall(24) under its own light.  Sizes 24x16, 17x9 and 9x9,
2, 3 and 5 frames from frame 1 and from frame 4, are the smallest shapes that still give, within one wave:
  * leaves where both frames pass the u test (neighbouring cells of the wall near the rays' origin; the random triangles),
  * leaves where only frame 0 or only frame 1 passes (two samples of one light on either side of a triangle's edge),
  * a lane closed in one frame and open in the other at a later leaf (the penumbra: one sample hidden, the other not),
  * a one-column square and a one-pixel square (17x9, 9x9: the walk runs with lanes off and EXEC = open | open_1 is no full mask)."""
import pytest

from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import RendererHIP
from tests import mixed_axis_scenes as mx
from tests import penumbra_scenes as ps
from tests import test_gpu_mixed_axis_groups as groups

pytestmark = pytest.mark.gpu

SIZES = ((24, 16), (17, 9), (9, 9))
MIXED_FORMS = ((0, 2), (2, 1))     # x mixed / y > 0 / z < 0 (the wall's commonest mixed form) and z mixed / x < 0 / y > 0


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no calibration launches: the packet walk, frame groups
    monkeypatch.setenv("LT_DEBUG_SHADOW_FRAMES", "1")


def assert_walked_together(seen):
    assert seen
    for W, H, first, count, portable, together, apart, per_form in seen:
        assert together > 0, (W, H, first, count, portable, together, apart, per_form)


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_wall(renderer, monkeypatch, capfd, size):
    s = synth.heightfield_wall(24).validate()
    cam0 = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
    assert_walked_together(groups.check_calls(renderer, monkeypatch, capfd, s, cam0, (size,), "leaf2 wall"))


@pytest.mark.parametrize("axis,k", MIXED_FORMS, ids=["%s%d" % ("xyz"[a], k) for a, k in MIXED_FORMS])
def test_random_triangles(renderer, monkeypatch, capfd, axis, k):
    form = mx.form_index(axis, k)
    seen = groups.check_calls(renderer, monkeypatch, capfd, mx.mixed_scene(axis, k), mx.camera(form, 0), SIZES, "leaf2 form %s%d" % ("xyz"[axis], k))
    assert_walked_together(seen)


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_penumbra(renderer, monkeypatch, capfd, size):
    W, H = size
    P, N, M, m = mx.penumbra_triangles(ps.floor_point(ps.CAM, W, H, W // 2, H // 2))
    s = sc.build_from_triangles(P, N, M, m).validate()
    assert_walked_together(groups.check_calls(renderer, monkeypatch, capfd, s, ps.CAM, (size,), "leaf2 penumbra"))
