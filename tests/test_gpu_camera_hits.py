"""GPU tests (-m gpu) of the camera-hit pass: a call of accumulator that renders two or more frames walks every camera ray once
(lt_camera_hits_kernel) and its render launches shade from the stored hits; basic_lighting walks its camera ray once for its 25
samples.  Neither may change a bit: every case is compared with LT_CAMERA_HITS=0 (every launch walks its camera rays), and
basic_lighting with the CPU oracle.  LT_DEBUG_CAMERA_HITS=1 has the library say on stderr whenever a call runs the pass, and how
many squares it walks: the tests check that the pass ran where it should, and only there."""
import re
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import RendererHIP, make_desc
from oracle import pyoracle as po
from tests.conftest import oracle_props

pytestmark = pytest.mark.gpu
CAM = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)   # the reference camera: the synthetic scenes fill its view


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def wall():
    return synth.heightfield_wall(48).validate()


@pytest.fixture(scope="module")
def soup():
    return synth.triangle_soup(3000).validate()


@pytest.fixture(autouse=True)
def fixed_shadow_walk(monkeypatch):
    """One shadow-ray walk per test unless it says otherwise: no timing launches between the two calls compared."""
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")


def render(r, scene, W, H, cam=CAM, program=C.PROGRAM_ACCUMULATOR, first=1, count=6, base=0, accumulate=True, tile=None, stats=False):
    """One call through lt_hip_render; the output starts from a fixed pattern (a running mean with accumulate_base > 0 reads it)."""
    r.set_scene(scene)
    d = make_desc(program, W, H, 3, cam, frame_first=first, frame_count=count, accumulate=accumulate, accumulate_base=base,
                  tile=tile, stats=stats)
    n = r.output_floats(d)
    out = (np.arange(n, dtype=np.float32) % 7.0) / 7.0
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out, r.stats()


@pytest.fixture(autouse=True)
def report_the_pass(monkeypatch):
    monkeypatch.setenv("LT_DEBUG_CAMERA_HITS", "1")


def passes(capfd):
    """(squares walked, squares of the call) of every camera-hit pass since the last look (the library's stderr)."""
    return [tuple(map(int, m)) for m in re.findall(r"camera-hit pass: (\d+) of (\d+) squares", capfd.readouterr().err)]


def on_off(monkeypatch, fn, capfd=None, ran=True):
    """fn() with the pass, then without; with capfd: checks that the first call ran one pass (ran) or none, the second none."""
    if capfd is not None:
        passes(capfd)
    monkeypatch.setenv("LT_CAMERA_HITS", "1")
    a = fn()
    if capfd is not None:
        got = passes(capfd)
        assert len(got) == (1 if ran else 0) and all(0 < w <= n for w, n in got), got
    monkeypatch.setenv("LT_CAMERA_HITS", "0")
    b = fn()
    monkeypatch.delenv("LT_CAMERA_HITS")
    if capfd is not None:
        assert passes(capfd) == []
    return a, b


def assert_same(a, b):
    (oa, sa), (ob, sb) = a, b
    assert np.array_equal(oa, ob, equal_nan=True), int((oa != ob).sum())
    assert sa["kernel_launches"] == sb["kernel_launches"] and sa["frames"] == sb["frames"]


@pytest.mark.parametrize("mode", ["0", "1", "2", "3"], ids=["per-lane", "packets", "per-wavefront", "queued"])
@pytest.mark.parametrize("name", ["wall", "soup"])
def test_accumulator_every_shadow_walk(renderer, monkeypatch, capfd, request, mode, name):
    monkeypatch.setenv("LT_SHADOW_PACKETS", mode)
    scene = request.getfixturevalue(name)
    a, b = on_off(monkeypatch, lambda: render(renderer, scene, 96, 64), capfd)
    assert a[1]["shadow_packets"] == int(mode)
    assert_same(a, b)


def test_basic_lighting_walks_its_camera_ray_once_and_matches_the_oracle(renderer, wall):
    W, H = 24, 16
    cam = sc.camera_with_frame(CAM, 3)
    out = np.full((H, W, 3), np.nan, dtype=np.float32)
    renderer.render(oracle_props("resources/kernels/opencl/basic_lighting.cl", (W, H, 3), out, wall, pCamera=cam))
    assert np.array_equal(out, po.render(wall, cam, W, H, po.PROGRAMS["basic_lighting"]))


def test_basic_lighting_several_frames_match_the_oracle(renderer, capfd, wall):
    """Several frames of a running mean (a fused launch): each frame's 25 samples shade the one walk of the camera ray."""
    W, H, first, count = 16, 12, 2, 3
    out = np.full((H, W, 3), np.nan, dtype=np.float32)
    passes(capfd)
    renderer.render(oracle_props("resources/kernels/opencl/basic_lighting.cl", (W, H, 3), out, wall, pCamera=CAM, frameFirst=first,
                                 frameCount=count, accumulate=True))
    assert passes(capfd) == []   # (basic_lighting needs no pass: its hoist is in registers)
    acc = np.zeros((H, W, 3), dtype=np.float32)
    for i, f in enumerate(range(first, first + count)):
        po.accumulate(acc, po.render(wall, sc.camera_with_frame(CAM, f), W, H, po.PROGRAMS["basic_lighting"]), i)
    assert np.array_equal(out, acc)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_fused_and_one_launch_per_frame(renderer, monkeypatch, capfd, wall, fused):
    monkeypatch.setenv("LT_FUSED_FRAMES", fused)
    a, b = on_off(monkeypatch, lambda: render(renderer, wall, 80, 56, count=5), capfd)
    assert a[1]["kernel_launches"] == (1 if fused == "1" else 5)
    assert_same(a, b)


def test_frames_in_several_fused_chunks(renderer, monkeypatch, capfd, wall):
    W, H = 72, 40
    monkeypatch.setenv("LT_FUSED_BYTES", str(3 * W * H * 3 * 4 + 100))   # three sample images per launch: 3 + 3 + 1
    a, b = on_off(monkeypatch, lambda: render(renderer, wall, W, H, count=7), capfd)   # (one pass serves the three launches)
    assert a[1]["kernel_launches"] == 3
    assert_same(a, b)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_frame_first_and_accumulate_base(renderer, monkeypatch, wall, fused):
    monkeypatch.setenv("LT_FUSED_FRAMES", fused)
    assert_same(*on_off(monkeypatch, lambda: render(renderer, wall, 64, 48, first=11, count=4, base=5)))


def test_frames_without_a_running_mean(renderer, monkeypatch, wall):
    assert_same(*on_off(monkeypatch, lambda: render(renderer, wall, 64, 48, count=3, accumulate=False)))


@pytest.mark.parametrize("W,H,tile", [(100, 70, (20, 12, 0, 1)), (128, 96, (16, 16, 3, 8)), (131, 77, (24, 20, 1, 3))],
                         ids=["tiles-not-multiples-of-8", "strided-like-a-multi-gpu-share", "strided-ragged"])
def test_tiled_calls(renderer, monkeypatch, capfd, wall, W, H, tile):
    assert_same(*on_off(monkeypatch, lambda: render(renderer, wall, W, H, tile=tile), capfd))


@pytest.mark.parametrize("yaw", [0.3, -0.7])
def test_rotated_camera(renderer, monkeypatch, capfd, wall, yaw):
    cam = sc.camera_bytes(0.5, 2.5, -50.0, yaw, 0.0, 0.0, 1)
    assert_same(*on_off(monkeypatch, lambda: render(renderer, wall, 96, 64, cam=cam), capfd))


def test_the_head_squares_stay_out_of_the_pass(renderer, monkeypatch, capfd, wall):
    """96 x 64 pixels, unrotated camera: 12 x 8 squares; the centre column's 8 and the centre row's 12 (one in common) start the
    render launch and walk there; with the natural order there is no head."""
    render(renderer, wall, 96, 64)
    monkeypatch.setenv("LT_NATURAL_ORDER", "1")
    render(renderer, wall, 96, 64)
    assert passes(capfd) == [(96 - 19, 96), (96, 96)]


def test_natural_order(renderer, monkeypatch, capfd, wall):
    monkeypatch.setenv("LT_NATURAL_ORDER", "1")
    assert_same(*on_off(monkeypatch, lambda: render(renderer, wall, 96, 64), capfd))


def test_one_frame_call(renderer, monkeypatch, capfd, wall):
    assert_same(*on_off(monkeypatch, lambda: render(renderer, wall, 96, 64, count=1), capfd, ran=False))


def test_no_hit_carries_over_to_the_next_call(renderer, monkeypatch, wall, soup):
    monkeypatch.setenv("LT_CAMERA_HITS", "1")
    moved = sc.camera_bytes(1.5, 3.0, -45.0, 0.05, 0.0, 0.0, 1)
    render(renderer, wall, 96, 64)
    after_move = render(renderer, wall, 96, 64, cam=moved)
    render(renderer, wall, 96, 64)
    after_edit = render(renderer, soup, 96, 64)   # another scene through lt_hip_set_scene, same image
    fresh = RendererHIP(0)
    try:
        assert_same(after_move, render(fresh, wall, 96, 64, cam=moved))
        fresh.close()
        fresh = RendererHIP(0)
        assert_same(after_edit, render(fresh, soup, 96, 64))
    finally:
        fresh.close()


def test_counting_call_counts_the_same_work(renderer, monkeypatch, capfd, wall):
    """A counting call walks every camera ray per frame, pass or no pass: its counts are the reference algorithm's."""
    a, b = on_off(monkeypatch, lambda: render(renderer, wall, 64, 48, count=4, stats=True), capfd, ran=False)
    assert_same(a, b)
    for k in ("rays", "shadow_rays", "node_visits", "tri_tests"):
        assert a[1][k] == b[1][k] and a[1][k] > 0, k
