"""GPU tests (-m gpu) of accumulator's frame groups: in a call whose camera hits are stored (lt_camera_hits_kernel), a work item of
the render launch covers two consecutive frames of a square, whose shadow rays leave the same points and walk the tree together
(shade_pixel2, packet_anyhit_walk2).  Not a bit may change: every case is compared with LT_SHADOW_FRAMES=1 (a work item per frame,
each frame's own walk), one with the CPU oracle.  LT_DEBUG_SHADOW_FRAMES=1 has the library say on stderr, for every render launch,
how many frames its work items cover and, where they cover two, how many waves walked both frames' shadow rays together and how many
rendered them apart (traverse_shadow2 found the rays of different octants, or not packets): the tests check that groups ran where they
should, and only there, and that both kinds of waves occur.  Without a walk forced, the calibration times walk 1 with groups and walk 2
without, and keeps what was faster."""
import ctypes
import os
import re

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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def wall():
    return synth.heightfield_wall(48).validate()


@pytest.fixture(scope="module")
def cornell():
    """The light in the ceiling, over the floor: a floor point's shadow rays towards two points of the light often differ in the
    sign of a direction component, so those waves' groups take each frame's own walk (traverse_shadow2)."""
    return sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches between the two calls compared
    monkeypatch.setenv("LT_DEBUG_SHADOW_FRAMES", "1")


def render(r, scene, W, H, cam=CAM, first=1, count=6, base=0, accumulate=True, stats=False):
    """One call through lt_hip_render; the output starts from a fixed pattern (a running mean with accumulate_base > 0 reads it)."""
    r.set_scene(scene)
    d = make_desc(C.PROGRAM_ACCUMULATOR, W, H, 3, cam, frame_first=first, frame_count=count, accumulate=accumulate,
                  accumulate_base=base, stats=stats)
    n = r.output_floats(d)
    out = (np.arange(n, dtype=np.float32) % 7.0) / 7.0
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out, r.stats()


WAVES = []   # (together, apart) of every launch with groups that groups() has seen, latest last


def groups(capfd):
    """(frames per work item, shadow walk, frames of the launch) of every render launch since the last look."""
    got = re.findall(r"shadow-ray frame groups: (\d+) \(walk (\d+), (\d+) frames\)(?:: (\d+) waves walked both frames together, (\d+) apart)?",
                     capfd.readouterr().err)
    WAVES.extend((int(m[3]), int(m[4])) for m in got if m[3])
    return [tuple(map(int, m[:3])) for m in got]


def grouped_and_not(monkeypatch, capfd, fn):
    """fn() with the default groups, then with LT_SHADOW_FRAMES=1; returns both results and the launches' groups of each."""
    groups(capfd)
    a = fn()
    ga = groups(capfd)
    monkeypatch.setenv("LT_SHADOW_FRAMES", "1")
    b = fn()
    gb = groups(capfd)
    monkeypatch.delenv("LT_SHADOW_FRAMES")
    assert gb and all(g[0] == 1 for g in gb), gb
    return a, b, ga


def assert_same(a, b):
    (oa, sa), (ob, sb) = a, b
    assert np.array_equal(oa, ob, equal_nan=True), int((oa != ob).sum())
    assert sa["kernel_launches"] == sb["kernel_launches"] and sa["frames"] == sb["frames"]


@pytest.mark.parametrize("count", [2, 3, 7, 16])
@pytest.mark.parametrize("base", [0, 5], ids=["base0", "base5"])
def test_frame_counts(renderer, monkeypatch, capfd, wall, count, base):
    a, b, ga = grouped_and_not(monkeypatch, capfd, lambda: render(renderer, wall, 96, 64, count=count, base=base))
    assert ga == [(2, 1, count)]
    assert_same(a, b)


@pytest.mark.parametrize("mode", ["1", "2"], ids=["packets", "per-wavefront"])
@pytest.mark.parametrize("name", ["wall", "cornell"])
def test_shadow_walks(renderer, monkeypatch, capfd, request, mode, name):
    monkeypatch.setenv("LT_SHADOW_PACKETS", mode)
    scene = request.getfixturevalue(name)
    a, b, ga = grouped_and_not(monkeypatch, capfd, lambda: render(renderer, scene, 96, 64, count=5))
    assert ga == [(2, int(mode), 5)]
    together, apart = WAVES[-1]
    if mode == "1":
        assert together > 0, WAVES[-1]   # the two-frame walk ran
        if name == "cornell":
            assert apart > 0, WAVES[-1]  # ... and so did the fallback
    else:   # (at 96 x 64 pixels a square's hit points lie too far apart for walk 2's packets: its groups render apart)
        assert together + apart > 0, WAVES[-1]
    assert a[1]["shadow_packets"] == int(mode)
    assert_same(a, b)


def test_rotated_camera(renderer, monkeypatch, capfd, cornell):
    cam = sc.camera_bytes(0.5, 2.5, -50.0, 0.3, 0.0, 0.0, 1)
    a, b, ga = grouped_and_not(monkeypatch, capfd, lambda: render(renderer, cornell, 80, 72, cam=cam, count=4))
    assert ga == [(2, 1, 4)]
    assert_same(a, b)


@pytest.mark.parametrize("mode", ["0", "3"], ids=["per-lane", "queued"])
def test_no_groups_for_the_other_walks(renderer, monkeypatch, capfd, wall, mode):
    monkeypatch.setenv("LT_SHADOW_PACKETS", mode)
    groups(capfd)
    render(renderer, wall, 96, 64, count=4)
    assert groups(capfd) == [(1, int(mode), 4)]


def test_no_groups_in_one_frame_or_counting_calls_or_without_stored_hits(renderer, monkeypatch, capfd, wall):
    groups(capfd)
    render(renderer, wall, 96, 64, count=1)
    assert groups(capfd) == [(1, 1, 1)]
    render(renderer, wall, 64, 48, count=4, stats=True)   # (a counting call renders a frame per launch)
    assert groups(capfd) == [(1, 1, 1)] * 4
    monkeypatch.setenv("LT_CAMERA_HITS", "0")
    render(renderer, wall, 96, 64, count=4)
    assert groups(capfd) == [(1, 1, 4)]


def test_the_library_chooses_the_walk(renderer, monkeypatch, capfd, wall):
    """No walk forced: the calibration times walk 1 with groups and walk 2 without, then the call keeps its choice and its groups."""
    monkeypatch.delenv("LT_SHADOW_PACKETS")
    fresh = RendererHIP(0)
    try:
        groups(capfd)
        out, st = render(fresh, wall, 96, 64, count=4)
        got = groups(capfd)
        mode = st["shadow_packets"]
        assert (2 if mode == 1 else 1, mode, 4) == got[-1]
        assert {(g[1], g[0]) for g in got[:-1]} >= {(1, 2), (0, 1), (2, 1)}, got
        monkeypatch.setenv("LT_SHADOW_PACKETS", str(mode))
        monkeypatch.setenv("LT_SHADOW_FRAMES", "1")
        assert np.array_equal(out, render(fresh, wall, 96, 64, count=4)[0])
    finally:
        fresh.close()


def test_several_frames_match_the_oracle(renderer, capfd, wall):
    W, H, first, count = 24, 16, 2, 3
    out = np.full((H, W, 3), np.nan, dtype=np.float32)
    groups(capfd)
    renderer.render(oracle_props("examples/accumulator/resources/kernels/accumulator.cl", (W, H, 3), out, wall, pCamera=CAM,
                                 frameFirst=first, frameCount=count, accumulate=True))
    assert (2, 1, count) in groups(capfd)
    acc = np.zeros((H, W, 3), dtype=np.float32)
    for i, f in enumerate(range(first, first + count)):
        po.accumulate(acc, po.render(wall, sc.camera_with_frame(CAM, f), W, H, po.ACCUMULATOR), i)
    assert np.array_equal(out, acc)
