"""GPU tests (-m gpu): every direction-sign octant of the three packet-walk families -- the closest-hit camera walk, the one-frame
any-hit shadow walk and the two-frame shadow walk (lt_walk_asm.hpp: one instance per octant each, chosen by the `switch` of
traverse_camera, traverse and traverse_shadow2 in lt_device.hpp) -- against the reference's own kernels and the CPU oracle.

The scenes and cameras come from tests/octant_scenes.py, whose construction tests/test_octant_scenes_cpu.py checks: a camera at
yaw 0 walks octants 0-3, at yaw pi octants 4-7; octant_scene(k) puts its light beyond the geometry on every axis, so that every
shadow ray has octant k's signs.  Comparisons, as in test_gpu_reference_kernels.py: the default flavour against the reference's
kernels built with NULL options, strictMath against the strict build -- every float the same bits, NaN where the reference has
NaN -- and the portable flavour against the oracle, float for float.  The two-frame walk runs in images whose sides are not
multiples of 8, one smaller than a square: lanes masked off by the image edge."""
import math
import os
import re

import numpy as np
import pytest

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, RenderPropertiesHIP
from oracle import pyoracle as po
from oracle import ref_gpu
from tests import octant_scenes as oc
from tests.conftest import fuzz_scene, oracle_props
from tests.test_gpu_own_hierarchy import doubled_scene

pytestmark = pytest.mark.gpu

PATHS = {
    "basic": "resources/kernels/opencl/basic.cl",
    "basic_lighting": "resources/kernels/opencl/basic_lighting.cl",
    "accumulator": "examples/accumulator/resources/kernels/accumulator.cl",
    "global_illumination": "examples/global_illumination/resources/kernels/global_illumination.cl",
    "custom_opencl": "examples/custom_kernel/resources/kernels/custom_opencl.cl",
}
YAWS = (0.0, math.pi, 1.2, -2.4)
# program, kernel mode, W, H: every program of the camera walk, both kernel modes, ragged sizes and one smaller than a square
CAMERA_CASES = [("basic", 0, 37, 29), ("basic", 1, 64, 48), ("custom_opencl", 0, 5, 3), ("custom_opencl", 1, 37, 29),
                ("accumulator", 0, 64, 48), ("accumulator", 1, 37, 29), ("global_illumination", 0, 37, 29),
                ("global_illumination", 1, 21, 13), ("basic_lighting", 0, 21, 13), ("basic_lighting", 1, 13, 11)]
BUILDS = ("default", "strict")


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no calibration launches: each test forces the walk it means
    monkeypatch.setenv("LT_DEBUG_SHADOW_FRAMES", "1")


_scenes = {}


def scene(kind, k):
    """("octant", k): octant_scene(k); ("doubled", k): every triangle twice with different materials (bit-equal hits)."""
    if (kind, k) not in _scenes:
        _scenes[kind, k] = oc.octant_scene(k, seed=k) if kind == "octant" else doubled_scene(100 + k, lens=k % 2 == 1)
    return _scenes[kind, k]


def camera(kind, s, yaw, frame):
    return oc.camera_for(yaw, frame=frame) if kind == "octant" else oc.camera_for(yaw, oc.box_of(s), frame=frame)


def assert_same(got, want, what):
    """Every float the same bits; NaN (a degenerate triangle's 0 / 0) where the other has NaN."""
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), got.size)


def hip(renderer, s, prog, W, H, cam, mode=0, build="default", start=None, **kw):
    out = np.full((H, W, 3), np.nan, dtype=np.float32) if start is None else start.copy()
    props = oracle_props if build == "portable" else RenderPropertiesHIP
    renderer.render(props(PATHS[prog], (W, H, 3), out, s, pCamera=cam, kernelMode=mode, strictMath=(build == "strict"), **kw))
    return out


def fold(start, frames, base):
    """Frames folded into the caller's running mean of `base` frames in float32 (accumulator.frag:10-20): frame k with
    n = base + k, the first one overwriting where n == 0 (the `if (frameCount > 0)` guard)."""
    acc = start.copy()
    for k, c in enumerate(frames):
        n = base + k
        acc = c.copy() if n == 0 else ((c + acc * np.float32(n)) / np.float32(n + 1)).astype(np.float32)
    return acc


def oracle_fold(s, cam, W, H, first, count, base, start):
    acc = start.copy()
    for k in range(count):
        po.accumulate(acc, po.render(s, sc.camera_with_frame(cam, first + k), W, H, po.ACCUMULATOR), base + k)
    return acc


WAVES = []   # (walk, together, apart) of every launch with frame groups seen so far


def groups(capfd):
    """(frames per work item, shadow walk, frames of the launch) of every render launch since the last look (LT_DEBUG_SHADOW_FRAMES)."""
    got = re.findall(r"shadow-ray frame groups: (\d+) \(walk (\d+), (\d+) frames\)(?:: (\d+) waves walked both frames together, (\d+) apart)?",
                     capfd.readouterr().err)
    WAVES.extend((int(m[1]), int(m[3]), int(m[4])) for m in got if m[3])
    return [tuple(map(int, m[:3])) for m in got]


def need_reference():
    if not ref_gpu.available():
        pytest.skip("oracle/_ref/*.co not built (needs the reference sources at build time)")


# ---------------------------------------------------------------------------------------------------------------------------
# Camera rays: the closest-hit walk in all eight octants (yaw 0: 0-3, yaw pi: 4-7), its rank8 ties on the doubled scene.

def test_the_parametrisation_covers_every_camera_octant():
    got = set()
    for yaw in YAWS:
        for _, _, W, H in CAMERA_CASES:
            got |= oc.camera_octants(oc.camera_for(yaw), W, H)
            got |= oc.camera_octants(camera("doubled", scene("doubled", 0), yaw, 0), W, H)
    assert got == set(range(8))


@pytest.mark.parametrize("against", ["reference", "oracle"])
@pytest.mark.parametrize("yaw", YAWS, ids=["yaw0", "yaw-pi", "yaw1.2", "yaw-2.4"])
@pytest.mark.parametrize("kind", ["octant", "doubled"])
def test_camera_walks(renderer, monkeypatch, kind, yaw, against):
    """reference: the default and strict flavours against the reference's two builds; oracle: the portable flavour (never skips)."""
    if against == "reference":
        need_reference()
    k = YAWS.index(yaw)
    s = scene(kind, k)
    cam = camera(kind, s, yaw, frame=3 + k)
    for prog, mode, W, H in CAMERA_CASES:
        for mega in (("0", "1") if prog == "global_illumination" else ("1",)):
            monkeypatch.setenv("LT_GI_MEGAKERNEL", mega)
            what = "%s %s yaw %g m%d %dx%d LT_GI_MEGAKERNEL=%s" % (kind, prog, yaw, mode, W, H, mega)
            for build in (BUILDS if against == "reference" else ("portable",)):
                got = hip(renderer, s, prog, W, H, cam, mode, build)
                assert renderer.stats()["own_tree_height"] > 0     # the packet walks are eligible
                want = (ref_gpu.render(s, cam, W, H, prog, build, mode) if against == "reference" else
                        po.render(s, cam, W, H, po.PROGRAMS[prog], mode=mode))
                assert_same(got, want, "%s: %s vs %s" % (what, build, against))


# ---------------------------------------------------------------------------------------------------------------------------
# Shadow rays of one frame: the any-hit walk in the octant of the light's placement, every shadow walk.

@pytest.mark.parametrize("packets", ["0", "1", "2", "3"])
@pytest.mark.parametrize("octant", range(8))
def test_one_frame_shadow_walks_match_the_reference(renderer, monkeypatch, octant, packets):
    need_reference()
    monkeypatch.setenv("LT_SHADOW_PACKETS", packets)
    monkeypatch.setenv("LT_SHADOW_SPREAD", "100")     # walk 2 takes every wave as a packet (no pixel depends on it)
    s = scene("octant", octant)
    yaw = YAWS[octant % len(YAWS)]
    for W, H in ((37, 29), (64, 48)):
        cam = oc.camera_for(yaw, frame=5 + octant)
        for mode in (0, 1):
            for build in BUILDS:
                got = hip(renderer, s, "accumulator", W, H, cam, mode, build)
                assert renderer.stats()["shadow_packets"] == int(packets)
                assert_same(got, ref_gpu.render(s, cam, W, H, "accumulator", build, mode),
                            "octant %d walk %s %dx%d m%d %s" % (octant, packets, W, H, mode, build))


# ---------------------------------------------------------------------------------------------------------------------------
# Shadow rays of two frames walked together (shade_pixel2 -> traverse_shadow2 -> packet_anyhit_walk2), every octant.

@pytest.mark.parametrize("packets", ["1", "2"])
@pytest.mark.parametrize("octant", range(8))
def test_two_frame_walks_match_reference_frames_folded(renderer, monkeypatch, capfd, octant, packets):
    need_reference()
    monkeypatch.setenv("LT_SHADOW_PACKETS", packets)
    monkeypatch.setenv("LT_SHADOW_SPREAD", "100")
    s = scene("octant", octant)
    yaw = YAWS[octant % len(YAWS)]
    rng = np.random.default_rng(octant * 2 + int(packets))
    first = 2 + octant
    cam = oc.camera_for(yaw, frame=first)
    together = 0
    for W, H in ((37, 29), (5, 3)):
        start = rng.random((H, W, 3), dtype=np.float32)
        ref = {b: [ref_gpu.render(s, sc.camera_with_frame(cam, first + k), W, H, "accumulator", b) for k in range(5)] for b in BUILDS}
        for count in (2, 5):
            for base in (0, 3):
                for build in BUILDS:
                    what = "octant %d walk %s %dx%d frames %d..%d base %d %s" % (octant, packets, W, H, first, first + count - 1, base, build)
                    kw = dict(start=start, frameFirst=first, frameCount=count, accumulate=True, accumulateBase=base)
                    groups(capfd)
                    seen = len(WAVES)
                    got = hip(renderer, s, "accumulator", W, H, cam, 0, build, **kw)
                    g = groups(capfd)
                    assert g and all(x == (2, int(packets), count) for x in g), (what, g)
                    together += sum(w[1] for w in WAVES[seen:])
                    assert_same(got, fold(start, ref[build][:count], base), what + " vs reference frames folded")
                    monkeypatch.setenv("LT_SHADOW_FRAMES", "1")
                    one = hip(renderer, s, "accumulator", W, H, cam, 0, build, **kw)
                    assert all(x[0] == 1 for x in groups(capfd))
                    monkeypatch.delenv("LT_SHADOW_FRAMES")
                    assert_same(got, one, what + " vs LT_SHADOW_FRAMES=1")
                    monkeypatch.setenv("LT_CAMERA_HITS", "0")
                    walked = hip(renderer, s, "accumulator", W, H, cam, 0, build, **kw)
                    monkeypatch.delenv("LT_CAMERA_HITS")
                    assert_same(got, walked, what + " vs LT_CAMERA_HITS=0")
    if packets == "1":
        assert together > 0, "octant %d: no wave walked both frames together" % octant
    # the portable flavour against the oracle's own running mean, at one size
    W, H, count, base = 37, 29, 3, 3
    start = rng.random((H, W, 3), dtype=np.float32)
    got = hip(renderer, s, "accumulator", W, H, cam, 0, "portable", start=start, frameFirst=first, frameCount=count, accumulate=True,
              accumulateBase=base)
    assert_same(got, oracle_fold(s, cam, W, H, first, count, base, start), "octant %d walk %s portable vs oracle" % (octant, packets))


def test_waves_walk_apart_where_walk_2_refuses_the_spread(renderer, monkeypatch, capfd):
    """Walk 2 with a spread no wave passes: every group renders its frames apart, and nothing changes; across the module both
    kinds of waves occurred."""
    monkeypatch.setenv("LT_SHADOW_PACKETS", "2")
    monkeypatch.setenv("LT_SHADOW_SPREAD", "1e-9")
    s = scene("octant", 6)
    cam = oc.camera_for(0.0, frame=4)
    W, H, first, count = 37, 29, 4, 4
    groups(capfd)
    seen = len(WAVES)
    got = hip(renderer, s, "accumulator", W, H, cam, frameFirst=first, frameCount=count, accumulate=True)
    g = groups(capfd)
    assert g and all(x == (2, 2, count) for x in g), g    # (a frame handed over with a changed scene is rendered again)
    assert sum(w[2] for w in WAVES[seen:]) > 0, WAVES[seen:]
    monkeypatch.setenv("LT_SHADOW_FRAMES", "1")
    assert_same(got, hip(renderer, s, "accumulator", W, H, cam, frameFirst=first, frameCount=count, accumulate=True), "apart")
    assert sum(w[1] for w in WAVES) > 0 and sum(w[2] for w in WAVES) > 0, WAVES


# ---------------------------------------------------------------------------------------------------------------------------
# Random geometry through the multi-frame paths.

@pytest.mark.parametrize("seed", range(int(os.environ.get("LT_FUZZ_SEEDS", "16"))))
def test_fuzz_multi_frame_against_reference_frames_folded(renderer, monkeypatch, seed):
    """tests.conftest.fuzz_scene's scenes: one accumulator call of 2-6 frames (the shadow walk cycling through 0-3 by seed) and
    one global_illumination call of 2-3 frames (on these small scenes the LDS-scene wavefront pipeline), each from a random first
    frame into a random running mean, against the reference's frames folded in float32."""
    need_reference()
    s, cam, W, H, rng = fuzz_scene(seed)
    monkeypatch.setenv("LT_SHADOW_PACKETS", str(seed % 4))
    monkeypatch.setenv("LT_GI_MEGAKERNEL", "0")
    build = BUILDS[seed % 2]
    for prog, count in (("accumulator", int(rng.integers(2, 7))), ("global_illumination", int(rng.integers(2, 4)))):
        first, base = int(rng.integers(0, 60)), int(rng.integers(0, 4))
        start = rng.random((H, W, 3), dtype=np.float32)
        got = hip(renderer, s, prog, W, H, cam, 0, build, start=start, frameFirst=first, frameCount=count, accumulate=True,
                  accumulateBase=base)
        frames = [ref_gpu.render(s, sc.camera_with_frame(cam, first + k), W, H, prog, build) for k in range(count)]
        assert_same(got, fold(start, frames, base), "seed %d %s %s %dx%d frames %d..%d base %d walk %d" % (
            seed, prog, build, W, H, first, first + count - 1, base, seed % 4))
