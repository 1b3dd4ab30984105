"""GPU (-m gpu): the global-illumination programs over caller-supplied rays (lt_hip_shade_paths / lt_hip_shade_paths_device,
lens_trace_amd/csrc/lt_paths.hip).  Every comparison is bit for bit, no case excluded.

1. a camera's rays give its render: both programs, both kernel modes, frame_first 0 and 7, 1 and 3 frames, gi_max_depth 1, 4 and 0
   (= 16); in the portable flavour at every yaw against `render` and against the CPU oracle, in the default and strict flavours at
   yaw 0 against `render` and, for turned cameras, with rays the GPU rendered itself (tests/user_kernels/camera_rays.hip); `prim`
   is trace_rays';
2. twelve cameras in one shuffled batch: every ray gets what its own camera's render gives it;
3. every form of the bounce stages on the Cornell batch against the oracle: the LDS scene, the five-launch form, the one-kernel
   stage, the caller's splits (LT_RETREE=0); and a scene whose boxes do not nest -- it gets no own tree, its camera rays walk the
   caller's tree per lane -- against its render;
4. synthetic scenes at 64 x 48 from their own cameras against the oracle;
5. sets and edges: batch sizes, LT_PATHS_SLOTS that splits the rays and then one ray's frames (never a frame's 25 samples),
   LT_TRACE_REFILL 1 and 64, the device entry point on a side stream with guard words behind the output;
6. rays of every kind (axis-parallel, signed zeros, non-finite, huge): prim is trace_rays', misses are {0, 0, 0, -1}, light hits
   are 1, the caller's splits give the same bytes;
7. the contract: errors leave the output untouched, the other programs are refused with a text that names lt_hip_shade_rays, a
   call between two renders or two shade_rays calls changes neither, a set_scene behind an enqueued call changes nothing, stats()
   reports the rays and the launches."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import (KERNEL_MODE_LINEAR, KERNEL_MODE_TILE, RendererHIP, RenderPropertiesHIP, make_rays,
                                     make_shade_rays, reference_camera_rays)
from oracle import pyoracle as po
from tests import shade_paths as P
from tests import shade_rays as F
from tests.test_gpu_trace_rays import random_rays

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CAMERA_RAYS = os.path.join(HERE, "user_kernels", "camera_rays.hip")
FLAVOURS = {"default": {}, "strict": {"strict_math": True}, "portable": {"portable_math": True}}
PROPS = {"default": {}, "strict": {"strictMath": True}, "portable": {"portableMath": True}}
PROGRAM_IDS = {"global_illumination": C.PROGRAM_GLOBAL_ILLUMINATION, "global_illumination25": C.PROGRAM_GLOBAL_ILLUMINATION_25}
MODES = (KERNEL_MODE_LINEAR, KERNEL_MODE_TILE)
FRAMES = ((0, 1), (7, 1), (0, 3), (7, 3))   # (frame_first, frame_count)


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render(r, s, cam, W, H, program, mode=KERNEL_MODE_LINEAR, frame_first=0, frame_count=1, flavour="portable", depth=0):
    """(W * H, 3): frames frame_first .. + frame_count - 1 of the render path, folded by its running mean from n = 0"""
    out = np.zeros((H, W, 3), dtype=np.float32)
    path = program if program.endswith(".hip") else program + ".cl"
    r.render(RenderPropertiesHIP(path, (W, H, 3), out, s, pCamera=cam, kernelMode=mode, frameFirst=frame_first, frameCount=frame_count,
                                 accumulate=frame_count > 1, giMaxDepth=depth, **PROPS[flavour]))
    return out.reshape(-1, 3)


def gpu_camera_rays(r, s, cam, W, H, flavour):
    """the render kernel's own camera rays of this flavour, as lt_hip_shade_ray records: a user program renders them"""
    o = render(r, s, cam, W, H, CAMERA_RAYS, KERNEL_MODE_TILE, 0, 1, flavour)
    d = render(r, s, cam, W, H, CAMERA_RAYS, KERNEL_MODE_TILE, 1, 1, flavour)
    f = render(r, s, cam, W, H, CAMERA_RAYS, KERNEL_MODE_TILE, 2, 1, flavour)
    assert (f[:, 2] == 2.0).all()   # origin.w + direction.w of camera_ray: 2 + 0
    return make_shade_rays(o, d, f[:, 0], f[:, 1])


def same(got, want, what):
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def check_against_render(r, s, rays, cam, W, H, program, flavour, modes=MODES, frames=FRAMES, depths=P.DEPTHS):
    for depth in depths:
        for mode in modes:
            for ff, fc in frames:
                want = render(r, s, cam, W, H, program, mode, ff, fc, flavour, depth)
                got = r.shade_paths(rays, program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc, kernel_mode=mode,
                                    **FLAVOURS[flavour])
                same(got["rgb"], want, (program, flavour, depth, mode, ff, fc))
                yield depth, mode, ff, fc, got


# ------------------------------------------------------------------------------------------------ 1: a camera's rays give its render
@pytest.mark.parametrize("yaw,dist", F.CAMERAS)
@pytest.mark.parametrize("program", list(PROGRAM_IDS))
def test_portable_rays_of_a_camera_give_its_render_and_the_oracles(renderer, program, yaw, dist):
    s = F.scene(P.SCENE)
    for W, H in F.SIZES:
        rays = F.camera_batch(yaw, dist, W, H)
        hits = None
        for depth, mode, ff, fc, got in check_against_render(renderer, s, rays, F.camera(yaw, dist), W, H, program, "portable"):
            same(got["rgb"], P.oracle_fold(yaw, dist, W, H, program, mode, ff, fc, depth), (program, yaw, W, H, depth, mode, ff, fc, "oracle"))
            if hits is None:
                hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], portable_math=True)
                assert 4 * (hits["prim"] >= 0).sum() >= len(rays)
            assert np.array_equal(got["prim"], hits["prim"])


@pytest.mark.parametrize("flavour", ["default", "strict"])
@pytest.mark.parametrize("program", list(PROGRAM_IDS))
def test_default_and_strict_rays_at_yaw_0_give_the_render(renderer, program, flavour):
    s = F.scene(P.SCENE)
    yaw, dist = F.CAMERAS[0]
    W, H = F.SIZES[0]   # powers of two: x / W is exact in every flavour, and at yaw 0 the rotation multiplies by 1 and 0
    assert yaw == 0.0 and (W, H) == (32, 16)
    rays = F.camera_batch(yaw, dist, W, H)
    assert np.array_equal(bits(rays), bits(gpu_camera_rays(renderer, s, F.camera(yaw, dist), W, H, flavour)))
    hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], **FLAVOURS[flavour])
    for _, _, _, _, got in check_against_render(renderer, s, rays, F.camera(yaw, dist), W, H, program, flavour):
        assert np.array_equal(got["prim"], hits["prim"])


@pytest.mark.parametrize("flavour", ["default", "strict"])
@pytest.mark.parametrize("yaw,dist", F.CAMERAS[1:])
def test_turned_cameras_in_the_default_and_strict_flavours_with_the_kernels_own_rays(renderer, yaw, dist, flavour):
    W, H = F.SIZES[1]
    s = F.scene(P.SCENE)
    cam = F.camera(yaw, dist)
    rays = gpu_camera_rays(renderer, s, cam, W, H, flavour)
    for program in PROGRAM_IDS:
        hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], **FLAVOURS[flavour])
        assert 4 * (hits["prim"] >= 0).sum() >= len(rays)
        for _, _, _, _, got in check_against_render(renderer, s, rays, cam, W, H, program, flavour, frames=((0, 1), (7, 3))):
            assert np.array_equal(got["prim"], hits["prim"])


# ------------------------------------------------------------------------------------------------ 2: many cameras, one shuffled batch
RING_CASES = (("global_illumination", 0, 3, 0), ("global_illumination25", 7, 3, 4), ("global_illumination25", 0, 1, 0))   # program, ff, fc, depth
_ring = {}


def ring_expected(r, program, ff, fc, depth, flavour, mode=KERNEL_MODE_LINEAR):
    """(rays, rgb): test 1's route for each of the twelve cameras, in ring_batch's order"""
    key = (program, ff, fc, depth, flavour, mode)
    if key not in _ring:
        W, H = F.RING_SIZE
        s = F.scene(P.SCENE)
        _, cam, pix = F.ring_batch()
        per_rays, per_rgb = [], []
        for yaw, dist in F.RING:
            c = F.camera(yaw, dist)
            per_rays.append(F.camera_batch(yaw, dist, W, H) if flavour == "portable" else gpu_camera_rays(r, s, c, W, H, flavour))
            per_rgb.append(render(r, s, c, W, H, program, mode, ff, fc, flavour, depth))
        _ring[key] = (np.ascontiguousarray(np.stack(per_rays)[cam, pix]), np.ascontiguousarray(np.stack(per_rgb)[cam, pix]))
    return _ring[key]


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("program,ff,fc,depth", RING_CASES)
def test_twelve_cameras_in_one_shuffled_batch(renderer, program, ff, fc, depth, flavour):
    rays, want = ring_expected(renderer, program, ff, fc, depth, flavour)
    if flavour == "portable":
        assert np.array_equal(bits(rays), bits(F.ring_batch()[0]))
        assert np.array_equal(bits(want), bits(P.ring_oracle(program, po.MODE_LINEAR, ff, fc, depth)))
    renderer.set_scene(F.scene(P.SCENE))
    got = renderer.shade_paths(rays, program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc, **FLAVOURS[flavour])
    same(got["rgb"], want, (program, ff, fc, depth, flavour))
    hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], **FLAVOURS[flavour])
    assert np.array_equal(got["prim"], hits["prim"])


# ------------------------------------------------------------------------------------------------ 3: every form of the bounce stages
STAGE_FORMS = {"lds_scene": {}, "five_launches": {"LT_GI_LDS_SCENE": "0"}, "one_kernel": {"LT_GI_LDS_SCENE": "0", "LT_GI_TRACE": "0"},
               "callers_splits": {"LT_RETREE": "0"}}
LAUNCHES = {"lds_scene": 2 + 1 + 16 + 1, "five_launches": 2 + 1 + 16 * 5 + 1, "one_kernel": 2 + 1 + 16 + 1, "callers_splits": 2 + 1 + 16 + 1}


@pytest.mark.parametrize("form", list(STAGE_FORMS))
def test_every_stage_form_on_the_cornell_batch_against_the_oracle(monkeypatch, form):
    for k, v in STAGE_FORMS[form].items():
        monkeypatch.setenv(k, v)
    r = RendererHIP(0)
    try:
        r.set_scene(F.scene(P.SCENE))
        rays = F.ring_batch()[0]
        for program, ff, fc, depth in RING_CASES:
            for mode in MODES:
                got = r.shade_paths(rays, program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc, kernel_mode=mode,
                                    portable_math=True)
                same(got["rgb"], P.ring_oracle(program, mode, ff, fc, depth), (form, program, mode))
        st = r.stats()
        assert st["own_tree_height"] > 0 and st["kernel_launches"] == LAUNCHES[form], st
    finally:
        r.close()


def no_own_tree_scene():
    from lens_trace_amd import synth
    s = synth.blob_in_box(3).validate()
    nodes = s.node_view
    leaves = np.flatnonzero(nodes["primitiveCount"] != 0)
    for k in leaves[::7]:                     # leaves that poke out of their ancestors: legal for the reference's traversal
        nodes["boundsMax"][k] += np.float32(0.75)
        nodes["boundsMin"][k] -= np.float32(0.25)
    return s


def test_a_scene_without_an_own_tree_walks_its_camera_rays_over_the_callers_tree(renderer):
    s = no_own_tree_scene()
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    lo, hi = s.node_view["boundsMin"][0], s.node_view["boundsMax"][0]
    cam = sc.camera_bytes(float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2), float(lo[2] - 40.0), 0.0)
    W, H = 37, 29
    rays = make_shade_rays(*reference_camera_rays(cam, W, H))
    hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=C.PROGRAM_GLOBAL_ILLUMINATION, portable_math=True)
    assert 4 * (hits["prim"] >= 0).sum() >= len(rays)
    for program in PROGRAM_IDS:
        for _, _, _, _, got in check_against_render(renderer, s, rays, cam, W, H, program, "portable", frames=((0, 1), (7, 3)), depths=(4,)):
            assert np.array_equal(got["prim"], hits["prim"])
    assert renderer.stats()["kernel_launches"] == 1 + 1 + 4 + 1   # the camera walk, the primary stage, four one-kernel stages, the resolve


# ------------------------------------------------------------------------------------------------ 4: synthetic scenes
@pytest.mark.parametrize("kind", ["wall", "soup", "blob"])
def test_synthetic_scenes_from_their_own_cameras_against_the_oracle(renderer, kind):
    s = P.synth_scene(kind)
    W, H = P.SYNTH_SIZE
    rays = make_shade_rays(*reference_camera_rays(s.camera, W, H))
    renderer.set_scene(s)
    for program, ff, fc in (("global_illumination", 0, 2), ("global_illumination25", 3, 1)):
        got = renderer.shade_paths(rays, program=PROGRAM_IDS[program], gi_max_depth=4, frame_first=ff, frame_count=fc, portable_math=True)
        same(got["rgb"], P.synth_oracle(kind, program, po.MODE_LINEAR, ff, fc, 4), (kind, program))
        assert (got["rgb"] != 0).any(axis=1).mean() > 0.25
    assert renderer.stats()["own_tree_height"] > 0


# ------------------------------------------------------------------------------------------------ 5: sets and edges
SHAPES = (1, 63, 64, 65, 127, 513, 3072)
SET_CASES = (("global_illumination", 0, 3, 0), ("global_illumination25", 7, 3, 4))


@pytest.mark.parametrize("program,ff,fc,depth", SET_CASES)
def test_batch_shapes(renderer, program, ff, fc, depth):
    rays, want = ring_expected(renderer, program, ff, fc, depth, "portable")
    renderer.set_scene(F.scene(P.SCENE))
    for n in SHAPES:
        got = renderer.shade_paths(rays[:n], program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc, portable_math=True)
        assert got.shape == (n,)
        same(got["rgb"], want[:n], (program, n))


# (slots per set; the single-sample program's 3 frames of 3072 rays are 9216 slots, the 25-sample program's 230 400)
@pytest.mark.parametrize("form", ["lds_scene", "five_launches"])
@pytest.mark.parametrize("program,ff,fc,depth,caps", [
    ("global_illumination", 0, 3, 0, (9215, 3 * 1000, 200, 3, 2, 1)),            # ranges of rays ... and, below 3, of one ray's frames
    ("global_illumination25", 7, 3, 4, (230399, 75 * 100, 75, 74, 50, 25, 1)),   # below 75: one ray's frames; 25 and below: one frame per set
])
def test_sets_of_every_size_give_the_unsplit_result(renderer, monkeypatch, program, ff, fc, depth, caps, form):
    for k, v in STAGE_FORMS[form].items():
        monkeypatch.setenv(k, v)
    rays, want = ring_expected(renderer, program, ff, fc, depth, "portable")
    renderer.set_scene(F.scene(P.SCENE))
    per_ray = fc * (25 if program.endswith("25") else 1)
    for cap in caps:
        n = len(rays) if cap >= 200 * per_ray // 3 else 96 if cap >= per_ray else 7   # (a set per ray and frame: a few rays will do)
        monkeypatch.setenv("LT_PATHS_SLOTS", str(cap))
        got = renderer.shade_paths(rays[:n], program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc, portable_math=True)
        same(got["rgb"], want[:n], (program, cap, n))
        per_frame = 25 if program.endswith("25") else 1
        frames_per_set = fc if cap >= per_ray else max(1, cap // per_frame)
        rays_per_set = min(n, max(1, max(cap, per_frame) // (frames_per_set * per_frame)))
        sets = -(-n // rays_per_set) * -(-fc // frames_per_set)
        stages = depth if depth else 16
        per_set = 2 + stages * (5 if form == "five_launches" else 1)
        assert renderer.stats()["kernel_launches"] == -(-n // rays_per_set) * 2 + sets * per_set, (cap, n, sets)
        assert sets > 1


@pytest.mark.parametrize("refill", ["1", "64"])
def test_trace_refill(renderer, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", refill)
    for form in ("lds_scene", "five_launches"):
        for k, v in STAGE_FORMS[form].items():
            monkeypatch.setenv(k, v)
        for program, ff, fc, depth in SET_CASES:
            rays, want = ring_expected(renderer, program, ff, fc, depth, "portable")
            renderer.set_scene(F.scene(P.SCENE))
            for n in (65, len(rays)):
                got = renderer.shade_paths(rays[:n], program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc, portable_math=True)
                same(got["rgb"], want[:n], (program, refill, form, n))


def test_device_entry_point_on_a_side_stream(renderer):
    import torch
    program, ff, fc, depth = RING_CASES[0]
    rays, want = ring_expected(renderer, program, ff, fc, depth, "default")
    renderer.set_scene(F.scene(P.SCENE))
    side = torch.cuda.Stream()
    for n in (0, 1, 65, 513, 3072):
        host = renderer.shade_paths(rays[:n], program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc)
        rt = torch.from_numpy(np.ascontiguousarray(rays[:n])).cuda()
        with torch.cuda.stream(side):
            got = renderer.shade_paths(rt, program=PROGRAM_IDS[program], gi_max_depth=depth, frame_first=ff, frame_count=fc)
        side.synchronize()
        assert got.shape == (n, 4) and got.dtype == torch.float32
        assert np.array_equal(bits(got.cpu().numpy()).reshape(-1), bits(host.view(np.uint32)).reshape(-1)), n
        same(host["rgb"], want[:n], n)
        # nothing past 16 n bytes: guard words behind the output keep their value
        buf = torch.full(((n + 70) * 4,), -7, dtype=torch.int32, device="cuda")
        d = C.PathsDesc(ctypes.sizeof(C.PathsDesc), PROGRAM_IDS[program], C.KERNEL_MODE_LINEAR, 0, ff, fc, depth, 0)
        assert renderer._L.lt_hip_shade_paths_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(rt.data_ptr() if n else 0), n,
                                                     ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4, ctypes.c_void_p(side.cuda_stream)) == 0
        side.synchronize()
        assert (buf[n * 4:].cpu().numpy() == -7).all(), n
        assert np.array_equal(buf[:n * 4].cpu().numpy().view(np.uint32), host.view(np.uint32).reshape(-1))


# ------------------------------------------------------------------------------------------------ 6: odd rays
def test_rays_of_every_kind(monkeypatch):
    s = F.scene(P.SCENE)
    rng = np.random.default_rng(21)
    q = random_rays(s, rng, 3000)
    rays = make_shade_rays(q[:, 0:3], q[:, 4:7], rng.uniform(-0.5, 0.5, len(q)), rng.uniform(-0.5, 0.5, len(q)))
    assert not np.isfinite(rays).all() and (np.abs(rays[np.isfinite(rays)]) > 2.0 ** 40).any() and (rays[:, 4:7] == 0).any()
    lights = F.light_prims(P.SCENE)
    outputs = {}
    for retree in (None, "0"):
        if retree is not None:
            monkeypatch.setenv("LT_RETREE", retree)
        r = RendererHIP(0)
        try:
            r.set_scene(s)
            for flavour, kw in FLAVOURS.items():
                h = r.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=C.PROGRAM_GLOBAL_ILLUMINATION, **kw)
                hit, lit = h["prim"] >= 0, np.isin(h["prim"], lights)
                assert hit.any() and not hit.all() and lit.any()
                for program, fc, mode in (("global_illumination", 2, KERNEL_MODE_TILE), ("global_illumination25", 1, KERNEL_MODE_LINEAR)):
                    got = r.shade_paths(rays, program=PROGRAM_IDS[program], gi_max_depth=4, frame_first=3, frame_count=fc, kernel_mode=mode, **kw)
                    assert np.array_equal(got["prim"], h["prim"]), (flavour, program)
                    assert (bits(got["rgb"][~hit]) == 0).all() and (got["rgb"][lit] == 1.0).all(), (flavour, program)
                    key = (flavour, program)
                    if key in outputs:
                        assert np.array_equal(got.view(np.uint32), outputs[key].view(np.uint32)), key
                    outputs[key] = got
            assert r.stats()["own_tree_height"] > 0
        finally:
            r.close()


# ------------------------------------------------------------------------------------------------ 7: the contract
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        rays = make_shade_rays(np.zeros((4, 3)), np.ones((4, 3)), 0.0, 0.0)
        out = np.full(16, 0x5a5a5a5a, dtype=np.uint32)
        R, O = rays.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

        def desc(program=C.PROGRAM_GLOBAL_ILLUMINATION, mode=C.KERNEL_MODE_LINEAR, flags=0, first=0, count=1, depth=0, reserved=0,
                 size=ctypes.sizeof(C.PathsDesc)):
            return ctypes.byref(C.PathsDesc(size, program, mode, flags, first, count, depth, reserved))

        assert L.lt_hip_shade_paths(r._ctx, desc(), R, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        r.set_scene(F.scene(P.SCENE))
        user = r.resolve_program(CAMERA_RAYS)
        assert user >= 1000
        others = (C.PROGRAM_BASIC, C.PROGRAM_BASIC_LIGHTING, C.PROGRAM_ACCUMULATOR, C.PROGRAM_CUSTOM_OPENCL)
        cases = [
            (None, R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), None, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 4, None, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 2 ** 32, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(size=28), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_PORTABLE_MATH), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_STATS), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_NO_WALK_TIMING), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=0x200), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(mode=2), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(mode=-1), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(count=0), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(depth=-1), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(depth=65), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(reserved=1), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
        ] + [(desc(program=p), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT) for p in others + (user,)] + [
            (desc(program=6), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(program=-1), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(program=user + 1), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(), R, 4, O, 4 * 16 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
        ]
        for i, (d, rp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_shade_paths(r._ctx, d, rp, n, op, nb) == want, i
            assert (out == 0x5a5a5a5a).all(), i
        for program in others + (user,):
            with pytest.raises(C.LensTraceError, match="lt_hip_shade_rays"):
                r.shade_paths(rays, program=program)
        assert L.lt_hip_shade_paths(r._ctx, desc(), R, 0, O, 0) == 0 and (out == 0x5a5a5a5a).all()
        assert L.lt_hip_shade_paths(r._ctx, desc(), None, 0, None, 0) == 0
        assert L.lt_hip_shade_paths(r._ctx, desc(depth=64, flags=C.TRACE_FLAG_COHERENT), R, 4, O, out.nbytes) == 0 and (out != 0x5a5a5a5a).any()
        # device entry point: the same checks, and 16-byte alignment
        rt = torch.from_numpy(rays).cuda()
        buf = torch.full((32,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        for rp, op in ((rt.data_ptr() + 4, buf.data_ptr()), (rt.data_ptr(), buf.data_ptr() + 8)):
            assert L.lt_hip_shade_paths_device(r._ctx, desc(), ctypes.c_void_p(rp), 3, ctypes.c_void_p(op), 64, None) == C.LT_ERR_INVALID_ARGUMENT
        assert L.lt_hip_shade_paths_device(r._ctx, desc(count=0), ctypes.c_void_p(rt.data_ptr()), 4, ctypes.c_void_p(buf.data_ptr()), 64, None) == C.LT_ERR_INVALID_ARGUMENT
        assert L.lt_hip_shade_paths_device(r._ctx, desc(), ctypes.c_void_p(rt.data_ptr()), 4, ctypes.c_void_p(buf.data_ptr()), 63, None) == C.LT_ERR_BUFFER_TOO_SMALL
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x5a5a5a5a).all()
    finally:
        r.close()


def test_calls_interleave_with_renders_shade_rays_and_scene_changes():
    import torch
    s = F.scene(P.SCENE)
    other = F.scene("cornell_box_lens_O0")
    cam = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
    W, H = 96, 64

    def frame(r):
        out = np.empty((H, W, 3), dtype=np.float32)
        r.render(RenderPropertiesHIP("global_illumination.cl", (W, H, 3), out, s, pCamera=cam, frameCount=4, accumulate=True))
        return out, r.stats()

    r1, r2 = RendererHIP(0), RendererHIP(0)
    try:
        a1, _ = frame(r1)
        b1, t1 = frame(r1)
        a2, _ = frame(r2)
        rays, want = ring_expected(r2, "global_illumination", 0, 3, 0, "default")
        r2.set_scene(s)
        got = r2.shade_paths(rays, frame_count=3)
        same(got["rgb"], want, "between two renders")
        st = r2.stats()
        assert st["rays"] == len(rays) and st["kernel_launches"] > 1 and st["kernel_ms"] > 0 and st["shadow_rays"] == 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0
        b2, t2 = frame(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):   # the render's statistics, not the call's
            assert t2[k] == t1[k], k
        # ... and between two shade_rays calls
        c1 = r2.shade_rays(rays, frame_count=2)
        r2.shade_paths(rays[:700], program=C.PROGRAM_GLOBAL_ILLUMINATION_25, gi_max_depth=2)
        c2 = r2.shade_rays(rays, frame_count=2)
        assert np.array_equal(c1.view(np.uint32), c2.view(np.uint32)) and np.array_equal(c1.view(np.uint32), r1_shade(r1, s, rays).view(np.uint32))
        # set_scene of another scene right behind an enqueued device call: the call keeps the old scene's results
        big = np.ascontiguousarray(rays[np.resize(np.arange(len(rays)), 100_000)])
        want = r2.shade_paths(big, frame_count=2)
        rt = torch.from_numpy(big).cuda()
        stream = torch.cuda.Stream()
        got = r2.shade_paths(rt, frame_count=2, stream=stream)
        r2.set_scene(other)
        stream.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()).reshape(-1), bits(want.view(np.uint32)).reshape(-1))
        changed = r2.shade_paths(big, frame_count=2)
        assert not np.array_equal(bits(changed["rgb"]), bits(want["rgb"]))
    finally:
        r1.close()
        r2.close()


def r1_shade(r, s, rays):
    """shade_rays on a context that never ran shade_paths"""
    r.set_scene(s)
    return r.shade_rays(rays, frame_count=2)
