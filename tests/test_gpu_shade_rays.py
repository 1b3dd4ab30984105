"""GPU (-m gpu): shading of caller-supplied rays (lt_hip_shade_rays / lt_hip_shade_rays_device, lens_trace_amd/csrc/lt_shade.hip).
Every comparison is bit for bit.

1. a camera's rays are its render: the four programs, both kernel modes, frame_first 0 and 7, 1 and 3 frames; in the portable
   flavour at every yaw against `render` and against the CPU oracle, in the default and strict flavours at yaw 0 against `render`
   and, for turned cameras, with rays the GPU rendered itself (tests/user_kernels/camera_rays.hip); `prim` is trace_rays';
2. twelve cameras in one shuffled batch: every ray gets what its own camera's render gives it;
3. batch sizes around the stage and the claim, LT_TRACE_REFILL 1 and 64, the device entry point on a side stream with guard
   words behind the output;
4. rays of every kind (random, axis-parallel, signed zeros, non-finite, huge) against closed forms, and a scene without an own
   tree against its render;
5. a soup whose walks leave the ten LDS stack rows, against its render;
6. the contract: errors leave the output untouched, GI and user programs are refused with a text, a call between two renders and
   a set_scene behind an enqueued call change nothing, stats() reports the rays."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import (KERNEL_MODE_LINEAR, KERNEL_MODE_TILE, RendererHIP, RenderPropertiesHIP, make_rays,
                                     make_shade_rays, reference_camera_rays)
from oracle import pyoracle as po
from tests import multihit_edges as me
from tests import query_edges as qe
from tests import shade_rays as F
from tests.test_gpu_trace_rays import random_rays

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CAMERA_RAYS = os.path.join(HERE, "user_kernels", "camera_rays.hip")
FLAVOURS = {"default": {}, "strict": {"strict_math": True}, "portable": {"portable_math": True}}
PROPS = {"default": {}, "strict": {"strictMath": True}, "portable": {"portableMath": True}}
PROGRAM_IDS = {"basic": C.PROGRAM_BASIC, "basic_lighting": C.PROGRAM_BASIC_LIGHTING, "accumulator": C.PROGRAM_ACCUMULATOR,
               "custom_opencl": C.PROGRAM_CUSTOM_OPENCL}
MODES = (KERNEL_MODE_LINEAR, KERNEL_MODE_TILE)
FRAMES = ((0, 1), (7, 1), (0, 3), (7, 3))   # (frame_first, frame_count)


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render(r, s, cam, W, H, program, mode=KERNEL_MODE_LINEAR, frame_first=0, frame_count=1, flavour="portable"):
    """(W * H, 3): frames frame_first .. + frame_count - 1 of the render path, folded by its running mean from n = 0"""
    out = np.zeros((H, W, 3), dtype=np.float32)
    path = program if program.endswith(".hip") else program + ".cl"
    r.render(RenderPropertiesHIP(path, (W, H, 3), out, s, pCamera=cam, kernelMode=mode, frameFirst=frame_first, frameCount=frame_count,
                                 accumulate=frame_count > 1, **PROPS[flavour]))
    return out.reshape(-1, 3)


def gpu_camera_rays(r, s, cam, W, H, flavour):
    """the render kernel's own camera rays of this flavour, as lt_hip_shade_ray records: a user program renders them"""
    o = render(r, s, cam, W, H, CAMERA_RAYS, KERNEL_MODE_TILE, 0, 1, flavour)
    d = render(r, s, cam, W, H, CAMERA_RAYS, KERNEL_MODE_TILE, 1, 1, flavour)
    f = render(r, s, cam, W, H, CAMERA_RAYS, KERNEL_MODE_TILE, 2, 1, flavour)
    assert (f[:, 2] == 2.0).all()   # origin.w + direction.w of camera_ray: 2 + 0
    return make_shade_rays(o, d, f[:, 0], f[:, 1])


def check_against_render(r, s, rays, cam, W, H, program, flavour, modes=MODES, frames=FRAMES):
    for mode in modes:
        for ff, fc in frames:
            want = render(r, s, cam, W, H, program, mode, ff, fc, flavour)
            got = r.shade_rays(rays, program=PROGRAM_IDS[program], frame_first=ff, frame_count=fc, kernel_mode=mode, **FLAVOURS[flavour])
            bad = np.flatnonzero((bits(got["rgb"]) != bits(want)).any(axis=1))
            assert len(bad) == 0, (program, flavour, mode, ff, fc, len(bad), bad[:5], got["rgb"][bad[:3]], want[bad[:3]])
            yield mode, ff, fc, got


# ------------------------------------------------------------------------------------------------ 1: a camera's rays are its render
@pytest.mark.parametrize("yaw,dist", F.CAMERAS)
@pytest.mark.parametrize("program", list(PROGRAM_IDS))
def test_portable_rays_of_a_camera_give_its_render_and_the_oracles(renderer, program, yaw, dist):
    name = F.scene_of(program)
    s = F.scene(name)
    for W, H in F.SIZES:
        rays = F.camera_batch(yaw, dist, W, H)
        hits = None
        for mode, ff, fc, got in check_against_render(renderer, s, rays, F.camera(yaw, dist), W, H, program, "portable"):
            want = F.oracle_fold(name, yaw, dist, W, H, program, mode, ff, fc)
            assert np.array_equal(bits(got["rgb"]), bits(want)), (program, yaw, W, H, mode, ff, fc)
            if hits is None:
                hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], portable_math=True)
                assert 4 * (hits["prim"] >= 0).sum() >= len(rays)
            assert np.array_equal(got["prim"], hits["prim"])


@pytest.mark.parametrize("flavour", ["default", "strict"])
@pytest.mark.parametrize("program", list(PROGRAM_IDS))
def test_default_and_strict_rays_at_yaw_0_give_the_render(renderer, program, flavour):
    s = F.scene(F.scene_of(program))
    yaw, dist = F.CAMERAS[0]
    W, H = F.SIZES[0]   # powers of two: x / W is exact in every flavour, and at yaw 0 the rotation multiplies by 1 and 0
    assert yaw == 0.0 and (W, H) == (32, 16)
    rays = F.camera_batch(yaw, dist, W, H)
    assert np.array_equal(bits(rays), bits(gpu_camera_rays(renderer, s, F.camera(yaw, dist), W, H, flavour)))
    hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], **FLAVOURS[flavour])
    for _, _, _, got in check_against_render(renderer, s, rays, F.camera(yaw, dist), W, H, program, flavour):
        assert np.array_equal(got["prim"], hits["prim"])


@pytest.mark.parametrize("flavour", ["default", "strict"])
@pytest.mark.parametrize("yaw,dist", F.CAMERAS[1:])
def test_turned_cameras_in_the_default_and_strict_flavours_with_the_kernels_own_rays(renderer, yaw, dist, flavour):
    W, H = F.SIZES[1]
    for program in PROGRAM_IDS:
        s = F.scene(F.scene_of(program))
        cam = F.camera(yaw, dist)
        rays = gpu_camera_rays(renderer, s, cam, W, H, flavour)
        hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], **FLAVOURS[flavour])
        assert 4 * (hits["prim"] >= 0).sum() >= len(rays)
        for _, _, _, got in check_against_render(renderer, s, rays, cam, W, H, program, flavour, frames=((0, 1), (7, 3))):
            assert np.array_equal(got["prim"], hits["prim"])


# ------------------------------------------------------------------------------------------------ 2: many cameras, one shuffled batch
RING_CASES = (("accumulator", 0, 2), ("basic_lighting", 0, 1), ("basic", 0, 1))
_ring = {}


def ring_expected(r, program, ff, fc, flavour, mode=KERNEL_MODE_LINEAR):
    """(rays, rgb): test 1's route for each of the twelve cameras, in ring_batch's order"""
    key = (program, ff, fc, flavour, mode)
    if key not in _ring:
        W, H = F.RING_SIZE
        s = F.scene(F.scene_of(program))
        _, cam, pix = F.ring_batch()
        per_rays, per_rgb = [], []
        for yaw, dist in F.RING:
            c = F.camera(yaw, dist)
            per_rays.append(F.camera_batch(yaw, dist, W, H) if flavour == "portable" else gpu_camera_rays(r, s, c, W, H, flavour))
            per_rgb.append(render(r, s, c, W, H, program, mode, ff, fc, flavour))
        _ring[key] = (np.ascontiguousarray(np.stack(per_rays)[cam, pix]), np.ascontiguousarray(np.stack(per_rgb)[cam, pix]))
    return _ring[key]


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("program,ff,fc", RING_CASES)
def test_twelve_cameras_in_one_shuffled_batch(renderer, program, ff, fc, flavour):
    rays, want = ring_expected(renderer, program, ff, fc, flavour)
    if flavour == "portable":
        assert np.array_equal(bits(rays), bits(F.ring_batch()[0]))
        assert np.array_equal(bits(want), bits(F.ring_oracle(program, po.MODE_LINEAR, ff, fc)))
    renderer.set_scene(F.scene(F.scene_of(program)))
    got = renderer.shade_rays(rays, program=PROGRAM_IDS[program], frame_first=ff, frame_count=fc, **FLAVOURS[flavour])
    bad = np.flatnonzero((bits(got["rgb"]) != bits(want)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], got["rgb"][bad[:3]], want[bad[:3]])
    hits = renderer.trace_rays(make_rays(rays[:, 0:3], rays[:, 4:7]), program=PROGRAM_IDS[program], **FLAVOURS[flavour])
    assert np.array_equal(got["prim"], hits["prim"])


# ------------------------------------------------------------------------------------------------ 3: batch shapes and refill
SHAPES = (1, 63, 64, 65, 127, 513, 4097)


@pytest.mark.parametrize("refill", [None, "1", "64"])
@pytest.mark.parametrize("program,ff,fc", RING_CASES)
def test_batch_shapes_and_refill(renderer, monkeypatch, program, ff, fc, refill):
    rays, want = ring_expected(renderer, program, ff, fc, "portable")
    renderer.set_scene(F.scene(F.scene_of(program)))
    if refill is not None:
        monkeypatch.setenv("LT_TRACE_REFILL", refill)
    for n in SHAPES:
        idx = np.resize(np.arange(len(rays)), n)
        got = renderer.shade_rays(rays[idx], program=PROGRAM_IDS[program], frame_first=ff, frame_count=fc, portable_math=True)
        assert got.shape == (n,) and np.array_equal(bits(got["rgb"]), bits(want[idx])), (n, refill)


def test_device_entry_point_on_a_side_stream(renderer):
    import torch
    program, ff, fc = RING_CASES[0]
    rays, want = ring_expected(renderer, program, ff, fc, "default")
    renderer.set_scene(F.scene(F.scene_of(program)))
    side = torch.cuda.Stream()
    for n in (0,) + SHAPES:
        idx = np.resize(np.arange(len(rays)), n)
        host = renderer.shade_rays(rays[idx], program=PROGRAM_IDS[program], frame_first=ff, frame_count=fc)
        rt = torch.from_numpy(np.ascontiguousarray(rays[idx])).cuda()
        with torch.cuda.stream(side):
            got = renderer.shade_rays(rt, program=PROGRAM_IDS[program], frame_first=ff, frame_count=fc)
        side.synchronize()
        assert got.shape == (n, 4) and got.dtype == torch.float32
        assert np.array_equal(bits(got.cpu().numpy()).reshape(-1), bits(host.view(np.uint32)).reshape(-1)), n
        assert np.array_equal(bits(host["rgb"]), bits(want[idx]))
        # nothing past 16 n bytes: guard words behind the output keep their value
        buf = torch.full(((n + 70) * 4,), -7, dtype=torch.int32, device="cuda")
        d = C.ShadeDesc(ctypes.sizeof(C.ShadeDesc), PROGRAM_IDS[program], C.KERNEL_MODE_LINEAR, 0, ff, fc)
        assert renderer._L.lt_hip_shade_rays_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(rt.data_ptr() if n else 0), n,
                                                    ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4, ctypes.c_void_p(side.cuda_stream)) == 0
        side.synchronize()
        assert (buf[n * 4:].cpu().numpy() == -7).all(), n
        assert np.array_equal(buf[:n * 4].cpu().numpy().view(np.uint32), host.view(np.uint32).reshape(-1))


# ------------------------------------------------------------------------------------------------ 4: any ray, closed forms
def closed_forms(r, s, rays, lens_free=True, need_light=True):
    lights = s.light_view[0]["primitives"][:int(s.light_view[0]["count"])]
    diffuse = s.material_view["diffuse"][s.prim_view["materialIndex"]]
    for flavour, kw in FLAVOURS.items():
        q = make_rays(rays[:, 0:3], rays[:, 4:7])
        h = r.trace_rays(q, program=C.PROGRAM_CUSTOM_OPENCL, **kw)
        hit = h["prim"] >= 0
        want = np.zeros((len(rays), 3), dtype=np.float32)
        want[hit, 0], want[hit, 1] = h["u"][hit], h["v"][hit]
        want[hit, 2] = ((1.0 - h["u"][hit].astype(np.float64)) - h["v"][hit].astype(np.float64)).astype(np.float32)
        for fc in (1, 2):
            got = r.shade_rays(rays, program=C.PROGRAM_CUSTOM_OPENCL, frame_count=fc, **kw)
            w = want if fc == 1 else ((want + want * np.float32(1)) / np.float32(2)).astype(np.float32)
            assert np.array_equal(bits(got["rgb"]), bits(w)) and np.array_equal(got["prim"], h["prim"]), (flavour, fc)
        assert hit.any() and not hit.all()
        if lens_free:
            h = r.trace_rays(q, program=C.PROGRAM_BASIC, **kw)
            want = np.where((h["prim"] >= 0)[:, None], diffuse[np.maximum(h["prim"], 0)], np.float32(0)).astype(np.float32)
            got = r.shade_rays(rays, program=C.PROGRAM_BASIC, **kw)
            assert np.array_equal(bits(got["rgb"]), bits(want)) and np.array_equal(got["prim"], h["prim"]), flavour
        h = r.trace_rays(q, program=C.PROGRAM_ACCUMULATOR, **kw)
        for mode in MODES:
            got = r.shade_rays(rays, program=C.PROGRAM_ACCUMULATOR, frame_first=3, frame_count=2, kernel_mode=mode, **kw)
            assert np.array_equal(got["prim"], h["prim"]), flavour
            lit = np.isin(h["prim"], lights)
            assert (lit.any() or not need_light) and (got["rgb"][lit] == 1.0).all() and (bits(got["rgb"][h["prim"] < 0]) == 0).all(), (flavour, mode)
        h = r.trace_rays(q, program=C.PROGRAM_BASIC_LIGHTING, **kw)
        got = r.shade_rays(rays, program=C.PROGRAM_BASIC_LIGHTING, **kw)
        assert np.array_equal(got["prim"], h["prim"]) and (bits(got["rgb"][h["prim"] < 0]) == 0).all(), flavour


def as_shade_rays(rays, rng):
    return make_shade_rays(rays[:, 0:3], rays[:, 4:7], rng.uniform(-0.5, 0.5, len(rays)), rng.uniform(-0.5, 0.5, len(rays)))


def test_rays_of_every_kind_against_closed_forms(renderer):
    s = F.scene("cornell_box_O0")
    assert (s.material_view["dissolve"] >= 1.0).all()
    renderer.set_scene(s)
    rng = np.random.default_rng(21)
    rays = as_shade_rays(random_rays(s, rng, 3000), rng)
    assert not np.isfinite(rays).all() and (np.abs(rays[np.isfinite(rays)]) > 2.0 ** 40).any() and (rays[:, 4:7] == 0).any()
    closed_forms(renderer, s, rays)
    assert renderer.stats()["own_tree_height"] > 0


def no_own_tree_scene():
    s = synth.blob_in_box(3).validate()
    nodes = s.node_view
    leaves = np.flatnonzero(nodes["primitiveCount"] != 0)
    for k in leaves[::7]:                     # leaves that poke out of their ancestors: legal for the reference's traversal
        nodes["boundsMax"][k] += np.float32(0.75)
        nodes["boundsMin"][k] -= np.float32(0.25)
    return s


def test_a_scene_without_an_own_tree_walks_the_callers_tree_in_every_phase(renderer):
    s = no_own_tree_scene()
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    rng = np.random.default_rng(22)
    closed_forms(renderer, s, as_shade_rays(random_rays(s, rng, 1000), rng), lens_free=bool((s.material_view["dissolve"] >= 1.0).all()),
                 need_light=False)
    lo, hi = s.node_view["boundsMin"][0], s.node_view["boundsMax"][0]
    cam = sc.camera_bytes(float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2), float(lo[2] - 40.0), 0.0)
    W, H = 37, 29
    rays = make_shade_rays(*reference_camera_rays(cam, W, H))
    for program in ("accumulator", "basic_lighting", "basic"):
        for _, _, _, got in check_against_render(renderer, s, rays, cam, W, H, program, "portable", frames=((0, 1), (7, 3))):
            pass
        assert 4 * (got["prim"] >= 0).sum() >= len(rays)


# ------------------------------------------------------------------------------------------------ 5: deep stacks and scale
def test_a_soup_whose_walks_leave_the_lds_stack_rows(renderer):
    """tests/multihit_edges.py's soup of 524 288 triangles; a 64 x 64 camera in a corner of it that looks along its diagonal.  Of
    its 4032 rays that walk the own tree (the others have a zero direction component), 643 need more than kTraceRows = 10 stack
    entries by stack_depths' lower bound (the deepest: 14)."""
    s = me.soup_scene()
    lo, hi = s.node_view["boundsMin"][0].astype(np.float64), s.node_view["boundsMax"][0].astype(np.float64)
    cam = sc.camera_bytes(float(lo[0] + 0.5), float((lo[1] + hi[1]) / 2), float(lo[2] + 0.5), 0.9)
    W = H = 64
    rays = make_shade_rays(*reference_camera_rays(cam, W, H))
    q = make_rays(rays[:, 0:3], rays[:, 4:7])
    deep = me.stack_depths(s, q[qe.own_ok(q)])
    assert (deep > me.TRACE_ROWS).sum() >= 64, int((deep > me.TRACE_ROWS).sum())
    for _, _, _, got in check_against_render(renderer, s, rays, cam, W, H, "accumulator", "portable", modes=(KERNEL_MODE_LINEAR,), frames=((0, 2),)):
        assert 4 * (got["prim"] >= 0).sum() >= len(rays)


# ------------------------------------------------------------------------------------------------ 6: the contract
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        rays = make_shade_rays(np.zeros((4, 3)), np.ones((4, 3)), 0.0, 0.0)
        out = np.full(16, 0x5a5a5a5a, dtype=np.uint32)
        R, O = rays.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

        def desc(program=C.PROGRAM_ACCUMULATOR, mode=C.KERNEL_MODE_LINEAR, flags=0, first=0, count=1, size=ctypes.sizeof(C.ShadeDesc)):
            return ctypes.byref(C.ShadeDesc(size, program, mode, flags, first, count))

        assert L.lt_hip_shade_rays(r._ctx, desc(), R, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        r.set_scene(F.scene("cornell_box_O0"))
        user = r.resolve_program(CAMERA_RAYS)
        assert user >= 1000
        cases = [
            (None, R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), None, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 4, None, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 2 ** 32, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(size=20), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_PORTABLE_MATH), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_STATS), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_NO_WALK_TIMING), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=0x200), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(mode=2), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(mode=-1), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(count=0), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(program=C.PROGRAM_GLOBAL_ILLUMINATION), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(program=C.PROGRAM_GLOBAL_ILLUMINATION_25), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(program=user), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(program=6), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(program=-1), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(program=user + 1), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(), R, 4, O, 4 * 16 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
        ]
        for i, (d, rp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_shade_rays(r._ctx, d, rp, n, op, nb) == want, i
            assert (out == 0x5a5a5a5a).all(), i
        for program, word in ((C.PROGRAM_GLOBAL_ILLUMINATION, "global-illumination"), (C.PROGRAM_GLOBAL_ILLUMINATION_25, "global-illumination"),
                              (user, "user programs")):
            with pytest.raises(C.LensTraceError, match=word):
                r.shade_rays(rays, program=program)
        assert L.lt_hip_shade_rays(r._ctx, desc(), R, 0, O, 0) == 0 and (out == 0x5a5a5a5a).all()
        assert L.lt_hip_shade_rays(r._ctx, desc(), None, 0, None, 0) == 0
        assert L.lt_hip_shade_rays(r._ctx, desc(flags=C.TRACE_FLAG_COHERENT), R, 4, O, out.nbytes) == 0 and (out != 0x5a5a5a5a).any()
        # device entry point: the same checks, and 16-byte alignment
        rt = torch.from_numpy(rays).cuda()
        buf = torch.full((32,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        for rp, op in ((rt.data_ptr() + 4, buf.data_ptr()), (rt.data_ptr(), buf.data_ptr() + 8)):
            assert L.lt_hip_shade_rays_device(r._ctx, desc(), ctypes.c_void_p(rp), 3, ctypes.c_void_p(op), 64, None) == C.LT_ERR_INVALID_ARGUMENT
        assert L.lt_hip_shade_rays_device(r._ctx, desc(count=0), ctypes.c_void_p(rt.data_ptr()), 4, ctypes.c_void_p(buf.data_ptr()), 64, None) == C.LT_ERR_INVALID_ARGUMENT
        assert L.lt_hip_shade_rays_device(r._ctx, desc(), ctypes.c_void_p(rt.data_ptr()), 4, ctypes.c_void_p(buf.data_ptr()), 63, None) == C.LT_ERR_BUFFER_TOO_SMALL
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x5a5a5a5a).all()
    finally:
        r.close()


def test_calls_interleave_with_renders_and_scene_changes():
    import torch
    s = F.scene("cornell_box_O0")
    other = F.scene("cornell_box_lens_O0")
    cam = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
    W, H = 96, 64

    def frame(r):
        out = np.empty((H, W, 3), dtype=np.float32)
        r.render(RenderPropertiesHIP("accumulator.cl", (W, H, 3), out, s, pCamera=cam, frameCount=4, accumulate=True))
        return out, r.stats()

    r1, r2 = RendererHIP(0), RendererHIP(0)
    try:
        a1, _ = frame(r1)
        b1, t1 = frame(r1)
        a2, _ = frame(r2)
        rays, _ = ring_expected(r2, "accumulator", 0, 2, "default")
        r2.set_scene(s)
        r2.shade_rays(rays, frame_count=2)
        st = r2.stats()
        assert st["rays"] == len(rays) and st["kernel_launches"] == 1 and st["kernel_ms"] > 0 and st["shadow_rays"] == 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0
        b2, t2 = frame(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):   # the render's statistics, not the shade call's
            assert t2[k] == t1[k], k
        # set_scene of another scene right behind an enqueued device call: the call keeps the old scene's results
        big = np.ascontiguousarray(rays[np.resize(np.arange(len(rays)), 200_000)])
        want = r2.shade_rays(big, frame_count=2)
        rt = torch.from_numpy(big).cuda()
        stream = torch.cuda.Stream()
        got = r2.shade_rays(rt, frame_count=2, stream=stream)
        r2.set_scene(other)
        stream.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()).reshape(-1), bits(want.view(np.uint32)).reshape(-1))
        changed = r2.shade_rays(big, frame_count=2)
        assert not np.array_equal(bits(changed["rgb"]), bits(want["rgb"]))
    finally:
        r1.close()
        r2.close()
