"""GPU (-m gpu): ray queries over the resident scene (lt_hip_trace_rays / lt_hip_trace_rays_device, lens_trace_amd/csrc/lt_query.hip).

* bit for bit the CPU oracle's lt_oracle_trace (the reference's intersect / intersectIgnorePrimitiveIndex, accumulator.cl:132-217)
  in the portable flavour: random, axis-parallel, signed-zero, non-finite and huge rays, rays that start on a triangle they ignore,
  tmax FLT_MAX / inf / random / 0 / negative / NaN; the three epsilon programs, closest and any hit, both kernels; on the Cornell
  box, fuzz scenes, bit-equal doubled triangles, a scene without an own tree, and the caller's splits (LT_RETREE=0);
* any hit reports what closest hit does, in every flavour;
* the default flavour is the render path's: closest hits of the camera rays equal a user program's render of its hits;
* at scale, the packet kernel and the refill kernel agree bit for bit, and a sample agrees with the oracle;
* the device entry point on a torch stream equals the host one and writes nothing past n records;
* every error leaves the output untouched; queries interleave with renders and scene changes."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import FLT_MAX, HIT_DTYPE, RendererHIP, make_rays
from oracle import pyoracle as po
from tests.conftest import GOLDEN, fuzz_scene
from tests.conftest import oracle_props as RenderPropertiesHIP
from tests.query_edges import Oracle, on_triangle, random_rays, root_box, same_hits   # noqa: F401 (other test files take them from here)
from tests.test_gpu_own_hierarchy import doubled_scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS_PROGRAMS = (C.PROGRAM_BASIC, C.PROGRAM_BASIC_LIGHTING, C.PROGRAM_ACCUMULATOR)
FLAVOURS = ({}, {"strict_math": True}, {"portable_math": True})


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


# (rays and the oracle: root_box, on_triangle, random_rays, Oracle and same_hits live in tests/query_edges.py, importable without a GPU)
def check_scene(r, s, rays, want=None, flavours_any=True):
    """Every epsilon program, both kinds, both kernels: portable = the oracle bit for bit; any == (closest prim >= 0) in every
    flavour."""
    r.set_scene(s)
    orc = Oracle(s)
    for prog in EPS_PROGRAMS:
        wh, wo = orc.trace(rays, prog)
        for coherent in (False, True):
            got = r.trace_rays(rays, program=prog, coherent=coherent, portable_math=True)
            bad = same_hits(got, wh)
            assert len(bad) == 0, (prog, coherent, bad[:5], rays[bad[:3]], got[bad[:3]], wh[bad[:3]])
            occ = r.trace_rays(rays, any_hit=True, program=prog, coherent=coherent, portable_math=True)
            assert np.array_equal(occ, wo), (prog, coherent, np.flatnonzero(occ != wo)[:5])
            if flavours_any:
                for fl in FLAVOURS[:2]:
                    h = r.trace_rays(rays, program=prog, coherent=coherent, **fl)
                    a = r.trace_rays(rays, any_hit=True, program=prog, coherent=coherent, **fl)
                    assert np.array_equal(a, (h["prim"] >= 0).astype(np.uint32)), (prog, coherent, fl)


# ------------------------------------------------------------------------------------------------------- 1, 2: oracle parity
def test_cornell_box_against_the_oracle(renderer):
    s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
    check_scene(renderer, s, random_rays(s, np.random.default_rng(1), 1500))
    assert renderer.stats()["own_tree_height"] > 0


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_scenes_against_the_oracle(renderer, seed):
    s = fuzz_scene(seed)[0]
    check_scene(renderer, s, random_rays(s, np.random.default_rng(seed), 300), flavours_any=seed % 4 == 0)


@pytest.mark.parametrize("seed", range(2))
def test_bit_equal_doubled_triangles_go_to_the_references_first_leaf(renderer, seed):
    s = doubled_scene(seed)
    rng = np.random.default_rng(50 + seed)
    rays = random_rays(s, rng, 600)
    # and rays straight at the triangles' centroids: every hit a bit-equal pair
    pv = s.prim_view
    p = rng.integers(0, s.n_prims, 256)
    c = (pv["positionA"][p] + pv["positionB"][p] + pv["positionC"][p]).astype(np.float32) / np.float32(3)
    org = np.tile(np.float32([0.5, 2.5, -30.0]), (256, 1))
    rays = np.concatenate([rays, make_rays(org, c - org)])
    check_scene(renderer, s, rays)
    h = renderer.trace_rays(rays[-256:], portable_math=True)
    assert (h["prim"] >= 0).mean() > 0.9


def test_a_scene_without_an_own_tree(renderer):
    s = synth.blob_in_box(3).validate()
    nodes = s.node_view
    leaves = np.flatnonzero(nodes["primitiveCount"] != 0)
    for k in leaves[::7]:                     # leaves that poke out of their ancestors: legal for the reference's traversal
        nodes["boundsMax"][k] += np.float32(0.75)
        nodes["boundsMin"][k] -= np.float32(0.25)
    check_scene(renderer, s, random_rays(s, np.random.default_rng(7), 800))
    assert renderer.stats()["own_tree_height"] == -1


def test_the_callers_splits(monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        s = fuzz_scene(3)[0]
        check_scene(r, s, random_rays(s, np.random.default_rng(3), 400), flavours_any=False)
        assert r.stats()["own_tree_height"] > 0
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------- 3: the render path
def wall_camera_rays(W, H, order="rows"):
    """linearKernel's camera rays (accumulator.cl:304-312) of camera_bytes(0, 2.5, -50), yaw 0, in float32 (W, H powers of two:
    x / W is exact in every flavour); order "squares": 8x8 squares, row-major inside each, squares row-major."""
    f32 = np.float32
    ys, xs = np.mgrid[0:H, 0:W]
    if order == "squares":
        ys = ys.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
        xs = xs.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    fx = xs.astype(f32) / f32(W) - f32(0.5)
    fy = ys.astype(f32) / f32(H) - f32(0.5)
    o = np.stack([f32(0.0) + fx, f32(2.5) + fy, np.full_like(fx, f32(-50.0))], axis=-1)
    d = np.stack([f32(0.0) - fx, f32(0.0) - fy, np.full_like(fx, f32(5.0))], axis=-1)
    return make_rays(o, d), xs, ys


@pytest.fixture(scope="module")
def wall():
    return synth.heightfield_wall()


def test_default_flavour_equals_the_render_path(renderer, wall):
    W, H = 512, 256
    got = np.empty((H, W, 3), dtype=np.float32)
    from lens_trace_amd.renderer import RenderPropertiesHIP as DefaultProps
    renderer.render(DefaultProps(os.path.join(HERE, "user_kernels", "hit_info.hip"), (W, H, 3), got, wall,
                                 pCamera=sc.camera_bytes(0.0, 2.5, -50.0, 0.0)))
    rays, xs, ys = wall_camera_rays(W, H)
    for coherent in (False, True):
        h = renderer.trace_rays(rays, program="accumulator.cl", coherent=coherent)
        px = got[ys, xs]
        assert np.array_equal(h["t"][h["prim"] >= 0].view(np.uint32), px[h["prim"] >= 0, 0].view(np.uint32))
        assert np.array_equal(h["prim"].astype(np.float32), px[:, 1])
        assert (h["prim"] >= 0).mean() > 0.5


# ------------------------------------------------------------------------------------------------------- 4: scale
def device_trace(r, rays_t, **kw):
    import torch
    out = r.trace_rays(rays_t, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_scale_coherent_equals_incoherent(renderer, wall):
    import torch
    renderer.set_scene(wall)
    rng = np.random.default_rng(4)
    orc = Oracle(wall)
    for order in ("squares", "rows"):
        rays, _, _ = wall_camera_rays(4096, 2048, order)
        rt = torch.from_numpy(rays).cuda()
        for any_hit in (False, True):
            a = device_trace(renderer, rt, any_hit=any_hit, portable_math=True)
            b = device_trace(renderer, rt, any_hit=any_hit, portable_math=True, coherent=True)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (order, any_hit)
        sample = rng.choice(len(rays), 5000, replace=False)
        wh, wo = orc.trace(rays[sample], C.PROGRAM_ACCUMULATOR)
        assert len(same_hits(device_trace(renderer, rt, portable_math=True)[sample], wh)) == 0
        assert np.array_equal(b[sample], wo)   # (b: the last any-hit result)
        del rt
    soup = synth.triangle_soup()
    renderer.set_scene(soup)
    lo, hi = root_box(soup)
    n = 2_000_000
    o = rng.uniform(lo, hi, (n, 3))
    rays = make_rays(o, rng.normal(0, 1, (n, 3)))
    rt = torch.from_numpy(rays).cuda()
    for any_hit in (False, True):
        a = device_trace(renderer, rt, any_hit=any_hit, portable_math=True)
        b = device_trace(renderer, rt, any_hit=any_hit, portable_math=True, coherent=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), any_hit
    sample = rng.choice(n, 5000, replace=False)
    wh, wo = Oracle(soup).trace(rays[sample], C.PROGRAM_ACCUMULATOR)
    h = device_trace(renderer, rt, portable_math=True)
    assert len(same_hits(h[sample], wh)) == 0
    assert np.array_equal(b[sample], wo)


# ------------------------------------------------------------------------------------------------------- 5: the device path
def test_device_path_equals_host_path(renderer):
    import torch
    s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
    renderer.set_scene(s)
    rng = np.random.default_rng(5)
    big = random_rays(s, rng, 1_000_003 - 256)
    side = torch.cuda.Stream()
    for n in (0, 1, 63, 65, 1_000_003):
        rays = big[:n]
        for any_hit in (False, True):
            for coherent in (False, True):
                want = renderer.trace_rays(rays, any_hit=any_hit, coherent=coherent)
                rt = torch.from_numpy(rays).cuda()
                with torch.cuda.stream(side):
                    got = renderer.trace_rays(rt, any_hit=any_hit, coherent=coherent)
                side.synchronize()
                assert got.shape == ((n,) if any_hit else (n, 4))
                assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)), (n, any_hit, coherent)
                # nothing past n records: a larger buffer full of a sentinel keeps its tail
                rec = 4 if any_hit else 16
                buf = torch.full(((n + 70) * rec // 4,), -7, dtype=torch.int32, device="cuda")
                d = C.TraceDesc(ctypes.sizeof(C.TraceDesc), C.PROGRAM_ACCUMULATOR, C.TRACE_ANY if any_hit else C.TRACE_CLOSEST,
                                C.TRACE_FLAG_COHERENT if coherent else 0)
                assert renderer._L.lt_hip_trace_rays_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(rt.data_ptr() if n else 0), n,
                                                            ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4, None) == 0
                torch.cuda.synchronize()
                tail = buf[n * rec // 4:].cpu().numpy()
                assert (tail == -7).all(), n
                assert np.array_equal(buf[:n * rec // 4].cpu().numpy().view(np.uint32), want.view(np.uint32).reshape(-1))
    renderer.trace_rays(big[:1000])
    st = renderer.stats()
    assert st["rays"] == 1000 and st["shadow_rays"] == 0 and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
    assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
    renderer.trace_rays(big[:999], any_hit=True)
    st = renderer.stats()
    assert st["rays"] == 0 and st["shadow_rays"] == 999 and st["kernel_launches"] == 1


# ------------------------------------------------------------------------------------------------------- 6: errors
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        rays = make_rays(np.zeros((4, 3)), np.ones((4, 3)))
        out = np.full(16, 0x5a5a5a5a, dtype=np.uint32)
        R, O = rays.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

        def desc(program=C.PROGRAM_ACCUMULATOR, kind=C.TRACE_CLOSEST, flags=0, size=ctypes.sizeof(C.TraceDesc)):
            return ctypes.byref(C.TraceDesc(size, program, kind, flags))

        assert L.lt_hip_trace_rays(r._ctx, desc(), R, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        cases = [
            (None, R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), None, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 4, None, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(kind=2), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(kind=-1), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 2 ** 32, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_PORTABLE_MATH), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_STATS), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_NO_WALK_TIMING), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=0x200), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(size=12), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(program=1000), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 4, O, 4 * 16 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(kind=C.TRACE_ANY), R, 4, O, 15, C.LT_ERR_BUFFER_TOO_SMALL),
        ]
        for i, (d, rp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_trace_rays(r._ctx, d, rp, n, op, nb) == want, i
            assert (out == 0x5a5a5a5a).all(), i
        assert L.lt_hip_trace_rays(r._ctx, desc(), R, 0, O, 0) == 0 and (out == 0x5a5a5a5a).all()
        assert L.lt_hip_trace_rays(r._ctx, desc(), None, 0, None, 0) == 0
        # device entry point: the same checks, and 16-byte alignment
        rt = torch.from_numpy(rays).cuda()
        buf = torch.full((32,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        for rp, op, want in ((rt.data_ptr() + 4, buf.data_ptr(), C.LT_ERR_INVALID_ARGUMENT), (rt.data_ptr(), buf.data_ptr() + 8, C.LT_ERR_INVALID_ARGUMENT)):
            assert L.lt_hip_trace_rays_device(r._ctx, desc(), ctypes.c_void_p(rp), 3, ctypes.c_void_p(op), 64, None) == want
        assert L.lt_hip_trace_rays_device(r._ctx, desc(), ctypes.c_void_p(rt.data_ptr()), 4, ctypes.c_void_p(buf.data_ptr()), 63, None) == C.LT_ERR_BUFFER_TOO_SMALL
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x5a5a5a5a).all()
        with pytest.raises(C.LensTraceError):
            r.trace_rays(rays, program=1000)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------- 7: interleaving
def test_queries_interleave_with_renders_and_scene_changes(wall):
    import torch
    s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
    cam = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
    W, H = 96, 64

    def render(r):
        out = np.empty((H, W, 3), dtype=np.float32)
        r.render(RenderPropertiesHIP("accumulator.cl", (W, H, 3), out, s, pCamera=cam, frameCount=4, accumulate=True))
        return out, r.stats()

    r1, r2 = RendererHIP(0), RendererHIP(0)
    try:
        a1, s1 = render(r1)
        b1, t1 = render(r1)
        a2, s2 = render(r2)
        rays = random_rays(s, np.random.default_rng(9), 3000)
        r2.trace_rays(rays, any_hit=True)
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # the walk verdict timed by the first render stands, and the stats are the render's, not the query's
        assert t2["shadow_packets"] == s2["shadow_packets"] and t1["shadow_packets"] == s1["shadow_packets"]
        assert t2["frames"] == 4 and t2["render_ms"] > 0
        # set_scene of another scene right after an enqueued device query: the query keeps the old scene's results
        r2.set_scene(wall)
        rays, _, _ = wall_camera_rays(2048, 1024)
        want = r2.trace_rays(rays)
        rt = torch.from_numpy(rays).cuda()
        stream = torch.cuda.Stream()
        got = r2.trace_rays(rt, stream=stream)
        r2.set_scene(s)
        stream.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1))
        assert (want["prim"] >= 0).mean() > 0.5
    finally:
        r1.close()
        r2.close()

