"""GPU (-m gpu): surface queries (lt_hip_trace_surface, lt_hip_surface_at and their device entry points,
lens_trace_amd/csrc/lt_query.hip).  Comparisons are of bytes, except that a NaN component of a position or a normal equals any
NaN (tests/surface.py, same: rays at the magnitude limits give hits whose u and v are NaN, and which NaN an operation on two
NaNs returns is the processor's choice).

1. edge batches: every batch of tests/query_edges.py's families and rays onto the lights, the three epsilon programs, both
   kernels, the three flavours: the hit part is trace_rays', the rest tests/surface.py's `expected`; one family against the CPU
   oracle; both `flags` values occur;
2. the render path: position and normal equal what two user programs render with the render path's own bary3, in every flavour;
   the default and strict positions differ (the flavour is wired);
3. sizes 1 .. 4097 of a shuffled batch, LT_TRACE_REFILL 1 and 64, both kernels; the device entry point on a side stream writes
   nothing behind 48 n bytes and equals the host path;
4. a scene without an own tree, and the caller's splits (LT_RETREE=0);
5. surface_at over trace_hits' K = 8 records, unused slots, hand-made records; trace_surface == surface_at(trace_rays);
6. the contract: errors write nothing, calls interleave with renders and scene changes, stats() reports the call.
(That a record with prim >= n_prims gives the miss form is the same unsigned compare as prim < 0 -- lt_surface_at_kernel --
and is not provoked here.)"""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import HIT_DTYPE, SURFACE_DTYPE, RendererHIP, RenderPropertiesHIP, make_rays, make_shade_rays
from tests import multihit as mh
from tests import query_edges as qe
from tests import surface as sf
from tests.conftest import GOLDEN, fuzz_scene
from tests.test_gpu_trace_rays import Oracle, on_triangle, random_rays, root_box, same_hits, wall_camera_rays

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS_PROGRAMS = (C.PROGRAM_BASIC, C.PROGRAM_BASIC_LIGHTING, C.PROGRAM_ACCUMULATOR)
HIT_WORDS = slice(0, 4)


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, a.dtype.itemsize // 4 if a.dtype.names else a.shape[-1])


def check(r, scene, rays, flavour, note, **kw):
    """trace_surface of the rays: the hit part is trace_rays' with the same arguments, the record `expected` of those hits."""
    fl = sf.FLAVOURS[flavour]
    got = r.trace_surface(rays, **kw, **fl)
    hits = r.trace_rays(rays, **kw, **fl)
    assert got.dtype == SURFACE_DTYPE and got.shape == (len(rays),)
    assert np.array_equal(words(got)[:, HIT_WORDS], words(hits)), note
    want = sf.expected(scene, hits, flavour)
    bad = sf.same(got, want)
    assert len(bad) == 0, (note, len(bad), bad[:5], words(got)[bad[:3]], words(want)[bad[:3]])
    miss = got["prim"] < 0
    assert (words(got)[miss, 4:] == np.uint32([0, 0, 0, 0xffffffff, 0, 0, 0, 0])).all(), note
    return got


# ------------------------------------------------------------------------------------------------------------- 1: edge batches
@pytest.fixture(scope="module")
def edge():
    scene = qe.base_scene(0)
    batches = [(b.name, b.rays) for b in qe.families(scene, 0)] + [("lights", sf.light_rays(scene))]
    return scene, batches


@pytest.mark.parametrize("program", EPS_PROGRAMS)
def test_edge_batches(renderer, edge, program):
    scene, batches = edge
    renderer.set_scene(scene)
    lit = dark = 0
    for name, rays in batches:
        for coherent in (False, True):
            for flavour in sf.FLAVOURS:
                got = check(renderer, scene, rays, flavour, (name, program, coherent, flavour), program=program, coherent=coherent)
        hit = got["prim"] >= 0
        lit += int((got["flags"][hit] == C.SURFACE_LIGHT).sum())
        dark += int((got["flags"][hit] == 0).sum())
        assert set(np.unique(got["flags"])) <= {0, C.SURFACE_LIGHT}
    assert lit >= 32 and dark >= 32, (lit, dark)


def test_one_family_against_the_oracle(renderer, edge):
    scene, batches = edge
    renderer.set_scene(scene)
    name, rays = batches[0]
    want, _ = Oracle(scene).trace(rays, C.PROGRAM_ACCUMULATOR)
    for coherent in (False, True):
        got = renderer.trace_surface(rays, coherent=coherent, portable_math=True)
        hit = np.zeros(len(rays), dtype=HIT_DTYPE)
        for k in HIT_DTYPE.names:
            hit[k] = got[k]
        assert len(same_hits(hit, want)) == 0, (name, coherent)
        assert len(sf.same(got, sf.expected(scene, want, "portable"))) == 0
    assert (want["prim"] >= 0).sum() >= 32


# ------------------------------------------------------------------------------------------------------------- 2: the render path
def test_position_and_normal_are_the_render_paths(renderer):
    wall = synth.heightfield_wall(48)
    W, H = 64, 32
    rays, xs, ys = wall_camera_rays(W, H)
    cam = sc.camera_bytes(0.0, 2.5, -50.0, 0.0)
    pos = {}
    for flavour, kw in (("default", {}), ("strict", {"strictMath": True}), ("portable", {"portableMath": True})):
        img = {}
        for what in ("position", "normal"):
            img[what] = np.empty((H, W, 3), dtype=np.float32)
            renderer.render(RenderPropertiesHIP(os.path.join(HERE, "user_kernels", "surface_%s.hip" % what), (W, H, 3), img[what], wall,
                                                pCamera=cam, **kw))
        prim = renderer.shade_rays(make_shade_rays(rays[:, 0:3], rays[:, 4:7], 0.0, 0.0), **sf.FLAVOURS[flavour])["prim"]
        for coherent in (False, True):
            s = renderer.trace_surface(rays, coherent=coherent, **sf.FLAVOURS[flavour])
            for what in ("position", "normal"):
                assert np.array_equal(s[what].view(np.uint32), img[what][ys, xs].view(np.uint32)), (flavour, coherent, what)
            assert np.array_equal(s["prim"], prim), (flavour, coherent)
        assert (s["prim"] >= 0).mean() > 0.5
        pos[flavour] = s["position"][s["prim"] >= 0]
    differ = (pos["default"].view(np.uint32) != pos["strict"].view(np.uint32)).any(axis=1)
    assert differ.mean() >= 0.01, differ.mean()


# ------------------------------------------------------------------------------------------------------------- 3: sizes
@pytest.fixture(scope="module")
def shuffled(edge):
    scene, batches = edge
    rays = np.concatenate([r for _, r in batches])
    rng = np.random.default_rng(3)
    rays = rays[rng.permutation(len(rays))]
    assert len(rays) >= 4097
    return rays[:4097]


@pytest.mark.parametrize("refill", (1, 64))
def test_sizes_and_the_device_entry_point(renderer, edge, shuffled, monkeypatch, refill):
    import torch
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    scene, _ = edge
    renderer.set_scene(scene)
    side = torch.cuda.Stream()
    for n in (1, 63, 64, 65, 127, 513, 4097):
        rays = shuffled[:n]
        for coherent in (False, True):
            want = check(renderer, scene, rays, "default", (n, refill, coherent), coherent=coherent)
            rt = torch.from_numpy(rays).cuda()
            with torch.cuda.stream(side):
                got = renderer.trace_surface(rt, coherent=coherent)
            side.synchronize()
            assert got.shape == (n, 12) and got.dtype == torch.float32
            assert np.array_equal(words(got.cpu().numpy()), words(want)), (n, refill, coherent)
            buf = torch.full((12 * n + 64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            d = C.TraceDesc(ctypes.sizeof(C.TraceDesc), C.PROGRAM_ACCUMULATOR, C.TRACE_CLOSEST, C.TRACE_FLAG_COHERENT if coherent else 0)
            assert renderer._L.lt_hip_trace_surface_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(rt.data_ptr()), n,
                                                           ctypes.c_void_p(buf.data_ptr()), 48 * n, ctypes.c_void_p(side.cuda_stream)) == 0
            side.synchronize()
            out = buf.cpu().numpy()
            assert (out[12 * n:] == 0x5a5a5a5a).all(), (n, refill, coherent)
            assert np.array_equal(out[:12 * n].view(np.uint32).reshape(-1, 12), words(want)), (n, refill, coherent)


# ------------------------------------------------------------------------------------------------------------- 4: other hierarchies
def aimed_rays(s, rng, n):
    """Rays from around the scene onto points of its triangles (random_rays alone may hit next to nothing of a small scene)."""
    lo, hi = root_box(s)
    o = rng.uniform(lo - 0.5 * (hi - lo) - 1.0, hi + 0.5 * (hi - lo) + 1.0, (n, 3))
    return make_rays(o, on_triangle(s, rng.integers(0, s.n_prims, n), rng) - o)


def test_a_scene_without_an_own_tree(renderer):
    s = synth.blob_in_box(3).validate()
    nodes = s.node_view
    leaves = np.flatnonzero(nodes["primitiveCount"] != 0)
    for k in leaves[::7]:                     # leaves that poke out of their ancestors: legal for the reference's traversal
        nodes["boundsMax"][k] += np.float32(0.75)
        nodes["boundsMin"][k] -= np.float32(0.25)
    renderer.set_scene(s)
    rng = np.random.default_rng(7)
    rays = np.concatenate([random_rays(s, rng, 800), aimed_rays(s, rng, 256)])
    for coherent in (False, True):
        for flavour in sf.FLAVOURS:
            got = check(renderer, s, rays, flavour, (coherent, flavour), coherent=coherent)
    assert renderer.stats()["own_tree_height"] == -1
    assert (got["prim"] >= 0).sum() >= 32


def test_the_callers_splits(monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        s = fuzz_scene(3)[0]
        r.set_scene(s)
        rng = np.random.default_rng(3)
        rays = np.concatenate([random_rays(s, rng, 400), aimed_rays(s, rng, 256)])
        for coherent in (False, True):
            for flavour in sf.FLAVOURS:
                got = check(r, s, rays, flavour, (coherent, flavour), coherent=coherent)
        assert r.stats()["own_tree_height"] > 0
        assert (got["prim"] >= 0).sum() >= 32
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 5: surface_at
def test_surface_at_over_the_first_eight_hits(renderer):
    import torch
    s = mh.sheets_scene()
    rays = mh.sheet_rays()[0].copy()
    payload = np.uint32([0x7fc12345, 0xffc00001, 0x7f800001]).view(np.float32)
    rays[5:8, 3] = payload                                     # NaN tmax with payloads: nothing is hit, every slot carries the bits
    renderer.set_scene(s)
    hits = renderer.trace_hits(rays, max_hits=8)
    assert hits.shape == (len(rays), 8)
    used = hits["prim"] >= 0
    assert used[:, 7].sum() >= 32 and (~used).sum() >= 32          # rays with eight hits, and unused slots
    for flavour in sf.FLAVOURS:
        got = renderer.surface_at(hits, **sf.FLAVOURS[flavour])
        assert got.shape == hits.shape and got.dtype == SURFACE_DTYPE
        assert len(sf.same(got, sf.expected(s, hits, flavour))) == 0, flavour
        tmax_bits = np.broadcast_to(rays[:, 3:4].view(np.uint32), hits.shape)
        assert np.array_equal(got["t"].view(np.uint32)[~used], tmax_bits[~used])
        assert (words(got)[(~used).reshape(-1), 1:] == np.uint32([0xffffffff, 0, 0, 0, 0, 0, 0xffffffff, 0, 0, 0, 0])).all()
        assert np.array_equal(got["t"].view(np.uint32)[5:8], np.repeat(payload.view(np.uint32)[:, None], 8, axis=1))
        # trace_surface == surface_at(trace_rays)
        for coherent in (False, True):
            first = renderer.trace_rays(rays, coherent=coherent, **sf.FLAVOURS[flavour])
            a = renderer.trace_surface(rays, coherent=coherent, **sf.FLAVOURS[flavour])
            b = renderer.surface_at(first, **sf.FLAVOURS[flavour])
            assert np.array_equal(words(a), words(b)), (flavour, coherent)
    # hand-made records: a primitive that is none gives the miss form, t as given
    hand = np.zeros(4, dtype=HIT_DTYPE)
    hand["t"], hand["prim"], hand["u"], hand["v"] = (1.5, -0.0, np.inf, 2.0), (-1, -7, -1, 3), 0.25, 0.5
    got = renderer.surface_at(hand)
    assert len(sf.same(got, sf.expected(s, hand))) == 0
    assert (got["prim"][:3] == -1).all() and (words(got)[:3, 2:] == np.uint32([0, 0, 0, 0, 0, 0xffffffff, 0, 0, 0, 0])).all()
    assert np.array_equal(got["t"].view(np.uint32), hand["t"].view(np.uint32)) and got["prim"][3] == 3 and got["material"][3] >= 0
    # torch: (..., 4) in, (..., 12) out, on a side stream
    side = torch.cuda.Stream()
    ht = torch.from_numpy(words(hits).view(np.float32).reshape(len(rays), 8, 4)).cuda()
    with torch.cuda.stream(side):
        gt = renderer.surface_at(ht)
    side.synchronize()
    assert gt.shape == (len(rays), 8, 12)
    assert np.array_equal(words(gt.cpu().numpy().reshape(-1, 12)), words(renderer.surface_at(hits)))
    st = renderer.stats()
    assert st["kernel_launches"] == 1 and st["kernel_ms"] > 0 and st["rays"] == 0 and st["shadow_rays"] == 0 and st["render_ms"] == 0


# ------------------------------------------------------------------------------------------------------------- 6: the contract
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        rays = make_rays(np.zeros((4, 3)), np.ones((4, 3)))
        hits = np.zeros(4, dtype=HIT_DTYPE)
        out = np.full(48, 0x5a5a5a5a, dtype=np.uint32)
        R, Hh, O = (x.ctypes.data_as(ctypes.c_void_p) for x in (rays, hits, out))

        def desc(program=C.PROGRAM_ACCUMULATOR, kind=C.TRACE_CLOSEST, flags=0, size=ctypes.sizeof(C.TraceDesc)):
            return ctypes.byref(C.TraceDesc(size, program, kind, flags))

        def sdesc(flags=0, size=ctypes.sizeof(C.SurfaceDesc)):
            return ctypes.byref(C.SurfaceDesc(size, flags))

        assert L.lt_hip_trace_surface(r._ctx, desc(), R, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        assert L.lt_hip_surface_at(r._ctx, sdesc(), Hh, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        assert (out == 0x5a5a5a5a).all()
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        user = r.resolve_program(os.path.join(HERE, "user_kernels", "hit_info.hip"))
        both = C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_PORTABLE_MATH
        cases = [
            (None, R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), None, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 4, None, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(kind=C.TRACE_ANY), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(kind=2), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(program=user), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(program=77), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(program=-1), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(flags=C.RENDER_FLAG_STATS), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=0x200), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=both), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(size=12), R, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 2 ** 32, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), R, 4, O, 4 * 48 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(), R, 4, O, 4 * 16, C.LT_ERR_BUFFER_TOO_SMALL),
        ]
        for i, (d, rp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_trace_surface(r._ctx, d, rp, n, op, nb) == want, i
            assert (out == 0x5a5a5a5a).all(), i
        at_cases = [
            (None, Hh, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(), None, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(), Hh, 4, None, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(flags=C.TRACE_FLAG_COHERENT), Hh, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(flags=C.RENDER_FLAG_STATS), Hh, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(flags=both), Hh, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(size=4), Hh, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(), Hh, 2 ** 32, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (sdesc(), Hh, 4, O, 4 * 48 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
        ]
        for i, (d, hp, n, op, nb, want) in enumerate(at_cases):
            assert L.lt_hip_surface_at(r._ctx, d, hp, n, op, nb) == want, i
            assert (out == 0x5a5a5a5a).all(), i
        assert L.lt_hip_trace_surface(r._ctx, desc(), R, 0, O, 0) == 0 and L.lt_hip_trace_surface(r._ctx, desc(), None, 0, None, 0) == 0
        assert L.lt_hip_surface_at(r._ctx, sdesc(), Hh, 0, O, 0) == 0 and L.lt_hip_surface_at(r._ctx, sdesc(), None, 0, None, 0) == 0
        assert (out == 0x5a5a5a5a).all()
        # the device entry points: the same checks, and 16-byte alignment
        rt = torch.from_numpy(rays).cuda()
        ht = torch.from_numpy(words(hits).view(np.float32)).cuda()
        buf = torch.full((64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        vp = ctypes.c_void_p
        for rp, op in ((rt.data_ptr() + 4, buf.data_ptr()), (rt.data_ptr(), buf.data_ptr() + 8)):
            assert L.lt_hip_trace_surface_device(r._ctx, desc(), vp(rp), 3, vp(op), 192, None) == C.LT_ERR_INVALID_ARGUMENT
        for hp, op in ((ht.data_ptr() + 4, buf.data_ptr()), (ht.data_ptr(), buf.data_ptr() + 8)):
            assert L.lt_hip_surface_at_device(r._ctx, sdesc(), vp(hp), 3, vp(op), 192, None) == C.LT_ERR_INVALID_ARGUMENT
        assert L.lt_hip_trace_surface_device(r._ctx, desc(), vp(rt.data_ptr()), 4, vp(buf.data_ptr()), 191, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert L.lt_hip_surface_at_device(r._ctx, sdesc(), vp(ht.data_ptr()), 4, vp(buf.data_ptr()), 191, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert L.lt_hip_trace_surface_device(r._ctx, desc(kind=C.TRACE_ANY), vp(rt.data_ptr()), 4, vp(buf.data_ptr()), 256, None) == C.LT_ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x5a5a5a5a).all()
        with pytest.raises(C.LensTraceError):
            r.trace_surface(rays, program=1000)
        with pytest.raises(C.LensTraceError):
            r.surface_at(hits, portable_math=True, strict_math=True)
    finally:
        r.close()


def test_calls_interleave_with_renders_and_scene_changes(edge):
    import torch
    s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
    cam = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
    W, H = 96, 64

    def render(r):
        out = np.empty((H, W, 3), dtype=np.float32)
        r.render(RenderPropertiesHIP("accumulator.cl", (W, H, 3), out, s, pCamera=cam, frameCount=4, accumulate=True, portableMath=True))
        return out, r.stats()

    r1, r2 = RendererHIP(0), RendererHIP(0)
    try:
        a1, s1 = render(r1)
        b1, t1 = render(r1)
        a2, s2 = render(r2)
        rays = random_rays(s, np.random.default_rng(9), 3000)
        surf = r2.trace_surface(rays)
        st = r2.stats()
        assert st["rays"] == len(rays) and st["shadow_rays"] == 0 and st["kernel_launches"] == 2 and st["kernel_ms"] > 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
        r2.surface_at(r2.trace_hits(rays, max_hits=2))
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        assert t2["shadow_packets"] == s2["shadow_packets"] and t2["frames"] == 4 and t2["render_ms"] > 0
        assert len(sf.same(surf, sf.expected(s, r2.trace_rays(rays)))) == 0
        # set_scene of another scene right behind enqueued device calls: they keep the old scene's results
        scene, batches = edge
        want = r2.trace_surface(rays)
        want_at = r2.surface_at(r2.trace_hits(rays, max_hits=2))
        rt = torch.from_numpy(rays).cuda()
        ht = r2.trace_hits(rt, max_hits=2)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        got = r2.trace_surface(rt, stream=stream)
        got_at = r2.surface_at(ht, stream=stream)
        r2.set_scene(scene)
        stream.synchronize()
        assert np.array_equal(words(got.cpu().numpy()), words(want))
        assert np.array_equal(words(got_at.cpu().numpy().reshape(-1, 12)), words(want_at))
        assert (want["prim"] >= 0).sum() >= 32 and (want_at["prim"] >= 0).sum() >= 32
    finally:
        r1.close()
        r2.close()
