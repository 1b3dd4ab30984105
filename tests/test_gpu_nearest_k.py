"""GPU (-m gpu): k-nearest queries (lt_hip_nearest_k and its device entry point, lt_nearest_k_kernel in
lens_trace_amd/csrc/lt_nearest.hip).  Every comparison is of words: a point's candidate sequence is a function of the scene and
the point alone (include/lenstrace_hip.h), restated in numpy by tests/nearest_k.py -- what that module claims is checked without
a GPU in tests/test_nearest_k_cpu.py.  K = 1, 3, 8 and the count throughout; K = 1 is compared with nearest_points as well.

1. every point family on the base scene, a height-field wall, the twelve-triangle fan and three scenes at the magnitude limits;
2. sizes 1 .. 4097 of a shuffled batch with LT_TRACE_REFILL 1 and 64;
3. scenes without an own tree (scanned leaf by leaf) and the caller's splits (LT_RETREE=0);
4. the stack's rows in private memory: a count with max_d2 = inf pushes every slot of a group tree of height >= 4;
5. the device entry point on a side stream from torch tensors equals the host path and writes nothing behind its bytes;
6. every error writes nothing, on both entry points;
7. surface_at over the K records gives tests/surface.py's records;
8. calls interleave with trace_rays, a render and a scene change, stats() reports the call, the answers are the host form's;
9. K = 8 records that pass byte 2^32 (record 2^28), against their base batch repeated."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import HIT_DTYPE, POINT_DTYPE, RendererHIP, RenderPropertiesHIP, make_points, make_rays, nearest_k_host
from tests import nearest as nr
from tests import nearest_k as nk
from tests import query_edges as qe
from tests import surface as sf
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = (1, 3, 8)
SCENES = ("base", "wall16", "fan12", "tiny", "large", "far+")
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def base():
    return qe.base_scene(0)


def scene_of(base, name):
    if name == "base":
        return base
    if name == "wall16":
        return synth.heightfield_wall(16)
    if name == "fan12":
        return nk.fan12()
    return qe.extreme_scene(base, name)[0]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)


def check(r, m, pts, note, n=None):
    """Every kind on pts[:n] against the model's sequences `m` of pts; returns the K = 8 records."""
    n = len(pts) if n is None else n
    got = None
    for k in KS:
        got = r.nearest_k(pts[:n], k=k)
        assert got.dtype == HIT_DTYPE and got.shape == (n, k)
        want = m.records(k)[:n]
        bad = nk.same(got, want)
        assert len(bad) == 0, (note, k, len(bad), bad[:5], pts[bad[:3] // k], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])
        if k == 1:
            assert np.array_equal(words(got), words(r.nearest_points(pts[:n]))), note
    count = r.nearest_k(pts[:n], count=True)
    assert count.dtype == np.uint32 and count.shape == (n,)
    assert np.array_equal(count, m.count[:n]), (note, np.flatnonzero(count != m.count[:n])[:5])
    return got


# ------------------------------------------------------------------------------------------------------------- 1: the model
@pytest.mark.parametrize("name", SCENES)
def test_against_the_model(renderer, base, name):
    s = scene_of(base, name)
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    pts = np.concatenate(list(nk.families(s, seed=SCENES.index(name)).values()))
    m = nk.sequences(s, pts)
    got = check(renderer, m, pts, name)
    assert (got["prim"] >= 0).sum() >= 2048 and (got["prim"] < 0).sum() >= 512
    dead = nr.no_walk(pts)
    assert dead.sum() >= 48 and (got["prim"][dead] == -1).all() and (m.count[dead] == 0).all()
    if name == "fan12":
        assert (m.ties >= 12).sum() >= 16


# ------------------------------------------------------------------------------------------------------------- 2: sizes
@pytest.fixture(scope="module")
def shuffled(base):
    pts = np.concatenate(list(nk.families(base, seed=5, n=512).values()))
    pts = pts[np.random.default_rng(3).permutation(len(pts))][:4097]
    assert len(pts) == 4097
    return pts, nk.sequences(base, pts)


@pytest.mark.parametrize("refill", (1, 64))
def test_batch_sizes_and_refill(renderer, base, shuffled, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    pts, m = shuffled
    renderer.set_scene(base)
    for n in (1, 63, 64, 65, 511, 4097):
        check(renderer, m, pts, (n, refill), n)
    assert (m.count > 8).sum() >= 1024 and (m.count == 0).sum() >= 256 and ((m.count > 0) & (m.count < 8)).sum() >= 64


# ------------------------------------------------------------------------------------------------------------- 3: other hierarchies
@pytest.mark.parametrize("name", ("nan_bound", "bound_at_limit"))
def test_scenes_without_an_own_tree(renderer, base, name):
    s = qe.extreme_scene(base, name)[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    pts = np.concatenate(list(nk.families(s, seed=7, n=96).values()))
    got = check(renderer, nk.sequences(s, pts), pts, name)
    assert (got["prim"] >= 0).sum() >= 1024


def test_the_callers_splits(base, monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(base)
        assert r.stats()["own_tree_height"] > 0
        pts = np.concatenate(list(nk.families(base, seed=9, n=96).values()))
        got = check(r, nk.sequences(base, pts), pts, "LT_RETREE=0")
        assert (got["prim"] >= 0).sum() >= 1024
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 4: the stack
def test_the_stack_rows_in_private_memory(renderer):
    """max_d2 = inf keeps every slot, so a group's four children are pushed and one popped: after h groups on the way down the
    stack holds 3 h entries -- beyond the 7 in LDS from height 3 on.  Every leaf is a candidate of every finite point."""
    s = synth.heightfield_wall(16)
    renderer.set_scene(s)
    own_height, group_height, groups, _ = renderer.scene_structure(3)
    assert group_height >= 4, (own_height, group_height, groups)
    off, _, _ = nr.leaves(s)
    fam = nr.families(s, seed=2, n=128)
    pts = np.concatenate([fam["a_uniform"], fam["c_off"], fam["f_nonfinite"]])
    pts[:, 3] = np.inf
    count = renderer.nearest_k(pts, count=True)
    finite = np.isfinite(pts[:, 0:3]).all(axis=1)
    assert finite.sum() >= 512 and (~finite).sum() >= 32
    assert (count[finite] == len(off)).all() and (count[~finite] == 0).all()
    assert np.array_equal(count, nk.sequences(s, pts).count)


# ------------------------------------------------------------------------------------------------------------- 5: the device entry point
def test_the_device_entry_point_on_a_side_stream(renderer, base, shuffled):
    import torch
    pts, m = shuffled
    renderer.set_scene(base)
    side = torch.cuda.Stream()
    for n in (1, 65, 4097):
        pt = torch.from_numpy(pts[:n]).cuda()
        for k in KS + (0,):
            count = k == 0
            host = renderer.nearest_k(pts[:n], k=max(k, 1), count=count)
            with torch.cuda.stream(side):
                got = renderer.nearest_k(pt, k=max(k, 1), count=count)
            side.synchronize()
            if count:
                assert got.shape == (n,) and got.dtype == torch.int32
                assert np.array_equal(got.cpu().numpy().view(np.uint32), host) and np.array_equal(host, m.count[:n]), n
            else:
                assert got.shape == (n, k, 4) and got.dtype == torch.float32
                assert np.array_equal(words(got.cpu().numpy()), words(host)) and len(nk.same(host, m.records(k)[:n])) == 0, (n, k)
            # (n, 3) positions with a per-point max_d2 tensor, the stream named: the same records
            got3 = renderer.nearest_k(pt[:, 0:3].contiguous(), k=max(k, 1), count=count, max_d2=pt[:, 3].contiguous(), stream=side)
            side.synchronize()
            assert torch.equal(got3.view(torch.int32), got.view(torch.int32)), (n, k)
            # the raw call into a sentinel-filled buffer: nothing behind 16 K n / 4 n bytes
            need = 4 * n if count else 16 * k * n
            buf = torch.full((need // 4 + 64,), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            d = C.NearestKDesc(ctypes.sizeof(C.NearestKDesc), 0, C.NEAREST_COUNT if count else C.NEAREST_FIRST_K, k)
            assert renderer._L.lt_hip_nearest_k_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(pt.data_ptr()), n,
                                                       ctypes.c_void_p(buf.data_ptr()), need, ctypes.c_void_p(side.cuda_stream)) == 0
            side.synchronize()
            out = buf.cpu().numpy()
            assert (out[need // 4:] == SENTINEL).all(), (n, k)
            assert np.array_equal(out[:need // 4].view(np.uint32), np.ascontiguousarray(host).view(np.uint32).reshape(-1)), (n, k)


# ------------------------------------------------------------------------------------------------------------- 6: errors
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        pts = make_points(np.zeros((4, 3)))
        out = np.full(4 * 4 * 2, SENTINEL, dtype=np.uint32)       # room for K = 2
        P, O = (x.ctypes.data_as(ctypes.c_void_p) for x in (pts, out))
        FIRST, COUNT = C.NEAREST_FIRST_K, C.NEAREST_COUNT

        def desc(kind=FIRST, max_k=2, flags=0, size=ctypes.sizeof(C.NearestKDesc)):
            return ctypes.byref(C.NearestKDesc(size, flags, kind, max_k))

        assert L.lt_hip_nearest_k(r._ctx, desc(), P, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        assert (out == SENTINEL).all()
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        INVALID = C.LT_ERR_INVALID_ARGUMENT
        cases = [
            (None, P, 4, O, out.nbytes, INVALID),
            (desc(size=12), P, 4, O, out.nbytes, INVALID),
            (desc(flags=1), P, 4, O, out.nbytes, INVALID),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH), P, 4, O, out.nbytes, INVALID),
            (desc(kind=2), P, 4, O, out.nbytes, INVALID),
            (desc(kind=-1), P, 4, O, out.nbytes, INVALID),
            (desc(max_k=0), P, 4, O, out.nbytes, INVALID),
            (desc(max_k=C.NEAREST_MAX_K + 1), P, 4, O, out.nbytes, INVALID),
            (desc(COUNT, 1), P, 4, O, out.nbytes, INVALID),
            (desc(), P, 2 ** 32, O, out.nbytes, INVALID),
            (desc(COUNT, 0), P, 2 ** 32, O, out.nbytes, INVALID),
            (desc(), None, 4, O, out.nbytes, INVALID),
            (desc(), P, 4, None, out.nbytes, INVALID),
            (desc(), P, 4, O, 16 * 2 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(max_k=8), P, 4, O, out.nbytes, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(COUNT, 0), P, 4, O, 4 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            # an unknown kind and a max_k out of range come before the buffer's size
            (desc(kind=7), P, 4, O, 0, INVALID),
            (desc(max_k=9), P, 4, O, 0, INVALID),
        ]
        for i, (d, pp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_nearest_k(r._ctx, d, pp, n, op, nb) == want, i
            assert (out == SENTINEL).all(), i
        assert L.lt_hip_nearest_k(r._ctx, desc(), P, 0, O, 0) == 0 and L.lt_hip_nearest_k(r._ctx, desc(COUNT, 0), None, 0, None, 0) == 0
        assert (out == SENTINEL).all()
        # the device entry point: the same checks, and 16-byte alignment
        pt = torch.from_numpy(pts).cuda()
        buf = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
        vp = ctypes.c_void_p
        f = L.lt_hip_nearest_k_device
        for pp, op in ((pt.data_ptr() + 4, buf.data_ptr()), (pt.data_ptr(), buf.data_ptr() + 8)):
            assert f(r._ctx, desc(), vp(pp), 3, vp(op), 128, None) == INVALID
            assert f(r._ctx, desc(COUNT, 0), vp(pp), 3, vp(op), 128, None) == INVALID
        assert f(r._ctx, desc(), vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 127, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert f(r._ctx, desc(COUNT, 0), vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 15, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert f(r._ctx, desc(flags=2), vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        assert f(r._ctx, desc(kind=3), vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        assert f(r._ctx, desc(max_k=9), vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 256, None) == INVALID
        assert f(r._ctx, None, vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
        with pytest.raises(ValueError):
            r.nearest_k(np.zeros((4, 2), dtype=F32))
        with pytest.raises(ValueError):
            r.nearest_k(pts, k=9)
        with pytest.raises(ValueError):
            r.nearest_k(pts, max_d2=1.0)
        # calls that work, on the same context
        got = r.nearest_k(pts.view(POINT_DTYPE).reshape(-1), k=2)
        assert (got["prim"] >= 0).all() and (r.nearest_k(pts, count=True) > 2).all()
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 7: surface records
def test_surface_records_of_the_k_closest_points(renderer, base):
    wall = synth.heightfield_wall(16)
    for s, seed in ((base, 1), (wall, 2)):
        renderer.set_scene(s)
        fam = nk.families(s, seed=seed, n=96)
        pts = np.concatenate([fam[k] for k in ("a_uniform", "b_on", "c_off", "g_radius")])
        near = renderer.nearest_k(pts, k=8)
        assert len(nk.same(near, nk.sequences(s, pts).records(8))) == 0
        for flavour in sf.FLAVOURS:
            got = renderer.surface_at(near, **sf.FLAVOURS[flavour])
            assert got.shape == near.shape and len(sf.same(got, sf.expected(s, near, flavour))) == 0, flavour
        hit = near["prim"] >= 0
        assert hit.sum() >= 2048 and (~hit).sum() >= 64
        # the position is the closest point of that primitive: its squared distance to P is the record's t, within the bound
        # tests/test_gpu_nearest.py derives for the nearest record (64 * 2^-24 m^2) -- the arithmetic is the same for every entry
        P = np.broadcast_to(pts[:, None, 0:3], near.shape + (3,))[hit].astype(np.float64)
        d2 = ((got["position"][hit].astype(np.float64) - P) ** 2).sum(axis=1)
        scale = (np.abs(P).max(axis=1) + np.abs(got["position"][hit]).max(axis=1)) ** 2
        assert (np.abs(d2 - near["t"][hit]) <= 64 * 2.0 ** -24 * scale).all()
        assert (got["material"][hit] >= 0).all() and (got["prim"][~hit] == -1).all()


# ------------------------------------------------------------------------------------------------------------- 8: the contract
def test_calls_interleave_and_stats_report_them(base):
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
        pts = np.concatenate(list(nk.families(s, seed=4, n=128).values()))
        m = nk.sequences(s, pts)
        rng = np.random.default_rng(9)
        rays = make_rays(rng.uniform(-5, 5, (512, 3)) + (0, 2.5, -20), rng.normal(0, 0.2, (512, 3)) + (0, 0, 1))
        hits_before = r2.trace_rays(rays)
        near = r2.nearest_k(pts, k=8)
        st = r2.stats()
        assert st["rays"] == len(pts) and st["shadow_rays"] == 0 and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
        count = r2.nearest_k(pts, count=True)
        st = r2.stats()
        assert st["rays"] == len(pts) and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        assert len(nk.same(near, m.records(8))) == 0 and np.array_equal(count, m.count)
        assert np.array_equal(words(r2.trace_rays(rays)), words(hits_before))
        assert np.array_equal(words(r2.nearest_k(pts, k=1)), words(r2.nearest_points(pts)))
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # the GPU's answers are the host form's
        for k in KS:
            assert len(nk.same(r2.nearest_k(pts, k=k), nearest_k_host(s, pts, k=k))) == 0, k
        assert np.array_equal(count, nearest_k_host(s, pts, count=True))
        assert (m.count > 8).sum() >= 256
        # set_scene of another scene right behind an enqueued device call: it keeps the old scene's results
        pt = torch.from_numpy(pts).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        got = r2.nearest_k(pt, k=3, stream=stream)
        r2.set_scene(base)
        stream.synchronize()
        assert np.array_equal(words(got.cpu().numpy()), words(m.records(3)))
        bpts = nk.families(base, seed=6, n=64)["c_off"]
        assert len(nk.same(r2.nearest_k(bpts, k=3), nk.sequences(base, bpts).records(3))) == 0
    finally:
        r1.close()
        r2.close()


# ------------------------------------------------------------------------------------------------------------- 9: past 4 GiB
def test_records_past_4_gib():
    """n = 2^25 + 2^12 + 5 points at K = 8: 128 n bytes of records, 4.3 GB, record 2^28 starts at byte 2^32.  A base batch of 4099
    (prime) points on the Cornell box, settled by the model, repeated on the device into a sentinel-filled output: every point's
    eight records must be the base's of the same phase and none may keep the sentinel (tests/large_offsets.py, check_periodic).
    Holds 16 n bytes of points, 128 n of records and the comparison's masks and temporaries."""
    import torch
    from tests import large_offsets as LO
    n, K = LO.N_HITS, 8
    need = 16 * n + 16 * K * n + LO.COMPARE_BYTES
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d bytes of device memory, the device has %d free" % (need, free))
    s = LO.scene()
    pts = np.concatenate(list(nk.families(s, seed=8, n=512).values()))
    pts = np.ascontiguousarray(pts[np.random.default_rng(8).permutation(len(pts))][:LO.B_PRIME])
    m = nk.sequences(s, pts)
    assert len(pts) == LO.B_PRIME and (m.count > 8).mean() > 0.3 and (m.count < 8).mean() > 0.05
    r = RendererHIP(0)
    big = out = base_t = None
    try:
        r.set_scene(s)
        base_t = torch.from_numpy(pts).cuda()
        base_out = r.nearest_k(base_t, k=K)
        assert len(nk.same(base_out.cpu().numpy(), m.records(K))) == 0
        big = base_t.repeat(-(-n // LO.B_PRIME), 1)[:n].contiguous()
        out = torch.full((4 * K * n,), LO.SENTINEL, dtype=torch.int32, device="cuda")
        d = C.NearestKDesc(ctypes.sizeof(C.NearestKDesc), 0, C.NEAREST_FIRST_K, K)
        r._check(r._L.lt_hip_nearest_k_device(r._ctx, ctypes.byref(d), ctypes.c_void_p(big.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                              16 * K * n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        rep = LO.check_periodic(out.view(n, 32), base_out.contiguous().view(torch.int32).view(LO.B_PRIME, 32))
        assert rep.ok, str(rep)
    finally:
        del big, out, base_t
        torch.cuda.synchronize()
        r.close()
        torch.cuda.empty_cache()
