"""GPU (-m gpu): box-overlap queries (lt_hip_overlap_boxes and its device entry point, lt_overlap_kernel and
lt_overlap_scan_kernel in lens_trace_amd/csrc/lt_overlap.hip).  Every comparison is of words: a box's sequence is a function of
the scene and the box alone (include/lenstrace_hip.h), restated in numpy by tests/overlap.py -- what that module claims is checked
without a GPU in tests/test_overlap_cpu.py.  K = 1, 3, 8, the count and any throughout.

1. every box family on the base scene, a height-field wall, the twelve-triangle fan and three scenes at the magnitude limits;
2. sizes 1 .. 4097 of a shuffled batch with LT_TRACE_REFILL 1 and 64;
3. scenes without an own tree (scanned leaf by leaf) and the caller's splits (LT_RETREE=0);
4. the stack's rows in private memory: the box that holds the whole scene pushes every slot of a group tree of height >= 4;
5. the device entry point on a side stream from torch tensors equals the host path and writes nothing behind its bytes;
6. every error writes nothing, on both entry points;
7. calls interleave with trace_rays, a render and a scene change, stats() reports the call, the answers are the host form's;
8. K = 8 with boxes and offsets that pass byte 2^32 (record 2^27), against their base batch repeated."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import BOX_DTYPE, RendererHIP, RenderPropertiesHIP, make_boxes, make_rays, overlap_boxes_host
from tests import nearest as nr
from tests import nearest_k as nk
from tests import overlap as ov
from tests import query_edges as qe
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


def check(r, m, bx, note, n=None):
    """Every kind on bx[:n] against the model's sequences `m` of bx; returns the K = 8 offsets."""
    n = len(bx) if n is None else n
    got = None
    for k in KS:
        got = r.overlap_boxes(bx[:n], k=k)
        assert got.dtype == np.int32 and got.shape == (n, k)
        want = m.first(k)[:n]
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (note, k, len(bad), bad[:5], bx[bad[:2]], got[bad[:2]], want[bad[:2]])
    count = r.overlap_boxes(bx[:n], count=True)
    hit = r.overlap_boxes(bx[:n], any=True)
    assert count.dtype == hit.dtype == np.uint32 and count.shape == hit.shape == (n,)
    assert np.array_equal(count, m.count[:n]), (note, np.flatnonzero(count != m.count[:n])[:5])
    assert np.array_equal(hit, m.any[:n]), (note, np.flatnonzero(hit != m.any[:n])[:5])
    return got


# ------------------------------------------------------------------------------------------------------------- 1: the model
@pytest.mark.parametrize("name", SCENES)
def test_against_the_model(renderer, base, name):
    s = scene_of(base, name)
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    bx = np.concatenate(list(ov.families(s, seed=SCENES.index(name)).values()))
    m = ov.sequences(s, bx)
    got = check(renderer, m, bx, name)
    assert (got >= 0).sum() >= 2048 and (got < 0).sum() >= 512
    dead = ov.empty(bx)
    assert dead.sum() >= 48 and (got[dead] == -1).all() and (m.count[dead] == 0).all()
    assert (m.count > 8).sum() >= 64 and ((m.count == 0) & ~dead).sum() >= 256


# ------------------------------------------------------------------------------------------------------------- 2: sizes
@pytest.fixture(scope="module")
def shuffled(base):
    bx = np.concatenate(list(ov.families(base, seed=5, n=512).values()))
    bx = np.ascontiguousarray(bx[np.random.default_rng(3).permutation(len(bx))][:4097])
    assert len(bx) == 4097
    return bx, ov.sequences(base, bx)


@pytest.mark.parametrize("refill", (1, 64))
def test_batch_sizes_and_refill(renderer, base, shuffled, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    bx, m = shuffled
    renderer.set_scene(base)
    for n in (1, 63, 64, 65, 511, 4097):
        check(renderer, m, bx, (n, refill), n)
    assert (m.count > 8).sum() >= 256 and (m.count == 0).sum() >= 256 and ((m.count > 0) & (m.count < 8)).sum() >= 64


# ------------------------------------------------------------------------------------------------------------- 3: other hierarchies
@pytest.mark.parametrize("name", ("nan_bound", "bound_at_limit"))
def test_scenes_without_an_own_tree(renderer, base, name):
    s = qe.extreme_scene(base, name)[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    bx = np.concatenate(list(ov.families(s, seed=7, n=96).values()))
    got = check(renderer, ov.sequences(s, bx), bx, name)
    assert (got >= 0).sum() >= 1024


def test_the_callers_splits(base, monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(base)
        assert r.stats()["own_tree_height"] > 0
        bx = np.concatenate(list(ov.families(base, seed=9, n=96).values()))
        got = check(r, ov.sequences(base, bx), bx, "LT_RETREE=0")
        assert (got >= 0).sum() >= 1024
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 4: the stack
def test_the_stack_rows_in_private_memory(renderer):
    """A box that holds the whole scene meets every slot, so a group's four children are pushed and one popped: after h groups on
    the way down the stack holds 3 h entries -- beyond the 12 in LDS from height 4 on.  Every leaf touches."""
    s = synth.heightfield_wall(16)
    renderer.set_scene(s)
    own_height, group_height, groups, _ = renderer.scene_structure(3)
    assert group_height >= 4, (own_height, group_height, groups)
    off, _, _ = nr.leaves(s)
    fam = ov.families(s, seed=2, n=128)
    whole = np.repeat(fam["g_whole"], 300, axis=0)
    bx = np.concatenate([whole, fam["h_empty"], fam["a_uniform"]])
    bx = np.ascontiguousarray(bx[np.random.default_rng(4).permutation(len(bx))])
    count = renderer.overlap_boxes(bx, count=True)
    m = ov.sequences(s, bx)
    full = m.count == len(off)
    assert full.sum() >= 600 and ov.empty(bx).sum() >= 32
    assert (count[full] == len(off)).all() and np.array_equal(count, m.count)
    first = renderer.overlap_boxes(bx, k=8)
    assert np.array_equal(first, m.first(8)) and (first[full] == np.sort(off)[:8]).all()
    assert np.array_equal(renderer.overlap_boxes(bx, any=True), m.any)


# ------------------------------------------------------------------------------------------------------------- 5: the device entry point
def test_the_device_entry_point_on_a_side_stream(renderer, base, shuffled):
    import torch
    bx, m = shuffled
    renderer.set_scene(base)
    side = torch.cuda.Stream()
    for n in (1, 65, 4097):
        bt = torch.from_numpy(bx[:n]).cuda()
        for k in KS + ("count", "any"):
            kw = dict(k=k) if isinstance(k, int) else {k: True}
            host = renderer.overlap_boxes(bx[:n], **kw)
            with torch.cuda.stream(side):
                got = renderer.overlap_boxes(bt, **kw)
            side.synchronize()
            want = m.first(k)[:n] if isinstance(k, int) else (m.count[:n] if k == "count" else m.any[:n])
            assert got.dtype == torch.int32 and got.shape == ((n, k) if isinstance(k, int) else (n,))
            assert np.array_equal(got.cpu().numpy().view(host.dtype), host) and np.array_equal(host, want), (n, k)
            # the stream named: the same words
            got2 = renderer.overlap_boxes(bt, stream=side, **kw)
            side.synchronize()
            assert torch.equal(got2, got), (n, k)
            # the raw call into a sentinel-filled buffer: nothing behind 4 K n / 4 n bytes
            words = n * k if isinstance(k, int) else n
            buf = torch.full((words + 64,), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            kind = C.OVERLAP_FIRST_K if isinstance(k, int) else C.OVERLAP_COUNT if k == "count" else C.OVERLAP_ANY
            d = C.OverlapDesc(ctypes.sizeof(C.OverlapDesc), 0, kind, k if isinstance(k, int) else 0)
            assert renderer._L.lt_hip_overlap_boxes_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(bt.data_ptr()), n,
                                                           ctypes.c_void_p(buf.data_ptr()), 4 * words, ctypes.c_void_p(side.cuda_stream)) == 0
            side.synchronize()
            out = buf.cpu().numpy()
            assert (out[words:] == SENTINEL).all(), (n, k)
            assert np.array_equal(out[:words].view(np.uint32), np.ascontiguousarray(host).view(np.uint32).reshape(-1)), (n, k)


# ------------------------------------------------------------------------------------------------------------- 6: errors
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        bx = make_boxes(np.full((4, 3), -100.0), np.full((4, 3), 100.0))
        out = np.full(4 * 2, SENTINEL, dtype=np.uint32)       # room for K = 2
        B, O = (x.ctypes.data_as(ctypes.c_void_p) for x in (bx, out))
        FIRST, COUNT, ANY = C.OVERLAP_FIRST_K, C.OVERLAP_COUNT, C.OVERLAP_ANY

        def desc(kind=FIRST, max_k=2, flags=0, size=ctypes.sizeof(C.OverlapDesc)):
            return ctypes.byref(C.OverlapDesc(size, flags, kind, max_k))

        assert L.lt_hip_overlap_boxes(r._ctx, desc(), B, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        assert (out == SENTINEL).all()
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        INVALID = C.LT_ERR_INVALID_ARGUMENT
        cases = [
            (None, B, 4, O, out.nbytes, INVALID),
            (desc(size=12), B, 4, O, out.nbytes, INVALID),
            (desc(flags=1), B, 4, O, out.nbytes, INVALID),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH), B, 4, O, out.nbytes, INVALID),
            (desc(kind=3), B, 4, O, out.nbytes, INVALID),
            (desc(kind=-1), B, 4, O, out.nbytes, INVALID),
            (desc(max_k=0), B, 4, O, out.nbytes, INVALID),
            (desc(max_k=C.OVERLAP_MAX_K + 1), B, 4, O, out.nbytes, INVALID),
            (desc(COUNT, 1), B, 4, O, out.nbytes, INVALID),
            (desc(ANY, 1), B, 4, O, out.nbytes, INVALID),
            (desc(), B, 2 ** 32, O, out.nbytes, INVALID),
            (desc(COUNT, 0), B, 2 ** 32, O, out.nbytes, INVALID),
            (desc(), None, 4, O, out.nbytes, INVALID),
            (desc(), B, 4, None, out.nbytes, INVALID),
            (desc(), B, 4, O, 4 * 2 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(max_k=8), B, 4, O, out.nbytes, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(COUNT, 0), B, 4, O, 4 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(ANY, 0), B, 4, O, 4 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            # an unknown kind and a max_k out of range come before the buffer's size
            (desc(kind=7), B, 4, O, 0, INVALID),
            (desc(max_k=9), B, 4, O, 0, INVALID),
        ]
        for i, (d, bp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_overlap_boxes(r._ctx, d, bp, n, op, nb) == want, i
            assert (out == SENTINEL).all(), i
        assert L.lt_hip_overlap_boxes(r._ctx, desc(), B, 0, O, 0) == 0 and L.lt_hip_overlap_boxes(r._ctx, desc(ANY, 0), None, 0, None, 0) == 0
        assert (out == SENTINEL).all()
        # the device entry point: the same checks, and 16-byte alignment
        bt = torch.from_numpy(bx).cuda()
        buf = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
        vp = ctypes.c_void_p
        f = L.lt_hip_overlap_boxes_device
        for bp, op in ((bt.data_ptr() + 4, buf.data_ptr()), (bt.data_ptr(), buf.data_ptr() + 8)):
            assert f(r._ctx, desc(), vp(bp), 3, vp(op), 128, None) == INVALID
            assert f(r._ctx, desc(COUNT, 0), vp(bp), 3, vp(op), 128, None) == INVALID
        assert f(r._ctx, desc(), vp(bt.data_ptr()), 4, vp(buf.data_ptr()), 31, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert f(r._ctx, desc(COUNT, 0), vp(bt.data_ptr()), 4, vp(buf.data_ptr()), 15, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert f(r._ctx, desc(flags=2), vp(bt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        assert f(r._ctx, desc(kind=3), vp(bt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        assert f(r._ctx, desc(max_k=9), vp(bt.data_ptr()), 4, vp(buf.data_ptr()), 256, None) == INVALID
        assert f(r._ctx, None, vp(bt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
        with pytest.raises(ValueError):
            r.overlap_boxes(np.zeros((4, 6), dtype=F32))
        with pytest.raises(ValueError):
            r.overlap_boxes(bx, k=9)
        with pytest.raises(ValueError):
            r.overlap_boxes(bx, k=2, count=True)
        with pytest.raises(ValueError):
            r.overlap_boxes(bx, count=True, any=True)
        with pytest.raises(ValueError):
            r.overlap_boxes(bt[:, :6].contiguous())
        # calls that work, on the same context
        got = r.overlap_boxes(bx.view(BOX_DTYPE).reshape(-1), k=2)
        assert (got == [0, 1]).all() and (r.overlap_boxes(bx, count=True) > 2).all() and (r.overlap_boxes(bx, any=True) == 1).all()
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 7: the contract
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
        bx = np.concatenate(list(ov.families(s, seed=4, n=128).values()))
        m = ov.sequences(s, bx)
        rng = np.random.default_rng(9)
        rays = make_rays(rng.uniform(-5, 5, (512, 3)) + (0, 2.5, -20), rng.normal(0, 0.2, (512, 3)) + (0, 0, 1))
        hits_before = r2.trace_rays(rays)
        first = r2.overlap_boxes(bx, k=8)
        st = r2.stats()
        assert st["rays"] == len(bx) and st["shadow_rays"] == 0 and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
        count = r2.overlap_boxes(bx, count=True)
        st = r2.stats()
        assert st["rays"] == len(bx) and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        hit = r2.overlap_boxes(bx, any=True)
        assert np.array_equal(first, m.first(8)) and np.array_equal(count, m.count) and np.array_equal(hit, m.any)
        assert np.array_equal(r2.trace_rays(rays).view(np.uint32), hits_before.view(np.uint32))
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # the GPU's answers are the host form's
        for k in KS:
            assert np.array_equal(r2.overlap_boxes(bx, k=k), overlap_boxes_host(s, bx, k=k)), k
        assert np.array_equal(count, overlap_boxes_host(s, bx, count=True)) and np.array_equal(hit, overlap_boxes_host(s, bx, any=True))
        assert (m.count > 8).sum() >= 32 and (m.count == 0).sum() >= 256
        # set_scene of another scene right behind an enqueued device call: it keeps the old scene's results
        bt = torch.from_numpy(bx).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        got = r2.overlap_boxes(bt, k=3, stream=stream)
        r2.set_scene(base)
        stream.synchronize()
        assert np.array_equal(got.cpu().numpy(), m.first(3))
        bb = ov.families(base, seed=6, n=64)["b_on"]
        assert np.array_equal(r2.overlap_boxes(bb, k=3), ov.sequences(base, bb).first(3))
    finally:
        r1.close()
        r2.close()


# ------------------------------------------------------------------------------------------------------------- 8: past 4 GiB
def test_records_past_4_gib():
    """n = 2^27 + 2^20 + 37 boxes at K = 8: 32 n bytes of boxes and 32 n bytes of offsets, 4.33 GB each, record 2^27 of either starts
    at byte 2^32.  A base batch of 4099 (prime) boxes on the Cornell box, settled by the model, repeated on the device into a
    sentinel-filled output: every box's eight offsets must be the base's of the same phase and none may keep the sentinel
    (tests/large_offsets.py, check_periodic).  Holds 8.66 GB of boxes and offsets and the comparison's masks and temporaries:
    9.8 GB of device memory, below the 16 GiB a test may hold."""
    import torch
    from tests import large_offsets as LO
    n, K = LO.N_RAYS, 8
    need = 32 * n + 4 * K * n + LO.COMPARE_BYTES
    assert need < LO.DEVICE_LIMIT and 32 * n > 2 ** 32 and 4 * K * n > 2 ** 32
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d bytes of device memory, the device has %d free" % (need, free))
    s = LO.scene()
    bx = np.concatenate(list(ov.families(s, seed=8, n=512).values()))
    bx = np.ascontiguousarray(bx[np.random.default_rng(8).permutation(len(bx))][:LO.B_PRIME])
    m = ov.sequences(s, bx)
    assert len(bx) == LO.B_PRIME and (m.count > 8).mean() > 0.02 and (m.count < 8).mean() > 0.3 and (m.count > 0).mean() > 0.3
    r = RendererHIP(0)
    big = out = base_t = None
    try:
        r.set_scene(s)
        base_t = torch.from_numpy(bx).cuda()
        base_out = r.overlap_boxes(base_t, k=K)
        assert np.array_equal(base_out.cpu().numpy(), m.first(K))
        big = base_t.repeat(-(-n // LO.B_PRIME), 1)[:n].contiguous()
        out = torch.full((K * n,), LO.SENTINEL, dtype=torch.int32, device="cuda")
        d = C.OverlapDesc(ctypes.sizeof(C.OverlapDesc), 0, C.OVERLAP_FIRST_K, K)
        r._check(r._L.lt_hip_overlap_boxes_device(r._ctx, ctypes.byref(d), ctypes.c_void_p(big.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                                  4 * K * n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        rep = LO.check_periodic(out.view(n, K), base_out.contiguous().view(LO.B_PRIME, K))
        assert rep.ok, str(rep)
    finally:
        del big, out, base_t
        torch.cuda.synchronize()
        r.close()
        torch.cuda.empty_cache()
