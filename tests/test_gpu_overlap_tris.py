"""GPU (-m gpu): triangle-overlap queries (lt_hip_overlap_tris and its device entry point, lt_overlap_tris_kernel and
lt_overlap_tris_scan_kernel in lens_trace_amd/csrc/lt_tritri.hip).  Every comparison is of words: a query's sequence is a function
of the scene and the query alone (include/lenstrace_hip.h), restated in numpy by tests/overlap_tris.py -- what that module claims
is checked without a GPU in tests/test_overlap_tris_cpu.py.  K = 1, 3, 8, the count and any throughout.

1. every query family on the base scene, a height-field wall, the twelve-triangle fan and three scenes at the magnitude limits;
2. sizes 1 .. 4097 of a shuffled batch with LT_TRACE_REFILL 1 and 64;
3. scenes without an own tree (scanned leaf by leaf) and the caller's splits (LT_RETREE=0);
4. the stack's rows in private memory: a cut whose box holds the whole scene pushes every slot of a group tree of height >= 4;
5. the device entry point on a side stream from torch tensors equals the host path and writes nothing behind its bytes;
6. every error writes nothing, on both entry points;
7. calls interleave with trace_rays, overlap_boxes, a render and a scene change, stats() reports the call, the answers are the
   host form's."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import TRI_DTYPE, RendererHIP, RenderPropertiesHIP, make_boxes, make_rays, make_tris, overlap_tris_host
from tests import nearest as nr
from tests import nearest_k as nk
from tests import overlap_tris as ot
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


def check(r, m, tr, note, n=None):
    """Every kind on tr[:n] against the model's sequences `m` of tr; returns the K = 8 offsets."""
    n = len(tr) if n is None else n
    got = None
    for k in KS:
        got = r.overlap_tris(tr[:n], k=k)
        assert got.dtype == np.int32 and got.shape == (n, k)
        want = m.first(k)[:n]
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (note, k, len(bad), bad[:5], tr[bad[:2]], got[bad[:2]], want[bad[:2]])
    count = r.overlap_tris(tr[:n], count=True)
    hit = r.overlap_tris(tr[:n], any=True)
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
    tr = np.concatenate(list(ot.families(s, seed=SCENES.index(name)).values()))
    m = ot.sequences(s, tr)
    got = check(renderer, m, tr, name)
    dead = ot.empty(tr)
    assert dead.sum() == 27 and (got[dead] == -1).all() and (m.count[dead] == 0).all()
    assert (got >= 0).sum() >= 1024 and (got < 0).sum() >= 512
    assert ((m.count > 0) & ~dead).sum() >= 32 and ((m.count == 0) & ~dead).sum() >= 32
    if name in ("base", "wall16", "fan12"):
        assert (m.count > 8).sum() >= 64 and ((m.count == 0) & ~dead).sum() >= 256 and ((m.count >= 1) & (m.count <= 7)).sum() >= 64


# ------------------------------------------------------------------------------------------------------------- 2: sizes
@pytest.fixture(scope="module")
def shuffled(base):
    tr = np.concatenate(list(ot.families(base, seed=5, n=768).values()))
    tr = np.ascontiguousarray(tr[np.random.default_rng(3).permutation(len(tr))][:4097])
    assert len(tr) == 4097
    return tr, ot.sequences(base, tr)


@pytest.mark.parametrize("refill", (1, 64))
def test_batch_sizes_and_refill(renderer, base, shuffled, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    tr, m = shuffled
    renderer.set_scene(base)
    for n in (1, 63, 64, 65, 511, 4097):
        check(renderer, m, tr, (n, refill), n)
    assert (m.count > 8).sum() >= 256 and (m.count == 0).sum() >= 256 and ((m.count > 0) & (m.count < 8)).sum() >= 64


# ------------------------------------------------------------------------------------------------------------- 3: other hierarchies
@pytest.mark.parametrize("name", ("nan_bound", "bound_at_limit"))
def test_scenes_without_an_own_tree(renderer, base, name):
    s = qe.extreme_scene(base, name)[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    tr = np.concatenate(list(ot.families(s, seed=7, n=96).values()))
    got = check(renderer, ot.sequences(s, tr), tr, name)
    assert (got >= 0).sum() >= 512


def test_the_callers_splits(base, monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(base)
        assert r.stats()["own_tree_height"] > 0
        tr = np.concatenate(list(ot.families(base, seed=9, n=96).values()))
        got = check(r, ot.sequences(base, tr), tr, "LT_RETREE=0")
        assert (got >= 0).sum() >= 512
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 4: the stack
def test_the_stack_rows_in_private_memory(renderer):
    """The cut's box holds the whole scene, so it meets every slot: a group's four children are pushed and one popped, and after h
    groups on the way down the stack holds 3 h entries -- beyond the 12 in LDS from height 4 on.  The count is the model's."""
    s = synth.heightfield_wall(16)
    renderer.set_scene(s)
    own_height, group_height, groups, _ = renderer.scene_structure(3)
    assert group_height >= 4, (own_height, group_height, groups)
    fam = ot.families(s, seed=2, n=128)
    cut = np.repeat(fam["g_whole"][:1], 300, axis=0)
    tr = np.concatenate([cut, fam["h_empty"], fam["a_uniform"]])
    tr = np.ascontiguousarray(tr[np.random.default_rng(4).permutation(len(tr))])
    lo, hi = nr.root_box(s)
    qlo, qhi = ot.query_box(cut[:1])
    assert (qlo <= lo).all() and (qhi >= hi).all()
    m = ot.sequences(s, tr)
    full = m.count == m.count.max()
    assert full.sum() == 300 and m.count.max() >= 16 and ot.empty(tr).sum() == 27
    assert np.array_equal(renderer.overlap_tris(tr, count=True), m.count)
    assert np.array_equal(renderer.overlap_tris(tr, k=8), m.first(8))
    assert np.array_equal(renderer.overlap_tris(tr, any=True), m.any)


# ------------------------------------------------------------------------------------------------------------- 5: the device entry point
def test_the_device_entry_point_on_a_side_stream(renderer, base, shuffled):
    import torch
    tr, m = shuffled
    renderer.set_scene(base)
    side = torch.cuda.Stream()
    for n in (1, 65, 4097):
        tt = torch.from_numpy(tr[:n]).cuda()
        for k in KS + ("count", "any"):
            kw = dict(k=k) if isinstance(k, int) else {k: True}
            host = renderer.overlap_tris(tr[:n], **kw)
            with torch.cuda.stream(side):
                got = renderer.overlap_tris(tt, **kw)
            side.synchronize()
            want = m.first(k)[:n] if isinstance(k, int) else (m.count[:n] if k == "count" else m.any[:n])
            assert got.dtype == torch.int32 and got.shape == ((n, k) if isinstance(k, int) else (n,))
            assert np.array_equal(got.cpu().numpy().view(host.dtype), host) and np.array_equal(host, want), (n, k)
            # the stream named: the same words
            got2 = renderer.overlap_tris(tt, stream=side, **kw)
            side.synchronize()
            assert torch.equal(got2, got), (n, k)
            # the raw call into a sentinel-filled buffer: nothing behind 4 K n / 4 n bytes
            words = n * k if isinstance(k, int) else n
            buf = torch.full((words + 64,), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            kind = C.OVERLAP_FIRST_K if isinstance(k, int) else C.OVERLAP_COUNT if k == "count" else C.OVERLAP_ANY
            d = C.OverlapDesc(ctypes.sizeof(C.OverlapDesc), 0, kind, k if isinstance(k, int) else 0)
            assert renderer._L.lt_hip_overlap_tris_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(tt.data_ptr()), n,
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
        tr = make_tris(np.full((4, 3), -100.0), np.tile([100.0, -100.0, 100.0], (4, 1)), np.tile([0.0, 200.0, 0.0], (4, 1)))
        out = np.full(4 * 2, SENTINEL, dtype=np.uint32)       # room for K = 2
        T, O = (x.ctypes.data_as(ctypes.c_void_p) for x in (tr, out))
        FIRST, COUNT, ANY = C.OVERLAP_FIRST_K, C.OVERLAP_COUNT, C.OVERLAP_ANY

        def desc(kind=FIRST, max_k=2, flags=0, size=ctypes.sizeof(C.OverlapDesc)):
            return ctypes.byref(C.OverlapDesc(size, flags, kind, max_k))

        assert L.lt_hip_overlap_tris(r._ctx, desc(), T, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        assert (out == SENTINEL).all()
        s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
        r.set_scene(s)
        INVALID = C.LT_ERR_INVALID_ARGUMENT
        cases = [
            (None, T, 4, O, out.nbytes, INVALID),
            (desc(size=12), T, 4, O, out.nbytes, INVALID),
            (desc(flags=1), T, 4, O, out.nbytes, INVALID),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH), T, 4, O, out.nbytes, INVALID),
            (desc(kind=3), T, 4, O, out.nbytes, INVALID),
            (desc(kind=-1), T, 4, O, out.nbytes, INVALID),
            (desc(max_k=0), T, 4, O, out.nbytes, INVALID),
            (desc(max_k=C.OVERLAP_MAX_K + 1), T, 4, O, out.nbytes, INVALID),
            (desc(COUNT, 1), T, 4, O, out.nbytes, INVALID),
            (desc(ANY, 1), T, 4, O, out.nbytes, INVALID),
            (desc(), T, 2 ** 32, O, out.nbytes, INVALID),
            (desc(COUNT, 0), T, 2 ** 32, O, out.nbytes, INVALID),
            (desc(), None, 4, O, out.nbytes, INVALID),
            (desc(), T, 4, None, out.nbytes, INVALID),
            (desc(), T, 4, O, 4 * 2 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(max_k=8), T, 4, O, out.nbytes, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(COUNT, 0), T, 4, O, 4 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(ANY, 0), T, 4, O, 4 * 4 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            # an unknown kind and a max_k out of range come before the buffer's size
            (desc(kind=7), T, 4, O, 0, INVALID),
            (desc(max_k=9), T, 4, O, 0, INVALID),
        ]
        for i, (d, tp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_overlap_tris(r._ctx, d, tp, n, op, nb) == want, i
            assert (out == SENTINEL).all(), i
        assert L.lt_hip_overlap_tris(r._ctx, desc(), T, 0, O, 0) == 0 and L.lt_hip_overlap_tris(r._ctx, desc(ANY, 0), None, 0, None, 0) == 0
        assert (out == SENTINEL).all()
        # the device entry point: the same checks, and 16-byte alignment of the input and of the output
        tt = torch.from_numpy(tr).cuda()
        buf = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
        vp = ctypes.c_void_p
        f = L.lt_hip_overlap_tris_device
        for tp, op in ((tt.data_ptr() + 4, buf.data_ptr()), (tt.data_ptr(), buf.data_ptr() + 8), (tt.data_ptr() + 8, buf.data_ptr() + 4)):
            assert f(r._ctx, desc(), vp(tp), 3, vp(op), 128, None) == INVALID
            assert f(r._ctx, desc(COUNT, 0), vp(tp), 3, vp(op), 128, None) == INVALID
            assert f(r._ctx, desc(ANY, 0), vp(tp), 3, vp(op), 128, None) == INVALID
        assert f(r._ctx, desc(), vp(tt.data_ptr()), 4, vp(buf.data_ptr()), 31, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert f(r._ctx, desc(COUNT, 0), vp(tt.data_ptr()), 4, vp(buf.data_ptr()), 15, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert f(r._ctx, desc(flags=2), vp(tt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        assert f(r._ctx, desc(kind=3), vp(tt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        assert f(r._ctx, desc(max_k=9), vp(tt.data_ptr()), 4, vp(buf.data_ptr()), 256, None) == INVALID
        assert f(r._ctx, None, vp(tt.data_ptr()), 4, vp(buf.data_ptr()), 128, None) == INVALID
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
        with pytest.raises(ValueError):
            r.overlap_tris(np.zeros((4, 8), dtype=F32))
        with pytest.raises(ValueError):
            r.overlap_tris(tr, k=9)
        with pytest.raises(ValueError):
            r.overlap_tris(tr, k=2, count=True)
        with pytest.raises(ValueError):
            r.overlap_tris(tr, count=True, any=True)
        with pytest.raises(ValueError):
            r.overlap_tris(tt[:, :8].contiguous())
        # calls that work, on the same context
        m = ot.sequences(s, tr)
        assert m.count[0] > 2
        assert np.array_equal(r.overlap_tris(tr.view(TRI_DTYPE).reshape(-1), k=2), m.first(2))
        assert np.array_equal(r.overlap_tris(tr, count=True), m.count) and (r.overlap_tris(tr, any=True) == 1).all()
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
        tr = np.concatenate(list(ot.families(s, seed=4, n=128).values()))
        m = ot.sequences(s, tr)
        rng = np.random.default_rng(9)
        rays = make_rays(rng.uniform(-5, 5, (512, 3)) + (0, 2.5, -20), rng.normal(0, 0.2, (512, 3)) + (0, 0, 1))
        lo, hi = nr.root_box(s)
        centres = rng.uniform(lo, hi, (256, 3))
        bx = make_boxes(centres - 0.5, centres + 0.5)
        hits_before = r2.trace_rays(rays)
        boxes_before = r2.overlap_boxes(bx, k=8)
        first = r2.overlap_tris(tr, k=8)
        st = r2.stats()
        assert st["rays"] == len(tr) and st["shadow_rays"] == 0 and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
        count = r2.overlap_tris(tr, count=True)
        st = r2.stats()
        assert st["rays"] == len(tr) and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        hit = r2.overlap_tris(tr, any=True)
        assert np.array_equal(first, m.first(8)) and np.array_equal(count, m.count) and np.array_equal(hit, m.any)
        assert np.array_equal(r2.trace_rays(rays).view(np.uint32), hits_before.view(np.uint32))
        assert np.array_equal(r2.overlap_boxes(bx, k=8), boxes_before) and (boxes_before >= 0).sum() >= 64
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # the GPU's answers are the host form's
        for k in KS:
            assert np.array_equal(r2.overlap_tris(tr, k=k), overlap_tris_host(s, tr, k=k)), k
        assert np.array_equal(count, overlap_tris_host(s, tr, count=True)) and np.array_equal(hit, overlap_tris_host(s, tr, any=True))
        assert (m.count > 8).sum() >= 16 and (m.count == 0).sum() >= 128
        # set_scene of another scene right behind an enqueued device call: it keeps the old scene's results
        tt = torch.from_numpy(tr).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        got = r2.overlap_tris(tt, k=3, stream=stream)
        r2.set_scene(base)
        stream.synchronize()
        assert np.array_equal(got.cpu().numpy(), m.first(3))
        tb = ot.families(base, seed=6, n=64)["c_pierce"]
        assert np.array_equal(r2.overlap_tris(tb, k=3), ot.sequences(base, tb).first(3))
    finally:
        r1.close()
        r2.close()
