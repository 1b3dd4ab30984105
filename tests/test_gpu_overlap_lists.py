"""GPU (-m gpu): the overlap lists (lt_hip_overlap_boxes_list, lt_hip_overlap_tris_list and their device entry points: the walks
of lt_overlap.hip and lt_tritri.hip with the sinks kCountWide and kList, the scan and the ordering of lt_overlist.hip).  The
reference throughout is the numpy model of the two queries with every sequence kept whole (tests/overlap_lists.py), never the
code under test; every comparison is of words.  The shapes follow kListScanTile and kListSortSpan as lt_overlist.hpp has them.

1. every box family on the base scene, the 16 x 16 wall, the twelve-triangle fan and the base scene at 2^35, with boxes half
   as wide as the scene and wider added: offsets and items word for word.  From the model alone: >= 64 segments longer than 64
   (where the scene has more than 64 leaves: the fan has twelve, and there >= 64 segments hold all twelve), >= 256 empty
   segments of boxes that are not empty, >= 48 empty boxes.  The same for triangles on the base scene and the fan, with
   triangles through the scene whose edges are 2^20 .. 2^33 scenes long added (their in-plane axes overflow and drop out, so they
   touch by the hundred);
2. sizes 1 .. 2 tile + 1 of a shuffled batch with LT_TRACE_REFILL 1 and 64;
3. segment lengths 0 .. 2 span + 64 on a row of triangles whose offsets are shuffled, in one batch and each alone, and a box of
   +-2^100;
4. scenes without an own tree (the scan kernels; one of them names a primitive in two leaves, so its items repeat) and the
   caller's splits (LT_RETREE=0);
5. the device entry point on a side stream from torch tensors: sizing plus FILL_ONLY equals the one-shot call equals the host
   path, nothing is written behind 8 (n + 1) and 4 total bytes, items one word short stay untouched with the offsets valid,
   FILL_ONLY with halved offsets stays inside its segments;
6. every error writes nothing, on both entry points;
7. calls interleave with trace_rays, a render and a scene change; stats() reports the call."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import (RendererHIP, RenderPropertiesHIP, make_boxes, make_rays, make_tris, overlap_boxes_list_host,
                                     overlap_tris_list_host)
from tests import multihit_edges as me
from tests import nearest as nr
from tests import nearest_k as nk
from tests import overlap as ov
from tests import overlap_lists as ol
from tests import overlap_tris as ot
from tests import query_edges as qe
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
SENTINEL = ol.SENTINEL
FILL = C.OVERLAP_LIST_FLAG_FILL_ONLY
TILE, SPAN = ol.tuning()
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def base():
    return qe.base_scene(0)


def desc(flags=0, size=ctypes.sizeof(C.OverlapListDesc)):
    return ctypes.byref(C.OverlapListDesc(size, flags))


def check(got, want, note):
    (go, gi), (wo, wi) = got, want
    assert go.dtype == np.uint64 and gi.dtype == np.int32 and go.shape == wo.shape, note
    assert np.array_equal(go, wo), (note, np.flatnonzero(go != wo)[:5])
    assert np.array_equal(gi, wi), (note, len(gi), len(wi), np.flatnonzero(gi[:len(wi)] != wi[:len(gi)])[:5])


def prefix(want, n):
    """The lists of the batch's first n queries."""
    wo, wi = want
    return wo[:n + 1], wi[:int(wo[n])]


# ------------------------------------------------------------------------------------------------------------- 1: the model
def scene_of(base, name):
    if name == "base":
        return base
    if name == "wall16":
        return synth.heightfield_wall(16)
    if name == "fan12":
        return nk.fan12()
    return qe.extreme_scene(base, name)[0]


def wide_boxes(s, seed, n=160):
    rng = np.random.default_rng(seed)
    lo, hi = nr.root_box(s)
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    with np.errstate(over="ignore"):
        return ov.centred(c + rng.uniform(-0.5, 0.5, (n, 3)) * half, half * rng.uniform(0.5, 1.0, (n, 3)))


def giant_tris(s, seed, n=192):
    """Triangles round a point of the scene, 2^20 .. 2^33 scenes across."""
    rng = np.random.default_rng(seed)
    lo, hi = nr.root_box(s)
    c, size = 0.5 * (lo + hi), float((hi - lo).max()) * 0.5
    R = size * 2.0 ** rng.integers(20, 34, (n, 1)).astype(np.float64)
    u, v = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3))
    p = c + rng.uniform(-0.5, 0.5, (n, 3)) * size
    return make_tris(p + R * u, p + R * (-0.5 * u + v), p + R * (-0.5 * u - v))


def long_enough(s, count):
    full = ol.leaves(s)
    return (count > 64).sum() >= 64 if full > 64 else (count == full).sum() >= 64


@pytest.mark.parametrize("name", ("base", "wall16", "fan12", "far+"))
def test_boxes_against_the_model(renderer, base, name):
    s = scene_of(base, name)
    bx = np.concatenate(list(ov.families(s, seed=3).values()) + [wide_boxes(s, 4)])
    m = ol.model_boxes(s, bx)
    dead = ov.empty(bx)
    assert long_enough(s, m.count) and ((m.count == 0) & ~dead).sum() >= 256 and dead.sum() >= 48 and (m.count[dead] == 0).all(), name
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check(renderer.overlap_boxes_list(bx), ol.csr(m), name)


@pytest.mark.parametrize("name", ("base", "fan12"))
def test_triangles_against_the_model(renderer, base, name):
    s = scene_of(base, name)
    tr = np.concatenate([t for seed in (3, 4) for t in ot.families(s, seed=seed).values()] + [giant_tris(s, 5)])
    m = ol.model_tris(s, tr)
    dead = ot.empty(tr)
    assert long_enough(s, m.count) and ((m.count == 0) & ~dead).sum() >= 256 and dead.sum() >= 48 and (m.count[dead] == 0).all(), name
    renderer.set_scene(s)
    check(renderer.overlap_tris_list(tr), ol.csr(m), name)


# ------------------------------------------------------------------------------------------------------------- 2: sizes
@pytest.fixture(scope="module")
def shuffled(base):
    n = 2 * TILE + 1
    bx = np.concatenate(list(ov.families(base, seed=5, n=512).values()) + [wide_boxes(base, 6)])
    assert len(bx) >= n
    bx = np.ascontiguousarray(bx[np.random.default_rng(3).permutation(len(bx))][:n])
    tr = np.concatenate(list(ot.families(base, seed=5, n=768).values()) + [giant_tris(base, 6)])
    assert len(tr) >= n
    tr = np.ascontiguousarray(tr[np.random.default_rng(4).permutation(len(tr))][:n])
    return bx, ol.csr(ol.model_boxes(base, bx)), tr, ol.csr(ol.model_tris(base, tr))


SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


@pytest.mark.parametrize("refill", (1, 64))
def test_batch_sizes_and_refill(renderer, base, shuffled, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    bx, want_b, tr, want_t = shuffled
    renderer.set_scene(base)
    for n in SIZES:
        check(renderer.overlap_boxes_list(bx[:n]), prefix(want_b, n), ("boxes", n, refill))
        check(renderer.overlap_tris_list(tr[:n]), prefix(want_t, n), ("tris", n, refill))


# ------------------------------------------------------------------------------------------------------------- 3: segment lengths
@pytest.fixture(scope="module")
def row():
    n = 2 * SPAN + 64
    s, x = ol.row_scene(n, seed=7)
    lengths = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3, n]
    big = np.float32(2.0 ** 100)
    bx = np.concatenate([ol.row_boxes(lengths), make_boxes([[-big] * 3], [[big] * 3])])
    m = ol.model_boxes(s, bx)
    assert m.count.tolist() == lengths + [n]
    # the walk does not meet the offsets in their order: neither the caller's leaves nor the row have them ascending
    off, llo, _ = nr.leaves(s)
    assert (np.diff(off) < 0).sum() > n // 4 and (np.diff(off[np.argsort(llo[:, 0], kind="stable")]) < 0).sum() > n // 4
    return s, bx, ol.csr(m)


def test_segment_lengths_in_one_batch(renderer, row):
    s, bx, want = row
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check(renderer.overlap_boxes_list(bx), want, "row")
    order = np.random.default_rng(1).permutation(len(bx))          # the long segments in other places of the batch
    wo, wi = want
    segs = [wi[int(wo[i]):int(wo[i + 1])] for i in order]
    check(renderer.overlap_boxes_list(np.ascontiguousarray(bx[order])),
          (np.concatenate([[0], np.cumsum([len(g) for g in segs])]).astype(np.uint64), np.concatenate(segs)), "row, permuted")


def test_segment_lengths_each_alone(renderer, row):
    s, bx, (wo, wi) = row
    renderer.set_scene(s)
    for i in range(len(bx)):
        seg = wi[int(wo[i]):int(wo[i + 1])]
        check(renderer.overlap_boxes_list(bx[i:i + 1]), (np.array([0, len(seg)], dtype=np.uint64), seg), ("row", i))
    # a needle along the row is the triangle query's long segment: every triangle it crosses
    tr = make_tris([[-0.5, 0.125, 0.0]], [[2.0 * SPAN + 2.5, 0.125, 0.0]], [[2.0 * SPAN + 2.5, 0.125, 0.0]])
    m = ol.model_tris(s, tr)
    assert m.count[0] > SPAN
    check(renderer.overlap_tris_list(tr), ol.csr(m), "row, needle")


# ------------------------------------------------------------------------------------------------------------- 4: other hierarchies
@pytest.mark.parametrize("name", ("nan_bound", "bound_at_limit", "twice"))
def test_scenes_without_an_own_tree(renderer, base, name):
    s = me.twice_named_scene()[0] if name == "twice" else qe.extreme_scene(base, name)[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    bx = np.concatenate(list(ov.families(s, seed=7, n=96).values()) + [wide_boxes(s, 8, 32)])
    want = ol.csr(ol.model_boxes(s, bx))
    check(renderer.overlap_boxes_list(bx), want, name)
    assert len(want[1]) >= 1024 or name == "twice"
    if name == "twice":     # equal words side by side in a segment
        wo, wi = want
        assert any((np.diff(wi[int(wo[i]):int(wo[i + 1])]) == 0).any() for i in range(len(bx)))
    tr = np.concatenate(list(ot.families(s, seed=7, n=96).values()) + [giant_tris(s, 8, 32)])
    check(renderer.overlap_tris_list(tr), ol.csr(ol.model_tris(s, tr)), name)


def test_the_callers_splits(base, monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(base)
        assert r.stats()["own_tree_height"] > 0
        bx = np.concatenate(list(ov.families(base, seed=9, n=96).values()) + [wide_boxes(base, 10)])
        check(r.overlap_boxes_list(bx), ol.csr(ol.model_boxes(base, bx)), "LT_RETREE=0")
        tr = np.concatenate(list(ot.families(base, seed=9, n=96).values()) + [giant_tris(base, 10, 64)])
        check(r.overlap_tris_list(tr), ol.csr(ol.model_tris(base, tr)), "LT_RETREE=0")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 5: the device entry point
@pytest.mark.parametrize("shape", ("boxes", "tris"))
def test_the_device_entry_point_on_a_side_stream(renderer, base, shuffled, shape):
    import torch
    bx, want_b, tr, want_t = shuffled
    rec, want = (bx, want_b) if shape == "boxes" else (tr, want_t)
    renderer.set_scene(base)
    f = getattr(renderer._L, "lt_hip_overlap_%s_list_device" % shape)
    lists = renderer.overlap_boxes_list if shape == "boxes" else renderer.overlap_tris_list
    side = torch.cuda.Stream()
    for n in (1, 65, TILE + 1):
        wo, wi = prefix(want, n)
        total = len(wi)
        rt = torch.from_numpy(rec[:n]).cuda()
        check(lists(rec[:n]), (wo, wi), (shape, n, "host path"))
        # sizing, one read, FILL_ONLY: the wrapper, on the current stream and on a named one
        with torch.cuda.stream(side):
            go, gi = lists(rt)
        side.synchronize()
        assert go.dtype == torch.int64 and gi.dtype == torch.int32
        check((go.cpu().numpy().view(np.uint64), gi.cpu().numpy()), (wo, wi), (shape, n, "wrapper"))
        go2, gi2 = lists(rt, stream=side)
        side.synchronize()
        assert torch.equal(go2, go) and torch.equal(gi2, gi)

        def raw(flags, offsets, items, items_words):
            rc = f(renderer._ctx, desc(flags), vp(rt.data_ptr()), n, vp(offsets.data_ptr()), 8 * (n + 1),
                   vp(items.data_ptr()) if items is not None else None, 4 * items_words, vp(side.cuda_stream))
            side.synchronize()
            return rc

        def fresh():
            o = torch.full((n + 1 + 16,), SENTINEL, dtype=torch.int64, device="cuda")
            i = torch.full((total + 64,), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            return o, i

        # the one-shot call into sentinel-filled buffers: nothing behind 8 (n + 1) and 4 total bytes
        o, i = fresh()
        assert raw(0, o, i, total) == 0
        oo, ii = o.cpu().numpy().view(np.uint64), i.cpu().numpy()
        check((oo[:n + 1], ii[:total]), (wo, wi), (shape, n, "one-shot"))
        assert (oo[n + 1:] == SENTINEL).all() and (ii[total:] == SENTINEL).all(), (shape, n)
        # the sizing call alone, then FILL_ONLY from its offsets
        o, i = fresh()
        assert raw(0, o, None, 0) == 0
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo) and (o.cpu().numpy()[n + 1:] == SENTINEL).all()
        assert raw(FILL, o, i, total) == 0
        ii = i.cpu().numpy()
        assert np.array_equal(ii[:total], wi) and (ii[total:] == SENTINEL).all(), (shape, n)
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo)
        if total == 0:
            continue
        # one word short: items untouched, offsets valid
        o, i = fresh()
        assert raw(0, o, i, total - 1) == 0
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo) and (i.cpu().numpy() == SENTINEL).all(), (shape, n)
        # FILL_ONLY with halved offsets (never larger than the true ones) on items of the true size: each query writes the
        # head of its sequence into its halved segment, in order; nothing else is written
        half = wo // np.uint64(2)
        o, i = fresh()
        o[:n + 1] = torch.from_numpy(half.view(np.int64)).cuda()
        torch.cuda.synchronize()
        assert raw(FILL, o, i, total) == 0
        ii = i.cpu().numpy()
        assert (ii[int(half[n]):] == SENTINEL).all(), (shape, n)
        for q in range(n):
            b, e = int(half[q]), int(half[q + 1])
            seq = wi[int(wo[q]):int(wo[q + 1])]
            # (the segment holds e - b of the sequence's words -- the first that the walk met -- sorted)
            assert np.isin(ii[b:e], seq).all() and (np.diff(ii[b:e]) >= 0).all(), (shape, n, q)


# ------------------------------------------------------------------------------------------------------------- 6: errors
def test_every_error_leaves_the_buffers_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        bx = make_boxes(np.full((4, 3), -100.0), np.full((4, 3), 100.0))
        tr = make_tris(np.full((4, 3), -100.0), np.full((4, 3), 100.0), np.array([[100.0, -100.0, 0.0]] * 4))
        offsets = np.full(8, SENTINEL, dtype=np.uint64)
        items = np.full(256, SENTINEL, dtype=np.int32)
        O, I = offsets.ctypes.data_as(vp), items.ctypes.data_as(vp)
        INVALID, SMALL = C.LT_ERR_INVALID_ARGUMENT, C.LT_ERR_BUFFER_TOO_SMALL
        for shape, rec in (("boxes", bx), ("tris", tr)):
            assert getattr(L, "lt_hip_overlap_%s_list" % shape)(r._ctx, desc(), rec.ctypes.data_as(vp), 4, O, 40, I, 1024) == C.LT_ERR_NO_SCENE
        assert (offsets == SENTINEL).all() and (items == SENTINEL).all()
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        for shape, rec in (("boxes", bx), ("tris", tr)):
            f = getattr(L, "lt_hip_overlap_%s_list" % shape)
            R = rec.ctypes.data_as(vp)
            cases = [
                (None, R, 4, O, 40, I, 1024, INVALID),
                (desc(size=4), R, 4, O, 40, I, 1024, INVALID),
                (desc(flags=2), R, 4, O, 40, I, 1024, INVALID),
                (desc(flags=FILL | 0x100), R, 4, O, 40, I, 1024, INVALID),
                (desc(), R, 2 ** 32, O, 40, I, 1024, INVALID),
                (desc(), None, 4, O, 40, I, 1024, INVALID),
                (desc(), R, 4, None, 40, I, 1024, INVALID),
                (desc(), R, 4, O, 40, None, 1024, INVALID),
                (desc(FILL), R, 4, O, 40, None, 0, INVALID),
                (desc(), R, 4, O, 39, I, 1024, SMALL),
                (desc(FILL), R, 4, O, 39, I, 1024, SMALL),
                (desc(), R, 4, O, 39, None, 0, SMALL),
                (desc(flags=4), R, 4, O, 0, I, 0, INVALID),          # an unknown flag comes before the buffers' sizes
            ]
            for i, (*args, want) in enumerate(cases):
                assert f(r._ctx, *args) == want, (shape, i)
                assert (offsets == SENTINEL).all() and (items == SENTINEL).all(), (shape, i)
            assert f(r._ctx, desc(FILL), None, 0, O, 8, I, 1024) == 0 and (offsets == SENTINEL).all() and (items == SENTINEL).all()
            assert f(r._ctx, desc(), None, 0, O, 8, None, 0) == 0 and offsets[0] == 0 and (offsets[1:] == SENTINEL).all()
            offsets[:] = SENTINEL
            # the device entry point: the same checks, and 16-byte alignment
            rt = torch.from_numpy(rec).cuda()
            ot_ = torch.full((16,), SENTINEL, dtype=torch.int64, device="cuda")
            it = torch.full((256,), SENTINEL, dtype=torch.int32, device="cuda")
            g = getattr(L, "lt_hip_overlap_%s_list_device" % shape)
            rp, op, ip = rt.data_ptr(), ot_.data_ptr(), it.data_ptr()
            for a, b, c in ((rp + 4, op, ip), (rp, op + 8, ip), (rp, op, ip + 4)):
                assert g(r._ctx, desc(), vp(a), 3, vp(b), 64, vp(c), 512, None) == INVALID
                assert g(r._ctx, desc(FILL), vp(a), 3, vp(b), 64, vp(c), 512, None) == INVALID
            assert g(r._ctx, desc(), vp(rp), 4, vp(op), 39, vp(ip), 1024, None) == SMALL
            assert g(r._ctx, desc(flags=2), vp(rp), 4, vp(op), 40, vp(ip), 1024, None) == INVALID
            assert g(r._ctx, None, vp(rp), 4, vp(op), 40, vp(ip), 1024, None) == INVALID
            assert g(r._ctx, desc(), vp(rp), 4, vp(op), 40, None, 4, None) == INVALID
            assert g(r._ctx, desc(FILL), vp(rp), 4, vp(op), 40, None, 0, None) == INVALID
            assert g(r._ctx, desc(), vp(rp), 2 ** 32, vp(op), 40, vp(ip), 1024, None) == INVALID
            torch.cuda.synchronize()
            assert (ot_.cpu().numpy() == SENTINEL).all() and (it.cpu().numpy() == SENTINEL).all()
            # the host entry point: items too small are LT_ERR_BUFFER_TOO_SMALL, with the offsets written and items untouched
            count = (r.overlap_boxes if shape == "boxes" else r.overlap_tris)(rec, count=True)
            total = int(count.sum())
            assert 4 <= total <= 256
            assert f(r._ctx, desc(), R, 4, O, 40, I, 4 * (total - 1)) == SMALL
            assert np.array_equal(np.diff(offsets[:5]), count) and (offsets[5:] == SENTINEL).all() and (items == SENTINEL).all()
            offsets[:] = SENTINEL
        with pytest.raises(ValueError):
            r.overlap_boxes_list(np.zeros((4, 6), dtype=np.float32))
        with pytest.raises(ValueError):
            r.overlap_tris_list(torch.zeros((4, 8), device="cuda"))
        with pytest.raises(TypeError):
            r.overlap_boxes_list([[0.0] * 8])
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
        a1, _ = render(r1)
        b1, t1 = render(r1)
        a2, _ = render(r2)
        bx = np.concatenate(list(ov.families(s, seed=4, n=128).values()))
        tr = np.concatenate(list(ot.families(s, seed=4, n=128).values()))
        want_b, want_t = ol.csr(ol.model_boxes(s, bx)), ol.csr(ol.model_tris(s, tr))
        rng = np.random.default_rng(9)
        rays = make_rays(rng.uniform(-5, 5, (512, 3)) + (0, 2.5, -20), rng.normal(0, 0.2, (512, 3)) + (0, 0, 1))
        hits_before = r2.trace_rays(rays)
        # the raw host calls: sizing 4 kernels, FILL_ONLY 2, both 6
        offsets = np.zeros(len(bx) + 1, dtype=np.uint64)
        items = np.zeros(len(want_b[1]), dtype=np.int32)
        f = r2._L.lt_hip_overlap_boxes_list
        for flags, it, launches in ((0, None, 4), (FILL, items, 2), (0, items, 6)):
            r2._check(f(r2._ctx, desc(flags), bx.ctypes.data_as(vp), len(bx), offsets.ctypes.data_as(vp), offsets.nbytes,
                        None if it is None else it.ctypes.data_as(vp), 0 if it is None else it.nbytes))
            st = r2.stats()
            assert st["rays"] == len(bx) and st["shadow_rays"] == 0 and st["kernel_launches"] == launches and st["kernel_ms"] > 0, (flags, st)
            assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
            check((offsets, items) if it is not None else (offsets, want_b[1]), want_b, flags)
        check(r2.overlap_tris_list(tr), want_t, "tris")
        assert r2.stats()["rays"] == len(tr) and r2.stats()["kernel_launches"] == 2
        assert np.array_equal(r2.overlap_boxes(bx, count=True).astype(np.uint64), np.diff(want_b[0]))
        assert np.array_equal(r2.trace_rays(rays).view(np.uint32), hits_before.view(np.uint32))
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # the GPU's lists are the host forms'
        check(r2.overlap_boxes_list(bx), overlap_boxes_list_host(s, bx), "host form")
        check(r2.overlap_tris_list(tr), overlap_tris_list_host(s, tr), "host form")
        # set_scene of another scene right behind an enqueued one-shot device call: it keeps the old scene's lists
        bt = torch.from_numpy(bx).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        od = torch.zeros(len(bx) + 1, dtype=torch.int64, device="cuda")
        idev = torch.zeros(len(want_b[1]), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r2._check(r2._L.lt_hip_overlap_boxes_list_device(r2._ctx, desc(), vp(bt.data_ptr()), len(bx), vp(od.data_ptr()), 8 * (len(bx) + 1),
                                                          vp(idev.data_ptr()), 4 * len(idev), vp(stream.cuda_stream)))
        r2.set_scene(base)
        stream.synchronize()
        check((od.cpu().numpy().view(np.uint64), idev.cpu().numpy()), want_b, "behind set_scene")
        bb = ov.families(base, seed=6, n=64)["b_on"]
        check(r2.overlap_boxes_list(bb), ol.csr(ol.model_boxes(base, bb)), "the new scene")
    finally:
        r1.close()
        r2.close()
