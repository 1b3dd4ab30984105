"""GPU (-m gpu): the radius lists (lt_hip_nearest_list and its device entry point: lt_nearest_k_kernel with the sinks kCountWide
and kList, the scan and the record ordering of lt_overlist.hip).  The reference throughout is the numpy model of the k-nearest
query with every sequence kept whole (tests/nearest_lists.py), never the code under test; every comparison is of bits.  The
shapes follow kListScanTile and kListSortSpanHits as lt_overlist.hpp has them.

1. every point family on the base scene, the 16 x 16 wall, the twelve-triangle fan and the base scene at 2^35, with 160 points in
   the root box whose radius is 0.25 .. 1.0 of its half-diagonal added: offsets and records bit for bit.  From the model alone:
   >= 64 segments longer than 64 (the fan: >= 64 segments that hold all twelve), >= 256 empty segments of points that do walk,
   >= 48 points that take no walk, >= 64 segments with two adjacent equal d2;
2. sizes 1 .. 2 tile + 1 of a shuffled batch with LT_TRACE_REFILL 1 and 64;
3. segment lengths 0 .. 2 span + 64 on a row of triangles whose offsets are shuffled, in one batch, permuted and each alone; a
   fan of 2 span + 64 triangles whose vertex has them all at d2 == +0 (the offset alone orders a segment longer than the LDS
   span); one point with max_d2 = inf on a scene whose group tree is at least four levels high;
4. scenes without an own tree (the scan path; one of them names a primitive in two leaves, so its records repeat) and the
   caller's splits (LT_RETREE=0);
5. the device entry point on a side stream from torch tensors: sizing plus FILL_ONLY equals the one-shot call equals the host
   path, nothing is written behind 8 (n + 1) and 16 total bytes, items one record short stay untouched with the offsets valid,
   FILL_ONLY with halved offsets stays inside its segments;
6. every error writes nothing, on both entry points;
7. calls interleave with trace_rays, a render and a scene change; stats() reports the call; the counts, the first eight and
   surface_at agree with the calls that exist."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import HIT_DTYPE, RendererHIP, RenderPropertiesHIP, make_points, make_rays, nearest_list_host
from tests import multihit_edges as me
from tests import nearest as nr
from tests import nearest_k as nk
from tests import nearest_lists as nl
from tests import overlap_lists as ol
from tests import query_edges as qe
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
SENTINEL = nl.SENTINEL
FILL = C.NEAREST_LIST_FLAG_FILL_ONLY
TILE, SPAN = nl.tuning()
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def base():
    return qe.base_scene(0)


def desc(flags=0, size=ctypes.sizeof(C.NearestListDesc)):
    return ctypes.byref(C.NearestListDesc(size, flags))


def check(got, want, note):
    why = nl.differ(got, want)
    assert why is None, (note, why)


def prefix(want, n):
    """The lists of the batch's first n points."""
    wo, wi = want
    return wo[:n + 1], wi[:int(wo[n])]


def records(t):
    """A (total, 4) float32 tensor, or its numpy copy, as HIT_DTYPE records."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return np.ascontiguousarray(a).view(HIT_DTYPE).reshape(-1)


# ------------------------------------------------------------------------------------------------------------- 1: the model
def scene_of(base, name):
    if name == "base":
        return base
    if name == "wall16":
        return synth.heightfield_wall(16)
    if name == "fan12":
        return nk.fan12()
    return qe.extreme_scene(base, name)[0]


def wide_points(s, seed, n=160):
    """Points in the root box whose radius is 0.25 .. 1.0 of the box's half-diagonal."""
    rng = np.random.default_rng(seed)
    lo, hi = nr.root_box(s)
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    radius = rng.uniform(0.25, 1.0, n) * float(np.sqrt((half * half).sum()))
    return make_points(c + rng.uniform(-1.0, 1.0, (n, 3)) * half, (radius * radius).astype(np.float32))


@pytest.mark.parametrize("name", ("base", "wall16", "fan12", "far+"))
def test_against_the_model(renderer, base, name):
    s = scene_of(base, name)
    pts = np.concatenate(list(nk.families(s, seed=3).values()) + [wide_points(s, 4)])
    m = nl.model(s, pts)
    want = nl.csr(m)
    full = nl.leaves(s)
    dead = nr.no_walk(pts)
    assert ((m.count > 64).sum() >= 64 if full > 64 else (m.count == full).sum() >= 64), name
    assert ((m.count == 0) & ~dead).sum() >= 256 and dead.sum() >= 48 and (m.count[dead] == 0).all(), name
    assert sum((np.diff(g["t"]) == 0).any() for g in nl.segments(want)) >= 64, name
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check(renderer.nearest_list(pts), want, name)


# ------------------------------------------------------------------------------------------------------------- 2: sizes
@pytest.fixture(scope="module")
def shuffled(base):
    n = 2 * TILE + 1
    pts = np.concatenate(list(nk.families(base, seed=5, n=640).values()) + [wide_points(base, 6, 16)])
    assert len(pts) >= n
    pts = np.ascontiguousarray(pts[np.random.default_rng(3).permutation(len(pts))][:n])
    return pts, nl.csr(nl.model(base, pts))


SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


@pytest.mark.parametrize("refill", (1, 64))
def test_batch_sizes_and_refill(renderer, base, shuffled, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    pts, want = shuffled
    renderer.set_scene(base)
    for n in SIZES:
        check(renderer.nearest_list(pts[:n]), prefix(want, n), (n, refill))


# ------------------------------------------------------------------------------------------------------------- 3: segment lengths
@pytest.fixture(scope="module")
def row():
    n = 2 * SPAN + 64
    s, x = ol.row_scene(n, seed=7)
    lengths = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3, n]
    pts = nl.row_points(lengths)
    m = nl.model(s, pts, chunk=4)
    assert m.count.tolist() == lengths
    # the walk does not meet the offsets in their order: neither the caller's leaves nor the row have them ascending
    off, llo, _ = nr.leaves(s)
    assert (np.diff(off) < 0).sum() > n // 4 and (np.diff(off[np.argsort(llo[:, 0], kind="stable")]) < 0).sum() > n // 4
    return s, pts, nl.csr(m)


def test_segment_lengths_in_one_batch(renderer, row):
    s, pts, want = row
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check(renderer.nearest_list(pts), want, "row")
    order = np.random.default_rng(1).permutation(len(pts))          # the long segments in other places of the batch
    check(renderer.nearest_list(np.ascontiguousarray(pts[order])), nl.gather(want, order), "row, permuted")


def test_segment_lengths_each_alone(renderer, row):
    s, pts, want = row
    renderer.set_scene(s)
    for i in range(len(pts)):
        check(renderer.nearest_list(pts[i:i + 1]), nl.gather(want, [i]), ("row", i))


def test_a_segment_of_equal_d2_longer_than_the_span(renderer):
    F = 2 * SPAN + 64
    s = nl.fan(F)
    V = nl.FAN_VERTEX
    rng = np.random.default_rng(2)
    near = V + rng.uniform(-0.25, 0.25, (13, 3)).astype(np.float32)
    # (every triangle holds V, so a point near V is at most |P - V| from each: radii of 0.3 .. 1.0 of that give partial segments)
    part = (np.linspace(0.3, 1.0, 13) * ((near - V) ** 2).sum(axis=1)).astype(np.float32)
    pts = make_points(np.concatenate([[V, V, V], near]), np.concatenate([np.float32([2.0 ** -20, 1.0, np.inf]), part]))
    m = nl.model(s, pts, chunk=4)
    want = nl.csr(m)
    seg = nl.segments(want)
    # at V with a small radius: every triangle at d2 == +0, so the offset key alone orders a segment longer than the LDS span
    assert len(seg[0]) == F > SPAN and (seg[0]["t"].view(np.uint32) == 0).all() and np.array_equal(seg[0]["prim"], np.arange(F))
    assert len(seg[2]) == F and ((m.count[3:] > 64) & (m.count[3:] < SPAN)).sum() >= 4 and ((m.count[3:] > SPAN) & (m.count[3:] < F)).any()
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check(renderer.nearest_list(pts), want, "fan")
    check(renderer.nearest_list(pts[:1]), nl.gather(want, [0]), "fan, the vertex alone")


def test_every_leaf_in_one_segment(renderer, row):
    s = row[0]
    renderer.set_scene(s)
    height, own, _ = C.own_hierarchy(s.node_view, len(s.prim_view))
    assert renderer.stats()["own_tree_height"] == height and C.own_wide(own, len(s.prim_view))[0] >= 4      # the group tree's height
    pts = make_points([[700.25, 0.5, 0.25]], np.inf)
    m = nl.model(s, pts, chunk=1)
    assert m.count[0] == nl.leaves(s) == 2 * SPAN + 64
    check(renderer.nearest_list(pts), nl.csr(m), "inf")


# ------------------------------------------------------------------------------------------------------------- 4: other hierarchies
@pytest.mark.parametrize("name", ("nan_bound", "bound_at_limit", "twice"))
def test_scenes_without_an_own_tree(renderer, base, name):
    s = me.twice_named_scene()[0] if name == "twice" else qe.extreme_scene(base, name)[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    pts = np.concatenate(list(nk.families(s, seed=7, n=96).values()) + [wide_points(s, 8, 32)])
    want = nl.csr(nl.model(s, pts))
    assert len(want[1]) >= 1024
    if name == "twice":     # equal records side by side in a segment
        assert sum(int(((g["prim"][1:] == g["prim"][:-1]) & (g["t"][1:] == g["t"][:-1])).sum()) for g in nl.segments(want)) >= 64
    check(renderer.nearest_list(pts), want, name)


def test_the_callers_splits(base, monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(base)
        assert r.stats()["own_tree_height"] > 0
        pts = np.concatenate(list(nk.families(base, seed=9, n=96).values()) + [wide_points(base, 10, 64)])
        check(r.nearest_list(pts), nl.csr(nl.model(base, pts)), "LT_RETREE=0")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 5: the device entry point
def test_the_device_entry_point_on_a_side_stream(renderer, base, shuffled):
    import torch
    pts, want = shuffled
    renderer.set_scene(base)
    f = renderer._L.lt_hip_nearest_list_device
    side = torch.cuda.Stream()
    for n in (1, 65, TILE + 1):
        wo, wi = prefix(want, n)
        total = len(wi)
        pt = torch.from_numpy(pts[:n]).cuda()
        check(renderer.nearest_list(pts[:n]), (wo, wi), (n, "host path"))
        # sizing, one read, FILL_ONLY: the wrapper, on the current stream and on a named one
        with torch.cuda.stream(side):
            go, gi = renderer.nearest_list(pt)
        side.synchronize()
        assert go.dtype == torch.int64 and gi.dtype == torch.float32 and tuple(gi.shape) == (total, 4)
        check((go.cpu().numpy().view(np.uint64), records(gi)), (wo, wi), (n, "wrapper"))
        go2, gi2 = renderer.nearest_list(pt, stream=side)
        side.synchronize()
        assert torch.equal(go2, go) and torch.equal(gi2.view(torch.int32), gi.view(torch.int32))
        # (n, 3) positions with max_d2 apart: the same records
        go3, gi3 = renderer.nearest_list(pt[:, 0:3].contiguous(), max_d2=pt[:, 3].contiguous(), stream=side)
        side.synchronize()
        assert torch.equal(go3, go) and torch.equal(gi3.view(torch.int32), gi.view(torch.int32))

        def raw(flags, offsets, items, items_records):
            rc = f(renderer._ctx, desc(flags), vp(pt.data_ptr()), n, vp(offsets.data_ptr()), 8 * (n + 1),
                   vp(items.data_ptr()) if items is not None else None, 16 * items_records, vp(side.cuda_stream))
            side.synchronize()
            return rc

        def fresh():
            o = torch.full((n + 1 + 16,), SENTINEL, dtype=torch.int64, device="cuda")
            i = torch.full((total + 64, 4), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            return o, i

        # the one-shot call into sentinel-filled buffers: nothing behind 8 (n + 1) and 16 total bytes
        o, i = fresh()
        assert raw(0, o, i, total) == 0
        oo, ii = o.cpu().numpy().view(np.uint64), i.cpu().numpy()
        check((oo[:n + 1], records(ii[:total])), (wo, wi), (n, "one-shot"))
        assert (oo[n + 1:] == SENTINEL).all() and (ii[total:] == SENTINEL).all(), n
        # the sizing call alone, then FILL_ONLY from its offsets
        o, i = fresh()
        assert raw(0, o, None, 0) == 0
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo) and (o.cpu().numpy()[n + 1:] == SENTINEL).all()
        assert raw(FILL, o, i, total) == 0
        ii = i.cpu().numpy()
        assert len(nr.same(records(ii[:total]), wi)) == 0 and (ii[total:] == SENTINEL).all(), n
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo)
        if total == 0:
            continue
        # one record short: items untouched, offsets valid
        o, i = fresh()
        assert raw(0, o, i, total - 1) == 0
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo) and (i.cpu().numpy() == SENTINEL).all(), n
        # FILL_ONLY with halved offsets (never larger than the true ones) on items of the true size: each point writes records
        # of its own sequence into its halved segment, sorted by (d2, prim); nothing else is written
        half = wo // np.uint64(2)
        o, i = fresh()
        o[:n + 1] = torch.from_numpy(half.view(np.int64)).cuda()
        torch.cuda.synchronize()
        assert raw(FILL, o, i, total) == 0
        ii = i.cpu().numpy()
        assert (ii[int(half[n]):] == SENTINEL).all(), n
        for q in range(n):
            b, e = int(half[q]), int(half[q + 1])
            seq = {r.tobytes() for r in wi[int(wo[q]):int(wo[q + 1])]}
            got = records(ii[b:e])
            # (the segment holds e - b of the sequence's records -- the first that the walk met -- sorted)
            assert all(r.tobytes() in seq for r in got) and nl.sorted_by_d2_and_prim(got), (n, q)


# ------------------------------------------------------------------------------------------------------------- 6: errors
def test_every_error_leaves_the_buffers_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        pts = make_points(np.array([[0.0, 2.5, 0.0]] * 4), 9.0)
        offsets = np.full(8, SENTINEL, dtype=np.uint64)
        items = np.full(4 * 256, SENTINEL, dtype=np.uint32).view(HIT_DTYPE)

        def clean():
            return bool((offsets == SENTINEL).all() and (items.view(np.uint32) == SENTINEL).all())

        O, I, R = offsets.ctypes.data_as(vp), items.ctypes.data_as(vp), pts.ctypes.data_as(vp)
        INVALID, SMALL = C.LT_ERR_INVALID_ARGUMENT, C.LT_ERR_BUFFER_TOO_SMALL
        f = L.lt_hip_nearest_list
        assert f(r._ctx, desc(), R, 4, O, 40, I, 4096) == C.LT_ERR_NO_SCENE and clean()
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        cases = [
            (None, R, 4, O, 40, I, 4096, INVALID),
            (desc(size=4), R, 4, O, 40, I, 4096, INVALID),
            (desc(flags=2), R, 4, O, 40, I, 4096, INVALID),
            (desc(flags=FILL | 0x100), R, 4, O, 40, I, 4096, INVALID),
            (desc(), R, 2 ** 32, O, 40, I, 4096, INVALID),
            (desc(), None, 4, O, 40, I, 4096, INVALID),
            (desc(), R, 4, None, 40, I, 4096, INVALID),
            (desc(), R, 4, O, 40, None, 4096, INVALID),
            (desc(FILL), R, 4, O, 40, None, 0, INVALID),
            (desc(), R, 4, O, 39, I, 4096, SMALL),
            (desc(FILL), R, 4, O, 39, I, 4096, SMALL),
            (desc(), R, 4, O, 39, None, 0, SMALL),
            (desc(flags=4), R, 4, O, 0, I, 0, INVALID),          # an unknown flag comes before the buffers' sizes
        ]
        for i, (*args, want) in enumerate(cases):
            assert f(r._ctx, *args) == want, i
            assert clean(), i
        assert f(r._ctx, desc(FILL), None, 0, O, 8, I, 4096) == 0 and clean()
        assert f(r._ctx, desc(), None, 0, O, 8, None, 0) == 0 and offsets[0] == 0 and (offsets[1:] == SENTINEL).all()
        offsets[:] = SENTINEL
        # the device entry point: the same checks, and 16-byte alignment
        pt = torch.from_numpy(pts).cuda()
        ot_ = torch.full((16,), SENTINEL, dtype=torch.int64, device="cuda")
        it = torch.full((256, 4), SENTINEL, dtype=torch.int32, device="cuda")
        g = L.lt_hip_nearest_list_device
        rp, op, ip = pt.data_ptr(), ot_.data_ptr(), it.data_ptr()
        for a, b, c in ((rp + 4, op, ip), (rp, op + 8, ip), (rp, op, ip + 4), (rp, op, ip + 8)):
            assert g(r._ctx, desc(), vp(a), 3, vp(b), 64, vp(c), 2048, None) == INVALID
            assert g(r._ctx, desc(FILL), vp(a), 3, vp(b), 64, vp(c), 2048, None) == INVALID
        assert g(r._ctx, desc(), vp(rp), 4, vp(op), 39, vp(ip), 4096, None) == SMALL
        assert g(r._ctx, desc(flags=2), vp(rp), 4, vp(op), 40, vp(ip), 4096, None) == INVALID
        assert g(r._ctx, None, vp(rp), 4, vp(op), 40, vp(ip), 4096, None) == INVALID
        assert g(r._ctx, desc(), vp(rp), 4, vp(op), 40, None, 16, None) == INVALID
        assert g(r._ctx, desc(FILL), vp(rp), 4, vp(op), 40, None, 0, None) == INVALID
        assert g(r._ctx, desc(), vp(rp), 2 ** 32, vp(op), 40, vp(ip), 4096, None) == INVALID
        torch.cuda.synchronize()
        assert (ot_.cpu().numpy() == SENTINEL).all() and (it.cpu().numpy() == SENTINEL).all()
        # the host entry point: items too small are LT_ERR_BUFFER_TOO_SMALL, with the offsets written and items untouched
        count = r.nearest_k(pts, count=True)
        total = int(count.sum())
        assert 4 <= total <= 256
        assert f(r._ctx, desc(), R, 4, O, 40, I, 16 * (total - 1)) == SMALL
        assert np.array_equal(np.diff(offsets[:5]), count) and (offsets[5:] == SENTINEL).all() and (items.view(np.uint32) == SENTINEL).all()
        with pytest.raises(ValueError):
            r.nearest_list(np.zeros((4, 6), dtype=np.float32))
        with pytest.raises(ValueError):
            r.nearest_list(torch.zeros((4, 8), device="cuda"))
        with pytest.raises(TypeError):
            r.nearest_list([[0.0] * 4])
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
        pts = np.concatenate(list(nk.families(s, seed=4, n=128).values()))
        m = nl.model(s, pts)
        want = nl.csr(m)
        assert (m.count > 8).sum() >= 64
        rng = np.random.default_rng(9)
        rays = make_rays(rng.uniform(-5, 5, (512, 3)) + (0, 2.5, -20), rng.normal(0, 0.2, (512, 3)) + (0, 0, 1))
        hits_before = r2.trace_rays(rays)
        # the raw host calls: sizing 4 kernels, FILL_ONLY 2, both 6
        offsets = np.zeros(len(pts) + 1, dtype=np.uint64)
        items = np.zeros(len(want[1]), dtype=HIT_DTYPE)
        f = r2._L.lt_hip_nearest_list
        for flags, it, launches in ((0, None, 4), (FILL, items, 2), (0, items, 6)):
            items[:] = 0
            r2._check(f(r2._ctx, desc(flags), pts.ctypes.data_as(vp), len(pts), offsets.ctypes.data_as(vp), offsets.nbytes,
                        None if it is None else it.ctypes.data_as(vp), 0 if it is None else it.nbytes))
            st = r2.stats()
            assert st["rays"] == len(pts) and st["shadow_rays"] == 0 and st["kernel_launches"] == launches and st["kernel_ms"] > 0, (flags, st)
            assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
            check((offsets, items) if it is not None else (offsets, want[1]), want, flags)
        assert np.array_equal(r2.nearest_k(pts, count=True).astype(np.uint64), np.diff(want[0]))
        k8 = r2.nearest_k(pts, k=8)
        for i, g in enumerate(nl.segments(want)):
            real = k8[i][k8[i]["prim"] >= 0]
            assert len(real) == min(8, len(g)) and len(nr.same(real, g[:8])) == 0, i
        got = r2.nearest_list(pts)
        check(got, want, "wrapper")
        assert len(nr.same(r2.surface_at(got[1]).view(np.uint32).reshape(-1, 4), r2.surface_at(want[1]).view(np.uint32).reshape(-1, 4))) == 0
        assert np.array_equal(r2.trace_rays(rays).view(np.uint32), hits_before.view(np.uint32))
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # the GPU's lists are the host form's
        check(r2.nearest_list(pts), nearest_list_host(s, pts), "host form")
        # set_scene of another scene right behind an enqueued one-shot device call: it keeps the old scene's lists
        pt = torch.from_numpy(pts).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        od = torch.zeros(len(pts) + 1, dtype=torch.int64, device="cuda")
        idev = torch.zeros((len(want[1]), 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r2._check(r2._L.lt_hip_nearest_list_device(r2._ctx, desc(), vp(pt.data_ptr()), len(pts), vp(od.data_ptr()), 8 * (len(pts) + 1),
                                                    vp(idev.data_ptr()), 16 * len(idev), vp(stream.cuda_stream)))
        r2.set_scene(base)
        stream.synchronize()
        check((od.cpu().numpy().view(np.uint64), records(idev)), want, "behind set_scene")
        pb = nk.families(base, seed=6, n=64)["a_uniform"]
        check(r2.nearest_list(pb), nl.csr(nl.model(base, pb)), "the new scene")
    finally:
        r1.close()
        r2.close()
