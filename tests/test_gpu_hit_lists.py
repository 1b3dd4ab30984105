"""GPU (-m gpu): the hit lists (lt_hip_trace_hits_list and its device entry point: lt_query_hits_kernel with the sinks kCountWide
and kList, the scan, and lt_list_order_kernel with the rays' rank order -- lt_query.hip, lt_overlist.hip).  The reference is the
peeling oracle (tests/multihit.py) or, for the identities, the calls that existed before; every comparison is of offsets and of
all four fields of every record, bit for bit.  Fixtures: tests/hit_lists.py, whose claims tests/test_hit_lists_cpu.py checks.

1. the portable flavour against the oracle: the 12 sheets and the Cornell box under the three epsilon programs; the scene that
   names a primitive twice, whose lists without their repeats are the peel sequences;
2. the identities in the three flavours -- the differences of the offsets are LT_TRACE_COUNT's words, the first eight records of a
   segment LT_TRACE_FIRST_K's real records at K = 8 and the other slots misses -- on those batches and on query_edges' families
   (octants, per-lane tmax, ignoring lanes, partial chunks, packet_ray_ok's limits: rays of one batch take different walks);
3. the 768 tie rays: 2 .. 12 triangles at one t in every octant, at +-0 too -- only rank8 orders them;
4. segment lengths 0 .. 2 span + 64 on the stack, in one batch, permuted, and each alone: the LDS sort and the in-place sort, short
   and long segments in neighbouring lanes, two waves;
5. scenes without an own tree (every ray keeps its segment sorted as it fills it; the sheets' duplicate gives bit-equal t at
   positions 2 and 3) and the caller's splits (LT_RETREE=0);
6. the contract: sizing, items one record short in both forms, FILL_ONLY from returned offsets and from offsets that are no scan
   at all, every argument error, n == 0, a side stream, calls between renders, set_scene behind an enqueued call, the statistics,
   LT_TRACE_REFILL 1 and 64."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import HIT_DTYPE, RendererHIP, RenderPropertiesHIP, make_rays
from oracle import pyoracle as po
from tests import hit_lists as hl
from tests import multihit as mh
from tests import multihit_edges as me
from tests import query_edges as qe
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
SENTINEL = hl.SENTINEL
FILL = C.TRACE_LIST_FLAG_FILL_ONLY
PORTABLE = C.RENDER_FLAG_PORTABLE_MATH
EPS_PROGRAMS = (C.PROGRAM_BASIC, C.PROGRAM_BASIC_LIGHTING, C.PROGRAM_ACCUMULATOR)
FLAVOURS = ({}, {"strict_math": True}, {"portable_math": True})
TILE, SPAN = hl.tuning()
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


def desc(flags=0, program=C.PROGRAM_ACCUMULATOR, size=ctypes.sizeof(C.HitsListDesc), reserved=0):
    return ctypes.byref(C.HitsListDesc(size, program, flags, reserved))


def check(got, want, note):
    why = hl.differ(got, want)
    assert why is None, (note, why)


def records(t):
    """A (total, 4) float32 or int32 tensor, or its numpy copy, as HIT_DTYPE records."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return np.ascontiguousarray(a).view(HIT_DTYPE).reshape(-1)


def first_eight(lists, rays):
    """What LT_TRACE_FIRST_K at K = 8 must hold given these lists: a segment's first eight records, then misses {tmax, -1, 0, 0}."""
    out = np.zeros((len(rays), 8), dtype=HIT_DTYPE)
    out["t"] = rays[:, 3:4]
    out["prim"] = -1
    for i, g in enumerate(hl.segments(lists)):
        out[i, :min(8, len(g))] = g[:8]
    return out


def identities(r, rays, note, program=C.PROGRAM_ACCUMULATOR, **flavour):
    got = r.trace_hits_list(rays, program=program, **flavour)
    offsets, items = got
    assert offsets.dtype == np.uint64 and offsets.shape == (len(rays) + 1,) and items.dtype == HIT_DTYPE and offsets[0] == 0
    assert len(items) == int(offsets[-1]), note
    n = r.trace_hits(rays, count=True, program=program, **flavour)
    bad = np.flatnonzero(np.diff(offsets) != n)
    assert len(bad) == 0, (note, len(bad), bad[:5], np.diff(offsets)[bad[:5]], n[bad[:5]])
    k8 = r.trace_hits(rays, max_hits=8, program=program, **flavour)
    bad = mh.same_records(first_eight(got, rays), k8)
    assert len(bad) == 0, (note, len(bad), bad[:5], hl.segments(got)[bad[0]][:8], k8[bad[0]])
    return got


# ------------------------------------------------------------------------------------------------------------- 1: the oracle
@pytest.mark.parametrize("prog", EPS_PROGRAMS)
@pytest.mark.parametrize("name", ["sheets", "cornell"])
def test_portable_flavour_equals_the_peeling_oracle(renderer, name, prog):
    s, rays = hl.batch(name)
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    want = hl.csr(hl.sequences(name, prog))
    print(name, prog, "rays", len(rays), "records", len(want[1]), "longest", int(np.diff(want[0]).max()))
    check(renderer.trace_hits_list(rays, program=prog, portable_math=True), want, (name, prog))


def test_leaves_that_name_one_primitive_twice(renderer):
    s = me.twice_named_scene()[0]
    rays = mh.sheet_rays()[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    seqs = mh.sequences("twice_named", s, rays, po.ACCUMULATOR)
    got = identities(renderer, rays, "twice", portable_math=True)
    length = mh.expected_counts(seqs)
    assert (np.diff(got[0]) > length).sum() >= 32
    kept = []
    for g in hl.segments(got):
        _, first = np.unique(g["prim"], return_index=True)
        kept.append([tuple(g[j]) for j in np.sort(first)])
    want = hl.csr(seqs)
    check(hl.csr(kept), want, "twice, without the repeats")
    # the sheets' duplicate: bit-equal t at positions 2 and 3, in traversal order
    assert sum(len(q) > 3 and q[2][0] == q[3][0] for q in seqs) >= 64


# ------------------------------------------------------------------------------------------------------------- 2: the identities
@pytest.mark.parametrize("flavour", FLAVOURS, ids=["default", "strict", "portable"])
def test_counts_and_first_eight_agree_with_trace_hits(renderer, flavour):
    for name in ("sheets", "cornell", "ties"):
        s, rays = hl.batch(name)
        renderer.set_scene(s)
        for prog in EPS_PROGRAMS:
            got = identities(renderer, rays, (name, prog), program=prog, **flavour)
        if name != "cornell":
            assert (np.diff(got[0]) > 8).sum() >= 64 and (np.diff(got[0]) == 0).sum() >= 64
    for scene, fams in ((me.base_scene(), me.base_families()), (me.dense_scene(), me.dense_families())):
        renderer.set_scene(scene)
        assert renderer.stats()["own_tree_height"] > 0
        for fam, rays in fams.items():
            identities(renderer, rays, fam, **flavour)
        rays = np.ascontiguousarray(np.concatenate(list(fams.values())))
        ok = qe.own_ok(rays)
        if "limits" in fams:                                    # rays of one batch, of one wave, take different walks
            assert 64 <= ok.sum() <= len(rays) - 64 and not qe.own_ok(fams["limits"]).all() and qe.own_ok(fams["limits"]).any()
        got = identities(renderer, rays, "all families", **flavour)
        assert (np.diff(got[0]) > 8).any()


# ------------------------------------------------------------------------------------------------------------- 3: ties
@pytest.mark.parametrize("prog", EPS_PROGRAMS)
def test_ties_come_in_the_references_traversal_order(renderer, prog):
    s, rays = hl.batch("ties")
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    seqs = hl.sequences("ties", prog)
    assert max(me.widest_tie(q) for q in seqs) == 12
    check(renderer.trace_hits_list(rays, program=prog, portable_math=True), hl.csr(seqs), ("ties", prog))


# ------------------------------------------------------------------------------------------------------------- 4: segment lengths
@pytest.fixture(scope="module")
def stack():
    rays, seqs, lengths = hl.stack_rays()
    return hl.stack_scene(), rays, hl.csr(seqs), lengths


def test_segment_lengths_in_one_batch(renderer, stack):
    s, rays, want, lengths = stack
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0 and qe.own_ok(rays).all() and len(rays) > 64
    assert np.diff(want[0]).tolist() == lengths.tolist() and lengths.max() == 2 * SPAN + 64
    check(renderer.trace_hits_list(rays, portable_math=True), want, "stack")
    order = np.random.default_rng(1).permutation(len(rays))          # the long segments in other lanes
    check(renderer.trace_hits_list(np.ascontiguousarray(rays[order]), portable_math=True), hl.gather(want, order), "stack, permuted")
    identities(renderer, rays, "stack")


def test_segment_lengths_each_alone(renderer, stack):
    s, rays, want, lengths = stack
    renderer.set_scene(s)
    for i in range(len(rays)):
        check(renderer.trace_hits_list(rays[i:i + 1], portable_math=True), hl.gather(want, [i]), ("stack", i, int(lengths[i])))


# ------------------------------------------------------------------------------------------------------------- 5: other hierarchies
@pytest.mark.parametrize("name", ("nan_bound", "bound_at_limit"))
def test_scenes_without_an_own_tree(renderer, name):
    s, rays = me.extreme(name)
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    want = hl.csr(mh.sequences("extreme_" + name, s, rays, po.ACCUMULATOR))
    assert len(want[1]) >= 1024
    check(renderer.trace_hits_list(rays, portable_math=True), want, name)
    for flavour in FLAVOURS:
        identities(renderer, rays, name, **flavour)


def test_the_stack_without_an_own_tree(renderer, stack):
    """Every ray inserts: segments of up to 2 span + 64 records kept sorted by the lane that fills them, half of them met nearest
    first and half farthest first."""
    s0, rays, want, _ = stack
    s = sc.Scene(s0.nodes.copy(), s0.prims.copy(), s0.materials.copy(), s0.lights.copy(), s0.camera)
    nv = s.node_view
    leaves = np.flatnonzero(nv["primitiveCount"] != 0)
    nv["boundsMax"][leaves[::7], 0] += np.float32(0.75)              # leaves that poke out of their ancestors: no own tree
    renderer.set_scene(s.validate())
    assert renderer.stats()["own_tree_height"] == -1
    check(renderer.trace_hits_list(rays, portable_math=True), want, "stack, the reference's order")


def test_the_callers_splits(monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        for name in ("sheets", "ties"):
            s, rays = hl.batch(name)
            r.set_scene(s)
            check(r.trace_hits_list(rays, portable_math=True), hl.csr(hl.sequences(name)), ("LT_RETREE=0", name))
            identities(r, rays, ("LT_RETREE=0", name))
        rays, seqs, _ = hl.stack_rays()
        r.set_scene(hl.stack_scene())
        check(r.trace_hits_list(rays, portable_math=True), hl.csr(seqs), "LT_RETREE=0, stack")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 6: the contract
@pytest.mark.parametrize("refill", (1, 64))
def test_batch_sizes_and_refill(renderer, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    s, rays = hl.batch("sheets")
    order = np.random.default_rng(3).permutation(len(rays))
    rays = np.ascontiguousarray(rays[order])
    want = hl.csr(hl.sequences("sheets"))
    renderer.set_scene(s)
    for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, len(rays)):
        check(renderer.trace_hits_list(rays[:n], portable_math=True), hl.gather(want, order[:n]), (n, refill))


def test_the_device_entry_point_on_a_side_stream(renderer):
    import torch
    s, all_rays = hl.batch("sheets")
    seqs = hl.sequences("sheets")
    renderer.set_scene(s)
    f = renderer._L.lt_hip_trace_hits_list_device
    side = torch.cuda.Stream()
    for n in (1, 65, TILE + 1):
        rays = np.array(all_rays[512:512 + n])                        # (random and axis rays, misses beside long lists, and on)
        wo, wi = want = hl.csr(seqs[512:512 + n])
        total = len(wi)
        assert total > 0
        rt = torch.from_numpy(rays).cuda()
        with torch.cuda.stream(side):
            go, gi = renderer.trace_hits_list(rt, portable_math=True)
        side.synchronize()
        assert go.dtype == torch.int64 and gi.dtype == torch.float32 and tuple(gi.shape) == (total, 4)
        check((go.cpu().numpy().view(np.uint64), records(gi)), want, (n, "wrapper"))
        go2, gi2 = renderer.trace_hits_list(rt, portable_math=True, stream=side)
        side.synchronize()
        assert torch.equal(go2, go) and torch.equal(gi2.view(torch.int32), gi.view(torch.int32))

        def raw(flags, offsets, items, items_records):
            rc = f(renderer._ctx, desc(flags | PORTABLE), vp(rt.data_ptr()), n, vp(offsets.data_ptr()), 8 * (n + 1),
                   vp(items.data_ptr()) if items is not None else None, 16 * items_records, vp(side.cuda_stream))
            side.synchronize()
            return rc

        def fresh(guard=64):
            o = torch.full((n + 1 + 16,), SENTINEL, dtype=torch.int64, device="cuda")
            i = torch.full((guard + total + guard, 4), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            return o, i, i[guard:]                                    # (64 records of 16 bytes: the items stay 16-byte aligned)

        # the one-shot call into sentinel-filled buffers: nothing in front of the items, nothing behind 8 (n + 1) and 16 total bytes
        o, whole, i = fresh()
        assert raw(0, o, i, total) == 0
        oo, ii = o.cpu().numpy().view(np.uint64), i.cpu().numpy()
        check((oo[:n + 1], records(ii[:total])), want, (n, "one-shot"))
        assert (oo[n + 1:] == SENTINEL).all() and (ii[total:] == SENTINEL).all() and (whole.cpu().numpy()[:64] == SENTINEL).all(), n
        # the sizing call alone, then FILL_ONLY from its offsets
        o, whole, i = fresh()
        assert raw(0, o, None, 0) == 0
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo) and (o.cpu().numpy()[n + 1:] == SENTINEL).all()
        assert (whole.cpu().numpy() == SENTINEL).all()
        assert raw(FILL, o, i, total) == 0
        ii = i.cpu().numpy()
        check((o.cpu().numpy().view(np.uint64)[:n + 1], records(ii[:total])), want, (n, "FILL_ONLY"))
        assert (ii[total:] == SENTINEL).all() and (whole.cpu().numpy()[:64] == SENTINEL).all(), n
        # one record short: nothing is written to the items, offsets[n] tells
        o, whole, i = fresh()
        assert raw(0, o, i, total - 1) == 0
        assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], wo) and (whole.cpu().numpy() == SENTINEL).all(), n
        # FILL_ONLY with offsets that are no scan -- reversed (decreasing), beyond the capacity, huge -- on items of the true size:
        # whatever is written lies inside items[0 .. total); the guards in front and behind stay
        rng = np.random.default_rng(n)
        for kind in ("reversed", "beyond", "huge", "random"):
            bad = {"reversed": wo[::-1].copy(), "beyond": wo + np.uint64(total // 2 + 1),
                   "huge": np.full(n + 1, 2 ** 64 - 1, dtype=np.uint64) - wo,
                   "random": rng.integers(0, 2 * total + 2, n + 1).astype(np.uint64)}[kind]
            o, whole, i = fresh()
            o[:n + 1] = torch.from_numpy(np.ascontiguousarray(bad).view(np.int64)).cuda()
            torch.cuda.synchronize()
            assert raw(FILL, o, i, total) == 0
            w = whole.cpu().numpy()
            assert (w[:64] == SENTINEL).all() and (w[64 + total:] == SENTINEL).all(), (n, kind)
            assert np.array_equal(o.cpu().numpy().view(np.uint64)[:n + 1], bad), (n, kind)
            # a written record is one of the batch's own
            own = {r.tobytes() for r in wi}
            touched = records(w[64:64 + total])
            touched = touched[(hl.words(touched) != SENTINEL).any(axis=1)]
            assert all(r.tobytes() in own for r in touched), (n, kind)


def test_every_error_leaves_the_buffers_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        rays = make_rays(np.array([[0.0, 2.5, -20.0]] * 4), np.array([[0.0, 0.0, 1.0]] * 4))
        offsets = np.full(8, SENTINEL, dtype=np.uint64)
        items = np.full(4 * 256, SENTINEL, dtype=np.uint32).view(HIT_DTYPE)

        def clean():
            return bool((offsets == SENTINEL).all() and (items.view(np.uint32) == SENTINEL).all())

        O, I, R = offsets.ctypes.data_as(vp), items.ctypes.data_as(vp), rays.ctypes.data_as(vp)
        INVALID, SMALL, UNKNOWN = C.LT_ERR_INVALID_ARGUMENT, C.LT_ERR_BUFFER_TOO_SMALL, C.LT_ERR_UNKNOWN_PROGRAM
        f = L.lt_hip_trace_hits_list
        assert f(r._ctx, desc(), R, 4, O, 40, I, 4096) == C.LT_ERR_NO_SCENE and clean()
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        cases = [
            (None, R, 4, O, 40, I, 4096, INVALID),
            (desc(size=8), R, 4, O, 40, I, 4096, INVALID),
            (desc(program=1000), R, 4, O, 40, I, 4096, INVALID),        # (LT_PROGRAM_USER_BASE: a user program)
            (desc(program=-1), R, 4, O, 40, I, 4096, UNKNOWN),
            (desc(program=C.PROGRAM_CUSTOM_OPENCL + 1), R, 4, O, 40, I, 4096, UNKNOWN),
            (desc(flags=1), R, 4, O, 40, I, 4096, INVALID),          # (the other lists' FILL_ONLY bit is not this family's)
            (desc(flags=FILL | 0x400), R, 4, O, 40, I, 4096, INVALID),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH | PORTABLE), R, 4, O, 40, I, 4096, INVALID),
            (desc(reserved=1), R, 4, O, 40, I, 4096, INVALID),
            (desc(), R, 2 ** 32, O, 40, I, 4096, INVALID),
            (desc(), None, 4, O, 40, I, 4096, INVALID),
            (desc(), R, 4, None, 40, I, 4096, INVALID),
            (desc(), R, 4, O, 40, None, 4096, INVALID),
            (desc(FILL), R, 4, O, 40, None, 0, INVALID),
            (desc(), R, 4, O, 39, I, 4096, SMALL),
            (desc(FILL), R, 4, O, 39, I, 4096, SMALL),
            (desc(), R, 4, O, 39, None, 0, SMALL),
            (desc(flags=4), R, 4, O, 0, I, 0, INVALID),              # an unknown flag comes before the buffers' sizes
        ]
        for i, (*args, want) in enumerate(cases):
            assert f(r._ctx, *args) == want, i
            assert clean(), i
        # every flag the family takes, and n == 0: nothing is launched; offsets[0] = 0 unless FILL_ONLY
        assert f(r._ctx, desc(FILL | C.TRACE_FLAG_COHERENT | PORTABLE), None, 0, O, 8, I, 4096) == 0 and clean()
        assert f(r._ctx, desc(C.TRACE_FLAG_COHERENT | C.RENDER_FLAG_STRICT_MATH), None, 0, O, 8, None, 0) == 0
        assert offsets[0] == 0 and (offsets[1:] == SENTINEL).all() and (items.view(np.uint32) == SENTINEL).all()
        offsets[:] = SENTINEL
        # the device entry point: the same checks, and 16-byte alignment
        rt = torch.from_numpy(rays).cuda()
        ot_ = torch.full((16,), SENTINEL, dtype=torch.int64, device="cuda")
        it = torch.full((256, 4), SENTINEL, dtype=torch.int32, device="cuda")
        g = L.lt_hip_trace_hits_list_device
        rp, op, ip = rt.data_ptr(), ot_.data_ptr(), it.data_ptr()
        for a, b, c in ((rp + 4, op, ip), (rp, op + 8, ip), (rp, op, ip + 4), (rp, op, ip + 8)):
            assert g(r._ctx, desc(), vp(a), 3, vp(b), 64, vp(c), 2048, None) == INVALID
            assert g(r._ctx, desc(FILL), vp(a), 3, vp(b), 64, vp(c), 2048, None) == INVALID
        assert g(r._ctx, desc(), vp(rp), 4, vp(op), 39, vp(ip), 4096, None) == SMALL
        assert g(r._ctx, desc(flags=2), vp(rp), 4, vp(op), 40, vp(ip), 4096, None) == INVALID
        assert g(r._ctx, desc(reserved=7), vp(rp), 4, vp(op), 40, vp(ip), 4096, None) == INVALID
        assert g(r._ctx, None, vp(rp), 4, vp(op), 40, vp(ip), 4096, None) == INVALID
        assert g(r._ctx, desc(), vp(rp), 4, vp(op), 40, None, 16, None) == INVALID
        assert g(r._ctx, desc(FILL), vp(rp), 4, vp(op), 40, None, 0, None) == INVALID
        assert g(r._ctx, desc(), vp(rp), 2 ** 32, vp(op), 40, vp(ip), 4096, None) == INVALID
        torch.cuda.synchronize()
        assert (ot_.cpu().numpy() == SENTINEL).all() and (it.cpu().numpy() == SENTINEL).all()
        assert g(r._ctx, desc(), None, 0, vp(op), 8, None, 0, None) == 0      # n == 0 on the device: offsets[0] = 0, nothing else
        torch.cuda.synchronize()
        assert ot_[0].item() == 0 and (ot_.cpu().numpy()[1:] == SENTINEL).all()
        # the host entry point: items too small are LT_ERR_BUFFER_TOO_SMALL, with the offsets written and the items untouched
        count = r.trace_hits(rays, count=True)
        total = int(count.sum())
        assert 4 <= total <= 256
        assert f(r._ctx, desc(), R, 4, O, 40, I, 16 * (total - 1)) == SMALL
        assert np.array_equal(np.diff(offsets[:5]), count) and (offsets[5:] == SENTINEL).all() and (items.view(np.uint32) == SENTINEL).all()
        with pytest.raises(ValueError):
            r.trace_hits_list(np.zeros((4, 6), dtype=np.float32))
        with pytest.raises(ValueError):
            r.trace_hits_list(torch.zeros((4, 4), device="cuda"))
        with pytest.raises(TypeError):
            r.trace_hits_list([[0.0] * 8])
        with pytest.raises(C.LensTraceError):
            r.trace_hits_list(rays, portable_math=True, strict_math=True)
    finally:
        r.close()


def test_calls_interleave_and_stats_report_them():
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
        _, rays = hl.batch("cornell")
        want = hl.csr(hl.sequences("cornell"))
        hits_before = r2.trace_rays(rays, portable_math=True)
        # the raw host calls: sizing 4 kernels, FILL_ONLY 2, both 6
        offsets = np.zeros(len(rays) + 1, dtype=np.uint64)
        items = np.zeros(len(want[1]), dtype=HIT_DTYPE)
        f = r2._L.lt_hip_trace_hits_list
        for flags, it, launches in ((0, None, 4), (FILL, items, 2), (0, items, 6)):
            items[:] = 0
            r2._check(f(r2._ctx, desc(flags | PORTABLE), rays.ctypes.data_as(vp), len(rays), offsets.ctypes.data_as(vp), offsets.nbytes,
                        None if it is None else it.ctypes.data_as(vp), 0 if it is None else it.nbytes))
            st = r2.stats()
            assert st["rays"] == len(rays) and st["shadow_rays"] == 0 and st["kernel_launches"] == launches and st["kernel_ms"] > 0, (flags, st)
            assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
            check((offsets, items) if it is not None else (offsets, want[1]), want, flags)
        got = r2.trace_hits_list(rays, portable_math=True)
        check(got, want, "wrapper")
        # surface_at takes the records as they are: the first record of a segment gives trace_surface's record
        first = got[0][:-1][np.diff(got[0]) > 0].astype(np.int64)
        surf = r2.surface_at(got[1], portable_math=True)
        ts = r2.trace_surface(rays, portable_math=True)[np.diff(got[0]) > 0]
        assert surf[first].tobytes() == ts.tobytes()
        assert np.array_equal(r2.trace_rays(rays, portable_math=True).view(np.uint32), hits_before.view(np.uint32))
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # set_scene of another scene right behind an enqueued one-shot device call: it keeps the old scene's lists
        rt = torch.from_numpy(np.array(rays)).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        od = torch.zeros(len(rays) + 1, dtype=torch.int64, device="cuda")
        idev = torch.zeros((len(want[1]), 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r2._check(r2._L.lt_hip_trace_hits_list_device(r2._ctx, desc(PORTABLE), vp(rt.data_ptr()), len(rays), vp(od.data_ptr()), 8 * (len(rays) + 1),
                                                       vp(idev.data_ptr()), 16 * len(idev), vp(stream.cuda_stream)))
        sheets, sheet_rays = hl.batch("sheets")
        r2.set_scene(sheets)
        stream.synchronize()
        check((od.cpu().numpy().view(np.uint64), records(idev)), want, "behind set_scene")
        check(r2.trace_hits_list(sheet_rays[:512], portable_math=True), hl.csr(hl.sequences("sheets")[:512]), "the new scene")
        # a scene without an own tree: a fill has no ordering launch
        r2.set_scene(me.twice_named_scene()[0])
        r2.trace_hits_list(sheet_rays[:64])
        assert r2.stats()["kernel_launches"] == 1
    finally:
        r1.close()
        r2.close()
