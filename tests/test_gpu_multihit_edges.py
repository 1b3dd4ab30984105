"""GPU (-m gpu): the multi-hit query (lt_hip_trace_hits: lt_query_hits_kernel, own_walk_step_all, HitList) at its edges, on the
fixtures of tests/multihit_edges.py (whose claims tests/test_multihit_edges_cpu.py checks), through RendererHIP.trace_hits.
`check` is tests/test_gpu_trace_hits.py's check_against_the_oracle: the portable flavour, K = 1, 3, 8 and the count, every ray
and every record bit for bit the peeling oracle, the miss records' tmax bits included.

1. exact ties of two to twelve hits on the own-tree walk, in every octant, wider than a list and straddling its end: only rank8
   orders them; the caller's splits (LT_RETREE=0) give the same bytes;
2. every family of tests/query_edges.py -- octants, per-lane tmax, ignoring lanes, intruders, partial chunks, packet_ray_ok's
   limits, epsilon bands -- on its base scene and on a dense one whose lists overflow; in the default and strict flavours the
   kinds agree with each other and with trace_rays; the epsilon bands tell the programs' counts apart;
3. the scenes at extreme magnitudes, where the count sees every wrongly rejected box, and origins far from a scene of unit size;
4. a soup deep enough for the stack's private-memory rows;
5. batches large enough for claims of 128 to 512 rays, a capped grid and the sweep over the other XCDs' eighths; small batches
   permuted and under LT_TRACE_REFILL = 1 and 64;
6. ignore values that name no primitive, a query followed at once by set_scene, a query between two renders, and the documented
   exception: leaves that name one primitive twice."""
import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import HIT_DTYPE, RendererHIP
from oracle import pyoracle as po
from tests import multihit as mh
from tests import multihit_edges as me
from tests import query_edges as qe
from tests.conftest import oracle_props as RenderPropertiesHIP
from tests.test_gpu_trace_hits import EPS_PROGRAMS, FLAVOURS, KS
from tests.test_gpu_trace_hits import check_against_the_oracle as check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


def all_kinds(r, rays, **kw):
    return [r.trace_hits(rays, max_hits=k, **kw) for k in KS] + [r.trace_hits(rays, count=True, **kw)]


def check_kinds_agree(r, rays, prog, flavour, what):
    """tests/test_gpu_trace_hits.py's test_kinds_agree_with_each_other_and_with_trace_rays, for one batch: K = 1 is the closest-hit
    query, K = 3 opens K = 8, the count agrees with both, any hit is count > 0.  Returns the counts."""
    first = r.trace_hits(rays, max_hits=1, program=prog, **flavour)
    closest = r.trace_rays(rays, program=prog, **flavour)
    assert first.tobytes() == closest.tobytes(), (what, prog, flavour)
    k3 = r.trace_hits(rays, max_hits=3, program=prog, **flavour)
    k8 = r.trace_hits(rays, max_hits=8, program=prog, **flavour)
    assert k3.tobytes() == np.ascontiguousarray(k8[:, :3]).tobytes(), (what, prog, flavour)
    n = r.trace_hits(rays, count=True, program=prog, **flavour)
    listed = (k8["prim"] >= 0).sum(axis=1)
    assert np.array_equal(n[listed < 8], listed[listed < 8]) and (n[listed == 8] >= 8).all(), (what, prog, flavour)
    anyhit = r.trace_rays(rays, any_hit=True, program=prog, **flavour)
    assert np.array_equal(anyhit, (n > 0).astype(np.uint32)), (what, prog, flavour)
    return n


# ------------------------------------------------------------------------------------------------------------ 1: exact ties
@pytest.mark.parametrize("prog", EPS_PROGRAMS)
def test_exact_ties_follow_the_references_leaf_order(renderer, prog):
    s = mh.sheets_scene()
    rays = me.dyadic_rays()[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check(renderer, "dyadic", s, rays, prog)


def test_exact_ties_with_the_callers_splits(renderer, monkeypatch):
    s = mh.sheets_scene()
    rays = me.dyadic_rays()[0]
    renderer.set_scene(s)
    want = {p: all_kinds(renderer, rays, program=p, portable_math=True) for p in EPS_PROGRAMS}
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(s)
        assert r.stats()["own_tree_height"] > 0
        for p in EPS_PROGRAMS:
            for g, w in zip(all_kinds(r, rays, program=p, portable_math=True), want[p]):
                assert g.tobytes() == w.tobytes(), p
    finally:
        r.close()


# ------------------------------------------------------------------------------------------- 2: query_edges' families, two scenes
FAMILY_CASES = [("base", f) for f in ("coherent", "tmax", "ignore", "ties", "intruders", "partial1", "partial33", "partial63", "limits", "eps")]
FAMILY_CASES += [("dense", f) for f in me.DENSE_FAMILIES]


@pytest.mark.parametrize("where,family", FAMILY_CASES, ids=["%s-%s" % c for c in FAMILY_CASES])
def test_query_edges_families(renderer, where, family):
    s = me.base_scene() if where == "base" else me.dense_scene()
    rays = (me.base_families() if where == "base" else me.dense_families())[family]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    for prog in EPS_PROGRAMS:
        check(renderer, "%s_%s" % (where, family), s, rays, prog)
    counts = {}
    for flavour in FLAVOURS:
        for prog in EPS_PROGRAMS:
            if flavour.get("portable_math"):          # (held against the oracle above)
                counts[prog] = renderer.trace_hits(rays, count=True, program=prog, **flavour)
            else:
                counts[prog] = check_kinds_agree(renderer, rays, prog, flavour, (where, family))
        if family == "eps":
            # the epsilon bands tell the programs apart (tests/test_gpu_query_edges.py: test_the_epsilon_bands_tell_the_programs_apart)
            differ = (counts[C.PROGRAM_BASIC] != counts[C.PROGRAM_ACCUMULATOR]).sum()
            print("eps", flavour, "rays whose count differs between basic and accumulator:", differ)
            assert differ >= 50, flavour
            assert np.array_equal(counts[C.PROGRAM_BASIC], counts[C.PROGRAM_BASIC_LIGHTING]), flavour


def test_the_family_fixtures_are_complete():
    assert sorted(f for w, f in FAMILY_CASES if w == "base") == sorted(me.base_families())


# ---------------------------------------------------------------------------------------------------- 3: extreme magnitudes
@pytest.mark.parametrize("name", sorted(qe.EXTREME))
def test_extreme_scenes(renderer, name):
    s, rays = me.extreme(name)
    renderer.set_scene(s)
    h = renderer.stats()["own_tree_height"]
    assert (h > 0) if qe.EXTREME[name][3] else (h == -1), (name, h)
    for prog in me.extreme_programs(name):
        check(renderer, "extreme_" + name, s, rays, prog)
    n = renderer.trace_hits(rays, count=True, portable_math=True)
    assert (n > 0).mean() >= 0.3


def test_far_origins(renderer):
    """Origins a thousand to 65 thousand scene extents away: where own16_ray's margin alone covers the roundings of o * inv
    (tests/multihit_edges.py: far_rays)."""
    s, rays = me.base_scene(), me.far_rays()
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check(renderer, "far", s, rays, C.PROGRAM_ACCUMULATOR)
    for flavour in FLAVOURS[:2]:
        check_kinds_agree(renderer, rays, C.PROGRAM_ACCUMULATOR, flavour, "far")


# ------------------------------------------------------------------------------------------------------ 4: the private stack
def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def test_the_soup_sample_equals_the_oracle(renderer):
    """K = 8 and the count of the rays the CPU peels (a twentieth of which, at least, walk with more than kTraceRows stack
    entries: tests/test_multihit_edges_cpu.py), traced within the whole batch."""
    import torch
    s = me.soup_scene()
    rays, sample = me.soup_rays()
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    seqs = mh.sequences("soup", s, rays[sample], po.ACCUMULATOR)
    rt = torch.from_numpy(np.array(rays)).cuda()
    k8 = renderer.trace_hits(rt, max_hits=8, portable_math=True)
    n = renderer.trace_hits(rt, count=True, portable_math=True)
    torch.cuda.synchronize()
    pick = torch.from_numpy(np.array(sample)).cuda()
    got = k8[pick].cpu().numpy().view(HIT_DTYPE).reshape(len(sample), 8)
    bad = mh.same_records(got, mh.expected_records(seqs, rays[sample], 8))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:2]], [seqs[i][:8] for i in bad[:2]])
    want_n = mh.expected_counts(seqs)
    got_n = n[pick].cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got_n != want_n)
    assert len(bad) == 0, (len(bad), bad[:5], got_n[bad[:5]], want_n[bad[:5]])
    assert (want_n > 8).sum() >= 32


@pytest.mark.parametrize("flavour", FLAVOURS, ids=["default", "strict", "portable"])
def test_the_soup_kinds_agree_on_every_ray(renderer, flavour):
    import torch
    s = me.soup_scene()
    renderer.set_scene(s)
    rt = torch.from_numpy(np.array(me.soup_rays()[0])).cuda()
    k1 = renderer.trace_hits(rt, max_hits=1, **flavour)
    closest = renderer.trace_rays(rt, **flavour)
    assert torch.equal(bits(k1).reshape(-1), bits(closest).reshape(-1))
    k3 = renderer.trace_hits(rt, max_hits=3, **flavour)
    k8 = renderer.trace_hits(rt, max_hits=8, **flavour)
    assert torch.equal(bits(k3), bits(k8[:, :3]))
    n = renderer.trace_hits(rt, count=True, **flavour).to(torch.int64)
    listed = (bits(k8)[:, :, 1] >= 0).sum(dim=1)
    assert torch.equal(n[listed < 8], listed[listed < 8]) and bool((n[listed == 8] >= 8).all())
    anyhit = renderer.trace_rays(rt, any_hit=True, **flavour).to(torch.int64)
    assert torch.equal(anyhit, (n > 0).to(torch.int64))
    assert int((n > 8).sum()) >= 1000 and int((n == 0).sum()) >= 1000


# ------------------------------------------------------------------------------------------------------- 5: the claim loop
def tiled(base, n):
    """The first n rays of the 2577-ray batch repeated (on the device)."""
    return base.repeat(-(-n // len(base)), 1)[:n].contiguous()


def kind_kw(k):
    return {"count": True} if k == 0 else {"max_hits": k}


def sheet_expectation(k):
    s, rays = mh.sheets_scene(), mh.sheet_rays()[0]
    seqs = mh.sequences("sheets", s, rays, po.ACCUMULATOR)
    return mh.expected_counts(seqs) if k == 0 else mh.expected_records(seqs, rays, k)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["claim128", "between", "claim512"])
@pytest.mark.parametrize("k", [0, 8], ids=["count", "first8"])
def test_large_batches_claim_more_than_a_stage(renderer, k, which):
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = me.claim_sizes(k, cu)[which]
    grid, claim = me.hits_launch(n, k, cu)
    print("CUs", cu, "n", n, "grid", grid, "claim", claim)
    assert claim == (128, claim, 512)[which] and 128 <= claim <= 512 and grid < -(-n // 64)
    renderer.set_scene(mh.sheets_scene())
    base = torch.from_numpy(np.array(mh.sheet_rays()[0])).cuda()
    m = len(base)
    out = renderer.trace_hits(tiled(base, n), portable_math=True, **kind_kw(k))
    torch.cuda.synchronize()
    out = bits(out).reshape(n, -1)
    # the first copy is the oracle's; every other copy is the first
    want = sheet_expectation(k)
    first = out[:m].cpu().numpy()
    bad = np.flatnonzero((first.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32).reshape(m, -1)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5])
    whole = n // m
    differ = (out[:whole * m].reshape(whole, m, -1) != out[:m]).any(dim=2)
    assert not bool(differ.any()), (int(differ.sum()), torch.nonzero(differ)[:5].tolist())
    assert torch.equal(out[whole * m:], out[:n - whole * m])


@pytest.mark.parametrize("n", me.SMALL_SIZES)
@pytest.mark.parametrize("k", [0, 8], ids=["count", "first8"])
def test_small_batches_permuted_and_refilled(renderer, monkeypatch, k, n):
    renderer.set_scene(mh.sheets_scene())
    base = np.array(mh.sheet_rays()[0])
    reps = -(-n // len(base))
    rays = np.tile(base, (reps, 1))[:n]
    want = np.concatenate([sheet_expectation(k)] * reps)[:n]
    got = renderer.trace_hits(rays, portable_math=True, **kind_kw(k))
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    perm = np.random.default_rng(n).permutation(n)
    assert renderer.trace_hits(rays[perm], portable_math=True, **kind_kw(k)).tobytes() == want[perm].tobytes()
    for refill in ("1", "64"):
        monkeypatch.setenv("LT_TRACE_REFILL", refill)
        assert renderer.trace_hits(rays, portable_math=True, **kind_kw(k)).tobytes() == want.tobytes(), refill


# ------------------------------------------------------------------------------------------------------------ 6: small pins
def test_ignore_values_outside_the_scene(renderer):
    s = mh.sheets_scene()
    rays, cat = mh.sheet_rays()
    through = np.array(rays[cat == "through"])
    renderer.set_scene(s)
    minus_one = all_kinds(renderer, through, portable_math=True)
    for v in me.odd_ignore_values(s.n_prims):
        r = me.with_ignore(through, v)
        check(renderer, "ignore_%d" % v, s, r, C.PROGRAM_ACCUMULATOR)
        if v < 0:                                   # every negative value is -1
            for g, w in zip(all_kinds(renderer, r, portable_math=True), minus_one):
                assert g.tobytes() == w.tobytes(), v
        for flavour in FLAVOURS[:2]:
            check_kinds_agree(renderer, r, C.PROGRAM_ACCUMULATOR, flavour, v)


def test_a_query_keeps_its_scene_when_set_scene_follows_at_once():
    import torch
    soup, sheets = me.soup_scene(), mh.sheets_scene()
    rays = np.array(me.soup_rays()[0])
    r = RendererHIP(0)
    try:
        r.set_scene(soup)
        want = [r.trace_hits(rays, max_hits=8), r.trace_hits(rays, count=True)]
        assert (want[1] > 0).mean() > 0.3
        rt = torch.from_numpy(rays).cuda()
        stream = torch.cuda.Stream()
        for kw, w in zip(({"max_hits": 8}, {"count": True}), want):
            r.set_scene(soup)
            got = r.trace_hits(rt, stream=stream, **kw)
            r.set_scene(sheets)
            stream.synchronize()
            assert got.cpu().numpy().tobytes() == w.tobytes(), kw
    finally:
        r.close()


def test_a_query_between_two_renders_changes_neither():
    import os
    from tests.conftest import GOLDEN
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
        rays = mh.cornell_rays()[1]
        n = r2.trace_hits(rays, count=True)
        r2.trace_hits(rays, max_hits=8)
        assert (n > 0).mean() > 0.3
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for key in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[key] == t1[key], key
        assert t2["shadow_packets"] == s2["shadow_packets"] and t1["shadow_packets"] == s1["shadow_packets"]
        assert t2["frames"] == 4 and t2["render_ms"] > 0
    finally:
        r1.close()
        r2.close()


def test_leaves_that_name_one_primitive_twice(renderer):
    """include/lenstrace_hip.h's exception: such a scene gets no own hierarchy, and there a primitive may appear once per leaf
    that names it.  Without the repeats the list is the peel sequence; the count exceeds the sequence's length by the second
    reports and nothing else."""
    s = me.twice_named_scene()[0]
    rays = mh.sheet_rays()[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    seqs = mh.sequences("twice_named", s, rays, po.ACCUMULATOR)
    sure, possible = me.twice_named_reach(rays, seqs)
    k8 = renderer.trace_hits(rays, max_hits=8, portable_math=True)
    n = renderer.trace_hits(rays, count=True, portable_math=True)
    length = mh.expected_counts(seqs)
    low, high = length + sure, length + possible
    bad = np.flatnonzero((n < low) | (n > high))
    assert len(bad) == 0, (len(bad), bad[:5], n[bad[:5]], low[bad[:5]], high[bad[:5]])
    print("rays whose count exceeds their sequence:", (n > length).sum(), "lists with a repeat:",
          sum(len(set(row["prim"][row["prim"] >= 0])) < (row["prim"] >= 0).sum() for row in k8))
    assert (n > length).sum() >= 32
    repeats = 0
    for i, (row, seq) in enumerate(zip(k8, seqs)):
        kept, seen = [], set()
        for rec in row[row["prim"] >= 0]:
            if int(rec["prim"]) not in seen:
                seen.add(int(rec["prim"]))
                kept.append(rec)
        listed = int((row["prim"] >= 0).sum())
        repeats += listed - len(kept)
        assert listed == min(8, int(n[i])), i
        got = np.array(kept, dtype=HIT_DTYPE)
        want = mh.expected_records([seq[:len(kept)]], rays[i:i + 1], max(len(kept), 1))[0][:len(kept)]
        assert got.tobytes() == want.tobytes(), (i, got, seq[:len(kept)])
        if listed < 8:
            assert len(kept) == len(seq), i
        # the slots behind the list are miss records with the ray's own tmax bits
        tail = row[listed:]
        assert (tail["prim"] == -1).all() and (tail["t"].view(np.uint32) == rays[i, 3:4].view(np.uint32)).all(), i
    assert repeats >= ((sure > 0) & (high <= 8)).sum() >= 8
