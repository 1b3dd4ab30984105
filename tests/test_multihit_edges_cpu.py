"""CPU tests of tests/multihit_edges.py: its fixtures hold what tests/test_gpu_multihit_edges.py relies on, each claim checked with
the peeling oracle -- exact ties of six and twelve in every octant whose peel order is SceneDev::rank8's, a dense scene whose rays
overflow their lists, rays that hit on every scene at extreme magnitudes, a soup whose rays leave the ten LDS rows of the stack,
the launch rule of lt_query.hip restated, leaves that name a primitive twice.  No GPU."""
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from oracle import pyoracle as po
from tests import multihit as mh
from tests import multihit_edges as me
from tests import query_edges as qe

PROGRAMS = (po.BASIC, po.BASIC_LIGHTING, po.ACCUMULATOR)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lens_trace_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------- the peel stop
def test_the_peel_stops_after_n_prims_plus_one(monkeypatch):
    s = mh.sheets_scene()
    p = mh.Peeler(s)
    assert p.pv.size == s.n_prims
    ray = mh.sheet_rays()[0][np.flatnonzero(mh.sheet_rays()[1] == "through")[0]]
    want = p.peel(ray, po.ACCUMULATOR)
    before = p.prims.copy()
    hit = p.trace(ray, po.ACCUMULATOR)
    monkeypatch.setattr(p, "trace", lambda ray, program: hit)        # a trace that never misses
    with pytest.raises(AssertionError, match="does not end"):
        p.peel(ray, po.ACCUMULATOR)
    assert np.array_equal(p.prims, before)                            # the scene copy is restored all the same
    monkeypatch.undo()
    assert p.peel(ray, po.ACCUMULATOR) == want
    assert len(p.peel(ray, po.ACCUMULATOR, limit=3)) == 3


# ------------------------------------------------------------------------------------------------------------ 1: exact ties
@pytest.mark.parametrize("prog", PROGRAMS)
def test_dyadic_rays_tie_as_claimed_and_peel_in_rank_order(prog):
    s = mh.sheets_scene()
    rays, kinds, ms = me.dyadic_rays()
    assert qe.own_ok(rays).all()
    octant = qe.octant(rays)
    assert (np.bincount(octant, minlength=8) >= 32).all()
    assert (ms == 0).sum() >= 64 and {"vertex", "x_edge", "y_edge", "diagonal"} == set(kinds)
    seqs = mh.sequences("dyadic", s, rays, prog)
    widest = np.array([me.widest_tie(q) for q in seqs])
    straddle = {k: sum(me.straddles(q, k) for q in seqs) for k in me.KS}
    minus = sum(any(h[0] == 0 and np.signbit(h[0]) for h in q) for q in seqs)
    plus = sum(any(h[0] == 0 and not np.signbit(h[0]) for h in q) for q in seqs)
    both = sum(me.both_zeros(q) for q in seqs)
    print("widest tie", np.bincount(widest), "straddling", straddle, "rays with -0 / +0 / both", minus, plus, both)
    assert (widest >= 6).sum() >= 128
    assert (widest >= 12).sum() >= 24 and C.TRACE_MAX_HITS < 12
    assert min(straddle.values()) >= 64
    # ties of 2 and 4 between DIFFERENT triangles: the edge and diagonal rays
    for kind in ("x_edge", "y_edge", "diagonal"):
        w = widest[kinds == kind]
        assert (w >= 2).sum() >= 32 and (w >= 4).sum() >= 4, kind
    # t = +-0: the construction gives no ray with both (dyadic_rays says why); each sign is there on its own
    assert minus >= 64 and plus >= 64 and both == 0
    # within every tie group the peel order is ascending in rank8[prim, octant]: the kernel's rule, restated against the oracle
    h, _, rank8 = C.own_hierarchy(s.node_view, s.n_prims, want_ranks=True)
    assert h > 0
    groups = 0
    for q, o in zip(seqs, octant):
        for a, b in me.tie_groups(q):
            r = [int(rank8[q[j][1], o]) for j in range(a, b)]
            assert r == sorted(r) and len(set(r)) == len(r), (q[a:b], o)
            groups += b - a > 1
    assert groups >= 1000


# ------------------------------------------------------------------------------------------------------- 2: the two scenes
def test_the_dense_scene_overflows_the_lists():
    s = me.dense_scene()
    assert C.own_hierarchy(s.node_view, s.n_prims)[0] > 0
    fams = me.dense_families()
    assert tuple(fams) == me.DENSE_FAMILIES
    n = mh.expected_counts(mh.sequences("dense_coherent", s, fams["coherent"], po.ACCUMULATOR))
    print("dense coherent: mean", n.mean(), "more than 8:", (n > 8).mean())
    assert n.mean() > 8 and (n > 8).mean() >= 0.25
    # the families are query_edges' own: every chunk qualifies as it is built to
    for name, rays in fams.items():
        assert len(rays) % qe.LANES == (33 if name == "partial33" else 0)
    assert all(v is not None for v in qe.chunk_verdicts(fams["coherent"], False))
    assert all(v is None for v in qe.chunk_verdicts(fams["ignore"], False))


def test_the_base_families_are_query_edges_own():
    fams = me.base_families()
    want = {b.name: b.rays for b in qe.families(qe.base_scene(0), 0)}
    assert sorted(fams) == sorted(want) and len(fams) == 10
    for name in want:
        assert fams[name].tobytes() == want[name].tobytes()
    n = mh.expected_counts(mh.sequences("base_coherent", me.base_scene(), fams["coherent"], po.ACCUMULATOR))
    assert 0.8 <= n.mean() <= 3.2


# ---------------------------------------------------------------------------------------------------- 3: extreme magnitudes
@pytest.mark.parametrize("name", sorted(qe.EXTREME))
def test_rays_hit_on_every_extreme_scene(name):
    s, rays = me.extreme(name)
    assert len(rays) == sum(len(me.base_families()[f]) for f in me.SCALED_FAMILIES)
    for prog in me.extreme_programs(name):
        n = mh.expected_counts(mh.sequences("extreme_" + name, s, rays, prog))
        print(name, prog, "rays with a hit: %.3f" % (n > 0).mean(), "hits per ray: %.2f" % n.mean())
        assert (n > 0).mean() >= 0.3
    assert (C.own_hierarchy(s.node_view, s.n_prims)[0] > 0) == qe.EXTREME[name][3]
    assert set(me.EXTREME_PROGRAMS) <= set(qe.EXTREME)


def test_the_far_rays():
    rays = me.far_rays()
    assert len(rays) == 64 * 64 * len(me.FAR_DISTANCES) and qe.own_ok(rays).all()
    assert (np.bincount(qe.octant(rays), minlength=8) == len(rays) // 8).all()
    assert all(v is not None for v in qe.chunk_verdicts(rays, False))
    dist = np.linalg.norm(rays[:, 0:3].astype(np.float64), axis=1).reshape(len(me.FAR_DISTANCES), -1)
    for d, far in zip(dist, me.FAR_DISTANCES):
        assert (np.abs(d - far) < 8).all() and far >= 1000 * 8
    n = mh.expected_counts(mh.sequences("far", me.base_scene(), rays, po.ACCUMULATOR)).reshape(len(me.FAR_DISTANCES), -1)
    print("far rays with a hit, per distance:", (n > 0).mean(axis=1), "hits per ray:", n.mean(axis=1))
    assert ((n > 0).mean(axis=1) >= 0.3).all()


# ----------------------------------------------------------------------------------------------------- 4: the private stack
def test_the_soup_rays_leave_the_stacks_lds_rows():
    with open(os.path.join(CSRC, "lt_device.hpp")) as f:
        assert int(re.search(r"constexpr int kTraceRows = (\d+);", f.read()).group(1)) == me.TRACE_ROWS
    s = me.soup_scene()
    rays, sample = me.soup_rays()
    assert s.n_prims >= me.SOUP_COUNT and len(rays) == me.SOUP_RAYS and len(sample) == me.SOUP_SAMPLE
    depth = me.stack_depths(s, rays[sample])
    print("N", me.SOUP_COUNT, "stack depths (lower bound)", np.bincount(depth), "above kTraceRows:", (depth > me.TRACE_ROWS).sum())
    assert (depth > me.TRACE_ROWS).sum() >= 64
    assert depth.max() < 64
    # what the GPU test asks of the whole batch, twenty times over in the sample: rays that overflow a list of 8, rays of no hit
    n = mh.expected_counts(mh.sequences("soup", s, rays[sample], po.ACCUMULATOR))
    print("hits per sampled ray: mean %.2f, most %d, more than 8: %d, none: %d" % (n.mean(), n.max(), (n > 8).sum(), (n == 0).sum()))
    assert (n > 8).sum() >= 40 and (n == 0).sum() >= 40


def test_the_lower_bound_walk_on_the_sheets():
    """stack_depths' walk on a scene small enough to say what it must find: a ray through all the sheets pops at least the
    leaves of the triangles it hits well inside (most of its thirteen), far fewer than the scene has, and its stack stays
    under the bound the build guarantees (3 heights of the group tree + 4)."""
    s = mh.sheets_scene()
    rays, cat = mh.sheet_rays()
    rays = rays[cat == "through"]
    depth, popped = me.stack_depths(s, rays, leaves=True)
    h, own, _ = C.own_hierarchy(s.node_view, s.n_prims)
    hw = C.own_wide(own, s.n_prims)[0]
    print("sheets: depth", np.bincount(depth), "leaves popped: min", popped.min(), "mean", popped.mean(), "max", popped.max())
    assert (depth >= 3).all() and depth.max() <= 3 * hw + 4
    assert (popped >= 8).all() and popped.mean() >= mh.SHEETS and popped.max() < s.n_prims // 4


# ------------------------------------------------------------------------------------------------------- 5: the claim loop
def test_the_launch_rule_is_the_kernels():
    with open(os.path.join(CSRC, "lt_device.hpp")) as f:
        dev = f.read()
    with open(os.path.join(CSRC, "lt_query.hip")) as f:
        q = f.read()

    def const(text, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))

    assert const(dev, "kBlock") == me.BLOCK
    assert const(dev, "kTraceRows") + const(dev, "kTraceStage") == me.STAGE_ROWS
    assert const(q, "kQueryClaim") == me.CLAIM_MAX
    body = q[q.index("static void launch_hits_one"):q.index("hipError_t launch_hits(")]
    assert "const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);" in body
    assert "const uint32_t rows = (uint32_t)(kTraceRows + kTraceStage) + 2u * p.maxHits;" in body
    m = re.search(r"fit = (\d+)u \* 1024u / \(rows \* kBlock \* \(uint32_t\)sizeof\(int\)\), perCu = fit < (\d+)u \? fit : (\d+)u;", body)
    assert m and int(m.group(1)) * 1024 == me.LDS_PER_CU and int(m.group(2)) == int(m.group(3)) == me.WAVES_PER_CU
    assert "const uint32_t resident = cuCount * perCu;" in body and "const dim3 grid(chunks < resident ? chunks : resident);" in body
    kernel = q[q.index("void lt_query_hits_kernel"):q.index("namespace lt_query {")]
    assert "const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;" in kernel
    assert ("const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kQueryClaim ? (uint32_t)kQueryClaim : share);"
            in kernel)
    # the rule on a chip of 256 CUs: 32 waves per CU for the count, 17 for lists of 8
    assert me.hits_launch(2577, 0, 256) == (41, 64) and me.hits_launch(4097, 8, 256) == (65, 64)
    assert me.hits_launch(10 ** 7, 0, 256) == (8192, 256) and me.hits_launch(10 ** 7, 8, 256) == (4352, 512)
    assert me.claim_sizes(0, 256) == (4_194_304, me.claim_sizes(0, 256)[1], 16_777_216 + 17)
    assert me.claim_sizes(8, 256) == (2_228_224, me.claim_sizes(8, 256)[1], 8_912_896 + 17)
    for k in (0, 8):
        for cu in (64, 256, 304):
            a, b, c = me.claim_sizes(k, cu)
            assert a < b < c and 128 < me.hits_launch(b, k, cu)[1] < 512
            # every size leaves the copies of the 2577-ray batch out of step with the lanes and the eighths
            assert all(n % 2577 and n % 64 for n in (b, c))
    assert len(mh.sheet_rays()[0]) == 2577 == 64 * 40 + 17


# ------------------------------------------------------------------------------------------------------------ 6: small pins
def test_odd_ignore_values_name_no_primitive():
    s = mh.sheets_scene()
    rays, cat = mh.sheet_rays()
    through = rays[cat == "through"][:32]
    p = mh.Peeler(s)
    want = [p.peel(r, po.ACCUMULATOR) for r in through]
    vals = me.odd_ignore_values(s.n_prims)
    assert vals == (936, 937, 2 ** 31 - 1, -2, -2 ** 31)
    for v in vals:
        r = me.with_ignore(through, v)
        assert (r[:, 7].view(np.int32) == v).all() and r[:, :7].tobytes() == through[:, :7].tobytes()
        assert [p.peel(x, po.ACCUMULATOR) for x in r] == want, v


def test_the_twice_named_leaves():
    s, nodes, prims, homes = me.twice_named_scene()
    s0 = mh.sheets_scene()
    nv, nv0 = s.node_view, s0.node_view
    assert len(nodes) >= 20 and (nv["offset"][nodes] == prims).all() and (nv0["offset"][nodes] != prims).all()
    assert (nv["offset"][homes] == prims).all() and (nv0["offset"][homes] == prims).all() and not set(homes) & set(nodes)
    leaves = np.flatnonzero(nv["primitiveCount"] != 0)
    named, times = np.unique(nv["offset"][leaves], return_counts=True)
    assert set(named[times == 2]) == set(prims) and times.max() == 2 and len(named) == s.n_prims - len(nodes)
    # the own hierarchy is built, its 4-wide groups are refused: the scene gets no own tree
    h, own, _ = C.own_hierarchy(nv, s.n_prims)
    assert h > 0
    with pytest.raises(C.LensTraceError):
        C.own_wide(own, s.n_prims)
    rays = mh.sheet_rays()[0]
    seqs = mh.sequences("twice_named", s, rays, po.ACCUMULATOR)
    sure, possible = me.twice_named_reach(rays, seqs)
    short = (sure > 0) & (mh.expected_counts(seqs) + possible <= 8)          # their K = 8 lists must hold the repeat
    print("rays that report a primitive twice for sure:", (sure > 0).sum(), "of them with a list that holds it all:", short.sum(),
          "possibly:", (possible > 0).sum())
    assert (sure <= possible).all() and (sure > 0).sum() >= 32 and short.sum() >= 8 and possible.max() <= len(nodes)
    # a primitive appears once in a peel sequence, however many leaves name it
    assert all(len({h[1] for h in q}) == len(q) for q in seqs)
