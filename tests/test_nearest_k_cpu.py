"""No GPU: lt_hip_nearest_k as far as it can be checked without one.

1. the three symbols are declared, exported and loadable, the descriptor's layout matches the header, a null context is an
   invalid argument, the host form's errors write nothing;
2. the host form (lt_hip_nearest_k_host: lt_nearest.hpp's list and counter in C++) equals tests/nearest_k.py's numpy model word
   for word on every point family of the base scene, a height-field wall and the twelve-triangle fan, for K = 1, 3, 8 and the
   count; K = 1 is lt_hip_nearest_points_host; the first 3 of K = 8 are K = 3; the count is the model's and covers the records;
3. the families are not vacuous -- counted from the model alone: ties across a list's end, sequences longer than 8 and shorter
   than K, twelve equal d2;
4. the pruning inequality for the K-th entry: with boxes quantised by the build's own arithmetic, no group slot whose bound is
   above the model's K-th d2 has a leaf beneath it whose candidate is one of the first K."""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import synth
from lens_trace_amd.renderer import HIT_DTYPE, POINT_DTYPE, make_points, nearest_k_host, nearest_points_host
from tests import nearest as nr
from tests import nearest_k as nk
from tests import query_edges as qe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lt_hip_nearest_k", "lt_hip_nearest_k_device", "lt_hip_nearest_k_host")
KS = (1, 3, 8)
F32 = np.float32
SENTINEL = 0x5a5a5a5a


# ------------------------------------------------------------------------------------------------------------- 1: the ABI
def test_the_three_symbols_are_declared_exported_and_loadable():
    L = C.load()
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lt_hip_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in C.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) in (6, 7, 9)
    assert L.lt_hip_abi_version() == 4


def test_the_descriptor_matches_the_header():
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    assert re.search(r"typedef struct lt_hip_nearest_k_desc \{\s*uint32_t struct_size;[^}]*uint32_t flags;[^}]*int32_t kind;[^}]*uint32_t max_k;[^}]*\} lt_hip_nearest_k_desc;", header)
    for name, value in (("LT_NEAREST_FIRST_K", C.NEAREST_FIRST_K), ("LT_NEAREST_COUNT", C.NEAREST_COUNT), ("LT_NEAREST_MAX_K", C.NEAREST_MAX_K)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    assert (C.NEAREST_FIRST_K, C.NEAREST_COUNT, C.NEAREST_MAX_K) == (0, 1, 8)
    D = C.NearestKDesc
    assert ctypes.sizeof(D) == 16 and [getattr(D, f).offset for f in ("struct_size", "flags", "kind", "max_k")] == [0, 4, 8, 12]
    assert ctypes.sizeof(C.TraceHit) == 16 == HIT_DTYPE.itemsize and ctypes.sizeof(C.Point) == 16 == POINT_DTYPE.itemsize


def desc(kind=C.NEAREST_FIRST_K, max_k=2, flags=0, size=ctypes.sizeof(C.NearestKDesc)):
    return ctypes.byref(C.NearestKDesc(size, flags, kind, max_k))


def test_a_null_context_is_an_invalid_argument_and_writes_nothing():
    L = C.load()
    out = np.full(16, SENTINEL, dtype=np.uint32)
    pts = make_points(np.zeros((2, 3)))
    O, P = (x.ctypes.data_as(ctypes.c_void_p) for x in (out, pts))
    assert L.lt_hip_nearest_k(None, desc(), P, 2, O, out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_nearest_k_device(None, desc(), P, 2, O, out.nbytes, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (out == SENTINEL).all()


def test_the_host_forms_errors_write_nothing():
    L = C.load()
    s = nr.hand_made()
    out = np.full(16, SENTINEL, dtype=np.uint32)
    pts = make_points(np.zeros((2, 3)))
    vp = ctypes.c_void_p
    N, Pr, P, O = (x.ctypes.data_as(vp) for x in (s.nodes, s.prims, pts, out))
    nb, pb = s.nodes.nbytes, s.prims.nbytes
    f = L.lt_hip_nearest_k_host
    INVALID = C.LT_ERR_INVALID_ARGUMENT
    assert f(N, nb, Pr, pb, None, P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(size=12), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(flags=1), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(kind=2), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(kind=-1), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(max_k=0), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(max_k=9), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(C.NEAREST_COUNT, 1), P, 2, O, 64) == INVALID
    assert f(None, nb, Pr, pb, desc(), P, 2, O, 64) == INVALID
    assert f(N, nb, None, pb, desc(), P, 2, O, 64) == INVALID
    assert f(N, nb - 1, Pr, pb, desc(), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb - 1, desc(), P, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), None, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), P, 2, None, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), P, 2 ** 32, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), P, 2, O, 63) == C.LT_ERR_BUFFER_TOO_SMALL             # 16 max_k n = 64
    assert f(N, nb, Pr, pb, desc(C.NEAREST_COUNT, 0), P, 2, O, 7) == C.LT_ERR_BUFFER_TOO_SMALL    # 4 n = 8
    assert f(N, nb, Pr, 76, desc(), P, 2, O, 64) == C.LT_ERR_BAD_SCENE                    # the second leaf's offset lies outside prims
    assert (out == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(), None, 0, None, 0) == 0
    assert f(N, nb, Pr, pb, desc(C.NEAREST_COUNT, 0), P, 2, O, 8) == 0 and (out[:2] == 2).all() and (out[2:] == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(), P, 2, O, 64) == 0 and (out != SENTINEL).all()
    with pytest.raises(ValueError):
        nearest_k_host(s, pts, k=9)
    with pytest.raises(ValueError):
        nearest_k_host(s, pts, k=0)


# ------------------------------------------------------------------------------------------------------------- the fixtures
@pytest.fixture(scope="module")
def cases():
    """name -> (scene, records of every family concatenated, the model's sequences): computed once."""
    scenes = {"base": qe.base_scene(0), "wall16": synth.heightfield_wall(16), "fan12": nk.fan12()}
    out = {}
    for i, (name, s) in enumerate(scenes.items()):
        pts = np.concatenate(list(nk.families(s, seed=i).values()))
        out[name] = (s, pts, nk.sequences(s, pts))
    return out


# ------------------------------------------------------------------------------------------------------------- 2: the host form
def test_the_host_form_equals_the_model(cases):
    for name, (s, pts, m) in cases.items():
        got = {}
        for k in KS:
            got[k] = nearest_k_host(s, pts, k=k)
            want = m.records(k)
            assert got[k].shape == (len(pts), k) and got[k].dtype == HIT_DTYPE
            bad = nk.same(got[k], want)
            assert len(bad) == 0, (name, k, len(bad), bad[:5], pts[bad[:3] // k], got[k].reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])
        count = nearest_k_host(s, pts, count=True)
        assert count.shape == (len(pts),) and count.dtype == np.uint32
        assert np.array_equal(count, m.count), (name, np.flatnonzero(count != m.count)[:5])
        # K = 1 is the nearest-point query; the first 3 of 8 are K = 3; the count covers the records
        assert len(nr.same(got[1].reshape(-1), nearest_points_host(s, pts))) == 0, name
        assert len(nk.same(got[8][:, :3], got[3])) == 0, name
        assert (count >= (got[8]["prim"] >= 0).sum(axis=1)).all(), name
        assert np.array_equal(np.minimum(count, 8), (got[8]["prim"] >= 0).sum(axis=1)), name
        # unused slots: max_d2's bits, -1, +0, +0
        unused = got[8]["prim"] < 0
        assert np.array_equal(got[8]["t"].view(np.uint32)[unused], np.broadcast_to(pts[:, 3].view(np.uint32)[:, None], unused.shape)[unused])
        assert (got[8]["u"].view(np.uint32)[unused] == 0).all() and (got[8]["v"].view(np.uint32)[unused] == 0).all()
        # POINT_DTYPE in, (n, 3) + max_d2 in: the same call
        assert len(nk.same(nearest_k_host(s, pts.view(POINT_DTYPE).reshape(-1), k=3), got[3])) == 0
        assert len(nk.same(nearest_k_host(s, pts[:, 0:3], k=3, max_d2=pts[:, 3]), got[3])) == 0


def test_the_order_of_the_records(cases):
    """ascending d2, ascending offset among equal d2 -- read off the host form's records, not the model's."""
    for name, (s, pts, m) in cases.items():
        got = nearest_k_host(s, pts, k=8)
        have = got["prim"][:, 1:] >= 0
        a, b = got["t"][:, :-1], got["t"][:, 1:]
        assert ((a < b) | ((a == b) & (got["prim"][:, :-1] < got["prim"][:, 1:])))[have].all(), name
        assert (got["t"][got["prim"] >= 0] < np.broadcast_to(pts[:, 3:4], got.shape)[got["prim"] >= 0]).all(), name


# ------------------------------------------------------------------------------------------------------------- 3: non-vacuity
def test_the_families_are_not_vacuous(cases):
    straddle = {k: 0 for k in KS}
    longer = twelve = 0
    short = {k: 0 for k in KS}
    for name, (s, pts, m) in cases.items():
        for k in KS:
            # a tie across the list's end: entries K - 1 and K both exist and have equal d2
            straddle[k] += int(((m.prim[:, k] >= 0) & (m.d2[:, k - 1] == m.d2[:, k])).sum())
            short[k] += int(((m.count < k) & ~nr.no_walk(pts)).sum())
        longer += int((m.count > 8).sum())
        twelve += int((m.ties >= 12).sum())
    assert sum(straddle.values()) >= 64 and min(straddle.values()) >= 64, straddle
    assert longer >= 64, longer
    assert min(short[3], short[8]) >= 64, short
    assert twelve >= 1, twelve


def test_the_fan_ties_wider_than_the_list():
    s = nk.fan12()
    at = np.concatenate([nk.FAN_VERTEX, F32([np.inf])])[None]
    m = nk.sequences(s, at)
    assert m.count[0] == 12 and (m.d2[0, :12].view(np.uint32) == 0).all()          # d2 == +0 twelve times
    assert np.array_equal(m.prim[0, :12], np.arange(12))
    pv = s.prim_view
    for corner in ("positionA", "positionB", "positionC"):                         # the vertex takes turns: four triangles each
        assert (pv[corner] == nk.FAN_VERTEX).all(axis=1).sum() == 4, corner
    got = nearest_k_host(s, at, k=8)
    assert np.array_equal(got["prim"][0], np.arange(8)) and (got["t"].view(np.uint32) == 0).all()
    assert nearest_k_host(s, at, count=True)[0] == 12
    off = at.copy()
    off[0, 0] += F32(2.0 ** -10)
    m = nk.sequences(s, off)
    d = m.d2[0, :12]
    assert m.count[0] == 12 and len(np.unique(d)) < 12 and (np.diff(d) >= 0).all()      # bit-equal d2 off the vertex too
    assert len(nk.same(nearest_k_host(s, off, k=8), m.records(8))) == 0


# ------------------------------------------------------------------------------------------------------------- 4: pruning
def test_the_pruning_inequality_for_the_kth_entry(cases):
    """The walk drops a slot once its bound is above the K-th entry's d2 (KList::reaches).  With the build's own quantised boxes:
    no slot whose bound is > the model's K-th d2 has a leaf beneath it whose candidate is one of the model's first K -- for the
    final K-th d2, which is <= every K-th d2 the walk holds on its way.  And while the list is not full: no slot whose bound is
    >= max_d2 has an accepted candidate beneath it.  The group tree is rebuilt from the links alone."""
    checked = 0
    for name, (s, pts, m) in cases.items():
        h, own, _ = C.own_hierarchy(s.node_view, s.n_prims)
        assert h >= 0, name
        _, O, S, slots = C.own_wide(own, s.n_prims)
        groups = len(slots)
        off, lo, hi = nr.leaves(s)
        leaf_of = {int(o): k for k, o in enumerate(off)}
        walk = np.flatnonzero(~nr.no_walk(pts))
        walk = walk[np.random.default_rng(12).permutation(len(walk))[:1200]]
        P = pts[walk, 0:3]
        bound = nr.slot_bound(slots["q"][None].astype(np.int64), O, S, P[:, None, None, :])   # [points, groups, 4]
        first = np.zeros((len(walk), len(off), len(KS)), dtype=bool)            # leaf is among the point's first K
        rows = np.arange(len(walk))
        for j, k in enumerate(KS):
            for e in range(k):
                leaf = m.leaf[walk, e]
                first[rows[leaf >= 0], leaf[leaf >= 0], j] = True
        accepted = np.zeros((len(walk), len(off)), dtype=bool)
        A, e1, e2 = nr.traversal_triangles(s, off)
        t, _, _, _ = nr.tri(P[:, None], A[None], e1[None], e2[None])
        with np.errstate(invalid="ignore"):
            accepted = nr.candidate_d2(t, nr.box_d2(P[:, None], lo[None], hi[None])).astype(F32) < pts[walk, 3:4]
        assert np.array_equal(accepted.sum(axis=1), m.count[walk])
        # the K-th d2 where the list ends full, else max_d2 (the list never fills)
        full = np.stack([m.prim[walk, k - 1] >= 0 for k in KS], axis=1)
        kth = np.stack([m.d2[walk, k - 1] for k in KS], axis=1)
        empty = 0x80000000 | (groups + s.n_prims)
        beneath = [None] * groups
        for gidx in range(groups - 1, -1, -1):
            mine = []
            for c in range(4):
                link = int(slots["link"][gidx, c])
                if link == empty:
                    continue
                sub = [leaf_of[(link & 0x7fffffff) - groups]] if link & 0x80000000 else beneath[link]
                b = bound[:, gidx, c]
                for j, k in enumerate(KS):
                    holds = first[:, sub, j].any(axis=1)
                    with np.errstate(invalid="ignore"):
                        dropped = np.where(full[:, j], b > kth[:, j], ~(b < pts[walk, 3]))
                    assert not (dropped & holds).any(), (name, gidx, c, k)
                # the count: a slot is dropped iff its bound is not below max_d2
                with np.errstate(invalid="ignore"):
                    assert not (~(b < pts[walk, 3]) & accepted[:, sub].any(axis=1)).any(), (name, gidx, c)
                checked += len(walk) * len(sub)
                mine += sub
            beneath[gidx] = mine
        assert sorted(beneath[0]) == list(range(len(off))), name
    assert checked > 10 ** 6
