"""No GPU: lt_hip_overlap_tris as far as it can be checked without one.

1. the three symbols are declared, exported and loadable, the record's layout matches the header, a null context is an invalid
   argument, the host form's errors write nothing, Python-level argument errors raise ValueError;
2. the host form (lt_hip_overlap_tris_host: lt_tritri.hpp in C++) equals tests/overlap_tris.py's numpy model word for word on
   every query family of the six scenes tests/test_gpu_overlap.py uses, for K = 1, 3, 8, the count and any;
3. the fixtures are not vacuous -- counted from the model alone, per scene; a query whose first vertex is a primitive's vertex
   bit for bit touches that primitive (family b); empty queries and the outside triangle of family g give -1 / 0;
4. the pruning rule: with boxes quantised by the build's own arithmetic, boxes_meet(qbox, slot box) holds on every slot above a
   touching leaf;
5. the accuracy of the 17-axis test against float64 on the same inputs.

   mu = the largest (gap / M) over the 17 axes in float64 (tests/overlap_tris.py, margins64: M is the sum of the magnitudes of
   the terms of the axis's expressions); the float32 and float64 verdicts agree wherever |mu| > c 2^-24.  Measured over base,
   wall16 and fan12 the smallest such c is 0.105 (the 16 x 16 wall; base 0.052, the fan 0.049); the test asserts twice that,
   c = 0.21.  The scenes at the magnitude limits take no part: their in-plane axes overflow or underflow by design.  (Below 1
   because M counts the operands of the differences A - P, Q - P, R - P, which are nearly exact where the triangles are near
   each other.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import synth
from lens_trace_amd.renderer import TRI_DTYPE, make_tris, overlap_tris_host
from tests import nearest as nr
from tests import nearest_k as nk
from tests import overlap as ov
from tests import overlap_tris as ot
from tests import query_edges as qe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lt_hip_overlap_tris", "lt_hip_overlap_tris_device", "lt_hip_overlap_tris_host")
SCENES = ("base", "wall16", "fan12", "tiny", "large", "far+")
ORDINARY = ("base", "wall16", "fan12")
KS = (1, 3, 8)
F32 = np.float32
SENTINEL = 0x5a5a5a5a
C_MEASURED, C_ASSERTED = 0.105, 0.21


# ------------------------------------------------------------------------------------------------------------- 1: the ABI
def test_the_three_symbols_are_declared_exported_and_loadable():
    L = C.load()
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lt_hip_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in C.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) in (6, 7, 9)
    assert L.lt_hip_abi_version() == 4


def test_the_record_matches_the_header():
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    assert re.search(r"typedef struct lt_hip_tri \{ float a\[3\]; uint32_t pad0; float b\[3\]; uint32_t pad1; float c\[3\]; uint32_t pad2; \} lt_hip_tri;",
                     header)
    assert ctypes.sizeof(C.Tri) == 48 == TRI_DTYPE.itemsize and (C.Tri.a.offset, C.Tri.b.offset, C.Tri.c.offset) == (0, 16, 32)
    assert [TRI_DTYPE.fields[k][1] for k in ("a", "b", "c")] == [0, 16, 32]
    t = make_tris([[1, 2, 3]], [[4, 5, 6]], [[7, 8, 9]])
    assert t.shape == (1, 12) and t.dtype == F32 and t.view(TRI_DTYPE)["c"].tolist() == [[[7.0, 8.0, 9.0]]]
    with pytest.raises(ValueError):
        make_tris([[1, 2, 3]], [[4, 5, 6]], [[7, 8]])


def desc(kind=C.OVERLAP_FIRST_K, max_k=2, flags=0, size=ctypes.sizeof(C.OverlapDesc)):
    return ctypes.byref(C.OverlapDesc(size, flags, kind, max_k))


def test_a_null_context_is_an_invalid_argument_and_writes_nothing():
    L = C.load()
    out = np.full(16, SENTINEL, dtype=np.uint32)
    tr = make_tris(np.zeros((2, 3)), np.ones((2, 3)), np.ones((2, 3)))
    O, T = (x.ctypes.data_as(ctypes.c_void_p) for x in (out, tr))
    assert L.lt_hip_overlap_tris(None, desc(), T, 2, O, out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_overlap_tris_device(None, desc(), T, 2, O, out.nbytes, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (out == SENTINEL).all()


def test_the_host_forms_errors_write_nothing():
    L = C.load()
    s = nr.hand_made()
    out = np.full(16, SENTINEL, dtype=np.uint32)
    big = np.array([[-40.0, -40.0, -40.0], [40.0, -40.0, 40.0], [0.0, 80.0, 0.0]])
    both = ot.sequences(s, make_tris(big[None, 0], big[None, 1], big[None, 2]))
    tr = np.repeat(both.tris, 2, axis=0)
    vp = ctypes.c_void_p
    N, Pr, T, O = (x.ctypes.data_as(vp) for x in (s.nodes, s.prims, tr, out))
    nb, pb = s.nodes.nbytes, s.prims.nbytes
    f = L.lt_hip_overlap_tris_host
    INVALID = C.LT_ERR_INVALID_ARGUMENT
    COUNT, ANY = C.OVERLAP_COUNT, C.OVERLAP_ANY
    assert f(N, nb, Pr, pb, None, T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(size=12), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(flags=1), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(kind=3), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(kind=-1), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(max_k=0), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(max_k=9), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(COUNT, 1), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(ANY, 1), T, 2, O, 64) == INVALID
    assert f(None, nb, Pr, pb, desc(), T, 2, O, 64) == INVALID
    assert f(N, nb, None, pb, desc(), T, 2, O, 64) == INVALID
    assert f(N, nb - 1, Pr, pb, desc(), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb - 1, desc(), T, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), None, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), T, 2, None, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), T, 2 ** 32, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), T, 2, O, 15) == C.LT_ERR_BUFFER_TOO_SMALL                 # 4 max_k n = 16
    assert f(N, nb, Pr, pb, desc(COUNT, 0), T, 2, O, 7) == C.LT_ERR_BUFFER_TOO_SMALL          # 4 n = 8
    assert f(N, nb, Pr, pb, desc(ANY, 0), T, 2, O, 7) == C.LT_ERR_BUFFER_TOO_SMALL
    assert f(N, nb, Pr, 76, desc(), T, 2, O, 64) == C.LT_ERR_BAD_SCENE                        # the second leaf's offset lies outside prims
    assert (out == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(), None, 0, None, 0) == 0
    assert f(N, nb, Pr, pb, desc(COUNT, 0), T, 2, O, 8) == 0 and (out[:2] == both.count[0]).all() and (out[2:] == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(ANY, 0), T, 2, O, 8) == 0 and (out[:2] == both.any[0]).all() and (out[2:] == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(), T, 2, O, 16) == 0 and out[:4].view(np.int32).tolist() == both.first(2)[0].tolist() * 2 and (out[4:] == SENTINEL).all()
    for bad in (dict(k=9), dict(k=0), dict(k=2, count=True), dict(count=True, any=True)):
        with pytest.raises(ValueError):
            overlap_tris_host(s, tr, **bad)
    with pytest.raises(ValueError):
        overlap_tris_host(s, tr[:, :8])
    with pytest.raises(ValueError):
        overlap_tris_host(s, tr.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------- the fixtures
def scene_of(base, name):
    if name == "base":
        return base
    if name == "wall16":
        return synth.heightfield_wall(16)
    if name == "fan12":
        return nk.fan12()
    return qe.extreme_scene(base, name)[0]


@pytest.fixture(scope="module")
def cases():
    """name -> (scene, the families, their records concatenated, the model's sequences): computed once."""
    base = qe.base_scene(0)
    out = {}
    for i, name in enumerate(SCENES):
        s = scene_of(base, name)
        fam = ot.families(s, seed=i)
        tr = np.concatenate(list(fam.values()))
        out[name] = (s, fam, tr, ot.sequences(s, tr, want_touch=True))
    return out


def spans(fam):
    """name -> slice of the family in the concatenated batch."""
    out, at = {}, 0
    for name, rec in fam.items():
        out[name] = slice(at, at + len(rec))
        at += len(rec)
    return out


def own_touch(s, fam, m, name):
    """Per query of family `name`: whether it touches the primitive it was made from."""
    off, _, _ = nr.leaves(s)
    leaf_of = {int(o): k for k, o in enumerate(off)}
    sl = spans(fam)[name]
    leaf = np.array([leaf_of[int(p)] for p in fam.prims[name]])
    return m.touch[np.arange(sl.start, sl.stop), leaf]


# ------------------------------------------------------------------------------------------------------------- 2: the host form
def test_the_host_form_equals_the_model(cases):
    for name, (s, fam, tr, m) in cases.items():
        got = {}
        for k in KS:
            got[k] = overlap_tris_host(s, tr, k=k)
            assert got[k].shape == (len(tr), k) and got[k].dtype == np.int32
            bad = np.flatnonzero((got[k] != m.first(k)).any(axis=1))
            assert len(bad) == 0, (name, k, len(bad), bad[:5], tr[bad[:2]], got[k][bad[:2]], m.first(k)[bad[:2]])
        count = overlap_tris_host(s, tr, count=True)
        hit = overlap_tris_host(s, tr, any=True)
        assert count.shape == hit.shape == (len(tr),) and count.dtype == hit.dtype == np.uint32
        assert np.array_equal(count, m.count), (name, np.flatnonzero(count != m.count)[:5])
        assert np.array_equal(hit, m.any), (name, np.flatnonzero(hit != m.any)[:5])
        # the first 3 of 8 are K = 3; the count covers the offsets; ascending offsets; -1 in unused slots
        assert np.array_equal(got[8][:, :3], got[3]) and np.array_equal(got[8][:, :1], got[1]), name
        used = got[8] >= 0
        assert np.array_equal(np.minimum(count, 8), used.sum(axis=1)), name
        assert (got[8][~used] == -1).all() and (np.diff(used.astype(np.int8), axis=1) <= 0).all(), name
        assert (got[8][:, :-1] < got[8][:, 1:])[used[:, 1:]].all(), name
        # TRI_DTYPE in: the same call; the pads are ignored
        assert np.array_equal(overlap_tris_host(s, tr.view(TRI_DTYPE).reshape(-1), k=3), got[3])
        padded = tr.copy()
        padded[:, 3] = np.nan
        padded[:, 7] = np.inf
        padded.view(np.uint32)[:, 11] = 0xdeadbeef
        assert np.array_equal(overlap_tris_host(s, padded, count=True), count), name


# ------------------------------------------------------------------------------------------------------------- 3: non-vacuity
def test_the_fixtures_are_not_vacuous(cases):
    for name, (s, fam, tr, m) in cases.items():
        live = ~ot.empty(tr)
        if name in ORDINARY:
            assert (m.count > 8).sum() >= 64, name
            assert ((m.count == 0) & live).sum() >= 256, name
            assert ((m.count >= 1) & (m.count <= 7)).sum() >= 64, name
            own = own_touch(s, fam, m, "e_coplanar")
            assert own.sum() >= 16 and (~own).sum() >= 16, (name, int(own.sum()))
        else:
            assert ((m.count > 0) & live).sum() >= 32 and ((m.count == 0) & live).sum() >= 32, name
    alone = sum(m.alone for _, _, _, m in cases.values())
    assert (alone[:3] >= 64).all() and (alone[3:] >= 8).all(), alone       # every class of axis separates pairs that no other does


def test_a_first_vertex_on_a_primitives_vertex_touches_it(cases):
    """Family b: the primitive's own triangle as (A, B, C), (B, C, A), (C, A, B).  s0, s1 or s2 is 0 exactly, so both projection
    sets hold 0 on every axis; the leaf's box holds the vertex, so boxes_meet holds."""
    for name, (s, fam, tr, m) in cases.items():
        own = own_touch(s, fam, m, "b_own")
        assert len(own) >= 3 * 64 and own.all(), (name, np.flatnonzero(~own)[:5])
        sl = spans(fam)["b_own"]
        assert (overlap_tris_host(s, tr[sl], any=True) == 1).all(), name
        # ... and on every primitive of the scene, each vertex first
        off, _, _ = nr.leaves(s)
        V = qe.corners(s)[off]
        for r in range(3):
            q = make_tris(V[:, r], V[:, (r + 1) % 3], V[:, (r + 2) % 3])
            t = ot.sequences(s, q, want_touch=True)
            assert t.touch[np.arange(len(off)), np.arange(len(off))].all(), (name, r)


def test_empty_queries_and_the_outside_triangle_meet_nothing(cases):
    for name, (s, fam, tr, m) in cases.items():
        sl = spans(fam)
        dead = ot.empty(tr)
        assert dead[sl["h_empty"]].all() and dead.sum() == 27 == len(fam["h_empty"]), name
        cols = np.array([np.flatnonzero(~np.isfinite(r))[0] for r in fam["h_empty"]])
        assert sorted(set(cols.tolist())) == [0, 1, 2, 4, 5, 6, 8, 9, 10], name         # each of the nine coordinates
        g = sl["g_whole"]
        outside = g.start + 1
        assert m.count[g.start] >= 8 and m.count[outside] == 0, (name, m.count[g])
        lo, hi = nr.root_box(s)
        qlo, qhi = ot.query_box(tr[g])
        assert (qlo <= lo).all() and (qhi >= hi).all(), name                           # their boxes hold the whole scene
        pick = np.concatenate([np.flatnonzero(dead), [outside]])
        assert (overlap_tris_host(s, tr[pick], k=8) == -1).all() and (overlap_tris_host(s, tr[pick], count=True) == 0).all()
        assert (overlap_tris_host(s, tr[pick], any=True) == 0).all(), name


# ------------------------------------------------------------------------------------------------------------- 4: pruning
def test_every_slot_above_a_touching_leaf_meets_the_querys_box(cases):
    """The walk drops a slot whose put-back box fails boxes_meet against the query's box.  With the build's own quantised boxes
    and an exact float32 fma: no such slot has a touching leaf beneath it.  The group tree is rebuilt from the links alone."""
    checked = dropped_total = touching = 0
    for name, (s, fam, tr, m) in cases.items():
        h, own, _ = C.own_hierarchy(s.node_view, s.n_prims)
        assert h >= 0, name
        _, O, S, slots = C.own_wide(own, s.n_prims)
        groups = len(slots)
        off, _, _ = nr.leaves(s)
        leaf_of = {int(o): k for k, o in enumerate(off)}
        assert len(leaf_of) == len(off), name           # an own tree's scene names every primitive once
        qlo, qhi = ot.query_box(tr)
        slo, shi = ov.slot_box(slots["q"].astype(np.int64), O, S)                       # [groups, 4, 3]
        meets = ov.boxes_meet(qlo[:, None, None], qhi[:, None, None], slo[None], shi[None])   # [queries, groups, 4]
        touching += int(m.touch.sum())
        empty = 0x80000000 | (groups + s.n_prims)
        beneath = [None] * groups
        for gidx in range(groups - 1, -1, -1):
            mine = []
            for c in range(4):
                link = int(slots["link"][gidx, c])
                if link == empty:
                    continue
                sub = [leaf_of[(link & 0x7fffffff) - groups]] if link & 0x80000000 else beneath[link]
                dropped = ~meets[:, gidx, c]
                assert not (dropped & m.touch[:, sub].any(axis=1)).any(), (name, gidx, c)
                dropped_total += int(dropped.sum())
                checked += len(tr) * len(sub)
                mine += sub
            beneath[gidx] = mine
        assert sorted(beneath[0]) == list(range(len(off))), name
    assert checked > 10 ** 6 and dropped_total > 10 ** 5 and touching > 5000


# ------------------------------------------------------------------------------------------------------------- 5: accuracy
def test_the_verdict_against_float64(cases):
    worst = {}
    for name in ORDINARY:
        s, fam, tr, m = cases[name]
        off, _, _ = nr.leaves(s)
        A, e1, e2 = nr.traversal_triangles(s, off)
        live = np.flatnonzero(~ot.empty(tr))
        P, Q, R = ot.vertices(tr)
        worst[name] = 0.0
        near = 0
        for a in range(0, len(live), 64):
            sel = live[a:a + 64]
            sep = ot.separated(P[sel, None], Q[sel, None], R[sel, None], A[None], e1[None], e2[None])
            mu = ot.margins64(P[sel, None], Q[sel, None], R[sel, None], A[None], e1[None], e2[None])
            differ = (sep[0] | sep[1] | sep[2] | sep[3] | sep[4]) != (mu > 0)
            near += int((np.abs(mu) <= 2.0 ** -20).sum())
            if differ.any():
                worst[name] = max(worst[name], float(np.abs(mu[differ]).max() / 2.0 ** -24))
        assert near >= 64, (name, near)      # pairs near the boundary exist: the bound is tried
    print("c per scene:", worst)
    c = max(worst.values())
    assert c <= C_ASSERTED, worst
    assert C_ASSERTED == pytest.approx(2 * C_MEASURED, rel=0.01)
