"""No GPU: lt_hip_overlap_boxes as far as it can be checked without one.

1. the three symbols are declared, exported and loadable, the records' layouts match the header, a null context is an invalid
   argument, the host form's errors write nothing;
2. the host form (lt_hip_overlap_boxes_host: lt_overlap.hpp in C++) equals tests/overlap.py's numpy model word for word on every
   box family of the six scenes tests/test_gpu_nearest_k.py uses, for K = 1, 3, 8, the count and any;
3. the families are not vacuous -- counted from the model alone: pairs that each class of axis separates alone, long, short and
   empty sequences, empty boxes; a point box on a primitive's vertex A touches that primitive;
4. the pruning rule: with boxes quantised by the build's own arithmetic, no group slot whose put-back box fails boxes_meet has a
   touching leaf beneath it;
5. the accuracy of the 13-axis test against float64 on the same inputs.

   mu = the largest (gap / M) over the 13 axes in float64 (tests/overlap.py, margins64: M is the sum of the magnitudes of the
   terms of the axis's expressions); the float32 and float64 verdicts agree wherever |mu| > c 2^-24.  Measured over the
   fixtures, the smallest such c is 0.184 (the 16 x 16 wall; base 0.061, fan 0, the scenes at 2^-40, 2^35 and 2^40 - 2^33: 0.036,
   0.055, 0.123); the test asserts twice that, c = 0.37.  (Below 1 because M counts the operands of the centring, |A| + |lo| +
   |hi|, whose difference -- A - c, nearly exact where the box is near the triangle -- is what the products see.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import synth
from lens_trace_amd.renderer import BOX_DTYPE, make_boxes, overlap_boxes_host
from tests import nearest as nr
from tests import nearest_k as nk
from tests import overlap as ov
from tests import query_edges as qe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lt_hip_overlap_boxes", "lt_hip_overlap_boxes_device", "lt_hip_overlap_boxes_host")
SCENES = ("base", "wall16", "fan12", "tiny", "large", "far+")
KS = (1, 3, 8)
F32 = np.float32
SENTINEL = 0x5a5a5a5a
C_MEASURED, C_ASSERTED = 0.184, 0.37


# ------------------------------------------------------------------------------------------------------------- 1: the ABI
def test_the_three_symbols_are_declared_exported_and_loadable():
    L = C.load()
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lt_hip_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in C.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) in (6, 7, 9)
    assert L.lt_hip_abi_version() == 4


def test_the_records_match_the_header():
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    assert re.search(r"typedef struct lt_hip_overlap_desc \{\s*uint32_t struct_size;[^}]*uint32_t flags;[^}]*int32_t kind;[^}]*uint32_t max_k;[^}]*\} lt_hip_overlap_desc;", header)
    assert re.search(r"typedef struct lt_hip_box \{ float lo\[3\]; uint32_t pad0; float hi\[3\]; uint32_t pad1; \} lt_hip_box;", header)
    for name, value in (("LT_OVERLAP_FIRST_K", C.OVERLAP_FIRST_K), ("LT_OVERLAP_COUNT", C.OVERLAP_COUNT), ("LT_OVERLAP_ANY", C.OVERLAP_ANY),
                        ("LT_OVERLAP_MAX_K", C.OVERLAP_MAX_K)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    assert (C.OVERLAP_FIRST_K, C.OVERLAP_COUNT, C.OVERLAP_ANY, C.OVERLAP_MAX_K) == (0, 1, 2, 8)
    D = C.OverlapDesc
    assert ctypes.sizeof(D) == 16 and [getattr(D, f).offset for f in ("struct_size", "flags", "kind", "max_k")] == [0, 4, 8, 12]
    assert ctypes.sizeof(C.Box) == 32 == BOX_DTYPE.itemsize and (C.Box.lo.offset, C.Box.hi.offset) == (0, 16)
    assert (BOX_DTYPE.fields["lo"][1], BOX_DTYPE.fields["hi"][1]) == (0, 16)
    b = make_boxes([[1, 2, 3]], [[4, 5, 6]])
    assert b.shape == (1, 8) and b.dtype == F32 and b.view(BOX_DTYPE)["hi"].tolist() == [[[4.0, 5.0, 6.0]]]


def desc(kind=C.OVERLAP_FIRST_K, max_k=2, flags=0, size=ctypes.sizeof(C.OverlapDesc)):
    return ctypes.byref(C.OverlapDesc(size, flags, kind, max_k))


def test_a_null_context_is_an_invalid_argument_and_writes_nothing():
    L = C.load()
    out = np.full(16, SENTINEL, dtype=np.uint32)
    bx = make_boxes(np.zeros((2, 3)), np.ones((2, 3)))
    O, B = (x.ctypes.data_as(ctypes.c_void_p) for x in (out, bx))
    assert L.lt_hip_overlap_boxes(None, desc(), B, 2, O, out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_overlap_boxes_device(None, desc(), B, 2, O, out.nbytes, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (out == SENTINEL).all()


def test_the_host_forms_errors_write_nothing():
    L = C.load()
    s = nr.hand_made()
    out = np.full(16, SENTINEL, dtype=np.uint32)
    bx = make_boxes(np.full((2, 3), -4.0), np.full((2, 3), 4.0))
    vp = ctypes.c_void_p
    N, Pr, B, O = (x.ctypes.data_as(vp) for x in (s.nodes, s.prims, bx, out))
    nb, pb = s.nodes.nbytes, s.prims.nbytes
    f = L.lt_hip_overlap_boxes_host
    INVALID = C.LT_ERR_INVALID_ARGUMENT
    COUNT, ANY = C.OVERLAP_COUNT, C.OVERLAP_ANY
    assert f(N, nb, Pr, pb, None, B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(size=12), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(flags=1), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(kind=3), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(kind=-1), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(max_k=0), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(max_k=9), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(COUNT, 1), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(ANY, 1), B, 2, O, 64) == INVALID
    assert f(None, nb, Pr, pb, desc(), B, 2, O, 64) == INVALID
    assert f(N, nb, None, pb, desc(), B, 2, O, 64) == INVALID
    assert f(N, nb - 1, Pr, pb, desc(), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb - 1, desc(), B, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), None, 2, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), B, 2, None, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), B, 2 ** 32, O, 64) == INVALID
    assert f(N, nb, Pr, pb, desc(), B, 2, O, 15) == C.LT_ERR_BUFFER_TOO_SMALL                 # 4 max_k n = 16
    assert f(N, nb, Pr, pb, desc(COUNT, 0), B, 2, O, 7) == C.LT_ERR_BUFFER_TOO_SMALL          # 4 n = 8
    assert f(N, nb, Pr, pb, desc(ANY, 0), B, 2, O, 7) == C.LT_ERR_BUFFER_TOO_SMALL
    assert f(N, nb, Pr, 76, desc(), B, 2, O, 64) == C.LT_ERR_BAD_SCENE                        # the second leaf's offset lies outside prims
    assert (out == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(), None, 0, None, 0) == 0
    assert f(N, nb, Pr, pb, desc(COUNT, 0), B, 2, O, 8) == 0 and (out[:2] == 2).all() and (out[2:] == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(ANY, 0), B, 2, O, 8) == 0 and (out[:2] == 1).all() and (out[2:] == SENTINEL).all()
    assert f(N, nb, Pr, pb, desc(), B, 2, O, 16) == 0 and out[:4].tolist() == [0, 1, 0, 1] and (out[4:] == SENTINEL).all()
    for bad in (dict(k=9), dict(k=0), dict(k=2, count=True), dict(count=True, any=True)):
        with pytest.raises(ValueError):
            overlap_boxes_host(s, bx, **bad)
    with pytest.raises(ValueError):
        overlap_boxes_host(s, bx[:, :6])


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
        fam = ov.families(s, seed=i)
        bx = np.concatenate(list(fam.values()))
        out[name] = (s, fam, bx, ov.sequences(s, bx, want_touch=True))
    return out


# ------------------------------------------------------------------------------------------------------------- 2: the host form
def test_the_host_form_equals_the_model(cases):
    for name, (s, fam, bx, m) in cases.items():
        got = {}
        for k in KS:
            got[k] = overlap_boxes_host(s, bx, k=k)
            assert got[k].shape == (len(bx), k) and got[k].dtype == np.int32
            bad = np.flatnonzero((got[k] != m.first(k)).any(axis=1))
            assert len(bad) == 0, (name, k, len(bad), bad[:5], bx[bad[:2]], got[k][bad[:2]], m.first(k)[bad[:2]])
        count = overlap_boxes_host(s, bx, count=True)
        hit = overlap_boxes_host(s, bx, any=True)
        assert count.shape == hit.shape == (len(bx),) and count.dtype == hit.dtype == np.uint32
        assert np.array_equal(count, m.count), (name, np.flatnonzero(count != m.count)[:5])
        assert np.array_equal(hit, m.any), (name, np.flatnonzero(hit != m.any)[:5])
        # the first 3 of 8 are K = 3; the count covers the offsets; ascending offsets; -1 in unused slots
        assert np.array_equal(got[8][:, :3], got[3]) and np.array_equal(got[8][:, :1], got[1]), name
        used = got[8] >= 0
        assert np.array_equal(np.minimum(count, 8), used.sum(axis=1)), name
        assert (got[8][~used] == -1).all() and (np.diff(used.astype(np.int8), axis=1) <= 0).all(), name
        both = used[:, 1:]
        assert (got[8][:, :-1] < got[8][:, 1:])[both].all(), name
        # BOX_DTYPE in: the same call; the pads are ignored
        assert np.array_equal(overlap_boxes_host(s, bx.view(BOX_DTYPE).reshape(-1), k=3), got[3])
        padded = bx.copy()
        padded[:, 3] = np.nan
        padded.view(np.uint32)[:, 7] = 0xdeadbeef
        assert np.array_equal(overlap_boxes_host(s, padded, count=True), count), name


# ------------------------------------------------------------------------------------------------------------- 3: non-vacuity
def test_the_families_are_not_vacuous(cases):
    alone = np.zeros(3, dtype=np.int64)
    longer = zero = short = empties = 0
    for name, (s, fam, bx, m) in cases.items():
        e = ov.empty(bx)
        alone += m.alone
        longer += int((m.count > 8).sum())
        zero += int(((m.count == 0) & ~e).sum())
        short += int(((m.count >= 1) & (m.count <= 7)).sum())
        empties += int(e.sum())
        assert (m.count[e] == 0).all() and e[-len(fam["i_off"]) - len(fam["h_empty"]):-len(fam["i_off"])].all(), name
        whole = sum(len(fam[k]) for k in ("a_uniform", "b_on", "c_vertex_a", "d_grid", "e_slab", "f_corner"))
        assert (m.count[whole:whole + 2] == len(nr.leaves(s)[0])).all(), name         # the scene's box and +-2^100 touch every leaf
    assert (alone >= 64).all(), alone                 # box axes, plane, edge axes: each alone separates pairs
    assert longer >= 256 and zero >= 256 and short >= 64 and empties >= 32, (longer, zero, short, empties)


def test_a_point_box_on_vertex_a_touches_its_primitive(cases):
    """lo = hi = A: c = A, h = 0, v0 = 0, so d = r = 0 and every projection of v0 is 0 -- min(p) <= 0 <= max(p) on every axis."""
    for name, (s, fam, bx, m) in cases.items():
        off, _, _ = nr.leaves(s)
        pv = s.prim_view
        A = pv["positionA"][off].astype(F32)
        pts = make_boxes(A, A)
        t = ov.sequences(s, pts, want_touch=True)
        assert t.touch[np.arange(len(off)), np.arange(len(off))].all(), name
        got = overlap_boxes_host(s, pts, any=True)
        assert (got == 1).all(), name
        # ... and the batch's own point boxes are among the counted
        a0 = len(fam["a_uniform"]) + len(fam["b_on"])
        assert (m.count[a0:a0 + len(fam["c_vertex_a"])] >= 1).all(), name


def test_grid_cells_share_their_faces_bit_for_bit(cases):
    """The eight cells round a vertex: one corner of each is the vertex itself, so no box axis separates the vertex's primitives."""
    for name, (s, fam, bx, m) in cases.items():
        g = fam["d_grid"].reshape(-1, 8, 8)
        lo, hi = g[..., 0:3], g[..., 4:7]
        V = hi[:, 0]                                   # cell 0 lies below the vertex on every axis
        for ix in range(8):
            pick = np.array([(ix >> a) & 1 for a in range(3)], dtype=bool)
            assert np.array_equal(np.where(pick, lo[:, ix], hi[:, ix]).view(np.uint32), V.view(np.uint32)), (name, ix)


# ------------------------------------------------------------------------------------------------------------- 4: pruning
def test_no_dropped_slot_holds_a_touching_leaf(cases):
    """The walk drops a slot whose put-back box fails boxes_meet.  With the build's own quantised boxes and an exact float32 fma:
    no such slot has a touching leaf beneath it.  The group tree is rebuilt from the links alone."""
    checked = dropped_total = 0
    for name, (s, fam, bx, m) in cases.items():
        h, own, _ = C.own_hierarchy(s.node_view, s.n_prims)
        assert h >= 0, name
        _, O, S, slots = C.own_wide(own, s.n_prims)
        groups = len(slots)
        off, _, _ = nr.leaves(s)
        leaf_of = {int(o): k for k, o in enumerate(off)}
        assert len(leaf_of) == len(off), name           # an own tree's scene names every primitive once
        pick = np.random.default_rng(12).permutation(len(bx))[:1200]
        lo, hi = bx[pick, 0:3], bx[pick, 4:7]
        slo, shi = ov.slot_box(slots["q"].astype(np.int64), O, S)                       # [groups, 4, 3]
        meets = ov.boxes_meet(lo[:, None, None], hi[:, None, None], slo[None], shi[None])   # [boxes, groups, 4]
        touch = m.touch[pick]
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
                assert not (dropped & touch[:, sub].any(axis=1)).any(), (name, gidx, c)
                dropped_total += int(dropped.sum())
                checked += len(pick) * len(sub)
                mine += sub
            beneath[gidx] = mine
        assert sorted(beneath[0]) == list(range(len(off))), name
    assert checked > 10 ** 6 and dropped_total > 10 ** 5


# ------------------------------------------------------------------------------------------------------------- 5: accuracy
def test_the_verdict_against_float64(cases):
    worst = {}
    for name, (s, fam, bx, m) in cases.items():
        off, _, _ = nr.leaves(s)
        A, e1, e2 = nr.traversal_triangles(s, off)
        live = np.flatnonzero(~ov.empty(bx))
        worst[name] = 0.0
        near = 0
        for a in range(0, len(live), 128):
            sel = live[a:a + 128]
            lo, hi = bx[sel, None, 0:3], bx[sel, None, 4:7]
            box, plane, edge = ov.classes(lo, hi, A[None], e1[None], e2[None])
            mu = ov.margins64(lo, hi, A[None], e1[None], e2[None])
            differ = (box | plane | edge) != (mu > 0)
            near += int((np.abs(mu) <= 2.0 ** -20).sum())
            if differ.any():
                worst[name] = max(worst[name], float(np.abs(mu[differ]).max() / 2.0 ** -24))
        assert near >= 64 or name == "fan12", (name, near)      # pairs near the boundary exist: the bound is tried
    print("c per scene:", worst)
    c = max(worst.values())
    assert c <= C_ASSERTED, worst
    assert C_ASSERTED == pytest.approx(2 * C_MEASURED, rel=0.01)
