"""No GPU: lt_hip_nearest_points as far as it can be checked without one.

1. the three symbols are declared, exported and loadable, the record layouts match the header, a null context is an invalid
   argument and writes nothing;
2. the host form (lt_hip_nearest_points_host: lt_nearest.hpp's functions in C++) equals tests/nearest.py's numpy model word for
   word on every point family of every scene;
3. the families are not vacuous -- counted from the model alone: ties between primitives settled by the lower offset, vertex,
   edge and face results, misses caused by max_d2, NaN candidates;
4. the model agrees with a float64 computation by another method within C_BOUND * 2^-24 * R^2;
5. the pruning inequality: with boxes quantised by the build's own arithmetic, the bound of every group slot is <= the box
   distance of every leaf beneath it, as floats."""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import synth
from lens_trace_amd.renderer import HIT_DTYPE, POINT_DTYPE, make_points, nearest_points_host
from tests import nearest as nr
from tests import query_edges as qe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lt_hip_nearest_points", "lt_hip_nearest_points_device", "lt_hip_nearest_points_host")
F32 = np.float32
# The largest |d2_32 - d2_64| / (2^-24 R^2) measured over these fixtures (test_the_model_against_float64 prints it) and the bound
# asserted: twice that -- the number of operations is fixed, so other seeds stay within a factor of two.
C_MEASURED = 3.483          # heightfield_wall(16); the other scenes: 1.9 .. 3.1
C_BOUND = 2.0 * C_MEASURED


# ------------------------------------------------------------------------------------------------------------- 1: the ABI
def test_the_three_symbols_are_declared_exported_and_loadable():
    L = C.load()
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lt_hip_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in C.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) in (6, 7, 8)
    assert L.lt_hip_abi_version() == 4
    assert re.search(r"#define\s+LT_HIP_ABI_VERSION\s+4\b", header)


def test_record_layouts_match_the_header():
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    assert re.search(r"typedef struct lt_hip_point \{\s*float p\[3\];\s*float max_d2;\s*\} lt_hip_point;", header)
    assert re.search(r"typedef struct lt_hip_nearest_desc \{\s*uint32_t struct_size;[^}]*uint32_t flags;[^}]*\} lt_hip_nearest_desc;", header)
    assert ctypes.sizeof(C.Point) == 16 == POINT_DTYPE.itemsize and C.Point.p.offset == 0 and C.Point.max_d2.offset == 12
    assert POINT_DTYPE.names == ("p", "max_d2") and POINT_DTYPE.fields["max_d2"][1] == 12 and POINT_DTYPE["p"].shape == (3,)
    assert ctypes.sizeof(C.NearestDesc) == 8 and C.NearestDesc.struct_size.offset == 0 and C.NearestDesc.flags.offset == 4
    assert ctypes.sizeof(C.TraceHit) == 16 == HIT_DTYPE.itemsize
    p = make_points(np.arange(6).reshape(2, 3), [0.5, np.inf])
    assert p.shape == (2, 4) and p.dtype == F32 and np.array_equal(p.view(POINT_DTYPE)["max_d2"].reshape(-1), F32([0.5, np.inf]))
    assert np.array_equal(p.view(POINT_DTYPE)["p"].reshape(2, 3), np.arange(6, dtype=F32).reshape(2, 3))


def test_a_null_context_is_an_invalid_argument_and_writes_nothing():
    L = C.load()
    out = np.full(8, 0x5a5a5a5a, dtype=np.uint32)
    pts = make_points(np.zeros((2, 3)))
    O, P = (x.ctypes.data_as(ctypes.c_void_p) for x in (out, pts))
    d = C.NearestDesc(ctypes.sizeof(C.NearestDesc), 0)
    assert L.lt_hip_nearest_points(None, ctypes.byref(d), P, 2, O, out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_nearest_points_device(None, ctypes.byref(d), P, 2, O, out.nbytes, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (out == 0x5a5a5a5a).all()


def test_the_host_forms_errors_write_nothing():
    L = C.load()
    s = nr.hand_made()
    out = np.full(8, 0x5a5a5a5a, dtype=np.uint32)
    pts = make_points(np.zeros((2, 3)))
    vp = ctypes.c_void_p
    N, Pr, P, O = (x.ctypes.data_as(vp) for x in (s.nodes, s.prims, pts, out))
    f = L.lt_hip_nearest_points_host
    assert f(None, s.nodes.nbytes, Pr, s.prims.nbytes, P, 2, O, 32) == C.LT_ERR_INVALID_ARGUMENT
    assert f(N, s.nodes.nbytes, None, s.prims.nbytes, P, 2, O, 32) == C.LT_ERR_INVALID_ARGUMENT
    assert f(N, s.nodes.nbytes - 1, Pr, s.prims.nbytes, P, 2, O, 32) == C.LT_ERR_INVALID_ARGUMENT
    assert f(N, s.nodes.nbytes, Pr, s.prims.nbytes - 1, P, 2, O, 32) == C.LT_ERR_INVALID_ARGUMENT
    assert f(N, s.nodes.nbytes, Pr, s.prims.nbytes, None, 2, O, 32) == C.LT_ERR_INVALID_ARGUMENT
    assert f(N, s.nodes.nbytes, Pr, s.prims.nbytes, P, 2, None, 32) == C.LT_ERR_INVALID_ARGUMENT
    assert f(N, s.nodes.nbytes, Pr, s.prims.nbytes, P, 2 ** 32, O, 32) == C.LT_ERR_INVALID_ARGUMENT
    assert f(N, s.nodes.nbytes, Pr, s.prims.nbytes, P, 2, O, 31) == C.LT_ERR_BUFFER_TOO_SMALL
    assert f(N, s.nodes.nbytes, Pr, 76, P, 2, O, 32) == C.LT_ERR_BAD_SCENE          # the second leaf's offset lies outside prims
    assert (out == 0x5a5a5a5a).all()
    assert f(N, s.nodes.nbytes, Pr, s.prims.nbytes, None, 0, None, 0) == 0
    assert f(N, s.nodes.nbytes, Pr, s.prims.nbytes, P, 2, O, 32) == 0 and (out != 0x5a5a5a5a).any()


# ------------------------------------------------------------------------------------------------------------- the fixtures
@pytest.fixture(scope="module")
def cases():
    """name -> (scene, {family: records}, expected records and details of all of them concatenated): computed once."""
    base = qe.base_scene(0)
    scenes = {"base": base, "wall16": synth.heightfield_wall(16)}
    for name in ("tiny", "large", "far+", "nan_bound"):
        scenes[name] = qe.extreme_scene(base, name)[0]
    scenes["hand_made"] = nr.hand_made()
    scenes["overflow"] = nr.hand_made_overflow()
    out = {}
    for i, (name, s) in enumerate(scenes.items()):
        fam = nr.families(s, seed=i)
        pts = np.concatenate(list(fam.values()))
        want, info = nr.expected(s, pts, details=True)
        out[name] = (s, fam, pts, want, info)
    return out


# ------------------------------------------------------------------------------------------------------------- 2: the host form
def test_the_host_form_equals_the_model(cases):
    for name, (s, fam, pts, want, _) in cases.items():
        got = nearest_points_host(s, pts)
        bad = nr.same(got, want)
        assert len(bad) == 0, (name, len(bad), bad[:5], pts[bad[:3]], got[bad[:3]], want[bad[:3]])
        # records in, POINT_DTYPE in, (n, 3) + max_d2 in: the same call
        assert len(nr.same(nearest_points_host(s, pts.view(POINT_DTYPE).reshape(-1)), want)) == 0
        assert len(nr.same(nearest_points_host(s, pts[:, 0:3], pts[:, 3]), want)) == 0
        miss = want["prim"] < 0
        assert np.array_equal(got["t"].view(np.uint32)[miss], pts[miss, 3].view(np.uint32)) and (got["u"].view(np.uint32)[miss] == 0).all()


# ------------------------------------------------------------------------------------------------------------- 3: non-vacuity
def test_the_families_are_not_vacuous(cases):
    tied = nan = by_max = 0
    regions = np.zeros(3, dtype=np.int64)
    for name, (s, fam, pts, want, info) in cases.items():
        hit = want["prim"] >= 0
        tied += int((info["tied"] > 0).sum())
        regions += np.bincount(info["region"][hit], minlength=3)
        nan += int(info["nan"].sum())
        # a miss caused by max_d2: the point has a finite nearest d2, and max_d2 is a number it is not below
        with np.errstate(invalid="ignore"):
            by_max += int((~hit & np.isfinite(pts[:, 0:3]).all(axis=1) & np.isfinite(info["d2_inf"]) & ~(info["d2_inf"] < pts[:, 3])).sum())
        if name in ("base", "wall16"):
            assert hit.mean() > 0.5, name
    assert tied >= 32, tied
    assert (regions >= 32).all(), regions
    assert by_max >= 32, by_max
    assert nan >= 1, nan


def test_a_tie_reports_the_lower_offset(cases):
    s, fam, pts, want, info = cases["base"]
    off, _, _ = nr.leaves(s)
    t = np.flatnonzero(info["tied"] > 0)
    assert len(t) >= 32
    pairs = set(qe.bit_equal_pairs(s).tolist())
    both = [i for i in t if int(want["prim"][i]) in pairs]
    assert len(both) >= 16
    key = np.ascontiguousarray(qe.corners(s).astype(F32)).view(np.uint8).reshape(s.n_prims, -1)
    for i in both[:16]:
        twins = np.flatnonzero((key == key[want["prim"][i]]).all(axis=1))
        assert want["prim"][i] == twins.min() and len(twins) > 1


# ------------------------------------------------------------------------------------------------------------- 4: float64
def ratio_against_float64(s, pts, want, info):
    """|d2_32 - d2_64| / (2^-24 R^2) of every hit: d2_64 by nearest.distance64 on the winner's traversal triangle, lifted to the
    leaf's box distance as the definition lifts it; R^2 the largest squared distance from P to the triangle's vertices."""
    hit = np.flatnonzero(want["prim"] >= 0)
    off, lo, hi = nr.leaves(s)
    leaf = info["cand"][hit]
    A, e1, e2 = (x.astype(np.float64) for x in nr.traversal_triangles(s, off[leaf]))
    P = pts[hit, 0:3].astype(np.float64)
    d64 = nr.distance64(P, A, e1, e2)
    g = np.maximum(np.maximum(lo[leaf].astype(np.float64) - P, P - hi[leaf].astype(np.float64)), 0.0)
    d64 = np.maximum(d64, (g * g).sum(axis=1))
    R2 = np.max([((P - V) ** 2).sum(axis=1) for V in (A, A + e1, A + e2)], axis=0)
    with np.errstate(all="ignore"):
        r = np.abs(want["t"][hit].astype(np.float64) - d64) / (2.0 ** -24 * R2)
    return np.where(R2 > 0, r, 0.0), hit


def test_the_model_against_float64(cases):
    worst = 0.0
    for name, (s, fam, pts, want, info) in cases.items():
        if name == "overflow":
            continue                                   # (its needle's edges are not numbers)
        r, hit = ratio_against_float64(s, pts, want, info)
        assert len(r) >= 32 or name == "hand_made", name
        print("%-10s %5d hits, largest |d2_32 - d2_64| / (2^-24 R^2) = %.3f" % (name, len(r), r.max()))
        bad = np.flatnonzero(~(r <= C_BOUND))
        assert len(bad) == 0, (name, r.max(), pts[hit[bad[:3]]], want[hit[bad[:3]]])
        worst = max(worst, float(r.max()))
    print("worst ratio %.3f, asserted %.3f" % (worst, C_BOUND))


# ------------------------------------------------------------------------------------------------------------- 5: pruning
def test_the_pruning_inequality(cases):
    """slot bound <= box distance of every leaf beneath the slot, as floats, for the build's own quantised boxes: a group tree is
    rebuilt here from the links alone (a leaf link names its primitive offset, a group link its group), so nothing about the
    order of the slots is assumed."""
    checked = 0
    for name, (s, fam, pts, want, info) in cases.items():
        h, own, _ = C.own_hierarchy(s.node_view, s.n_prims)
        if h < 0:
            assert name in ("nan_bound", "overflow"), name       # (a NaN bound; bounds beyond 2^40)
            continue
        _, O, S, slots = C.own_wide(own, s.n_prims)
        groups = len(slots)
        off, lo, hi = nr.leaves(s)
        leaf_of = {int(o): k for k, o in enumerate(off)}
        rng = np.random.default_rng(11)
        P = pts[np.isfinite(pts[:, 0:3]).all(axis=1), 0:3]
        P = P[rng.permutation(len(P))[:2000]] if len(P) > 2000 else P
        if len(P) < 2000:                          # 2000 points per scene: the families' own and points around them
            lo0, hi0 = nr.root_box(s)
            with np.errstate(over="ignore"):
                more = (0.5 * (lo0 + hi0) + rng.uniform(-2, 2, (2000 - len(P), 3)) * 0.5 * (hi0 - lo0)).astype(F32)
            P = np.concatenate([P, more[np.isfinite(more).all(axis=1)]])
        lb = nr.box_d2(P[:, None, :], lo[None], hi[None])                      # [points, leaves]
        bound = nr.slot_bound(slots["q"][None].astype(np.int64), O, S, P[:, None, None, :])   # [points, groups, 4]
        empty = 0x80000000 | (groups + s.n_prims)
        # leaves beneath every group, children before parents: groups are numbered parents first
        beneath = [None] * groups
        for gidx in range(groups - 1, -1, -1):
            mine = []
            for k in range(4):
                link = int(slots["link"][gidx, k])
                if link == empty:
                    continue
                sub = [leaf_of[(link & 0x7fffffff) - groups]] if link & 0x80000000 else beneath[link]
                assert sub is not None and len(sub) > 0
                worst = lb[:, sub].min(axis=1)
                with np.errstate(invalid="ignore"):
                    assert (bound[:, gidx, k] <= worst).all(), (name, gidx, k)
                checked += len(P) * len(sub)
                mine += sub
            beneath[gidx] = mine
        assert sorted(beneath[0]) == list(range(len(off))), name
    assert checked > 10 ** 6
