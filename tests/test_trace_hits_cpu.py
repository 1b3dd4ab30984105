"""CPU-side checks of the multi-hit query ABI (lt_hip_trace_hits / lt_hip_trace_hits_device) and of what tests/multihit.py claims
about its oracle, its scene and its ray batch.  No GPU."""
import ctypes
import re

import numpy as np

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import FLT_MAX, HIT_DTYPE, make_rays
from oracle import pyoracle as po
from tests import multihit as mh
from tests import query_edges as qe
from tests.test_trace_rays_cpu import HEADER


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_library_exports_the_multihit_entry_points():
    L = C.load()
    for name in ("lt_hip_trace_hits", "lt_hip_trace_hits_device"):
        assert name in C.EXPORTS
        assert re.search(r"^int\s+%s\s*\(" % name, HEADER, flags=re.M)
        assert getattr(L, name) is not None
    assert L.lt_hip_abi_version() == 4


def test_descriptor_layout_and_constants_match_the_header():
    D = C.MultiHitDesc
    assert ctypes.sizeof(D) == 24
    assert [getattr(D, k).offset for k in ("struct_size", "program", "kind", "flags", "max_hits", "reserved")] == [0, 4, 8, 12, 16, 20]
    body = re.search(r"typedef struct lt_hip_multihit_desc \{(.*?)\} lt_hip_multihit_desc;", HEADER, flags=re.S).group(1)
    assert re.findall(r"(?:u?int32_t)\s+(\w+);", body) == ["struct_size", "program", "kind", "flags", "max_hits", "reserved"]
    assert re.search(r"LT_TRACE_FIRST_K\s*=\s*0\s*,\s*LT_TRACE_COUNT\s*=\s*1", HEADER)
    assert (C.TRACE_FIRST_K, C.TRACE_COUNT) == (0, 1)
    m = re.search(r"#define\s+LT_TRACE_MAX_HITS\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == C.TRACE_MAX_HITS == 8
    # the existing query's descriptor and kinds are as they were
    assert ctypes.sizeof(C.TraceDesc) == 16 and (C.TRACE_CLOSEST, C.TRACE_ANY) == (0, 1)


def test_null_context_is_an_invalid_argument():
    L = C.load()
    d = C.MultiHitDesc(ctypes.sizeof(C.MultiHitDesc), C.PROGRAM_ACCUMULATOR, C.TRACE_FIRST_K, 0, 2, 0)
    rays = make_rays(np.zeros((2, 3)), np.ones((2, 3)))
    out = np.full((2, 2), 7, dtype=HIT_DTYPE)
    before = out.copy()
    assert L.lt_hip_trace_hits(None, ctypes.byref(d), rays.ctypes.data_as(ctypes.c_void_p), 2,
                               out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_trace_hits_device(None, ctypes.byref(d), None, 0, None, 0, None) == C.LT_ERR_INVALID_ARGUMENT
    assert out.tobytes() == before.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the oracle
def axis_ray(x, y, front=True, **kw):
    return make_rays([[x, y, -2.0 if front else 8.0]], [[0, 0, 1.0 if front else -1.0]], **kw)[0]


def test_peel_returns_the_sheets_in_order():
    s = mh.sheets_scene()
    sheet = mh.sheet_of(s)
    assert np.array_equal(np.bincount(sheet), [72, 72, 144] + [72] * 9)
    for front in (True, False):
        seq = mh.peel(s, axis_ray(0.3, -1.6, front))
        want = sorted(list(range(mh.SHEETS)) + [mh.DOUBLED], reverse=not front)
        assert [sheet[h[1]] for h in seq] == want
        t = np.array([h[0] for h in seq])
        assert (np.diff(t) >= 0).all() and len({h[1] for h in seq}) == len(seq)
        z = np.array(want) * mh.SPACING + mh.TILT * 0.3
        assert np.allclose(t, z + 2 if front else 8 - z, rtol=0, atol=1e-5)
    # tmax cuts the sequence; a NaN tmax accepts nothing
    assert len(mh.peel(s, axis_ray(0.3, -1.6, tmax=np.float32(2.0 + 0.75)))) == 2
    assert mh.peel(s, axis_ray(0.3, -1.6, tmax=np.float32(np.nan))) == []
    assert len(mh.peel(s, axis_ray(0.3, -1.6), limit=5)) == 5
    # a ray that starts inside a triangle's box beyond its plane hits it behind its origin: the reference has no t > 0 test
    seq = mh.peel(s, make_rays([[0.5, 0.25, 0.125 + 0.05]], [[0.1, 0.2, 1.0]])[0])
    assert seq[0][0] < 0 and sheet[seq[0][1]] == 0 and [sheet[h[1]] for h in seq[1:4]] == [1, 2, 2]


def test_the_doubled_sheet_ties_fall_in_the_references_traversal_order():
    """Of two bit-equal triangles the reference keeps the one whose leaf it reaches first: peeling must return that one first,
    and the other next with the same t, u and v."""
    s = mh.sheets_scene()
    dbl = set(mh.doubled_prims(s).tolist())
    assert len(dbl) == 2 * 2 * mh.CELLS * mh.CELLS
    # the reference's depth-first leaf order per direction-sign octant, from the host library (what SceneDev::rank8 holds)
    h, _, rank8 = C.own_hierarchy(s.node_view, s.n_prims, want_ranks=True)
    assert h > 0
    rng = np.random.default_rng(3)
    lower_first = []
    for _ in range(40):
        x, y = rng.uniform(-2.9, 2.9, 2)
        for front in (True, False):
            seq = mh.peel(s, axis_ray(x, y, front))
            pos = [j for j, h in enumerate(seq) if h[1] in dbl]
            assert pos == ([2, 3] if front else [9, 10]) and len(seq) == mh.SHEETS + 1
            a, b = seq[pos[0]], seq[pos[1]]
            assert a[0] == b[0] and a[2:] == b[2:] and a[1] != b[1]
            octant = 0 if front else 4
            assert rank8[a[1], octant] < rank8[b[1], octant]
            lower_first.append(a[1] < b[1])
    assert len(lower_first) == 80


def test_peel_limit_one_is_the_oracles_trace():
    s = mh.sheets_scene()
    rays, _ = mh.sheet_rays()
    for prog in (po.BASIC, po.BASIC_LIGHTING, po.ACCUMULATOR):
        for r in rays[::37]:
            ign = int(r[7:8].view(np.int32)[0])
            hit, prim, tuv = po.trace(s, np.float32([r[0], r[1], r[2], 1]), np.float32([r[4], r[5], r[6], 0]), prog, r[3],
                                      ign if ign >= 0 else None)
            seq = mh.peel(s, r, prog, 1)
            if hit:
                assert len(seq) == 1 and seq[0][1] == prim
                assert np.array_equal(np.float32([seq[0][0], seq[0][2], seq[0][3]]).view(np.uint32), tuv.view(np.uint32))
            else:
                assert seq == []


# ---------------------------------------------------------------------------------------------------------------- the batch
def test_the_batch_holds_what_it_claims():
    s = mh.sheets_scene()
    rays, cat = mh.sheet_rays()
    assert len(rays) == 64 * 40 + 17 and len(cat) == len(rays)
    for name in mh.CATEGORIES:
        assert (cat == name).sum() >= 64, name
    seqs = mh.sequences("sheets", s, rays, po.ACCUMULATOR)
    n = mh.expected_counts(seqs)
    assert (n > 8).sum() >= 64
    straddle = [len(q) > 3 and q[2][0] == q[3][0] for q in seqs]
    assert sum(straddle) >= 64
    assert (n[cat == "miss"] == 0).all() and (n[cat == "through"] >= mh.SHEETS + 1).all()
    # cheap and expensive rays side by side
    i = np.flatnonzero(cat == "miss")
    assert (cat[i + 1] == "through").all()
    # an ignoring ray would hit the primitive it ignores, and its sequence leaves it out
    p = mh.Peeler(s)
    for i in np.flatnonzero(cat == "ignore"):
        ign = int(rays[i, 7:8].view(np.int32)[0])
        free = rays[i].copy()
        free[7:8].view(np.int32)[0] = -1
        assert ign >= 0 and ign in [h[1] for h in p.peel(free, po.ACCUMULATOR)] and ign not in [h[1] for h in seqs[i]]
    t = rays[:, 3]
    assert (t[cat == "tmax_fltmax"] == np.float32(FLT_MAX)).all() and np.isposinf(t[cat == "tmax_inf"]).all()
    assert (t[cat == "tmax_zero"] == 0).all() and (t[cat == "tmax_negative"] < 0).all() and np.isnan(t[cat == "tmax_nan"]).all()
    assert (n[cat == "tmax_nan"] == 0).all() and (n[cat == "tmax_zero"] > 0).sum() >= 60 and (n[cat == "tmax_negative"] > 0).sum() >= 60
    b = cat == "tmax_between"
    assert ((n[b] > 0) & (n[b] < mh.SHEETS + 1)).all() and np.isfinite(t[b]).all()
    # the fallback rays have a zero or non-finite component; the axis rays too (their inverse direction is infinite)
    bad = ~qe.own_ok(rays)                                  # lt_query.hip: finite_ray && packet_ray_ok
    assert bad[cat == "fallback"].all() and bad[cat == "axis"].all() and not bad[cat == "through"].any()
    assert (n[cat == "fallback"] > 0).sum() >= 32
    # rays from inside the stack have hits on both sides of their origin
    tt = [np.array([h[0] for h in seqs[i]]) for i in np.flatnonzero(cat == "inside")]
    assert sum(1 for x in tt if (x < 0).any() and (x > 0).any()) >= 64
    # vertex and edge rays meet several triangles of a sheet at one t
    ties = [any(q[j][0] == q[j + 1][0] for j in range(len(q) - 1)) for q in seqs]
    assert np.array(ties)[cat == "axis"].sum() >= 64


def test_expected_records_pad_with_the_rays_own_tmax_bits():
    rays = np.array(make_rays(np.zeros((2, 3)), np.ones((2, 3))))
    rays[1, 3:4].view(np.uint32)[0] = 0x7fc12345
    rec = mh.expected_records([[(np.float32(1.5), 7, np.float32(0.25), np.float32(0.5))], []], rays, 2)
    assert rec.shape == (2, 2) and rec[0, 0].tolist() == (1.5, 7, 0.25, 0.5)
    assert rec[0, 1]["prim"] == -1 and rec[0, 1]["t"] == np.float32(FLT_MAX) and rec[0, 1]["u"] == 0
    assert rec["t"].view(np.uint32)[1].tolist() == [0x7fc12345] * 2 and (rec["prim"][1] == -1).all()


# ------------------------------------------------------------------------------------------- the wrappers' numpy ray batches
def test_ray_records_normalises_numpy_batches_and_refuses_the_rest():
    import pytest
    from lens_trace_amd.renderer import RAY_DTYPE, SHADE_RAY_DTYPE, make_shade_rays, ray_records
    rng = np.random.default_rng(3)
    n = 7
    packed = {"RAY_DTYPE": make_rays(rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), 9.0, np.arange(n)),
              "SHADE_RAY_DTYPE": make_shade_rays(rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), 0.25, rng.uniform(size=n))}
    for (name, rays), dtype, maker in zip(packed.items(), (RAY_DTYPE, SHADE_RAY_DTYPE), ("make_rays", "make_shade_rays")):
        names = (maker, name)
        text = "rays must be an (n, 8) float32 array (%s) or a %s array" % names
        wide = np.repeat(rays, 2, axis=0)
        wide[1::2] = -1.0
        cases = (rays.reshape(-1).view(dtype), rays, wide[::2], np.asfortranarray(rays), np.zeros((0, 8), dtype=np.float32))
        assert cases[0].shape == (n,) and not cases[2].flags.c_contiguous and not cases[3].flags.c_contiguous
        for a, want in zip(cases, (rays, rays, rays, rays, rays[:0])):
            got = ray_records(a, dtype, names)
            assert got.dtype == np.float32 and got.shape == want.shape and got.flags.c_contiguous
            assert got.tobytes() == want.tobytes()
        other = SHADE_RAY_DTYPE if dtype is RAY_DTYPE else RAY_DTYPE
        for bad in (rays.astype(np.float64), rays.reshape(-1), rays[:, :7], rays.reshape(n, 2, 4), rays.reshape(-1).view(other),
                    rays.reshape(-1).view(dtype).reshape(n, 1), rays.view(np.int32)):
            with pytest.raises(ValueError) as e:
                ray_records(bad, dtype, names)
            assert str(e.value) == text
