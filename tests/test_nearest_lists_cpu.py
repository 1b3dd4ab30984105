"""No GPU: the radius lists (lt_hip_nearest_list) as far as they can be checked without one.

1. the three symbols are declared, exported and loadable, the descriptor's layout matches the header, the header states the
   order's argument and the cost, the sort span is lt_overlist.hpp's own constant, a null context is an invalid argument;
2. the host form equals the numpy model (tests/nearest_k.py with keep = the number of leaves) bit for bit on every family of
   the base scene, the 16 x 16 wall, the twelve-triangle fan and the base scene at 2^35, and on the scene that names a primitive
   in two leaves; the differences of the offsets are LT_NEAREST_COUNT's words and the first eight records of a segment
   LT_NEAREST_FIRST_K's real records, both of the existing host form;
3. the sizing call writes offsets alone; items that are too small come back untouched with LT_ERR_BUFFER_TOO_SMALL and the
   offsets valid; LT_NEAREST_LIST_FLAG_FILL_ONLY from the returned offsets gives the same items, and with offsets that are not
   the batch's own nothing is written outside the segments or the buffer;
4. every error writes nothing;
5. the row's segment lengths and the fans' all-tie segments."""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import synth
from lens_trace_amd.renderer import HIT_DTYPE, POINT_DTYPE, make_points, nearest_k_host, nearest_list_host
from tests import multihit_edges as me
from tests import nearest as nr
from tests import nearest_k as nk
from tests import nearest_lists as nl
from tests import overlap_lists as ol
from tests import query_edges as qe

NAMES = ["lt_hip_nearest_list", "lt_hip_nearest_list_device", "lt_hip_nearest_list_host"]
SENTINEL = nl.SENTINEL
FILL = C.NEAREST_LIST_FLAG_FILL_ONLY
vp = ctypes.c_void_p


def desc(flags=0, size=ctypes.sizeof(C.NearestListDesc)):
    return ctypes.byref(C.NearestListDesc(size, flags))


def sentinel_items(n):
    return np.full(4 * n, SENTINEL, dtype=np.uint32).view(HIT_DTYPE)


def untouched(items):
    return bool((items.view(np.uint32) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------- 1: the ABI
def test_the_three_symbols_are_declared_exported_and_loadable():
    L = C.load()
    header = open(os.path.join(nl.ROOT, "include", "lenstrace_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lt_hip_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in C.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) == (9 if name.endswith("_device") else 11 if name.endswith("_host") else 8)
    assert L.lt_hip_abi_version() == 4 and re.search(r"#define\s+LT_HIP_ABI_VERSION\s+4\b", header)


def test_the_descriptor_and_the_header_text():
    header = open(os.path.join(nl.ROOT, "include", "lenstrace_hip.h")).read()
    assert re.search(r"typedef struct lt_hip_nearest_list_desc \{\s*uint32_t struct_size;[^}]*uint32_t flags;[^}]*\} lt_hip_nearest_list_desc;", header)
    assert re.search(r"#define\s+LT_NEAREST_LIST_FLAG_FILL_ONLY\s+0x1u", header) and FILL == 1
    D = C.NearestListDesc
    assert ctypes.sizeof(D) == 8 and (D.struct_size.offset, D.flags.offset) == (0, 4)
    text = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("are bit-identical, so the multiset sorted by (d2, offset) is the sequence", "Accepted d2 are never NaN",
                   "items == NULL with items_bytes == 0 writes the offsets only", "give a finite radius",
                   "lt_hip_nearest_k, lt_hip_nearest_list, lt_hip_overlap_boxes"):
        assert phrase in text, phrase
    tile, span = nl.tuning()
    assert tile == ol.tuning()[0] and span >= 64 and span & (span - 1) == 0
    assert 16 * span == 4 * ol.tuning()[1]          # both ordering kernels keep the same bytes of LDS


def test_a_null_context_is_an_invalid_argument_and_writes_nothing():
    L = C.load()
    offsets = np.full(8, SENTINEL, dtype=np.uint64)
    items = sentinel_items(8)
    pts = make_points(np.zeros((2, 3)), 1.0)
    O, I, P = offsets.ctypes.data_as(vp), items.ctypes.data_as(vp), pts.ctypes.data_as(vp)
    assert L.lt_hip_nearest_list(None, desc(), P, 2, O, 64, I, 128) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_nearest_list_device(None, desc(), P, 2, O, 64, I, 128, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (offsets == SENTINEL).all() and untouched(items)


# ------------------------------------------------------------------------------------------------------------- the fixtures
@pytest.fixture(scope="module")
def cases():
    """name -> (scene, points, the model's sequences, its CSR): computed once."""
    base = qe.base_scene(0)
    scenes = {"base": base, "wall16": synth.heightfield_wall(16), "fan12": nk.fan12(), "far+": qe.extreme_scene(base, "far+")[0],
              "twice": me.twice_named_scene()[0]}
    out = {}
    for i, (name, s) in enumerate(scenes.items()):
        pts = np.concatenate(list(nk.families(s, seed=i).values()))
        m = nl.model(s, pts)
        out[name] = (s, pts, m, nl.csr(m))
    return out


def raw(s, pts, flags, offsets, items, items_bytes=None, n=None, offsets_bytes=None):
    return C.load().lt_hip_nearest_list_host(
        s.nodes.ctypes.data_as(vp), s.nodes.nbytes, s.prims.ctypes.data_as(vp), s.prims.nbytes, desc(flags), pts.ctypes.data_as(vp),
        len(pts) if n is None else n, offsets.ctypes.data_as(vp), offsets.nbytes if offsets_bytes is None else offsets_bytes,
        None if items is None else items.ctypes.data_as(vp), (0 if items is None else items.nbytes) if items_bytes is None else items_bytes)


# ------------------------------------------------------------------------------------------------------------- 2: the host form
def test_the_host_form_equals_the_model(cases):
    for name, (s, pts, m, want) in cases.items():
        got = nearest_list_host(s, pts)
        assert got[0].shape == (len(pts) + 1,)
        assert nl.differ(got, want) is None, (name, nl.differ(got, want))
        # the batch has long, short and empty sequences, and records that tie in d2
        full = nl.leaves(s)
        assert ((m.count > 8).sum() >= 32 if full > 8 else (m.count == full).sum() >= 32) and (m.count == 0).sum() >= 64, name
        assert ((m.count > 0) & (m.count <= 8)).sum() >= 32, name
        assert sum((np.diff(g["t"]) == 0).any() for g in nl.segments(want)) >= 32, name
        # POINT_DTYPE in, (n, 3) + max_d2 in: the same call
        assert nl.differ(nearest_list_host(s, pts.view(POINT_DTYPE).reshape(-1)), want) is None
        assert nl.differ(nearest_list_host(s, pts[:, 0:3], max_d2=pts[:, 3]), want) is None


def test_a_primitive_named_twice_lies_side_by_side(cases):
    s, pts, m, want = cases["twice"]
    twins = 0
    for g in nl.segments(want):
        same = (g["prim"][1:] == g["prim"][:-1]) & (g["t"][1:] == g["t"][:-1])     # (the two leaves' boxes may give two d2)
        twins += int(same.sum())
        assert len(nr.same(g[1:][same], g[:-1][same])) == 0          # the same record, bit for bit: the sort needs no third key
    assert twins >= 64
    assert nl.differ(nearest_list_host(s, pts), want) is None


def test_the_counts_and_the_first_eight_are_the_existing_host_form(cases):
    for name, (s, pts, m, _) in cases.items():
        offsets, items = nearest_list_host(s, pts)
        assert offsets[0] == 0 and offsets[-1] == len(items)
        assert np.array_equal(np.diff(offsets), nearest_k_host(s, pts, count=True).astype(np.uint64)), name
        k8 = nearest_k_host(s, pts, k=8)
        for i, g in enumerate(nl.segments((offsets, items))):
            real = k8[i][k8[i]["prim"] >= 0]
            assert len(real) == min(8, len(g)) and len(nr.same(g[:8], real)) == 0 and nl.sorted_by_d2_and_prim(g), (name, i)


# ------------------------------------------------------------------------------------------------------------- 3: sizing and filling
def test_sizing_too_small_and_fill_only(cases):
    for name, (s, pts, m, (offsets, items)) in cases.items():
        total = len(items)
        # the sizing call: the offsets alone
        got_o = np.full(len(pts) + 2, SENTINEL, dtype=np.uint64)
        assert raw(s, pts, 0, got_o, None, offsets_bytes=8 * (len(pts) + 1)) == 0
        assert np.array_equal(got_o[:-1], offsets) and got_o[-1] == SENTINEL
        # one record short: LT_ERR_BUFFER_TOO_SMALL, offsets valid, items untouched -- and one byte short of the exact size
        for short in (16 * (total - 1), 16 * total - 1):
            got_o[:] = SENTINEL
            got_i = sentinel_items(total + 16)
            assert raw(s, pts, 0, got_o, got_i, items_bytes=short, offsets_bytes=8 * (len(pts) + 1)) == C.LT_ERR_BUFFER_TOO_SMALL
            assert np.array_equal(got_o[:-1], offsets) and got_o[-1] == SENTINEL and untouched(got_i)
        # the exact size: both, and nothing behind them
        assert raw(s, pts, 0, got_o, got_i, items_bytes=16 * total, offsets_bytes=8 * (len(pts) + 1)) == 0
        assert np.array_equal(got_o[:-1], offsets) and len(nr.same(got_i[:total], items)) == 0 and untouched(got_i[total:])
        # FILL_ONLY from the returned offsets: the same items, the offsets as they were
        got_i = sentinel_items(total + 16)
        kept = got_o.copy()
        assert raw(s, pts, FILL, got_o, got_i, items_bytes=16 * total) == 0
        assert np.array_equal(got_o, kept) and len(nr.same(got_i[:total], items)) == 0 and untouched(got_i[total:])


def test_fill_only_stays_inside_whatever_the_offsets_hold(cases):
    s, pts, m, (offsets, items) = cases["base"]
    total = len(items)
    # halved offsets: point i writes min(its length, the halved segment's) records at offsets[i] // 2; the rest keeps the sentinel
    half = offsets // np.uint64(2)
    got = sentinel_items(total + 16)
    assert raw(s, pts, FILL, half, got, items_bytes=16 * total) == 0
    want = sentinel_items(total + 16)
    for i, g in enumerate(nl.segments((offsets, items))):
        b, e = int(half[i]), int(half[i + 1])
        want[b:e] = g[:e - b]
    assert len(nr.same(got, want)) == 0
    # a capacity in the middle of a segment, descending offsets, offsets behind the buffer: nothing outside items[0 .. capacity)
    cap = total // 2 + 1
    for bad in (offsets, offsets[::-1].copy(), offsets + np.uint64(total), np.full(len(offsets), 2 ** 64 - 1, dtype=np.uint64)):
        got = sentinel_items(total + 16)
        assert raw(s, pts, FILL, bad, got, items_bytes=16 * cap) == 0
        assert untouched(got[cap:])
        if bad is offsets:
            assert len(nr.same(got[:cap], items[:cap])) == 0
        else:                   # every segment begins at or behind its end, or behind the capacity
            assert untouched(got)


# ------------------------------------------------------------------------------------------------------------- 4: errors
def test_every_error_writes_nothing():
    s = nr.hand_made()
    pts = make_points(np.zeros((2, 3)), 1e6)
    offsets = np.full(8, SENTINEL, dtype=np.uint64)
    items = sentinel_items(16)
    INVALID, SMALL = C.LT_ERR_INVALID_ARGUMENT, C.LT_ERR_BUFFER_TOO_SMALL
    f = C.load().lt_hip_nearest_list_host
    N, Pr, R, O, I = (x.ctypes.data_as(vp) for x in (s.nodes, s.prims, pts, offsets, items))
    nb, pb = s.nodes.nbytes, s.prims.nbytes
    cases = [
        (N, nb, Pr, pb, None, R, 2, O, 24, I, 256, INVALID),
        (N, nb, Pr, pb, desc(size=4), R, 2, O, 24, I, 256, INVALID),
        (N, nb, Pr, pb, desc(flags=2), R, 2, O, 24, I, 256, INVALID),
        (N, nb, Pr, pb, desc(flags=FILL | 4), R, 2, O, 24, I, 256, INVALID),
        (None, nb, Pr, pb, desc(), R, 2, O, 24, I, 256, INVALID),
        (N, nb, None, pb, desc(), R, 2, O, 24, I, 256, INVALID),
        (N, nb - 1, Pr, pb, desc(), R, 2, O, 24, I, 256, INVALID),
        (N, nb, Pr, pb - 1, desc(), R, 2, O, 24, I, 256, INVALID),
        (N, nb, Pr, pb, desc(), R, 2 ** 32, O, 24, I, 256, INVALID),
        (N, nb, Pr, pb, desc(), None, 2, O, 24, I, 256, INVALID),
        (N, nb, Pr, pb, desc(), R, 2, None, 24, I, 256, INVALID),
        (N, nb, Pr, pb, desc(), R, 2, O, 24, None, 256, INVALID),              # items NULL with items_bytes != 0
        (N, nb, Pr, pb, desc(FILL), R, 2, O, 24, None, 0, INVALID),            # FILL_ONLY without items
        (N, nb, Pr, 76, desc(), R, 2, O, 24, I, 256, C.LT_ERR_BAD_SCENE),      # the second leaf's offset lies outside prims
        (N, nb, Pr, pb, desc(), R, 2, O, 23, I, 256, SMALL),                   # 8 (n + 1) = 24
        (N, nb, Pr, pb, desc(FILL), R, 2, O, 23, I, 256, SMALL),
        (N, nb, Pr, pb, desc(), R, 0, O, 7, None, 0, SMALL),
        # an unknown flag comes before the buffers' sizes
        (N, nb, Pr, pb, desc(flags=8), R, 2, O, 0, I, 0, INVALID),
    ]
    for i, (*args, want) in enumerate(cases):
        assert f(*args) == want, i
        assert (offsets == SENTINEL).all() and untouched(items), i
    # n == 0 writes offsets[0] = 0 and nothing else; with FILL_ONLY nothing at all
    assert f(N, nb, Pr, pb, desc(FILL), None, 0, O, 8, I, 256) == 0 and (offsets == SENTINEL).all() and untouched(items)
    assert f(N, nb, Pr, pb, desc(), None, 0, O, 8, None, 0) == 0 and offsets[0] == 0 and (offsets[1:] == SENTINEL).all()
    offsets[:] = SENTINEL
    # a call that works, against the existing host form: both leaves lie within the radius of both points
    first = nearest_k_host(s, pts, k=2)
    assert (first["prim"] >= 0).all()
    assert f(N, nb, Pr, pb, desc(), R, 2, O, 24, I, 64) == 0
    assert offsets[:3].tolist() == [0, 2, 4] and len(nr.same(items[:4], first.reshape(-1))) == 0
    assert (offsets[3:] == SENTINEL).all() and untouched(items[4:])
    with pytest.raises(ValueError):
        nearest_list_host(s, pts[:, :2])
    with pytest.raises(ValueError):
        nearest_list_host(s, pts, max_d2=1.0)             # ready records carry their own max_d2


# ------------------------------------------------------------------------------------------------------------- 5: lengths and ties
def test_the_rows_segment_lengths():
    span = nl.tuning()[1]
    n = 2 * span + 64
    s, _ = ol.row_scene(n, seed=7)
    lengths = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, span - 1, span, span + 1, 2 * span + 3, n]
    pts = nl.row_points(lengths)
    m = nl.model(s, pts, chunk=4)
    assert m.count.tolist() == lengths
    got = nearest_list_host(s, pts)
    assert nl.differ(got, nl.csr(m)) is None
    assert np.diff(got[0]).tolist() == lengths


@pytest.mark.parametrize("F", (200, 2112))
def test_the_fans_all_tie_segments(F):
    s = nl.fan(F)
    assert nl.leaves(s) == F
    pts = make_points(np.array([nl.FAN_VERTEX, nl.FAN_VERTEX, nl.FAN_VERTEX + np.float32([0.0, 0.0, 0.125])]),
                      np.float32([2.0 ** -20, np.inf, 0.5]))
    m = nl.model(s, pts, chunk=4)
    offsets, items = nearest_list_host(s, pts)
    assert nl.differ((offsets, items), nl.csr(m)) is None
    seg = nl.segments((offsets, items))
    # at V with a small radius: all F triangles at d2 == +0, so the offset alone orders the segment
    assert len(seg[0]) == F and (seg[0]["t"].view(np.uint32) == 0).all() and np.array_equal(seg[0]["prim"], np.arange(F))
    assert len(seg[1]) == F and 0 < len(seg[2]) <= F
