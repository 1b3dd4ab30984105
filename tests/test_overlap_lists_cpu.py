"""No GPU: the overlap lists (lt_hip_overlap_boxes_list, lt_hip_overlap_tris_list) as far as they can be checked without one.

1. the six symbols are declared, exported and loadable, the descriptor's layout matches the header, the header states the
   sizing rule and its exception, a null context is an invalid argument;
2. both host forms equal the numpy model (tests/overlap.py, tests/overlap_tris.py with keep = the number of leaves) word for word
   on every family of the base scene and the twelve-triangle fan; the differences of the offsets are LT_OVERLAP_COUNT's words and
   the first eight of a segment LT_OVERLAP_FIRST_K's, both of the existing host forms;
3. the sizing call writes offsets alone; items that are too small come back untouched with LT_ERR_BUFFER_TOO_SMALL and the
   offsets valid; LT_OVERLAP_LIST_FLAG_FILL_ONLY from the returned offsets gives the same items, and with offsets that are not
   the batch's own nothing is written outside the segments or the buffer;
4. every error writes nothing."""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import (box_records, make_boxes, make_tris, overlap_boxes_host, overlap_boxes_list_host, overlap_tris_host,
                                     overlap_tris_list_host, tri_records)
from tests import nearest as nr
from tests import nearest_k as nk
from tests import overlap as ov
from tests import overlap_lists as ol
from tests import overlap_tris as ot
from tests import query_edges as qe

NAMES = [f % shape for shape in ("boxes", "tris") for f in ("lt_hip_overlap_%s_list", "lt_hip_overlap_%s_list_device", "lt_hip_overlap_%s_list_host")]
SENTINEL = ol.SENTINEL
FILL = C.OVERLAP_LIST_FLAG_FILL_ONLY
vp = ctypes.c_void_p


def desc(flags=0, size=ctypes.sizeof(C.OverlapListDesc)):
    return ctypes.byref(C.OverlapListDesc(size, flags))


# ------------------------------------------------------------------------------------------------------------- 1: the ABI
def test_the_six_symbols_are_declared_exported_and_loadable():
    L = C.load()
    header = open(os.path.join(ol.ROOT, "include", "lenstrace_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lt_hip_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in C.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) == (9 if name.endswith("_device") else 11 if name.endswith("_host") else 8)
    assert L.lt_hip_abi_version() == 4 and re.search(r"#define\s+LT_HIP_ABI_VERSION\s+4\b", header)


def test_the_descriptor_and_the_header_text():
    header = open(os.path.join(ol.ROOT, "include", "lenstrace_hip.h")).read()
    assert re.search(r"typedef struct lt_hip_overlap_list_desc \{\s*uint32_t struct_size;[^}]*uint32_t flags;[^}]*\} lt_hip_overlap_list_desc;", header)
    assert re.search(r"#define\s+LT_OVERLAP_LIST_FLAG_FILL_ONLY\s+0x1u", header) and FILL == 1
    D = C.OverlapListDesc
    assert ctypes.sizeof(D) == 8 and (D.struct_size.offset, D.flags.offset) == (0, 4)
    text = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("items == NULL with items_bytes == 0 writes the offsets only", "the one exception to \"a failed call writes nothing\"",
                   "slow, but correct", "lt_hip_overlap_boxes_list, lt_hip_overlap_tris_list, host and _device forms) share the context's work counters"):
        assert phrase in text, phrase
    tile, span = ol.tuning()
    assert tile >= 64 and span >= 64 and tile & (tile - 1) == 0


def test_a_null_context_is_an_invalid_argument_and_writes_nothing():
    L = C.load()
    offsets = np.full(8, SENTINEL, dtype=np.uint64)
    items = np.full(8, SENTINEL, dtype=np.int32)
    bx = make_boxes(np.zeros((2, 3)), np.ones((2, 3)))
    tr = make_tris(np.zeros((2, 3)), np.ones((2, 3)), np.ones((2, 3)))
    O, I = offsets.ctypes.data_as(vp), items.ctypes.data_as(vp)
    for shape, rec in (("boxes", bx), ("tris", tr)):
        R = rec.ctypes.data_as(vp)
        assert getattr(L, "lt_hip_overlap_%s_list" % shape)(None, desc(), R, 2, O, 64, I, 32) == C.LT_ERR_INVALID_ARGUMENT
        assert getattr(L, "lt_hip_overlap_%s_list_device" % shape)(None, desc(), R, 2, O, 64, I, 32, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (offsets == SENTINEL).all() and (items == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------- the fixtures
@pytest.fixture(scope="module")
def cases():
    """(shape, scene name) -> (scene, records, the model's sequences, its CSR): computed once."""
    out = {}
    for i, (name, s) in enumerate((("base", qe.base_scene(0)), ("fan12", nk.fan12()))):
        bx = np.concatenate(list(ov.families(s, seed=i).values()))
        m = ol.model_boxes(s, bx)
        out["boxes", name] = (s, bx, m, ol.csr(m))
        tr = np.concatenate(list(ot.families(s, seed=i).values()))
        m = ol.model_tris(s, tr)
        out["tris", name] = (s, tr, m, ol.csr(m))
    return out


def raw(shape, s, rec, flags, offsets, items, items_bytes=None, n=None, offsets_bytes=None):
    f = getattr(C.load(), "lt_hip_overlap_%s_list_host" % shape)
    return f(s.nodes.ctypes.data_as(vp), s.nodes.nbytes, s.prims.ctypes.data_as(vp), s.prims.nbytes, desc(flags), rec.ctypes.data_as(vp),
             len(rec) if n is None else n, offsets.ctypes.data_as(vp), offsets.nbytes if offsets_bytes is None else offsets_bytes,
             None if items is None else items.ctypes.data_as(vp), (0 if items is None else items.nbytes) if items_bytes is None else items_bytes)


# ------------------------------------------------------------------------------------------------------------- 2: the host forms
def test_the_host_forms_equal_the_model(cases):
    for (shape, name), (s, rec, m, (offsets, items)) in cases.items():
        host = overlap_boxes_list_host if shape == "boxes" else overlap_tris_list_host
        got_o, got_i = host(s, rec)
        assert got_o.dtype == np.uint64 and got_o.shape == (len(rec) + 1,) and got_i.dtype == np.int32
        assert np.array_equal(got_o, offsets), (shape, name, np.flatnonzero(got_o != offsets)[:5])
        assert np.array_equal(got_i, items), (shape, name, np.flatnonzero(got_i != items)[:5])
        # the batch has long, short and empty sequences
        assert (m.count > 8).sum() >= 32 and (m.count == 0).sum() >= 64 and ((m.count > 0) & (m.count <= 8)).sum() >= 32, (shape, name)
        assert shape == "tris" or int(m.count.max()) == ol.leaves(s), (shape, name)            # a box that holds the whole scene


def test_the_counts_and_the_first_eight_are_the_existing_host_forms(cases):
    for (shape, name), (s, rec, m, _) in cases.items():
        host, first = (overlap_boxes_list_host, overlap_boxes_host) if shape == "boxes" else (overlap_tris_list_host, overlap_tris_host)
        offsets, items = host(s, rec)
        assert offsets[0] == 0 and offsets[-1] == len(items)
        assert np.array_equal(np.diff(offsets), first(s, rec, count=True).astype(np.uint64)), (shape, name)
        k8 = first(s, rec, k=8)
        for i in range(len(rec)):
            seg = items[int(offsets[i]):int(offsets[i + 1])]
            assert np.array_equal(seg[:8], k8[i][k8[i] >= 0]) and (np.diff(seg) >= 0).all(), (shape, name, i)


# ------------------------------------------------------------------------------------------------------------- 3: sizing and filling
def test_sizing_too_small_and_fill_only(cases):
    for (shape, name), (s, rec, m, (offsets, items)) in cases.items():
        total = len(items)
        # the sizing call: the offsets alone
        got_o = np.full(len(rec) + 2, SENTINEL, dtype=np.uint64)
        assert raw(shape, s, rec, 0, got_o, None, offsets_bytes=8 * (len(rec) + 1)) == 0
        assert np.array_equal(got_o[:-1], offsets) and got_o[-1] == SENTINEL
        # one word short: LT_ERR_BUFFER_TOO_SMALL, offsets valid, items untouched
        got_o[:] = SENTINEL
        got_i = np.full(total + 16, SENTINEL, dtype=np.int32)
        assert raw(shape, s, rec, 0, got_o, got_i, items_bytes=4 * (total - 1), offsets_bytes=8 * (len(rec) + 1)) == C.LT_ERR_BUFFER_TOO_SMALL
        assert np.array_equal(got_o[:-1], offsets) and got_o[-1] == SENTINEL and (got_i == SENTINEL).all()
        # the exact size: both, and nothing behind them
        assert raw(shape, s, rec, 0, got_o, got_i, items_bytes=4 * total, offsets_bytes=8 * (len(rec) + 1)) == 0
        assert np.array_equal(got_o[:-1], offsets) and np.array_equal(got_i[:total], items) and (got_i[total:] == SENTINEL).all()
        # FILL_ONLY from the returned offsets: the same items, the offsets as they were
        got_i[:] = SENTINEL
        kept = got_o.copy()
        assert raw(shape, s, rec, FILL, got_o, got_i, items_bytes=4 * total) == 0
        assert np.array_equal(got_o, kept) and np.array_equal(got_i[:total], items) and (got_i[total:] == SENTINEL).all()


def test_fill_only_stays_inside_whatever_the_offsets_hold(cases):
    s, rec, m, (offsets, items) = cases["boxes", "base"]
    total = len(items)
    # halved offsets: query i writes min(its length, the halved segment's) words at offsets[i] // 2; the rest keeps the sentinel
    half = offsets // np.uint64(2)
    got = np.full(total + 16, SENTINEL, dtype=np.int32)
    assert raw("boxes", s, rec, FILL, half, got, items_bytes=4 * total) == 0
    want = np.full(total + 16, SENTINEL, dtype=np.int32)
    for i in range(len(rec)):
        b, e = int(half[i]), int(half[i + 1])
        want[b:e] = items[int(offsets[i]):int(offsets[i + 1])][:e - b]
    assert np.array_equal(got, want)
    # a capacity in the middle of a segment, descending offsets, offsets behind the buffer: nothing outside items[0 .. capacity)
    cap = total // 2 + 1
    for bad in (offsets, offsets[::-1].copy(), offsets + np.uint64(total), np.full(len(offsets), 2 ** 64 - 1, dtype=np.uint64)):
        got[:] = SENTINEL
        assert raw("boxes", s, rec, FILL, bad, got, items_bytes=4 * cap) == 0
        assert (got[cap:] == SENTINEL).all()
        if bad is offsets:
            assert np.array_equal(got[:cap], items[:cap])
        else:                   # every segment begins at or behind its end, or behind the capacity
            assert (got == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------- 4: errors
def test_every_error_writes_nothing():
    s = nr.hand_made()
    bx = make_boxes(np.full((2, 3), -4.0), np.full((2, 3), 4.0))
    tr = make_tris(np.full((2, 3), -4.0), np.full((2, 3), 4.0), np.array([[4.0, -4.0, 0.0]] * 2))
    offsets = np.full(8, SENTINEL, dtype=np.uint64)
    items = np.full(16, SENTINEL, dtype=np.int32)
    INVALID, SMALL = C.LT_ERR_INVALID_ARGUMENT, C.LT_ERR_BUFFER_TOO_SMALL
    L = C.load()
    for shape, rec in (("boxes", bx), ("tris", tr)):
        f = getattr(L, "lt_hip_overlap_%s_list_host" % shape)
        N, Pr, R, O, I = (x.ctypes.data_as(vp) for x in (s.nodes, s.prims, rec, offsets, items))
        nb, pb = s.nodes.nbytes, s.prims.nbytes
        cases = [
            (N, nb, Pr, pb, None, R, 2, O, 24, I, 64, INVALID),
            (N, nb, Pr, pb, desc(size=4), R, 2, O, 24, I, 64, INVALID),
            (N, nb, Pr, pb, desc(flags=2), R, 2, O, 24, I, 64, INVALID),
            (N, nb, Pr, pb, desc(flags=FILL | 4), R, 2, O, 24, I, 64, INVALID),
            (None, nb, Pr, pb, desc(), R, 2, O, 24, I, 64, INVALID),
            (N, nb, None, pb, desc(), R, 2, O, 24, I, 64, INVALID),
            (N, nb - 1, Pr, pb, desc(), R, 2, O, 24, I, 64, INVALID),
            (N, nb, Pr, pb - 1, desc(), R, 2, O, 24, I, 64, INVALID),
            (N, nb, Pr, pb, desc(), R, 2 ** 32, O, 24, I, 64, INVALID),
            (N, nb, Pr, pb, desc(), None, 2, O, 24, I, 64, INVALID),
            (N, nb, Pr, pb, desc(), R, 2, None, 24, I, 64, INVALID),
            (N, nb, Pr, pb, desc(), R, 2, O, 24, None, 64, INVALID),               # items NULL with items_bytes != 0
            (N, nb, Pr, pb, desc(FILL), R, 2, O, 24, None, 0, INVALID),            # FILL_ONLY without items
            (N, nb, Pr, 76, desc(), R, 2, O, 24, I, 64, C.LT_ERR_BAD_SCENE),       # the second leaf's offset lies outside prims
            (N, nb, Pr, pb, desc(), R, 2, O, 23, I, 64, SMALL),                    # 8 (n + 1) = 24
            (N, nb, Pr, pb, desc(FILL), R, 2, O, 23, I, 64, SMALL),
            (N, nb, Pr, pb, desc(), R, 0, O, 7, None, 0, SMALL),
            # an unknown flag comes before the buffers' sizes
            (N, nb, Pr, pb, desc(flags=8), R, 2, O, 0, I, 0, INVALID),
        ]
        for i, (*args, want) in enumerate(cases):
            assert f(*args) == want, (shape, i)
            assert (offsets == SENTINEL).all() and (items == SENTINEL).all(), (shape, i)
        # n == 0 writes offsets[0] = 0 and nothing else; with FILL_ONLY nothing at all
        assert f(N, nb, Pr, pb, desc(FILL), None, 0, O, 8, I, 64) == 0 and (offsets == SENTINEL).all() and (items == SENTINEL).all()
        assert f(N, nb, Pr, pb, desc(), None, 0, O, 8, None, 0) == 0 and offsets[0] == 0 and (offsets[1:] == SENTINEL).all()
        offsets[:] = SENTINEL
        # a call that works, against the existing host form (both leaves touch both boxes)
        first = (overlap_boxes_host if shape == "boxes" else overlap_tris_host)(s, rec, k=2)
        want = first[first >= 0]
        assert len(want) >= 2 and (shape == "tris" or want.tolist() == [0, 1, 0, 1])
        assert f(N, nb, Pr, pb, desc(), R, 2, O, 24, I, 16) == 0
        assert offsets[:3].tolist() == [0, (first[0] >= 0).sum(), len(want)] and items[:len(want)].tolist() == want.tolist()
        assert (offsets[3:] == SENTINEL).all() and (items[len(want):] == SENTINEL).all()
        offsets[:] = SENTINEL
        items[:] = SENTINEL
    with pytest.raises(ValueError):
        overlap_boxes_list_host(s, bx[:, :6])
    with pytest.raises(ValueError):
        overlap_tris_list_host(s, tr[:, :8])
    assert box_records(bx).shape == (2, 8) and tri_records(tr).shape == (2, 12)
