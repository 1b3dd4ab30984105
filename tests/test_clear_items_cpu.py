"""The item table and the fold map of a set of entry cuts (lt_entry_cut.hpp: item_entries, item_write, fold_mark_square), through the host export lt_hip_clear_items_test_host, which lays them out share by share as
lt_clear_items_kernel does.  No GPU.

On recorded mark arrays (word 0 of every square's list: 0xffffffff clear, else a count): all clear, none clear, alternating, shares
of unequal size (a number of squares that is no multiple of eight), group counts 1, 3 (five frames: two do not divide them) and 8.
The export runs those functions square by square, in order; the scan and the scatter that lt_clear_items_kernel puts around the
same functions run on the GPU only, where tests/test_gpu_clear_items.py holds their totals and every pixel against them.
Checked: every (square, group) is in exactly one entry, a whole entry standing for all groups of its square; the entries of a share
are in the share's order; the eight lengths add up; the map has exactly the clear squares' segments."""
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C

CLEAR = 0xFFFFFFFF
WHOLE = 0x80000000
HEADER = 16


def share(n, xcd):
    q, r = divmod(n, 8)
    size = q + (1 if xcd < r else 0)
    start = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return start, size


def build(marks, groups, order=None, tile=None):
    L = C.load()
    marks = np.ascontiguousarray(marks, dtype=np.uint32)
    n = marks.size
    table = np.full(HEADER + n * groups, 0xDEADBEEF, dtype=np.uint32)
    tw, th, tiles = tile if tile else (0, 0, 0)
    seg = tiles * th * (tw // 8) if tile else 0
    fmap = np.full(seg, 0x77, dtype=np.uint8) if tile else None
    o = np.ascontiguousarray(order, dtype=np.uint32) if order is not None else None
    rc = L.lt_hip_clear_items_test_host(marks.ctypes.data, o.ctypes.data if o is not None else None, n, groups, tw, th, tiles,
                                        table.ctypes.data, fmap.ctypes.data if fmap is not None else None)
    assert rc == 0
    return table, fmap


def patterns(n):
    rng = np.random.default_rng(7)
    counts = rng.integers(0, 16, n).astype(np.uint32)
    yield "all-clear", np.full(n, CLEAR, dtype=np.uint32)
    yield "none-clear", counts
    alt = counts.copy()
    alt[::2] = CLEAR
    yield "alternating", alt
    rnd = counts.copy()
    rnd[rng.random(n) < 0.7] = CLEAR
    yield "random", rnd


@pytest.mark.parametrize("n", [1, 6, 8, 13, 64, 2051])
@pytest.mark.parametrize("groups", [1, 3, 8])
def test_every_group_of_every_square_once_and_in_order(n, groups):
    for name, marks in patterns(n):
        table, _ = build(marks, groups)
        lengths = table[:8]
        clear = marks == CLEAR
        assert int(lengths.sum()) == int(clear.sum()) + int((~clear).sum()) * groups, name
        seen = np.zeros((n, groups), dtype=np.int32)
        for xcd in range(8):
            start, size = share(n, xcd)
            want_len = int(clear[start:start + size].sum()) + int((~clear[start:start + size]).sum()) * groups
            assert int(lengths[xcd]) == want_len, (name, xcd)
            entries = table[HEADER + start * groups: HEADER + start * groups + want_len]
            keys = []
            for e in entries:
                e = int(e)
                t = e & ~WHOLE
                local, g = divmod(t, groups)
                assert local < size, (name, xcd, hex(e))
                if e & WHOLE:
                    assert g == 0 and clear[start + local], (name, xcd, hex(e))
                    seen[start + local, :] += 1
                else:
                    assert not clear[start + local], (name, xcd, hex(e))
                    seen[start + local, g] += 1
                keys.append(t)
            assert keys == sorted(keys) and len(set(keys)) == len(keys), (name, xcd, "order")
            # (what lies behind a share's entries is not the export's to write)
            rest = table[HEADER + start * groups + want_len: HEADER + (start + size) * groups]
            assert (rest == 0xDEADBEEF).all(), (name, xcd)
        assert (seen == 1).all(), name


@pytest.mark.parametrize("tile", [(24, 16, 1), (64, 64, 3), (16, 12, 2), (8, 8, 5)])
def test_the_map_has_exactly_the_clear_squares_segments(tile):
    tw, th, tiles = tile
    bptx, bpty = tw // 8, (th + 7) // 8
    n = tiles * bptx * bpty
    rng = np.random.default_rng(11)
    order = rng.permutation(n).astype(np.uint32)
    for name, marks in patterns(n):
        for o in (None, order):
            _, fmap = build(marks, 3, order=o, tile=tile)
            want = np.zeros((tiles * th, bptx), dtype=np.uint8)
            for p in range(n):
                b = int(o[p]) if o is not None else p
                k, sb = divmod(b, bptx * bpty)
                sby, sbx = divmod(sb, bptx)
                rows = slice(k * th + sby * 8, k * th + min(sby * 8 + 8, th))
                want[rows, sbx] = 1 if marks[p] == CLEAR else 0
            assert np.array_equal(fmap.reshape(tiles * th, bptx), want), (name, o is not None)
            # a float of the output is folded by the square's own wave iff its segment is marked: float i lies in segment i // 24
            floats = tiles * th * tw * 3
            pix = np.arange(floats) // 3
            assert np.array_equal(np.arange(floats) // 24, (pix // tw) * bptx + (pix % tw) // 8)


def test_bad_arguments_are_refused():
    L = C.load()
    marks = np.zeros(4, dtype=np.uint32)
    table = np.zeros(HEADER + 4, dtype=np.uint32)
    fmap = np.zeros(64, dtype=np.uint8)
    assert L.lt_hip_clear_items_test_host(marks.ctypes.data, None, 4, 0, 0, 0, 0, table.ctypes.data, None) != 0       # no groups
    assert L.lt_hip_clear_items_test_host(marks.ctypes.data, None, 4, 1, 17, 9, 1, table.ctypes.data, fmap.ctypes.data) != 0   # a width that is no multiple of 8
    assert L.lt_hip_clear_items_test_host(marks.ctypes.data, None, 4, 1, 16, 8, 1, table.ctypes.data, fmap.ctypes.data) != 0   # 2 squares, not 4
