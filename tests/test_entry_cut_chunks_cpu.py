"""CPU tests of entry cuts that take several 64-byte records (lens_trace_amd/csrc/lt_entry_cut.hpp: Chunks): the arithmetic that
both the builder and the walk rely on, as the host compiles it (lt_hip_entry_cut_chunks_test_host), and the construction of
tests/entry_cut_chunk_scenes.py's scene, which tests/test_gpu_entry_cut_chunks.py relies on."""
import ctypes

import numpy as np

from lens_trace_amd import _capi as C
from tests import entry_cut_chunk_scenes as cs

K = 15              # lt_entry_cut::kCut
MAX_CHUNKS = 16     # lt_entry_cut::kMaxChunks


def chunk_arithmetic(heights, chunks, entries, which):
    lib = C.load()
    n = len(heights)
    a = [np.ascontiguousarray(heights, np.int32)] + [np.ascontiguousarray(x, np.uint32) for x in (chunks, entries, which)]
    out = np.zeros((n, 4), np.uint32)
    rc = lib.lt_hip_entry_cut_chunks_test_host(*[x.ctypes.data_as(ctypes.c_void_p) for x in a], ctypes.c_uint64(n), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def expected_limit(height):
    """A list's entries wait on the walk's 64-slot stack under the 2 * height + 2 slots of the deepest path."""
    if height < 0:
        return 0
    room = min(K, 64 - (2 * height + 2))
    return room if room >= 2 else 0


def test_limits_by_tree_height():
    heights = list(range(-2, 40))
    out = chunk_arithmetic(heights, [1] * len(heights), [0] * len(heights), [0] * len(heights))
    assert [int(v) for v in out[:, 0]] == [expected_limit(h) for h in heights]
    # (the heights where a record holds fewer than fifteen entries, and where it holds none)
    assert expected_limit(23) == 15 and expected_limit(24) == 14 and expected_limit(30) == 2 and expected_limit(31) == 0


def test_a_list_is_its_chunks_and_no_chunk_exceeds_the_limit():
    """For every tree height, every cap and every list length up to what the cap allows: the chunks' counts add up to the list, no
    chunk holds more than the height's limit, every chunk before the last is full, the chunks after the last are empty, and there
    are no more chunks than the cap."""
    cases = 0
    for height in (-1, 0, 5, 23, 24, 27, 30, 31, 40):
        limit = expected_limit(height)
        for cap in (0, 1, 2, 3, 4, 8, 15, 16, 17, 1000):
            capacity = limit * min(max(cap, 1), MAX_CHUNKS)
            lengths = sorted(set([0, 1, 2, limit, limit + 1, 2 * limit - 1, 2 * limit, 2 * limit + 1, capacity - 1, capacity]) & set(range(capacity + 1)))
            for entries in lengths:
                which = list(range(MAX_CHUNKS + 2))
                out = chunk_arithmetic([height] * len(which), [cap] * len(which), [entries] * len(which), which)
                assert (out[:, 0] == limit).all() and (out[:, 1] == capacity).all()
                counts = [int(v) for v in out[:, 3]]
                used = int(out[0, 2])
                assert sum(counts) == entries, (height, cap, entries, counts)
                assert max(counts) <= limit
                assert used <= min(max(cap, 1), MAX_CHUNKS)
                assert all(c == limit for c in counts[:max(used - 1, 0)]) and all(c == 0 for c in counts[used:])
                assert used == 0 or counts[used - 1] > 0
                cases += 1
    assert cases > 200


def test_grazing_field_squares_keep_tens_to_hundreds_of_leaves():
    s, cam = cs.scene("grazing-field")
    seen = []
    for W, H in cs.SIZES:
        counts = cs.surviving_leaves(s, cam, W, H)
        print("grazing-field %dx%d: surviving leaves per square %r" % (W, H, counts))
        seen += counts
    assert max(seen) < 400
    assert sum(1 for c in seen if 16 <= c <= 30) >= 2       # two records
    assert sum(1 for c in seen if 31 <= c <= 60) >= 2       # three or four
    assert sum(1 for c in seen if c > 120) >= 2             # more than eight hold


# ---- the cut over the pruned tree (lt_entry_cut.hpp: pruned_mark, pruned_cut_select), on recorded trees

NONE = 0xffff


def recorded_tree(rng, leaves_wanted, reach=0.85):
    """A tree as the leaf pass writes it down: records in the order it visits them (a stack: right child pushed first, left popped
    first), refs (interior: the record's own number; leaf: bit 31 set), parents, kids (NONE: a child the pass did not reach)."""
    refs, parents, kids = [], [], []
    stack = [(NONE, 0, 0)]      # (record it came from, which child, depth)
    leaves = 0
    while stack:
        came, side, depth = stack.pop()
        v = len(refs)
        if came != NONE:
            kids[2 * came + side] = v
        parents.append(came)
        kids += [NONE, NONE]
        leaf = depth >= 3 and (depth >= 12 or leaves + len(stack) >= leaves_wanted or rng.random() < 0.25)
        if leaf:
            refs.append(0x80000000 | v)
            leaves += 1
        else:
            refs.append(v)
            both = [s for s in (1, 0) if rng.random() < reach] or [int(rng.integers(2))]
            for s in both:
                stack.append((v, s, depth + 1))
    return np.array(refs, np.uint32), np.array(parents, np.uint16), np.array(kids, np.uint16)


def pruned_cut(refs, parents, kids, survives, cap):
    lib = C.load()
    out = np.zeros(cap, np.uint32)
    count = ctypes.c_uint32(0)
    rc = lib.lt_hip_entry_cut_pruned_test_host(*[a.ctypes.data_as(ctypes.c_void_p) for a in (refs, parents, kids, survives)], ctypes.c_uint32(len(refs)),
                                               ctypes.c_uint32(cap), out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count))
    assert rc == 0
    return [int(x) for x in out[:count.value]]


def test_a_pruned_cut_covers_every_surviving_leaf_exactly_once():
    """On recorded trees of 30 to 500 records with a tenth to all of their leaves surviving, under caps from 2 to 240: every surviving
    leaf has exactly one entry of the cut on its way to the root (itself included); every entry has a surviving leaf below it; the
    cut is no longer than the cap and its records no longer than the limit; where the survivors fit the cap the cut is the survivors;
    a tree without survivors has the empty cut."""
    rng = np.random.default_rng(20261021)
    trees = 0
    for wanted in (8, 20, 60, 150, 240):
        for share in (0.1, 0.5, 1.0):
            refs, parents, kids = recorded_tree(rng, wanted)
            assert 10 <= len(refs) <= 512 and parents[0] == NONE
            is_leaf = (refs >> 31) == 1
            survives = (is_leaf & (rng.random(len(refs)) < share)).astype(np.uint8)
            if not survives.any():
                survives[np.nonzero(is_leaf)[0][0]] = 1
            by_ref = {int(r): v for v, r in enumerate(refs)}
            for cap in (2, 3, 15, 16, 30, 60, 240):
                cut = pruned_cut(refs, parents, kids, survives, cap)
                assert 0 < len(cut) <= cap and len(set(cut)) == len(cut)
                entries = set(by_ref[r] for r in cut)
                covered = set()
                for v in np.nonzero(survives)[0]:
                    on_the_way, u = 0, int(v)
                    while u != NONE:
                        on_the_way += u in entries
                        u = int(parents[u])
                    assert on_the_way == 1, (wanted, share, cap, int(v), on_the_way)
                    u = int(v)
                    while u not in entries:
                        u = int(parents[u])
                    covered.add(u)
                assert covered == entries, "an entry without a surviving leaf below it"
                limit = expected_limit(10)
                out = chunk_arithmetic([10] * 17, [16] * 17, [len(cut)] * 17, list(range(17)))
                assert int(out[:, 3].max()) <= limit and int(out[:, 3].sum()) == len(cut)
                if int(survives.sum()) <= cap:
                    assert sorted(cut) == sorted(int(refs[v]) for v in np.nonzero(survives)[0])
            assert pruned_cut(refs, parents, kids, np.zeros(len(refs), np.uint8), 30) == []
            trees += 1
    assert trees == 15
