"""GPU tests (-m gpu) of entry cuts that take several 64-byte records (lens_trace_amd/csrc/lt_entry_cut.hpp: Chunks;
lt_entry_cut_kernel; packet_walk2): with LT_ENTRY_CUT_CHUNKS=N a square's list -- of nodes, or of the leaves that survive the leaf
pass -- may take up to N records of at most fifteen entries, and the square's two-frame shadow walk goes through them one after the
other with the rays that are still unoccluded.

Not a bit may change.  Every call runs in a context whose buffers were poisoned before use (LT_DEBUG_POISON) and is compared word
for word with the same call in a fresh context with LT_ENTRY_CUT_CHUNKS=1 (one record per list, as before there were chunks) and in
one with LT_ENTRY_CUT=0 (every walk from the root).  The counters (RendererHIP.entry_cut_chunk_counts) are printed per case and
asserted: some square's list takes exactly two records and some square's takes N, there is a list of leaves longer than fifteen, a
cut over the pruned tree and a node list longer than fifteen.

Scenes: those of tests/entry_cut_leaf_scenes.py and tests/entry_cut_chunk_scenes.py's grazing field, whose squares keep from 20 to
240 leaves.  24x16, 17x9 and 9x9; 2, 3 and 5 frames from frame 1 and from frame 4; a first call and reusing calls; an edit of
primitives and one of lights in one context.  LT_HIP_LIBRARY=<a -DLT_NO_ASM_WALKS build> runs the same file against the plain-C++
walk."""
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, make_desc
from tests.entry_cut_chunk_scenes import SCENES, SIZES, scene

pytestmark = pytest.mark.gpu

COUNTS = (2, 3, 5)
FIRSTS = (1, 4)
ACC = C.PROGRAM_ACCUMULATOR
CHUNKS = 4          # the cap of the cases over all scenes; the grazing field also runs with 2, 8 and 16
BASELINES = (("LT_ENTRY_CUT_CHUNKS", "1", "one record per list"), ("LT_ENTRY_CUT", "0", "every walk from the root"))
POISON = "0xa5"     # (as a count: 0xa5a5a5a5 entries)

_fresh = {}


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches: the packet walk, frame groups
    for name in ("LT_ENTRY_CUT", "LT_ENTRY_CUT_LEAVES", "LT_ENTRY_CUT_CHUNKS", "LT_ENTRY_CUT_NODE_CHUNKS", "LT_DEBUG_POISON"):
        monkeypatch.delenv(name, raising=False)


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def call(r, name, W, H, first=1, count=3):
    s, cam = scene(name)
    r.set_scene(s)
    base = 0 if first == FIRSTS[0] else 3
    d = make_desc(ACC, W, H, 3, sc.camera_with_frame(cam, first), frame_first=first, frame_count=count, accumulate=True, accumulate_base=base)
    out = start_pattern(r.output_floats(d))
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def fresh(monkeypatch, switch, value, name, W, H, **kw):
    """The same call in a context of its own with `switch` set to `value`."""
    key = (switch, name, W, H, tuple(sorted(kw.items())))
    if key not in _fresh:
        monkeypatch.setenv(switch, value)
        r = RendererHIP(0)
        try:
            _fresh[key] = call(r, name, W, H, **kw)
            assert sum(r.entry_cut_chunk_counts()["squares_by_chunks"][k] for k in range(2, 17)) == 0
        finally:
            r.close()
            monkeypatch.delenv(switch)
    return _fresh[key]


def poisoned(monkeypatch, chunks):
    """A context whose buffers are filled with POISON before their first use, building lists of up to `chunks` records."""
    monkeypatch.setenv("LT_DEBUG_POISON", POISON)      # (read when the context is created)
    r = RendererHIP(0)
    monkeypatch.delenv("LT_DEBUG_POISON")
    monkeypatch.setenv("LT_ENTRY_CUT_CHUNKS", str(chunks))
    monkeypatch.setenv("LT_ENTRY_CUT_NODE_CHUNKS", str(chunks))      # (lists of nodes as long as lists of leaves: by default they end at two records)
    return r


def assert_same(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), got.size)


def check(monkeypatch, r, chunks, name, W, H, what, **kw):
    got = call(r, name, W, H, **kw)
    monkeypatch.delenv("LT_ENTRY_CUT_CHUNKS")
    for switch, value, means in BASELINES:
        assert_same(got, fresh(monkeypatch, switch, value, name, W, H, **kw),
                    "%s %s %dx%d %r with %d chunks vs a fresh context with %s=%s (%s)" % (what, name, W, H, kw, chunks, switch, value, means))
    monkeypatch.setenv("LT_ENTRY_CUT_CHUNKS", str(chunks))
    return got


def check_counts(r, chunks, name, W, H, builds_expected=1):
    builds = r.entry_cut_counts()[0]
    leaf_lists, leaf_entries = r.entry_cut_leaf_counts()[1:]
    c = r.entry_cut_chunk_counts()
    by = c["squares_by_chunks"]
    print("%s %dx%d, %d chunks: cut builds %d; lists of leaves in one record %d (%d entries), in several %d (%d entries); cuts over the pruned "
          "tree %d (%d entries); node lists in several records %d (%d entries); squares by records %r" % (
              name, W, H, chunks, builds, leaf_lists, leaf_entries, c["leaf"][0], c["leaf"][1], c["pruned"][0], c["pruned"][1], c["plain"][0],
              c["plain"][1], {k: v for k, v in by.items() if v}))
    assert builds == r.camera_hit_passes() == builds_expected
    assert c["chunks"] == chunks and all(by[k] == 0 for k in range(chunks + 1, 17))
    assert leaf_lists <= leaf_entries <= 15 * leaf_lists
    for squares, entries in (c["leaf"], c["pruned"], c["plain"]):
        assert 15 * squares < entries <= 15 * chunks * squares or squares == entries == 0
    if chunks > 1:      # (a cut over the pruned tree stands for more leaves than the cap: it has at least cap - 1 entries)
        assert c["pruned"][1] >= (15 * chunks - 1) * c["pruned"][0]
    assert sum(by[k] for k in range(2, 17)) == c["leaf"][0] + c["pruned"][0] + c["plain"][0]
    return c


def run_case(monkeypatch, chunks, name, W, H):
    r = poisoned(monkeypatch, chunks)
    try:
        for count in COUNTS:
            for first in (FIRSTS[0],) * 3 + FIRSTS[1:]:     # a first call, two reusing calls, then frame_first moved on
                check(monkeypatch, r, chunks, name, W, H, "call", first=first, count=count)
        assert r.camera_hit_passes() <= 1
        check_counts(r, chunks, name, W, H)
    finally:
        r.close()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", SCENES)
def test_same_words_with_lists_of_several_records(monkeypatch, name, size):
    run_case(monkeypatch, CHUNKS, name, size[0], size[1])


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("chunks", [2, 8, 16])
def test_grazing_field_under_other_caps(monkeypatch, chunks, size):
    run_case(monkeypatch, chunks, "grazing-field", size[0], size[1])


@pytest.mark.parametrize("edited", ["grazing-field-edited-prims", "grazing-field-edited-lights"])
def test_an_edit_rebuilds_the_chunks(monkeypatch, edited):
    """The grazing field, the field with primitives or lights edited (lt_hip_set_scene's edit path), the field again, each rendered
    twice: a build each in the call that reuses its hits, every image a fresh context's, and the field's counters the same before
    and after the edit."""
    W, H = 17, 9
    r = poisoned(monkeypatch, CHUNKS)
    try:
        seen = []
        for i, name in enumerate(("grazing-field", edited, "grazing-field")):
            check(monkeypatch, r, CHUNKS, name, W, H, "edit %d" % i)
            assert sum(r.entry_cut_chunk_counts()["squares_by_chunks"].values()) == 0      # (a call that runs its own pass builds none, and the old cuts are gone)
            check(monkeypatch, r, CHUNKS, name, W, H, "edit %d, reusing" % i, first=4)
            seen.append(check_counts(r, CHUNKS, name, W, H, i + 1))
        assert seen[0] == seen[2] and seen[0]["leaf"][0] + seen[0]["pruned"][0] + seen[0]["plain"][0] > 0
        check(monkeypatch, r, CHUNKS, "grazing-field", W, H, "after the edits", first=4, count=5)
        assert r.entry_cut_counts()[0] == 3
    finally:
        r.close()


def test_another_cap_rebuilds_the_lists(monkeypatch):
    """One context, the cap changed between reusing calls: the lists are built again for the new cap, and the images stay."""
    W, H = 17, 9
    r = poisoned(monkeypatch, 2)
    try:
        check(monkeypatch, r, 2, "grazing-field", W, H, "first")
        for i, chunks in enumerate((2, 8, 1, 4)):
            monkeypatch.setenv("LT_ENTRY_CUT_CHUNKS", str(chunks))
            check(monkeypatch, r, chunks, "grazing-field", W, H, "reusing, cap %d" % chunks, first=4)
            c = check_counts(r, chunks, "grazing-field", W, H, builds_expected=1) if i == 0 else r.entry_cut_chunk_counts()
            assert c["chunks"] == chunks and r.entry_cut_counts()[0] == i + 1 and r.camera_hit_passes() == 1
    finally:
        r.close()


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_grazing_field_under_the_default_caps(monkeypatch, size):
    """Neither switch set: lists of leaves of up to sixteen records, lists of nodes of up to two."""
    W, H = size
    r = poisoned(monkeypatch, 16)
    monkeypatch.delenv("LT_ENTRY_CUT_CHUNKS")
    monkeypatch.delenv("LT_ENTRY_CUT_NODE_CHUNKS")
    try:
        for first in (1, 1, 4):
            got = call(r, "grazing-field", W, H, first=first)
            for switch, value, means in BASELINES:
                assert_same(got, fresh(monkeypatch, switch, value, "grazing-field", W, H, first=first), "default caps, grazing-field %dx%d first %d vs %s=%s" % (W, H, first, switch, value))
        c = r.entry_cut_chunk_counts()
        print("grazing-field %dx%d, default caps: %r" % (W, H, c))
        # (the squares of 24x16 keep 75 - 116 leaves by the CPU's count: five records and more; no square keeps the 226 - 240 that
        # take sixteen, which test_grazing_field_under_other_caps reaches with node lists)
        assert c["chunks"] == 16 and c["plain"][1] <= 30 * c["plain"][0] and c["leaf"][0] + c["plain"][0] > 0
        if (W, H) == (24, 16):
            assert sum(c["squares_by_chunks"][k] for k in range(5, 17)) > 0
    finally:
        r.close()


def counts_of(monkeypatch, chunks, W, H, budget=None):
    """The counters of the grazing field's cuts under a cap (for lists of leaves and of nodes alike) and a budget of the leaf pass."""
    r = poisoned(monkeypatch, chunks)
    if budget is not None:
        monkeypatch.setenv("LT_ENTRY_CUT_LEAVES", str(budget))
    try:
        call(r, "grazing-field", W, H)
        call(r, "grazing-field", W, H, first=4)
        return check_counts(r, chunks, "grazing-field", W, H)
    finally:
        r.close()
        monkeypatch.delenv("LT_ENTRY_CUT_LEAVES", raising=False)


def test_some_list_takes_two_records_and_some_takes_the_cap(monkeypatch):
    """Non-vacuity, by the counters of the grazing field's cuts, which this test builds itself, under every cap of this file.  By
    the CPU's count (tests/test_entry_cut_chunks_cpu.py) squares keep 20, 27 and 29 leaves -- two records --, and squares keep
    more leaves than any cap but sixteen allows: their list fills the cap, whatever its kind.  The leaf pass of the six squares of
    24x16 (75 - 116 leaves) and of two squares of 17x9 (44, 46) finishes within its 512 records: under the caps of 30 and 60
    entries that they exceed, their lists are cuts over the pruned tree.  With a budget of 64 records no pass over more than 32
    leaves finishes: those squares keep their node lists."""
    for chunks in (2, CHUNKS, 8, 16):
        cases = [counts_of(monkeypatch, chunks, W, H) for W, H in SIZES]
        two = sum(v["squares_by_chunks"][2] for v in cases)
        full = sum(v["squares_by_chunks"][chunks] for v in cases)
        leaf = sum(v["leaf"][0] for v in cases)
        pruned = sum(v["pruned"][0] for v in cases)
        plain = sum(v["plain"][0] for v in cases)
        print("%d chunks: %d squares with two records, %d with %d; lists longer than fifteen: %d of leaves, %d cuts over the pruned tree, %d of nodes" % (
            chunks, two, full, chunks, leaf, pruned, plain))
        assert two > 0 and full > 0 and leaf > 0, chunks
        if chunks in (2, CHUNKS):
            assert pruned > 0, chunks
    short = counts_of(monkeypatch, CHUNKS, 24, 16, budget=64)
    assert short["plain"][0] > 0 and short["pruned"][0] == 0 and short["plain"][1] > 15 * short["plain"][0]
