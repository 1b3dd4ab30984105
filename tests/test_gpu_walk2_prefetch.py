"""GPU tests (-m gpu) of the two-frame walk's leaf runs (lens_trace_amd/csrc/lt_walk_asm.hpp: LT_ASM_LEAF2_RUN): while a leaf's two
frame tests run, the record of the leaf under it on the stack is fetched into the other register bank, and the leaf body exists
once per bank.  The same leaves meet the same tests in the same order, so not a bit may change.

Every call runs in a context whose buffers were poisoned before use (LT_DEBUG_POISON) -- a first call and reusing calls; 2, 3 and 5
frames from frame 1 and from frame 4; LT_SHADOW_PACKETS=1 -- and is compared word for word with the same call in a fresh context
with LT_ENTRY_CUT=0, whose walks start at the root.  Scenes: those of tests/entry_cut_chunk_scenes.py (the grazing field keeps 3 to
242 leaves per square) and tests/walk2_prefetch_scenes.py's shaded field, at 24x16, 17x9 and 9x9, under the default caps of the
lists and under LT_ENTRY_CUT_CHUNKS = LT_ENTRY_CUT_NODE_CHUNKS = 1, 2, 4 and 16.  LT_HIP_LIBRARY=<a -DLT_NO_ASM_WALKS build> runs
the same file against the plain-C++ walk, which has no banks; a dump made with that build is compared across builds by
tests/tools/ab_compare.py.

What the walks ran through is read back, not guessed: the cuts as the walk reads them (lt_hip_read_entry_cuts) and the records
their entries name (lt_hip_read_scene_structure kind 4).  test_the_cases_hold_what_the_two_banks_can_get_wrong asserts that the
cases taken together contain a record of leaves alone -- one run, popped from its top entry down, the first leaf in bank 0 and then alternating -- with
1, 2, an odd number above 2, an even number above 2 and 15 entries (so runs that end in bank 0 and in bank 1); a record with a
leaf directly over a node and one with a node directly over a leaf; a square whose own primitive -- the `ignore` of some lane --
is popped at an even and at an odd position of a run; and a walking square of the shaded field, every pixel of which is exactly
0.0f after a call of two frames (both frames' rays of every lane occluded: an unoccluded sample adds diffuse * n.l), whose list
holds the shading triangle's leaf anywhere but at the bottom of its last record: the walk ended with entries left.

Which square a record belongs to: these images have at most six squares, fewer than the eight shares of the hand-out order
(lt_capi.hip: ensure_square_order), so every share is one square and hand-out position p is the row-major square p.

Mutated copies of the library that fail this file (stated in the commit that added it): the bank-1 leaf comparing bank 0's
primitive word with `ignore`; the interior node under a leaf not put back when no leaf could be fetched ahead; the second of two
consecutive leaves tested with the first one's registers."""
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, make_desc, make_rays, reference_camera_rays
from tests.walk2_prefetch_scenes import SCENES, SIZES, scene, shade_primitive

pytestmark = pytest.mark.gpu

COUNTS = (2, 3, 5)
FIRSTS = (1, 1, 4)      # a first call, a reusing call, frame_first moved on
CAPS = (None, 1, 2, 4, 16)      # None: neither switch set
ACC = C.PROGRAM_ACCUMULATOR
POISON = "0xa5"
CLEAR = 0xffffffff
LEAF = 0x80000000

_fresh = {}
_runs = {}
_own = {}


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches: the packet walk, frame groups
    for name in ("LT_ENTRY_CUT", "LT_ENTRY_CUT_LEAVES", "LT_ENTRY_CUT_CHUNKS", "LT_ENTRY_CUT_NODE_CHUNKS", "LT_DEBUG_POISON"):
        monkeypatch.delenv(name, raising=False)


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def call(r, name, W, H, first, count):
    s, cam = scene(name)
    r.set_scene(s)
    base = 0 if first == 1 else 3
    d = make_desc(ACC, W, H, 3, sc.camera_with_frame(cam, first), frame_first=first, frame_count=count, accumulate=True, accumulate_base=base)
    out = start_pattern(r.output_floats(d))
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def fresh(monkeypatch, name, W, H, first, count):
    """The same call in a context of its own whose walks start at the root."""
    key = (name, W, H, first, count)
    if key not in _fresh:
        monkeypatch.setenv("LT_ENTRY_CUT", "0")
        r = RendererHIP(0)
        try:
            _fresh[key] = call(r, name, W, H, first, count)
            assert r.entry_cuts() is None
        finally:
            r.close()
            monkeypatch.delenv("LT_ENTRY_CUT")
    return _fresh[key]


def run(monkeypatch, name, W, H, cap):
    """Every call of one poisoned context under one cap: {"images": {(count, call index): words}, "cuts", "planes", "pairs"}."""
    key = (name, W, H, cap)
    if key in _runs:
        return _runs[key]
    monkeypatch.setenv("LT_DEBUG_POISON", POISON)      # (read when the context is created)
    r = RendererHIP(0)
    monkeypatch.delenv("LT_DEBUG_POISON")
    if cap is not None:
        monkeypatch.setenv("LT_ENTRY_CUT_CHUNKS", str(cap))
        monkeypatch.setenv("LT_ENTRY_CUT_NODE_CHUNKS", str(cap))
    try:
        images = {}
        for count in COUNTS:
            for i, first in enumerate(FIRSTS):
                images[(count, i)] = call(r, name, W, H, first, count)
        assert r.camera_hit_passes() == 1 and r.entry_cut_counts()[0] == 1
        cuts = r.entry_cuts()
        planes = r.entry_cut_chunk_counts()["chunks"]
        pairs = r.scene_structure(4)
        _runs[key] = {"images": images, "cuts": cuts, "planes": planes, "pairs": None if pairs is None else pairs.view(np.uint32).reshape(-1, 16)}
    finally:
        r.close()
        monkeypatch.delenv("LT_ENTRY_CUT_CHUNKS", raising=False)
        monkeypatch.delenv("LT_ENTRY_CUT_NODE_CHUNKS", raising=False)
    return _runs[key]


def assert_same(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), got.size)


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", SCENES)
def test_same_words_as_walks_from_the_root(monkeypatch, name, size):
    W, H = size
    for cap in CAPS:
        got = run(monkeypatch, name, W, H, cap)
        for (count, i), image in got["images"].items():
            assert_same(image, fresh(monkeypatch, name, W, H, FIRSTS[i], count),
                        "%s %dx%d, cap %r, %d frames, call %d (from frame %d) vs a fresh context with LT_ENTRY_CUT=0" % (name, W, H, cap, count, i, FIRSTS[i]))


def squares_of(W, H):
    bx, by = (W + 7) // 8, (H + 7) // 8
    return [(8 * (p % bx), 8 * (p // bx), min(8 * (p % bx) + 8, W), min(8 * (p // bx) + 8, H)) for p in range(bx * by)]


def lists_of(got, n):
    """Per hand-out position: None (marked clear), or the records of the square's list as the walk goes through them -- each the
    entries in stack order, index 0 at the bottom; no record: the walk starts at the root."""
    cuts, planes = got["cuts"], got["planes"]
    assert cuts is not None and cuts.shape == (planes * n, 16)
    out = []
    for p in range(n):
        if int(cuts[p, 0]) == CLEAR:
            out.append(None)
            continue
        records = []
        for c in range(planes):
            count = int(cuts[c * n + p, 0])
            if not 1 <= count <= 15:      # (packet_walk2's guard: a word that is no count of a further record ends the list)
                break
            records.append(cuts[c * n + p, 1:1 + count].copy())
        out.append(records)
    return out


def own_primitives(name, W, H):
    """[H, W]: the primitive under each pixel's camera ray (-1: none)."""
    key = (name, W, H)
    if key not in _own:
        s, cam = scene(name)
        r = RendererHIP(0)
        try:
            r.set_scene(s)
            o, d, _, _ = reference_camera_rays(cam, W, H)
            _own[key] = r.trace_rays(make_rays(o, d))["prim"].astype(np.int64).reshape(H, W)
        finally:
            r.close()
    return _own[key]


def test_the_cases_hold_what_the_two_banks_can_get_wrong(monkeypatch):
    leaf_counts, mixed = set(), set()
    own_parity = set()
    ended_early = []
    for name in SCENES:
        s = scene(name)[0]
        lights = set(int(p) for p in s.light_view[0]["primitives"][:int(s.light_view[0]["count"])])
        for W, H in SIZES:
            squares = squares_of(W, H)
            assert len(squares) < 8
            own = own_primitives(name, W, H)
            for cap in CAPS:
                got = run(monkeypatch, name, W, H, cap)
                if got["cuts"] is None:
                    continue
                pairs = got["pairs"]
                for p, records in enumerate(lists_of(got, len(squares))):
                    if not records:
                        continue
                    x0, y0, x1, y1 = squares[p]
                    mine = set(int(v) for v in own[y0:y1, x0:x1].ravel())
                    all_leaves = all(bool((rec & LEAF).all()) for rec in records)
                    for rec in records:
                        leaf = (rec & LEAF) != 0
                        if leaf.all():
                            leaf_counts.add(len(rec))
                            for i, e in enumerate(rec):
                                if int(pairs[int(e) & 0x7fffffff, 15]) in mine:
                                    own_parity.add((len(rec) - 1 - i) % 2)      # (its position in the run: the top entry is popped first)
                        for i in range(len(rec) - 1):
                            if leaf[i + 1] != leaf[i]:
                                mixed.add("leaf over node" if leaf[i + 1] else "node over leaf")
                    if name == "shaded-field" and not all_leaves:
                        print("shaded-field %dx%d cap %r square %d: a list of nodes, records %r" % (W, H, cap, p, [len(rec) for rec in records]))
                    if name == "shaded-field" and all_leaves:
                        shade = shade_primitive(s)
                        where = [(c, i) for c, rec in enumerate(records) for i, e in enumerate(rec) if int(pairs[int(e) & 0x7fffffff, 15]) == shade]
                        block = own[y0:y1, x0:x1]
                        casting = (block >= 0).all() and shade not in mine and not (mine & lights)
                        # (the calls from frame 1 overwrite the buffer: the first call, whose walks start at the root, and the reusing one)
                        dark = all((got["images"][(2, i)].reshape(H, W, 3)[y0:y1, x0:x1] == 0.0).all() for i in (0, 1))
                        print("shaded-field %dx%d cap %r square %d: shade at %r of records %r, casting %s, dark %s" % (
                            W, H, cap, p, where, [len(rec) for rec in records], casting, dark))
                        if len(where) == 1 and where[0] != (len(records) - 1, 0) and casting and dark:
                            ended_early.append((W, H, cap, p, where[0], [len(rec) for rec in records]))
    print("records of leaves alone have %r entries; mixed records hold %r; a square's own primitive is popped at run positions of parity %r; "
          "shaded squares whose walk ends with entries left: %r" % (sorted(leaf_counts), sorted(mixed), sorted(own_parity), ended_early[:6]))
    assert {1, 2, 15} <= leaf_counts
    assert any(c > 2 and c % 2 == 1 for c in leaf_counts) and any(c > 2 and c % 2 == 0 for c in leaf_counts)
    assert {(c - 1) % 2 for c in leaf_counts} == {0, 1}      # the bank of a run's last leaf
    assert mixed == {"leaf over node", "node over leaf"}
    assert own_parity == {0, 1}
    assert ended_early


def test_the_read_back_is_the_cuts_the_context_holds(monkeypatch):
    """lt_hip_read_entry_cuts: nothing before a reusing call has built cuts, then one plane of one record per square
    for every record a list may take, every first word a count, 0 .. 15, or the clear mark; nothing again once the scene is set anew."""
    W, H = 17, 9
    monkeypatch.setenv("LT_ENTRY_CUT_CHUNKS", "4")
    r = RendererHIP(0)
    try:
        call(r, "grazing-field", W, H, 1, 2)
        assert r.entry_cuts() is None
        call(r, "grazing-field", W, H, 1, 2)
        cuts = r.entry_cuts()
        assert cuts.dtype == np.uint32 and cuts.shape == (4 * 6, 16)
        assert ((cuts[:, 0] <= 15) | ((cuts[:, 0] == CLEAR) & (np.arange(len(cuts)) < 6))).all()
        # ... and they are the cuts the counters speak of: the squares marked clear, the squares by the records their list takes
        assert int((cuts[:6, 0] == CLEAR).sum()) == r.entry_cut_leaf_counts()[0]
        taken = [len(records) for records in lists_of({"cuts": cuts, "planes": 4}, 6) if records]
        by = r.entry_cut_chunk_counts()["squares_by_chunks"]
        assert all(by[k] == taken.count(k) for k in range(2, 17)) and max(taken) > 1
        call(r, "fine-field", W, H, 1, 2)
        assert r.entry_cuts() is None
    finally:
        r.close()
