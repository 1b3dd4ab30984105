"""GPU tests (-m gpu) of the entry cuts' leaf pass (lens_trace_amd/csrc/lt_entry_cut.hpp: may_accept; lt_entry_cut_kernel;
traverse_shadow2): after the node lists, the build tests the triangles of the leaves a square's rays can reach against the shaft
from its stored camera hits towards the light box; a square none of whose leaves survives is marked clear and its two-frame
shadow walks are not run, a square with a few survivors walks those leaves alone.

Not a bit may change.  Every call is compared word for word with the same call in a fresh context with LT_ENTRY_CUT_LEAVES=0 (node
lists only) and in one with LT_ENTRY_CUT=0 (every walk from the root) and, in the portable flavour, with the CPU oracle's frames
folded by its own running mean.  The counters (RendererHIP.entry_cut_leaf_counts: clear squares, squares with a list of leaves,
entries) are printed per case; over the scenes some square must be clear and some must have a leaf list, and
RendererHIP.entry_cut_counts must report the node lists as it does without the pass.

Scenes: those of tests/entry_cut_scenes.py and the four of tests/entry_cut_leaf_scenes.py (a fine height field, a flat grid whose
pixel centres fall on shared edges and vertices, a ridge where a neighbour behind the origin occludes by a negative t, a small far
occluder that covers part of the light for a few pixels).  24x16, 17x9 and 9x9; 2, 3 and 5 frames from frame 1 and from frame 4; a
first call and reusing calls; an edit of primitives and one of lights in one context.  LT_HIP_LIBRARY=<a -DLT_NO_ASM_WALKS build>
runs the same file against the plain-C++ walk."""
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, make_desc
from oracle import pyoracle as po
from tests import mixed_axis_scenes as mx
from tests.entry_cut_leaf_scenes import NEW, SCENES, SIZES, scene

pytestmark = pytest.mark.gpu

COUNTS = (2, 3, 5)
FIRSTS = (1, 4)
ACC = C.PROGRAM_ACCUMULATOR
BASELINES = (("LT_ENTRY_CUT_LEAVES", "node lists only"), ("LT_ENTRY_CUT", "every walk from the root"))

_fresh = {}
_oracle = {}
_casting = {}
_seen = {}          # (name, W, H) -> (clear, lists, entries), for the test over all scenes at the end of the file


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches: the packet walk, frame groups
    monkeypatch.delenv("LT_ENTRY_CUT", raising=False)
    monkeypatch.delenv("LT_ENTRY_CUT_LEAVES", raising=False)


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def call(r, name, W, H, first=1, count=3, portable=False):
    s, cam = scene(name)
    r.set_scene(s)
    base = 0 if first == FIRSTS[0] else 3
    d = make_desc(ACC, W, H, 3, sc.camera_with_frame(cam, first), frame_first=first, frame_count=count, accumulate=True, accumulate_base=base,
                  portable_math=portable)
    out = start_pattern(r.output_floats(d))
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def fresh(monkeypatch, switch, name, W, H, **kw):
    """The same call in a context of its own with `switch` off."""
    key = (switch, name, W, H, tuple(sorted(kw.items())))
    if key not in _fresh:
        monkeypatch.setenv(switch, "0")
        r = RendererHIP(0)
        try:
            _fresh[key] = call(r, name, W, H, **kw)
            assert r.entry_cut_leaf_counts() == (0, 0, 0)
        finally:
            r.close()
            monkeypatch.delenv(switch)
    return _fresh[key]


def oracle_fold(name, W, H, first, count):
    s, cam = scene(name)
    acc = start_pattern(W * H * 3).reshape(H, W, 3)
    base = 0 if first == FIRSTS[0] else 3
    for i in range(count):
        k = (name, W, H, first + i)
        if k not in _oracle:
            _oracle[k] = po.render(s, sc.camera_with_frame(cam, first + i), W, H, po.ACCUMULATOR)
        po.accumulate(acc, _oracle[k], base + i)
    return acc.reshape(-1)


def assert_same(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), got.size)


def check(monkeypatch, r, name, W, H, what, **kw):
    got = call(r, name, W, H, **kw)
    for switch, means in BASELINES:
        assert_same(got, fresh(monkeypatch, switch, name, W, H, **kw), "%s %s %dx%d %r vs a fresh context with %s=0 (%s)" % (what, name, W, H, kw, switch, means))
    if kw.get("portable"):
        assert_same(got, oracle_fold(name, W, H, kw.get("first", 1), kw.get("count", 3)), "%s %s %dx%d %r vs the oracle's frames folded" % (what, name, W, H, kw))
    return got


def casting_squares(name, W, H):
    """The 8x8 squares with a pixel that casts shadow rays (tests/test_gpu_entry_cut.py: casting_squares)."""
    if (name, W, H) not in _casting:
        s, cam = scene(name)
        has = mx.camera_hits(s, cam, W, H)[0]
        _casting[(name, W, H)] = sum(1 for y in range(0, H, 8) for x in range(0, W, 8) if has[y:y + 8, x:x + 8].any())
    return _casting[(name, W, H)]


def node_counts(monkeypatch, name, W, H, portable):
    """entry_cut_counts of the same two calls with LT_ENTRY_CUT_LEAVES=0: what the node lists are without the pass."""
    monkeypatch.setenv("LT_ENTRY_CUT_LEAVES", "0")
    r = RendererHIP(0)
    try:
        call(r, name, W, H, portable=portable)
        call(r, name, W, H, portable=portable)
        return r.entry_cut_counts()
    finally:
        r.close()
        monkeypatch.delenv("LT_ENTRY_CUT_LEAVES")


def check_counts(r, name, W, H, builds_expected=1):
    builds, lists, entries = r.entry_cut_counts()
    clear, leaf_lists, leaf_entries = r.entry_cut_leaf_counts()
    casting = casting_squares(name, W, H)
    print("%s %dx%d: cut builds %d; node lists %d with %d entries; of %d casting squares %d clear, %d with a list of leaves (%d entries)" % (
        name, W, H, builds, lists, entries, casting, clear, leaf_lists, leaf_entries))
    assert builds == r.camera_hit_passes() == builds_expected
    assert clear + leaf_lists <= casting
    assert leaf_lists <= leaf_entries <= 15 * leaf_lists
    _seen[(name, W, H)] = (clear, leaf_lists, leaf_entries)
    return builds, lists, entries


def run_case(monkeypatch, name, W, H, portable):
    r = RendererHIP(0)
    try:
        for count in COUNTS:
            for first in (FIRSTS[0],) * 3 + FIRSTS[1:]:     # a first call, two reusing calls, then frame_first moved on
                check(monkeypatch, r, name, W, H, "call", first=first, count=count, portable=portable)
        assert r.camera_hit_passes() <= 1
        counts = check_counts(r, name, W, H)
        assert counts[1:] == node_counts(monkeypatch, name, W, H, portable)[1:], "the node lists' counters changed with the leaf pass"
    finally:
        r.close()


@pytest.mark.parametrize("portable", [True, False], ids=["portable", "default"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", SCENES)
def test_same_words_with_and_without_the_leaf_pass(monkeypatch, name, size, portable):
    run_case(monkeypatch, name, size[0], size[1], portable)


@pytest.mark.parametrize("edited", ["wall-edited-prims", "wall-edited-lights"])
def test_an_edit_rebuilds_the_leaf_lists(monkeypatch, edited):
    """The wall, the wall with primitives or lights edited (lt_hip_set_scene's edit path), the wall again, each rendered twice: a
    build each in the call that reuses its hits, every image a fresh context's, and the wall's leaf counters the same before and
    after the edit."""
    W, H = 24, 16
    r = RendererHIP(0)
    try:
        leaf = []
        for i, name in enumerate(("wall", edited, "wall")):
            check(monkeypatch, r, name, W, H, "edit %d" % i, portable=True)
            assert r.entry_cut_leaf_counts() == (0, 0, 0)      # (a call that runs its own pass builds none, and the old cuts are gone)
            check(monkeypatch, r, name, W, H, "edit %d, reusing" % i, first=4, portable=True)
            check_counts(r, name, W, H, i + 1)
            leaf.append(r.entry_cut_leaf_counts())
        assert leaf[0] == leaf[2] and sum(leaf[0]) > 0
        check(monkeypatch, r, "wall", W, H, "after the edits", first=4, count=5, portable=True)
        assert r.entry_cut_counts()[0] == 3
    finally:
        r.close()


def test_switch_off(monkeypatch):
    monkeypatch.setenv("LT_ENTRY_CUT_LEAVES", "0")
    r = RendererHIP(0)
    try:
        call(r, "fine-field", 24, 16)
        call(r, "fine-field", 24, 16, first=4)
        builds, lists, entries = r.entry_cut_counts()
        assert r.camera_hit_passes() == 1 and builds == 1 and entries > lists > 0 and r.entry_cut_leaf_counts() == (0, 0, 0)
    finally:
        r.close()


def test_some_scene_has_clear_squares_and_some_a_leaf_list(monkeypatch):
    """Non-vacuity over the scenes (the cases above have filled _seen; alone, this test renders the new scenes itself)."""
    if not any(k[0] in NEW for k in _seen):
        for name in NEW:
            r = RendererHIP(0)
            try:
                call(r, name, 24, 16)
                call(r, name, 24, 16, first=4)
                check_counts(r, name, 24, 16)
            finally:
                r.close()
    clear = sorted(k for k, v in _seen.items() if v[0] > 0)
    listed = sorted(k for k, v in _seen.items() if v[1] > 0)
    print("clear squares in %d cases, leaf lists in %d of %d" % (len(clear), len(listed), len(_seen)))
    assert clear and listed
