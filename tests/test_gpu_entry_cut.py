"""GPU tests (-m gpu) of the entry cut (lens_trace_amd/csrc/lt_entry_cut.hpp, lt_entry_cut_kernel, LT_ASM_WALK2's prologue): with the
camera hits that accumulator keeps, every square keeps a list of at most fifteen nodes of the own tree that its shadow rays can reach
at all, and the two-frame shadow walks of the square start there instead of the root.

Not a bit may change.  Every call is compared word for word with the same call in a fresh context with LT_ENTRY_CUT=0 (every walk
from the root) and, in the portable flavour, with the CPU oracle's frames folded by its own running mean.  The counter
(RendererHIP.entry_cut_counts: builds, squares with a non-empty list, entries) says that the lists are there: more than half of the
squares that cast shadow rays at all have one (casting_squares) and a list has more than one entry on average -- in every scene but the one with two lights far apart, whose
cut may be fat or empty and must still be exact.

Shapes: 24x16, 17x9 (a one-column and a single-pixel square: the walk runs with lanes off and its stack register parked) and 9x9;
2, 3 and 5 frames from frame 1 and from frame 4; a first call and
reusing calls.  Scenes: synth.heightfield_wall(24); every form of tests/mixed_axis_scenes.py, its two-mixed-axes scene and its
penumbra; the Cornell golden scene (the light's box lies over the receivers: origins inside the slab); two lights far apart; and a
floor in the plane y = 0 with a light in that same plane (every ray towards it has a direction component of exactly 0) beside one
above; and a wide light whose outer quarter alone is hidden by an occluder (a cut made for too small a light box loses it).  Edits of primitives and of lights in one context rebuild the cuts; tile descs as the multi-GPU split makes them."""
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, make_desc
from oracle import pyoracle as po
from tests import mixed_axis_scenes as mx
from tests.entry_cut_scenes import SCENES, SIZES, scene

pytestmark = pytest.mark.gpu

COUNTS = (2, 3, 5)
FIRSTS = (1, 4)
ACC = C.PROGRAM_ACCUMULATOR

_fresh = {}
_oracle = {}


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches: the packet walk, frame groups
    monkeypatch.delenv("LT_ENTRY_CUT", raising=False)


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def call(r, name, W, H, first=1, count=3, tile=None, portable=False):
    s, cam = scene(name)
    r.set_scene(s)
    base = 0 if first == FIRSTS[0] else 3
    d = make_desc(ACC, W, H, 3, sc.camera_with_frame(cam, first), frame_first=first, frame_count=count, accumulate=True, accumulate_base=base,
                  tile=tile, portable_math=portable)
    out = start_pattern(r.output_floats(d))
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def fresh(monkeypatch, name, W, H, **kw):
    """The same call in a context of its own whose walks all start at the root."""
    key = (name, W, H, tuple(sorted(kw.items())))
    if key not in _fresh:
        monkeypatch.setenv("LT_ENTRY_CUT", "0")
        r = RendererHIP(0)
        try:
            _fresh[key] = call(r, name, W, H, **kw)
            assert r.entry_cut_counts() == (0, 0, 0)
        finally:
            r.close()
            monkeypatch.delenv("LT_ENTRY_CUT")
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


def oracle_fold_tiled(name, W, H, first, count, tile, floats):
    """oracle_fold in a tile desc's layout: tile k of the call (tile_first + k * tile_stride of the image's tiles, row-major) at
    [k]; and the mask of the floats that belong to pixels of the image (what an edge tile holds beyond it is nobody's)."""
    tw, th, t0, stride = tile
    s, cam = scene(name)
    base = 0 if first == FIRSTS[0] else 3
    out = start_pattern(floats).reshape(-1, th, tw, 3)
    inside = np.zeros(out.shape, bool)
    tiles_x, tiles_y = (W + tw - 1) // tw, (H + th - 1) // th
    assert out.shape[0] == len(range(t0, tiles_x * tiles_y, stride))
    for i in range(count):
        k = (name, W, H, first + i)
        if k not in _oracle:
            _oracle[k] = po.render(s, sc.camera_with_frame(cam, first + i), W, H, po.ACCUMULATOR)
    for j, t in enumerate(range(t0, tiles_x * tiles_y, stride)):
        x0, y0 = (t % tiles_x) * tw, (t // tiles_x) * th
        w, h = min(tw, W - x0), min(th, H - y0)
        acc = np.ascontiguousarray(out[j, :h, :w])
        for i in range(count):
            po.accumulate(acc, np.ascontiguousarray(_oracle[(name, W, H, first + i)].reshape(H, W, 3)[y0:y0 + h, x0:x0 + w]), base + i)
        out[j, :h, :w] = acc
        inside[j, :h, :w] = True
    return out.reshape(-1), inside.reshape(-1)


def assert_same(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), got.size)


def check(monkeypatch, r, name, W, H, what, **kw):
    got = call(r, name, W, H, **kw)
    assert_same(got, fresh(monkeypatch, name, W, H, **kw), "%s %s %dx%d %r vs a fresh context with LT_ENTRY_CUT=0" % (what, name, W, H, kw))
    if kw.get("portable"):
        first, count = kw.get("first", 1), kw.get("count", 3)
        if kw.get("tile") is None:
            want, inside = oracle_fold(name, W, H, first, count), slice(None)
        else:
            want, inside = oracle_fold_tiled(name, W, H, first, count, kw["tile"], got.size)
        assert_same(got[inside], want[inside], "%s %s %dx%d %r vs the oracle's frames folded" % (what, name, W, H, kw))
    return got


_casting = {}


def casting_squares(name, W, H):
    """The 8x8 squares with a pixel that casts shadow rays -- its camera ray hits a surface that is no light (the oracle's hits,
    mixed_axis_scenes.camera_hits).  Only those have a shadow walk, and so a reader of their list: they are the squares the
    non-vacuity bound speaks of (a square of background pixels gets the empty list and nothing ever looks at it)."""
    if (name, W, H) not in _casting:
        s, cam = scene(name)
        has = mx.camera_hits(s, cam, W, H)[0]
        _casting[(name, W, H)] = sum(1 for y in range(0, H, 8) for x in range(0, W, 8) if has[y:y + 8, x:x + 8].any())
    return _casting[(name, W, H)]


def check_lists(r, name, W, H, builds_expected=1):
    """Non-vacuity, by the counter: printed, then asserted."""
    builds, lists, entries = r.entry_cut_counts()
    casting = casting_squares(name, W, H)
    print("%s %dx%d: passes %d, cut builds %d, %d of %d casting squares with a list, %d entries" % (name, W, H, r.camera_hit_passes(), builds, lists, casting, entries))
    assert builds == r.camera_hit_passes() == builds_expected
    assert lists <= casting
    if name != "two-lights":
        assert 2 * lists > casting, (name, W, H, lists, casting)
        assert entries > lists, (name, W, H, lists, entries)
    return builds, lists, entries


def run_case(monkeypatch, name, W, H, portable):
    """The call that runs the camera-hit pass walks from the root; the first call that reuses its hits builds the cuts and walks
    from them, the later ones find them there: one pass, one build."""
    r = RendererHIP(0)
    try:
        for count in COUNTS:
            for first in (FIRSTS[0],) * 3 + FIRSTS[1:]:     # a first call, two reusing calls, then frame_first moved on
                check(monkeypatch, r, name, W, H, "call", first=first, count=count, portable=portable)
        assert r.camera_hit_passes() <= 1
        check_lists(r, name, W, H)
    finally:
        r.close()


@pytest.mark.parametrize("portable", [True, False], ids=["portable", "default"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", SCENES)
def test_same_words_with_and_without_cuts(monkeypatch, name, size, portable):
    run_case(monkeypatch, name, size[0], size[1], portable)


@pytest.mark.parametrize("portable", [True, False], ids=["portable", "default"])
@pytest.mark.parametrize("case", sorted(mx.PENUMBRA_CASES))
def test_penumbra(monkeypatch, case, portable):
    c = mx.PENUMBRA_CASES[case]
    run_case(monkeypatch, "penumbra-" + case, c["W"], c["H"], portable)


@pytest.mark.parametrize("edited", ["wall-edited-prims", "wall-edited-lights"])
def test_an_edit_rebuilds_the_cuts(monkeypatch, edited):
    """The wall, the wall with primitives or lights edited (the nodes stay: lt_hip_set_scene's edit path), the wall again, each
    rendered twice: a pass each and, in the call that reuses its hits, a build each, every image a fresh context's; then one more
    reusing call: no fourth."""
    W, H = 24, 16
    r = RendererHIP(0)
    try:
        for i, name in enumerate(("wall", edited, "wall")):
            check(monkeypatch, r, name, W, H, "edit %d" % i, portable=True)
            assert r.entry_cut_counts() == (i, 0, 0)      # (a call that runs its own pass builds none, and the old cuts are gone)
            check(monkeypatch, r, name, W, H, "edit %d, reusing" % i, first=4, portable=True)
            check_lists(r, name, W, H, i + 1)
        check(monkeypatch, r, "wall", W, H, "after the edits", first=4, count=5, portable=True)
        assert r.entry_cut_counts()[0] == 3
    finally:
        r.close()


# (8-pixel tiles of 24x16: tiles 1, 3, 4 and 5 are head squares; 16x8 tiles of 40x24: interleaved as two ranks take them)
TILES = [("wall", 24, 16, (8, 8, 0, 2)), ("wall", 24, 16, (8, 8, 0, 3)), ("wall", 40, 24, (16, 8, 1, 2)), ("cornell", 40, 24, (16, 8, 0, 2))]


@pytest.mark.parametrize("name,W,H,tile", TILES, ids=["%s-%dx%d-%s" % (n, w, h, "_".join(map(str, t))) for n, w, h, t in TILES])
def test_tile_descs(monkeypatch, name, W, H, tile):
    r = RendererHIP(0)
    try:
        for i, portable in enumerate((True, False)):
            for first, count in ((1, 3), (1, 3), (4, 5), (1, 2)):
                check(monkeypatch, r, name, W, H, "tiles", first=first, count=count, tile=tile, portable=portable)
            builds, lists, entries = r.entry_cut_counts()
            print("%s %dx%d tile %r: builds %d, lists %d, entries %d" % (name, W, H, tile, builds, lists, entries))
            assert builds == r.camera_hit_passes() == i + 1 and entries > lists > 0
    finally:
        r.close()


def test_switch_off(monkeypatch):
    monkeypatch.setenv("LT_ENTRY_CUT", "0")
    r = RendererHIP(0)
    try:
        call(r, "wall", 24, 16)
        call(r, "wall", 24, 16, first=4)
        assert r.camera_hit_passes() == 1 and r.entry_cut_counts() == (0, 0, 0)
    finally:
        r.close()
