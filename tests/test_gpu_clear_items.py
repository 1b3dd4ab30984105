"""Clear squares handed out whole from the item table, their samples folded by their own wave (lt_entry_cut.hpp: kItemWhole,
fold_segment; lt_clear_items_kernel; render_kernel_body; render_square's fold; lt_running_mean4_kernel's map).

Not a word may change.  Every call is compared word for word with the same call in a fresh context under LT_CLEAR_ITEMS=0 (the
hand-out and the fold without a table) and in one under LT_PERSISTENT=0 (one square per workgroup: no queue, no table).  Every
buffer of the context under test is poisoned: a folded square's sample words are never written, and a fold that read them, or a
square that nobody rendered, shows.

Cases: the scenes of tests/entry_cut_leaf_scenes.py at 24x16 (folds), 9x9 and 17x9 (a width that is no multiple of 8: whole squares,
no fold), each with 16, 5, 3, 2 and 1 frames from frame 1 (base 0) and from frame 4 (base 3); a first call, a reusing call, a second reusing
call; launches cut into chunks (LT_FUSED_BYTES); an edit of lights and one of primitives between reusing calls; a tiled desc
(64x64 tiles, stride 2); depth 4 (channel 3 stays the caller's, no fold); lt_hip_render_device beside lt_hip_render (whose last
fold comes in pieces only for large images: the Cornell case); the Cornell box from close by at a size whose table queues pass
the length from which a queue is claimed in pairs.  The counters (RendererHIP.clear_item_counts) are printed and asserted per case."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, make_desc
from tests.entry_cut_leaf_scenes import SCENES, scene

pytestmark = pytest.mark.gpu

ACC = C.PROGRAM_ACCUMULATOR
POISON = "0xa5"
BASELINES = (("LT_CLEAR_ITEMS", "0", "no item table"), ("LT_PERSISTENT", "0", "one square per workgroup"))
COUNTS = (16, 5, 3, 2, 1)
SIZES = ((24, 16), (9, 9), (17, 9))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_fresh = {}


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches: the packet walk, frame groups
    # the table however few squares are clear: unset, a context drops it once the build's counters have come back and say that fewer
    # than a third are -- when they come back is the device's timing (test_the_table_is_dropped_where_few_squares_are_clear)
    monkeypatch.setenv("LT_CLEAR_ITEMS", "1")
    for name in ("LT_PERSISTENT", "LT_ENTRY_CUT", "LT_ENTRY_CUT_LEAVES", "LT_DEBUG_POISON", "LT_FUSED_BYTES", "LT_FUSED_FRAMES"):
        monkeypatch.delenv(name, raising=False)


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def get_scene(name):
    if name == "cornell-close":
        if name not in _fresh:
            _fresh[name] = (sc.load_ltsb(os.path.join(ROOT, "tests", "golden", "cornell_box_O0.ltsb")).validate(),
                            sc.camera_bytes(0.0, 2.5, -20.0, 0.0, 0.0, 0.0, 1))
        return _fresh[name]
    return scene(name)


def call(r, name, W, H, first=1, count=3, base=None, depth=3, tile=None, device=False):
    s, cam = get_scene(name)
    r.set_scene(s)
    base = (0 if first == 1 else first - 1) if base is None else base
    d = make_desc(ACC, W, H, depth, sc.camera_with_frame(cam, first), frame_first=first, frame_count=count, accumulate=True, accumulate_base=base, tile=tile)
    out = start_pattern(r.output_floats(d))
    if device:
        import torch
        t = torch.from_numpy(out).cuda()
        r.render_device(d, t.data_ptr(), out.nbytes)
        r.synchronize()
        return t.cpu().numpy()
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def fresh(monkeypatch, switch, value, name, W, H, **kw):
    """The same call through lt_hip_render in a context of its own with `switch` set to `value`."""
    kw = dict(kw, device=False)
    key = (switch, name, W, H, tuple(sorted(kw.items())))
    if key not in _fresh:
        monkeypatch.setenv(switch, value)
        r = RendererHIP(0)
        try:
            _fresh[key] = call(r, name, W, H, **kw)
            c = r.clear_item_counts()
            assert c["entries"] == c["whole"] == c["folded"] == c["builds"] == 0, "%s=%s builds no table: %r" % (switch, value, c)
        finally:
            r.close()
            monkeypatch.delenv(switch)
            monkeypatch.setenv("LT_CLEAR_ITEMS", "1")
    return _fresh[key]


def poisoned(monkeypatch):
    monkeypatch.setenv("LT_DEBUG_POISON", POISON)      # (read when the context is created)
    r = RendererHIP(0)
    monkeypatch.delenv("LT_DEBUG_POISON")
    return r


def assert_same(got, want, what):
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ.size == 0, "%s: %d of %d words differ, the first at float %d: %r against %r" % (what, differ.size, got.size, differ[0], got[differ[0]], want[differ[0]])


def check(monkeypatch, r, name, W, H, what, **kw):
    got = call(r, name, W, H, **kw)
    for switch, value, means in BASELINES:
        assert_same(got, fresh(monkeypatch, switch, value, name, W, H, **kw),
                    "%s %s %dx%d %r vs a fresh context with %s=%s (%s)" % (what, name, W, H, kw, switch, value, means))
    return got


def squares_of(W, H, tile=None):
    if tile is None:
        return ((W + 7) // 8) * ((H + 7) // 8)
    tw, th, first, stride = tile
    tiles = ((W + tw - 1) // tw) * ((H + th - 1) // th)
    return len(range(first, tiles, stride)) * ((tw + 7) // 8) * ((th + 7) // 8)


def check_counts(r, what, squares, frames, folds):
    """Of the table the context holds after a reusing call of `frames` >= 2 frames: a whole square per clear square, `groups` entries
    per other square; folded by their own wave all of them (folds) or none."""
    c = r.clear_item_counts()
    clear = r.entry_cut_leaf_counts()[0]
    groups = (frames + 1) // 2
    print("%s: %d squares, %d frames: %r; clear squares %d" % (what, squares, frames, c, clear))
    if r.entry_cut_counts()[0] == 0:      # (a scene that gets no cuts -- no own tree, no light -- gets no table)
        assert c["entries"] == c["whole"] == c["folded"] == c["builds"] == 0
        return c
    assert c["whole"] == clear and c["entries"] == clear + (squares - clear) * groups
    assert c["folded"] == (c["whole"] if folds else 0)
    return c


def folds(W, depth=3, tile=None):
    return depth == 3 and (tile[0] if tile else W) % 8 == 0


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", SCENES)
def test_same_words_as_without_the_table(monkeypatch, name, size):
    W, H = size
    r = poisoned(monkeypatch)
    try:
        builds = 0
        for n, count in enumerate(COUNTS):
            for i, first in enumerate((1, 1, 1, 4)):     # a first call, two reusing calls, then a continuation from frame 4 on a mean of 3
                check(monkeypatch, r, name, W, H, "call %d" % i, first=first, count=count)
                reusing = n > 0 or i >= 1      # (the context's very first call runs its own camera-hit pass: no cuts, no table)
                if count >= 2 and reusing:
                    builds += i == (1 if n == 0 else 0)     # (another number of frame groups: the table is built again, once)
                    c = check_counts(r, "%s %dx%d call %d" % (name, W, H, i), squares_of(W, H), count, folds(W))
                    assert c["builds"] == (builds if r.entry_cut_counts()[0] else 0)
                    # the scenes known to have clear squares: some but not all fold at 24x16; none folds at 17x9 and 9x9, yet squares go out whole
                    if name in ("wall", "fine-field"):
                        assert c["used"] and 0 < c["whole"] < squares_of(W, H)
                        assert 0 < c["folded"] < squares_of(W, H) if folds(W) else c["folded"] == 0
        assert r.camera_hit_passes() == 1
    finally:
        r.close()


@pytest.mark.parametrize("name", ["far-occluder", "wall"])
def test_chunked_launches_and_device_output(monkeypatch, name):
    """16 and 5 frames in launches of at most 5 and 3 (LT_FUSED_BYTES): a last launch of one frame (no table), of two (one group);
    through lt_hip_render and lt_hip_render_device."""
    W, H = 24, 16
    r = poisoned(monkeypatch)
    try:
        for device in (False, True):
            call(r, name, W, H, first=1, count=2, device=device)
            for count, per in ((16, 5), (5, 3), (3, 2)):
                for first in (1, 4):
                    monkeypatch.setenv("LT_FUSED_BYTES", str(per * W * H * 3 * 4))      # (read by every render call)
                    got = call(r, name, W, H, first=first, count=count, device=device)
                    monkeypatch.delenv("LT_FUSED_BYTES")
                    for switch, value, means in BASELINES:
                        assert_same(got, fresh(monkeypatch, switch, value, name, W, H, first=first, count=count),
                                    "%s %d frames in launches of %d from %d, device=%r vs %s=%s" % (name, count, per, first, device, switch, value))
            check(monkeypatch, r, name, W, H, "whole launch, device=%r" % device, first=4, count=16, device=device)
            check_counts(r, "%s device=%r" % (name, device), squares_of(W, H), 16, True)
    finally:
        r.close()


@pytest.mark.parametrize("edited", ["wall-edited-prims", "wall-edited-lights"])
def test_an_edit_rebuilds_the_table(monkeypatch, edited):
    """The wall, the wall with primitives or lights edited (lt_hip_set_scene's edit path), the wall again, each rendered three times:
    the table is built behind the cuts of the call that reuses the hits, once per scene, and every image is a fresh context's."""
    W, H = 24, 16
    r = poisoned(monkeypatch)
    try:
        seen = []
        for i, name in enumerate(("wall", edited, "wall")):
            check(monkeypatch, r, name, W, H, "edit %d" % i, first=1, count=5)
            c = r.clear_item_counts()
            assert c["entries"] == c["whole"] == c["folded"] == 0 and c["builds"] == i      # (a call that runs its own pass: no cuts, no table)
            check(monkeypatch, r, name, W, H, "edit %d, reusing" % i, first=4, count=5)
            check(monkeypatch, r, name, W, H, "edit %d, reusing again" % i, first=9, count=5, base=8)
            c = check_counts(r, "%s after edit %d" % (name, i), squares_of(W, H), 5, True)
            assert c["builds"] == i + 1
            seen.append((c["entries"], c["whole"]))
        assert seen[0] == seen[2]
    finally:
        r.close()


@pytest.mark.parametrize("name", ["far-occluder", "fine-field"])
def test_tiled_desc(monkeypatch, name):
    """64x64 tiles, every second one: two stacked tiles of a 128x128 image (no padded tile: folds), three of a 136x72 image (padded
    tiles: whole squares, no fold)."""
    for W, H, fold in ((128, 128, True), (136, 72, False)):
        tile = (64, 64, 0, 2)
        r = poisoned(monkeypatch)
        try:
            for first, count in ((1, 5), (1, 5), (4, 16), (4, 3)):
                check(monkeypatch, r, name, W, H, "tiled", first=first, count=count, tile=tile)
            c = check_counts(r, "%s %dx%d tiled" % (name, W, H), squares_of(W, H, tile), 3, fold)
            assert c["used"] and 0 < c["whole"] < squares_of(W, H, tile)      # (both scenes have clear squares in both images)
            assert 0 < c["folded"] < squares_of(W, H, tile) if fold else c["folded"] == 0
        finally:
            r.close()


@pytest.mark.parametrize("name", ["far-occluder", "wall"])
def test_depth_four_keeps_the_fourth_channel(monkeypatch, name):
    W, H = 24, 16
    r = poisoned(monkeypatch)
    try:
        for first, count in ((1, 5), (1, 5), (4, 16)):
            check(monkeypatch, r, name, W, H, "depth 4", first=first, count=count, depth=4)
            # (lt_hip_render hands back its staging buffer's fourth channel; the caller's own stays where the image is the caller's)
            got = call(r, name, W, H, first=first, count=count, depth=4, device=True)
            want = fresh(monkeypatch, "LT_CLEAR_ITEMS", "0", name, W, H, first=first, count=count, depth=4)
            for ch in range(3):
                assert_same(got[ch::4], want[ch::4], "depth 4, device output, channel %d" % ch)
            assert np.array_equal(got[3::4], start_pattern(got.size)[3::4])
        c = check_counts(r, "%s depth 4" % name, squares_of(W, H), 16, False)
        if name == "wall":      # (one of its six squares is clear: handed out whole, not folded)
            assert c["used"] and c["whole"] > 0 and c["folded"] == 0
    finally:
        r.close()


CORNELL = 2056      # 257 x 257 squares, 41 531 of them clear
FRAMES = 24         # twelve frame groups: 335 747 entries, 10 492 per queue and four waves of an MI355X


def test_cornell_pairs_over_the_table(monkeypatch):
    """The Cornell box from close by (tests/test_gpu_claim_pairs.py's camera), large enough that the table's queues hold more than four
    entries per wave of the launch -- their mean does, so at least one does: the length from which a queue without a table is
    claimed in pairs (kClaimPair), which the table's bound is taken from; lt_hip_render folds its last launch in the pieces of the
    read-back."""
    import torch
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 32
    r = poisoned(monkeypatch)
    try:
        W = H = CORNELL
        for i, (first, count, base) in enumerate(((1, 2, 0), (3, FRAMES, 2), (3 + FRAMES, FRAMES, 2 + FRAMES))):
            check(monkeypatch, r, "cornell-close", W, H, "call %d" % i, first=first, count=count, base=base)
        c = check_counts(r, "cornell %d" % W, squares_of(W, H), FRAMES, True)
        assert 0 < c["whole"] < squares_of(W, H)
        assert c["entries"] // 8 // 4 > waves, "the table's queues must hold more than four entries per wave (%d waves) on average: %r" % (waves, c)
    finally:
        r.close()


def test_hand_out_alone(monkeypatch):
    """LT_CLEAR_ITEMS=2: whole squares from the table, their samples stored and folded by the fold kernel: the same words."""
    W, H = 24, 16
    monkeypatch.setenv("LT_CLEAR_ITEMS", "2")
    r = poisoned(monkeypatch)
    try:
        for first, count in ((1, 5), (1, 5), (4, 16), (4, 3)):
            monkeypatch.setenv("LT_CLEAR_ITEMS", "2")      # (fresh() leaves it at 1)
            check(monkeypatch, r, "wall", W, H, "hand-out alone", first=first, count=count)
        c = check_counts(r, "wall, hand-out alone", squares_of(W, H), 3, False)
        assert c["used"] and c["whole"] > 0 and c["folded"] == 0
    finally:
        r.close()


def test_the_table_is_dropped_where_few_squares_are_clear(monkeypatch):
    """LT_CLEAR_ITEMS unset.  The wall at 24x16 has one clear square of six, fewer than a third: once the build's counters are back
    -- clear_item_counts waits for the render they travel behind -- a reusing call takes no table and folds nothing.  The fine field
    at 17x9 has five of six: it keeps the table.  The same words in both."""
    for name, W, H, keeps in (("wall", 24, 16, False), ("fine-field", 17, 9, True)):
        r = poisoned(monkeypatch)
        try:
            for i, first in enumerate((1, 4, 9, 14)):
                monkeypatch.delenv("LT_CLEAR_ITEMS", raising=False)      # (fresh() leaves it at 1)
                check(monkeypatch, r, name, W, H, "call %d" % i, first=first, count=5, base=first - 1)
                c = r.clear_item_counts()
                print("%s %dx%d call %d: %r" % (name, W, H, i, c))
                if i == 0:
                    assert not c["used"] and c["builds"] == 0      # (its own camera-hit pass: no cuts)
                if i >= 2:      # (the counters came back before call 2 was enqueued)
                    assert c["used"] == keeps and c["builds"] == 1 and c["whole"] > 0 and c["folded"] == 0
        finally:
            r.close()
