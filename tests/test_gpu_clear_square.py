"""A clear square's two-frame groups rendered in one pass over the square (lt_kernel.hpp: render_clear_square; lt_device.hpp:
shadow_frames_walk_together): the per-pixel set-up once, two new randoms per group, the running mean in registers.

Not a word may change.  tests/test_gpu_clear_items.py's method: LT_SHADOW_PACKETS=1 and LT_CLEAR_ITEMS=1 pinned, every buffer of the
context under test poisoned, every call compared word for word with the same call in fresh contexts under LT_CLEAR_SQUARE=0 (the
per-group path), LT_CLEAR_ITEMS=0 (no item table) and LT_PERSISTENT=0 (one square per workgroup).

The counters (RendererHIP.clear_square_counts: squares that entered the pass, squares that left it before their last group, groups
rendered in it) say that the pass ran: in a call of n frames a square that stays renders n // 2 groups and, where n is odd, leaves
for its last one-frame group; a square that leaves earlier renders fewer.  The general path keeps no count of its own of the groups
it renders for such squares, so "groups in the pass + groups of the general path = squares * groups" cannot be checked as a sum:
what is checked are the bounds that follow from it -- squares entered = the table's whole squares, stayed * (n // 2) <= groups <=
stayed * (n // 2) + left * (n // 2 - 1), at least one group missing per square that left -- and the pixels, which show that the
missing groups were rendered.  Under LT_CLEAR_SQUARE=0 all three are zero."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, make_desc
from tests import entry_cut_scenes as ecs
from tests.entry_cut_leaf_scenes import SCENES, scene

pytestmark = pytest.mark.gpu

ACC = C.PROGRAM_ACCUMULATOR
POISON = "0xa5"
BASELINES = (("LT_CLEAR_SQUARE", "0", "every group through the per-group path"), ("LT_CLEAR_ITEMS", "0", "no item table"),
             ("LT_PERSISTENT", "0", "one square per workgroup"))
COUNTS = (16, 5, 3, 2, 1)
SIZES = ((24, 16), (17, 9), (9, 9))
# A light over the floor whose long side spans the lower squares in z and whose rim in x lies just inside the lower right square of
# 24x16 (its camera hits start at x = 1.596): that square's rays are mixed in z in every frame pair and in x only where a sample of
# its leftmost lanes falls beyond them -- by the oracle's random(), from frame 1 not in the pair (1, 2) but in (3, 4): the square
# leaves at group 1.  The squares in the middle see the light on both sides along both axes at once: they leave at group 0.
RIM_LIGHT = (1.2, 1.66, 13.0, -8.0, 2.0)

_fresh = {}
_scenes = {}


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")
    monkeypatch.setenv("LT_CLEAR_ITEMS", "1")
    for name in ("LT_CLEAR_SQUARE", "LT_PERSISTENT", "LT_ENTRY_CUT", "LT_ENTRY_CUT_LEAVES", "LT_DEBUG_POISON", "LT_FUSED_BYTES", "LT_FUSED_FRAMES",
                 "LT_DEBUG_SHADOW_FRAMES", "LT_SHADOW_FRAMES"):
        monkeypatch.delenv(name, raising=False)


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def get_scene(name):
    if name == "rim-light":
        if name not in _scenes:
            _scenes[name] = (ecs._flat_scene([RIM_LIGHT]), ecs.ps.CAM)
        return _scenes[name]
    return scene(name)


def call(r, name, W, H, first=1, count=3, depth=3, tile=None, device=False, math=None):
    s, cam = get_scene(name)
    r.set_scene(s)
    base = 0 if first == 1 else first - 1
    d = make_desc(ACC, W, H, depth, sc.camera_with_frame(cam, first), frame_first=first, frame_count=count, accumulate=True, accumulate_base=base, tile=tile,
                  **({math + "_math": True} if math else {}))
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
    key = (switch, os.environ["LT_SHADOW_PACKETS"], name, W, H, tuple(sorted(kw.items())))      # (the pinned walk: a baseline is walked as the call is)
    if key not in _fresh:
        monkeypatch.setenv(switch, value)
        r = RendererHIP(0)
        try:
            _fresh[key] = call(r, name, W, H, **kw)
            c = r.clear_square_counts()
            assert c == {"entered": 0, "left": 0, "groups": 0}, "%s=%s renders no square in one pass: %r" % (switch, value, c)
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


def check_counts(r, what, frames):
    """After a call of `frames` frames in one launch: every whole square of the table entered the pass (their cuts' word 0 is the clear
    mark the table was made from); one that stayed rendered frames // 2 groups, one that left fewer; an odd count makes every square
    leave.  Returns (counters, groups that squares which left early rendered inside the pass: -1 where the count is odd and the
    two kinds of leaving cannot be told apart)."""
    c = r.clear_square_counts()
    items = r.clear_item_counts()
    full, groups = frames // 2, (frames + 1) // 2
    print("%s: %d frames: %r; table %r" % (what, frames, c, items))
    if not items["used"] or frames < 2:
        assert c == {"entered": 0, "left": 0, "groups": 0}
        return c, 0
    assert c["entered"] == items["whole"]
    assert c["left"] <= c["entered"] and c["groups"] <= c["entered"] * full
    # (what the general path must have rendered is the remainder, not a count of its own: at least one group per square that left)
    assert c["entered"] * groups - c["groups"] >= c["left"]
    if frames % 2:
        assert c["left"] == c["entered"]
        return c, -1
    stayed = c["entered"] - c["left"]
    assert c["groups"] >= stayed * full and c["groups"] <= stayed * full + c["left"] * (full - 1)
    return c, c["groups"] - stayed * full


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", SCENES)
def test_same_words_as_the_per_group_path(monkeypatch, name, size):
    """The leaf-pass scenes: 16, 5, 3, 2 and 1 frames; a first call, two reusing calls (base 0: the first frame overwrites), one from
    frame 4 (base 3).  24x16 folds; 17x9 and 9x9 hand squares out whole that store their samples."""
    W, H = size
    r = poisoned(monkeypatch)
    try:
        for n, count in enumerate(COUNTS):
            for i, first in enumerate((1, 1, 1, 4)):
                check(monkeypatch, r, name, W, H, "call %d" % i, first=first, count=count)
                reusing = n > 0 or i >= 1      # (the context's very first call runs its own camera-hit pass: no cuts, no table)
                c, _ = check_counts(r, "%s %dx%d call %d" % (name, W, H, i), count if reusing else 0)
                if name in ("wall", "fine-field") and reusing and count >= 2:      # (the scenes known to have clear squares)
                    assert c["entered"] > 0 and (c["groups"] > 0 or count // 2 == 0 or c["left"] == c["entered"])
                    if name == "fine-field":
                        assert c["groups"] > 0
    finally:
        r.close()


@pytest.mark.parametrize("name", ["far-occluder", "wall"])
def test_chunks_of_unequal_length_and_device_output(monkeypatch, name):
    """16, 5 and 3 frames in launches of at most 5, 3 and 2 (LT_FUSED_BYTES): launches of another number of groups, a last launch of
    one frame; through lt_hip_render and lt_hip_render_device."""
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
            c, _ = check_counts(r, "%s device=%r" % (name, device), 16)
            if name == "wall":      # (one of its six squares is clear; the far occluder's image has none at this size)
                assert c["entered"] > 0 and c["groups"] > 0
    finally:
        r.close()


@pytest.mark.parametrize("name", ["far-occluder", "fine-field"])
def test_tiled_desc(monkeypatch, name):
    """64x64 tiles, every second one: 128x128 (folds) and 136x72 (padded tiles: whole squares that store)."""
    for W, H in ((128, 128), (136, 72)):
        tile = (64, 64, 0, 2)
        r = poisoned(monkeypatch)
        try:
            for first, count in ((1, 5), (1, 5), (4, 16), (4, 3)):
                check(monkeypatch, r, name, W, H, "tiled", first=first, count=count, tile=tile)
            c, _ = check_counts(r, "%s %dx%d tiled" % (name, W, H), 3)
            assert c["entered"] > 0 and c["groups"] > 0
        finally:
            r.close()


@pytest.mark.parametrize("name", ["far-occluder", "wall"])
def test_depth_four(monkeypatch, name):
    """Depth 4: no fold, the fourth channel stays the caller's."""
    W, H = 24, 16
    r = poisoned(monkeypatch)
    try:
        for first, count in ((1, 5), (1, 5), (4, 16)):
            check(monkeypatch, r, name, W, H, "depth 4", first=first, count=count, depth=4)
        c, _ = check_counts(r, "%s depth 4" % name, 16)
        if name == "wall":
            assert c["entered"] > 0 and c["groups"] > 0
    finally:
        r.close()


@pytest.mark.parametrize("name", ["fine-field", "far-occluder"])
def test_walk_two(monkeypatch, name):
    """LT_SHADOW_PACKETS=2: the spread test is part of what decides whether a group's frames walk together."""
    W, H = 24, 16
    monkeypatch.setenv("LT_SHADOW_PACKETS", "2")
    r = poisoned(monkeypatch)
    try:
        for first, count in ((1, 5), (1, 16), (4, 16)):
            check(monkeypatch, r, name, W, H, "walk 2", first=first, count=count)
        c, _ = check_counts(r, "%s walk 2" % name, 16)
        if name == "fine-field":      # (its clear square's rays are spread too far for walk 2's test: it leaves at group 0)
            assert c["entered"] > 0
    finally:
        r.close()


@pytest.mark.parametrize("math", ["portable", "strict"])
@pytest.mark.parametrize("name", ["fine-field", "far-occluder"])
def test_other_math_flavours(monkeypatch, name, math):
    """The other math flavours, each a kernel of its own (the default one is every other case's)."""
    W, H = 24, 16
    r = poisoned(monkeypatch)
    try:
        for first, count in ((1, 5), (1, 16), (4, 5)):
            check(monkeypatch, r, name, W, H, math + " math", first=first, count=count, math=math)
        c, _ = check_counts(r, "%s %s" % (name, math), 5)
        if name == "fine-field":
            assert c["entered"] > 0 and c["groups"] > 0
    finally:
        r.close()


def test_squares_that_leave_early(monkeypatch):
    """Groups with two mixed axes render apart: the light that straddles the floor, the two-axes scene, and a light whose rim lies
    inside a square (RIM_LIGHT).  Some squares leave the pass early and some stay; across these scenes one leaves at group 0 (a call of one group in which a
    square leaves) and one at a later group (a call of 8 groups in which the squares that left rendered some group inside)."""
    W, H = 24, 16
    at_zero = later = some_left = some_stayed = 0
    for name in ("penumbra-24x16", "two-axes", "wide-light-bare", "rim-light"):
        r = poisoned(monkeypatch)
        try:
            check(monkeypatch, r, name, W, H, "first call", first=1, count=2)
            for first, count in ((1, 2), (3, 2), (1, 16), (5, 16), (4, 5), (9, 6)):
                check(monkeypatch, r, name, W, H, "leaving early", first=first, count=count)
                c, inside = check_counts(r, "%s from %d" % (name, first), count)
                some_left += c["left"] if count % 2 == 0 else 0
                some_stayed += c["entered"] - c["left"]
                if count == 2:
                    at_zero += c["left"]
                elif inside > 0:
                    later += 1
        finally:
            r.close()
    assert some_left > 0 and some_stayed > 0, "squares that left early: %d, that stayed: %d" % (some_left, some_stayed)
    assert at_zero > 0, "no square left the pass at group 0"
    assert later > 0, "no square left the pass at a later group"
