"""GPU tests (-m gpu) of the camera hits that accumulator keeps from one call to the next (lt_capi.hip: camera_hits_key,
launch_camera_hits): a call with the same scene, camera, image, tile set and math flavour as the one before it launches no
camera-hit pass and renders every square, the head squares included, in frame groups from the stored hits.

Not a bit may change.  Every call is compared word for word with the same call in a fresh context that keeps nothing
(LT_CAMERA_HITS_KEEP=0: every call runs its pass, the head squares walk in the render launches) and, in the portable flavour, with
the CPU oracle's frames folded by its own running mean, as tests/test_gpu_leaf2_shared.py does.  lt_hip_camera_hit_passes counts the
passes a context has launched: the tests hold it to the number of distinct keys the calls had.

Shapes: 24x16 (even in both dimensions: the centre row and the centre column give 4 head squares of 6), 17x9 (a one-column
square) and 9x9 (a one-pixel square); 2, 3 and 5 frames from frame 1 and from frame 4; synth.heightfield_wall(24) and the Cornell
golden scene.  The camera has no field of view of its own (the aperture is fixed, lt_capi.hip: frame_params); the bytes of its
pitch and roll, which no ray reads but which are part of what the hits are kept for, stand in for it."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import RendererHIP, make_desc, make_rays
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
SIZES = ((24, 16), (17, 9), (9, 9))
COUNTS = (2, 3, 5)
FIRSTS = (1, 4)
ACC = C.PROGRAM_ACCUMULATOR

_scenes = {}
_fresh = {}     # the reference renders, made once and shared: (scene, call) -> pixels
_oracle = {}    # the oracle's frames: (scene, W, H, camera, frame) -> pixels


def scene(name):
    if name not in _scenes:
        if name == "wall":
            _scenes[name] = synth.heightfield_wall(24).validate()
        elif name == "cornell":
            _scenes[name] = sc.load_ltsb(os.path.join(ROOT, "tests", "golden", "cornell_box_O0.ltsb")).validate()
        elif name == "wall-edited":   # the wall with other normals on its first primitives: same nodes, an edit through lt_hip_set_scene
            w = scene("wall")
            prims = np.array(w.prims, dtype=np.uint8, copy=True)
            f = prims.view(np.float32).reshape(-1, 19)
            f[:16, 9:18] = np.float32(0.5)
            _scenes[name] = dataclasses.replace(w, prims=prims).validate()
        else:
            raise KeyError(name)
    return _scenes[name]


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches: the packet walk, frame groups
    monkeypatch.delenv("LT_CAMERA_HITS_KEEP", raising=False)


@pytest.fixture
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def call(r, name, W, H, cam=CAM, first=1, count=3, tile=None, portable=False, strict=False, program=ACC, stats=False):
    """One call through lt_hip_render: `count` frames of a running mean from `first` on (a mean already 3 frames long when it does
    not start at frame 1), over a fixed pattern."""
    r.set_scene(scene(name))
    base = 0 if first == FIRSTS[0] else 3
    d = make_desc(program, W, H, 3, sc.camera_with_frame(cam, first), frame_first=first, frame_count=count, accumulate=True,
                  accumulate_base=base, tile=tile, portable_math=portable, strict_math=strict, stats=stats)
    out = start_pattern(r.output_floats(d))
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def fresh(monkeypatch, name, W, H, **kw):
    """The same call in a context of its own that keeps nothing."""
    key = (name, W, H, tuple(sorted(kw.items())))
    if key not in _fresh:
        monkeypatch.setenv("LT_CAMERA_HITS_KEEP", "0")
        r = RendererHIP(0)
        try:
            _fresh[key] = call(r, name, W, H, **kw)
            assert r.camera_hit_passes() <= 1
        finally:
            r.close()
            monkeypatch.delenv("LT_CAMERA_HITS_KEEP")
    return _fresh[key]


def oracle_fold(name, W, H, cam, first, count):
    acc = start_pattern(W * H * 3).reshape(H, W, 3)
    base = 0 if first == FIRSTS[0] else 3
    for i in range(count):
        k = (name, W, H, bytes(cam[:24]), first + i)
        if k not in _oracle:
            _oracle[k] = po.render(scene(name), sc.camera_with_frame(cam, first + i), W, H, po.ACCUMULATOR)
        po.accumulate(acc, _oracle[k], base + i)
    return acc.reshape(-1)


def assert_same(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), got.size)


def check(monkeypatch, r, name, W, H, what, **kw):
    got = call(r, name, W, H, **kw)
    assert_same(got, fresh(monkeypatch, name, W, H, **kw), "%s %s %dx%d %r vs a fresh context" % (what, name, W, H, kw))
    return got


@pytest.mark.parametrize("portable", [True, False], ids=["portable", "default"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", ["wall", "cornell"])
def test_repeats_launch_one_pass(renderer, monkeypatch, name, size, portable):
    """The same call three times, then with frame_first moved on, for 2, 3 and 5 frames: one pass in all -- the frames are not part
    of what the hits are kept for."""
    W, H = size
    assert renderer.camera_hit_passes() == 0
    for count in COUNTS:
        for first in (FIRSTS[0],) * 3 + FIRSTS[1:]:
            got = check(monkeypatch, renderer, name, W, H, "repeat", first=first, count=count, portable=portable)
            if portable:
                assert_same(got, oracle_fold(name, W, H, CAM, first, count), "%s %dx%d frames %d+%d vs the oracle's frames folded" % (name, W, H, first, count))
            assert renderer.camera_hit_passes() == 1, (count, first)


def test_keep_off_runs_a_pass_per_call(renderer, monkeypatch):
    monkeypatch.setenv("LT_CAMERA_HITS_KEEP", "0")
    for i in range(3):
        call(renderer, "wall", 24, 16)
        assert renderer.camera_hit_passes() == i + 1


def test_head_squares_store_their_hits(monkeypatch):
    """24x16: six squares, four of them head squares, in a context whose buffers are born poisoned.  The second call shades every
    square, the head squares too, from what the first call stored: were a slot of a head square left as allocated, or filled with
    anything but the hit the pass would have found, the call would differ from fresh.  (The hits cannot be read back: the library's
    debug read-back covers the scene's structures only.)  It also equals a call whose pass is forced over all squares -- the natural
    hand-out order has no head -- in a context of its own."""
    W, H = 24, 16
    monkeypatch.setenv("LT_DEBUG_POISON", "0xab")
    r = RendererHIP(0)
    try:
        check(monkeypatch, r, "wall", W, H, "first call")
        second = {first: check(monkeypatch, r, "wall", W, H, "second call", first=first, count=5) for first in FIRSTS}
        assert r.camera_hit_passes() == 1
    finally:
        r.close()
    monkeypatch.delenv("LT_DEBUG_POISON")
    monkeypatch.setenv("LT_NATURAL_ORDER", "1")
    monkeypatch.setenv("LT_CAMERA_HITS_KEEP", "0")
    r = RendererHIP(0)
    try:
        for first in FIRSTS:
            assert_same(second[first], call(r, "wall", W, H, first=first, count=5), "vs a pass over all squares, frames from %d" % first)
        assert r.camera_hit_passes() == len(FIRSTS)
    finally:
        r.close()


MOVED = sc.camera_bytes(1.5, 3.0, -45.0, 0.0, 0.0, 0.0, 1)
ROTATED = sc.camera_bytes(0.0, 2.5, -50.0, 0.3, 0.0, 0.0, 1)
PITCHED = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.25, -0.125, 1)
INVALIDATIONS = {
    "camera-position": (dict(), dict(cam=MOVED)),
    "camera-rotation": (dict(), dict(cam=ROTATED)),
    "camera-pitch-roll-bytes": (dict(), dict(cam=PITCHED)),
    "width": (dict(), dict(W=32)),
    "height": (dict(), dict(H=24)),
    # (8-pixel tiles of 24x16: tiles 1, 3, 4 and 5 are head squares; every call here keeps a square for the pass: tiles 0, 2, 0)
    "tile-first": (dict(tile=(8, 8, 0, 3)), dict(tile=(8, 8, 2, 3))),
    "tile-stride": (dict(tile=(8, 8, 0, 2)), dict(tile=(8, 8, 0, 3))),
    "portable-math": (dict(), dict(portable=True)),
    "strict-math": (dict(), dict(strict=True)),
    "another-scene": (dict(), dict(name="cornell")),
    "edited-primitives": (dict(), dict(name="wall-edited")),
    "larger-image-between": (dict(), dict(W=64, H=48)),
}


@pytest.mark.parametrize("case", sorted(INVALIDATIONS))
def test_a_changed_input_forces_a_new_pass(renderer, monkeypatch, case):
    """The call, the call with one input changed, the call again: three passes, each equal to fresh; then the last one once more
    with frame_first moved on: no fourth."""
    base, changed = INVALIDATIONS[case]
    a = dict(dict(name="wall", W=24, H=16), **base)
    b = dict(a, **changed)
    for i, kw in enumerate((a, b, a)):
        kw = dict(kw)
        check(monkeypatch, renderer, kw.pop("name"), kw.pop("W"), kw.pop("H"), case, **kw)
        assert renderer.camera_hit_passes() == i + 1, (case, i)
    kw = dict(a)
    check(monkeypatch, renderer, kw.pop("name"), kw.pop("W"), kw.pop("H"), case, first=4, **kw)
    assert renderer.camera_hit_passes() == 3


def test_the_identical_scene_forces_no_new_pass(renderer, monkeypatch):
    check(monkeypatch, renderer, "wall", 24, 16, "before")
    w = scene("wall")
    twin = dataclasses.replace(w, nodes=w.nodes.copy(), prims=w.prims.copy(), materials=w.materials.copy(), lights=w.lights.copy())
    _scenes["wall-twin"] = twin
    got = call(renderer, "wall-twin", 24, 16, first=4)
    assert_same(got, fresh(monkeypatch, "wall", 24, 16, first=4), "the same bytes in other buffers")
    assert renderer.camera_hit_passes() == 1
    assert renderer.stats()["scene_reused"] >= 1


def test_bystanders_neither_use_nor_disturb_the_hits(renderer, monkeypatch):
    W, H = 24, 16
    check(monkeypatch, renderer, "wall", W, H, "before")
    call(renderer, "wall", W, H, stats=True)                                    # the counting kernels
    call(renderer, "wall", W, H, count=1)                                       # one frame: the walk stays in the launch
    call(renderer, "wall", W, H, program=C.PROGRAM_BASIC)
    rays = make_rays(np.array([[0.0, 2.5, -50.0]] * 70, dtype=np.float32), np.array([[0.0, 0.0, 1.0]] * 70, dtype=np.float32))
    renderer.trace_rays(rays)
    call(renderer, "wall", W, H, program=C.PROGRAM_GLOBAL_ILLUMINATION, count=2)
    assert renderer.camera_hit_passes() == 1
    check(monkeypatch, renderer, "wall", W, H, "after", first=4, count=5)
    assert renderer.camera_hit_passes() == 1
    monkeypatch.setenv("LT_CAMERA_HITS", "0")                                   # every launch walks its camera rays
    check(monkeypatch, renderer, "wall", W, H, "LT_CAMERA_HITS=0")
    monkeypatch.setenv("LT_CAMERA_HITS", "1")
    monkeypatch.setenv("LT_PERSISTENT", "0")                                    # one square per workgroup
    check(monkeypatch, renderer, "wall", W, H, "LT_PERSISTENT=0")
    monkeypatch.delenv("LT_PERSISTENT")
    check(monkeypatch, renderer, "wall", W, H, "after the switches", first=4)
    assert renderer.camera_hit_passes() == 1


def test_poisoned_buffers(monkeypatch):
    monkeypatch.setenv("LT_DEBUG_POISON", "0xff")
    r = RendererHIP(0)
    monkeypatch.delenv("LT_DEBUG_POISON")   # (read when the context is created; the fresh contexts are not poisoned)
    try:
        for name in ("wall", "cornell"):
            for W, H in SIZES:
                for first in (1, 1, 4):
                    check(monkeypatch, r, name, W, H, "poisoned", first=first)
    finally:
        r.close()


def test_two_contexts_do_not_share_hits(monkeypatch):
    a, b = RendererHIP(0), RendererHIP(0)
    try:
        check(monkeypatch, a, "wall", 24, 16, "context a")
        check(monkeypatch, b, "wall", 24, 16, "context b", cam=MOVED)
        check(monkeypatch, a, "wall", 24, 16, "context a again", first=4)
        check(monkeypatch, b, "wall", 24, 16, "context b again", cam=MOVED, first=4)
        assert a.camera_hit_passes() == 1 and b.camera_hit_passes() == 1
    finally:
        a.close()
        b.close()


def test_two_streams(renderer, monkeypatch):
    """Call A on stream 1, the same call B on stream 2, call C with another camera on stream 1, no host synchronisation between
    them: B reuses the hits A's pass is still writing, C overwrites the hits B is still reading.  512x512, so that the launches
    are long enough to overlap if nothing orders them."""
    import torch
    W = H = 512
    dev = torch.device("cuda", 0)
    renderer.set_scene(scene("wall"))
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    outs = [torch.zeros(W * H * 3, dtype=torch.float32, device=dev) for _ in range(3)]
    torch.cuda.synchronize(dev)
    calls = ((CAM, s1), (CAM, s2), (MOVED, s1))
    for (cam, s), out in zip(calls, outs):
        d = make_desc(ACC, W, H, 3, sc.camera_with_frame(cam, 1), frame_first=1, frame_count=3, accumulate=True)
        renderer.render_device(d, out.data_ptr(), out.numel() * 4, s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert renderer.camera_hit_passes() == 2
    for (cam, s), out, what in zip(calls, outs, "ABC"):
        monkeypatch.setenv("LT_CAMERA_HITS_KEEP", "0")
        f = RendererHIP(0)
        try:
            f.set_scene(scene("wall"))
            d = make_desc(ACC, W, H, 3, sc.camera_with_frame(cam, 1), frame_first=1, frame_count=3, accumulate=True)
            want = np.zeros(W * H * 3, dtype=np.float32)
            f._check(f._L.lt_hip_render(f._ctx, ctypes.byref(d), want.ctypes.data_as(ctypes.c_void_p), want.nbytes))
        finally:
            f.close()
            monkeypatch.delenv("LT_CAMERA_HITS_KEEP")
        assert_same(out.cpu().numpy(), want, "call %s" % what)
