"""Persistent wavefronts take two indices per claim from a queue that holds more than four items per wave of the launch
(lt_kernel.hpp: kClaimPair, render_kernel_body).  Every item must still be rendered exactly once: an item that nobody renders
leaves what its buffer held, and an index past the end must not be rendered at all.

Not a word may change.  Every call is compared word for word with the same call in a fresh context with LT_PERSISTENT=0: one
square per workgroup, no queue and no claim.  The image is the smallest whose queues reach that length with a few frames on an
MI355X (8192 wave slots, so 32 768 items): 2056 x 2056 pixels are 257 x 257 = 66 049 squares, eight shares of 8257 (one) and 8256
(seven).  Nine frames in frame groups make 5 items per square: queues of 41 285 and 41 280, an odd and an even one in every
launch, so a pair that begins at the last index occurs in one of them; the camera-hit pass in front of them is a persistent launch
of its own with short queues, and the second call of a context renders from kept hits, entry cuts and clear marks.  One-frame
calls have short queues too: one index per claim, the same loop.  The Cornell box from close by, so that four fifths of the image
are lit and a lost square shows; every buffer poisoned, so that it shows whatever its colour.  A few milliseconds per call.
"""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, make_desc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 2056
SQUARES = ((W + 7) // 8) * ((H + 7) // 8)
CAMERA = sc.camera_bytes(0.0, 2.5, -20.0, 0.0, 0.0, 0.0, 1)   # close enough that the box fills the image: four fifths of it are lit

_scene = []
_baseline = {}


def cornell():
    if not _scene:
        _scene.append(sc.load_ltsb(os.path.join(ROOT, "tests", "golden", "cornell_box_O0.ltsb")).validate())
    return _scene[0]


def start_pattern(n):
    return (np.arange(n, dtype=np.float32) % 7.0) / 7.0


def call(r, program, first, count, base):
    d = make_desc(program, W, H, 3, sc.camera_with_frame(CAMERA, first), frame_first=first, frame_count=count, accumulate=True, accumulate_base=base)
    out = start_pattern(r.output_floats(d))
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def calls(monkeypatch, program, walk, sequence, persistent):
    """The calls of `sequence` = ((first, count, base), ...) on one fresh context: their images."""
    key = (program, walk, sequence, persistent)
    if persistent or key not in _baseline:
        monkeypatch.setenv("LT_SHADOW_PACKETS", str(walk))   # a forced walk: no timing launches
        # every buffer of the context starts as 0x5a bytes (1.5e16 as floats): what an item that nobody renders leaves behind is then
        # no colour of the scene -- fresh device memory is zeros, and half of this image is black
        monkeypatch.setenv("LT_DEBUG_POISON", "0x5a")
        if persistent:
            monkeypatch.delenv("LT_PERSISTENT", raising=False)
        else:
            monkeypatch.setenv("LT_PERSISTENT", "0")
        r = RendererHIP(0)
        try:
            r.set_scene(cornell())
            images = [call(r, program, *c) for c in sequence]
        finally:
            r.close()
            monkeypatch.delenv("LT_PERSISTENT", raising=False)
            monkeypatch.delenv("LT_DEBUG_POISON")
        if persistent:
            return images
        _baseline[key] = images
    return _baseline[key]


def test_the_queues_are_long_enough_to_be_claimed_in_pairs():
    import torch
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 32
    assert 4 * (SQUARES // 8) // 4 > waves, "a queue of four or more items per square must hold more than four items per wave of the launch (%d waves): else no claim takes a pair" % waves
    assert sorted({SQUARES // 8, (SQUARES + 7) // 8}) == [8256, 8257], "an odd and an even queue"


@pytest.mark.parametrize("program,walk,sequence", [
    (C.PROGRAM_ACCUMULATOR, 1, ((1, 1, 0),)),                  # one frame: a short queue, one index per claim
    (C.PROGRAM_ACCUMULATOR, 1, ((1, 9, 0), (10, 9, 3))),       # the camera-hit pass and 5 frame groups per square: odd and even queues; then kept hits, cuts, clear marks
    (C.PROGRAM_ACCUMULATOR, 1, ((1, 2, 0), (3, 16, 2))),       # 8 frame groups: a pair is two frame groups of one square
    (C.PROGRAM_ACCUMULATOR, 3, ((1, 5, 0),)),                  # queued shadow rays: an item per frame, slots mapped by item
    (C.PROGRAM_BASIC, 0, ((1, 5, 0),)),                        # another program's kernel through the same hand-out
], ids=["one-frame", "nine-frames-twice", "two-then-sixteen", "queued", "basic"])
def test_same_words_as_one_square_per_workgroup(monkeypatch, program, walk, sequence):
    got = calls(monkeypatch, program, walk, sequence, True)
    want = calls(monkeypatch, program, walk, sequence, False)
    for i, (g, w) in enumerate(zip(got, want)):
        differ = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        assert differ.size == 0, "call %d %r: %d words differ from LT_PERSISTENT=0, the first at float %d (pixel %d, %d): %r against %r" % (
            i, sequence[i], differ.size, differ[0], differ[0] // 3 % W, differ[0] // 3 // W, g[differ[0]], w[differ[0]])
