"""GPU tests (-m gpu) of the two-frame shadow walk where its frames' rays part: a penumbra (tests/penumbra_scenes.py).  Frame 1's
rays are asked about a child of an interior record only where frame 0's rays all miss it (lt_walk_asm.hpp: LT_ASM_TESTS2); a child
skipped wrongly would leave a shadowed pixel lit.  Every call is compared bit for bit with LT_SHADOW_FRAMES=1 (a work item per frame,
each frame's own walk) and with the CPU oracle's accumulated frames, and must have walked groups together.  The small images end in
squares of one column and of a single pixel: the walk runs with lanes off (its stack register parked), and one frame's `open` mask
empties while the other frame still looks."""
import ctypes
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP
from oracle import pyoracle as po
from tests import penumbra_scenes as ps
from tests.conftest import oracle_desc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    return {name: ps.case_scene(name) for name in ps.CASES}


@pytest.fixture(scope="module")
def oracle_frames(scenes):
    """name -> {frame: the oracle's image}, every frame a case's calls cover, rendered once."""
    out = {}
    for name, c in ps.CASES.items():
        frames = range(min(c["firsts"]), max(c["firsts"]) + max(ps.COUNTS))
        out[name] = {f: po.render(scenes[name], sc.camera_with_frame(ps.CAM, f), c["W"], c["H"], po.ACCUMULATOR) for f in frames}
    return out


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")
    monkeypatch.setenv("LT_DEBUG_SHADOW_FRAMES", "1")


def render(r, scene, W, H, first, count):
    r.set_scene(scene)
    d = oracle_desc(C.PROGRAM_ACCUMULATOR, W, H, 3, ps.CAM, frame_first=first, frame_count=count, accumulate=True)
    out = np.full(r.output_floats(d), np.nan, dtype=np.float32)
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out.reshape(H, W, 3)


def launches(capfd):
    """(frames per work item, waves that walked both frames together, apart) of every render launch since the last look."""
    got = re.findall(r"shadow-ray frame groups: (\d+) \(walk \d+, \d+ frames\)(?:: (\d+) waves walked both frames together, (\d+) apart)?",
                     capfd.readouterr().err)
    return [(int(g), int(t or 0), int(a or 0)) for g, t, a in got]


@pytest.mark.parametrize("count", ps.COUNTS)
@pytest.mark.parametrize("name,first", [(n, f) for n in sorted(ps.CASES) for f in ps.CASES[n]["firsts"]])
def test_penumbra(renderer, scenes, oracle_frames, monkeypatch, capfd, name, first, count):
    c = ps.CASES[name]
    W, H = c["W"], c["H"]
    launches(capfd)
    grouped = render(renderer, scenes[name], W, H, first, count)
    got = launches(capfd)
    assert len(got) == 1 and got[0][0] == 2 and got[0][1] > 0, got       # groups of two frames, some walked together
    monkeypatch.setenv("LT_SHADOW_FRAMES", "1")
    alone = render(renderer, scenes[name], W, H, first, count)
    got = launches(capfd)
    assert len(got) == 1 and got[0][0] == 1, got
    assert np.array_equal(grouped, alone), int((grouped != alone).sum())
    acc = np.zeros((H, W, 3), dtype=np.float32)
    for i in range(count):
        po.accumulate(acc, oracle_frames[name][first + i], i)
    assert np.array_equal(grouped, acc), int((grouped != acc).sum())
