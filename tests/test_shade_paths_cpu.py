"""CPU: the shaded-path interface (lt_hip_shade_paths) as far as it goes without a GPU, and the fixtures of the GPU tests
(tests/shade_paths.py) held against the CPU oracle.

* the library exports both entry points, the descriptor has the header's 32 bytes and fields, a null context is refused,
  RendererHIP.shade_paths rejects a wrongly shaped array before it calls the library;
* the fixtures hold what the GPU tests lean on, by the oracle's per-pixel counters of the single-sample program at 16 bounces
  (extension rays of a pixel = rays - shadow rays - 1), for every camera of tests/shade_rays.py at both sizes: at least 10 % of
  the rays trace 3 extension rays or more, at least 3 % trace 8 or more, some ray traces all 16, and at least 10 % of the pixels
  exceed 1 in tile mode (the clamp is exercised); 25 % of the ring's rays trace 3 or more.  (Measured: the worst of the twelve
  cases has 15 %, 4.5 % and 15.6 %; the ring 38 %.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import renderer as R
from oracle import pyoracle as po
from tests import shade_paths as P
from tests import shade_rays as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_entry_points_and_the_descriptor_has_the_headers_size():
    L = C.load()
    assert hasattr(L, "lt_hip_shade_paths") and hasattr(L, "lt_hip_shade_paths_device")
    assert "lt_hip_shade_paths" in C.EXPORTS and "lt_hip_shade_paths_device" in C.EXPORTS
    assert ctypes.sizeof(C.PathsDesc) == 32
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    for name in ("lt_hip_paths_desc", "lt_hip_shade_paths", "lt_hip_shade_paths_device"):
        assert re.search(r"\b%s\b" % name, header), name
    fields = re.search(r"typedef struct lt_hip_paths_desc \{(.*?)\} lt_hip_paths_desc;", header, re.S).group(1)
    assert re.findall(r"(?:uint32_t|int32_t) (\w+);", fields) == [n for n, _ in C.PathsDesc._fields_]
    assert L.lt_hip_abi_version() == 4


def test_a_null_context_is_an_invalid_argument():
    L = C.load()
    d = C.PathsDesc(ctypes.sizeof(C.PathsDesc), C.PROGRAM_GLOBAL_ILLUMINATION, C.KERNEL_MODE_LINEAR, 0, 0, 1, 0, 0)
    rays = R.make_shade_rays(np.zeros((2, 3)), np.ones((2, 3)), 0.0, 0.0)
    out = np.full(8, 0x5a5a5a5a, dtype=np.uint32)
    assert L.lt_hip_shade_paths(None, ctypes.byref(d), rays.ctypes.data_as(ctypes.c_void_p), 2, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_shade_paths_device(None, ctypes.byref(d), None, 0, None, 0, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (out == 0x5a5a5a5a).all()


def test_shade_paths_rejects_a_wrongly_shaped_array():
    r = R.RendererHIP.__new__(R.RendererHIP)   # (no context: the shape is checked before the library is called)
    for bad in (np.zeros((4, 7), dtype=np.float32), np.zeros((4, 8), dtype=np.float64), np.zeros(8, dtype=np.float32), np.zeros((2, 4, 8), dtype=np.float32)):
        with pytest.raises(ValueError):
            R.RendererHIP.shade_paths(r, bad, program=C.PROGRAM_GLOBAL_ILLUMINATION)
    with pytest.raises(TypeError):
        R.RendererHIP.shade_paths(r, [[0.0] * 8], program=C.PROGRAM_GLOBAL_ILLUMINATION)


@pytest.mark.parametrize("W,H", F.SIZES)
@pytest.mark.parametrize("yaw,dist", F.CAMERAS)
def test_every_cameras_batch_holds_long_paths_and_pixels_the_clamp_changes(yaw, dist, W, H):
    ext = P.extension_rays(yaw, dist, W, H)
    n = len(ext)
    assert n == W * H and ext.min() >= 0 and ext.max() <= 16
    assert 10 * (ext >= 3).sum() >= n, (ext >= 3).mean()
    assert 100 * (ext >= 8).sum() >= 3 * n, (ext >= 8).mean()
    assert (ext == 16).any()
    tile = P.oracle_image(yaw, dist, W, H, "global_illumination", po.MODE_TILE, 0, 0).reshape(-1, 3)
    assert 10 * (tile > 1.0).any(axis=1).sum() >= n, (tile > 1.0).any(axis=1).mean()
    lin = P.oracle_image(yaw, dist, W, H, "global_illumination", po.MODE_LINEAR, 0, 0).reshape(-1, 3)
    assert np.array_equal(lin, np.clip(tile, 0.0, 1.0)) and lin.max() == 1.0


def test_a_quarter_of_the_rings_rays_trace_three_extension_rays_or_more():
    W, H = F.RING_SIZE
    _, cam, pix = F.ring_batch()
    ext = np.stack([P.extension_rays(yaw, dist, W, H) for yaw, dist in F.RING])[cam, pix]
    assert 4 * (ext >= 3).sum() >= len(ext), (ext >= 3).mean()
