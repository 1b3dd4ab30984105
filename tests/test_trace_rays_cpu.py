"""CPU-side checks of the ray-query ABI (lt_hip_trace_rays / lt_hip_trace_rays_device): the library exports it, the records
have the header's layout, a call without a context is refused, and make_rays packs rays as the kernels read them.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import FLT_MAX, HIT_DTYPE, RAY_DTYPE, make_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()


def test_library_exports_the_query_entry_points():
    L = C.load()
    for name in ("lt_hip_trace_rays", "lt_hip_trace_rays_device"):
        assert name in C.EXPORTS
        assert re.search(r"^int\s+%s\s*\(" % name, HEADER, flags=re.M)
        assert getattr(L, name) is not None
    assert L.lt_hip_abi_version() == 4


def test_record_layouts_and_constants_match_the_header():
    assert ctypes.sizeof(C.TraceRay) == 32 and RAY_DTYPE.itemsize == 32
    assert ctypes.sizeof(C.TraceHit) == 16 and HIT_DTYPE.itemsize == 16
    assert ctypes.sizeof(C.TraceDesc) == 16
    assert [C.TraceRay.origin.offset, C.TraceRay.tmax.offset, C.TraceRay.direction.offset, C.TraceRay.ignore.offset] == [0, 12, 16, 28]
    assert [RAY_DTYPE.fields[k][1] for k in ("origin", "tmax", "direction", "ignore")] == [0, 12, 16, 28]
    assert [C.TraceHit.t.offset, C.TraceHit.prim.offset, C.TraceHit.u.offset, C.TraceHit.v.offset] == [0, 4, 8, 12]
    assert [HIT_DTYPE.fields[k][1] for k in ("t", "prim", "u", "v")] == [0, 4, 8, 12]
    assert [C.TraceDesc.struct_size.offset, C.TraceDesc.program.offset, C.TraceDesc.kind.offset, C.TraceDesc.flags.offset] == [0, 4, 8, 12]
    assert re.search(r"LT_TRACE_CLOSEST\s*=\s*0\s*,\s*LT_TRACE_ANY\s*=\s*1", HEADER)
    assert (C.TRACE_CLOSEST, C.TRACE_ANY) == (0, 1)
    m = re.search(r"#define\s+LT_TRACE_FLAG_COHERENT\s+(0x[0-9a-fA-F]+)u", HEADER)
    assert m and int(m.group(1), 16) == C.TRACE_FLAG_COHERENT == 0x100
    # the flags a query takes besides COHERENT are the render path's
    assert C.TRACE_FLAG_COHERENT & (C.RENDER_FLAG_STATS | C.RENDER_FLAG_PIXEL_COUNTERS | C.RENDER_FLAG_PORTABLE_MATH |
                                    C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_NO_WALK_TIMING) == 0


def test_null_context_is_an_invalid_argument():
    L = C.load()
    d = C.TraceDesc(ctypes.sizeof(C.TraceDesc), C.PROGRAM_ACCUMULATOR, C.TRACE_CLOSEST, 0)
    rays = make_rays(np.zeros((2, 3)), np.ones((2, 3)))
    out = np.full(2, 7, dtype=HIT_DTYPE)
    before = out.copy()
    assert L.lt_hip_trace_rays(None, ctypes.byref(d), rays.ctypes.data_as(ctypes.c_void_p), 2,
                               out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_trace_rays_device(None, ctypes.byref(d), None, 0, None, 0, None) == C.LT_ERR_INVALID_ARGUMENT
    assert out.tobytes() == before.tobytes()


def test_make_rays_packs_records():
    o = np.array([[1, 2, 3], [-4, 5.5, 0]], dtype=np.float64)
    d = np.array([[0, 0, 1], [-0.0, 1, np.inf]], dtype=np.float32)
    r = make_rays(o, d)
    assert r.dtype == np.float32 and r.shape == (2, 8) and r.flags.c_contiguous
    assert np.array_equal(r[:, 0:3], o.astype(np.float32)) and np.array_equal(r[:, 4:7], d)
    assert np.signbit(r[1, 4])   # -0 kept
    # defaults: tmax is FLT_MAX (the reference's payload start, not inf), ignore -1
    assert FLT_MAX == float(np.finfo(np.float32).max)
    assert np.array_equal(r[:, 3], np.full(2, np.finfo(np.float32).max, dtype=np.float32))
    assert np.array_equal(r[:, 7].view(np.int32), [-1, -1])
    r = make_rays(o, d, tmax=np.array([0.5, -np.inf]), ignore=np.array([12345678, 0]))
    assert np.array_equal(r[:, 3], np.array([0.5, -np.inf], dtype=np.float32))
    assert np.array_equal(r[:, 7].view(np.int32), [12345678, 0])   # bits, not a float conversion
    rec = r.view(RAY_DTYPE).reshape(-1)
    assert rec["ignore"].tolist() == [12345678, 0] and rec["tmax"][0] == np.float32(0.5)
    assert make_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 8)
    nan = make_rays(o, d, tmax=np.nan)
    assert np.isnan(nan[:, 3]).all()


@pytest.mark.parametrize("o,d,kw", [
    (np.zeros(3), np.zeros(3), {}),
    (np.zeros((2, 4)), np.zeros((2, 4)), {}),
    (np.zeros((2, 3)), np.zeros((3, 3)), {}),
    (np.zeros((2, 3)), np.zeros((2, 3)), {"tmax": np.zeros(3)}),
    (np.zeros((2, 3)), np.zeros((2, 3)), {"ignore": np.zeros(3, dtype=np.int32)}),
    (np.zeros((2, 3)), np.zeros((2, 3)), {"ignore": 1.5}),
    (np.zeros((2, 3)), np.zeros((2, 3)), {"ignore": 2 ** 31}),
])
def test_make_rays_rejects_bad_shapes(o, d, kw):
    with pytest.raises(ValueError):
        make_rays(o, d, **kw)
