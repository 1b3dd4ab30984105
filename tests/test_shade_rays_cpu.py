"""CPU: the shaded-ray interface (lt_hip_shade_rays) as far as it goes without a GPU, and the fixtures of the GPU tests
(tests/shade_rays.py) held against the CPU oracle.

* the library exports both entry points, the records have the header's sizes, a null context is refused, make_shade_rays packs
  origin, film_x, direction, film_y;
* reference_camera_rays gives the reference camera's rays: the oracle's custom_opencl render -- (u, v, 1 - u - v) of each pixel's
  camera hit -- equals the barycentrics lt_oracle_trace finds along these rays, bit for bit, at every yaw and size the GPU tests use;
* the fixtures hold what the GPU tests rely on: every camera's batch hits geometry with a quarter of its rays at least; in the
  accumulator batches 5 % at least of the hits on non-light primitives are unoccluded and 5 % occluded; in the lens scene 5 % of
  the rays take the lens chain; the cameras' direction octants are all eight."""
import ctypes
import os
import re

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import renderer as R
from oracle import pyoracle as po
from tests import shade_rays as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_entry_points_and_the_records_have_the_headers_sizes():
    L = C.load()
    assert hasattr(L, "lt_hip_shade_rays") and hasattr(L, "lt_hip_shade_rays_device")
    assert "lt_hip_shade_rays" in C.EXPORTS and "lt_hip_shade_rays_device" in C.EXPORTS
    assert ctypes.sizeof(C.ShadeRay) == 32 and ctypes.sizeof(C.ShadeResult) == 16 and ctypes.sizeof(C.ShadeDesc) == 24
    assert C.SHADE_RAY_DTYPE.itemsize == 32 and C.SHADE_DTYPE.itemsize == 16
    assert C.SHADE_DTYPE.fields["prim"][1] == 12 and C.SHADE_RAY_DTYPE.fields["film_x"][1] == 12 and C.SHADE_RAY_DTYPE.fields["film_y"][1] == 28
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    for name in ("lt_hip_shade_ray", "lt_hip_shade", "lt_hip_shade_desc", "lt_hip_shade_rays", "lt_hip_shade_rays_device"):
        assert re.search(r"\b%s\b" % name, header), name
    fields = re.search(r"typedef struct lt_hip_shade_desc \{(.*?)\} lt_hip_shade_desc;", header, re.S).group(1)
    assert re.findall(r"(?:uint32_t|int32_t) (\w+);", fields) == [n for n, _ in C.ShadeDesc._fields_]
    for name, value in (("LT_TRACE_FLAG_COHERENT", C.TRACE_FLAG_COHERENT),):
        assert int(re.search(r"#define %s (0x[0-9a-f]+)u" % name, header).group(1), 16) == value
    for name, value in (("LT_RENDER_FLAG_PORTABLE_MATH", C.RENDER_FLAG_PORTABLE_MATH), ("LT_RENDER_FLAG_STRICT_MATH", C.RENDER_FLAG_STRICT_MATH)):
        assert int(re.search(r"%s\s*=?\s*(0x[0-9a-f]+|\d+)" % name, header).group(1), 0) == value
    assert re.search(r"LT_KERNEL_MODE_LINEAR = 0, LT_KERNEL_MODE_TILE = 1", header) and (C.KERNEL_MODE_LINEAR, C.KERNEL_MODE_TILE) == (0, 1)
    assert L.lt_hip_abi_version() == 4


def test_a_null_context_is_an_invalid_argument():
    L = C.load()
    d = C.ShadeDesc(ctypes.sizeof(C.ShadeDesc), C.PROGRAM_ACCUMULATOR, C.KERNEL_MODE_LINEAR, 0, 0, 1)
    rays = R.make_shade_rays(np.zeros((2, 3)), np.ones((2, 3)), 0.0, 0.0)
    out = np.full(8, 0x5a5a5a5a, dtype=np.uint32)
    assert L.lt_hip_shade_rays(None, ctypes.byref(d), rays.ctypes.data_as(ctypes.c_void_p), 2, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_shade_rays_device(None, ctypes.byref(d), None, 0, None, 0, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (out == 0x5a5a5a5a).all()


def test_make_shade_rays_packs_origin_film_x_direction_film_y():
    o = np.arange(12, dtype=np.float64).reshape(4, 3)
    d = -np.arange(12, dtype=np.float64).reshape(4, 3) - 1
    fx = np.float32([0.25, -0.5, 0.0, -0.0])
    rays = R.make_shade_rays(o, d, fx, 0.125)
    assert rays.dtype == np.float32 and rays.shape == (4, 8) and rays.flags.c_contiguous
    rec = rays.view(R.SHADE_RAY_DTYPE).reshape(-1)
    assert np.array_equal(rec["origin"], o.astype(np.float32)) and np.array_equal(rec["direction"], d.astype(np.float32))
    assert np.array_equal(rec["film_x"].view(np.uint32), fx.view(np.uint32)) and (rec["film_y"] == np.float32(0.125)).all()
    assert R.make_shade_rays(np.zeros((0, 3)), np.zeros((0, 3)), 0, 0).shape == (0, 8)
    for bad in ((np.zeros((4, 2)), d, 0, 0), (o, d[:3], 0, 0), (o, d, np.zeros(3), 0), (o, d, 0, np.zeros((4, 1)))):
        with pytest.raises(ValueError):
            R.make_shade_rays(*bad)


CAMERA_CASES = [(yaw, dist, W, H) for yaw, dist in F.CAMERAS for W, H in F.SIZES] + [(yaw, dist) + F.RING_SIZE for yaw, dist in F.RING]


@pytest.mark.parametrize("yaw,dist,W,H", CAMERA_CASES)
def test_reference_camera_rays_are_the_oracles_camera_rays(yaw, dist, W, H):
    o, d, fx, fy = R.reference_camera_rays(F.camera(yaw, dist), W, H)
    assert o.shape == d.shape == (W * H, 3) and fx.shape == fy.shape == (W * H,) and o.dtype == d.dtype == fx.dtype == fy.dtype == np.float32
    x, y = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    assert np.array_equal(fx, (x.astype(np.float32) / np.float32(W) - np.float32(0.5))) and np.array_equal(fy, (y.astype(np.float32) / np.float32(H) - np.float32(0.5)))
    name = "cornell_box_O0"
    want = F.oracle_image(name, yaw, dist, W, H, "custom_opencl", po.MODE_LINEAR, 0).reshape(-1, 3)
    prim, uv = F.oracle_hits(name, F.camera_batch(yaw, dist, W, H), po.CUSTOM)
    got = np.zeros((W * H, 3), dtype=np.float32)
    h = prim >= 0
    got[h, 0], got[h, 1] = uv[h, 0], uv[h, 1]
    got[h, 2] = ((1.0 - uv[h, 0].astype(np.float64)) - uv[h, 1].astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())
    assert h.mean() >= 0.25


def test_the_fixtures_hold_what_the_gpu_tests_rely_on():
    octants = set()
    for name in ("cornell_box_O0", "cornell_box_lens_O0"):
        for W, H in F.SIZES + (F.RING_SIZE,):
            cams = F.RING if (W, H) == F.RING_SIZE else F.CAMERAS
            total = dict(n=0, nonlight=0, lit=0, occluded=0, lens=0)
            for yaw, dist in cams:
                f = F.batch_facts(name, yaw, dist, W, H)
                assert 4 * f["hit"] >= f["n"], (name, yaw, dist, W, H, f)
                if name == "cornell_box_O0" and cams is F.CAMERAS:   # an accumulator batch of its own
                    assert 20 * f["lit"] >= f["nonlight"] > 0 and 20 * f["occluded"] >= f["nonlight"], (yaw, dist, W, H, f)
                for k in total:
                    total[k] += f[k]
                octants |= f["octants"]
            # the batches that go out as one: the ring's rays; the lens scene's cameras between them
            assert 20 * total["lit"] >= total["nonlight"] > 0 and 20 * total["occluded"] >= total["nonlight"], (name, W, H, total)
            if name == "cornell_box_lens_O0":
                assert 20 * total["lens"] >= total["n"], (W, H, total)
        assert octants == set(range(8))
    assert set().union(*(F.batch_facts("cornell_box_O0", yaw, dist, *F.SIZES[0])["octants"] for yaw, dist in F.CAMERAS)) == set(range(8))
    assert set().union(*(F.batch_facts("cornell_box_O0", yaw, dist, *F.RING_SIZE)["octants"] for yaw, dist in F.RING)) == set(range(8))
    rays, cam, pix = F.ring_batch()
    assert len(rays) == 12 * 256 and sorted(zip(cam.tolist(), pix.tolist())) == [(c, p) for c in range(12) for p in range(256)]
    assert (np.diff(cam) != 0).mean() > 0.8   # shuffled: neighbours come from different cameras
