"""The surface record of a hit, restated in numpy, and rays aimed at a scene's lights: what the tests of the surface queries
(tests/test_gpu_surface.py; what this module claims: tests/test_surface_cpu.py) compare lt_hip_trace_surface and
lt_hip_surface_at with.

* expected(scene, hits, flavour): the SURFACE_DTYPE records of HIT_DTYPE records -- t, u, v copied; b = ((float)(1.0 - u - v)
  evaluated in double, u, v); position and normal A*b.x + B*b.y + C*b.z of the primitive's positions and normals, in the
  "default" flavour as fma(C, b.z, fma(A, b.x, B*b.y)) with each fma rounded ONCE, in "strict" and "portable" with the three
  products and the two sums rounded to float32 one by one; the material index; LT_SURFACE_LIGHT from the light list.  A record whose
  prim is none of the scene's primitives gives the miss form.
* fma32(a, b, c): float32 fused multiply-add, exact: the product of two float32 is exact in float64, the float64 sum is turned
  into its round-to-odd value with the sum's exact error (TwoSum), and a round-to-odd value of 53 bits rounds to 24 bits as the
  exact sum would.
* light_rays(scene): rays from near the light primitives onto points of them."""
import numpy as np

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import HIT_DTYPE, SURFACE_DTYPE, make_rays

F32 = np.float32
FLAVOURS = {"default": {}, "strict": {"strict_math": True}, "portable": {"portable_math": True}}


def fma32(a, b, c):
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    p = a * b                                   # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)             # s + err == p + c exactly
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0) & even & np.isfinite(s)
    with np.errstate(invalid="ignore"):
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where(fix, odd, s).astype(F32)


def interpolate(A, B, Cc, b, flavour):
    """A*b.x + B*b.y + C*b.z per component: A, B, Cc (n, 3) float32, b (n, 3) float32."""
    A, B, Cc, b = (np.asarray(x, dtype=F32) for x in (A, B, Cc, b))
    bx, by, bz = b[:, 0:1], b[:, 1:2], b[:, 2:3]
    if flavour == "default":
        return fma32(Cc, bz, fma32(A, bx, B * by))
    return (A * bx + B * by) + Cc * bz


def barycentrics(u, v):
    u, v = np.asarray(u, dtype=F32), np.asarray(v, dtype=F32)
    return np.stack([((1.0 - u.astype(np.float64)) - v.astype(np.float64)).astype(F32), u, v], axis=-1)


def expected(scene, hits, flavour="default"):
    assert flavour in FLAVOURS and hits.dtype == HIT_DTYPE
    flat = np.ascontiguousarray(hits).reshape(-1)
    out = np.zeros(len(flat), dtype=SURFACE_DTYPE)
    out["t"] = flat["t"]
    out["prim"] = -1
    out["material"] = -1
    ok = (flat["prim"] >= 0) & (flat["prim"] < scene.n_prims)
    p = flat["prim"][ok]
    pv = scene.prim_view
    lv = scene.light_view[0]
    with np.errstate(invalid="ignore", over="ignore"):
        b = barycentrics(flat["u"][ok], flat["v"][ok])
        pos = interpolate(pv["positionA"][p], pv["positionB"][p], pv["positionC"][p], b, flavour)
        nrm = interpolate(pv["normalA"][p], pv["normalB"][p], pv["normalC"][p], b, flavour)
    out["prim"][ok] = p
    out["u"][ok], out["v"][ok] = flat["u"][ok], flat["v"][ok]
    out["position"][ok], out["normal"][ok] = pos, nrm
    out["material"][ok] = pv["materialIndex"][p]
    out["flags"][ok] = np.where(np.isin(p, lv["primitives"][:int(lv["count"])]), C.SURFACE_LIGHT, 0)
    return out.reshape(hits.shape)


def light_prims(scene):
    lv = scene.light_view[0]
    return lv["primitives"][:int(lv["count"])].astype(np.int64)


def light_rays(scene, n=128, seed=0):
    """n rays (a multiple of 64), each from a point within a few units of a light primitive onto a point of its interior."""
    rng = np.random.default_rng(seed)
    lp = light_prims(scene)
    assert len(lp) > 0 and n % 64 == 0
    p = lp[rng.integers(0, len(lp), n)]
    pv = scene.prim_view
    A, B, Cc = (pv[k][p].astype(np.float64) for k in ("positionA", "positionB", "positionC"))
    b = rng.dirichlet([2, 2, 2], n)
    target = b[:, 0:1] * A + b[:, 1:2] * B + b[:, 2:3] * Cc
    nrm = np.cross(B - A, Cc - A)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    away = nrm * rng.choice([-1.0, 1.0], (n, 1)) * rng.uniform(1.0, 3.0, (n, 1)) + rng.normal(0, 0.3, (n, 3))
    o = target + away
    return make_rays(o, target - o)


FLOAT_WORDS = [4, 5, 6, 8, 9, 10]   # position and normal


def same(got, want):
    """Indices of the records that differ in any bit -- except that in a position or normal component any two NaNs are equal
    (u or v NaN: which of two NaN operands an operation returns, and with which sign, differs between processors)."""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 12)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 12)
    differ = g != w
    both_nan = np.isnan(g[:, FLOAT_WORDS].view(np.float32)) & np.isnan(w[:, FLOAT_WORDS].view(np.float32))
    differ[:, FLOAT_WORDS] &= ~both_nan
    return np.flatnonzero(differ.any(axis=1))
