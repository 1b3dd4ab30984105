"""No GPU: the surface queries' C ABI as far as it can be checked without one (symbols, record layouts, the null-context error),
and what tests/surface.py claims -- its fused multiply-add is exact, its records stay within the rounding bound of the float64
value, its fixtures hit lights and non-lights."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import HIT_DTYPE, SURFACE_DTYPE
from oracle import pyoracle as po
from tests import query_edges as qe
from tests import surface as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lt_hip_trace_surface", "lt_hip_trace_surface_device", "lt_hip_surface_at", "lt_hip_surface_at_device")
F32 = np.float32


def test_the_four_symbols_are_declared_exported_and_loadable():
    L = C.load()
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    declared = set(re.findall(r"^int\s+(lt_hip_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in C.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int and len(getattr(L, name).argtypes) in (6, 7)
    assert L.lt_hip_abi_version() == 4
    assert re.search(r"#define\s+LT_HIP_ABI_VERSION\s+4\b", header)


def test_record_layouts_match_the_header():
    header = open(os.path.join(ROOT, "include", "lenstrace_hip.h")).read()
    body = re.search(r"typedef struct lt_hip_surface \{(.*?)\} lt_hip_surface;", header, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.match(r"\s*([a-z_]+)(?:\[(\d+)\])?\s*$", nm)
            fields.append((m.group(1), typ, int(m.group(2) or 1)))
    assert [f[0] for f in fields] == ["t", "prim", "u", "v", "position", "material", "normal", "flags"]
    assert [f[1] for f in fields] == ["float", "int32_t", "float", "float", "float", "int32_t", "float", "uint32_t"]
    off = 0
    for name, _, count in fields:      # every member is 4-byte words: the header's offsets are the running sum
        assert getattr(C.Surface, name).offset == off == SURFACE_DTYPE.fields[name][1], name
        off += 4 * count
    assert off == 48 == ctypes.sizeof(C.Surface) == SURFACE_DTYPE.itemsize
    assert ctypes.sizeof(C.SurfaceDesc) == 8 and C.SurfaceDesc.struct_size.offset == 0 and C.SurfaceDesc.flags.offset == 4
    assert re.search(r"typedef struct lt_hip_surface_desc \{\s*uint32_t struct_size;[^}]*uint32_t flags;\s*\} lt_hip_surface_desc;", header)
    assert re.search(r"#define\s+LT_SURFACE_LIGHT\s+1u\b", header) and C.SURFACE_LIGHT == 1
    assert SURFACE_DTYPE.names == ("t", "prim", "u", "v", "position", "material", "normal", "flags")
    assert SURFACE_DTYPE["position"].shape == (3,) and SURFACE_DTYPE["normal"].shape == (3,)


def test_a_null_context_is_an_invalid_argument_and_writes_nothing():
    L = C.load()
    out = np.full(24, 0x5a5a5a5a, dtype=np.uint32)
    rays = np.zeros((2, 8), dtype=F32)
    hits = np.zeros(2, dtype=HIT_DTYPE)
    O, R, H = (x.ctypes.data_as(ctypes.c_void_p) for x in (out, rays, hits))
    td = C.TraceDesc(ctypes.sizeof(C.TraceDesc), C.PROGRAM_ACCUMULATOR, C.TRACE_CLOSEST, 0)
    sd = C.SurfaceDesc(ctypes.sizeof(C.SurfaceDesc), 0)
    assert L.lt_hip_trace_surface(None, ctypes.byref(td), R, 2, O, out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_trace_surface_device(None, ctypes.byref(td), R, 2, O, out.nbytes, None) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_surface_at(None, ctypes.byref(sd), H, 2, O, out.nbytes) == C.LT_ERR_INVALID_ARGUMENT
    assert L.lt_hip_surface_at_device(None, ctypes.byref(sd), H, 2, O, out.nbytes, None) == C.LT_ERR_INVALID_ARGUMENT
    assert (out == 0x5a5a5a5a).all()


# ---------------------------------------------------------------------------------------------------- tests/surface.py itself
def round_to_f32(q):
    """The Fraction q rounded once to float32, ties to even."""
    f = F32(float(q))                            # within one float32 step of q
    cands = sorted({f, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf))}, key=float)
    best = None
    for c in cands:
        d = abs(Fraction(float(c)) - q)
        even = (np.array([c], dtype=F32).view(np.uint32)[0] & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    return best[1]


def random_hits(rng, n, n_prims):
    h = np.zeros(n, dtype=HIT_DTYPE)
    h["prim"] = rng.integers(0, n_prims, n)
    h["u"] = rng.uniform(-1e-3, 1.0, n)
    h["v"] = rng.uniform(-1e-3, 1.0, n)
    h["t"] = rng.uniform(0, 10, n)
    return h


def test_the_default_flavour_is_an_exact_fused_multiply_add():
    scene = qe.base_scene(0)
    rng = np.random.default_rng(0)
    h = random_hits(rng, 200, scene.n_prims)
    got = sf.expected(scene, h, "default")
    pv = scene.prim_view
    b = sf.barycentrics(h["u"], h["v"])
    for field, keys in (("position", ("positionA", "positionB", "positionC")), ("normal", ("normalA", "normalB", "normalC"))):
        for i in range(len(h)):
            A, B, Cc = (pv[k][h["prim"][i]] for k in keys)
            bx, by, bz = (Fraction(float(x)) for x in b[i])
            for c in range(3):
                prod = Fraction(float(F32(B[c]) * F32(b[i, 1])))                       # B * b.y: a float32 product
                inner = round_to_f32(Fraction(float(A[c])) * bx + prod)                 # fma(A, b.x, .)
                want = round_to_f32(Fraction(float(Cc[c])) * bz + Fraction(float(inner)))   # fma(C, b.z, .)
                assert got[field][i, c].view(np.uint32) == np.asarray(want).view(np.uint32), (field, i, c)
    # and fma32 where a float64 emulation double-rounds: a * b + c = 1 + 2^-23 + 2^-24 - 2^-70 lies below the tie, the float64
    # sum on it
    a, bb, c = F32(2.0 ** -12 * (1 + 2.0 ** -23)), F32(2.0 ** -12 * (1 - 2.0 ** -23)), F32(1 + 2.0 ** -23)
    assert F32(np.float64(a) * np.float64(bb) + np.float64(c)) == F32(1 + 2.0 ** -22)
    assert sf.fma32(a, bb, c) == F32(1 + 2.0 ** -23) == round_to_f32(Fraction(float(a)) * Fraction(float(bb)) + Fraction(float(c)))
    assert sf.fma32(-a, bb, -c) == -F32(1 + 2.0 ** -23)
    # the strict flavour differs from it somewhere in the last bit (the flavours are two forms, not one)
    strict = sf.expected(scene, h, "strict")
    assert (strict["position"].view(np.uint32) != got["position"].view(np.uint32)).any()
    assert np.array_equal(strict.view(np.uint32), sf.expected(scene, h, "portable").view(np.uint32))


def test_expected_stays_within_the_rounding_bound_of_the_float64_value():
    """One rounding for b.x, three products and two sums, each at most 2^-24 of a value of the coordinates' size (|b.x|, |u|, |v|
    <= 1): within 4 * 2^-23 * max |vertex coordinate| per component of the float64 value, for u, v in [-1e-3, 1]."""
    scene = qe.base_scene(0)
    rng = np.random.default_rng(1)
    h = random_hits(rng, 20000, scene.n_prims)
    pv = scene.prim_view
    u, v = h["u"].astype(np.float64), h["v"].astype(np.float64)
    w = np.stack([1.0 - u - v, u, v], axis=-1)
    for flavour in sf.FLAVOURS:
        got = sf.expected(scene, h, flavour)
        for field, keys in (("position", ("positionA", "positionB", "positionC")), ("normal", ("normalA", "normalB", "normalC"))):
            V = np.stack([pv[k][h["prim"]].astype(np.float64) for k in keys], axis=1)       # [n, 3 vertices, 3]
            exact = np.einsum("nk,nkc->nc", w, V)
            bound = 4 * 2.0 ** -23 * np.abs(V).max(axis=(1, 2))[:, None]
            err = np.abs(got[field].astype(np.float64) - exact)
            assert (err <= bound).all(), (flavour, field, float((err / np.maximum(bound, 1e-300)).max()))
    assert np.array_equal(got["material"], pv["materialIndex"][h["prim"]])


def test_expected_gives_the_miss_form_outside_the_scenes_primitives():
    scene = qe.base_scene(0)
    h = np.zeros(4, dtype=HIT_DTYPE)
    h["prim"] = (-1, -7, scene.n_prims, 2 ** 31 - 1)
    h["t"], h["u"], h["v"] = (1.5, np.nan, np.inf, -0.0), 0.25, 0.5
    e = sf.expected(scene, h.reshape(2, 2))
    assert e.shape == (2, 2) and (e["prim"] == -1).all() and (e["material"] == -1).all() and (e["flags"] == 0).all()
    assert np.array_equal(e["t"].view(np.uint32), h["t"].view(np.uint32).reshape(2, 2))
    for k in ("u", "v", "position", "normal"):
        assert (e[k].view(np.uint32) == 0).all(), k


def test_the_fixtures_hit_lights_and_other_primitives():
    scene = qe.base_scene(0)
    lights = set(int(p) for p in sf.light_prims(scene))
    assert lights

    def traced(rays):
        out = []
        for r in rays:
            if not np.isfinite(r[:7]).all():
                continue
            g = int(r[7:8].view(np.int32)[0])
            hit, prim, _ = po.trace(scene, np.append(r[0:3], F32(1)), np.append(r[4:7], F32(0)), po.ACCUMULATOR, tmax=float(r[3]),
                                    ignore=g if g >= 0 else None)
            out.append(prim if hit else -1)
        return np.array(out)

    lr = sf.light_rays(scene)
    assert lr.shape == (128, 8) and lr.dtype == F32
    on_light = traced(lr)
    assert sum(int(p) in lights for p in on_light) >= 32
    others = traced(qe.families(scene, 0)[0].rays[:256])
    assert sum(p >= 0 and int(p) not in lights for p in others) >= 32
