"""Inputs for the tests of the math flavours' leaf functions (tests/test_math_edges_cpu.py, tests/test_gpu_math_edges.py): per
operation, named families of raw float32 bit patterns at the edges where a hand restatement of a device library goes wrong
-- every binary exponent, denormals, FLT_MIN and its neighbours, zeros, infinities, NaN, squared lengths that straddle FLT_MIN or
overflow, differences that cancel, operands whose fused and unfused evaluation differ -- next to random bit patterns and
ordinary values of the kind images produce.  Plain numpy, seeded: every call returns the same arrays.

inputs(op) -> list of (family name, (n, k) uint32 array), k the operation's input words (oracle/pyoracle.LEAF_OPS, the layout of
oracle/math_probe.cl's kernels).  Exact float32 helpers (round_f32, fma32, exact dot / cross) serve as the high-precision
reference where float64 is not enough."""
import math
from fractions import Fraction

import numpy as np

f32, u32, f64 = np.float32, np.uint32, np.float64
FLT_MIN_BITS, FLT_MAX_BITS, INF_BITS, NAN_BITS = 0x00800000, 0x7f7fffff, 0x7f800000, 0x7fc00000
FLT_MIN = float(np.finfo(f32).tiny)
SIGN = 0x80000000

# operation -> (probe id, input words, output words): oracle/pyoracle.LEAF_OPS
OPS = {"normalize": (1, 4, 4), "distance": (2, 8, 1), "dot4": (3, 8, 1), "dot2": (4, 4, 1), "cross": (5, 8, 4),
       "clamp01": (6, 1, 1), "sin": (7, 1, 1), "cos": (8, 1, 1), "fdiv": (9, 2, 1), "rcp": (10, 1, 1), "div25": (11, 1, 1),
       "sqrt": (12, 1, 1), "mad1": (13, 3, 1), "mad2": (14, 4, 1), "mad3": (15, 6, 1), "mad1d": (16, 6, 2), "rsqrt": (17, 1, 1)}


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(u32)


def floats(b):
    return np.ascontiguousarray(b, dtype=u32).view(f32)


def _both_signs(b):
    b = np.asarray(b, dtype=u32)
    return np.concatenate([b, b | u32(SIGN)])


# ---------------------------------------------------------------------------------------------------------------- scalars
def scalar_families(seed=1):
    """Named families of float32 bit patterns, (n,) uint32 each."""
    rng = np.random.default_rng(seed)
    exps = np.arange(1, 255, dtype=u32) << u32(23)
    fam = {}
    fam["exponents"] = _both_signs(np.concatenate([exps, exps | u32(0x7fffff), exps | rng.integers(1, 0x7fffff, exps.size).astype(u32)]))
    fam["denormals"] = _both_signs(np.concatenate([np.array([1, 2, 3, 0x7fffff, 0x7ffffe, 0x400000, 0x3fffff], dtype=u32),
                                                    u32(1) << np.arange(23, dtype=u32), rng.integers(1, 0x800000, 64).astype(u32)]))
    fam["flt_min_neighbours"] = _both_signs(np.array([FLT_MIN_BITS - 1, FLT_MIN_BITS, FLT_MIN_BITS + 1], dtype=u32))
    fam["zeros_infinities"] = np.array([0, SIGN, INF_BITS, INF_BITS | SIGN], dtype=u32)
    fam["nan"] = np.array([NAN_BITS, NAN_BITS | SIGN, 0x7fc00001, 0x7f800001, 0xffffffff], dtype=u32)
    fam["random_bits"] = rng.integers(0, 2 ** 32, 1024, dtype=np.uint64).astype(u32)
    fam["ordinary"] = bits(np.concatenate([rng.uniform(0.0, 1.0, 128), rng.uniform(-10.0, 10.0, 128), 10.0 ** rng.uniform(0.0, 4.0, 128),
                                           np.arange(0.0, 26.0), rng.uniform(0.0, 2.0 * math.pi, 128), rng.uniform(-1.5, 2.5, 64)]))
    return fam


def angle_families(seed=2):
    """sin / cos: multiples of pi/2 and their float neighbours, arguments up to 2^127."""
    rng = np.random.default_rng(seed)
    k = np.concatenate([np.arange(0, 65), 2 ** np.arange(7, 40, dtype=f64), 2 ** np.arange(7, 40, dtype=f64) + 1, rng.integers(65, 10 ** 6, 64)]).astype(f64)
    centre = bits((k * (math.pi / 2)).astype(f32)).astype(np.int64)
    near = np.concatenate([centre + d for d in (-2, -1, 0, 1, 2)])
    near = near[near >= 0].astype(u32)
    e = np.repeat(np.arange(104, 255, dtype=u32), 3) << u32(23)   # 2^-23 .. 2^127
    huge = e | rng.integers(0, 0x800000, e.size).astype(u32)
    return {"pi_half_multiples": _both_signs(near), "up_to_2p127": _both_signs(huge)}


def division_families(seed=3):
    """(n, 2) uint32: numerator, denominator."""
    rng = np.random.default_rng(seed)
    s = scalar_families()
    fam = {}
    sweep = s["exponents"]
    fam["exponents_over_exponents"] = np.stack([sweep, rng.permutation(sweep)], axis=-1)
    fam["ordinary_over_exponents"] = np.stack([np.resize(s["ordinary"], sweep.size), sweep], axis=-1)
    fam["exponents_over_ordinary"] = np.stack([sweep, np.resize(s["ordinary"], sweep.size)], axis=-1)

    def mant(n):
        return rng.integers(0, 0x800000, n).astype(u32)

    def pair(ea, eb, n=None):   # biased exponents (0 = denormal) with random mantissas and signs
        ea, eb = np.asarray(ea, dtype=u32), np.asarray(eb, dtype=u32)
        a = (ea << u32(23)) | mant(ea.size) | (rng.integers(0, 2, ea.size).astype(u32) << u32(31))
        b = (eb << u32(23)) | mant(eb.size) | (rng.integers(0, 2, eb.size).astype(u32) << u32(31))
        return np.stack([a, b], axis=-1)
    hi = rng.integers(200, 255, 256)
    fam["quotient_overflows"] = pair(hi, np.maximum(hi.astype(np.int64) - rng.integers(129, 200, 256), 0))
    lo = rng.integers(1, 100, 256)
    fam["quotient_denormal"] = pair(lo, lo + rng.integers(127, 150, 256))       # quotient around 2^-127 .. 2^-150
    fam["quotient_near_flt_min"] = pair(lo, lo + rng.integers(125, 128, 256))
    d = _both_signs(np.concatenate([np.array([1, 2, 3, 0x7fffff, 0x400000], dtype=u32), rng.integers(1, 0x800000, 120).astype(u32)]))
    fam["denormal_over_denormal"] = np.stack([d, rng.permutation(d)], axis=-1)
    fam["denormal_over_normal"] = np.stack([d, np.resize(sweep[::3], d.size)], axis=-1)
    fam["normal_over_denormal"] = np.stack([np.resize(sweep[::3], d.size), d], axis=-1)
    sp = np.concatenate([s["zeros_infinities"], s["flt_min_neighbours"], bits([1.0, -1.0, 3.0, 25.0]), np.array([1, FLT_MAX_BITS], dtype=u32)])
    fam["zeros_infinities"] = np.stack(np.meshgrid(sp, sp, indexing="ij"), axis=-1).reshape(-1, 2)
    nan = s["nan"]
    fam["nan"] = np.concatenate([np.stack([nan, np.resize(sp, nan.size)], axis=-1), np.stack([np.resize(sp, nan.size), nan], axis=-1),
                                 np.stack([nan, nan], axis=-1)])
    fam["random_bits"] = rng.integers(0, 2 ** 32, (1024, 2), dtype=np.uint64).astype(u32)
    width = rng.choice([64, 96, 100, 128, 256, 480, 1920, 3840], 384).astype(f64)
    fam["ordinary"] = np.concatenate([np.stack([bits(np.floor(rng.uniform(0, 1, 384) * width)), bits(width)], axis=-1),
                                      np.stack([bits(rng.uniform(1.0, 2.0, 128)), bits(rng.uniform(1.0, 2.0, 128))], axis=-1)])
    return fam


# ---------------------------------------------------------------------------------------------------------------- vectors
def _scaled_to_l2(rng, n, l2, dominant=False):
    """n random float32 4-vectors whose squared length (float64) is close to l2[i]."""
    d = rng.normal(0.0, 1.0, (n, 4))
    if dominant:
        d[:, 0] = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
        d[:, 1:] *= 2.0 ** rng.integers(-30, -8, (n, 3))
        d = np.take_along_axis(d, np.argsort(rng.random((n, 4)), axis=1), axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return bits((d * np.sqrt(np.asarray(l2, dtype=f64))[:, None]).astype(f32))


def vector_families(seed=4):
    """Named families of float32 4-vectors, (n, 4) uint32 each."""
    rng = np.random.default_rng(seed)
    fam = {}
    fam["zero"] = np.array([[SIGN if (m >> j) & 1 else 0 for j in range(4)] for m in range(16)], dtype=u32)
    # squared length straddling FLT_MIN: within a few ulps either side, and up to a factor 4 either side
    n = 384
    rel = np.concatenate([1.0 + rng.integers(-40, 41, n // 2) * 2.0 ** -24, 2.0 ** rng.uniform(-2.0, 2.0, n // 2)])
    fam["l2_straddles_flt_min"] = np.concatenate([_scaled_to_l2(rng, n, FLT_MIN * rel), _scaled_to_l2(rng, n, FLT_MIN * rel, dominant=True)])
    small = 2.0 ** rng.uniform(-149.0, -64.0, 256)
    fam["l2_below_flt_min"] = _scaled_to_l2(rng, 256, small * small)
    den = rng.integers(0, 0x800000, (256, 4)).astype(u32) | (rng.integers(0, 2, (256, 4)).astype(u32) << u32(31))
    den[:8] = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [1, 1, 1, 1], [0x7fffff] * 4, [0x7fffff, 1, 0, 0], [0, 0x400000, 0, 0], [1, SIGN | 1, 1, SIGN | 1], [0, 0, 1, 0]], dtype=u32)
    fam["all_denormal"] = den
    # l2 overflows, every component finite: components from 2^63.5 up to FLT_MAX
    big = 2.0 ** rng.uniform(63.5, 127.99, (256, 4)) * rng.choice([-1.0, 1.0], (256, 4))
    b = bits(big.astype(f32)).reshape(256, 4)
    b[:6] = np.array([[FLT_MAX_BITS] * 4, [FLT_MAX_BITS, 0, 0, 0], [0, SIGN | FLT_MAX_BITS, 0, 0], [FLT_MAX_BITS, 1, SIGN, 0x3f800000],
                      [0x5f800000, 0, 0, 0], [0x5f3504f4, 0x5f3504f4, 0, 0]], dtype=u32)   # 2^64; 2^63.5 (rounded up) twice
    fam["l2_overflows_components_finite"] = b
    one_big = _scaled_to_l2(rng, 128, np.full(128, 1.0))
    one_big[np.arange(128), rng.integers(0, 4, 128)] = bits((2.0 ** rng.uniform(64.0, 127.99, 128) * rng.choice([-1.0, 1.0], 128)).astype(f32))
    fam["l2_overflows_one_component"] = one_big
    lim = 2.0 ** rng.uniform(-2.0, 2.0, 128) * 2.0 ** 128
    fam["l2_straddles_overflow"] = _scaled_to_l2(rng, 128, lim)
    # infinite components (the only vectors whose l2 still overflows after the 2^-66 rescale: FLT_MAX * 2^-66 squares to 2^124)
    inf = []
    for mask in range(1, 16):
        for rep in range(6):
            v = bits(rng.normal(0.0, 10.0 ** rng.uniform(-3, 30), 4).astype(f32)).copy()
            if rep == 0:
                v[:] = [0, SIGN, 0, SIGN]
            if rep == 1:
                v[:] = [FLT_MAX_BITS, SIGN | FLT_MAX_BITS, 1, SIGN | 1]
            for j in range(4):
                if (mask >> j) & 1:
                    v[j] = INF_BITS | (SIGN if rng.integers(0, 2) else 0)
            inf.append(v)
    fam["infinite_components"] = np.array(inf, dtype=u32)
    nanv = bits(rng.normal(0.0, 1.0, (24, 4)).astype(f32)).reshape(24, 4)
    nanv[np.arange(24), np.arange(24) % 4] = np.resize(np.array([NAN_BITS, NAN_BITS | SIGN, 0x7f800001], dtype=u32), 24)
    nanv[4:8][:, :] = np.where(np.eye(4, dtype=bool), u32(NAN_BITS), u32(0))                     # NaN next to zeros
    nanv[8:12][:, :] = np.where(np.eye(4, dtype=bool), u32(NAN_BITS), u32(INF_BITS))             # NaN next to infinities
    fam["nan_component"] = nanv
    fam["random_bits"] = rng.integers(0, 2 ** 32, (768, 4), dtype=np.uint64).astype(u32)
    o = np.concatenate([rng.normal(0.0, 1.0, (128, 4)), rng.uniform(-60.0, 60.0, (128, 4)), rng.normal(0.0, 1.0, (128, 4)) * 10.0 ** rng.uniform(-3, 3, (128, 1))])
    o[:, 3] = np.where(rng.random(384) < 0.5, 0.0, o[:, 3])   # directions carry w = 0
    fam["ordinary"] = bits(o.astype(f32)).reshape(-1, 4)
    return fam


def pair_families(seed=5):
    """(n, 8) uint32: two 4-vectors.  For distance the first family names describe a - b (b = 0 or a vector of the same family)."""
    rng = np.random.default_rng(seed)
    fam = {}
    for name, v in vector_families().items():
        zero = np.zeros_like(v)
        fam[name] = np.concatenate([np.concatenate([v, zero], axis=1), np.concatenate([zero, v], axis=1),
                                    np.concatenate([v, rng.permutation(v)], axis=1), np.concatenate([v, v ^ u32(SIGN)], axis=1)])
    # differences that cancel to zero or to a denormal
    base = bits((rng.normal(0.0, 1.0, (256, 4)) * 2.0 ** rng.integers(-125, -100, (256, 1))).astype(f32)).reshape(256, 4)
    other = (base.astype(np.int64) + rng.integers(-3, 4, (256, 4))).astype(u32)
    fam["difference_cancels"] = np.concatenate([np.concatenate([base, base], axis=1), np.concatenate([base, other], axis=1)])
    o = bits(rng.uniform(-60.0, 60.0, (256, 4)).astype(f32)).reshape(256, 4)
    o2 = (o.astype(np.int64) + rng.integers(-2, 3, (256, 4))).astype(u32)
    fam["difference_of_neighbours"] = np.concatenate([o, o2], axis=1)
    return fam


# ---------------------------------------------------------------------------------------------------------------- contraction
def contraction_families(terms, seed=6, double=False):
    """a*b + c [+ d*e ...] with `terms` products.  fused_differs: the first product has a non-zero low part and the addend all but
    cancels its high part, so one rounding (fused) and two (unfused) give different results."""
    rng = np.random.default_rng(seed + terms + (10 if double else 0))
    n = 512
    ft = f64 if double else f32
    scale = 2.0 ** rng.integers(-30, 30, n)
    a = (rng.uniform(1.0, 2.0, n) * scale).astype(ft)
    b = rng.uniform(1.0, 2.0, n).astype(ft) * rng.choice([-1.0, 1.0], n).astype(ft)
    p = (a * b).astype(ft)                          # the rounded product: the addend cancels it, the low part is what is left
    cols = [a, b]
    if terms == 1:
        cols.append(-p)
    else:                                           # the second product IS rounded in either evaluation: make it cancel p
        c = rng.uniform(1.0, 2.0, n).astype(ft)
        d = (-p / c).astype(ft)
        cols += [c, d]
        if terms == 3:
            cols += [(rng.uniform(1.0, 2.0, n) * scale * 2.0 ** -20).astype(ft), rng.uniform(1.0, 2.0, n).astype(ft)]
    fam = {"fused_differs": np.stack(cols, axis=-1)}
    k = len(cols)
    fam["ordinary"] = rng.uniform(-2.0, 2.0, (512, k)).astype(ft)
    fam["wide_range"] = (rng.normal(0.0, 1.0, (512, k)) * 2.0 ** rng.integers(-60 if not double else -400, 60 if not double else 400, (512, k))).astype(ft)
    if double:
        sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 1113.1, 1.0])
        fam["specials"] = sp[rng.integers(0, sp.size, (256, k))]
        return {name: np.ascontiguousarray(v, dtype=f64).view(u32).reshape(v.shape[0], 2 * k) for name, v in fam.items()}
    sp = np.concatenate([scalar_families()[x] for x in ("zeros_infinities", "nan", "flt_min_neighbours", "denormals")])
    out = {name: bits(v).reshape(v.shape[0], k) for name, v in fam.items()}
    out["specials"] = sp[rng.integers(0, sp.size, (512, k))]
    out["random_bits"] = rng.integers(0, 2 ** 32, (512, k), dtype=np.uint64).astype(u32)
    return out


_cache = {}


def inputs(op):
    """[(family name, (n, k) uint32 array)] for one operation of OPS."""
    if op in _cache:
        return _cache[op]
    if op in ("clamp01", "rcp", "div25", "sqrt", "rsqrt"):
        fam = {k: v[:, None] for k, v in scalar_families().items()}
    elif op in ("sin", "cos"):
        fam = {k: v[:, None] for k, v in {**scalar_families(), **angle_families()}.items()}
    elif op == "fdiv":
        fam = division_families()
    elif op == "normalize":
        fam = vector_families()
    elif op in ("distance", "dot4", "cross"):
        fam = pair_families()
    elif op == "dot2":
        fam = {k: v[:, [0, 1, 4, 5]] for k, v in pair_families().items()}
    elif op in ("mad1", "mad2", "mad3"):
        fam = contraction_families(int(op[3]))
    elif op == "mad1d":
        fam = contraction_families(1, double=True)
    else:
        raise KeyError(op)
    out = [(k, np.ascontiguousarray(v, dtype=u32)) for k, v in fam.items()]
    assert all(v.ndim == 2 and v.shape[1] == OPS[op][1] for _, v in out), op
    _cache[op] = out
    return out


def all_inputs(op):
    """One (n, k) array for the operation and the family index of every row."""
    fams = inputs(op)
    return np.concatenate([v for _, v in fams]), np.concatenate([np.full(v.shape[0], i) for i, (_, v) in enumerate(fams)]), [k for k, _ in fams]


# ---------------------------------------------------------------------------------------------------------------- probe records
RECORD_WORDS = 18   # op id, 8 input words, 4 expected words, 5 spare: two primitives' normals


def pack_records(batches):
    """batches: [(op, inputs (n, k), expected (n, m))] -> the (records, 18) uint32 array tests/user_kernels/math_probe.hip reads."""
    rows = []
    for op, words_in, expected in batches:
        opid, k, m = OPS[op]
        assert words_in.shape[1] == k and expected.shape == (words_in.shape[0], m)
        r = np.zeros((words_in.shape[0], RECORD_WORDS), dtype=u32)
        r[:, 0] = opid
        r[:, 1:1 + k] = words_in
        r[:, 9:9 + m] = expected
        rows.append(r)
    return np.concatenate(rows)


def probe_payload(records, W, H):
    """The word stream of the primitives' normals: a header primitive (W, H, records), then the records; returns (n_prims, 9) uint32."""
    assert records.shape[0] <= W * H
    words = np.concatenate([np.array([W, H, records.shape[0], 0, 0, 0, 0, 0, 0], dtype=u32), records.reshape(-1)])
    return words.reshape(-1, 9)


# ---------------------------------------------------------------------------------------------------------------- exact float32
def round_f32(q):
    """The float32 nearest (ties to even) to the rational q, overflow to infinity; the sign of an exact zero is the caller's."""
    if q == 0:
        return 0.0
    s, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                     # 2^e <= q < 2^(e+1)
    e = max(e, -126)
    m = q / Fraction(2) ** (e - 23)                # significand in units of the last place
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    if n >= 2 ** 24 and e >= 127:
        return s * math.inf
    v = math.ldexp(n, e - 23)
    return s * (math.inf if v > 3.4028234663852886e38 else v)


def fma32(a, b, c):
    """float32 fma(a, b, c) with one rounding, on Python floats that hold float32 values."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(f64(a) * f64(b) + f64(c))   # (no rounding matters once something is infinite or NaN)
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:                                       # IEEE: the sum of opposite-signed zeros / exact cancellation is +0, like signs keep theirs
        p = a * b
        neg = math.copysign(1.0, p) < 0 and math.copysign(1.0, c) < 0 if (p == 0 and c == 0) else False
        return -0.0 if neg else 0.0
    return round_f32(q)


def mul32(a, b):
    return float(f32(a) * f32(b))


def dot4_exact_chain(a, b):
    """fma(a.w, b.w, fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))): the OpenCL device library's dot, every step rounded once."""
    with np.errstate(all="ignore"):
        r = mul32(a[0], b[0])
    for j in range(1, len(a)):
        r = fma32(a[j], b[j], r)
    return r


def cross_exact_chain(a, b):
    with np.errstate(all="ignore"):
        return [fma32(a[1], b[2], -mul32(a[2], b[1])), fma32(a[2], b[0], -mul32(a[0], b[2])), fma32(a[0], b[1], -mul32(a[1], b[0])), 0.0]


def ulp32(x):
    """Spacing of float32 at |x| (float64 array), the denormal spacing below FLT_MIN."""
    x = np.abs(np.asarray(x, dtype=f64))
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.maximum(x, FLT_MIN)))
    return 2.0 ** (np.clip(e, -126, 127) - 23)


_PI_BITS = 1400


def _pi_scaled():
    """floor(pi * 2^_PI_BITS) by Machin's formula in integer arithmetic."""
    one = 1 << (_PI_BITS + 32)

    def atan_inv(x):
        t = one // x
        s, k, x2, sign = t, 1, x * x, 1
        while t:
            t //= x2
            k += 2
            sign = -sign
            s += sign * (t // k)
        return s
    return (4 * (4 * atan_inv(5) - atan_inv(239))) >> 32


_pi_int = None


def sincos_reference(x):
    """(sin x, cos x) of a finite float to about 2^-52 relative: the argument is reduced modulo pi/2 exactly (integers, 1400 bits of
    pi: a float32's 2^127 needs under 300), the reduced argument's sine and cosine are math.sin / math.cos of a double."""
    global _pi_int
    if _pi_int is None:
        _pi_int = _pi_scaled()
    q = Fraction(x)
    half_pi = Fraction(_pi_int, 1 << (_PI_BITS + 1))
    k = round(q / half_pi)
    r = float(q - k * half_pi)                      # |r| <= pi/4; absolute error 2^-1100 |k|, relative error of the rounding 2^-53
    s, c = math.sin(r), math.cos(r)
    return [(s, c), (c, -s), (-s, -c), (-c, s)][k % 4]
