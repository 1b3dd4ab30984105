"""CPU tests of tests/math_edges.py -- each input family really is what its name claims, checked in float64 / exact rational
arithmetic -- and of the CPU oracle's leaf functions (oracle/lt_oracle.c: normalize4, distance4, rsqrt_portable, sinf_portable,
cosf_portable, clamp01, dot4, dot2, cross4, through lt_oracle_leaf) against a high-precision reference on the whole input set.
tests/test_gpu_math_edges.py then holds the HIP path's portable flavour against these oracle functions bit for bit."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import math_edges as me

f32, f64, u32 = np.float32, np.float64, np.uint32
INF = math.inf
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered in cast")   # signalling NaNs widened to float64


def fam(op, name):
    return dict(me.inputs(op))[name]


def l2_chain(v):
    """float32 dot(v, v) as the device library's fma chain computes it, exactly."""
    x = [float(t) for t in me.floats(v)]
    return me.dot4_exact_chain(x, x)


def same_bits_or_nan(got, want):
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    return (got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))


# ------------------------------------------------------------------------------------------------ the families' own claims
def test_scalar_families_are_what_they_claim():
    s = me.scalar_families()
    e = s["exponents"]
    for sign in (0, 1):
        assert set(((e[(e >> 31) == sign] >> 23) & 0xff).tolist()) == set(range(1, 255)), "every normal binary exponent, both signs"
    m = e & 0x7fffff
    assert (m == 0).sum() >= 508 and (m == 0x7fffff).sum() >= 508 and ((m != 0) & (m != 0x7fffff)).sum() >= 500
    d = s["denormals"]
    assert ((d >> 23) & 0xff).max() == 0 and (d & 0x7fffff).min() == 1 and (d & 0x7fffff).max() == 0x7fffff
    assert sorted(me.floats(s["flt_min_neighbours"])[:3].astype(f64).tolist()) == [me.FLT_MIN - 2.0 ** -149, me.FLT_MIN, me.FLT_MIN + 2.0 ** -149]
    z = me.floats(s["zeros_infinities"]).astype(f64)
    assert z.tolist() == [0.0, 0.0, INF, -INF] and np.signbit(z).tolist() == [False, True, False, True]
    assert np.isnan(me.floats(s["nan"])).all()
    o = me.floats(s["ordinary"])
    assert np.isfinite(o).all() and np.abs(o).max() <= 1e4
    a = me.angle_families()
    x = me.floats(a["pi_half_multiples"]).astype(f64)
    k = np.round(x / (math.pi / 2))
    assert (np.abs(x - k * (math.pi / 2)) <= 3.0 * me.ulp32(x)).all() and np.abs(k).max() >= 2 ** 39
    assert np.abs(me.floats(a["up_to_2p127"])).max() >= 2.0 ** 127 and np.isfinite(me.floats(a["up_to_2p127"])).all()


def test_division_families_are_what_they_claim():
    d = me.division_families()

    def quotient(name):
        a, b = me.floats(d[name][:, 0]).astype(f64), me.floats(d[name][:, 1]).astype(f64)
        return np.abs(a / b)     # exact to 2^-53: float64 holds every float32 quotient's magnitude
    assert (quotient("quotient_overflows") > float(np.finfo(f32).max)).all()
    q = quotient("quotient_denormal")
    assert (q < me.FLT_MIN).all() and (q > 2.0 ** -151).all()
    q = quotient("quotient_near_flt_min")
    assert (q < me.FLT_MIN).any() and (q >= me.FLT_MIN).any() and (q < 8 * me.FLT_MIN).all() and (q > me.FLT_MIN / 8).all()
    for name, cols in (("denormal_over_denormal", (0, 1)), ("denormal_over_normal", (0,)), ("normal_over_denormal", (1,))):
        for c in (0, 1):
            e = (d[name][:, c] >> 23) & 0xff
            assert ((e == 0).all() and (d[name][:, c] & 0x7fffff).all()) if c in cols else (e > 0).all(), name
    assert np.isnan(me.floats(d["nan"])).any(axis=1).all()
    assert np.isfinite(me.floats(d["ordinary"])).all()


def test_vector_families_are_what_they_claim():
    v = me.vector_families()
    assert (v["zero"] & 0x7fffffff).max() == 0 and len({tuple(r) for r in v["zero"].tolist()}) == 16
    l2 = np.array([l2_chain(r) for r in v["l2_straddles_flt_min"]])
    below = l2 < me.FLT_MIN
    assert below.sum() >= 100 and (~below).sum() >= 100 and (l2 > 0).all()
    assert (np.abs(l2 / me.FLT_MIN - 1.0) < 1e-5).sum() >= 100, "within ulps of FLT_MIN"
    dominant = v["l2_straddles_flt_min"][384:]
    x = np.abs(me.floats(dominant).astype(f64))
    assert (np.sort(x, axis=1)[:, 2] <= np.sort(x, axis=1)[:, 3] * 2.0 ** -5).all(), "one component dominating"
    assert all(l2_chain(r) < me.FLT_MIN for r in v["l2_below_flt_min"])
    assert all(l2_chain(r) < me.FLT_MIN for r in v["all_denormal"])
    assert ((v["all_denormal"] >> 23) & 0xff).max() == 0 and (v["all_denormal"] & 0x7fffff).any(axis=1).all()
    for name in ("l2_overflows_components_finite", "l2_overflows_one_component"):
        x = me.floats(v[name])
        assert np.isfinite(x).all()
        assert all(l2_chain(r) == INF for r in v[name]), name
        assert all(math.isfinite(l2_chain(me.bits(me.floats(r) * f32(2.0 ** -66)))) for r in v[name]), "the 2^-66 rescale brings l2 back"
    assert np.abs(me.floats(v["l2_overflows_components_finite"])).min(axis=1).max() >= 2.0 ** 127 and (
        np.abs(me.floats(v["l2_overflows_components_finite"])[6:]).min() >= 2.0 ** 63.49)
    l2 = np.array([l2_chain(r) for r in v["l2_straddles_overflow"]])
    assert (l2 == INF).sum() >= 20 and (l2 < INF).sum() >= 20
    x = me.floats(v["infinite_components"])
    assert np.isinf(x).any(axis=1).all() and not np.isnan(x).any()
    assert {int(c) for c in np.isinf(x).sum(axis=1)} == {1, 2, 3, 4}
    assert all(l2_chain(me.bits(r * f32(2.0 ** -66))) == INF for r in x), "l2 still overflows after the rescale"
    assert np.isnan(me.floats(v["nan_component"])).any(axis=1).all()
    assert np.isfinite(me.floats(v["ordinary"])).all()
    p = me.pair_families()["difference_cancels"]
    with np.errstate(all="ignore"):
        diff = me.floats(p[:, :4]) - me.floats(p[:, 4:])
    assert (np.abs(diff) < 2.0 ** -120).all() and (diff == 0).all(axis=1).sum() >= 256 and (diff != 0).any(axis=1).sum() >= 200
    assert all(l2_chain(me.bits(r)) < me.FLT_MIN for r in diff)


@pytest.mark.parametrize("op", ["mad1", "mad2", "mad3", "mad1d"])
def test_contraction_family_separates_fused_from_unfused(op):
    """The fused_differs operands give different results with and without contraction, so a mad() of the wrong kind shows."""
    w = fam(op, "fused_differs")
    differ = 0
    if op == "mad1d":
        for a, b, c in w.view(f64).tolist():
            differ += float(Fraction(a) * Fraction(b) + Fraction(c)) != a * b + c
    else:
        for r in me.floats(w).astype(f64).tolist():
            a, b = r[0], r[1]
            if op == "mad1":
                fused, unfused = me.fma32(a, b, r[2]), float(f32(f32(a) * f32(b)) + f32(r[2]))
            else:
                cd = me.mul32(r[2], r[3])
                fused, unfused = me.fma32(a, b, cd), float(f32(f32(a) * f32(b)) + f32(cd))
                if op == "mad3":
                    fused, unfused = me.fma32(r[4], r[5], fused), float(f32(unfused) + f32(f32(r[4]) * f32(r[5])))
            differ += fused != unfused
    assert differ >= 0.95 * w.shape[0], "%d of %d differ" % (differ, w.shape[0])


def test_exact_helpers():
    rng = np.random.default_rng(7)
    x = rng.normal(0, 1, 2000) * 2.0 ** rng.integers(-160, 130, 2000)
    with np.errstate(over="ignore"):
        assert [me.round_f32(Fraction(v)) for v in x.tolist()] == x.astype(f32).astype(f64).tolist()
    assert me.round_f32(Fraction(2) ** 128 - Fraction(2) ** 103) == INF and me.round_f32(Fraction(2) ** 128 - Fraction(2) ** 103 - 1) < INF
    assert me.fma32(3.0, 5.0, -15.0) == 0.0 and math.copysign(1.0, me.fma32(-0.0, 1.0, -0.0)) == -1.0
    s, c = me.sincos_reference(float(f32(2.0 ** 127)))
    assert abs(s - 0.6233855129558702) < 1e-15 and abs(c - 0.78191463871496) < 1e-15     # (sin, cos)(2^127) to 16 digits
    s, c = me.sincos_reference(float(f32(math.pi)))
    assert abs(s - -8.742278000372475e-08) < 1e-22 and abs(c - (-1.0 + s * s / 2)) < 2e-16


# ------------------------------------------------------------------------------------------------ the oracle's leaf functions
@pytest.mark.parametrize("op", ["dot4", "dot2", "cross"])
def test_oracle_dot_and_cross_are_the_exact_fma_chains(op):
    """dot = fma(w, w', fma(z, z', fma(y, y', x x'))), cross = fma(a, b, -(c d)) per component: every step rounded once, checked
    with exact rational arithmetic, bit for bit, on every family."""
    w, family, names = me.all_inputs(op)
    got = me.floats(po.leaf(op, w))
    k = w.shape[1] // 2
    x = me.floats(w).astype(f64)
    for i in range(w.shape[0]):
        a, b = x[i, :k].tolist(), x[i, k:].tolist()
        want = me.cross_exact_chain(a, b) if op == "cross" else [me.dot4_exact_chain(a, b)]
        assert same_bits_or_nan(got[i], want).all(), (op, names[family[i]], w[i], got[i], want)


def test_oracle_clamp01():
    w, family, names = me.all_inputs("clamp01")
    x = me.floats(w[:, 0]).astype(f64)
    got = me.floats(po.leaf("clamp01", w))[:, 0].astype(f64)
    nan = np.isnan(x)
    assert (got[~nan] == np.clip(x[~nan], 0.0, 1.0)).all()
    # (NaN through clamp is left out everywhere: OpenCL leaves it undefined, and C's fmax / fmin treat quiet and signalling NaNs
    # differently from library to library)
    assert nan.sum() <= 0.01 * x.size


def test_oracle_rsqrt_is_within_half_an_ulp():
    """r = rsqrt_portable(x) is checked through its residual: |r^2 x - 1| <= 2 (1/2 + 2^-29) 2^-23, i.e. r is within half a
    float32 ulp (plus the double rounding) of 1/sqrt(x); float64 holds r^2 x to 2^-52."""
    w, family, names = me.all_inputs("rsqrt")
    x = me.floats(w[:, 0]).astype(f64)
    r = me.floats(po.leaf("rsqrt", w))[:, 0].astype(f64)
    pos = np.isfinite(x) & (x > 0)
    assert pos.sum() > 1500
    bound = 2.0 * (0.5 + 2.0 ** -29) * 2.0 ** -24 * 2.0     # relative half-ulp is at most 2^-24 (r in [1, 2) 2^e) ... doubled for r^2
    assert (np.abs(r[pos] * r[pos] * x[pos] - 1.0) <= bound).all(), names
    assert np.isnan(r[(x < 0) | np.isnan(x)]).all()
    assert (r[x == 0] == np.where(np.signbit(x[x == 0]), -INF, INF)).all() and (r[x == INF] == 0).all()


@pytest.mark.parametrize("op", ["sin", "cos"])
def test_oracle_sin_cos_are_correctly_rounded_doubles(op):
    """sinf_portable / cosf_portable = (float) of the C library's double function: within half a float32 ulp (+ 2^-29 for the
    double's own error) of the true value, for every argument up to 2^127 -- the reference reduces the argument exactly."""
    w, family, names = me.all_inputs(op)
    x = me.floats(w[:, 0]).astype(f64)
    got = me.floats(po.leaf(op, w))[:, 0].astype(f64)
    fin = np.isfinite(x)
    assert np.isnan(got[~fin]).all()
    want = np.array([me.sincos_reference(v)[op == "cos"] for v in x[fin].tolist()])
    err = np.abs(got[fin] - want) / me.ulp32(want)
    worst = int(np.argmax(err))
    assert err.max() <= 0.5 + 2.0 ** -20, (err.max(), x[fin][worst], names[family[fin][worst]])
    zero = fin & (x == 0)
    assert (w[zero, 0] == po.leaf(op, w)[zero, 0]).all() if op == "sin" else (got[zero] == 1.0).all()


# normalize: the largest error of the oracle on the ordinary family, in units of 2^-24 (half an ulp of a unit vector's largest
# components), measured by test_oracle_normalize below: 1.41; the guard branches add two roundings: twice that for every family
NORMALIZE_ORDINARY_MAX_ERR = 1.41


def test_oracle_normalize():
    """normalize4 against the exact unit vector (float64: every float32 vector's squared length is a normal double).  Error: the
    largest component difference in units of 2^-24.  Measured on the ordinary family: 1.41 (asserted to be what this docstring
    says within 2 %, so that the tolerance stays a measured one); every finite non-zero vector of every family -- denormal, l2
    below FLT_MIN, l2 overflowing -- is within twice that.  Zero vectors come back as they went in; with infinite components the
    result is the unit vector over the infinite components' signs, the finite ones +-0; a NaN component makes all four NaN."""
    w, family, names = me.all_inputs("normalize")
    x = me.floats(w).astype(f64)
    got_bits = po.leaf("normalize", w)
    got = me.floats(got_bits).astype(f64)
    finite = np.isfinite(x).all(axis=1) & (x != 0).any(axis=1)
    exact = x[finite] / np.sqrt((x[finite] * x[finite]).sum(axis=1))[:, None]
    err = np.abs(got[finite] - exact).max(axis=1) / 2.0 ** -24
    ordinary = family[finite] == names.index("ordinary")
    measured = err[ordinary].max()
    assert abs(measured / NORMALIZE_ORDINARY_MAX_ERR - 1.0) <= 0.02, measured
    for i, name in enumerate(names):
        sel = family[finite] == i
        if sel.any():
            assert err[sel].max() <= 2.0 * NORMALIZE_ORDINARY_MAX_ERR, (name, err[sel].max())
    zero = (x == 0).all(axis=1)
    assert zero.sum() >= 16 and (got_bits[zero] == w[zero]).all()
    nan = np.isnan(x).any(axis=1)
    assert np.isnan(got[nan]).all()
    inf = np.isinf(x).any(axis=1) & ~nan
    assert inf.sum() >= 90
    want = np.where(np.isinf(x[inf]), 1.0, 0.0) / np.sqrt(np.isinf(x[inf]).sum(axis=1))[:, None]
    assert (np.abs(np.abs(got[inf]) - want) <= 2.0 ** -24).all() and (np.signbit(got[inf]) == np.signbit(x[inf])).all()
    assert (got[inf][~np.isinf(x[inf])] == 0).all()


def test_oracle_distance():
    """distance4 against float64 (exact differences, a normal double for every squared length).  Bound, from the operation's own
    roundings: each of four differences 1/2 ulp (1/2 ulp of the length at most), the fma chain of four non-negative terms 2 ulp of
    l2 (1 ulp of the length), the square root and the rescale 1/2 ulp each: 3 ulp, in float32 spacing at the exact value (the
    denormal spacing below FLT_MIN, where the 2^-86 rescale rounds)."""
    w, family, names = me.all_inputs("distance")
    x = me.floats(w).astype(f64)
    got = me.floats(po.leaf("distance", w))[:, 0].astype(f64)
    with np.errstate(all="ignore"):
        d32 = (me.floats(w[:, :4]) - me.floats(w[:, 4:])).astype(f64)          # the float32 differences decide overflow
        d = x[:, :4] - x[:, 4:]
        exact = np.sqrt((d * d).sum(axis=1))
    nan = np.isnan(d32).any(axis=1)
    assert np.isnan(got[nan]).all()
    inf = ~nan & np.isinf(d32).any(axis=1)
    assert (got[inf] == INF).all()
    fin = ~nan & ~inf
    over = fin & (exact >= 2.0 ** 128)
    assert (got[over] == INF).all()
    ok = fin & ~over
    err = np.abs(got[ok] - exact[ok]) / me.ulp32(exact[ok])
    worst = int(np.argmax(err))
    assert err.max() <= 3.0, (err.max(), names[family[ok][worst]], w[ok][worst])
    assert (got[fin & (exact == 0)] == 0).all()
