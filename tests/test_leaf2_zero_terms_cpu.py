"""The two-frame walk's leaf (lt_walk_asm.hpp: LT_ASM_TRI2_PART1 / _PART2; lt_device.hpp: leaf2_frame) leaves out four
instructions of the one-frame leaf, the ones that restate dot4's `a.w * b.w` term where that product is zero:

    det  = e1 . pvec    (+ 0)         tvec . pvec (+ 0)         d . qvec (+ 0 * dw)         e2 . qvec (+ 0)

This is a float32 model of everything the leaf does with those four numbers -- !(|det| < eps), 1 / det, u, v, u + v and t and their
compares -- run over every combination of sign, zero, subnormal, ordinary, huge, infinite and NaN values, with and without the four
terms.  The walk returns the accept and nothing else, so the accept is what must not change.  It does not, under the two facts the
walk's header states: eps > 0 (accumulator.cl's 1e-4) and dw = 0 * s, the w of normalize4's result (s = rsqrt(l2)), with a
direction consistent with that s.  It DOES change once eps is 0 or dw is any float a caller may supply, which is why the one-frame
walks -- kBasic's epsilon, lt_query.hip's caller-made rays, the closest-hit walk's u, v, t -- keep their terms."""
import itertools

import numpy as np

f32 = np.float32
EPS = np.array([0x38d1b718], dtype=np.uint32).view(np.float32)[0]      # the float `(double)fabs(det) < 1e-4` amounts to
TINY = f32(1.4e-45)
NAN, INF = f32(np.nan), f32(np.inf)


def both_signs(values):
    return np.array([s * v for v in values for s in (f32(1), f32(-1))], dtype=np.float32)


# zero, subnormal (smallest and ordinary), smallest normal, around eps, ordinary, huge, infinite; NaN
CLASSES = np.concatenate([both_signs([f32(0), TINY, f32(1e-40), f32(1.17549435e-38), np.nextafter(EPS, f32(0)), EPS, f32(0.25), f32(1), f32(3),
                                      f32(3e38), INF]), [NAN]]).astype(np.float32)
ZEROS = both_signs([f32(0)])
INF_OR_NAN = np.array([INF, -INF, NAN], dtype=np.float32)
TMAX = np.array([10.0, -0.005, 0.0, np.inf, np.nan], dtype=np.float32)    # distance - 0.01: positive, negative near the light, NaN
ALL_TERMS = (True, True, True, True)
NO_TERMS = (False, False, False, False)


def accept(det, tp, dq, eq, dw, tmax, eps, terms):
    """The leaf's accept for det = e1 . pvec, tp = tvec . pvec, dq = d . qvec, eq = e2 . qvec as the fma chains leave them; terms =
    which of the four `w` terms are added (det, tp, dq, eq).  (fma(0, dw, dq) = dq + 0 * dw exactly: the product is +-0 or NaN.)"""
    with np.errstate(all="ignore"):
        zero = f32(0)
        if terms[0]:
            det = det + zero
        if terms[1]:
            tp = tp + zero
        if terms[2]:
            dq = dq + zero * dw
        if terms[3]:
            eq = eq + zero
        ok = ~(np.abs(det) < eps)
        inv = f32(1) / det
        u = tp * inv
        ok &= ~(u < zero) & ~(u > f32(1))
        v = dq * inv
        ok &= ~(v < zero) & ~(u + v > f32(1))
        t = eq * inv
        return ok & (t < tmax)


def grid(det, tp, dq, eq, dw):
    return np.meshgrid(det, tp, dq, eq, dw, TMAX, indexing="ij")


# dw = 0 * s and what a direction d = s * (p.x, p.y, p.z) makes of det and d . qvec, per class of s
def rays_of_normalize4():
    with np.errstate(all="ignore"):
        zero = f32(0)
        return {
            # any finite s != 0: dw = +-0, nothing known about the other numbers
            "finite": grid(CLASSES, CLASSES, CLASSES, CLASSES, ZEROS),
            # s = 0: d = 0, so pvec = 0 and det, d . qvec are zeros
            "zero": grid(ZEROS, CLASSES, ZEROS, CLASSES, ZEROS),
            # s = inf: every component of d is +-inf or NaN, so are pvec's, det's and d . qvec's; dw = 0 * inf
            "inf": grid(INF_OR_NAN, CLASSES, INF_OR_NAN, CLASSES, np.array([zero * INF])),
            # s = NaN: d, pvec, det and d . qvec are NaN
            "nan": grid([NAN], CLASSES, [NAN], CLASSES, [NAN]),
        }


def test_the_four_terms_change_no_accept():
    """... together, each alone and in every combination: term by term, as the header argues it."""
    for s_class, g in rays_of_normalize4().items():
        want = accept(*g, EPS, ALL_TERMS)
        for terms in itertools.product((True, False), repeat=4):
            got = accept(*g, EPS, terms)
            assert np.array_equal(got, want), (s_class, terms, int((got != want).sum()))
    # (the enumeration is not vacuous: some combinations are accepted, most are not)
    g = rays_of_normalize4()["finite"]
    a = accept(*g, EPS, NO_TERMS)
    assert a.any() and not a.all()


def test_a_zero_eps_would_let_a_negative_zero_det_through():
    """eps = 0: det = -0 passes !(|det| < 0), 1 / det is -inf where 1 / (det + 0) is +inf, and t's sign turns."""
    g = rays_of_normalize4()["finite"]
    assert not np.array_equal(accept(*g, f32(0), ALL_TERMS), accept(*g, f32(0), NO_TERMS))
    one = [np.array([v], dtype=np.float32) for v in (-0.0, 0.0, 0.0, -1.0, 0.0, 10.0)]     # det, tp, dq, eq, dw, tmax
    assert accept(*one, f32(0), ALL_TERMS)[0] and not accept(*one, f32(0), NO_TERMS)[0]
    assert not accept(*one, EPS, ALL_TERMS)[0] and not accept(*one, EPS, NO_TERMS)[0]
    # ... and the term that matters there is det's
    assert not accept(*one, f32(0), (False, True, True, True))[0]


def test_a_callers_dw_would_change_v():
    """dw = inf or NaN beside a finite direction (lt_query.hip takes rays as they come): 0 * dw is NaN, v is NaN and passes both of
    its tests, where d . qvec alone gives a v < 0 that fails."""
    g = grid(CLASSES, CLASSES, CLASSES, CLASSES, np.array([INF, NAN, f32(1)]))
    assert not np.array_equal(accept(*g, EPS, ALL_TERMS), accept(*g, EPS, NO_TERMS))
    one = [np.array([v], dtype=np.float32) for v in (1.0, 0.25, -0.25, 1.0, np.inf, 10.0)]
    assert accept(*one, EPS, ALL_TERMS)[0] and not accept(*one, EPS, NO_TERMS)[0]
    # a finite dw of a caller's is harmless: 0 * dw = +-0
    g = grid(CLASSES, CLASSES, CLASSES, CLASSES, np.array([1.0, -3e38, 1e-40], dtype=np.float32))
    assert np.array_equal(accept(*g, EPS, ALL_TERMS), accept(*g, EPS, NO_TERMS))


def normalize4_w_scale(p):
    """normalize4's s = rsqrt(l2) for p = (x, y, z, 0) (lt_device.hpp; the portable rsqrt -- the device flavours' differs in the last
    bits of a finite, positive s only), or None where p is returned as it is."""
    with np.errstate(all="ignore"):
        p = np.asarray(p, dtype=np.float32)
        if not p.any() and not np.isnan(p).any():
            return None

        def dot(q):
            acc = q[0] * q[0]
            for c in q[1:]:
                acc = f32(np.float64(c) * np.float64(c) + np.float64(acc))     # fma
            return acc
        l2 = dot(p)
        if l2 < f32(1.17549435e-38):
            p = f32(2.0 ** 86) * p
            l2 = dot(p)
        elif l2 == INF:
            p = f32(2.0 ** -66) * p
            l2 = dot(p)
            if l2 == INF:
                p = np.copysign(np.isinf(p).astype(np.float32), p)
                l2 = dot(p)
        return f32(1.0 / np.sqrt(np.float64(l2)))


def test_normalize4_scales_by_a_finite_positive_number_or_nan():
    """What `dw = 0 * s` above rests on: s is finite and positive, or NaN (and then every component of the direction is NaN)."""
    edge = [0.0, -0.0, 1.4e-45, -1e-40, 1.17549435e-38, 1e-20, -1.0, 3.0, 1e19, -3e38, np.inf, -np.inf, np.nan]
    for x, y, z in itertools.product(edge, repeat=3):
        s = normalize4_w_scale([x, y, z, 0.0])
        if s is None:
            assert x == 0 and y == 0 and z == 0
        elif np.isnan([x, y, z]).any():
            assert np.isnan(s), (x, y, z, s)
        else:
            assert np.isfinite(s) and s > 0, (x, y, z, s)
