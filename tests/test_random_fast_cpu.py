"""random()'s short sine (lt_device.hpp: random_fast_r) as the host compiles it -- lt_hip_random_fast_test_host, the kernels'
operation sequence -- against sin(r) * 43758.5453 in x87 extended precision (64-bit mantissa), over 2 * 10^7 arguments:

  grid      the (pixel, seed) arguments of a 3840 x 2160 film for seeds 0 .. 40, every fourth pixel each way, the argument formed
            as the portable flavour forms it (odd seeds) and as the as-shipped flavour does (even seeds);
  sweep     r over (-pi, pi) and the 10^4 doubles next to 0, +-pi/2 and +-pi;
  ties      r = asin(m / 43758.5453) for float midpoints m (mpmath), its +-3 neighbours, their negatives and reflections pi - r.

What is asserted (delta = 2^-46, the CLAIM in front of random_fast_r):
  * |p~ - truth| <= delta / 2 * |truth| everywhere (plus one subnormal double, 2^-1074, which no double product can do without);
  * where the flag says `determined`, the float is the float of BOTH ends of the truth widened by 2^-49 relative (4 ulp of a sine
    and the product's rounding: where the library's own product can lie);
  * the flag is clear for at most 4 * 2^-21 of the grid arguments (2^-21 = 2 delta 2^24, the derived rate) and is clear on ties;
  * three mutated copies are caught: a coefficient off by 2^-38 relative, delta = 0, pi_lo dropped.
"""
import ctypes
import struct

import numpy as np
import pytest

from lens_trace_amd import _capi

K = np.longdouble(43758.5453)          # (the double constant, widened)
DELTA = 2.0 ** -46
RATE = 2.0 ** -21
PARAMS = [float.fromhex(h) for h in (
    "-0x1.5555555555555p-3", "0x1.1111111111107p-7", "-0x1.a01a01a018aacp-13", "0x1.71de3a5456633p-19",
    "-0x1.ae6455a1cdfddp-26", "0x1.61240158708f1p-33", "-0x1.ae5137d193396p-41", "0x1.89a46890c7ff8p-49",
    "0x1.1a62633145c07p-53")] + [DELTA]
PI_HI = float.fromhex("0x1.921fb54442d18p+1")


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def fast(r=None, args3=None, flavour=0, params=None):
    lib = _capi.load()
    n = len(r) if r is not None else len(args3)
    r_out = np.empty(n, dtype=np.float64)
    p = np.empty(n, dtype=np.float64)
    det = np.empty(n, dtype=np.uint8)
    a = np.empty(n, dtype=np.float32)
    if r is not None:
        r = np.ascontiguousarray(r, dtype=np.float64)
    if args3 is not None:
        args3 = np.ascontiguousarray(args3, dtype=np.float32)
    par = np.asarray(params, dtype=np.float64) if params is not None else None
    rc = lib.lt_hip_random_fast_test_host(flavour, _ptr(args3), _ptr(r), ctypes.c_uint64(n), _ptr(par), _ptr(r_out), _ptr(p), _ptr(det), _ptr(a))
    assert rc == 0
    return r_out, p, det.astype(bool), a


def truth(r):
    assert np.finfo(np.longdouble).nmant >= 63, "needs x87 extended precision as the truth"
    return np.sin(r.astype(np.longdouble)) * K


def bound_violations(t, p):
    """lanes where |p~ - truth t| > delta / 2 |t| + 2^-1074; and the largest relative error among normal products"""
    err = np.abs(p.astype(np.longdouble) - t)
    bad = err > np.longdouble(DELTA / 2) * np.abs(t) + np.longdouble(2.0) ** -1074
    normal = np.abs(t) > np.longdouble(2.0) ** -1000
    worst = float(np.max(err[normal] / np.abs(t[normal]))) if normal.any() else 0.0
    return int(bad.sum()), worst


def determined_violations(t, det, a):
    """determined lanes whose float is not the float of both ends of truth t * (1 -+ 2^-49)"""
    t = t[det]
    w = np.longdouble(2.0) ** -49
    lo = (t * (1 - w)).astype(np.float32)
    hi = (t * (1 + w)).astype(np.float32)
    got = a[det]
    return int(((lo != got) | (hi != got)).sum())


def neighbours(x, k):
    """the k doubles on either side of each x, and x"""
    out = [x]
    up, dn = x, x
    for _ in range(k):
        up = np.nextafter(up, np.inf)
        dn = np.nextafter(dn, -np.inf)
        out += [up, dn]
    return np.concatenate(out)


@pytest.fixture(scope="module")
def sweep():
    rng = np.random.default_rng(20261021)
    dense = rng.uniform(-PI_HI, PI_HI, 1_500_000)
    dense = dense[np.abs(dense) < PI_HI]
    run = np.arange(1, 10001, dtype=np.float64)
    tiny = run * 5e-324                                                # the 10^4 doubles next to 0
    half = np.float64(PI_HI / 2) + (run - 5000) * 2.0 ** -52           # around pi/2, both sides
    top = np.float64(PI_HI) - run * 2.0 ** -51                         # the 10^4 doubles below pi
    edge = np.concatenate([tiny, half, top, [0.0], 2.0 ** -np.arange(1, 1070, dtype=np.float64)])
    return np.concatenate([dense, edge, -edge])


@pytest.fixture(scope="module")
def ties():
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.default_rng(7)
    f = np.concatenate([rng.uniform(0.001, 1.0, 600), rng.uniform(1.0, 100.0, 600), rng.uniform(100.0, 43758.0, 1800)]).astype(np.float32)
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2      # exact: 25 bits
    mid = mid[mid < 43758.5]
    kk = mpmath.mpf(struct.unpack("<d", struct.pack("<d", 43758.5453))[0])
    r0 = np.array([float(mpmath.asin(mpmath.mpf(m) / kk)) for m in mid])
    # (the reflection only where rounding pi - r to a double moves the product by less than 2^-50 of itself: tan r > 1/2)
    r1 = np.array([float(mpmath.pi - mpmath.asin(mpmath.mpf(m) / kk)) for m in mid[r0 > 0.5]])
    centre = np.concatenate([r0, r1])
    centre = centre[np.abs(centre) < PI_HI]
    return centre, np.concatenate([neighbours(centre, 3), -neighbours(centre, 3)])


def grid_args(seed):
    x = np.arange(0, 3840, 4, dtype=np.float32)
    y = np.arange(0, 2160, 4, dtype=np.float32)
    fx = x / np.float32(3840) - np.float32(0.5)
    fy = y / np.float32(2160) - np.float32(0.5)
    a = np.empty((len(y), len(x), 3), dtype=np.float32)
    a[..., 0] = fx[None, :]
    a[..., 1] = fy[:, None]
    a[..., 2] = np.float32(seed)
    return a.reshape(-1, 3)


def test_film_grid_bound_determined_lanes_and_fallback_rate():
    n = fallbacks = 0
    for seed in range(41):
        r, p, det, a = fast(args3=grid_args(seed), flavour=2 if seed % 2 == 0 else 0)
        assert np.all(np.abs(r) < PI_HI)
        t = truth(r)
        bad, worst = bound_violations(t, p)
        assert bad == 0, "seed %d: %d values off by more than delta / 2 (worst %.3g)" % (seed, bad, worst)
        assert determined_violations(t, det, a) == 0
        n += len(r)
        fallbacks += int((~det).sum())
    assert n >= 2 * 10 ** 7
    print("grid: %d arguments, %d not determined (derived rate: at most %.1f)" % (n, fallbacks, n * RATE))
    assert fallbacks <= 4 * RATE * n


def test_sweep_of_r_with_the_neighbours_of_zero_half_pi_and_pi(sweep):
    r, p, det, a = fast(r=sweep)
    t = truth(sweep)
    bad, worst = bound_violations(t, p)
    print("sweep: %d arguments, worst relative error %.3g = 2^%.2f, %d not determined" % (len(sweep), worst, np.log2(worst), int((~det).sum())))
    assert bad == 0
    assert worst <= DELTA / 2
    assert determined_violations(t, det, a) == 0
    assert det[sweep == 0.0].all()


def test_ties_are_not_determined(ties):
    centre, allr = ties
    r, p, det, a = fast(r=allr)
    t = truth(allr)
    bad, worst = bound_violations(t, p)
    assert bad == 0
    assert determined_violations(t, det, a) == 0
    _, _, det_c, _ = fast(r=centre)
    print("ties: %d arguments, %d not determined; of the %d nearest a tie %d" % (len(allr), int((~det).sum()), len(centre), int((~det_c).sum())))
    assert not det_c.any(), "a bracket of 2^-46 around a value within 2^-52 of a tie contains it"
    assert int((~det).sum()) > 0


def test_nan_and_infinity_are_not_determined():
    # (a reduced argument is finite or NaN: fmod of an infinity is NaN)
    _, p, det, _ = fast(r=np.array([np.nan, -np.nan]))
    assert not det.any()
    args = np.array([[0.1, 0.2, np.inf], [0.1, 0.2, -np.inf], [0.1, 0.2, np.nan], [np.inf, 0.2, 3.0], [np.nan, 0.2, 3.0]], dtype=np.float32)
    for flavour in (0, 1, 2):
        r, p, det, _ = fast(args3=args, flavour=flavour)
        assert np.isnan(r).all() and not det.any()


def test_mutated_copies_are_caught(sweep, ties):
    centre, allr = ties
    # the production parameters handed in as a mutant's would be: the same bits as the built-in ones
    r, p, det, a = fast(r=sweep)
    r2, p2, det2, a2 = fast(r=sweep, params=PARAMS)
    assert np.array_equal(p.view(np.uint64), p2.view(np.uint64)) and np.array_equal(det, det2) and np.array_equal(a.view(np.uint32), a2.view(np.uint32))
    ts, tt = truth(sweep), truth(allr)
    # (1) a coefficient off by 2^-38 relative: c1 and c2 (the terms m^5 / 120 and m^7 / 5040: 2^-41.6 and 2^-45.7 of the sine at
    # pi / 2) break the delta / 2 bound; from c3 on the term is below 2^-50 and stays inside it -- and inside delta's margin
    caught = []
    for k in range(1, 5):
        par = list(PARAMS)
        par[k] *= 1 + 2.0 ** -38
        _, pm, _, _ = fast(r=sweep, params=par)
        caught.append(bound_violations(ts, pm)[0] > 0)
    print("coefficient mutants c1 .. c4 caught by the bound:", caught)
    assert caught[0] and caught[1]
    # (2) delta = 0: every lane `determined`, ties among them, with a float the library need not return
    par = list(PARAMS)
    par[9] = 0.0
    _, _, dm, am = fast(r=allr, params=par)
    assert dm.all()
    assert determined_violations(tt, dm, am) > 0
    # (3) pi_lo dropped: the reflected argument is off by 1.2e-16 in absolute terms, everything near pi
    par = list(PARAMS)
    par[8] = 0.0
    _, pm, _, _ = fast(r=sweep, params=par)
    assert bound_violations(ts, pm)[0] > 0
