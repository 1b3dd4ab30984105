"""CPU test of the entry cut's interval test (lens_trace_amd/csrc/lt_entry_cut.hpp: light_box_pad, lane_set, may_reach), as the host
compiles it (lt_hip_entry_cut_test_host), against a float32 restatement of the reference's slab test in oracle/lt_oracle.c's form
(intersectBounds: the pairwise `>` compares, then tMax > 0; NaN compares false).

The claim in front of the header: a shadow ray from a lane's origin towards a point of the light box that passes the slab test of a
box B passes the interval test of every box A that encloses B.  Here: 1.2 million cases -- random boxes and origins over six
decades of scale, light boxes, targets inside the light box (half of them aimed through B, so that the slab test passes often),
nested ancestors -- plus the enumerated edge classes: the origin on a face of B or of A, a direction component of exactly 0, an
infinite inverse (a component that underflows in the normalisation), subnormal extents and coordinates, flat boxes, the light box
touching, overlapping or inside the node, the origin inside the light box.  The direction is normalised three ways (the scale one
float, then two and four ulps off: the math flavours' rsqrt).  Every case whose slab test of B passes must not be excluded for A:
none is left out -- a lane that lane_set refuses (status 2) starts at the root, which is no exclusion either."""
import ctypes

import numpy as np

from lens_trace_amd import _capi as C

F = np.float32
N = 200_000          # per class


def interval_test(o, L, box):
    lib = C.load()
    n = o.shape[0]
    out = np.zeros(n, np.uint8)
    o, L, box = (np.ascontiguousarray(a, F) for a in (o, L, box))
    rc = lib.lt_hip_entry_cut_test_host(o.ctypes.data_as(ctypes.c_void_p), L.ctypes.data_as(ctypes.c_void_p), box.ctypes.data_as(ctypes.c_void_p),
                                        n, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def normalize(p, ulps):
    """normalize4 (lt_device.hpp) on xyz with w = 0: the zero vector as it is, p rescaled where p . p leaves the normal range, then
    every component times ONE float -- 1 / sqrt(p . p) moved by `ulps`."""
    p = p.copy()
    l2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    small = l2 < F(1.17549435e-38)
    p[small] = p[small] * F(2.0 ** 86)
    big = np.isinf(l2)
    p[big] = p[big] * F(2.0 ** -66)
    l2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    s = F(1) / np.sqrt(l2)
    for _ in range(abs(ulps)):
        s = np.nextafter(s, F(np.inf) if ulps > 0 else F(0))
    d = p * s[:, None]
    zero = (p == 0).all(axis=1)
    d[zero] = 0
    return d


def slab(o, inv, lo, hi):
    """oracle/lt_oracle.c: intersectBounds."""
    neg = inv < 0
    near = np.where(neg, hi, lo)
    far = np.where(neg, lo, hi)
    tn = (near - o) * inv
    tf = (far - o) * inv
    tMin, tMax = tn[:, 0].copy(), tf[:, 0].copy()
    ok = ~((tMin > tf[:, 1]) | (tn[:, 1] > tMax))
    tMin = np.where(tn[:, 1] > tMin, tn[:, 1], tMin)
    tMax = np.where(tf[:, 1] < tMax, tf[:, 1], tMax)
    ok &= ~((tMin > tf[:, 2]) | (tn[:, 2] > tMax))
    tMax = np.where(tf[:, 2] < tMax, tf[:, 2], tMax)
    return ok & (tMax > 0)


def base_cases(rng, n):
    scale = (10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F)
    c = (rng.normal(0, 1, (n, 3)) * scale).astype(F)
    h = (np.abs(rng.normal(0, 0.3, (n, 3))) * scale * (rng.random((n, 3)) > 0.15)).astype(F)     # (some extents exactly 0: flat boxes)
    blo, bhi = c - h, c + h
    grow = (np.abs(rng.normal(0, 1, (n, 2, 3))) * scale[:, None] * (rng.random((n, 2, 3)) > 0.3)).astype(F)
    alo, ahi = np.minimum(blo - grow[:, 0], blo), np.maximum(bhi + grow[:, 1], bhi)
    o = (c + rng.normal(0, 3, (n, 3)) * scale).astype(F)
    inside = rng.random(n) < 0.1
    o[inside] = (blo + (bhi - blo) * rng.random((n, 3)).astype(F))[inside]
    lc = (c + rng.normal(0, 5, (n, 3)) * scale).astype(F)
    lh = (np.abs(rng.normal(0, 1, (n, 3))) * scale * (rng.random((n, 3)) > 0.2)).astype(F)
    # half of the cases: the light lies beyond a point of B as seen from the origin
    aim = rng.random(n) < 0.5
    q = blo + (bhi - blo) * rng.random((n, 3)).astype(F)
    k = (1.0 + 10.0 ** rng.uniform(-2, 1, (n, 1))).astype(F)
    lc[aim] = (o + (q - o) * k)[aim]
    llo, lhi = lc - lh, lc + lh
    t = rng.random((n, 3)).astype(F)
    t[rng.random((n, 3)) < 0.1] = 0
    t[rng.random((n, 3)) < 0.1] = 1
    l = np.clip(llo + (lhi - llo) * t, llo, lhi)
    centre = aim & (rng.random(n) < 0.7)
    l[centre] = lc[centre]
    return dict(o=o, blo=blo, bhi=bhi, alo=alo, ahi=ahi, llo=llo, lhi=lhi, l=l)


def widen_light(k):
    k["llo"] = np.minimum(k["llo"], k["l"])
    k["lhi"] = np.maximum(k["lhi"], k["l"])


def edge_origin_on_face(rng, n):
    k = base_cases(rng, n)
    a = rng.integers(0, 3, n)
    which = rng.integers(0, 4, n)
    face = np.stack([k["blo"], k["bhi"], k["alo"], k["ahi"]])[which, np.arange(n)]
    k["o"][np.arange(n), a] = face[np.arange(n), a]
    both = rng.random(n) < 0.3     # ... on an edge or a corner
    a2 = (a + 1) % 3
    k["o"][both, a2[both]] = face[both, a2[both]]
    return k


def edge_zero_component(rng, n):
    k = base_cases(rng, n)
    a = rng.integers(0, 3, n)
    k["l"][np.arange(n), a] = k["o"][np.arange(n), a]
    two = rng.random(n) < 0.2
    a2 = (a + 1) % 3
    k["l"][two, a2[two]] = k["o"][two, a2[two]]
    three = rng.random(n) < 0.02
    k["l"][three] = k["o"][three]
    widen_light(k)
    return k


def edge_infinite_inverse(rng, n):
    """A component of l - o so small beside the others that its normalised value underflows to a subnormal or to 0."""
    k = base_cases(rng, n)
    a = rng.integers(0, 3, n)
    tiny = (10.0 ** rng.uniform(-45, -36, n)).astype(F) * rng.choice([-1, 1], n).astype(F)
    near0 = rng.random(n) < 0.7    # (o_a + tiny is o_a unless o_a is itself tiny)
    k["o"][near0, a[near0]] = (tiny * F(3))[near0]
    k["l"][np.arange(n), a] = k["o"][np.arange(n), a] + tiny
    step = ~near0
    k["l"][step, a[step]] = np.nextafter(k["o"][step, a[step]], F(np.inf) * np.sign(tiny[step]))
    widen_light(k)
    return k


def edge_subnormal(rng, n):
    k = base_cases(rng, n)
    a = rng.integers(0, 3, n)
    i = np.arange(n)
    sub = (rng.integers(1, 1 << 20, n).astype(np.uint32)).view(F)      # subnormal floats
    k["blo"][i, a] = k["blo"][i, a] * F(0) + sub * rng.choice([-1, 1], n).astype(F)
    k["bhi"][i, a] = k["blo"][i, a] + sub
    k["alo"][i, a] = np.minimum(k["alo"][i, a], k["blo"][i, a] - sub * (rng.random(n) < 0.5))
    k["ahi"][i, a] = np.maximum(k["ahi"][i, a], k["bhi"][i, a] + sub * (rng.random(n) < 0.5))
    near = rng.random(n) < 0.5
    k["o"][near, a[near]] = (sub * rng.integers(-3, 4, n).astype(F))[near]
    # (the box and the origin have moved: aim again, through the box as it is now)
    aim = rng.random(n) < 0.6
    q = k["blo"] + (k["bhi"] - k["blo"]) * rng.random((n, 3)).astype(F)
    far = (1.0 + 10.0 ** rng.uniform(-2, 1, (n, 1))).astype(F)
    k["l"][aim] = (k["o"] + (q - k["o"]) * far)[aim]
    widen_light(k)
    return k


def edge_light_touches(rng, n):
    k = base_cases(rng, n)
    a = rng.integers(0, 3, n)
    i = np.arange(n)
    how = rng.integers(0, 4, n)
    ext = k["lhi"][i, a] - k["llo"][i, a]
    m = how == 0      # the light box begins where A ends
    k["llo"][m, a[m]] = k["ahi"][m, a[m]]
    k["lhi"][m, a[m]] = k["ahi"][m, a[m]] + ext[m]
    m = how == 1      # ... ends where A begins
    k["lhi"][m, a[m]] = k["alo"][m, a[m]]
    k["llo"][m, a[m]] = k["alo"][m, a[m]] - ext[m]
    m = how == 2      # the light box inside B
    k["llo"][m] = k["blo"][m]
    k["lhi"][m] = k["bhi"][m]
    m = how == 3      # the origin inside the light box, the light box over A
    k["llo"][m] = np.minimum(k["alo"][m], k["o"][m])
    k["lhi"][m] = np.maximum(k["ahi"][m], k["o"][m])
    t = rng.random((n, 3)).astype(F)
    t[rng.random((n, 3)) < 0.2] = 0
    t[rng.random((n, 3)) < 0.2] = 1
    k["l"] = np.clip(k["llo"] + (k["lhi"] - k["llo"]) * t, k["llo"], k["lhi"])
    return k


CLASSES = [("random", base_cases), ("origin on a face", edge_origin_on_face), ("zero direction component", edge_zero_component),
           ("infinite inverse", edge_infinite_inverse), ("subnormal extents", edge_subnormal), ("light box touches the node", edge_light_touches)]


def test_interval_test_accepts_whatever_the_slab_test_accepts():
    total = passed = excluded_of_failing = failing = 0
    with np.errstate(all="ignore"):
        for ci, (name, make) in enumerate(CLASSES):
            rng = np.random.default_rng(1000 + ci)
            k = make(rng, N)
            assert (k["alo"] <= k["blo"]).all() and (k["bhi"] <= k["ahi"]).all() and (k["blo"] <= k["bhi"]).all()
            assert ((k["llo"] <= k["l"]) & (k["l"] <= k["lhi"])).all()
            o = k["o"]
            L = np.concatenate([k["llo"], k["lhi"]], axis=1)
            outer = interval_test(o, L, np.concatenate([k["alo"], k["ahi"]], axis=1))
            inner = interval_test(o, L, np.concatenate([k["blo"], k["bhi"]], axis=1))
            p = k["l"] - o
            hit_any = np.zeros(N, bool)
            for ulps in (0, 2, -4):
                d = normalize(p, ulps)
                inv = F(1) / d
                hit = slab(o, inv, k["blo"], k["bhi"])
                hit_any |= hit
                for what, res in (("the enclosing box", outer), ("the box itself", inner)):
                    bad = np.flatnonzero(hit & (res == 0))
                    assert bad.size == 0, "%s: %d of %d rays that pass the slab test of B are excluded for %s; first: o %r l %r B %r %r A %r %r L %r %r" % (
                        name, bad.size, int(hit.sum()), what, o[bad[0]], k["l"][bad[0]], k["blo"][bad[0]], k["bhi"][bad[0]], k["alo"][bad[0]], k["ahi"][bad[0]],
                        k["llo"][bad[0]], k["lhi"][bad[0]])
            total += N
            passed += int(hit_any.sum())
            failing += int((~hit_any).sum())
            excluded_of_failing += int((~hit_any & (outer == 0)).sum())
            assert hit_any.sum() > N // 20, (name, int(hit_any.sum()))     # the class is not vacuous
    assert total >= 1_000_000
    assert passed > 200_000
    # ... and the test is no constant: it excludes a good share of what the slab test of B rejects
    assert excluded_of_failing > failing // 10, (excluded_of_failing, failing)


def test_refused_lanes_and_nan_boxes_exclude_nothing():
    o = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [2.0 ** 41, 0, 0], [0, 0, 0], [0, 0, 0]], F)
    L = np.array([[5, 5, 5, 6, 6, 6]] * 4 + [[5, 5, 5, np.inf, 6, 6], [5, 5, 5, 6, 6, 6]], F)
    box = np.array([[-9, -9, -9, -8, -8, -8]] * 5 + [[np.nan, -9, -9, -8, -8, -8]], F)
    got = interval_test(o, L, box)
    assert list(got) == [0, 2, 2, 2, 2, 1] or list(got[:5]) == [0, 2, 2, 2, 2] and got[5] != 2
