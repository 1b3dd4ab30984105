"""CPU test of the entry cut's triangle test (lens_trace_amd/csrc/lt_entry_cut.hpp: may_accept), as the host compiles it
(lt_hip_entry_cut_triangle_test_host), against a float32 restatement of the walks' leaf (LT_ASM_TRI2_*, leaf2_frame; the
reference's intersect_triangle_data) in each flavour's operation order:

  portable   every product and sum rounded on its own, 1 / det a division;
  shipped    the fma chains of the as-shipped build (a * b + c in float64, rounded once more to float32: within the claim's five
             roundings per product), 1 / det the division moved by up to two ulps (its rcp), u + v as a sum and as one more fma.

The claim in front of may_accept: a shadow ray from a lane's origin towards a point of the light box that passes the float triangle
test -- the 1e-4 gate on det, u and v in range, t below shade_lighting2's tmax; no test of t > 0, a triangle behind the origin
occludes -- is not excluded.  Here:
2.4 million cases in eight families (below), each with light points at the eight corners of the light box, at its centre and at
three random points inside, the direction normalised as tests/test_entry_cut_cpu.py does (the scale one float, two and four ulps
off).  Rays that traverse_shadow2 would not send through a packet walk (an inverse direction that is not finite or not below 2^60)
are not the claim's and are left out.  No accepted ray may belong to an excluded triangle.

Non-vacuity: the share of the neighbour family that is excluded is printed beside the share a float64 version with no margin
excludes, and asserted to be most of it.

Mutations tried on a copy of the header (check_all with the copy's host library; not part of the suite), 300 000 cases per family,
accepted rays of excluded triangles (the header as it is: 0):
  forward half-lines only (a triangle whose plane every line meets at t < 0 excluded):  1 196 604 -- behind the origin 347 740,
      origin on an edge 598 981, neighbours 71 262, coplanar fans 28 107, scaled 150 514;
  the margin dropped (G = 0, Z = 0):  178 378 -- origin on an edge 147 843 (u or v of exactly 0 in the walk, a rounding apart in the
      range), coplanar fans 7 655, neighbours 2 451, scaled 20 429;
  the light box halved about its centre:  75 741, in every family (the corner samples)."""
import ctypes

import numpy as np

from lens_trace_amd import _capi as C
from tests.test_entry_cut_cpu import normalize

F = np.float32
D = np.float64
N = 300_000          # per family
EPS = np.uint32(0x38d1b718).view(F)


def triangle_test(o, L, tri, lib=None):
    lib = lib or C.load()
    n = o.shape[0]
    out = np.zeros(n, np.uint8)
    o, L, tri = (np.ascontiguousarray(a, F) for a in (o, L, tri))
    rc = lib.lt_hip_entry_cut_triangle_test_host(o.ctypes.data_as(ctypes.c_void_p), L.ctypes.data_as(ctypes.c_void_p), tri.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.c_uint64(n), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


# ------------------------------------------------------------------------------------------- the walks' leaf, restated
def fma(a, b, c):
    return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)


def cross_plain(x, y):
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)


def cross_fma(x, y):   # v_mul x_c * -y_b, then v_fmac y_c * x_b
    return np.stack([fma(y[:, 2], x[:, 1], -(x[:, 2] * y[:, 1])), fma(y[:, 0], x[:, 2], -(x[:, 0] * y[:, 2])), fma(y[:, 1], x[:, 0], -(x[:, 1] * y[:, 0]))], axis=1)


def dot_plain(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def dot_fma(x, y):
    return fma(x[:, 2], y[:, 2], fma(x[:, 1], y[:, 1], x[:, 0] * y[:, 0]))


def ray_tmax(o, l, ulps):
    """shade_lighting2: (float)((double)distance4(position, lightPosition) - 0.01), the root moved by `ulps`."""
    e = o - l
    dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    for _ in range(abs(ulps)):
        dist = np.nextafter(dist, F(np.inf) if ulps > 0 else F(0))
    return (dist.astype(D) - 0.01).astype(F)


def leaf_accepts(o, d, tri, rcp_ulps, tmax):
    """Does the ray pass the float triangle test in some flavour?  (The gate, u, v, u + v and t < tmax: what the claim speaks of.)"""
    A, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    T = o - A
    any_ = np.zeros(o.shape[0], bool)
    for shipped in (False, True):
        cross, dot = (cross_fma, dot_fma) if shipped else (cross_plain, dot_plain)
        p = cross(d, e2)
        det = dot(e1, p)
        inv = F(1) / det
        if shipped:
            for _ in range(abs(rcp_ulps)):
                inv = np.nextafter(inv, F(np.inf) if rcp_ulps > 0 else F(-np.inf))
        un = dot(T, p)
        u = un * inv
        q = cross(T, e1)
        vn = dot(d, q)
        v = vn * inv
        t = dot(e2, q) * inv
        ok = ~(np.abs(det) < EPS) & ~(u < 0) & ~(u > 1) & ~(v < 0) & (t < tmax)
        sums = [u + v] + ([fma(vn, inv, u)] if shipped else [])
        for s in sums:
            any_ |= ok & ~(s > 1)
    return any_


def exact_excludes(o, llo, lhi, tri):
    """may_accept's corner test in float64 over the light box as it is, no margin: what could be excluded at all."""
    o, llo, lhi, tri = (a.astype(D) for a in (o, llo, lhi, tri))
    A, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    T = o - A
    wl, wh = llo - o, lhi - o

    def rng_(c):
        a, b = c * wl, c * wh
        return np.minimum(a, b).sum(axis=1), np.maximum(a, b).sum(axis=1)

    cD, cU, cV = np.cross(e2, e1), np.cross(e2, T), np.cross(T, e1)
    lo, hi = rng_(cD)
    s = np.where(lo > 0, 1.0, np.where(hi < 0, -1.0, 0.0))[:, None]
    cD, cU, cV = s * cD, s * cU, s * cV
    ex = rng_(cU)[1] < 0
    ex |= rng_(cV)[1] < 0
    ex |= rng_(cU - cD)[0] > 0
    ex |= rng_(cU + cV - cD)[0] > 0
    return ex & (s[:, 0] != 0)


# ------------------------------------------------------------------------------------------------------------- the families
def trav(v0, v1, v2):
    """The traversal triangle of a leaf record: v0, v1 - v0, v2 - v0 in floats."""
    v0, v1, v2 = (np.asarray(v, F) for v in (v0, v1, v2))
    return np.concatenate([v0, v1 - v0, v2 - v0], axis=1)


def rotate(rng, v0, v1, v2):
    k = rng.integers(0, 3, v0.shape[0])[:, None]
    a = np.where(k == 0, v0, np.where(k == 1, v1, v2))
    b = np.where(k == 0, v1, np.where(k == 1, v2, v0))
    c = np.where(k == 0, v2, np.where(k == 1, v0, v1))
    return a, b, c


def unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)


def own_triangles(rng, n):
    scale = 10.0 ** rng.uniform(-2, 2, (n, 1))
    c = rng.normal(0, 3, (n, 3)) * scale
    v = (c[:, None, :] + rng.normal(0, 0.3, (n, 3, 3)) * scale[:, None, :]).astype(F)
    return scale, v[:, 0], v[:, 1], v[:, 2]


def bary(v0, v1, v2, w):
    w = w.astype(F)
    return (v0 * w[:, 0:1] + v1 * w[:, 1:2]) + v2 * w[:, 2:3]      # bary3, the portable flavour


def light_for(rng, o, scale, towards):
    """A light box around o + dist * direction (direction near `towards`), sizes from a tenth to three times the scene's scale."""
    n = o.shape[0]
    direction = unit(unit(towards) + rng.normal(0, 0.6, (n, 3)))
    dist = scale * 10.0 ** rng.uniform(0, 2, (n, 1))
    lc = o + direction * dist
    lh = scale * 10.0 ** rng.uniform(-1, 0.5, (n, 3)) * (rng.random((n, 3)) > 0.15)     # (some extents exactly 0: a flat light)
    return (lc - lh).astype(F), (lc + lh).astype(F)


def fam_neighbours(rng, n):
    scale, v0, v1, v2 = own_triangles(rng, n)
    w = rng.dirichlet([1, 1, 1], n)
    near = rng.random(n) < 0.4          # close to the shared edge
    w[near, 0] *= 10.0 ** rng.uniform(-6, -1, near.sum())
    w /= w.sum(axis=1, keepdims=True)
    o = bary(v0, v1, v2, w)
    nrm = np.cross((v1 - v0).astype(D), (v2 - v0).astype(D))
    fold = rng.normal(0, 0.2, (n, 1)) * (rng.random((n, 1)) > 0.3)          # 0: the neighbour continues the plane
    v3 = ((v1.astype(D) + v2) - v0 + unit(nrm) * fold * scale + rng.normal(0, 0.05, (n, 3)) * scale * (fold != 0)).astype(F)
    vertex_only = rng.random(n) < 0.3   # shares v1 alone
    r = (rng.normal(0, 0.3, (n, 3)) * scale).astype(F)
    far2 = np.where(vertex_only[:, None], v1 + r, v2)
    a, b, c = rotate(rng, v1, v3, far2)
    llo, lhi = light_for(rng, o, scale, nrm * rng.choice([-1.0, 1.0], (n, 1), p=[0.1, 0.9]))
    return dict(o=o, llo=llo, lhi=lhi, tri=trav(a, b, c))


def fam_origin_on_edge(rng, n):
    scale, v0, v1, v2 = own_triangles(rng, n)
    t = rng.random((n, 1)).astype(F)
    t[rng.random(n) < 0.2] = 0
    t[rng.random(n) < 0.2] = 1
    t[rng.random(n) < 0.1] = 0.5
    o = v1 + (v2 - v1) * t              # on the edge v1 v2 (at a vertex where t is 0 or 1), as floats can be
    nrm = np.cross((v1 - v0).astype(D), (v2 - v0).astype(D))
    fold = rng.normal(0, 0.3, (n, 1)) * (rng.random((n, 1)) > 0.3)
    v3 = ((v1.astype(D) + v2) - v0 + unit(nrm) * fold * scale).astype(F)
    a, b, c = rotate(rng, v1, v3, v2)
    llo, lhi = light_for(rng, o, scale, nrm * rng.choice([-1.0, 1.0], (n, 1)))
    return dict(o=o, llo=llo, lhi=lhi, tri=trav(a, b, c))


def fam_coplanar_fans(rng, n):
    """A fan of six triangles around a centre in one plane -- an axis plane (exactly coplanar) or a tilted one (as coplanar as floats
    make it); the origin in the first triangle or on its spoke, the triangle under test another one of the fan."""
    scale = 10.0 ** rng.uniform(-2, 2, (n, 1))
    c = (rng.normal(0, 3, (n, 3)) * scale).astype(F)
    a = unit(rng.normal(0, 1, (n, 3)))
    b = unit(np.cross(a, rng.normal(0, 1, (n, 3))))
    axis = rng.random(n) < 0.5
    a[axis] = [1.0, 0.0, 0.0]
    b[axis] = [0.0, 0.0, 1.0]
    rad = scale * rng.uniform(0.1, 1.0, (n, 6))

    def spoke(k):
        ang = (k * (np.pi / 3))[:, None]
        return (c + (a * np.cos(ang) + b * np.sin(ang)) * np.take_along_axis(rad, (k % 6)[:, None], axis=1)).astype(F)

    zero = np.zeros(n, int)
    w = rng.dirichlet([1, 1, 1], n)
    on_spoke = rng.random(n) < 0.3
    w[on_spoke, 2] = 0
    w /= w.sum(axis=1, keepdims=True)
    o = bary(c, spoke(zero), spoke(zero + 1), w)
    k = rng.integers(1, 6, n)
    v0, v1, v2 = rotate(rng, c, spoke(k), spoke(k + 1))
    nrm = np.cross(a, b)
    llo, lhi = light_for(rng, o, scale, nrm * rng.choice([-1.0, 1.0], (n, 1)))
    return dict(o=o, llo=llo, lhi=lhi, tri=trav(v0, v1, v2))


def aimed(rng, n, place, sampled=False, dead_on=0.0):
    """A triangle placed on the line from the origin through a point of the light box (sampled: a corner or the centre, the points
    check_family looks from), at parameter `place` of the way (negative: behind the origin), jittered sideways by about the light's
    own spread there, of a size that makes hits common."""
    scale = 10.0 ** rng.uniform(-2, 2, (n, 1))
    o = (rng.normal(0, 3, (n, 3)) * scale).astype(F)
    llo, lhi = light_for(rng, o, scale, rng.normal(0, 1, (n, 3)))
    l = llo + (lhi - llo) * (rng.integers(0, 3, (n, 3)) * 0.5 if sampled else rng.random((n, 3)))
    f = place(rng, n)
    spread = np.abs(f) * (lhi - llo).astype(D).max(axis=1, keepdims=True) + 1e-3 * scale
    centre = o + (l - o) * f + rng.normal(0, 0.5, (n, 3)) * spread * (rng.random((n, 1)) >= dead_on)      # (dead_on: that share on the line itself)
    return scale, o, llo, lhi, centre, spread


def fam_behind(rng, n):
    scale, o, llo, lhi, centre, spread = aimed(rng, n, lambda rng, n: -(10.0 ** rng.uniform(-3, 0.5, (n, 1))))
    v = (centre[:, None, :] + rng.normal(0, 1.0, (n, 3, 3)) * spread[:, None, :]).astype(F)
    return dict(o=o, llo=llo, lhi=lhi, tri=trav(v[:, 0], v[:, 1], v[:, 2]))


def fam_far_small(rng, n):
    scale, o, llo, lhi, centre, spread = aimed(rng, n, lambda rng, n: rng.uniform(0.3, 1.5, (n, 1)), sampled=True, dead_on=0.5)
    size = scale * 10.0 ** rng.uniform(-4, -2, (n, 1))
    v = (centre[:, None, :] + rng.normal(0, 1.0, (n, 3, 3)) * size[:, None, :]).astype(F)
    return dict(o=o, llo=llo, lhi=lhi, tri=trav(v[:, 0], v[:, 1], v[:, 2]))


def fam_straddle(rng, n):
    """The light box straddles the triangle's plane: its centre lies in that plane, beside the triangle."""
    scale, v0, v1, v2 = own_triangles(rng, n)
    e1, e2 = (v1 - v0).astype(D), (v2 - v0).astype(D)
    nrm = unit(np.cross(e1, e2))
    st = rng.normal(0, 3, (n, 2))
    lc = v0 + e1 * st[:, 0:1] + e2 * st[:, 1:2]
    lh = scale * 10.0 ** rng.uniform(-1, 0.5, (n, 3))
    o = (v0 + e1 * rng.normal(0.3, 1, (n, 1)) + e2 * rng.normal(0.3, 1, (n, 1)) + nrm * scale * rng.normal(0, 0.3, (n, 1)) * (rng.random((n, 1)) > 0.2)).astype(F)
    a, b, c = rotate(rng, v0, v1, v2)
    return dict(o=o, llo=(lc - lh).astype(F), lhi=(lc + lh).astype(F), tri=trav(a, b, c))


def fam_at_the_light(rng, n):
    """The light's own two triangles (the light box is their vertex box), and copies of them moved towards the origin by nothing, by
    less than the shadow epsilon 0.01, by about it and by more: in an axis plane or tilted, seen from one to a hundred units away."""
    dist = 10.0 ** rng.uniform(0, 2, (n, 1))
    o = rng.normal(0, 3, (n, 3)).astype(F)
    away = unit(rng.normal(0, 1, (n, 3)))
    a = unit(np.cross(away, rng.normal(0, 1, (n, 3))))
    b = unit(np.cross(away, a))
    axis = rng.random(n) < 0.6          # the wall's and the Cornell box's lights: flat along one axis
    k = rng.integers(0, 3, n)
    for ax in range(3):
        m = axis & (k == ax)
        away[m], a[m], b[m] = np.roll([1.0, 0, 0], ax), np.roll([0, 1.0, 0], ax), np.roll([0, 0, 1.0], ax)
    away *= rng.choice([-1.0, 1.0], (n, 1))
    tilt = unit(away + rng.normal(0, 0.5, (n, 3)) * ~axis[:, None] + (a * rng.normal(0, 0.7, (n, 1)) + b * rng.normal(0, 0.7, (n, 1))))
    c = o + tilt * dist                 # the light's centre: seen at an angle, its plane's normal is `away`
    ha, hb = a * 10.0 ** rng.uniform(-1, 0.7, (n, 1)), b * 10.0 ** rng.uniform(-1, 0.7, (n, 1))
    q = [(c - ha - hb).astype(F), (c + ha - hb).astype(F), (c + ha + hb).astype(F), (c - ha + hb).astype(F)]
    llo, lhi = np.minimum.reduce(q), np.maximum.reduce(q)
    shift = rng.choice([0.0, 0.003, 0.009, 0.011, 0.02, 0.1, -0.05], (n, 1)) * rng.uniform(0.9, 1.1, (n, 1)) * -away
    second = rng.random(n)[:, None] < 0.5
    v0, v1, v2 = q[0], np.where(second, q[2], q[1]), np.where(second, q[3], q[2])
    v0, v1, v2 = ((v + shift).astype(F) for v in (v0, v1, v2))
    v0, v1, v2 = rotate(rng, v0, v1, v2)
    return dict(o=o, llo=llo, lhi=lhi, tri=trav(v0, v1, v2))


def fam_scaled(rng, n):
    """The families above with everything times 2^20 or 2^-20 (exact in floats)."""
    parts = []
    for i, make in enumerate((fam_neighbours, fam_behind, fam_far_small, fam_origin_on_edge)):
        k = make(rng, n // 4)
        s = F(2.0 ** 20) if i % 2 == 0 else F(2.0 ** -20)
        flip = rng.random(n // 4) < 0.5
        m = np.where(flip, s, F(1) / s).astype(F)[:, None]
        parts.append({key: val * m for key, val in k.items()})
    return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}


FAMILIES = [("neighbours", fam_neighbours), ("origin on an edge", fam_origin_on_edge), ("coplanar fans", fam_coplanar_fans),
            ("behind the origin", fam_behind), ("light box straddles the plane", fam_straddle), ("far small triangles", fam_far_small),
            ("at the light", fam_at_the_light), ("scaled by 2^+-20", fam_scaled)]
# Families whose triangles are put where the lines go, and the share of a case's count that the accepted rays must exceed.  (A far small
# triangle is met by one of its case's twelve light points at the most, in the half of the cases that lie on that line, and a line
# through a point near three random vertices passes between them about one time in four: one per cent, asked for by half.)
AIMED = {"behind the origin": 10, "light box straddles the plane": 10, "far small triangles": 200, "at the light": 10}


def light_points(rng, llo, lhi):
    n = llo.shape[0]
    for corner in range(8):
        yield np.where([(corner >> a) & 1 for a in range(3)], lhi, llo)
    yield np.clip(llo + (lhi - llo) * F(0.5), llo, lhi)
    for _ in range(3):
        yield np.clip(llo + (lhi - llo) * rng.random((n, 3)).astype(F), llo, lhi)


def check_family(name, k, rng, lib=None):
    """-> (cases, excluded, kept, not covered, accepted rays, accepted rays of excluded triangles, first such case or None)"""
    o, llo, lhi, tri = k["o"], k["llo"], k["lhi"], k["tri"]
    assert (llo <= lhi).all()
    status = triangle_test(o, np.concatenate([llo, lhi], axis=1), tri, lib)
    accepted = bad_total = 0
    first = None
    for i, l in enumerate(light_points(rng, llo, lhi)):
        d = normalize(l - o, (0, 2, -4)[i % 3])
        inv = F(1) / d
        sent = (np.isfinite(inv) & (np.abs(inv) < F(2.0 ** 60))).all(axis=1)       # packet_ray_ok
        acc = leaf_accepts(o, d, tri, (0, 2, -2)[(i // 3) % 3], ray_tmax(o, l, (0, 2, -2)[(i // 2) % 3])) & sent
        accepted += int(acc.sum())
        bad = np.flatnonzero(acc & (status == 0))
        bad_total += bad.size
        if bad.size and first is None:
            j = bad[0]
            first = "%s: o %r l %r L %r %r triangle %r" % (name, o[j], l[j], llo[j], lhi[j], tri[j])
    return o.shape[0], int((status == 0).sum()), int((status == 1).sum()), int((status == 2).sum()), accepted, bad_total, first


def check_all(lib=None, n=N, report=print):
    totals = {}
    with np.errstate(all="ignore"):
        for fi, (name, make) in enumerate(FAMILIES):
            rng = np.random.default_rng(2000 + fi)
            k = make(rng, n)
            res = check_family(name, k, rng, lib)
            exact = int(exact_excludes(k["o"], k["llo"], k["lhi"], k["tri"]).sum())
            report("%-30s %7d cases: excluded %7d (float64, no margin: %7d), kept %7d, not covered %d; accepted rays %8d, of excluded triangles %d" % (
                (name,) + res[:2] + (exact,) + res[2:6]))
            totals[name] = res + (exact,)
    return totals


def test_no_accepted_ray_of_an_excluded_triangle():
    totals = check_all()
    assert sum(t[0] for t in totals.values()) >= 2_000_000
    for name, t in totals.items():
        assert t[5] == 0, "%d accepted rays of excluded triangles; first: %s" % (t[5], t[6])
        assert t[4] > 0, name                                   # some ray is accepted in every family
        if name in AIMED:
            assert t[4] > t[0] // AIMED[name], (name, t[4])     # ... and many where the triangle was aimed at
        assert t[1] > 0, name
    # the neighbours: what the leaf pass is for.  Excluded by the float test with its margin: most of what no margin at all excludes.
    cases, excluded, _, _, _, _, _, exact = totals["neighbours"]
    print("neighbours: %.1f %% excluded, %.1f %% by the float64 test without a margin" % (100.0 * excluded / cases, 100.0 * exact / cases))
    assert excluded != 0
    assert excluded > 0.9 * exact, (excluded, exact)
    assert excluded > cases // 2, (excluded, cases)


def test_what_the_claim_does_not_cover_keeps_the_triangle():
    tri = np.array([[10, 0, 0, 0, 1, 0, 0, 0, 1]], F)
    o = np.array([[0, 0.1, 0.1]], F)
    L = np.array([[-6, 0, 0, -5, 0.2, 0.2]], F)                   # the light lies the other way: the line still meets the triangle
    assert list(triangle_test(o, L, tri)) == [1]
    assert list(triangle_test(o, np.array([[-6, 5, 5, -5, 5.2, 5.2]], F), tri)) == [0]
    cases = [
        (np.array([[np.nan, 0, 0]], F), L, tri, 2),
        (np.array([[2.0 ** 41, 0, 0]], F), L, tri, 2),
        (o, np.array([[-6, 0, 0, np.inf, 0.2, 0.2]], F), tri, 2),
        (o, np.array([[-6, 5, 5, -5, 5.2, 5.2]], F), np.array([[10, 0, 0, 0, np.nan, 0, 0, 0, 1]], F), 1),
        (o, np.array([[-6, 5, 5, -5, 5.2, 5.2]], F), np.array([[10, 0, 0, 0, np.inf, 0, 0, 0, 1]], F), 1),
        (o, np.array([[-6, 5, 5, -5, 5.2, 5.2]], F), np.array([[2.0 ** 41, 0, 0, 0, 1, 0, 0, 0, 1]], F), 1),
        (o, np.array([[-1, -1, -1, 1, 1, 1]], F), np.array([[10, 50, 50, 0, 1, 0, 0, 0, 1]], F), 1),      # the light box contains the origin
        (o, np.array([[-6, 5, 5, -5, 5.2, 5.2]], F), np.array([[10, 0, 0, 0, 0, 0, 0, 0, 1]], F), 1),   # a degenerate triangle: det is 0
    ]
    for oo, LL, tt, want in cases:
        assert list(triangle_test(oo, LL, tt)) == [want], (oo, LL, tt)
