"""The nearest-point query restated in numpy, and its point batches: what the tests of lt_hip_nearest_points compare the kernel
and the host form with (tests/test_gpu_nearest.py, tests/test_nearest_cpu.py; the latter also checks what this module claims).

* expected(scene, points): brute force over every leaf of the caller's tree in float32 -- each numpy operation is one IEEE
  operation rounded once, in the order of lens_trace_amd/csrc/lt_nearest.hpp (tri, box_d2, candidate_d2), then the selection
  of include/lenstrace_hip.h: accepted iff d2 < max_d2, the smallest d2, the lowest primitive offset among equal d2; a miss is
  (max_d2's bits, -1, +0, +0).  details=True also returns what the non-vacuity checks count.
* distance64(P, A, e1, e2): the squared distance by another method in float64 -- the foot of the perpendicular where it lies
  inside, else the nearest of the three segments.
* slot_bound(q, O, S, P): lt_nearest.hpp's bound of a quantised child slot, with tests/surface.py's exact fma32.
* families(scene, seed): the point batches, name -> (n, 4) float32 lt_hip_point records.
* hand_made(), hand_made_overflow(): three-node trees -- a collinear needle and a point triangle; a needle whose edges overflow
  (its d2 is a NaN: never accepted) beside an ordinary triangle."""
import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import HIT_DTYPE, make_points
from tests import query_edges as qe
from tests import surface as sf

F32 = np.float32
ZERO, ONE = F32(0.0), F32(1.0)


# --------------------------------------------------------------------------------------------------------- the definition
def leaves(scene):
    """(primitive offsets [L], box lo [L, 3], box hi [L, 3]) of the caller's leaves, in node order."""
    nv = scene.node_view
    i = np.flatnonzero(nv["primitiveCount"] != 0)
    return nv["offset"][i].astype(np.int64), nv["boundsMin"][i].astype(F32), nv["boundsMax"][i].astype(F32)


def traversal_triangles(scene, off):
    """A, e1 = fl(B - A), e2 = fl(C - A) of the primitives `off`: the scene's structure kind 5."""
    pv = scene.prim_view
    A, B, Cc = (pv[k][off].astype(F32) for k in ("positionA", "positionB", "positionC"))
    with np.errstate(all="ignore"):
        return A, (B - A).astype(F32), (Cc - A).astype(F32)


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def unit_clamp(t):
    t = np.where(t > ZERO, t, ZERO)
    return np.where(t > ONE, ONE, t)


def residual2(ap, e1, e2, u, v):
    r = (ap - u[..., None] * e1) - v[..., None] * e2
    return (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]


def tri(P, A, e1, e2):
    """lt_nearest::tri on broadcastable float32 arrays [..., 3]: (d2, u, v, region)."""
    with np.errstate(all="ignore"):
        ap = P - A
        a, b, c = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2)
        d, e = dot3(e1, ap), dot3(e2, ap)
        qab = d / a
        tab, tac = unit_clamp(qab), unit_clamp(e / c)
        k = b / a
        g = e2 - k[..., None] * e1
        vf = dot3(ap, g) / dot3(g, g)
        uf = qab - vf * k
        f = e2 - e1
        bp = ap - e1
        tbc = unit_clamp(dot3(bp, f) / dot3(f, f))
        ubc = ONE - tbc
        zero = np.zeros_like(tab)

        def held(t):
            return np.where((t > ZERO) & (t < ONE), 1, 0)

        d2, u, v, region = residual2(ap, e1, e2, tab, zero), tab, zero, held(tab)
        for cd2, cu, cv, cr, ok in ((residual2(ap, e1, e2, zero, tac), zero, tac, held(tac), True),
                                    (residual2(ap, e1, e2, ubc, tbc), ubc, tbc, held(tbc), True),
                                    (residual2(ap, e1, e2, uf, vf), uf, vf, np.full(tab.shape, 2), (uf >= ZERO) & (vf >= ZERO) & (uf + vf <= ONE))):
            take = ok & (cd2 < d2)
            d2, u, v, region = np.where(take, cd2, d2), np.where(take, cu, u), np.where(take, cv, v), np.where(take, cr, region)
    assert d2.dtype == F32 and u.dtype == F32 and v.dtype == F32
    return d2, u, v, region


def box_d2(P, lo, hi):
    """lt_nearest::box_d2: per axis g = max(lo - p, p - hi, +0), a NaN bound taking no part."""
    with np.errstate(all="ignore"):
        below, above = lo - P, P - hi
        g = np.where(below > ZERO, below, ZERO)
        g = np.where(above > g, above, g).astype(F32)
        return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def candidate_d2(t, box):
    with np.errstate(invalid="ignore"):
        return np.where(t < box, box, t)


def slot_bound(q, O, S, P):
    """q [..., 6] grid coordinates (lo.xyz, hi.xyz), O and S [3], P [..., 3]: fma(q, S, O) rounded once, then box_d2."""
    q = np.asarray(q).astype(F32)
    lo = np.stack([sf.fma32(q[..., a], S[a], O[a]) for a in range(3)], axis=-1)
    hi = np.stack([sf.fma32(q[..., 3 + a], S[a], O[a]) for a in range(3)], axis=-1)
    return box_d2(P, lo, hi)


def no_walk(points):
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(points[:, 0:3]).all(axis=1) | ~(points[:, 3] > ZERO)


def expected(scene, points, details=False, chunk=256):
    """points: (n, 4) float32 lt_hip_point records.  Returns the HIT_DTYPE records of the definition; with details also a dict
    of per-point arrays: region (0 vertex, 1 edge, 2 face, -1 miss), tied (an accepted candidate of another primitive has the
    winner's d2 bits: the lower offset was reported), nan (candidates whose d2 is a NaN), cand (the winner's leaf, -1 on a
    miss), d2_inf (the smallest finite d2 whatever max_d2 says; inf where there is none)."""
    pts = np.ascontiguousarray(points, dtype=F32).reshape(-1, 4)
    off, lo, hi = leaves(scene)
    A, e1, e2 = traversal_triangles(scene, off)
    n = len(pts)
    out = np.zeros(n, dtype=HIT_DTYPE)
    out["t"], out["prim"] = pts[:, 3], -1
    info = {k: np.zeros(n, dtype=np.int64) for k in ("region", "tied", "nan", "cand")}
    info["region"][:] = -1
    info["cand"][:] = -1
    info["d2_inf"] = np.full(n, np.inf, dtype=F32)
    walk = ~no_walk(pts)
    for s in range(0, n, chunk):
        P = pts[s:s + chunk, None, 0:3]
        t, u, v, region = tri(P, A[None], e1[None], e2[None])
        d2 = candidate_d2(t, box_d2(P, lo[None], hi[None])).astype(F32)
        with np.errstate(invalid="ignore"):
            ok = (d2 < pts[s:s + chunk, 3:4]) & walk[s:s + chunk, None]
        key = np.where(ok, d2, np.inf)
        best = key.min(axis=1)
        tie = ok & (d2 == best[:, None])
        pick = np.where(tie, off[None], np.iinfo(np.int64).max).argmin(axis=1)
        hit = ok.any(axis=1)
        rows = np.arange(len(best))
        sel = slice(s, s + len(best))
        out["t"][sel] = np.where(hit, d2[rows, pick], pts[sel, 3])
        out["prim"][sel] = np.where(hit, off[pick], -1)
        out["u"][sel] = np.where(hit, u[rows, pick], ZERO)
        out["v"][sel] = np.where(hit, v[rows, pick], ZERO)
        info["region"][sel] = np.where(hit, region[rows, pick], -1)
        info["tied"][sel] = hit & ((tie & (off[None] != off[pick][:, None])).sum(axis=1) > 0)
        info["nan"][sel] = np.isnan(d2).sum(axis=1) * walk[sel]
        info["cand"][sel] = np.where(hit, pick, -1)
        info["d2_inf"][sel] = np.where(np.isfinite(d2), d2, np.inf).min(axis=1)
    # a miss keeps max_d2's bits, a NaN's payload included
    miss = out["prim"] < 0
    out["t"].view(np.uint32)[miss] = pts[miss, 3].view(np.uint32)
    return (out, info) if details else out


def same(got, want):
    """Indices of the records that differ in any bit."""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    return np.flatnonzero((g != w).any(axis=1))


# --------------------------------------------------------------------------------------------------------- float64, another way
def segment64(ap, e):
    den = (e * e).sum(axis=-1)
    with np.errstate(all="ignore"):
        t = np.clip(np.where(den > 0, (ap * e).sum(axis=-1) / den, 0.0), 0.0, 1.0)
    r = ap - t[..., None] * e
    return (r * r).sum(axis=-1)


def distance64(P, A, e1, e2):
    """Squared distance of P to the triangle A, A + e1, A + e2, all [n, 3], in float64: the foot of the perpendicular by the
    plane's normal where it lies inside the triangle, else the nearest of the three segments."""
    P, A, e1, e2 = (np.asarray(x, dtype=np.float64) for x in (P, A, e1, e2))
    ap = P - A
    nrm = np.cross(e1, e2)
    nn = (nrm * nrm).sum(axis=-1)
    with np.errstate(all="ignore"):
        h = (ap * nrm).sum(axis=-1) / nn
        foot = ap - h[..., None] * nrm
        # barycentrics of the foot by signed areas
        u = (np.cross(foot, e2) * nrm).sum(axis=-1) / nn
        v = (np.cross(e1, foot) * nrm).sum(axis=-1) / nn
        inside = (nn > 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        plane = h * h * nn
    edges = np.minimum(np.minimum(segment64(ap, e1), segment64(ap, e2)), segment64(ap - e1, e2 - e1))
    return np.where(inside, plane, edges)


# --------------------------------------------------------------------------------------------------------- the point batches
def root_box(scene):
    nv = scene.node_view
    return nv["boundsMin"][0].astype(np.float64), nv["boundsMax"][0].astype(np.float64)


def normals64(scene, prims):
    P = qe.corners(scene)[prims]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(ln > 0, nrm / ln, np.array([0.0, 0.0, 1.0]))


def three_node_tree(triangles):
    """Two triangles [2, 3, 3] under one root: leaf boxes are the triangles' own, one primitive per leaf."""
    T = np.asarray(triangles, dtype=F32)
    prims = np.zeros(2, dtype=sc.PRIM_DTYPE)
    for k, name in enumerate(("positionA", "positionB", "positionC")):
        prims[name] = T[:, k]
    for name in ("normalA", "normalB", "normalC"):
        prims[name] = (0, 0, 1)
    nodes = np.zeros(3, dtype=sc.NODE_DTYPE)
    nodes["boundsMin"][1:], nodes["boundsMax"][1:] = T.min(axis=1), T.max(axis=1)
    nodes["boundsMin"][0], nodes["boundsMax"][0] = T.min(axis=(0, 1)), T.max(axis=(0, 1))
    nodes["offset"] = (2, 0, 1)
    nodes["primitiveCount"] = (0, 1, 1)
    mats = np.zeros(1, dtype=sc.MATERIAL_DTYPE)
    mats["diffuse"], mats["ior"], mats["dissolve"] = 0.5, 1.0, 1.0
    return sc.Scene(nodes=nodes.view(np.uint8).reshape(-1).copy(), prims=prims.view(np.uint8).reshape(-1).copy(),
                    materials=mats.view(np.uint8).reshape(-1).copy(), lights=np.zeros(260, dtype=np.uint8)).validate()


def hand_made():
    return three_node_tree([[(0, 0, 0), (1, 1, 1), (2.5, 2.5, 2.5)], [(3, -1, 2), (3, -1, 2), (3, -1, 2)]])


def hand_made_overflow():
    return three_node_tree([[(-3e38, 0, 0), (3e38, 0, 0), (0, 0, 0)], [(1, 0, 0), (0, 2, 0), (0, 0, 3)]])


def families(scene, seed=0, n=192):
    """name -> (m, 4) float32 records.  (a) uniform in the root box inflated 1.5 x; (b) interior / edge / vertex points of
    triangles rounded to float32 (the bit-equal pairs among them: ties); (c) the same pushed off along the normal by 2^-k of the
    scene's size; (d) far points, 2^20 box sizes out, and beyond 2^64 (d2 overflows: a miss); (e) max_d2 of every kind, the
    model's own d2 (strict `<` loses it) and the float above it; (f) NaN and infinite components."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _families(scene, seed, n)


def _families(scene, seed, n):
    rng = np.random.default_rng(seed)
    lo, hi = root_box(scene)
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    size = float(half.max())
    fam = {}
    fam["a_uniform"] = make_points(c + rng.uniform(-1.5, 1.5, (n, 3)) * half)
    pairs = qe.bit_equal_pairs(scene)
    prims = rng.integers(0, scene.n_prims, n)
    if len(pairs):
        prims[: n // 3] = rng.choice(pairs, n // 3)
    on = np.concatenate([qe.points_on(scene, prims, rng, w) for w in ("interior", "edge", "vertex")])
    on_prims = np.tile(prims, 3)
    fam["b_on"] = make_points(on)
    k = rng.integers(0, 24, len(on))
    side = rng.choice([-1.0, 1.0], len(on))
    fam["c_off"] = make_points(on + normals64(scene, on_prims) * (side * size * 2.0 ** -k)[:, None])
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = c + d * size * 2.0 ** 20
    huge = d * 2.0 ** rng.uniform(64.5, 120, (n, 1))
    with np.errstate(over="ignore"):
        fam["d_far"] = make_points(np.concatenate([far[: n // 2], huge[: n // 2]]))
    base = np.concatenate([fam["a_uniform"], fam["c_off"]])[rng.permutation(n + len(on))[: 2 * n]]
    free = expected(scene, base)
    e = base.copy()
    third = len(e) // 3
    kinds = qe.TMAX_KINDS[rng.integers(0, len(qe.TMAX_KINDS), third)]
    rnd = rng.integers(0, 2, third) == 0                      # ... and fractions / multiples of the point's own d2
    with np.errstate(all="ignore"):
        kinds[rnd] = (free["t"][:third][rnd] * rng.choice(F32([0.25, 0.5, 2.0, 4.0]), rnd.sum())).astype(F32)
    e[:third, 3] = kinds
    e[third:2 * third, 3] = free["t"][third:2 * third]                                       # the model's own d2: `<` loses it
    e[2 * third:, 3] = np.nextafter(free["t"][2 * third:], F32(np.inf))                     # the float above: accepted
    fam["e_max_d2"] = e
    bad = fam["a_uniform"][: 48].copy()
    vals = F32([np.nan, np.inf, -np.inf])
    for i in range(len(bad)):
        bad[i, rng.integers(0, 3)] = vals[i % 3]
    bad[::4, 3] = F32(1.0)
    fam["f_nonfinite"] = bad
    return fam
