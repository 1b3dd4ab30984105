"""The box-overlap query (lt_hip_overlap_boxes) restated in numpy, and its box batches: what tests/test_overlap_cpu.py and
tests/test_gpu_overlap.py compare the host form and the kernel with (the former also checks what this module claims).

* classes(lo, hi, A, e1, e2): the three classes of the 13-axis test -- box axes, plane, edge axes -- each on its own, in float32:
  every numpy operation is one IEEE operation rounded once, in the order of lens_trace_amd/csrc/lt_overlap.hpp.
* sequences(scene, boxes): brute force over every leaf of the caller's tree; a Sequences holds, for every box, the first KEEP
  entries of its sequence (ascending primitive offset, then node index), its length, and how many (box, leaf) pairs each class
  of axis separated alone.
* margins64(lo, hi, A, e1, e2): the same 13 axes in float64 on the same float32 inputs: per pair the largest gap / M over the
  axes (> 0: separated), M the sum of the magnitudes of the terms of that axis's expressions.
* slot_box(q, O, S): lt_overlap.hpp's put-back box of a quantised child slot, with tests/surface.py's exact fma32.
* families(scene, seed): the box batches, name -> (m, 8) float32 lt_hip_box records."""
from dataclasses import dataclass

import numpy as np

from lens_trace_amd.renderer import make_boxes
from tests import nearest as nr
from tests import query_edges as qe
from tests import surface as sf

F32 = np.float32
HALF = F32(0.5)
KEEP = 9        # entries kept per box: LT_OVERLAP_MAX_K and the one behind it
EDGE_AXES = ((2, 1), (0, 2), (1, 0))     # unit axis x, y, z: p = v[a] f[b] - v[b] f[a], r = h[a] |f[b]| + h[b] |f[a]|


# --------------------------------------------------------------------------------------------------------- the definition
def empty(boxes):
    """A bound that is not finite, or lo <= hi failing on an axis."""
    b = np.asarray(boxes, dtype=F32).reshape(-1, 8)
    lo, hi = b[:, 0:3], b[:, 4:7]
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1))


def boxes_meet(qlo, qhi, blo, bhi):
    with np.errstate(invalid="ignore"):
        return ((qlo <= bhi) & (blo <= qhi)).all(axis=-1)


def min3(a, b, c):
    m = np.where(b < a, b, a)
    return np.where(c < m, c, m)


def max3(a, b, c):
    m = np.where(b > a, b, a)
    return np.where(c > m, c, m)


def centre(lo, hi, A, e1, e2):
    c = HALF * lo + HALF * hi
    h = HALF * hi - HALF * lo
    v0 = A - c
    return h, v0, v0 + e1, v0 + e2


def classes(lo, hi, A, e1, e2):
    """Broadcastable float32 arrays [..., 3] -> (box axes separate, the plane separates, an edge axis separates)."""
    with np.errstate(all="ignore"):
        B, Cc = A + e1, A + e2
        box = ((min3(A, B, Cc) > hi) | (max3(A, B, Cc) < lo)).any(axis=-1)
        h, v0, v1, v2 = centre(lo, hi, A, e1, e2)
        n = [e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
             e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]]
        d = (n[0] * v0[..., 0] + n[1] * v0[..., 1]) + n[2] * v0[..., 2]
        r = (np.abs(n[0]) * h[..., 0] + np.abs(n[1]) * h[..., 1]) + np.abs(n[2]) * h[..., 2]
        assert d.dtype == F32 and r.dtype == F32
        plane = (d > r) | (d < -r)
        edge = np.zeros(plane.shape, dtype=bool)
        for f in (e1, e2 - e1, -e2):
            for a, b in EDGE_AXES:
                p = [v[..., a] * f[..., b] - v[..., b] * f[..., a] for v in (v0, v1, v2)]
                r = h[..., a] * np.abs(f[..., b]) + h[..., b] * np.abs(f[..., a])
                assert p[0].dtype == F32 and r.dtype == F32
                edge = edge | (min3(*p) > r) | (max3(*p) < -r)
    return box, plane, edge


def margins64(lo, hi, A, e1, e2):
    """The 13 axes in float64 on the same inputs: mu = the largest gap / M over the axes (an axis whose M is 0 -- a zero axis of a
    needle or a point triangle against a point box -- takes no part).  mu > 0: separated.  M: box axis k,
    |A| + |e1| + |e2| + |lo| + |hi| of that coordinate; plane, sum over i of (|e1_j e2_k| + |e1_k e2_j|) (|A_i| + |lo_i| + |hi_i|);
    edge axis (a, b), V_a F_b + V_b F_a with V = |A| + |lo| + |hi| + |e1| + |e2| and F = |e1| + |e2| per coordinate."""
    lo, hi, A, e1, e2 = (np.asarray(x, dtype=np.float64) for x in (lo, hi, A, e1, e2))
    gaps, Ms = [], []
    B, Cc = A + e1, A + e2
    mn, mx = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
    Mbox = np.abs(A) + np.abs(e1) + np.abs(e2) + np.abs(lo) + np.abs(hi)
    for k in range(3):
        gaps.append(np.maximum(mn[..., k] - hi[..., k], lo[..., k] - mx[..., k]))
        Ms.append(Mbox[..., k])
    c, h = 0.5 * lo + 0.5 * hi, 0.5 * hi - 0.5 * lo
    v0 = A - c
    v1, v2 = v0 + e1, v0 + e2
    n = np.cross(np.broadcast_to(e1, np.broadcast_shapes(e1.shape, e2.shape)), np.broadcast_to(e2, np.broadcast_shapes(e1.shape, e2.shape)))
    gaps.append(np.abs((n * v0).sum(axis=-1)) - (np.abs(n) * h).sum(axis=-1))
    N = [np.abs(e1[..., 1] * e2[..., 2]) + np.abs(e1[..., 2] * e2[..., 1]), np.abs(e1[..., 2] * e2[..., 0]) + np.abs(e1[..., 0] * e2[..., 2]),
         np.abs(e1[..., 0] * e2[..., 1]) + np.abs(e1[..., 1] * e2[..., 0])]
    W = np.abs(A) + np.abs(lo) + np.abs(hi)
    Ms.append(N[0] * W[..., 0] + N[1] * W[..., 1] + N[2] * W[..., 2])
    V = W + np.abs(e1) + np.abs(e2)
    Fm = np.abs(e1) + np.abs(e2)
    for f in (e1, e2 - e1, -e2):
        for a, b in EDGE_AXES:
            p = [v[..., a] * f[..., b] - v[..., b] * f[..., a] for v in (v0, v1, v2)]
            r = h[..., a] * np.abs(f[..., b]) + h[..., b] * np.abs(f[..., a])
            gaps.append(np.maximum(np.minimum(np.minimum(p[0], p[1]), p[2]) - r, -r - np.maximum(np.maximum(p[0], p[1]), p[2])))
            Ms.append(V[..., a] * Fm[..., b] + V[..., b] * Fm[..., a])
    shape = np.broadcast_shapes(*(g.shape for g in gaps))
    mu = np.full(shape, -np.inf)
    for g, M in zip(gaps, Ms):
        with np.errstate(all="ignore"):
            ratio = np.where(M > 0, g / M, -np.inf)
        mu = np.maximum(mu, np.where(np.isnan(ratio), -np.inf, ratio))
    return mu


def slot_box(q, O, S):
    """q [..., 6] grid coordinates (lo.xyz, hi.xyz), O and S [3]: fma(q, S, O) rounded once -> (lo [..., 3], hi [..., 3])."""
    q = np.asarray(q).astype(F32)
    lo = np.stack([sf.fma32(q[..., a], S[a], O[a]) for a in range(3)], axis=-1)
    hi = np.stack([sf.fma32(q[..., 3 + a], S[a], O[a]) for a in range(3)], axis=-1)
    return lo, hi


@dataclass
class Sequences:
    boxes: np.ndarray      # (n, 8) float32
    prim: np.ndarray       # (n, KEEP) int32, -1 behind the sequence's end
    count: np.ndarray      # (n,) uint32: the length of the whole sequence
    alone: np.ndarray      # (3,) pairs (non-empty box, leaf) that the box axes / the plane / the edge axes separated alone
    touch: np.ndarray      # (n, L) bool, over nearest.leaves(scene), when asked for

    def first(self, k):
        """(n, k) int32: LT_OVERLAP_FIRST_K with max_k = k."""
        return np.ascontiguousarray(self.prim[:, :k])

    @property
    def any(self):
        return (self.count != 0).astype(np.uint32)


def sequences(scene, boxes, keep=KEEP, chunk=128, want_touch=False):
    bx = np.ascontiguousarray(boxes, dtype=F32).reshape(-1, 8)
    off, llo, lhi = nr.leaves(scene)
    A, e1, e2 = nr.traversal_triangles(scene, off)
    n, L = len(bx), len(off)
    s = Sequences(bx, np.full((n, keep), -1, dtype=np.int32), np.zeros(n, dtype=np.uint32), np.zeros(3, dtype=np.int64),
                  np.zeros((n, L), dtype=bool) if want_touch else None)
    live = ~empty(bx)
    order = np.argsort(off, kind="stable")            # ascending offset, node index among equal offsets
    for a in range(0, n, chunk):
        sel = slice(a, min(n, a + chunk))
        lo, hi = bx[sel, None, 0:3], bx[sel, None, 4:7]
        box, plane, edge = classes(lo, hi, A[None], e1[None], e2[None])
        touch = boxes_meet(lo, hi, llo[None], lhi[None]) & ~(box | plane | edge) & live[sel, None]
        pairs = live[sel, None] & np.ones((1, L), dtype=bool)
        s.alone += [(pairs & box & ~plane & ~edge).sum(), (pairs & ~box & plane & ~edge).sum(), (pairs & ~box & ~plane & edge).sum()]
        s.count[sel] = touch.sum(axis=1)
        if want_touch:
            s.touch[sel] = touch
        ts = touch[:, order]
        for i in range(ts.shape[0]):
            got = off[order[np.flatnonzero(ts[i])[:keep]]]
            s.prim[a + i, :len(got)] = got
    return s


# --------------------------------------------------------------------------------------------------------- the box batches
def centred(c, half):
    c, half = np.asarray(c, dtype=np.float64), np.asarray(half, dtype=np.float64)
    return make_boxes(c - half, c + half)


def families(scene, seed=0, n=192):
    """name -> (m, 8) float32 records.  (a) uniform in the root box inflated 1.5 x, half-sizes 2^-1 .. 2^-10 of the scene;
    (b) centred on interior, edge and vertex points of triangles; (c) point boxes on vertex A of a primitive; (d) the eight cells
    of a regular grid round a vertex, whose faces pass through its coordinates bit for bit; (e) slabs, thin on one axis and
    spanning the scene; (f) boxes inside a triangle's bounding box, at one of its corners; (g) one box that holds the whole scene
    and one of +-2^100; (h) empty boxes: inverted, NaN, +-inf; (i) boxes off a triangle's plane by about their own size."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _families(scene, seed, n)


def _families(scene, seed, n):
    rng = np.random.default_rng(seed)
    lo, hi = nr.root_box(scene)
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    size = float(half.max())
    pv = scene.prim_view
    fam = {}
    k = rng.integers(1, 11, (n, 1))
    fam["a_uniform"] = centred(c + rng.uniform(-1.5, 1.5, (n, 3)) * half, size * 2.0 ** -k * rng.uniform(0.5, 1.0, (n, 3)))
    prims = rng.integers(0, scene.n_prims, n)
    on = np.concatenate([qe.points_on(scene, prims, rng, w) for w in ("interior", "edge", "vertex")])
    k = rng.integers(3, 17, (len(on), 1))
    fam["b_on"] = centred(on, size * 2.0 ** -k * rng.uniform(0.5, 1.0, (len(on), 3)))
    A = pv["positionA"][rng.integers(0, scene.n_prims, n)].astype(F32)
    fam["c_vertex_a"] = make_boxes(A, A)
    cells = []
    for _ in range(n // 8):
        V = pv[("positionA", "positionB", "positionC")[rng.integers(0, 3)]][rng.integers(0, scene.n_prims)].astype(F32)
        step = F32(size * 2.0 ** -float(rng.integers(2, 12)))
        below, above = (V - step).astype(F32), (V + step).astype(F32)
        for ix in range(8):
            pick = np.array([(ix >> a) & 1 for a in range(3)], dtype=bool)
            cells.append(np.concatenate([np.where(pick, V, below), [0], np.where(pick, above, V), [0]]))
    fam["d_grid"] = np.array(cells, dtype=F32)
    m = n // 2
    axis = rng.integers(0, 3, m)
    at = c + rng.uniform(-1.0, 1.0, (m, 3)) * half
    hs = np.tile(1.5 * half, (m, 1))
    hs[np.arange(m), axis] = size * 2.0 ** -rng.integers(5, 15, m)
    span = np.tile(c, (m, 1))
    span[np.arange(m), axis] = at[np.arange(m), axis]
    fam["e_slab"] = centred(span, hs)
    P = qe.corners(scene)[rng.integers(0, scene.n_prims, n)]
    tlo, thi = P.min(axis=1), P.max(axis=1)
    corner = np.where(rng.integers(0, 2, (n, 3)) == 0, tlo, thi)
    mid = 0.5 * (tlo + thi)
    fam["f_corner"] = centred(corner + (mid - corner) * rng.uniform(0.03, 0.2, (n, 1)), (thi - tlo) * rng.uniform(0.01, 0.1, (n, 1)))
    big = F32(2.0 ** 100)
    fam["g_whole"] = np.concatenate([make_boxes([lo - 0.01 * size], [hi + 0.01 * size]), make_boxes([[-big] * 3], [[big] * 3])])
    bad = fam["a_uniform"][:48].copy()
    vals = F32([np.nan, np.inf, -np.inf])
    for i in range(len(bad)):
        a = int(rng.integers(0, 3))
        if i % 4 == 3:
            bad[i, a], bad[i, 4 + a] = max(bad[i, a], bad[i, 4 + a]) + F32(size * 2.0 ** -6), min(bad[i, a], bad[i, 4 + a])     # inverted
        else:
            bad[i, a + 4 * int(rng.integers(0, 2))] = vals[i % 4]
    fam["h_empty"] = bad
    prims = rng.integers(0, scene.n_prims, n)
    d = size * 2.0 ** -rng.integers(3, 14, (n, 1)).astype(np.float64)
    inner = qe.points_on(scene, prims, rng, "interior")
    fam["i_off"] = centred(inner + nr.normals64(scene, prims) * d * rng.choice([-1.0, 1.0], (n, 1)), d * rng.uniform(0.3, 1.5, (n, 3)))
    return fam
