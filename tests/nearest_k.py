"""The k-nearest query (lt_hip_nearest_k) restated in numpy, on tests/nearest.py's arithmetic: what tests/test_nearest_k_cpu.py and
tests/test_gpu_nearest_k.py compare the host form and the kernel with.

* sequences(scene, points): brute force over every leaf of the caller's tree in float32 (nearest.tri, box_d2, candidate_d2), the
  accepted candidates (d2 < max_d2, the point walks at all: nearest.no_walk) in a stable sort by (d2, primitive offset, node
  index); a Sequences holds the first `keep` entries of every point and the length of the whole sequence.
* Sequences.records(k): the (n, k) HIT_DTYPE records of LT_NEAREST_FIRST_K, unused slots the miss record (max_d2's bits, -1, +0,
  +0); Sequences.count: LT_NEAREST_COUNT's words.
* families(scene, seed): nearest.families and one more, g_radius: points whose max_d2 is the d2 of one of their own entries (the
  strict `<` drops it and everything behind it) or the float above it.
* fan12(): twelve triangles round one vertex, which takes turns being A, B and C: the point at that vertex has twelve equal d2
  (+0), a tie wider than LT_NEAREST_MAX_K."""
from dataclasses import dataclass

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import HIT_DTYPE
from tests import nearest as nr

F32 = np.float32
KEEP = 13       # entries kept per point: LT_NEAREST_MAX_K, the one behind it (a tie across the list's end), the fan's twelve


@dataclass
class Sequences:
    points: np.ndarray     # (n, 4) float32
    d2: np.ndarray         # (n, keep) float32, inf behind the sequence's end
    prim: np.ndarray       # (n, keep) int64, -1 behind the end
    leaf: np.ndarray       # (n, keep) index into nearest.leaves(scene), -1 behind the end
    u: np.ndarray          # (n, keep) float32
    v: np.ndarray
    count: np.ndarray      # (n,) uint32: the length of the whole sequence
    ties: np.ndarray       # (n,) accepted candidates whose d2 equals the first entry's

    def records(self, k):
        """(n, k) HIT_DTYPE: LT_NEAREST_FIRST_K with max_k = k."""
        n = len(self.points)
        out = np.zeros((n, k), dtype=HIT_DTYPE)
        have = self.prim[:, :k] >= 0
        out["t"] = np.where(have, self.d2[:, :k], F32(0))
        out["prim"] = self.prim[:, :k]
        out["u"] = np.where(have, self.u[:, :k], F32(0))
        out["v"] = np.where(have, self.v[:, :k], F32(0))
        # an unused slot keeps max_d2's bits, a NaN's payload included
        bits = out["t"].view(np.uint32)
        bits[~have] = np.broadcast_to(self.points[:, 3].view(np.uint32)[:, None], (n, k))[~have]
        return out


def sequences(scene, points, keep=KEEP, chunk=256):
    pts = np.ascontiguousarray(points, dtype=F32).reshape(-1, 4)
    off, lo, hi = nr.leaves(scene)
    A, e1, e2 = nr.traversal_triangles(scene, off)
    n, L = len(pts), len(off)
    w = min(keep, L)
    s = Sequences(pts, np.full((n, keep), np.inf, dtype=F32), np.full((n, keep), -1, dtype=np.int64), np.full((n, keep), -1, dtype=np.int64),
                  np.zeros((n, keep), dtype=F32), np.zeros((n, keep), dtype=F32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int64))
    walk = ~nr.no_walk(pts)
    node = np.arange(L)
    for a in range(0, n, chunk):
        sel = slice(a, min(n, a + chunk))
        P = pts[sel, None, 0:3]
        t, u, v, _ = nr.tri(P, A[None], e1[None], e2[None])
        d2 = nr.candidate_d2(t, nr.box_d2(P, lo[None], hi[None])).astype(F32)
        with np.errstate(invalid="ignore"):
            ok = (d2 < pts[sel, 3:4]) & walk[sel, None]
        key = np.where(ok, d2, np.inf)
        shape = key.shape
        order = np.lexsort((np.broadcast_to(node, shape), np.broadcast_to(off, shape), key), axis=1)[:, :w]    # (stable; last key first)
        rows = np.arange(shape[0])[:, None]
        took = ok[rows, order]
        s.d2[sel, :w] = np.where(took, d2[rows, order], np.inf)
        s.prim[sel, :w] = np.where(took, off[order], -1)
        s.leaf[sel, :w] = np.where(took, order, -1)
        s.u[sel, :w] = np.where(took, u[rows, order], F32(0))
        s.v[sel, :w] = np.where(took, v[rows, order], F32(0))
        s.count[sel] = ok.sum(axis=1)
        s.ties[sel] = (ok & (d2 == key.min(axis=1, keepdims=True))).sum(axis=1)
    return s


def same(got, want):
    """Indices (flat, over every record) of the records that differ in any bit."""
    return nr.same(np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1))


def families(scene, seed=0, n=192):
    """nearest.families and g_radius: 2 n points of a_uniform and c_off whose max_d2 is the d2 of their own entry j (j drawn from
    0 .. 10: the sequence then ends in front of it, ties with it included) or, every other point, the float above that d2."""
    fam = nr.families(scene, seed, n)
    rng = np.random.default_rng(seed + 1000)
    base = np.concatenate([fam["a_uniform"], fam["c_off"]])
    base = base[rng.permutation(len(base))[: 2 * n]].copy()
    free = sequences(scene, base)
    j = rng.integers(0, 11, len(base))
    d = free.d2[np.arange(len(base)), j]
    with np.errstate(invalid="ignore", over="ignore"):
        d[1::2] = np.nextafter(d[1::2], F32(np.inf))
    base[:, 3] = d                  # (inf where the point has fewer entries: everything is accepted)
    fam["g_radius"] = base
    return fam


def fan12():
    """Twelve triangles (V, R_i, R_i+1) round V = (0.5, 0.25, 1), the ring R of radius about 1 rising and falling in z; triangle i
    lists its corners rotated by i, so V is positionA in triangles 0, 3, .., positionC in 1, 4, .., positionB in 2, 5, ...  Every
    coordinate is a multiple of 2^-6: B - A and C - A are exact."""
    V = np.array([0.5, 0.25, 1.0])
    ang = 2.0 * np.pi * np.arange(12) / 12.0
    ring = V + np.stack([np.cos(ang), np.sin(ang), 0.25 * np.cos(3.0 * ang)], axis=1)
    ring = np.round(ring * 64.0) / 64.0
    pos = np.zeros((12, 3, 3), dtype=F32)
    for i in range(12):
        corners = [V, ring[i], ring[(i + 1) % 12]]
        pos[i] = np.roll(np.array(corners), i % 3, axis=0)
    nrm = np.zeros_like(pos)
    nrm[..., 2] = 1.0
    mats = np.zeros(1, dtype=sc.MATERIAL_DTYPE)
    mats["diffuse"], mats["ior"], mats["dissolve"] = 0.5, 1.0, 1.0
    return sc.build_from_triangles(pos, nrm, np.zeros(12, dtype=np.int32), mats).validate()


FAN_VERTEX = F32([0.5, 0.25, 1.0])
