#!/usr/bin/env python3
"""A CPU model of the entry cuts' leaf pass (lens_trace_amd/csrc/lt_entry_cut.hpp: may_accept; lt_entry_cut_kernel): how many 8x8
squares of bench.py's wall need no shadow walk at all, because no triangle of the wall meets the square's shaft -- the lines from its
64 camera hits towards any point of the light's box.  It is tests/tools/entry_cut_model.py's model (the same wall, camera, light,
rectangle-halving tree -- NOT the library's, and without the light's own two triangles, which the library's tree holds and the
header's `beyond the light` test removes) with
  * a depth-first pass from the root: a child where some lane may reach its box (entry_cut_model.may_reach), and at a leaf its own
    box, then
  * the corner test of the triangle, the lanes that start on it left out: with tvec = o - A the Moeller-Trumbore numerators
    det = w . (e2 x e1), U = w . (e2 x tvec), V = w . (tvec x e1) are linear in the direction w, so over the lane's direction box
    each keeps a sign iff it does at the 8 corners; where det has one sign s the lane cannot be accepted if, at every corner,
    s (U + delta det) < 0, or s (U - (1 + delta) det) > 0, or s (V + delta det) < 0, or s (U + V - (1 + delta) det) > 0 -- a
    barycentric margin delta, in doubles (the header derives its margin from the float operations instead; the table shows what a
    flat one costs).  No t anywhere: a triangle behind the origin counts.
For every delta it prints the squares in which no leaf survives ("proved clear") beside the squares that are truly clear in 16
frames of brute-force reference accepts (negative t allowed, the leaf's own slab test applied), whether a proved-clear square had
an occluded ray (it must not), and the box-reachable and surviving leaves of clear, unshadowed and shadowed squares.

usage: python tests/tools/clear_square_model.py [squares=40] [seed=23] [delta ...=1e-5 1e-3 1e-2]
DESIGN.md 5.1 has the table, beside the library's counters on the GPU."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entry_cut_model as ec   # noqa: E402
import leaf2_cost_model as m   # noqa: E402

CORNERS = np.array(list(itertools.product((0, 1), repeat=3)), bool)     # [8,3]


def may_accept(v, o, delta):
    """[64] bool: the lanes that some line of their shaft may be accepted on, triangle v [3,3]."""
    A, e1, e2 = v[0], v[1] - v[0], v[2] - v[0]
    T = o - A                                                            # [64,3]
    wl, wh = ec.LIGHT_LO - o, ec.LIGHT_HI - o
    w = np.where(CORNERS[None, :, :], wh[:, None, :], wl[:, None, :])    # [64,8,3]
    D = w @ np.cross(e2, e1)                                             # [64,8]
    U = np.einsum("lca,la->lc", w, np.cross(e2, T))
    V = np.einsum("lca,la->lc", w, np.cross(T, e1))
    pos, neg = (D > 0).all(1), (D < 0).all(1)
    s = np.where(pos, 1.0, -1.0)[:, None]
    out = ((s * (U + delta * D) < 0).all(1) | (s * (U - (1 + delta) * D) > 0).all(1) | (s * (V + delta * D) < 0).all(1) |
           (s * (U + V - (1 + delta) * D) > 0).all(1))
    return ~((pos | neg) & out)


def leaf_pass(wall, o, own, delta):
    """(box-reachable leaves, surviving leaves) of one square."""
    stack, reached, kept = [wall.root()], [], []
    while stack:
        n = stack.pop()
        if n[4] < 0:
            stack += [c for c in wall.children(n) if ec.may_reach(wall.box(c), o).any()]
            continue
        if not ec.may_reach(wall.box(n), o).any():
            continue
        reached.append(n)
        if (may_accept(wall.triangle(n), o, delta) & ~own(n)).any():
            kept.append(n)
    return reached, kept


def reference_accepts(wall, leaves, o, own, rng, frames=16):
    """Occluded rays among `frames` frames of the square, by brute force over `leaves` (every box-reachable leaf: by the entry cut's
    claim no other leaf accepts): the float test's rules, no t > 0, t < tmax, the leaf's own slab test."""
    occluded = 0
    for _ in range(frames):
        to = m.light_points(rng) - o
        length = np.linalg.norm(to, axis=1)
        d, tmax = to / length[:, None], length - 0.01
        hit = np.zeros(64, bool)
        for n in leaves:
            _, _, near = m.triangle_test(wall.triangle(n), o, d, tmax)
            hit |= near & ~own(n) & m.slab(wall.box(n), o, 1.0 / d)
        occluded += int(hit.sum())
    return occluded


def facet(wall, wx, wy):
    """(cell i, cell j, lower triangle?, z) of the wall's triangulated surface at (wx, wy) -- the origins must lie ON the triangles
    they start from, as the library's do; on the smooth height function they float a little over or under the facets and the
    neighbours of an origin's own triangle are met at small negative t."""
    ci = np.clip(((wx + 5.0) / 10.0 * wall.cells).astype(int), 0, wall.cells - 1)
    cj = np.clip(((wy + 2.5) / 10.0 * wall.cells).astype(int), 0, wall.cells - 1)
    a, b = (wx - wall.x[ci]) / (wall.x[1] - wall.x[0]), (wy - wall.y[cj]) / (wall.y[1] - wall.y[0])
    z00, z10, z11, z01 = wall.Z[cj, ci], wall.Z[cj, ci + 1], wall.Z[cj + 1, ci + 1], wall.Z[cj + 1, ci]
    lower = a >= b
    z = np.where(lower, z00 + a * (z10 - z00) + b * (z11 - z10), z00 + a * (z11 - z01) + b * (z01 - z00))
    return ci, cj, lower, z


def main():
    squares = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 23
    deltas = [float(a) for a in sys.argv[3:]] or [1e-5, 1e-3, 1e-2]
    wall = m.Wall(m.CELLS)
    rng = np.random.default_rng(seed)
    truly = 0
    proved = dict((d, 0) for d in deltas)
    wrong = dict((d, 0) for d in deltas)
    stats = dict(clear=[], unshadowed=[], shadowed=[])
    for _ in range(squares):
        sx, sy = rng.integers(0, m.WIDTH // 8), rng.integers(0, m.HEIGHT // 8)
        fx = (sx * 8 + np.tile(np.arange(8), 8)) / m.WIDTH - 0.5
        fy = (sy * 8 + np.repeat(np.arange(8), 8)) / m.HEIGHT - 0.5
        t = np.full(64, 10.0)
        for _ in range(30):
            wx, wy = fx - fx * t, 2.5 + fy - fy * t
            t = (facet(wall, wx, wy)[3] + 50.0) / 5.0
        ci, cj, lower, wz = facet(wall, wx, wy)
        o = np.stack([wx, wy, wz], 1)

        def own(n):
            return (ci == n[0]) & (cj == n[2]) & (lower == (n[4] == 0))
        kept = {}
        for d in deltas:
            reached, kept[d] = leaf_pass(wall, o, own, d)
        occluded = reference_accepts(wall, reached, o, own, rng)
        truly += occluded == 0
        for d in deltas:
            proved[d] += not kept[d]
            wrong[d] += (not kept[d]) and occluded != 0
        kind = "shadowed" if occluded else "clear" if not kept[deltas[0]] else "unshadowed"
        stats[kind].append((len(reached), len(kept[deltas[0]])))
    print("%d squares, seed %d: truly clear in 16 frames %d" % (squares, seed, truly))
    for d in deltas:
        print("  delta %-8g proved clear %3d   (proved clear with an occluded ray: %d)" % (d, proved[d], wrong[d]))
    for kind in ("clear", "unshadowed", "shadowed"):
        if stats[kind]:
            r, k = np.array(stats[kind]).T
            print("  %-10s squares %3d: box-reachable leaves %d..%d, surviving at delta %g %d..%d" % (kind, len(r), r.min(), r.max(), deltas[0], k.min(), k.max()))


if __name__ == "__main__":
    main()
