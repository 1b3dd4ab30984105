#!/usr/bin/env python3
"""A CPU model of the two-frame shadow walk (lt_walk_asm.hpp: LT_ASM_WALK2) on bench.py's wall, to see where its vector
instructions go: records per walk, VALU instructions per walk at interior and leaf records, and how often a frame's leaf test gets
past the u test (LT_ASM_TRI2_PART2) and to the late box test -- for the leaf that recomputes tvec / qvec / e2 . qvec per frame and
keeps dot4's four zero-valued terms ("before"), for the leaf as it is now, which computes tvec once per record and drops the terms
("after"), and for the form that was built and measured but not kept, qvec and e2 . qvec once per record as well ("all shared").

numpy only, nothing is read from the library: the wall's height field (lens_trace_amd/synth.py: heightfield_wall) under a
rectangle-halving hierarchy down to single triangles (not the library's tree: the same kind of tree), random 8x8 squares of the
bench camera, two frames of random light samples per lane, and the walk's own rules -- a child is pushed if any open lane of either
frame enters it, frame 1 is tested only where frame 0 misses, a leaf's test narrows test by test and exits early when no lane is
left.  Instruction counts are those of the macros (the as-shipped 1 / det).  It is reasoning about the kernel, not a measurement of
it; DESIGN.md 5.1 sets its output beside the measured counters.  Both say that about one of a leaf record's two frame tests gets
past u (the wall's triangles are small, 0.014 on a side, so |det| is near accumulator.cl's 1e-4 and the det test alone turns many
lanes away): computing qvec and e2 . qvec up front for both frames saves nothing, which is what decided against "all shared".

usage: python tests/tools/leaf2_cost_model.py [squares=40] [seed=7]"""
import sys

import numpy as np

CELLS, WIDTH, HEIGHT = 708, 3840, 2160
EPS = 1e-4

# VALU instructions of the macros (lt_walk_asm.hpp)
BOX_OCTANT, BOX_MIXED = 11, 13             # LT_ASM_BOXC / LT_ASM_BOXC_M, per child and frame
PUSH = 1                                   # v_writelane
IGNORE = 1
LATE_OCTANT, LATE_MIXED = 16 + 1, 18 + 1   # LT_ASM_BOXX_LATE / LT_ASM_BOXX_M_LATE and the t < tmax compare
FORMS = dict(
    before=dict(shared=0, part1=26, part2=19),         # LT_ASM_TRI_PART1 / PART2 per frame: tvec 3, qvec 6, e2 . qvec 3, four zero terms
    after=dict(shared=3, part1=21, part2=17),          # LT_ASM_TRI2_TVEC once per record, LT_ASM_TRI2_PART1 / PART2 per frame
    all_shared=dict(shared=12, part1=21, part2=8))     # (not kept) tvec, qvec, e2 . qvec once per record


def height(X, Y):
    return 0.35 * np.sin(1.7 * X) * np.sin(1.3 * Y) + 0.08 * np.sin(9.0 * X + 5.0 * Y) + 0.03 * np.sin(23.0 * X - 17.0 * Y)


class Wall:
    """Nodes are (i0, i1, j0, j1, t): a rectangle of cells (t = -1) or triangle t = 0 / 1 of a single cell."""

    def __init__(self, cells):
        self.cells = cells
        self.x = np.linspace(-5.0, 5.0, cells + 1)
        self.y = np.linspace(-2.5, 7.5, cells + 1)
        self.Z = height(*np.meshgrid(self.x, self.y))
        self.boxes = {}

    def root(self):
        return (0, self.cells, 0, self.cells, -1)

    def children(self, n):
        i0, i1, j0, j1, _ = n
        if i1 - i0 == 1 and j1 - j0 == 1:
            return (i0, i1, j0, j1, 0), (i0, i1, j0, j1, 1)
        if i1 - i0 >= j1 - j0:
            m = (i0 + i1) // 2
            return (i0, m, j0, j1, -1), (m, i1, j0, j1, -1)
        m = (j0 + j1) // 2
        return (i0, i1, j0, m, -1), (i0, i1, m, j1, -1)

    def triangle(self, n):
        i, _, j, _, t = n
        P = lambda a, b: np.array([self.x[a], self.y[b], self.Z[b, a]])
        return np.stack([P(i, j), P(i + 1, j), P(i + 1, j + 1)] if t == 0 else [P(i, j), P(i + 1, j + 1), P(i, j + 1)])

    def box(self, n):
        if n not in self.boxes:
            i0, i1, j0, j1, t = n
            if t < 0:
                z = self.Z[j0:j1 + 1, i0:i1 + 1]
                self.boxes[n] = (np.array([self.x[i0], self.y[j0], z.min()]), np.array([self.x[i1], self.y[j1], z.max()]))
            else:
                v = self.triangle(n)
                self.boxes[n] = (v.min(0), v.max(0))
        return self.boxes[n]


def slab(box, o, inv):
    t1, t2 = (box[0] - o) * inv, (box[1] - o) * inv
    return np.maximum(t1, t2).min(1) >= np.maximum(np.minimum(t1, t2).max(1), 1e-45)


def triangle_test(v, o, d, tmax):
    """(lanes past the det and u tests, lanes past the v and u + v tests, lanes with t < tmax among those)"""
    A, e1, e2 = v[0], v[1] - v[0], v[2] - v[0]
    p = np.cross(d, e2)
    det = p @ e1
    ok = np.abs(det) >= EPS
    inv = 1.0 / np.where(det == 0, 1.0, det)
    tv = o - A
    u = (tv * p).sum(1) * inv
    past_u = ok & (u >= 0) & (u <= 1)
    q = np.cross(tv, e1)
    vv = (d * q).sum(1) * inv
    past_v = past_u & (vv >= 0) & (u + vv <= 1)
    return past_u, past_v, past_v & ((q @ e2) * inv < tmax)


class Counts:
    def __init__(self):
        self.walks = self.interior = self.leaves = 0
        self.interior_valu = 0
        self.leaf_valu = dict((k, 0) for k in FORMS)
        self.frame_tests = self.part2 = self.late = 0
        self.both_open = self.part2_both = self.part2_any = 0
        self.rays = self.unoccluded = 0


def walk(wall, c, o, d, tmax, own):
    """One two-frame walk of 64 lanes: o [64,3], d[f] [64,3], tmax[f] [64]; own(n) = the lanes that start on triangle n."""
    inv = [1.0 / d[0], 1.0 / d[1]]
    sign = np.concatenate([d[0] < 0, d[1] < 0])
    mixed = bool((sign.any(0) & ~sign.all(0)).any())
    box_cost, late_cost = (BOX_MIXED, LATE_MIXED) if mixed else (BOX_OCTANT, LATE_OCTANT)
    live = [np.ones(64, bool), np.ones(64, bool)]
    stack = [wall.root()]
    while stack and (live[0].any() or live[1].any()):
        n = stack.pop()
        if n[4] < 0:
            c.interior += 1
            for child in wall.children(n):
                b = wall.box(child)
                hit0 = slab(b, o, inv[0]) & live[0]
                if live[0].any():
                    c.interior_valu += box_cost
                hit1 = np.zeros(64, bool)
                if live[1].any() and not hit0.any():
                    c.interior_valu += box_cost
                    hit1 = slab(b, o, inv[1]) & live[1]
                c.interior_valu += PUSH
                if hit0.any() or hit1.any():
                    stack.append(child)
            continue
        c.leaves += 1
        v = wall.triangle(n)
        reached2 = []
        cost = dict((k, m["shared"]) for k, m in FORMS.items())
        for f in (0, 1):
            if not live[f].any():
                continue
            c.frame_tests += 1
            lanes = live[f] & ~own(n)
            past_u, past_v, near = triangle_test(v, o, d[f], tmax[f])
            p2, p3 = bool((lanes & past_u).any()), bool((lanes & past_v).any())
            for k, m in FORMS.items():
                cost[k] += IGNORE + m["part1"] + (m["part2"] if p2 else 0) + (late_cost if p3 else 0)
            c.part2 += p2
            c.late += p3
            reached2.append(p2)
            live[f] = live[f] & ~(lanes & near & slab(wall.box(n), o, inv[f]))
        for k in cost:
            c.leaf_valu[k] += cost[k]
        if len(reached2) == 2:
            c.both_open += 1
            c.part2_both += reached2[0] and reached2[1]
            c.part2_any += reached2[0] or reached2[1]
    c.walks += 1
    c.rays += 128
    c.unoccluded += int(live[0].sum() + live[1].sum())


def light_points(rng):
    """64 points on the wall's light (two triangles of the quad x in [-1.5, 1.5], y = 9.5, z in [-9, -6])."""
    u, v = rng.random(64), rng.random(64)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u)[:, None], np.where(fold, 1 - v, v)[:, None]
    A, B, C, D = (np.array(p) for p in ([-1.5, 9.5, -9.0], [1.5, 9.5, -9.0], [1.5, 9.5, -6.0], [-1.5, 9.5, -6.0]))
    first = (rng.random(64) < 0.5)[:, None]
    return np.where(first, A + u * (B - A) + v * (C - A), A + u * (C - A) + v * (D - A))


def square(wall, c, rng):
    """One random 8x8 square of the bench camera at (0, 2.5, -50): its camera hits on the wall, then two groups of two frames."""
    sx, sy = rng.integers(0, WIDTH // 8), rng.integers(0, HEIGHT // 8)
    fx = (sx * 8 + np.tile(np.arange(8), 8)) / WIDTH - 0.5
    fy = (sy * 8 + np.repeat(np.arange(8), 8)) / HEIGHT - 0.5
    t = np.full(64, 10.0)              # film point (fx, 2.5 + fy, -50), direction (-fx, -fy, 5)
    for _ in range(30):
        wx, wy = fx - fx * t, 2.5 + fy - fy * t
        t = (height(wx, wy) + 50.0) / 5.0
    o = np.stack([wx, wy, height(wx, wy)], 1)
    ci = np.clip(((wx + 5.0) / 10.0 * wall.cells).astype(int), 0, wall.cells - 1)
    cj = np.clip(((wy + 2.5) / 10.0 * wall.cells).astype(int), 0, wall.cells - 1)
    lower = (wx - wall.x[ci]) / (wall.x[1] - wall.x[0]) >= (wy - wall.y[cj]) / (wall.y[1] - wall.y[0])

    def own(n):
        return (ci == n[0]) & (cj == n[2]) & (lower == (n[4] == 0))
    for _ in range(2):
        to = [light_points(rng) - o for _ in range(2)]
        length = [np.linalg.norm(v, axis=1) for v in to]
        walk(wall, c, o, [to[f] / length[f][:, None] for f in (0, 1)], [length[f] - 0.01 for f in (0, 1)], own)


def main():
    squares = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
    wall, c = Wall(CELLS), Counts()
    for _ in range(squares):
        square(wall, c, rng)
    w = float(c.walks)
    print("%d squares, %d two-frame walks; unoccluded rays %.1f %%" % (squares, c.walks, 100.0 * c.unoccluded / c.rays))
    print("records per walk: %.1f interior + %.1f leaf = %.1f" % (c.interior / w, c.leaves / w, (c.interior + c.leaves) / w))
    print("per-frame leaf tests: %.1f %% reach PART2 (past u), %.1f %% reach the late box test" % (
        100.0 * c.part2 / c.frame_tests, 100.0 * c.late / c.frame_tests))
    print("leaf visits: both frames open %.1f %%; of those, PART2 in both %.1f %%, in at least one %.1f %%" % (
        100.0 * c.both_open / c.leaves, 100.0 * c.part2_both / c.both_open, 100.0 * c.part2_any / c.both_open))
    for k in FORMS:
        leaf, total = c.leaf_valu[k] / w, (c.leaf_valu[k] + c.interior_valu) / w
        print("%-10s VALU per walk: interior %.0f + leaf %.0f = %.0f (leaf share %.1f %%); per leaf record %.1f" % (
            k, c.interior_valu / w, leaf, total, 100.0 * leaf / total, c.leaf_valu[k] / float(c.leaves)))
    for k in ("after", "all_shared"):
        print("%s / before: leaf %.3f, walk %.3f" % (k, c.leaf_valu[k] / float(c.leaf_valu["before"]),
                                                     (c.leaf_valu[k] + c.interior_valu) / float(c.leaf_valu["before"] + c.interior_valu)))


if __name__ == "__main__":
    main()
