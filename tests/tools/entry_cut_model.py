#!/usr/bin/env python3
"""A CPU model of the entry cut (lens_trace_amd/csrc/lt_entry_cut.hpp): what a two-frame shadow walk of bench.py's wall saves when
it starts from a stored list of at most N nodes instead of the root.  It is tests/tools/leaf2_cost_model.py's model -- the same wall,
camera, light, rectangle-halving tree (NOT the library's) and walk rules, the "after" leaf form -- with
  * the interval test: a node's box against the half-lines from a square's 64 origins towards any point of the light's box, the
    axes treated independently (for each axis the interval of ray parameters for which some direction of the lane's direction
    interval lies inside the slab; excluded iff the largest lower bound exceeds the smallest upper bound), in doubles and without
    the header's outward margins;
  * the cut: the root expanded shallowest interior entry first, an entry replaced by those of its two children that some lane can
    reach, until a replacement would make the list longer than N;
  * the walk started with the list on its stack.
For every N it prints records per walk (interior + leaf), the walk's VALU instructions relative to the root start, whether any
node a root walk visits with a hit lies outside the list's subtrees (it must not), and the unoccluded share (it must not change).

usage: python tests/tools/entry_cut_model.py [squares=40] [seed=7] [N ...=4 8 16]
DESIGN.md 5.1 has the table for squares=40 and seeds 7 and 11, beside what the library's tree gave on the GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leaf2_cost_model as m   # noqa: E402

LIGHT_LO, LIGHT_HI = np.array([-1.5, 9.5, -9.0]), np.array([1.5, 9.5, -6.0])


def may_reach(box, o):
    """[64] bool: the lanes some half-line of which, from o towards a point of the light's box, meets the box."""
    lo, hi = box
    wl, wh = LIGHT_LO - o, LIGHT_HI - o                     # [64,3]
    below, above = o < lo, o > hi
    with np.errstate(divide="ignore", invalid="ignore"):
        enter = np.where(below, (lo - o) / np.where(wh > 0, wh, np.nan), np.where(above, (o - hi) / np.where(wl < 0, -wl, np.nan), 0.0))
        leave = np.where(wl > 0, (hi - o) / wl, np.where(wh < 0, (o - lo) / -wh, np.inf))
    dead = np.isnan(enter).any(1)                            # (below with no direction going up, above with none going down)
    return ~dead & ~(np.where(np.isnan(enter), 0.0, enter).max(1) > leave.min(1))


def entry_cut(wall, o, limit):
    cut = [(wall.root(), 0)]
    while True:
        interior = [i for i, (n, _) in enumerate(cut) if n[4] < 0]
        if not interior:
            break
        pick = min(interior, key=lambda i: cut[i][1])
        n, depth = cut[pick]
        kids = [(c, depth + 1) for c in wall.children(n) if may_reach(wall.box(c), o).any()]
        if len(cut) - 1 + len(kids) > limit:
            break
        cut = cut[:pick] + cut[pick + 1:] + kids
        if not cut:
            break
    return [n for n, _ in cut]


def walk(wall, c, o, d, tmax, own, start):
    """leaf2_cost_model.walk with the stack starting as `start`; returns the leaves at which some lane was stopped."""
    inv = [1.0 / d[0], 1.0 / d[1]]
    sign = np.concatenate([d[0] < 0, d[1] < 0])
    mixed = bool((sign.any(0) & ~sign.all(0)).any())
    box_cost, late_cost = (m.BOX_MIXED, m.LATE_MIXED) if mixed else (m.BOX_OCTANT, m.LATE_OCTANT)
    form = m.FORMS["after"]
    live = [np.ones(64, bool), np.ones(64, bool)]
    stack = list(start)
    stopped = []
    while stack and (live[0].any() or live[1].any()):
        n = stack.pop()
        if n[4] < 0:
            c.interior += 1
            for child in wall.children(n):
                b = wall.box(child)
                hit0 = m.slab(b, o, inv[0]) & live[0]
                if live[0].any():
                    c.interior_valu += box_cost
                hit1 = np.zeros(64, bool)
                if live[1].any() and not hit0.any():
                    c.interior_valu += box_cost
                    hit1 = m.slab(b, o, inv[1]) & live[1]
                c.interior_valu += m.PUSH
                if hit0.any() or hit1.any():
                    stack.append(child)
            continue
        c.leaves += 1
        v = wall.triangle(n)
        cost = form["shared"]
        for f in (0, 1):
            if not live[f].any():
                continue
            lanes = live[f] & ~own(n)
            past_u, past_v, near = m.triangle_test(v, o, d[f], tmax[f])
            cost += m.IGNORE + form["part1"] + (form["part2"] if (lanes & past_u).any() else 0) + (late_cost if (lanes & past_v).any() else 0)
            stop = lanes & near & m.slab(wall.box(n), o, inv[f])
            if stop.any():
                stopped.append(n)
            live[f] = live[f] & ~stop
        c.leaf_valu["after"] += cost
    c.walks += 1
    c.rays += 128
    c.unoccluded += int(live[0].sum() + live[1].sum())
    return stopped, [l.copy() for l in live]


def below(n, cut):
    return any(c[0] <= n[0] and n[1] <= c[1] and c[2] <= n[2] and n[3] <= c[3] and (c[4] < 0 or c[4] == n[4]) for c in cut)


def main():
    squares = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    limits = [int(a) for a in sys.argv[3:]] or [4, 8, 16]
    wall = m.Wall(m.CELLS)
    counts = dict((k, m.Counts()) for k in [0] + limits)
    outside = dict((k, 0) for k in limits)
    same = dict((k, True) for k in limits)
    sizes = dict((k, []) for k in limits)
    rng = np.random.default_rng(seed)
    for _ in range(squares):
        # (leaf2_cost_model.square's camera hits, restated: its walk is the one replaced here)
        sx, sy = rng.integers(0, m.WIDTH // 8), rng.integers(0, m.HEIGHT // 8)
        fx = (sx * 8 + np.tile(np.arange(8), 8)) / m.WIDTH - 0.5
        fy = (sy * 8 + np.repeat(np.arange(8), 8)) / m.HEIGHT - 0.5
        t = np.full(64, 10.0)
        for _ in range(30):
            wx, wy = fx - fx * t, 2.5 + fy - fy * t
            t = (m.height(wx, wy) + 50.0) / 5.0
        o = np.stack([wx, wy, m.height(wx, wy)], 1)
        ci = np.clip(((wx + 5.0) / 10.0 * wall.cells).astype(int), 0, wall.cells - 1)
        cj = np.clip(((wy + 2.5) / 10.0 * wall.cells).astype(int), 0, wall.cells - 1)
        lower = (wx - wall.x[ci]) / (wall.x[1] - wall.x[0]) >= (wy - wall.y[cj]) / (wall.y[1] - wall.y[0])

        def own(n):
            return (ci == n[0]) & (cj == n[2]) & (lower == (n[4] == 0))
        cuts = dict((k, entry_cut(wall, o, k)) for k in limits)
        for k in limits:
            sizes[k].append(len(cuts[k]))
        for _ in range(2):
            to = [m.light_points(rng) - o for _ in range(2)]
            length = [np.linalg.norm(v, axis=1) for v in to]
            d, tmax = [to[f] / length[f][:, None] for f in (0, 1)], [length[f] - 0.01 for f in (0, 1)]
            stopped, live0 = walk(wall, counts[0], o, d, tmax, own, [wall.root()])
            for k in limits:
                _, live = walk(wall, counts[k], o, d, tmax, own, cuts[k])
                outside[k] += sum(1 for n in stopped if not below(n, cuts[k]))
                same[k] = same[k] and all((a == b).all() for a, b in zip(live0, live))
    base = counts[0]
    total0 = (base.interior_valu + base.leaf_valu["after"]) / float(base.walks)
    print("%d squares, seed %d, %d two-frame walks each; unoccluded rays %.1f %%" % (squares, seed, base.walks, 100.0 * base.unoccluded / base.rays))
    print("%-14s %-34s %s" % ("start", "records per walk (interior + leaf)", "walk VALU relative to the root start"))
    for k in [0] + limits:
        c = counts[k]
        w = float(c.walks)
        total = (c.interior_valu + c.leaf_valu["after"]) / w
        print("%-14s %-34s %.2f%s" % ("root" if k == 0 else "list of <= %d" % k, "%.1f + %.1f" % (c.interior / w, c.leaves / w), total / total0,
                                       "" if k == 0 else "   (entries per list %.1f; stopping leaves outside the list: %d; every ray's fate the same: %s)" % (
                                           np.mean(sizes[k]), outside[k], same[k])))


if __name__ == "__main__":
    main()
