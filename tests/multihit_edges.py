"""Fixtures of the multi-hit query's edge tests (tests/test_gpu_multihit_edges.py; what each of them claims:
tests/test_multihit_edges_cpu.py), on top of tests/multihit.py (the peeling oracle, the sheets) and tests/query_edges.py (the
packet families, the scenes at extreme magnitudes).

* dyadic_rays(): rays through the sheets' grid vertices and the midpoints of their cell edges and diagonals whose every product
  in the triangle test is exact -- all the triangles round such a point report bit-equal t, so only SceneDev::rank8 orders them;
* dense_scene() and its families: query_edges' batches on a scene where most rays have more hits than a list holds;
* extreme(name): the scaled families on the scenes of query_edges.EXTREME; far_rays(): origins thousands of extents away;
* soup_scene(), soup_rays() and stack_depths(): a scene deep enough for own_walk_step_all's private-memory stack rows, and a
  lower bound of the depth each ray's stack reaches;
* hits_launch(n, k, cu): lt_query.hip's launch_hits_one and lt_query_hits_kernel's share / claim lines restated, and claim_sizes,
  the batch sizes at which the claim first reaches 128, lies between 128 and 512, and reaches 512;
* twice_named_scene(): the sheets with a few leaves pointed at a neighbour leaf's primitive."""
import functools

import numpy as np

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import make_rays
from tests import multihit as mh
from tests import octant_scenes as oc
from tests import query_edges as qe

F32 = np.float32
KS = (1, 3, 8)


def frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------- 1: exact ties (the sheets)
DYADIC_XY = ((1.0, 0.5), (2.0, 1.0), (0.5, 0.25), (1.0, 2.0))
DYADIC_P = (1.0, 0.5, 2.0)
DYADIC_M = (-2, -1, 0, 1, 2, 3)
DYADIC_TARGETS = ("vertex", "vertex", "vertex", "x_edge", "y_edge", "diagonal")


@functools.lru_cache(maxsize=None)
def dyadic_rays(seed=0, n=768):
    """(rays, target kind per ray, m per ray).  Every sheet triangle has e1 x e2 = (-TILT, 0, 1) (both triangles of a cell wind
    the same way), so det = dz - 0.25 dx.  Directions (+-dx, +-dy, sz p + 0.25 (+-dx)) with (dx, dy) of DYADIC_XY and p of
    DYADIC_P have det = sz p, a power of two, three nonzero components and every octant (ray i: octant i % 8); origins are
    v - m d with m of DYADIC_M (m = 0: the origin ON the point, t = +-0) and v a grid vertex of a sheet (integer x, y in
    [-2, 2], z = 0.5 k + 0.25 x; a quarter of the rays on the doubled sheet), the midpoint of a cell edge or of a cell's
    diagonal.  All coordinates are multiples of 2^-4 below 2^4: every product and sum of the triangle test is exact in float32,
    and the six triangles round a vertex (twelve on the doubled sheet), the two of an edge or a diagonal (four) report the same
    bits of t.  On their way the rays cross the other sheets at vertices, edges and interiors alike.

    With seed 0, under each of the three epsilon programs (tests/test_multihit_edges_cpu.py asserts floors below these): 96 rays
    per octant; the widest tie is 6 for 203 rays and 12 for 73; a tie group straddles K = 1, 3, 8 for 300, 329 and 215 rays;
    280 rays have a hit at t = 0, 140 of them at -0.  NO ray has both a -0 and a +0: the numerator of t is an exact +0 for every
    triangle round the point (a cancellation, or products of the +0 of o - A), so the zero takes the sign of 1 / det, which is
    one sign per ray as all the triangles wind the same way.  The t = 0 rays stay: their lists order -0 (or +0) ties by rank
    among hits of negative and positive t."""
    rng = np.random.default_rng(seed)
    rays, kinds, ms = [], [], []
    for i in range(n):
        sx, sy, sz = oc.octant_signs(i % 8)
        while True:                                            # (p = 0.5 against dx = 2 of the other sign: dz = 0, drawn again)
            dx, dy = DYADIC_XY[rng.integers(0, len(DYADIC_XY))]
            p = DYADIC_P[rng.integers(0, len(DYADIC_P))]
            d = np.array([sx * dx, sy * dy, sz * p + mh.TILT * sx * dx])
            if d[2] != 0 and np.sign(d[2]) == sz:
                break
        kind = DYADIC_TARGETS[rng.integers(0, len(DYADIC_TARGETS))]
        x, y = (float(c) for c in rng.integers(-2, 3, 2))
        if kind in ("x_edge", "diagonal"):
            x += 0.5 * rng.choice([-1.0, 1.0])
        if kind in ("y_edge", "diagonal"):
            y += 0.5 * rng.choice([-1.0, 1.0])
        k = mh.DOUBLED if rng.integers(0, 4) == 0 else int(rng.integers(0, mh.SHEETS))
        v = np.array([x, y, mh.SPACING * k + mh.TILT * x])
        m = DYADIC_M[(i // 8) % len(DYADIC_M)]
        o = v - m * d
        assert (o.astype(F32) == o).all() and (d.astype(F32) == d).all() and (d != 0).all()
        rays.append(make_rays([o], [d])[0])
        kinds.append(kind)
        ms.append(m)
    return frozen(np.array(rays, dtype=F32)), np.array(kinds), np.array(ms)


def tie_groups(seq):
    """The runs of equal t (float ==: -0 and +0 are one run) of a hit sequence: a list of (start, end) index pairs."""
    out, a = [], 0
    for j in range(1, len(seq) + 1):
        if j == len(seq) or seq[j][0] != seq[a][0]:
            out.append((a, j))
            a = j
    return out


def widest_tie(seq):
    return max((b - a for a, b in tie_groups(seq)), default=0)


def straddles(seq, k):
    """A tie group holds entries k - 1 and k: only the tie rule decides which of its hits a list of k keeps."""
    return len(seq) > k and seq[k - 1][0] == seq[k][0]


def both_zeros(seq):
    t = np.array([h[0] for h in seq], dtype=F32)
    z = t == 0
    return bool((z & np.signbit(t)).any() and (z & ~np.signbit(t)).any())


# ------------------------------------------------------------------------------------------- 2: query_edges' families, two scenes
DENSE_FAMILIES = ("coherent", "tmax", "ignore", "ties", "intruders", "partial33")


@functools.lru_cache(maxsize=None)
def base_scene():
    return qe.base_scene(0)


@functools.lru_cache(maxsize=None)
def dense_scene():
    """octant_scene's geometry with 3000 triangles in the same box: ten times the base scene's hits per ray."""
    return oc.octant_scene(0, 1, n=3000)


@functools.lru_cache(maxsize=None)
def base_families():
    return {b.name: frozen(b.rays) for b in qe.families(base_scene(), 0)}


@functools.lru_cache(maxsize=None)
def dense_families():
    s = dense_scene()
    rng = np.random.default_rng(1)
    fams = [qe.fam_coherent(s, rng), qe.fam_tmax(s, rng), qe.fam_ignore(s, rng), qe.fam_ties(s, rng), qe.fam_intruders(s, rng),
            qe.fam_partial(s, rng, 33)]
    assert tuple(b.name for b in fams) == DENSE_FAMILIES
    return {b.name: frozen(b.rays) for b in fams}


# ---------------------------------------------------------------------------------------------------- 3: extreme magnitudes
SCALED_FAMILIES = ("coherent", "tmax", "ignore", "intruders", "partial33")      # (tests/test_gpu_query_edges.py's)
EXTREME_PROGRAMS = {"tiny": (C.PROGRAM_ACCUMULATOR, C.PROGRAM_BASIC), "large": (C.PROGRAM_ACCUMULATOR, C.PROGRAM_BASIC)}


@functools.lru_cache(maxsize=None)
def extreme(name):
    """(scene, rays) of query_edges.EXTREME[name]: the base scene under x -> s x + t and the scaled families mapped onto it."""
    s, _, scale, t = qe.extreme_scene(base_scene(), name)
    fams = base_families()
    return s, frozen(np.concatenate([qe.scale_rays(fams[f], scale, t) for f in SCALED_FAMILIES]))


def extreme_programs(name):
    return EXTREME_PROGRAMS.get(name, (C.PROGRAM_ACCUMULATOR,))


FAR_DISTANCES = (2.0 ** 13, 2.0 ** 16, 2.0 ** 19)


@functools.lru_cache(maxsize=None)
def far_rays(seed=0, chunks=64):
    """Rays from FAR away at vertices and edge points of the base scene's triangles (they lie on the faces of the leaf boxes):
    per distance `chunks` chunks of 64 rays of one octant each, origins target - dist * (a unit direction of the octant), dist
    of FAR_DISTANCES (a thousand to 65 thousand times the scene's extent of 8), the direction fl32(target - origin) moved by up
    to three float steps per component.

    Why: own16_ray's margin m = 2^-21 K covers the roundings of the conservative test, K = E |inv| + |O inv| + |o inv| per axis.
    Where the origin is about as large as the scene, K |inv|^-1 is about |lo|, and the boxes' own slack -- 8 * 2^-24 |lo| from
    `outwards`, up to a grid step of 2^-16 E from the quantisation -- covers those roundings even with m = 0 (measured on the
    CPU with tests/test_own_hierarchy_cpu.py's restatement: no box missed of 150 000 grazing rays per scene, the scenes at
    extreme magnitudes included, whose origins scale with them).  With |o| >> |lo| the roundings of o inv dominate and only m
    is left: of the grazing rays the reference lets into a box, m = 2^-24 K misses 3 in 78 000 at a thousand extents and 31 in
    63 000 at a hundred thousand; m = 2^-23 K misses none."""
    s = base_scene()
    rng = np.random.default_rng(seed)
    pool = qe.geometry_prims(s)
    out = []
    for dist in FAR_DISTANCES:
        for c in range(chunks):
            sg = oc.octant_signs(c % 8)
            target = qe.points_on(s, rng.choice(pool, qe.LANES), rng, "vertex" if c % 2 else "edge")
            u = sg * rng.uniform(0.05, 1.0, (qe.LANES, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            o = (target - dist * u).astype(F32)
            d = (target - o.astype(np.float64)).astype(F32)
            d = (d * (1 + rng.integers(-3, 4, (qe.LANES, 3)) * 2.0 ** -23)).astype(F32)
            out.append(make_rays(o, d))
    return frozen(np.concatenate(out).astype(F32))


# ------------------------------------------------------------------------------------------------------ 4: the private stack
TRACE_ROWS = 10          # lt_device.hpp: kTraceRows, the stack rows own_walk_step_all<PROGRAM, kTraceRows> keeps in LDS
SOUP_COUNT = 524288
SOUP_RAYS = 200_000
SOUP_SAMPLE = 2000


@functools.lru_cache(maxsize=None)
def soup_scene():
    """synth.triangle_soup with N = 524 288 triangles.  Of the 2000 sampled rays, stack_depths' lower bound exceeds kTraceRows = 10
    for 2 at N = 65 536, 33 at N = 262 144, 102 at N = 524 288 (deepest: 15) and 229 at N = 1 048 576: N = 524 288 is the first
    power of two that gives the 64 rays tests/test_multihit_edges_cpu.py asks for."""
    return synth.triangle_soup(count=SOUP_COUNT).validate()


@functools.lru_cache(maxsize=None)
def soup_rays(seed=4):
    """(rays, sample): random rays from inside the root box (tests/test_gpu_trace_rays.py's test_scale_coherent_equals_incoherent
    draws them the same way) and the indices of those the CPU also peels."""
    s = soup_scene()
    nv = s.node_view
    lo, hi = nv["boundsMin"][0].astype(np.float64), nv["boundsMax"][0].astype(np.float64)
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (SOUP_RAYS, 3))
    rays = make_rays(o, rng.normal(0, 1, (SOUP_RAYS, 3)))
    sample = np.sort(rng.choice(SOUP_RAYS, SOUP_SAMPLE, replace=False))
    return frozen(rays), frozen(sample)


def stack_depths(scene, rays, leaves=False):
    """A LOWER bound of the deepest stack own_walk_step_all reaches for each ray: the kernel's walk over the 4-wide groups
    (lt_hip_own_hierarchy + lt_hip_own_wide) -- the entered slots of a group pushed in the order 0..3, the last one pushed popped
    first, a leaf record popped and nothing pushed -- where a slot counts as entered only when a float64 slab test of its
    dequantised box [O + ql S, O + qh S] against the ray's float32 inverse direction accepts by a clear margin: exit - enter
    above 2^-20 (E |inv| + |O inv| + |o inv|) summed over the axes, sixteen times the rounding error of own16_box_test's float32
    arithmetic, whose own margins only widen what it accepts.  The kernel therefore enters a superset of these slots in the
    same order: by induction what is pending on this walk's stack is pending on the kernel's, and at every group this walk
    visits the kernel's stack is at least as deep.  All rays walk in lockstep, one record per step.  leaves=True: also the
    number of leaf records each ray pops."""
    h, own, _ = C.own_hierarchy(scene.node_view, scene.n_prims)
    assert h > 0
    _, O, S, slots = C.own_wide(own, scene.n_prims)
    O, S = O.astype(np.float64), S.astype(np.float64)
    q = slots["q"].astype(np.float64)                         # [G, 4, 6]
    link = slots["link"].astype(np.int64)                     # [G, 4]
    n = len(rays)
    o = rays[:, 0:3].astype(np.float64)
    inv = qe.inverse(rays[:, 4:7]).astype(np.float64)
    assert qe.own_ok(rays).all()
    neg = inv < 0
    margin = (2.0 ** -20 * (65535.0 * S * np.abs(inv) + np.abs(O * inv) + np.abs(o * inv))).sum(axis=1)
    stack = np.zeros((n, 64), dtype=np.int64)
    sp = np.zeros(n, dtype=np.int64)
    e = np.zeros(n, dtype=np.int64)                            # the root's group
    deepest = np.zeros(n, dtype=np.int64)
    popped = np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    while len(live):
        g = live[e[live] < 0x80000000]                         # the rays at a group
        popped[live[e[live] >= 0x80000000]] += 1
        if len(g):
            for k in range(4):
                qk = q[e[g], k]                                # [g, 6]
                l0 = (O + qk[:, :3] * S - o[g]) * inv[g]
                l1 = (O + qk[:, 3:] * S - o[g]) * inv[g]
                t_in = np.where(neg[g], l1, l0).max(axis=1)
                t_out = np.where(neg[g], l0, l1).min(axis=1)
                ok = t_out - np.maximum(t_in, 0.0) > margin[g]
                r = g[ok]
                stack[r, sp[r]] = link[e[r], k]
                sp[r] += 1
            deepest[g] = np.maximum(deepest[g], sp[g])
        live = live[sp[live] > 0]
        sp[live] -= 1
        e[live] = stack[live, sp[live]]
    return (deepest, popped) if leaves else deepest


# ------------------------------------------------------------------------------------------------------- 5: the claim loop
BLOCK = 64               # kBlock
STAGE_ROWS = 20          # kTraceRows + kTraceStage
CLAIM_MAX = 512          # kQueryClaim
LDS_PER_CU = 160 * 1024
WAVES_PER_CU = 32
SMALL_SIZES = (511, 512, 513, 4095, 4097)


def hits_launch(n, k, cu):
    """(grid, claim) of lt_hip_trace_hits for n rays and lists of k entries (0: the count) on a chip of cu CUs: launch_hits_one's
    grid and lt_query_hits_kernel's `share` / `claim` lines (lens_trace_amd/csrc/lt_query.hip)."""
    fit = LDS_PER_CU // ((STAGE_ROWS + 2 * k) * BLOCK * 4)
    resident = cu * min(WAVES_PER_CU, fit)
    grid = min(-(-n // BLOCK), resident)
    share = n // (grid * 4) // BLOCK * BLOCK
    return grid, min(max(share, BLOCK), CLAIM_MAX)


def claim_sizes(k, cu):
    """(smallest n whose claim is 128, an n whose claim lies strictly between 128 and 512, the smallest n whose claim is 512
    plus 17): the smallest batches at which the kernel's claims of more than one stage run at all."""
    def first(c):
        lo, hi = 1, 2 ** 31                                    # (the claim does not fall as n grows)
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if hits_launch(mid, k, cu)[1] >= c else (mid + 1, hi)
        return lo
    a, b = first(128), first(CLAIM_MAX)
    between = first(320) + 2577
    assert hits_launch(a, k, cu)[1] == 128 and hits_launch(a - 1, k, cu)[1] == 64
    assert 128 < hits_launch(between, k, cu)[1] < CLAIM_MAX
    assert hits_launch(b, k, cu)[1] == CLAIM_MAX and hits_launch(b - 1, k, cu)[1] < CLAIM_MAX
    return a, between, b + 17


# ------------------------------------------------------------------------------------------------------------ 6: small pins
def odd_ignore_values(n_prims):
    """Ignore values outside [0, n_prims): the ones at and above n_prims name no primitive, every negative one means -1."""
    return (n_prims, n_prims + 1, 2 ** 31 - 1, -2, -2 ** 31)


def with_ignore(rays, value):
    r = np.array(rays)
    r[:, 7] = np.int32(value).view(F32)
    return r


TWICE_NAMED_STRIDE = 37


@functools.lru_cache(maxsize=None)
def twice_named_scene():
    """(scene, the re-pointed leaves' node indices, the primitive each now names, the leaves that named those primitives all
    along): the sheets scene with every 37th leaf's `offset` pointed at the primitive of the leaf that follows it in the node
    array -- its neighbour in the tree, a triangle beside or near its own, inside or overlapping its box.  The leaf's own
    primitive is then named by no leaf."""
    s0 = mh.sheets_scene()
    s = sc.Scene(s0.nodes.copy(), s0.prims.copy(), s0.materials.copy(), s0.lights.copy(), s0.camera)
    nv = s.node_view
    leaves = np.flatnonzero(nv["primitiveCount"] != 0)
    which = np.arange(3, len(leaves) - 1, TWICE_NAMED_STRIDE)
    prims = nv["offset"][leaves[which + 1]].copy()
    nv["offset"][leaves[which]] = prims
    return s.validate(), leaves[which], prims, leaves[which + 1]


def twice_named_reach(rays, seqs):
    """Per ray, (sure, possible): how many re-pointed leaves add a second report of their primitive to the ray's walk over the
    caller's tree, which happens when the ray hits the primitive (it is in the ray's sequence) and passes the box tests of both
    leaves that name it (their ancestors' boxes enclose them).  `possible` counts every re-pointed leaf whose primitive the ray
    hits; `sure` those where a float64 slab test enters both boxes by a margin far above float32's rounding."""
    s, nodes, prims, homes = twice_named_scene()
    nv = s.node_view
    sure, possible = np.zeros(len(rays), dtype=int), np.zeros(len(rays), dtype=int)

    def enters(leaf, o, inv):
        a, b = (nv["boundsMin"][leaf].astype(np.float64) - o) * inv, (nv["boundsMax"][leaf].astype(np.float64) - o) * inv
        t_in, t_out = np.minimum(a, b).max(axis=1), np.maximum(a, b).min(axis=1)
        return t_out - np.maximum(t_in, 0.0) > 1e-3 * (1.0 + np.abs(t_in) + np.abs(t_out))

    for i, (r, seq) in enumerate(zip(rays, seqs)):
        hit = np.isin(prims, [h[1] for h in seq])
        possible[i] = hit.sum()
        if hit.any() and qe.own_ok(r[None])[0]:
            o, inv = r[0:3].astype(np.float64), qe.inverse(r[4:7]).astype(np.float64)
            sure[i] = (enters(nodes[hit], o, inv) & enters(homes[hit], o, inv)).sum()
    return sure, possible
