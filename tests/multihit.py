"""The oracle, the scene and the ray batch of the multi-hit query tests (tests/test_gpu_trace_hits.py; what each of them claims:
tests/test_trace_hits_cpu.py).

lt_hip_trace_hits (include/lenstrace_hip.h) defines a ray's HIT SEQUENCE by peeling: hit 0 is the reference's closest hit, hit j
the closest hit once the primitives of hits 0 .. j-1 are degenerate (B = C = A), until the first miss.

* peel(scene, ray, program, limit): exactly that, with the CPU oracle's lt_oracle_trace (the reference's intersect /
  intersectIgnorePrimitiveIndex) on a copy of the scene.  sequences(...) peels a whole batch once and keeps the result.
* sheets_scene(): 12 parallel sheets of 6 x 6 cells on the integer grid [-3, 3]^2, z = 0.5 k + 0.25 x (tilted: a triangle's box has
  a depth, so a ray that starts inside it can hit the triangle BEHIND its origin, at negative t); sheet 2 is there twice, vertex
  for vertex, so every ray through it meets two bit-equal t -- from the front at positions 2 and 3 of its sequence.
* sheet_rays(): about 64 x 40 + 17 rays in the categories of CATEGORIES; lt_query_hits_kernel hands neighbouring rays to
  neighbouring lanes, so the batch puts rays of a few hits beside rays of a hundred.
* expected_records / expected_counts: what LT_TRACE_FIRST_K and LT_TRACE_COUNT must write."""
import ctypes
import functools

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import FLT_MAX, HIT_DTYPE, make_rays
from oracle import pyoracle as po

F32 = np.float32
SHEETS = 12
CELLS = 6
HALF = CELLS / 2.0
SPACING = 0.5
TILT = 0.25                    # dz / dx of every sheet
DOUBLED = 2                    # the sheet that is there twice
CATEGORIES = ("random", "axis", "miss", "through", "ignore", "tmax_fltmax", "tmax_inf", "tmax_zero", "tmax_negative", "tmax_nan",
              "tmax_between", "fallback", "inside")


# ------------------------------------------------------------------------------------------------------------------ the oracle
class Peeler:
    """lt_oracle_trace over a private copy of the scene whose primitives can be made degenerate and restored."""

    def __init__(self, scene):
        self.L = po.lib()
        self.nodes = np.ascontiguousarray(scene.nodes).copy()
        self.prims = np.ascontiguousarray(scene.prims).copy()
        self.pv = self.prims.view(sc.PRIM_DTYPE)
        self.o, self.d = np.ones(4, dtype=F32), np.zeros(4, dtype=F32)   # origin.w = 1, direction.w = +0
        self.tuv = np.zeros(3, dtype=F32)
        self.prim = ctypes.c_int(0)
        vp = ctypes.c_void_p
        self.ptrs = [a.ctypes.data_as(vp) for a in (self.nodes, self.prims, self.o, self.d, self.tuv)]

    def trace(self, ray, program):
        """(t, prim, u, v) of the reference's closest hit of the lt_hip_ray record `ray`, or None."""
        self.o[:3], self.d[:3] = ray[0:3], ray[4:7]
        ign = int(ray[7:8].view(np.int32)[0])
        n, p, o, d, tuv = self.ptrs
        hit = self.L.lt_oracle_trace(program, n, p, o, d, ctypes.c_float(ray[3]), 1 if ign >= 0 else 0, max(ign, 0),
                                     ctypes.byref(self.prim), tuv)
        return (self.tuv[0].copy(), self.prim.value, self.tuv[1].copy(), self.tuv[2].copy()) if hit else None

    def peel(self, ray, program, limit=None):
        """Every peel takes one primitive out of the scene, so a sequence has at most n_prims entries and peel n_prims + 1 is a
        miss: the loop stops there at the latest, and a peel that would go on is an assertion, not a hang."""
        seq, saved = [], []
        stop = self.pv.size + 1
        try:
            while limit is None or len(seq) < limit:
                h = self.trace(ray, program)
                if h is None:
                    break
                assert len(seq) + 1 < stop, ("peel %d of a scene of %d primitives is a hit: the peel does not end" % (stop, stop - 1), h, ray)
                seq.append(h)
                p = h[1]
                saved.append((p, self.pv["positionB"][p].copy(), self.pv["positionC"][p].copy()))
                self.pv["positionB"][p] = self.pv["positionA"][p]
                self.pv["positionC"][p] = self.pv["positionA"][p]
        finally:
            for p, b, c in reversed(saved):
                self.pv["positionB"][p], self.pv["positionC"][p] = b, c
        return seq


def peel(scene, ray, program=po.ACCUMULATOR, limit=None):
    """The first `limit` entries (None: all) of the hit sequence of one lt_hip_ray record: a list of (t, prim, u, v)."""
    return Peeler(scene).peel(np.asarray(ray, dtype=F32).reshape(8), program, limit)


_kept = {}


def sequences(name, scene, rays, program):
    """The whole hit sequence of every ray of a batch, peeled once per (name, program) and shared; do not modify."""
    key = (name, program)
    if key not in _kept:
        p = Peeler(scene)
        _kept[key] = [p.peel(r, program) for r in rays]
    return _kept[key]


def expected_records(seqs, rays, k):
    """LT_TRACE_FIRST_K's output: (n, k) HIT_DTYPE; slots behind a sequence's end hold {tmax (the ray's own bits), -1, 0, 0}."""
    out = np.zeros((len(rays), k), dtype=HIT_DTYPE)
    out["t"] = rays[:, 3:4]
    out["prim"] = -1
    for i, s in enumerate(seqs):
        for j, h in enumerate(s[:k]):
            out[i, j] = h
    return out


def expected_counts(seqs):
    return np.array([len(s) for s in seqs], dtype=np.uint32)


def same_records(got, want):
    """Indices of the rays whose records differ in any bit."""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), -1)
    return np.flatnonzero((g != w).any(axis=1))


# ------------------------------------------------------------------------------------------------------------------- the scene
def sheet_z(k, x=0.0):
    return F32(k * SPACING) + F32(TILT) * F32(x)      # (exact for grid vertices)


def sheet_of(scene):
    """The sheet each primitive lies in."""
    a = scene.prim_view["positionA"]
    return np.rint((a[:, 2] - F32(TILT) * a[:, 0]) / SPACING).astype(int)


@functools.lru_cache(maxsize=None)
def sheets_scene():
    tris = []
    for k in list(range(SHEETS)) + [DOUBLED]:
        for j in range(CELLS):
            for i in range(CELLS):
                x0, x1, y0, y1 = i - HALF, i + 1 - HALF, j - HALF, j + 1 - HALF
                z0, z1 = sheet_z(k, x0), sheet_z(k, x1)
                tris.append([(x0, y0, z0), (x1, y0, z1), (x1, y1, z1)])
                tris.append([(x0, y0, z0), (x1, y1, z1), (x0, y1, z0)])
    pos = np.array(tris, dtype=F32)
    nrm = np.tile(F32([0, 0, -1]), (len(pos), 3, 1))
    m = np.zeros(2, dtype=sc.MATERIAL_DTYPE)
    m["diffuse"], m["ior"], m["dissolve"] = 0.5, 1.3, 1.0
    m[1]["emission"] = (1, 1, 1)
    return sc.build_from_triangles(pos, nrm, np.zeros(len(pos), dtype=np.int32), m).validate()


def doubled_prims(scene):
    """Primitives whose three corners have the bits of another primitive's."""
    pv = scene.prim_view
    key = np.concatenate([pv["positionA"], pv["positionB"], pv["positionC"]], axis=1).view(np.uint32)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return np.flatnonzero(cnt[inv.reshape(-1)] > 1)


# --------------------------------------------------------------------------------------------------------------- the ray batch
def _through(rng, n, front=None):
    """Rays that cross the whole stack inside the sheets' outline: from z < 0 to z > 5.5 (front) or back, chosen per ray."""
    z0, z1 = -2.0, float(sheet_z(SHEETS - 1, HALF)) + 1.0
    a = np.column_stack([rng.uniform(-HALF + 0.1, HALF - 0.1, (n, 2)), np.full(n, z0)])
    b = np.column_stack([rng.uniform(-HALF + 0.1, HALF - 0.1, (n, 2)), np.full(n, z1)])
    f = rng.integers(0, 2, n) == 0 if front is None else np.full(n, front)
    o = np.where(f[:, None], a, b)
    return make_rays(o, np.where(f[:, None], b, a) - o)


def _missers(rng, n):
    """Rays beside the stack, parallel to it or pointing away: no box of the scene and no triangle on their way."""
    o = np.column_stack([rng.uniform(HALF + 1.0, HALF + 3.0, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-HALF, HALF, n), rng.uniform(-2, 7.5, n)])
    d = np.column_stack([np.sign(o[:, 0]) * rng.uniform(0.1, 1.0, n), rng.normal(0, 1, n), rng.normal(0, 1, n)])
    return make_rays(o, d)


def _inside(rng, scene, n):
    """Rays that start inside the box of a triangle a little BEYOND its plane: that triangle is hit at t = -s < 0.  Returns the
    rays and s."""
    pv = scene.prim_view
    rays, back = [], []
    while len(rays) < n:
        p = int(rng.integers(0, scene.n_prims))
        A, B, Cc = (pv[k][p].astype(np.float64) for k in ("positionA", "positionB", "positionC"))
        b = rng.dirichlet([2, 2, 2])
        P = b[0] * A + b[1] * B + b[2] * Cc
        d = np.array([rng.normal(0, 1), rng.normal(0, 1), rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.0)])
        s = rng.uniform(0.02, 0.2)
        o = (P + s * d).astype(F32).astype(np.float64)
        lo, hi = np.minimum(np.minimum(A, B), Cc), np.maximum(np.maximum(A, B), Cc)
        if (o > lo + 1e-3).all() and (o < hi - 1e-3).all():
            rays.append(make_rays([o], [d])[0])
            back.append(s)
    return np.array(rays), np.array(back)


@functools.lru_cache(maxsize=None)
def sheet_rays(seed=0):
    """(rays, category): the batch as make_rays records and each ray's category name (numpy array of str); read only."""
    rng = np.random.default_rng(seed)
    s = sheets_scene()
    zmid = float(sheet_z(SHEETS - 1)) / 2
    ztop = float(sheet_z(SHEETS - 1, HALF))
    parts, cats = [], []

    def add(name, rays):
        parts.append(rays.astype(F32))
        cats.extend([name] * len(rays))

    # random rays through the bounds: from anywhere around the stack towards a point inside it
    o = rng.uniform([-6, -6, -4], [6, 6, 9.5], (640, 3))
    add("random", make_rays(o, rng.uniform([-HALF, -HALF, 0], [HALF, HALF, 2 * zmid], (640, 3)) - o))
    # axis-parallel rays: through grid vertices, through cell edges, and inside the sheets' planes along cell edges
    g = rng.integers(-3, 4, (128, 2)).astype(np.float64)
    add("axis", make_rays(np.column_stack([g, np.where(rng.integers(0, 2, 128) == 0, -2.0, ztop + 1)]), [[0, 0, 1]] * 128))
    parts[-1][parts[-1][:, 2] > 0, 6] = -1.0
    e = np.column_stack([rng.integers(-3, 4, 128), rng.uniform(-HALF, HALF, 128)])
    e[::2] = e[::2, ::-1]
    add("axis", make_rays(np.column_stack([e, np.full(128, -2.0)]), [[0, 0, 1]] * 128))
    xi = rng.integers(-3, 4, 128)                                          # along the y edges of the cells: inside a sheet
    inplane = np.column_stack([xi, np.full(128, -5.0), rng.integers(0, SHEETS, 128) * SPACING + TILT * xi])
    add("axis", make_rays(inplane, [[0, 1, 0]] * 128))
    # rays that miss everything beside rays through every sheet, lane by lane
    mix = np.empty((256, 8), dtype=F32)
    mix[0::2], mix[1::2] = _missers(rng, 128), _through(rng, 128)
    parts.append(mix)
    cats.extend(["miss", "through"] * 128)
    # rays that ignore a primitive they would hit
    r = _through(rng, 128)
    p = Peeler(s)
    for i in range(len(r)):
        seq = p.peel(r[i], po.ACCUMULATOR)
        r[i, 7:8].view(np.int32)[0] = seq[rng.integers(0, len(seq))][1]
    add("ignore", r)
    # tmax: rays through every sheet; a tmax of 0 or below accepts only hits behind the origin
    for name, val in (("tmax_fltmax", FLT_MAX), ("tmax_inf", np.inf), ("tmax_nan", np.nan)):
        r = _through(rng, 64)
        r[:, 3] = val
        add(name, r)
    r, back = _inside(rng, s, 128)
    r[:64, 3], r[64:, 3] = 0.0, -0.5 * back[64:]
    add("tmax_zero", r[:64])
    add("tmax_negative", r[64:])
    r = _through(rng, 64)
    for i in range(len(r)):                                                # a value between two of the ray's own hits
        t = np.unique([h[0] for h in p.peel(r[i], po.ACCUMULATOR)])
        j = rng.integers(0, len(t) - 1)
        r[i, 3] = (np.float64(t[j]) + np.float64(t[j + 1])) / 2
    add("tmax_between", r)
    # rays the own tree does not take: a zero or non-finite component
    r = _through(rng, 128)
    k = rng.integers(0, 4, 128)
    ax = rng.integers(0, 2, 128)
    rows = np.arange(128)
    r[rows[k == 0], 4 + ax[k == 0]] = 0.0
    r[rows[k == 1], 4 + ax[k == 1]] = -0.0
    r[rows[k == 2], 4 + rng.integers(0, 3, (k == 2).sum())] = np.nan          # (an infinite component has a finite inverse: the own tree takes it)
    r[rows[k == 3], rng.integers(0, 3, (k == 3).sum())] = rng.choice([np.inf, -np.inf, np.nan], (k == 3).sum())
    add("fallback", r)
    # origins inside the stack: hits at negative t
    add("inside", _inside(rng, s, 192)[0])
    rays = np.concatenate(parts)
    n_fill = 64 * 40 + 17 - len(rays)
    o = rng.uniform([-6, -6, -4], [6, 6, 9.5], (n_fill, 3))
    rays = np.concatenate([rays, make_rays(o, rng.uniform([-HALF, -HALF, 0], [HALF, HALF, 2 * zmid], (n_fill, 3)) - o)])
    cats.extend(["random"] * n_fill)
    rays.setflags(write=False)
    return rays, np.array(cats)


@functools.lru_cache(maxsize=None)
def cornell_rays(seed=1, n=1500):
    """Random rays around the committed Cornell box: mixed tmax, some ignoring a primitive, some axis-parallel or non-finite."""
    from tests.conftest import GOLDEN
    import os
    s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
    rng = np.random.default_rng(seed)
    nv = s.node_view
    lo, hi = nv["boundsMin"][0].astype(np.float64), nv["boundsMax"][0].astype(np.float64)
    ext = hi - lo
    o = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (n, 3))
    d = rng.normal(0, 1, (n, 3))
    k = rng.integers(0, 12, n)
    rows = np.arange(n)
    d[rows[k == 0], rng.integers(0, 3, (k == 0).sum())] = 0.0
    d[rows[k == 1], rng.integers(0, 3, (k == 1).sum())] = rng.choice([np.inf, np.nan], (k == 1).sum())
    tmax = np.full(n, FLT_MAX, dtype=np.float64)
    t = rng.integers(0, 8, n)
    tmax[t == 0] = rng.uniform(0, np.linalg.norm(ext), (t == 0).sum())
    tmax[t == 1] = rng.choice([np.inf, 0.0, -1.0, np.nan], (t == 1).sum())
    ign = np.where(k >= 10, rng.integers(0, s.n_prims, n), -1)
    rays = make_rays(o, d, tmax.astype(F32), ign)
    rays.setflags(write=False)
    return s, rays
