"""Scenes and cameras whose rays have known direction-sign octants, for the tests of the packet walks' per-octant instances
(tests/test_gpu_octants.py; the construction itself: tests/test_octant_scenes_cpu.py).

An octant NEG has bit 0 set for x < 0, bit 1 for y < 0, bit 2 for z < 0 -- the `switch` of traverse_camera, traverse and
traverse_shadow2 (lens_trace_amd/csrc/lt_device.hpp), one walk instance per value (lt_walk_asm.hpp, LT_NF_0 .. LT_NF_7).

* octant_scene(octant, seed): random geometry in the box B = [-4, 4]^3 and a small emissive patch in a box L that lies beyond B on
  every axis, on the side the octant's sign bits name.  Every shadow ray from a point of B towards a point of L then has the
  octant's signs, whatever the random draws: a wave of accumulator's shadow rays walks that octant's any-hit instance.
* camera_for(yaw, box): a camera that has the box in view at any yaw; camera_octants(cam, W, H): the octants of the 8x8 squares
  whose camera rays share their signs, i.e. the closest-hit instances a render of that size walks."""
import math

import numpy as np

from lens_trace_amd import scene as sc

BOX = 4.0                    # B = [-BOX, BOX]^3
LIGHT_CENTRE = 14.0          # L: centre at +-LIGHT_CENTRE on every axis, half size LIGHT_HALF
LIGHT_HALF = 1.0
MARGIN = LIGHT_CENTRE - LIGHT_HALF - BOX   # the gap between B and L on every axis
FILM_HALF = 0.5 / 5.0        # camera_ray: d = (-fx, -fy, 5) with |fx|, |fy| <= 0.5 before the yaw


def octant_signs(octant):
    """(sx, sy, sz): -1 where the octant's bit says the direction component is negative, else +1."""
    return np.array([-1.0 if (octant >> a) & 1 else 1.0 for a in range(3)])


def octant_of(d):
    """The octant of direction(s) d [..., 3] (the walks' `1 / d < 0`, i.e. d < 0 or d == -0)."""
    d = np.asarray(d)
    neg = np.signbit(d)
    return neg[..., 0] * 1 + neg[..., 1] * 2 + neg[..., 2] * 4


def light_box(octant):
    """(lo, hi) of L for the octant."""
    c = octant_signs(octant) * LIGHT_CENTRE
    return c - LIGHT_HALF, c + LIGHT_HALF


def octant_triangles(octant, seed, n=300, doubles=40, slivers=4, lights=3):
    """The triangles of octant_scene: (positions [N,3,3], normals [N,3,3], material indices [N], materials, is_light [N])."""
    rng = np.random.default_rng(7919 * seed + 101 * octant + 17)
    centre = rng.uniform(-0.8 * BOX, 0.8 * BOX, (n, 3))
    size = 10.0 ** rng.uniform(-1.0, 0.0, (n, 1, 1))
    pos = np.clip(centre[:, None, :] + rng.normal(0, 1, (n, 3, 3)) * size, -BOX, BOX)
    # slivers: a third vertex a hair off the middle of the first two; one triangle of zero area (a repeated vertex)
    a, b = rng.uniform(-BOX, BOX, (slivers, 3)), rng.uniform(-BOX, BOX, (slivers, 3))
    off = rng.normal(0, 1, (slivers, 3)) * 10.0 ** rng.uniform(-5, -3, (slivers, 1))
    sl = np.stack([a, b, np.clip(0.5 * (a + b) + off, -BOX, BOX)], axis=1)
    z = rng.uniform(-BOX, BOX, (2, 3))
    zero = np.stack([z[0], z[0], z[1]])[None]
    geo = np.concatenate([pos, sl, zero]).astype(np.float32)
    ng = geo.shape[0]
    k = 6                                    # materials 0..4 geometry (1 and 3 lens materials), 5 the light
    m = np.zeros(k, dtype=sc.MATERIAL_DTYPE)
    m["diffuse"] = rng.uniform(0.1, 1, (k, 3))
    m["ior"] = rng.uniform(1.0, 2.0, k)
    m["dissolve"] = 1.0
    m["dissolve"][[1, 3]] = 0.25
    m[k - 1]["emission"] = (1, 1, 1)
    mi = rng.integers(0, k - 1, ng)
    # exact duplicates with another material: bit-equal hits, settled by the reference's leaf order (SceneDev::rank8)
    dup = rng.choice(n, doubles, replace=False)
    geo = np.concatenate([geo, geo[dup]])
    mi = np.concatenate([mi, (mi[dup] + rng.integers(1, k - 1, doubles)) % (k - 1)])
    # normals leaning towards the light, so that most hits are lit (the shadow ray is walked either way)
    s = octant_signs(octant)
    nrm = s + rng.normal(0, 0.6, (geo.shape[0], 3, 3))
    # the light: a patch of triangles inside L
    lo, hi = light_box(octant)
    lp = rng.uniform(lo, hi, (lights, 3, 3))
    ln = np.tile(-s, (lights, 3, 1)).astype(np.float64)
    P = np.concatenate([geo, lp]).astype(np.float32)
    N = np.concatenate([nrm, ln])
    N = (N / np.linalg.norm(N, axis=-1, keepdims=True)).astype(np.float32)
    M = np.concatenate([mi, np.full(lights, k - 1)]).astype(np.int32)
    light = np.concatenate([np.zeros(geo.shape[0], bool), np.ones(lights, bool)])
    perm = rng.permutation(P.shape[0])
    if light[perm[0]]:                       # primitive 0 is not emissive
        j = int(np.flatnonzero(~light[perm])[0])
        perm[[0, j]] = perm[[j, 0]]
    return P[perm], N[perm], M[perm], m, light[perm]


def octant_scene(octant, seed, **kw):
    """A validated random scene whose shadow rays (B -> L) all have the octant's direction signs."""
    P, N, M, m, _ = octant_triangles(octant, seed, **kw)
    return sc.build_from_triangles(P, N, M, m).validate()


def box_of(scene_or_triangles):
    """(lo, hi) of a scene's root box, or of triangles [N,3,3]."""
    if isinstance(scene_or_triangles, np.ndarray):
        p = scene_or_triangles.reshape(-1, 3)
        return p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    root = scene_or_triangles.node_view[0]
    return np.float64(root["boundsMin"][:3]), np.float64(root["boundsMax"][:3])


def camera_for(yaw, box=(-BOX * np.ones(3), BOX * np.ones(3)), frame=0):
    """A camera at centre - R * (sin yaw, 0, cos yaw), R such that the film's extent at the box's centre covers the box's largest
    half-extent; the position is moved by nothing else (camera_ray adds the film offset (fx, fy, 0) to it, < 0.5 units)."""
    lo, hi = (np.asarray(v, dtype=np.float64) for v in box)
    c = 0.5 * (lo + hi)
    R = float((hi - lo).max()) / 2.0 / FILM_HALF
    return sc.camera_bytes(float(c[0] - R * math.sin(yaw)), float(c[1]), float(c[2] - R * math.cos(yaw)), float(yaw), 0.0, 0.0, frame)


def camera_directions(cam, W, H, dtype=np.float32):
    """The camera rays' directions [H, W, 3] as camera_ray computes them (aperture (0, 0, 5) minus the film point, turned by the
    yaw), in float32 -- the host's cos / sin of the yaw, rounded to float -- or, dtype=float64, in double throughout."""
    import struct
    yaw = struct.unpack("<6fI", bytes(cam))[3]
    f = dtype
    x, y = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    fx = x / f(W) - f(0.5)
    fy = y / f(H) - f(0.5)
    dx, dy, dz = f(0) - fx, f(0) - fy, np.full_like(fx, f(5))
    cy, sy = f(math.cos(float(yaw))), f(math.sin(float(yaw)))
    return np.stack([cy * dx + sy * dz, dy, -sy * dx + cy * dz], axis=-1).astype(f)


def square_lanes(W, H, tile=None):
    """The pixels of every 8x8 square a render launch hands out: a list of (ys, xs) index arrays, the image's own pixels only
    (render_square / square_pixel: squares tile each tile from its corner; tile = (tile_w, tile_h) or None for the whole image)."""
    tw, th = tile if tile else (W, H)
    out = []
    for ty in range(0, H, th):
        for tx in range(0, W, tw):
            for sy in range(0, th, 8):
                for sx in range(0, tw, 8):
                    ys = np.arange(ty + sy, min(ty + sy + 8, ty + th, H))
                    xs = np.arange(tx + sx, min(tx + sx + 8, tx + tw, W))
                    if ys.size and xs.size:
                        out.append(np.meshgrid(ys, xs, indexing="ij"))
    return out


def camera_octants(cam, W, H, tile=None, margin=1e-4, dtype=np.float32):
    """The octants of the squares whose camera rays all share their direction signs (the closest-hit walk of that octant).  A
    square with a direction component within `margin` of 0 counts for none: the default flavour's device sinf / cosf of the yaw
    could flip its sign, and an exact 0 sends the square to the per-lane walk."""
    d = camera_directions(cam, W, H, dtype)
    got = set()
    for ys, xs in square_lanes(W, H, tile):
        q = d[ys, xs].reshape(-1, 3)
        if (np.abs(q) <= margin).any():
            continue
        o = octant_of(q)
        if (o == o[0]).all():
            got.add(int(o[0]))
    return got
