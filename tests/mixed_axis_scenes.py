"""Scenes whose two-frame shadow-ray groups have mixed direction signs along a known axis, for the tests of the two-frame walk's
one-mixed-axis forms (tests/test_gpu_mixed_axis_groups.py; the construction itself: tests/test_mixed_axis_scenes_cpu.py).

traverse_shadow2 (lens_trace_amd/csrc/lt_device.hpp) walks the 128 shadow rays of a square's two frames together when their signs
are mixed along at most one axis: form 0 .. 7 = one octant (tests/octant_scenes.py), form 8 + 4 * axis + k = `axis` mixed, k = the
signs along the other two axes in x, y, z order (bit 0: the first of them negative, bit 1: the second) -- lt_walk_asm.hpp,
LT_NF_X0 .. LT_NF_Z3.  Two or three mixed axes: the frames render apart.

* mixed_scene(axis, k, seed): random geometry in B = [-BOX, BOX]^3 (octant_scenes) and emissive triangles in a box L that is centred
  at 0 along `axis` with a half-extent larger than BOX -- every point of B has points of L on both sides -- and lies beyond B along
  the other two axes, on the side k names.
* two_axis_scene(seed): L centred over B along x and z, beyond it in +y: squares with two mixed axes.
* penumbra_scene(name): tests/penumbra_scenes.py's floor and occluder under a light that straddles the floor in x.
* camera_hits / shadow_directions: the shadow rays accumulator's frame casts, from the oracle's camera hits and random();
  square_forms(...): the form of every square's frame pair (first, first + 1)."""
import numpy as np

from lens_trace_amd import scene as sc
from oracle import pyoracle as po
from tests import octant_scenes as oc
from tests import penumbra_scenes as ps

BOX = oc.BOX
MIXED_HALF = 6.0             # L's half-extent along the mixed axis (> BOX), centred at 0
FAR_CENTRE = oc.LIGHT_CENTRE  # ... its centre along the other axes, +-; half-extent oc.LIGHT_HALF
FORMS = [(axis, k) for axis in range(3) for k in range(4)]
SIZES = ((24, 16), (17, 9))  # 17x9 ends in a one-column square and (with its 9th row) a single-pixel square
COUNTS = (2, 3, 5)           # frames of a call: one group; one group and a frame alone; two groups and a frame alone
FIRSTS = (1, 4)
MARGIN = 1e-3                # a direction component this close to 0 has no sign the test would rely on


def form_index(axis, k):
    return 8 + 4 * axis + k


def form_signs(axis, k):
    """(sx, sy, sz): 0 along the mixed axis, -1 / +1 along the others as k's bits say."""
    others = [a for a in range(3) if a != axis]
    s = np.zeros(3)
    for bit, a in enumerate(others):
        s[a] = -1.0 if (k >> bit) & 1 else 1.0
    return s


def light_box(signs):
    """(lo, hi) of L: centred at 0 with half-extent MIXED_HALF where signs is 0, at signs * FAR_CENTRE with oc.LIGHT_HALF elsewhere."""
    s = np.asarray(signs, dtype=np.float64)
    c = s * FAR_CENTRE
    h = np.where(s == 0.0, MIXED_HALF, oc.LIGHT_HALF)
    return c - h, c + h


def triangles(signs, seed, n=220, lights=6):
    """(positions [N,3,3], normals [N,3,3], material indices [N], materials, is_light [N])."""
    s = np.asarray(signs, dtype=np.float64)
    rng = np.random.default_rng(104729 * seed + 31)
    centre = rng.uniform(-0.8 * BOX, 0.8 * BOX, (n, 3))
    size = 10.0 ** rng.uniform(-1.0, 0.0, (n, 1, 1))
    geo = np.clip(centre[:, None, :] + rng.normal(0, 1, (n, 3, 3)) * size, -BOX, BOX).astype(np.float32)
    k = 5                                    # materials 0..3 geometry, 4 the light
    m = np.zeros(k, dtype=sc.MATERIAL_DTYPE)
    m["diffuse"] = rng.uniform(0.1, 1, (k, 3))
    m["ior"] = rng.uniform(1.0, 2.0, k)
    m["dissolve"] = 1.0
    m[k - 1]["emission"] = (1, 1, 1)
    mi = rng.integers(0, k - 1, n)
    nrm = s + rng.normal(0, 0.6, (n, 3, 3))  # leaning towards the light: most hits are lit
    lo, hi = light_box(s)
    lp = rng.uniform(lo, hi, (lights, 3, 3))
    mixed = np.flatnonzero(s == 0.0)
    lp[:, 0, mixed] = lo[mixed]              # every light triangle spans L along the mixed axes
    lp[:, 1, mixed] = hi[mixed]
    ln = np.tile(-s, (lights, 3, 1))
    P = np.concatenate([geo, lp]).astype(np.float32)
    N = np.concatenate([nrm, ln])
    N = (N / np.linalg.norm(N, axis=-1, keepdims=True)).astype(np.float32)
    M = np.concatenate([mi, np.full(lights, k - 1)]).astype(np.int32)
    light = np.concatenate([np.zeros(n, bool), np.ones(lights, bool)])
    return P, N, M, m, light                 # (primitive 0 is not emissive)


def mixed_scene(axis, k, seed=None):
    P, N, M, m, _ = triangles(form_signs(axis, k), form_index(axis, k) if seed is None else seed)
    return sc.build_from_triangles(P, N, M, m).validate()


TWO_AXIS_SIGNS = (0.0, 1.0, 0.0)             # L centred over B along x and z, beyond it in +y


def two_axis_scene(seed=3):
    P, N, M, m, _ = triangles(TWO_AXIS_SIGNS, seed)
    return sc.build_from_triangles(P, N, M, m).validate()


def camera(form, first):
    """The camera of a form's calls: in front of B (yaw 0) or behind it (yaw pi)."""
    return oc.camera_for((0.0, np.pi)[form % 2], frame=first)


# ---- the penumbra under a light that straddles the floor in x: every floor point has the light on both sides in x, above it in y and
# behind it in z -- form (x mixed, y > 0, z < 0), LT_NF_X2 -- and an occluder large enough that a good share of the light is hidden
PENUMBRA_FORM = (0, 2)
PENUMBRA_LIGHT_X, PENUMBRA_LIGHT_Y, PENUMBRA_LIGHT_Z = (-7.0, 7.0), 13.0, (-16.0, -14.0)
PENUMBRA_LIGHT_CENTRE = np.array([0.0, 13.0, -15.0])
PENUMBRA_OCCLUDER_HALF = 2.0
PENUMBRA_CASES = {"24x16": dict(W=24, H=16, target=(12, 8)), "17x9": dict(W=17, H=9, target=(16, 4))}


def penumbra_triangles(target):
    """(positions [5,3,3], normals [5,3,3], material indices [5], materials): floor (2), occluder (1), light (2)."""
    fp, fn = ps.floor_triangles()
    (x0, x1), y, (z0, z1) = PENUMBRA_LIGHT_X, PENUMBRA_LIGHT_Y, PENUMBRA_LIGHT_Z
    lp = np.float32([[[x0, y, z0], [x1, y, z0], [x1, y, z1]], [[x0, y, z0], [x1, y, z1], [x0, y, z1]]])
    ln = np.tile(np.float32([0, -1, 0]), (2, 3, 1))
    t = np.asarray(target, dtype=np.float64)
    axis = PENUMBRA_LIGHT_CENTRE - t
    c = t + ps.OCCLUDER_AT * axis
    axis /= np.linalg.norm(axis)
    u = np.cross(axis, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(axis, u)
    h = PENUMBRA_OCCLUDER_HALF
    op = np.float32([[c + h * (-u - 0.6 * v), c + h * (u - 0.6 * v), c + h * 1.2 * v]])
    on = np.tile(np.float32(-axis), (1, 3, 1))
    _, _, _, m = ps.penumbra_triangles(target)
    return np.concatenate([fp, op, lp]), np.concatenate([fn, on, ln]), np.int32([0, 0, 1, 2, 2]), m


def penumbra_scene(name):
    c = PENUMBRA_CASES[name]
    P, N, M, m = penumbra_triangles(ps.floor_point(ps.CAM, c["W"], c["H"], *c["target"]))
    return sc.build_from_triangles(P, N, M, m).validate()


# ---- what the frames' shadow rays are (acc.cl:239-279: the light's primitive from random(fx, fy, frame), the point on it from
# random(fx, fy, frame + 1) and random(fx, fy, frame + 2); the ray from the camera hit's interpolated position)
def camera_hits(scene, cam, W, H):
    """(has [H,W] bool: the pixel's camera ray hits a primitive that is no light, position [H,W,3] float32, film [H,W,2] float32,
    primitive [H,W] int)."""
    import struct
    px, py, pz = struct.unpack("<6fI", bytes(cam))[:3]
    f = np.float32
    d = oc.camera_directions(cam, W, H)
    pv, lv = scene.prim_view, scene.light_view[0]
    emissive = set(int(p) for p in lv["primitives"][:int(lv["count"])])
    has = np.zeros((H, W), bool)
    pos = np.zeros((H, W, 3), f)
    film = np.zeros((H, W, 2), f)
    prims = np.full((H, W), -1)
    for y in range(H):
        for x in range(W):
            fx, fy = f(x) / f(W) - f(0.5), f(y) / f(H) - f(0.5)
            film[y, x] = fx, fy
            o = np.array([f(px) + fx, f(py) + fy, f(pz), 1], f)
            hit, prim, tuv = po.trace(scene, o, np.append(d[y, x], f(0)))
            if hit and prim not in emissive:
                u, v = np.float64(tuv[1]), np.float64(tuv[2])
                p = pv[prim]
                pos[y, x] = (np.float64(p["positionA"]) * (1.0 - u - v) + np.float64(p["positionB"]) * u + np.float64(p["positionC"]) * v)
                has[y, x] = True
                prims[y, x] = prim
    return has, pos, film, prims


def shadow_directions(scene, hits, frame):
    """[H,W,3]: light point minus hit point for every pixel of `frame` (zeros where the pixel casts no shadow ray)."""
    has, pos, film, _ = hits
    pv, lv = scene.prim_view, scene.light_view[0]
    count = int(lv["count"])
    out = np.zeros(pos.shape, np.float64)
    f = np.float32
    for y, x in zip(*np.nonzero(has)):
        fx, fy = float(film[y, x, 0]), float(film[y, x, 1])
        r = [f(po.random(fx, fy, float(frame + i))) for i in range(3)]
        idx = int(f(r[0]) * f(count))
        lp = pv[int(lv["primitives"][idx]) if 0 <= idx < 64 else 0]
        u, v = (f(1) - r[1], f(1) - r[2]) if r[1] + r[2] > f(1) else (r[1], r[2])
        u, v = np.float64(u), np.float64(v)
        l = np.float64(lp["positionA"]) * (1.0 - u - v) + np.float64(lp["positionB"]) * u + np.float64(lp["positionC"]) * v
        out[y, x] = l - np.float64(pos[y, x])
    return out


def square_forms(scene, cam, W, H, first, hits=None):
    """The form of the frame pair (first, first + 1) in every square (oc.square_lanes order): an octant 0 .. 7, a one-mixed-axis
    form 8 .. 19, -2 / -3 for two / three mixed axes, None for a square without shadow rays or with a direction component within
    MARGIN of 0.  Also returns the per-square pixel index arrays and the hits."""
    hits = hits or camera_hits(scene, cam, W, H)
    d = [shadow_directions(scene, hits, first + j) for j in range(2)]
    forms, lanes = [], oc.square_lanes(W, H)
    for ys, xs in lanes:
        on = hits[0][ys, xs].reshape(-1)
        q = np.concatenate([dj[ys, xs].reshape(-1, 3)[on] for dj in d])
        if q.shape[0] == 0 or (np.abs(q) <= MARGIN).any():
            forms.append(None)
            continue
        neg = q < 0
        mixed = [a for a in range(3) if neg[:, a].any() and not neg[:, a].all()]
        if len(mixed) > 1:
            forms.append(-len(mixed))
        elif not mixed:
            forms.append(int(neg[0, 0]) + 2 * int(neg[0, 1]) + 4 * int(neg[0, 2]))
        else:
            others = [a for a in range(3) if a != mixed[0]]
            forms.append(form_index(mixed[0], int(neg[0, others[0]]) + 2 * int(neg[0, others[1]])))
    return forms, lanes, hits


def call_pairs(first, count):
    """The first frames of a call's two-frame groups."""
    return [first + 2 * i for i in range(count // 2)]
