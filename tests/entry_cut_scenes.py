"""Scenes of the entry cut's tests (tests/test_gpu_entry_cut.py; the wide-light construction itself: tests/test_entry_cut_scenes_cpu.py):
synth.heightfield_wall(24) and two edits of it that leave its nodes alone, the Cornell golden scene, every scene of
tests/mixed_axis_scenes.py, and three of their own over tests/penumbra_scenes.py's floor -- two lights far apart, a light in the
floor's own plane y = 0 beside one above, and a wide light whose outer quarter alone is hidden by an occluder.  scene(name) ->
(scene, camera)."""
import dataclasses
import os

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from tests import mixed_axis_scenes as mx
from tests import penumbra_scenes as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
SIZES = ((24, 16), (17, 9), (9, 9))

_scenes = {}


def _flat_scene(lights, extra=()):
    """ps's floor, the given light quads (x0, x1, y, z0, z1) and a few occluder triangles."""
    fp, fn = ps.floor_triangles()
    P, N, M = [fp], [fn], [0, 0]
    _, _, _, m = ps.penumbra_triangles((0.0, 2.5, 0.0))
    for x0, x1, y, z0, z1 in lights:
        P.append(np.float32([[[x0, y, z0], [x1, y, z0], [x1, y, z1]], [[x0, y, z0], [x1, y, z1], [x0, y, z1]]]))
        N.append(np.tile(np.float32([0, -1, 0]), (2, 3, 1)))
        M += [2, 2]
    for t in extra:
        P.append(np.float32([t]))
        N.append(np.tile(np.float32([0, 0, -1]), (1, 3, 1)))
        M.append(1)
    return sc.build_from_triangles(np.concatenate(P), np.concatenate(N), np.int32(M), m).validate()


def _plane_scene():
    """A floor in the plane y = 0 (every camera hit on it has y = +0 exactly), a light in that plane beyond it, a light above, two
    occluders standing on the floor."""
    a, b, c, d = (-12.0, 0.0, -24.0), (12.0, 0.0, -24.0), (12.0, 0.0, 60.0), (-12.0, 0.0, 60.0)
    P = [np.float32([[a, b, c], [a, c, d]])]
    N = [np.tile(np.float32([0, 1, 0]), (2, 3, 1))]
    M = [0, 0]
    _, _, _, m = ps.penumbra_triangles((0.0, 2.5, 0.0))
    for quad in (((-2.0, 0.0, 62.0), (2.0, 0.0, 62.0), (2.0, 0.0, 64.0), (-2.0, 0.0, 64.0)), ((-1.0, 9.0, -3.0), (1.0, 9.0, -3.0), (1.0, 9.0, -1.0), (-1.0, 9.0, -1.0))):
        P.append(np.float32([[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]))
        N.append(np.tile(np.float32([0, -1, 0]), (2, 3, 1)))
        M += [2, 2]
    for t in (((-1.0, 0.0, 30.0), (1.0, 0.0, 30.0), (0.0, 1.5, 30.0)), ((-0.5, 3.0, 0.0), (0.5, 3.0, 0.0), (0.0, 3.0, 1.0))):
        P.append(np.float32([t]))
        N.append(np.tile(np.float32([0, 0, -1]), (1, 3, 1)))
        M.append(1)
    return sc.build_from_triangles(np.concatenate(P), np.concatenate(N), np.int32(M), m).validate()


# A light forty units wide over ps's floor and one small occluder that hides only its outer quarter: on the way from the floor's
# middle to the light point at x = 18.  A cut made for a light box half as wide (x in [-10, 10]) does not hold the occluder --
# at the parameter where a ray passes its height, no ray towards that box is further out than x = 7 -- and the floor would stay lit
# where tests/test_entry_cut_scenes_cpu.py finds it shadowed.
WIDE_LIGHT = (-20.0, 20.0, 13.0, -16.0, -14.0)
WIDE_TARGET, WIDE_LIGHT_POINT, WIDE_AT, WIDE_HALF = np.array([0.0, 2.5, 0.0]), np.array([18.0, 13.0, -15.0]), 0.65, 0.45


def wide_light_occluder():
    axis = WIDE_LIGHT_POINT - WIDE_TARGET
    c = WIDE_TARGET + WIDE_AT * axis
    axis = axis / np.linalg.norm(axis)
    u = np.cross(axis, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(axis, u)
    return tuple(tuple(p) for p in (c + WIDE_HALF * (-u - 0.6 * v), c + WIDE_HALF * (u - 0.6 * v), c + WIDE_HALF * 1.2 * v))


def scene(name):
    """(scene, camera)"""
    if name not in _scenes:
        if name == "wall":
            _scenes[name] = (synth.heightfield_wall(24).validate(), CAM)
        elif name == "wall-edited-prims":   # other normals on its first primitives: same nodes, an edit through lt_hip_set_scene
            w = scene("wall")[0]
            prims = np.array(w.prims, dtype=np.uint8, copy=True)
            prims.view(np.float32).reshape(-1, 19)[:16, 9:18] = np.float32(0.5)
            _scenes[name] = (dataclasses.replace(w, prims=prims).validate(), CAM)
        elif name == "wall-edited-lights":  # one light triangle of its two
            w = scene("wall")[0]
            lights = np.array(w.lights, dtype=np.uint8, copy=True)
            assert lights.view(sc.LIGHT_DTYPE)["count"][0] == 2
            lights.view(sc.LIGHT_DTYPE)["count"][0] = 1
            _scenes[name] = (dataclasses.replace(w, lights=lights).validate(), CAM)
        elif name == "cornell":
            _scenes[name] = (sc.load_ltsb(os.path.join(ROOT, "tests", "golden", "cornell_box_O0.ltsb")).validate(), CAM)
        elif name.startswith("mixed-"):
            axis, k = "xyz".index(name[6]), int(name[7])
            _scenes[name] = (mx.mixed_scene(axis, k), mx.camera(mx.form_index(axis, k), 1))
        elif name == "two-axes":
            _scenes[name] = (mx.two_axis_scene(), mx.camera(0, 1))
        elif name.startswith("penumbra-"):
            _scenes[name] = (mx.penumbra_scene(name[9:]), ps.CAM)
        elif name == "two-lights":
            occ = [((-1.0, 4.0, -2.0), (1.0, 4.0, -2.0), (0.0, 5.0, -1.0)), ((2.0, 6.0, 4.0), (3.0, 6.0, 4.0), (2.5, 7.0, 5.0))]
            _scenes[name] = (_flat_scene([(8.0, 10.0, 13.0, -16.0, -14.0), (-60.0, -58.0, 40.0, 30.0, 32.0)], occ), ps.CAM)
        elif name in ("wide-light", "wide-light-bare"):
            _scenes[name] = (_flat_scene([WIDE_LIGHT], [] if name.endswith("bare") else [wide_light_occluder()]), ps.CAM)
        elif name == "light-in-plane":
            _scenes[name] = (_plane_scene(), CAM)
        else:
            raise KeyError(name)
    return _scenes[name]


MIXED = ["mixed-%s%d" % ("xyz"[a], k) for a, k in mx.FORMS]
SCENES = ["wall", "cornell"] + MIXED + ["two-axes", "two-lights", "light-in-plane", "wide-light"]
