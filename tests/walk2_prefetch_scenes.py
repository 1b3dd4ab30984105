"""The scene tests/test_gpu_walk2_prefetch.py adds to those of tests/entry_cut_chunk_scenes.py, framed for the same camera.
scene(name) -> (scene, camera), for this name and for entry_cut_chunk_scenes'.

* shaded-field: the grazing field with one triangle in the plane y = 8.0, between the field (y <= 7.5) and the light (y = 8.2),
  that every segment from a point of the field to a point of the light passes through: the light spans x in [-5, 5], z in
  [-4, -2], the field z in [-0.5, 0.5], so the segment meets the plane at x in [-5, 5], z in [-4, 0), at least 0.2 short of its
  end (the walk's tmax stops 0.01 short), and the triangle covers x in [-15, 15] there.  It lies above the camera's view (y <= 7.8
  out to z = 8).  So every shadow ray of every frame is occluded, by this triangle if by nothing before it: a square's two-frame
  walk ends, both `open` masks empty, no later than at this triangle's leaf, wherever that leaf is in the square's list."""
import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from tests import entry_cut_chunk_scenes as cs

CAM = cs.CAM
NEW = ["shaded-field"]
SCENES = cs.SCENES + NEW
SIZES = cs.SIZES

SHADE = ((-30.0, 8.0, -8.0), (30.0, 8.0, -8.0), (0.0, 8.0, 8.0))

_scenes = {}


def shaded_field():
    wall = synth.heightfield_wall(cs.GRAZING_CELLS)
    pv = wall.prim_view
    n = len(pv) - 2     # (the wall's own light: its last two triangles)
    P = np.stack([pv["positionA"][:n, :3], pv["positionB"][:n, :3], pv["positionC"][:n, :3]], axis=1)
    N = np.stack([pv["normalA"][:n, :3], pv["normalB"][:n, :3], pv["normalC"][:n, :3]], axis=1)
    lp, ln = synth._light_quad(*cs.GRAZING_LIGHT)
    mats = synth._materials([(0.8, 0.8, 0.8)])
    mi = np.concatenate([np.zeros(n + 1, np.int32), np.full(2, 1, np.int32)])
    shade_p, shade_n = np.float32([SHADE]), np.tile(np.float32([0, -1, 0]), (1, 3, 1))
    return sc.build_from_triangles(np.concatenate([P, shade_p, lp]).astype(np.float32), np.concatenate([N, shade_n, ln]).astype(np.float32), mi,
                                   mats).validate()


def shade_primitive(s):
    """The index of the shading triangle among the scene's primitives."""
    pv = s.prim_view
    V = np.stack([pv["positionA"][:, :3], pv["positionB"][:, :3], pv["positionC"][:, :3]], axis=1).astype(np.float32)
    found = [i for i in range(len(V)) if sorted(map(tuple, V[i].tolist())) == sorted(map(tuple, np.float32(SHADE).tolist()))]
    assert len(found) == 1
    return found[0]


def scene(name):
    """(scene, camera)"""
    if name not in NEW:
        return cs.scene(name)
    if name not in _scenes:
        _scenes[name] = (shaded_field(), CAM)
    return _scenes[name]
