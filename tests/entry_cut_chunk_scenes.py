"""The scene of the tests of entry cuts that take several records (tests/test_gpu_entry_cut_chunks.py; the construction itself:
tests/test_entry_cut_chunks_cpu.py), beside those of tests/entry_cut_leaf_scenes.py.  Framed for the reference camera, whose view at
z = 0 spans x in [-4.5, 4.5], y in [-2, 7].  scene(name) -> (scene, camera), for this name and for entry_cut_leaf_scenes'.

* grazing-field: synth.heightfield_wall's surface with GRAZING_CELLS cells a side under a light as wide as the wall, low over its
  upper edge: the lines from a square's pixels towards it run along the wall, over dozens of its triangles.  From 20 to some 240
  leaves survive the leaf pass in all but one square of the tests' sizes (surviving_leaves below counts them on the CPU with the
  library's own host-compiled tests; 24x16: 75 - 116, 17x9: 20 - 159, 9x9: 3 - 242): more than one 64-byte record holds, in some
  squares fewer than two records hold, in others more than eight."""
import ctypes
import dataclasses

import numpy as np

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from tests import entry_cut_leaf_scenes as ls
from tests import mixed_axis_scenes as mx

CAM = ls.CAM
NEW = ["grazing-field"]
EDITED = ["grazing-field-edited-prims", "grazing-field-edited-lights"]     # (edits through lt_hip_set_scene that leave the nodes alone)
SCENES = ls.SCENES + NEW
SIZES = ls.SIZES

GRAZING_CELLS = 20
GRAZING_LIGHT = (-5.0, 5.0, 8.2, -4.0, -2.0)      # x0, x1, y, z0, z1 (synth._light_quad)

_scenes = {}


def grazing_field(cells=GRAZING_CELLS, light=GRAZING_LIGHT):
    wall = synth.heightfield_wall(cells)
    pv = wall.prim_view
    n = len(pv) - 2     # (the wall's own light: its last two triangles)
    P = np.stack([pv["positionA"][:n, :3], pv["positionB"][:n, :3], pv["positionC"][:n, :3]], axis=1)
    N = np.stack([pv["normalA"][:n, :3], pv["normalB"][:n, :3], pv["normalC"][:n, :3]], axis=1)
    lp, ln = synth._light_quad(*light)
    mats = synth._materials([(0.8, 0.8, 0.8)])
    mi = np.concatenate([np.zeros(n, np.int32), np.full(2, 1, np.int32)])
    return sc.build_from_triangles(np.concatenate([P, lp]).astype(np.float32), np.concatenate([N, ln]).astype(np.float32), mi, mats).validate()


def scene(name):
    """(scene, camera)"""
    if name not in NEW + EDITED:
        return ls.scene(name)
    if name not in _scenes:
        if name == "grazing-field":
            _scenes[name] = (grazing_field(), CAM)
        elif name == "grazing-field-edited-prims":     # four rows of triangles shrunk to half towards their first vertex (inside their boxes: same nodes)
            g = scene("grazing-field")[0]
            prims = np.array(g.prims, dtype=np.uint8, copy=True)
            rows = prims.view(np.float32).reshape(-1, 19)
            strip = slice(GRAZING_CELLS * GRAZING_CELLS, GRAZING_CELLS * GRAZING_CELLS + 8 * GRAZING_CELLS)
            for v in (3, 6):
                rows[strip, v:v + 3] = (rows[strip, 0:3] + rows[strip, v:v + 3]) * np.float32(0.5)
            _scenes[name] = (dataclasses.replace(g, prims=prims).validate(), CAM)
        else:                                          # one light triangle of its two
            g = scene("grazing-field")[0]
            lights = np.array(g.lights, dtype=np.uint8, copy=True)
            assert lights.view(sc.LIGHT_DTYPE)["count"][0] == 2
            lights.view(sc.LIGHT_DTYPE)["count"][0] = 1
            _scenes[name] = (dataclasses.replace(g, lights=lights).validate(), CAM)
    return _scenes[name]


def _host_test(fn, o, L, third):
    n = o.shape[0]
    out = np.zeros(n, np.uint8)
    o, L, third = (np.ascontiguousarray(a, np.float32) for a in (o, L, third))
    rc = fn(o.ctypes.data_as(ctypes.c_void_p), L.ctypes.data_as(ctypes.c_void_p), third.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
            out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def surviving_leaves(s, cam, W, H):
    """Per 8x8 square (row-major), the triangles that some casting pixel of the square which does not lie on them may reach (the
    triangle's own box) and may accept: what the leaf pass of lt_entry_cut_kernel keeps, but for the boxes above the leaves, by the
    library's host-compiled may_reach and may_accept."""
    lib = C.load()
    has, pos, _, prims = mx.camera_hits(s, cam, W, H)
    pv, lv = s.prim_view, s.light_view[0]
    lights = [int(p) for p in lv["primitives"][:int(lv["count"])]]
    V = np.stack([pv["positionA"][:, :3], pv["positionB"][:, :3], pv["positionC"][:, :3]], axis=1).astype(np.float32)
    lverts = V[lights].reshape(-1, 3)
    L = np.concatenate([lverts.min(axis=0), lverts.max(axis=0)])
    boxes = np.concatenate([V.min(axis=1), V.max(axis=1)], axis=1)
    tris = np.concatenate([V[:, 0], V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]], axis=1)
    counts = []
    for y0 in range(0, H, 8):
        for x0 in range(0, W, 8):
            keep = np.zeros(len(V), bool)
            for y in range(y0, min(y0 + 8, H)):
                for x in range(x0, min(x0 + 8, W)):
                    if not has[y, x]:
                        continue
                    o = np.broadcast_to(pos[y, x], (len(V), 3))
                    LL = np.broadcast_to(L, (len(V), 6))
                    ok = (_host_test(lib.lt_hip_entry_cut_test_host, o, LL, boxes) == 1) & (_host_test(lib.lt_hip_entry_cut_triangle_test_host, o, LL, tris) == 1)
                    ok[int(prims[y, x])] = False
                    keep |= ok
            counts.append(int(keep.sum()))
    return counts
