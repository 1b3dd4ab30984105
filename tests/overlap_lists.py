"""Overlap lists (lt_hip_overlap_boxes_list, lt_hip_overlap_tris_list): what tests/test_overlap_lists_cpu.py and
tests/test_gpu_overlap_lists.py share.  The reference is the numpy model of the two queries -- tests/overlap.py's and
tests/overlap_tris.py's sequences with keep = the number of leaves, so that every sequence is whole -- put into CSR by csr().

* tuning(): kListScanTile and kListSortSpan as lens_trace_amd/csrc/lt_overlist.hpp has them: the tests' shapes move with a retune.
* csr(m): a model's Sequences -> (offsets uint64 [n + 1], items int32 [total]).
* model_boxes / model_tris(scene, records): the whole sequences of a batch.
* row_scene(n, seed): n small triangles at x = 0, 1, 2 .., in a shuffled primitive order; row_boxes(lengths): boxes with exactly
  those numbers of members."""
import os
import re

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import make_boxes
from tests import nearest as nr
from tests import overlap as ov
from tests import overlap_tris as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5a5a5a5a


def tuning():
    text = open(os.path.join(ROOT, "lens_trace_amd", "csrc", "lt_overlist.hpp")).read()
    tile = re.search(r"constexpr uint32_t kListScanTile = (\d+);", text)
    span = re.search(r"constexpr uint32_t kListSortSpan = (\d+);", text)
    assert tile and span
    return int(tile.group(1)), int(span.group(1))


def leaves(scene):
    return len(nr.leaves(scene)[0])


def csr(m):
    """A Sequences whose keep covers every sequence -> (offsets, items)."""
    assert int(m.count.max(initial=0)) <= m.prim.shape[1]
    offsets = np.zeros(len(m.count) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(m.count.astype(np.uint64))
    used = np.arange(m.prim.shape[1])[None, :] < m.count[:, None]
    assert (m.prim[used] >= 0).all() and (m.prim[~used] == -1).all()
    return offsets, np.ascontiguousarray(m.prim[used], dtype=np.int32)


def model_boxes(scene, boxes):
    return ov.sequences(scene, boxes, keep=max(1, leaves(scene)))


def model_tris(scene, tris):
    return ot.sequences(scene, tris, keep=max(1, leaves(scene)))


def row_scene(n, seed=0):
    """Triangle i of the row: (i, 0, 0), (i + 0.25, 0, 0), (i, 0.25, 0) -- then the primitives are shuffled, so that a walk in
    space order meets the offsets out of order.  Returns the scene and x: the row position of every primitive offset."""
    pos = np.zeros((n, 3, 3), dtype=np.float32)
    pos[:, :, 0] = np.arange(n)[:, None]
    pos[:, 1, 0] += 0.25
    pos[:, 2, 1] = 0.25
    nrm = np.zeros_like(pos)
    nrm[:, :, 2] = 1.0
    m = np.zeros(1, dtype=sc.MATERIAL_DTYPE)
    m["ior"], m["dissolve"], m["diffuse"] = 1.45, 1.0, (0.8, 0.8, 0.8)
    s = sc.build_from_triangles(pos, nrm, np.zeros(n, dtype=np.int32), m)
    # the build puts the primitives in the order of its leaves: move primitive o to a random offset and rename it in its leaf
    to = np.random.default_rng(seed).permutation(n).astype(np.int32)
    prims = s.prim_view.copy()
    prims[to] = s.prim_view
    nodes = s.node_view.copy()
    leaf = nodes["primitiveCount"] > 0
    assert (nodes["primitiveCount"][leaf] == 1).all() and s.light_view[0]["count"] == 0
    nodes["offset"][leaf] = to[nodes["offset"][leaf]]
    s = sc.Scene(nodes.view(np.uint8).reshape(-1), prims.view(np.uint8).reshape(-1), s.materials, s.lights, s.camera).validate()
    return s, s.prim_view["positionA"][:, 0].astype(np.float64)


def row_boxes(lengths):
    """[-0.5, L - 0.5] in x, [-1, 1] in y and z: the L triangles at x = 0 .. L - 1 (L = 0: a box in front of the row)."""
    L = np.asarray(lengths, dtype=np.float64)
    lo = np.stack([np.where(L > 0, -0.5, -3.0), -np.ones(len(L)), -np.ones(len(L))], axis=1)
    hi = np.stack([np.where(L > 0, L - 0.5, -2.0), np.ones(len(L)), np.ones(len(L))], axis=1)
    return make_boxes(lo, hi)
