"""Radius lists (lt_hip_nearest_list): what tests/test_nearest_lists_cpu.py and tests/test_gpu_nearest_lists.py share.  The
reference is the numpy model of the k-nearest query -- tests/nearest_k.py's sequences with keep = the number of leaves, so that
every sequence is whole -- put into CSR by csr().  Every comparison is of bits: nearest.same on the records, array_equal on the
offsets.

* tuning(): kListScanTile and kListSortSpanHits as lens_trace_amd/csrc/lt_overlist.hpp has them: the tests' shapes move with a
  retune.
* model(scene, points): the whole sequences of a batch; csr(m): a model's Sequences -> (offsets uint64 [n + 1], items HIT_DTYPE
  [total]).
* row_points(lengths): points in front of overlap_lists.row_scene with exactly those numbers of triangles within their radius.
* fan(F): nearest_k.fan12 with F triangles; the point at its vertex has F candidates at d2 == +0."""
import os
import re

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import HIT_DTYPE, make_points
from tests import nearest as nr
from tests import nearest_k as nk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SENTINEL = 0x5a5a5a5a
FAN_VERTEX = nk.FAN_VERTEX


def tuning():
    text = open(os.path.join(ROOT, "lens_trace_amd", "csrc", "lt_overlist.hpp")).read()
    tile = re.search(r"constexpr uint32_t kListScanTile = (\d+);", text)
    span = re.search(r"constexpr uint32_t kListSortSpanHits = (\d+);", text)
    assert tile and span
    return int(tile.group(1)), int(span.group(1))


def leaves(scene):
    return len(nr.leaves(scene)[0])


def model(scene, points, chunk=256):
    return nk.sequences(scene, points, keep=max(1, leaves(scene)), chunk=chunk)


def csr(m):
    """A Sequences whose keep covers every sequence -> (offsets, items)."""
    assert int(m.count.max(initial=0)) <= m.prim.shape[1]
    offsets = np.zeros(len(m.count) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(m.count.astype(np.uint64))
    used = np.arange(m.prim.shape[1])[None, :] < m.count[:, None]
    assert (m.prim[used] >= 0).all() and (m.prim[~used] == -1).all()
    items = np.zeros(int(offsets[-1]), dtype=HIT_DTYPE)
    items["t"], items["prim"], items["u"], items["v"] = m.d2[used], m.prim[used], m.u[used], m.v[used]
    return offsets, items


def segments(lists):
    offsets, items = lists
    return [items[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def gather(lists, order):
    """The lists of the batch's queries `order`, in that order."""
    segs = [segments(lists)[i] for i in order]
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in segs])]).astype(np.uint64)
    return offsets, (np.concatenate(segs) if segs else np.zeros(0, dtype=HIT_DTYPE))


def differ(got, want):
    """Why two lists differ, or None: the dtypes, the offsets word for word, the records bit for bit."""
    (go, gi), (wo, wi) = got, want
    if go.dtype != np.uint64 or gi.dtype != HIT_DTYPE or go.shape != wo.shape:
        return "dtypes or shapes", go.dtype, gi.dtype, go.shape, wo.shape
    if not np.array_equal(go, wo):
        return "offsets", np.flatnonzero(go != wo)[:5]
    if len(gi) != len(wi):
        return "records", len(gi), len(wi)
    bad = nr.same(gi, wi)
    return ("records", bad[:5]) if len(bad) else None


def sorted_by_d2_and_prim(seg):
    """Whether a segment's records ascend by (d2, prim)."""
    d, p = seg["t"][1:], seg["prim"][1:]
    e, q = seg["t"][:-1], seg["prim"][:-1]
    return bool(((e < d) | ((e == d) & (q <= p))).all())


def row_points(lengths):
    """The point (-0.5, 0, 0) in front of overlap_lists.row_scene with max_d2 = float32(L^2): triangle i is i + 0.5 away, so
    exactly the L triangles at x = 0 .. L - 1 are within the radius (L = 0: max_d2 = 0, a point that takes no walk)."""
    L = np.asarray(lengths, dtype=np.float64)
    return make_points(np.tile(F32([-0.5, 0.0, 0.0]), (len(L), 1)), (L * L).astype(F32))


def fan(F):
    """nearest_k.fan12 generalised: F triangles (V, R_i, R_i+1) round V = (0.5, 0.25, 1); triangle i lists its corners rotated by
    i % 3, so V takes turns being positionA, positionC and positionB; R_i lies at angle a = 2 pi i / F, radius 1 + 0.5 (i % 3) and
    height 0.25 cos 3a.  Every coordinate is a multiple of 2^-12, so B - A and C - A are exact and the point at V has d2 == +0
    to every triangle."""
    V = np.array([0.5, 0.25, 1.0])
    i = np.arange(F)
    ang = 2.0 * np.pi * i / F
    radius = 1.0 + 0.5 * (i % 3)
    ring = V + np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.25 * np.cos(3.0 * ang)], axis=1)
    ring = np.round(ring * 4096.0) / 4096.0
    pos = np.zeros((F, 3, 3), dtype=F32)
    for k in range(F):
        pos[k] = np.roll(np.array([V, ring[k], ring[(k + 1) % F]]), k % 3, axis=0)
    nrm = np.zeros_like(pos)
    nrm[..., 2] = 1.0
    mats = np.zeros(1, dtype=sc.MATERIAL_DTYPE)
    mats["diffuse"], mats["ior"], mats["dissolve"] = 0.5, 1.0, 1.0
    return sc.build_from_triangles(pos, nrm, np.zeros(F, dtype=np.int32), mats).validate()
