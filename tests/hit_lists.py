"""Fixtures of the hit-list tests (tests/test_gpu_hit_lists.py; what each of them claims: tests/test_hit_lists_cpu.py), on top of
tests/multihit.py (the peeling oracle, the sheets, the Cornell rays) and tests/multihit_edges.py (the tie rays, query_edges'
families, the twice-named scene).

lt_hip_trace_hits_list (include/lenstrace_hip.h) returns the WHOLE hit sequence of every ray as CSR: offsets[n + 1] in uint64 and
items[offsets[n]] lt_hip_hit records.

* csr(seqs): the lists of a batch whose sequences the oracle peeled; differ(got, want): the first difference in any bit;
* batch(name), sequences(name): the three batches the oracle is held against -- the sheets, the Cornell box, the tie rays;
* stack_scene(), stack_rays(): stack_sheets() = 2 kListSortSpanHits + 64 parallel triangles, one primitive per hit, and rays along
  a few lines through all of them whose tmax lies between two sheets, so that the segment lengths are stack_lengths(); the
  expected sequence of a ray is the prefix with t < tmax of its line's whole sequence (tests/test_hit_lists_cpu.py checks that
  rule where the peeler can afford both);
* tuning(): kListScanTile and kListSortSpanHits as lt_overlist.hpp has them."""
import functools
import os
import re

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import FLT_MAX, HIT_DTYPE, make_rays
from oracle import pyoracle as po
from tests import multihit as mh
from tests import multihit_edges as me

F32 = np.float32
SENTINEL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def tuning():
    """(kListScanTile, kListSortSpanHits) read from lt_overlist.hpp."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lens_trace_amd", "csrc", "lt_overlist.hpp")
    text = open(path).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % k, text).group(1)) for k in ("kListScanTile", "kListSortSpanHits"))


# ------------------------------------------------------------------------------------------------------------------ the lists
def csr(seqs):
    """(offsets, items) of a batch from its sequences (lists of (t, prim, u, v))."""
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    items = np.zeros(int(offsets[-1]), dtype=HIT_DTYPE)
    at = 0
    for s in seqs:
        for h in s:
            items[at] = h
            at += 1
    return offsets, items


def segments(lists):
    offsets, items = lists
    return [items[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def gather(lists, order):
    """The lists of the batch's rays `order`, in that order."""
    seg = segments(lists)
    offsets = np.zeros(len(order) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(seg[i]) for i in order], dtype=np.uint64)
    items = np.concatenate([seg[i] for i in order]) if len(order) else np.zeros(0, dtype=HIT_DTYPE)
    return offsets, items.astype(HIT_DTYPE)


def words(items):
    return np.ascontiguousarray(items).view(np.uint32).reshape(-1, 4)


def differ(got, want):
    """None when the offsets and all four fields of every record agree bit for bit, else where they first do not."""
    go, gi = got
    wo, wi = want
    go, wo = np.asarray(go).view(np.uint64), np.asarray(wo).view(np.uint64)
    if go.shape != wo.shape:
        return "offsets: %s words for %s" % (go.shape, wo.shape)
    bad = np.flatnonzero(go != wo)
    if len(bad):
        return "offsets[%d] = %d, not %d (%d differ)" % (bad[0], go[bad[0]], wo[bad[0]], len(bad))
    if gi.dtype != HIT_DTYPE or len(gi) != len(wi):
        return "items: %s of %s for %d records" % (gi.shape, gi.dtype, len(wi))
    bad = np.flatnonzero((words(gi) != words(wi)).any(axis=1))
    if len(bad):
        ray = int(np.searchsorted(wo, bad[0], side="right")) - 1
        return "record %d (ray %d, hit %d) = %s, not %s (%d differ)" % (bad[0], ray, bad[0] - int(wo[ray]), gi[bad[0]], wi[bad[0]], len(bad))
    return None


# ---------------------------------------------------------------------------------------------------------------- the batches
def batch(name):
    """(scene, rays) of "sheets", "cornell" or "ties"."""
    if name == "sheets":
        return mh.sheets_scene(), mh.sheet_rays()[0]
    if name == "cornell":
        return mh.cornell_rays()
    assert name == "ties"
    return mh.sheets_scene(), me.dyadic_rays()[0]


def sequences(name, program=po.ACCUMULATOR):
    """The peeled sequences of batch(name), shared with the multi-hit tests' (tests/multihit.py keeps them per name and program)."""
    s, rays = batch(name)
    return mh.sequences({"ties": "dyadic"}.get(name, name), s, rays, program)


def octants(rays):
    """The direction-sign octant of each ray as own_ray computes it: the signs of 1 / direction (-0 counts as negative)."""
    d = np.asarray(rays)[:, 4:7]
    neg = np.signbit(d) & ~np.isnan(d)
    return neg[:, 0] * 1 + neg[:, 1] * 2 + neg[:, 2] * 4


# ------------------------------------------------------------------------------------------------------------------ the stack
STACK_GAP = 0.25
STACK_LINES = 4


def stack_sheets():
    return 2 * tuning()[1] + 64


def stack_lengths():
    span, n = tuning()[1], stack_sheets()
    return (0, 1, 2, 63, 64, 65, span - 1, span, span + 1, n, 3, 127, 128, 129, span // 2, span + span // 2, 2 * span - 1, 2 * span, 2 * span + 1,
            n - 1)


def stack_triangles(n):
    z = (np.arange(n) * STACK_GAP).astype(F32)
    pos = np.zeros((n, 3, 3), dtype=F32)
    pos[:, 0, :2], pos[:, 1, :2], pos[:, 2, :2] = (-8.0, -8.0), (8.0, -8.0), (0.0, 8.0)
    pos[:, :, 2] = z[:, None]
    return pos


def scene_of_triangles(pos, seed):
    """The scene of these triangles, handed to the builder in a shuffled order."""
    pos = pos[np.random.default_rng(seed).permutation(len(pos))]
    nrm = np.tile(F32([0, 0, -1]), (len(pos), 3, 1))
    m = np.zeros(1, dtype=sc.MATERIAL_DTYPE)
    m["diffuse"], m["ior"], m["dissolve"] = 0.5, 1.3, 1.0
    return sc.build_from_triangles(pos, nrm, np.zeros(len(pos), dtype=np.int32), m).validate()


@functools.lru_cache(maxsize=None)
def stack_scene(n=None):
    return scene_of_triangles(stack_triangles(stack_sheets() if n is None else n), 11)


def stack_lines(n):
    """STACK_LINES lines through all n sheets, one per octant of the upper or the lower half: (origins, directions)."""
    top = (n - 1) * STACK_GAP
    o = np.array([[-0.5, -0.25, -1.0], [0.75, -0.5, -1.5], [0.25, 0.5, top + 1.0], [-0.75, 0.25, top + 2.0]])
    d = np.array([[0.003, 0.002, 1.0], [-0.002, 0.004, 1.0], [0.001, -0.003, -1.0], [-0.004, -0.001, -1.0]])
    return o[:STACK_LINES], d[:STACK_LINES]


def rays_of_lengths(scene, n, lengths, program=po.ACCUMULATOR):
    """(rays, whole): for every line and every length L a ray on that line whose tmax lies between the line's hits L - 1 and L
    (L = 0: half the first t; L = n: FLT_MAX) -- ray len(lines) j + k has length lengths[j] on line k, so neighbouring rays lie on
    different lines and `lengths` decides which lengths share a wave; whole[k] is the peeled sequence of line k with tmax = FLT_MAX."""
    o, d = stack_lines(n)
    lines = make_rays(o, d)
    p = mh.Peeler(scene)
    whole = [p.peel(r, program) for r in lines]
    rays = []
    for j, L in enumerate(lengths):
        for k in range(len(lines)):
            t = np.array([h[0] for h in whole[k]], dtype=np.float64)
            assert len(t) == n and (np.diff(t) > 0).all() and t[0] > 0
            tmax = FLT_MAX if L == n else F32(0.5 * t[0]) if L == 0 else F32(0.5 * (t[L - 1] + t[L]))
            assert L == n or (L == 0 or t[L - 1] < tmax) and tmax < t[L]
            r = lines[k].copy()
            r[3] = tmax
            rays.append(r)
    rays = np.array(rays, dtype=F32)
    rays.setflags(write=False)
    return rays, whole


def prefix_sequences(rays, whole):
    """The expected sequence of each ray of rays_of_lengths: the hits of its line's whole sequence with t < tmax."""
    return [[h for h in whole[i % len(whole)] if h[0] < rays[i, 3]] for i in range(len(rays))]


@functools.lru_cache(maxsize=None)
def stack_rays():
    """(rays, expected sequences, lengths per ray) on stack_scene()."""
    n = stack_sheets()
    rays, whole = rays_of_lengths(stack_scene(), n, stack_lengths())
    lengths = np.repeat(stack_lengths(), STACK_LINES)
    return rays, prefix_sequences(rays, whole), lengths
