"""The scenes on which the point and box queries (lt_hip_nearest_points, lt_hip_nearest_k, lt_hip_overlap_boxes) meet every shape
of tree the library makes, with their batches and the models' answers: what tests/test_query_shapes_cpu.py and
tests/test_gpu_query_shapes.py compare the host forms and the kernels with.  numpy only; every comparison is of words.

* NAMES, scene(name): the list -- a root group with one to four filled slots and the first second-level group (random1 ..
  random5), the builder's boundaries (random17: more than one level of groups; random64 / random65: one wavefront per subtree
  against one per range; random2049: many workgroups), shared centroids and repeated triangles, leaves of three primitives, a
  primitive that two leaves name (no own tree, and the only scene with equal offsets in a sequence), +-0, denormal and
  2^40 - ulp leaf bounds on a flat axis, a wall with soup around it.  Built once per process, never modified.
* EDIT: the scene of tests/test_gpu_scene_history.py's edit of the primitives, before and after; both share one pair of batches.
* points(name), boxes(name): tests/nearest_k.py's and tests/overlap.py's families at n = 48, 624 points and 458 boxes.
* expected(name): the models' answers of every kind (KINDS), kept; expected(name, pidx, bidx) the same for the batches indexed.
* every_kind(...): the same kinds asked of an implementation; differing(got, want): the kinds whose words differ.
* OWN_TREE, OWN_TREE_CALLERS_SPLITS: whether the library gives the scene an own tree (tests/test_query_shapes_cpu.py computes
  them with the host builder; tests/test_gpu_query_shapes.py holds lt_hip_get_stats against them)."""
import functools

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from tests import multihit_edges as me
from tests import nearest as nr
from tests import nearest_k as nk
from tests import overlap as ov
from tests.test_gpu_device_prep import random_triangles
from tests.test_structures_cpu import edge_scene, multi_primitive_leaf_scene

N = 48          # the families' n: 624 points and 458 boxes per scene
KS = (1, 3, 8)
RANDOM = (1, 2, 3, 4, 5, 17, 64, 65, 2049)
NAMES = tuple("random%d" % n for n in RANDOM) + ("coincident", "multi", "twice", "edge", "mixed")
EDIT = ("edit_base", "edit_moved")
KINDS = (("nearest_points",) + tuple("nearest_k%d" % k for k in KS) + ("nearest_count",) + tuple("overlap_k%d" % k for k in KS) +
         ("overlap_count", "overlap_any"))
POINT_KINDS = tuple(k for k in KINDS if k.startswith("nearest"))

# Whether lt_hip_set_scene gives the scene its own tree (lt_hip_get_stats: own_tree_height > 0) or scans / walks the caller's
# (-1): a tree of one leaf has nothing to build, and two leaves on one primitive get no group records.
OWN_TREE = {name: name not in ("random1", "twice") for name in NAMES}
OWN_TREE_CALLERS_SPLITS = {name: True for name in ("random5", "random65", "multi", "edge", "mixed")}   # LT_RETREE=0


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("random"):
        n = int(name[len("random"):])
        return random_triangles(n, n)
    if name == "coincident":
        return random_triangles(7, 300, coincident=64)
    if name == "multi":
        return multi_primitive_leaf_scene()
    if name == "twice":
        return me.twice_named_scene()[0]
    if name == "edge":
        return edge_scene()
    if name == "mixed":
        return synth.wall_and_soup(12, 600).validate()
    if name == "edit_base":
        return random_triangles(4, 2049)
    if name == "edit_moved":
        # tests/test_gpu_scene_history.py, test_an_edit_of_the_primitives_remakes_the_leaf_records_alone: the same nodes
        base = scene("edit_base")
        prims = base.prim_view.copy()
        rng = np.random.default_rng(5)
        for k in ("positionA", "positionB", "positionC"):
            prims[k] += rng.normal(0, 0.01, prims[k].shape).astype(np.float32)
        return sc.Scene(nodes=base.nodes, prims=prims.view(np.uint8).reshape(-1), materials=base.materials, lights=base.lights, camera=base.camera)
    raise KeyError(name)


def batch_scene(name):
    """The scene whose families the batches of `name` are: its own, but for the edited scene its base's."""
    return "edit_base" if name == "edit_moved" else name


def seed(name):
    return (NAMES + EDIT).index(batch_scene(name))


@functools.lru_cache(maxsize=None)
def points(name):
    """(624, 4) float32 lt_hip_point records, read-only."""
    if name != batch_scene(name):
        return points(batch_scene(name))
    return frozen(np.ascontiguousarray(np.concatenate(list(nk.families(scene(name), seed=seed(name), n=N).values()))))


@functools.lru_cache(maxsize=None)
def boxes(name):
    """(458, 8) float32 lt_hip_box records, read-only."""
    if name != batch_scene(name):
        return boxes(batch_scene(name))
    return frozen(np.ascontiguousarray(np.concatenate(list(ov.families(scene(name), seed=seed(name), n=N).values()))))


def whole_box(name):
    """Index into boxes(name) of the box that holds the whole scene (the first of family g_whole)."""
    fam = ov.families(scene(batch_scene(name)), seed=seed(name), n=N)
    at = 0
    for key, b in fam.items():
        if key == "g_whole":
            return at
        at += len(b)
    raise KeyError("g_whole")


@functools.lru_cache(maxsize=None)
def point_sequences(name):
    return nk.sequences(scene(name), points(name))


@functools.lru_cache(maxsize=None)
def box_sequences(name):
    return ov.sequences(scene(name), boxes(name))


@functools.lru_cache(maxsize=None)
def _expected(name):
    s = scene(name)
    ps, bs = point_sequences(name), box_sequences(name)
    want = {"nearest_points": nr.expected(s, points(name)), "nearest_count": ps.count, "overlap_count": bs.count, "overlap_any": bs.any}
    for k in KS:
        want["nearest_k%d" % k] = ps.records(k)
        want["overlap_k%d" % k] = bs.first(k)
    return {kind: frozen(np.ascontiguousarray(want[kind])) for kind in KINDS}


def expected(name, pidx=None, bidx=None):
    """kind -> the model's answers for points(name)[pidx] and boxes(name)[bidx] (None: the whole batch)."""
    want = _expected(name)
    out = {}
    for kind, a in want.items():
        idx = pidx if kind in POINT_KINDS else bidx
        out[kind] = a if idx is None else np.ascontiguousarray(a[idx])
    return out


def every_kind(nearest_points, nearest_k, overlap_boxes, pts, bxs, kinds=KINDS):
    """kind -> what the three callables (RendererHIP's methods, or the _host forms with the scene bound) give for the batches."""
    got = {}
    for kind in kinds:
        if kind == "nearest_points":
            got[kind] = nearest_points(pts)
        elif kind == "nearest_count":
            got[kind] = nearest_k(pts, count=True)
        elif kind.startswith("nearest_k"):
            got[kind] = nearest_k(pts, k=int(kind[len("nearest_k"):]))
        elif kind == "overlap_count":
            got[kind] = overlap_boxes(bxs, count=True)
        elif kind == "overlap_any":
            got[kind] = overlap_boxes(bxs, any=True)
        else:
            got[kind] = overlap_boxes(bxs, k=int(kind[len("overlap_k"):]))
    return got


def words(a):
    """The answer's bytes as uint32, flat: numpy of the host forms, torch of the device forms."""
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def as_words(got):
    """kind -> flat uint32 copies: what a test keeps of a context's answers to compare bytes later."""
    return {kind: words(a).copy() for kind, a in got.items()}


def differing(got, want):
    """[(kind, words that differ, the first few of them)] over the kinds of `got`; empty: the same words everywhere."""
    bad = []
    for kind, a in got.items():
        g, w = words(a), words(want[kind])
        if g.shape != w.shape:
            bad.append((kind, "sizes", g.shape, w.shape))
            continue
        at = np.flatnonzero(g != w)
        if len(at):
            bad.append((kind, len(at), at[:4].tolist(), g[at[:4]].tolist(), w[at[:4]].tolist()))
    return bad


def repeated(n, m, rng_seed):
    """m indices into a batch of n by repetition, shuffled."""
    return np.random.default_rng(rng_seed).permutation(np.resize(np.arange(n), m))


def named_offsets(s):
    """The primitive offsets the leaves of the scene name."""
    return np.unique(nr.leaves(s)[0])
