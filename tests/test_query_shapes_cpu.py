"""CPU checks (no GPU) of tests/query_shapes.py, the scenes on which tests/test_gpu_query_shapes.py runs the point and box queries:

* the three GPU-free forms (lt_hip_nearest_points_host, lt_hip_nearest_k_host, lt_hip_overlap_boxes_host) equal the numpy models
  word for word for every kind on every scene -- the models are what the kernels are then held against;
* the batches are not vacuous on any scene: counted from the models alone, these are conditions on the inputs, not on the library.
  Measured (624 points and 458 boxes per scene): 482 .. 503 points and 270 .. 332 boxes with a non-empty sequence; from 17 leaves
  on 380 .. 409 points with more than eight candidates; boxes with more than eight: 3 on random64, 4 on random65, 42 on random2049,
  69 on coincident, 58 on twice, 27 on mixed;
* the scene whose leaves name a primitive twice reports it twice, and neither it nor the scene with leaves of three primitives
  ever reports a primitive that no leaf names;
* the table of which scenes get an own tree is what the host builder says (lt_hip_own_hierarchy, then lt_hip_own_wide: the
  library takes the own structures all or none)."""
import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import nearest_k_host, nearest_points_host, overlap_boxes_host
from tests import nearest as nr
from tests import overlap as ov
from tests import query_shapes as qs


def leaf_count(name):
    return len(nr.leaves(qs.scene(name))[0])


def host_forms(name):
    s = qs.scene(name)
    return qs.every_kind(lambda p: nearest_points_host(s, p), lambda p, **kw: nearest_k_host(s, p, **kw),
                         lambda b, **kw: overlap_boxes_host(s, b, **kw), qs.points(name), qs.boxes(name))


@pytest.mark.parametrize("name", qs.NAMES + qs.EDIT)
def test_the_host_forms_equal_the_models(name):
    assert qs.points(name).shape == (624, 4) and qs.boxes(name).shape == (458, 8)
    got = host_forms(name)
    assert sorted(got) == sorted(qs.KINDS)
    assert qs.differing(got, qs.expected(name)) == []


@pytest.mark.parametrize("name", qs.NAMES)
def test_the_batches_are_not_vacuous(name):
    ps, bs = qs.point_sequences(name), qs.box_sequences(name)
    n = leaf_count(name)
    assert (ps.count > 0).sum() >= 256 and (bs.count > 0).sum() >= 256
    assert (ps.count == 0).sum() >= 64 and (bs.count == 0).sum() >= 64          # (misses, empty boxes and dead points among them)
    assert nr.no_walk(qs.points(name)).sum() >= 32 and ov.empty(qs.boxes(name)).sum() >= 32
    if n >= 17:
        assert (ps.count > 8).sum() >= 256
    if n >= 65:
        assert (bs.count > 8).sum() >= 3
    if name in ("random2049", "coincident", "twice", "mixed"):
        assert (bs.count > 8).sum() >= 24
    # the box that holds the whole scene touches every leaf
    assert bs.count[qs.whole_box(name)] == n


def test_the_list_covers_the_tree_shapes_it_names():
    assert [leaf_count("random%d" % n) for n in qs.RANDOM] == list(qs.RANDOM)
    assert leaf_count("multi") == 2 and qs.scene("multi").n_prims == 6
    assert leaf_count("coincident") == 300 and leaf_count("edge") == 8
    # one to four filled slots in the root's group, then the first second-level group
    for n, groups, filled in ((2, 1, 2), (3, 1, 3), (4, 1, 4), (5, 2, None)):
        s = qs.scene("random%d" % n)
        _, own, _ = C.own_hierarchy(s.node_view, s.n_prims, 2)
        slots = C.own_wide(own, s.n_prims)[3]
        assert len(slots) == groups
        if filled is not None:
            assert int((slots["link"][0] != (0x80000000 | (groups + s.n_prims))).sum()) == filled


@pytest.mark.parametrize("name", ("twice", "multi"))
def test_no_answer_names_a_primitive_that_no_leaf_names(name):
    s = qs.scene(name)
    named = qs.named_offsets(s)
    assert len(named) < s.n_prims                                                # (some primitive is named by no leaf)
    ps, bs = qs.point_sequences(name), qs.box_sequences(name)
    got = host_forms(name)
    for prims in (ps.prim, bs.prim, got["nearest_points"]["prim"], got["nearest_k8"]["prim"], got["overlap_k8"]):
        prims = np.asarray(prims).reshape(-1)
        assert np.isin(prims[prims >= 0], named).all()
    if name == "multi":
        assert named.tolist() == [0, 2]


def test_the_twice_named_primitive_is_reported_twice():
    s = qs.scene("twice")
    off = nr.leaves(s)[0]
    whole = qs.boxes("twice")[qs.whole_box("twice")][None]
    seq = ov.sequences(s, whole, keep=len(off))
    assert seq.count[0] == len(off)
    assert (np.diff(seq.prim[0]) >= 0).all() and (np.diff(seq.prim[0]) == 0).sum() == len(off) - len(np.unique(off)) > 0
    # and within the first eight of some box of the batch, and of some point: the kernels' lists meet equal offsets
    bs, ps = qs.box_sequences("twice"), qs.point_sequences("twice")
    assert ((bs.prim[:, 1:8] == bs.prim[:, :7]) & (bs.prim[:, :7] >= 0)).any()
    first8 = np.sort(ps.prim[:, :8], axis=1)
    assert ((first8[:, 1:] == first8[:, :-1]) & (first8[:, :-1] >= 0)).any()


def own_tree(name, slack):
    s = qs.scene(name)
    h, own, _ = C.own_hierarchy(s.node_view, s.n_prims, slack)
    if h < 0:
        return False
    try:
        C.own_wide(own, s.n_prims)
    except C.LensTraceError:
        return False
    return True


def test_the_table_of_own_trees_is_the_host_builders():
    assert sorted(qs.OWN_TREE) == sorted(qs.NAMES)
    assert {name: own_tree(name, 2) for name in qs.NAMES} == qs.OWN_TREE
    assert {name: own_tree(name, -1) for name in qs.OWN_TREE_CALLERS_SPLITS} == qs.OWN_TREE_CALLERS_SPLITS    # LT_RETREE=0: the caller's splits
    assert not qs.OWN_TREE["twice"]


def test_the_edit_changes_the_answers():
    """tests/test_gpu_query_shapes.py's edit of the primitives would pass on stale leaf records if the models of the two scenes
    agreed: at least a quarter of the points that hit in either have another record."""
    a, b = qs.expected("edit_base")["nearest_points"], qs.expected("edit_moved")["nearest_points"]
    hit = (a["prim"] >= 0) | (b["prim"] >= 0)
    differ = np.zeros(len(a), dtype=bool)
    differ[nr.same(a, b)] = True
    assert hit.sum() >= 256 and 4 * (differ & hit).sum() >= hit.sum()
    assert qs.scene("edit_base").nodes.tobytes() == qs.scene("edit_moved").nodes.tobytes()
    for kind in qs.KINDS:
        assert qs.differing({kind: qs.expected("edit_base")[kind]}, qs.expected("edit_moved")) != [], kind
