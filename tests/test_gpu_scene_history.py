"""GPU (-m gpu): scene preparation and the walks do not depend on what their buffers held before.

The pool of lt_hip_set_scene hands the next scene the previous scene's buffers of the same sizes, unchanged, and the scratch of
the render and query calls is kept between calls: every kernel that reads a word has to have been preceded by one that wrote it.
Fresh memory in a young process is zero pages, which hides a missing write.  Here the structures a scene leaves in device memory
are read back (lt_hip_read_scene_structure, kinds 0..5) and compared byte for byte -- no tolerance anywhere in this file --

a. with the numpy reference of the records (tests/structures.py), in a fresh context: the traversal triangles, the packet walks'
   records and the per-lane walks' records, neither of which any other test reads;
b. across LT_DEBUG_POISON 0x00 / 0xFF / 0x7F (every buffer filled before use with zero words, with all-ones words -- kNone, NaN, the
   largest count --, with a large finite float that is also a large positive integer) and without the switch;
c. after real leftovers: sequences of scenes in one context against the same scene in a fresh one, and an edit of the primitives;
d. and the walks themselves run on poisoned scratch: renders and ray queries against the CPU oracle and a context without the
   switch.

The only bytes left out of any comparison are the kind-2 leaf records of primitive offsets no leaf names (structures.unlinked):
nobody writes them and no walk reads them.  That set is asserted empty except for the scene with leaves of three primitives.
The sizes: 64 / 65 leaves (one wavefront finishes the subtree / one wavefront per range), 2048 / 2049 (one / many workgroups),
5000 (several many-workgroup levels)."""
import contextlib
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import KERNEL_MODE_LINEAR, RendererHIP, RenderPropertiesHIP, make_rays, make_shade_rays, reference_camera_rays
from oracle import pyoracle as po
from tests import multihit as M
from tests import shade_rays as F
from tests import structures as st
from tests import surface as S
from tests.test_gpu_device_prep import random_triangles
from tests.test_gpu_shade_paths import STAGE_FORMS
from tests.test_structures_cpu import multi_primitive_leaf_scene

pytestmark = pytest.mark.gpu

SIZES = (64, 65, 2048, 2049, 5000)
POISONS = (0x00, 0xFF, 0x7F)
KINDS = (0, 1, 2, 3, 4, 5)


@contextlib.contextmanager
def environment(**env):
    """Sets the variables for the block (None: unset) and puts back what was there."""
    before = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def context(poison=None, **env):
    """A new context; LT_DEBUG_POISON and what else is read when a context is created are set for that moment only."""
    with environment(LT_DEBUG_POISON=None if poison is None else "0x%02X" % poison, **env):
        return RendererHIP(0)


def read_all(r):
    return [r.scene_structure(k) for k in KINDS]


_scenes = {}


def scene(name):
    """("random", seed, n) | "cornell" | "multi" | "mixed": built once per process, never modified."""
    if name not in _scenes:
        if name == "cornell":
            s = F.scene()
        elif name == "multi":
            s = multi_primitive_leaf_scene()
        elif name == "mixed":
            s = synth.wall_and_soup(60, 9000).validate()
        else:
            s = random_triangles(name[1], name[2])
        _scenes[name] = s
    return _scenes[name]


def rows(a, width):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, width)


def keep_rows(got):
    """The rows of kind 2 a comparison covers (structures.wide_mask), from kinds 0 and 3 of the same read-back; None: all."""
    if got[0] is None:
        return None
    keep = st.wide_mask(got[0], got[3][2], len(got[5]) // 48)
    return None if keep.all() else keep


def same_kinds(got, want, what, info_words=4):
    """Kinds 0, 1, 4, 5 byte for byte, kind 2 outside `unlinked`, the first info_words words of kind 3."""
    assert got[3][:info_words] == want[3][:info_words], (what, got[3], want[3])
    for k, width in ((0, 32), (1, 32), (4, 64), (5, 48), (2, 64)):
        assert (got[k] is None) == (want[k] is None), (what, k)
        if got[k] is None:
            continue
        a, b = rows(got[k], width), rows(want[k], width)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        differ = (a != b).any(axis=1)
        if k == 2:
            keep, keep_want = keep_rows(got), keep_rows(want)
            assert (keep is None) == (keep_want is None) and (keep is None or np.array_equal(keep, keep_want)), what
            if keep is not None:
                differ &= keep
        bad = np.flatnonzero(differ)
        assert len(bad) == 0, "%s: kind %d: %d of %d records differ, first at %d: %s / %s" % (
            what, k, len(bad), len(a), bad[0], a[bad[0]].view(np.uint32), b[bad[0]].view(np.uint32))


_fresh = {}


def fresh(name, device, poison=None, **env):
    """Kinds 0..5 of scene(name) prepared in a context of its own; kept per (scene, who prepares, poison, knobs)."""
    key = (name, device, poison, tuple(sorted(env.items())))
    if key not in _fresh:
        with environment(LT_DEVICE_BUILD="1" if device else "0", **env):
            r = context(poison)
            try:
                r.set_scene(scene(name))
                _fresh[key] = read_all(r)
            finally:
                r.close()
    return _fresh[key]


# ---------------------------------------------------------------------------------------- a: the records against the reference
_reference = {}


def reference(own, s):
    """(kind 2 rows with their mask, kind 4 rows) of tests/structures.py for this own tree, kept by the tree's bytes."""
    key = (own.tobytes(), s.prims.tobytes())
    if key not in _reference:
        children, groupOf = st.collapse(own)
        wide, ok = st.wide_records(own, children, groupOf, s.prim_view, s.n_prims)
        assert ok
        # the groups are lt_hip_own_wide's (what tests/test_structures_cpu.py holds the reference against), slot for slot
        _, origin, step, slots = C.own_wide(own, s.n_prims)
        assert wide[1: 1 + len(children)].tobytes() == slots.tobytes()
        assert wide[0, 8:11].tobytes() == origin.tobytes() and wide[0, 12:15].tobytes() == step.tobytes()
        _reference[key] = (wide, st.wide_mask(own, len(children), s.n_prims), st.pair_records(own, s.prim_view))
    return _reference[key]


def check_against_reference(got, s, what, unlinked=0):
    own = got[0]
    assert own is not None and got[2] is not None and got[4] is not None, what
    assert got[5].tobytes() == st.retile(s.prim_view).tobytes(), (what, "traversal triangles")
    wide, keep, pairs = reference(own, s)
    assert int((~keep).sum()) == unlinked == len(st.unlinked(own, s.n_prims)), what
    a, b = rows(got[4], 64), rows(pairs, 64)
    bad = np.flatnonzero((a != b).any(axis=1)) if a.shape == b.shape else [-1]
    assert len(bad) == 0, "%s: packet-walk records: %d of %d differ, first at %s: %s / %s" % (
        what, len(bad), len(b), bad[0], a[bad[0]].view(np.uint32), b[bad[0]].view(np.uint32))
    a, b = rows(got[2], 64), rows(wide, 64)
    bad = np.flatnonzero((a != b).any(axis=1) & keep) if a.shape == b.shape else [-1]
    assert len(bad) == 0, "%s: per-lane walk records: %d of %d differ, first at %s: %s / %s" % (
        what, len(bad), len(b), bad[0], a[bad[0]].view(np.uint32), b[bad[0]].view(np.uint32))


REFERENCE_SCENES = [("random", n, n) for n in SIZES] + ["cornell", "multi"]


@pytest.mark.parametrize("retree", ["1", "0"])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", REFERENCE_SCENES, ids=str)
def test_records_of_a_fresh_context_equal_the_numpy_reference(name, device, retree):
    s = scene(name)
    got = fresh(name, device, LT_RETREE=retree)
    check_against_reference(got, s, (name, device, retree), unlinked=4 if name == "multi" else 0)
    assert len(got[4]) == 64 * len(got[0]) and len(got[5]) == 48 * s.n_prims and got[3][0] > 0


def test_a_scene_without_own_structures_has_no_packet_records_but_its_triangles():
    base = scene(("random", 9, 400))
    nodes = base.node_view.copy()
    nodes["boundsMax"][np.flatnonzero(nodes["primitiveCount"] != 0)[5]] += 100.0   # a box outside its parent's
    s = sc.Scene(nodes=nodes.view(np.uint8).reshape(-1), prims=base.prims, materials=base.materials, lights=base.lights, camera=base.camera)
    r = context()
    try:
        r.set_scene(s)
        got = read_all(r)
        assert got[0] is None and got[1] is None and got[2] is None and got[4] is None
        assert got[5].tobytes() == st.retile(s.prim_view).tobytes()
        with pytest.raises(C.LensTraceError):
            r.scene_structure(6)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------- b: poison
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", [("random", n, n) for n in SIZES] + ["mixed"], ids=str)
def test_preparation_does_not_depend_on_the_bytes_its_buffers_held(name, device):
    plain = fresh(name, device)
    assert plain[0] is not None and plain[3][3] == int(device)
    assert keep_rows(plain) is None   # (every primitive of a built scene is named by a leaf: nothing is left out below)
    for poison in POISONS:
        r = context(poison)
        try:
            with environment(LT_DEVICE_BUILD="1" if device else "0"):
                r.set_scene(scene(name))
            same_kinds(read_all(r), plain, (name, device, hex(poison)), info_words=3)
        finally:
            r.close()


def test_the_poison_switch_fills_what_nobody_writes():
    """The switch works at all: the kind-2 leaf records no leaf names (the one region of a resident structure that no kernel writes)
    come back holding the byte."""
    s = scene("multi")
    for poison in POISONS:
        r = context(poison)
        try:
            r.set_scene(s)
            got = read_all(r)
            keep = keep_rows(got)
            assert keep is not None and int((~keep).sum()) == 4
            assert (rows(got[2], 64)[~keep] == poison).all(), hex(poison)
            check_against_reference(got, s, ("multi", hex(poison)), unlinked=4)
        finally:
            r.close()


# ---------------------------------------------------------------------------------------- c: real leftovers
def run_sequence(names, device, context_env=None, **env):
    """One context, a set_scene per name: after each, all kinds equal those of the same scene in a fresh context."""
    r = context(**(context_env or {}))
    try:
        with environment(LT_DEVICE_BUILD="1" if device else "0", **env):
            for step, name in enumerate(names):
                r.set_scene(scene(name))
                same_kinds(read_all(r), fresh(name, device, **env), (names, step, device, env))
        assert r.stats()["scene_uploads"] == len(names)
    finally:
        r.close()


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("n", [65, 2049, 5000])
def test_three_scenes_of_one_size_each_on_the_leftovers_of_the_one_before(n, device):
    run_sequence([("random", seed, n) for seed in (1, 2, 3)], device)


@pytest.mark.parametrize("device", [True, False])
def test_a_scene_comes_back_after_another(device):
    a, b = ("random", 1, 2049), ("random", 2, 2049)
    run_sequence([a, b, a], device)


@pytest.mark.parametrize("device", [True, False])
def test_large_then_small_then_large(device):
    run_sequence([("random", 1, 5000), ("random", 1, 65), ("random", 2, 5000)], device)


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("env", [{"LT_RETREE": "0"}, {"LT_RETREE_SLACK": "0"}], ids=str)
def test_two_scenes_under_the_other_split_rules(env, device):
    run_sequence([("random", 1, 2049), ("random", 2, 2049)], device, **env)
    run_sequence([("random", 1, 5000), ("random", 2, 5000)], device, **env)


@pytest.mark.parametrize("device", [True, False])
def test_two_scenes_without_a_pool(device):
    run_sequence([("random", 1, 2049), ("random", 2, 2049)], device, context_env={"LT_SCENE_POOL_BYTES": "0"})


@pytest.mark.parametrize("n", [2049, 5000])
def test_a_good_scene_after_one_the_device_declined_half_way(n):
    """The declined scene's scratch block and leaf order table went back into the pool partly written (its checks had run, its
    build had not); the host prepared it.  The next scene has the same sizes and takes those buffers."""
    first, second = ("random", 1, n), ("random", 2, n)
    base = scene(first)
    nodes = base.node_view.copy()
    nodes["boundsMax"][np.flatnonzero(nodes["primitiveCount"] != 0)[5]] += 100.0
    declined = sc.Scene(nodes=nodes.view(np.uint8).reshape(-1), prims=base.prims, materials=base.materials, lights=base.lights, camera=base.camera)
    r = context()
    try:
        with environment(LT_DEVICE_BUILD="1"):
            for step in range(2):
                r.set_scene(declined)
                got = read_all(r)
                assert got[3][3] == 0 and got[0] is None and got[4] is None
                assert got[5].tobytes() == st.retile(base.prim_view).tobytes()
                name = (second, first)[step]
                r.set_scene(scene(name))
                same_kinds(read_all(r), fresh(name, True), (name, "after a declined scene"))
    finally:
        r.close()


@pytest.mark.parametrize("device", [True, False])
def test_an_edit_of_the_primitives_remakes_the_leaf_records_alone(device):
    name = ("random", 4, 2049)
    base = scene(name)
    prims = base.prim_view.copy()
    rng = np.random.default_rng(5)
    for k in ("positionA", "positionB", "positionC"):
        prims[k] += rng.normal(0, 0.01, prims[k].shape).astype(np.float32)
    edited = sc.Scene(nodes=base.nodes, prims=prims.view(np.uint8).reshape(-1), materials=base.materials, lights=base.lights, camera=base.camera)
    r = context()
    try:
        with environment(LT_DEVICE_BUILD="1" if device else "0"):
            r.set_scene(scene(("random", 3, 2049)))   # (the scene before: its buffers are the ones the next one takes)
            r.set_scene(base)
            before = read_all(r)
            uploads = r.stats()["scene_uploads"]
            r.set_scene(edited)
            got = read_all(r)
        assert r.stats()["scene_uploads"] == uploads + 1 and got[3] == before[3]
        assert got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes()   # the trees are the nodes' alone
        assert got[5].tobytes() != before[5].tobytes()
        check_against_reference(got, edited, (name, device, "edited"))
    finally:
        r.close()


# ---------------------------------------------------------------------------------------- d: the walks on poisoned memory
W, H = 96, 64
WALK_SCENES = {"random5000": (("random", 5000, 5000), (0.0, 0.0, 0.0), 0.3, 45.0), "cornell": ("cornell", F.CENTRE, 0.3, 50.0)}
WALK_POISONS = (0xFF, 0x7F)
ACC = "accumulator.cl"
GI = "examples/global_illumination/resources/kernels/global_illumination.cl"
GI_FORMS = dict({k: dict(v, LT_GI_MEGAKERNEL="0") for k, v in STAGE_FORMS.items() if "LT_RETREE" not in v}, megakernel={"LT_GI_MEGAKERNEL": "1"})
assert sorted(GI_FORMS) == ["five_launches", "lds_scene", "megakernel", "one_kernel"]


def walk_camera(which, frame=0):
    _, centre, yaw, dist = WALK_SCENES[which]
    return sc.camera_bytes(float(np.float32(centre[0] - dist * np.sin(yaw))), centre[1], float(np.float32(centre[2] - dist * np.cos(yaw))),
                           float(np.float32(yaw)), 0.0, 0.0, frame)


def walk_scene(which):
    return scene(WALK_SCENES[which][0])


_oracle = {}


def oracle_fold(which, program, w, h, frame_first, frame_count):
    """(h, w, 3): the oracle's frames folded by the running mean from n = 0; kept."""
    key = (which, program, w, h, frame_first, frame_count)
    if key not in _oracle:
        acc = np.zeros((h, w, 3), dtype=np.float32)
        for i in range(frame_count):
            po.accumulate(acc, np.ascontiguousarray(po.render(walk_scene(which), walk_camera(which, frame_first + i), w, h, program, threads=8)), i)
        _oracle[key] = F.frozen(acc)
    return _oracle[key]


def render(r, which, path, w, h, frame_first, frame_count, portable=True):
    out = np.zeros((h, w, 3), dtype=np.float32)
    r.render(RenderPropertiesHIP(path, (w, h, 3), out, walk_scene(which), pCamera=walk_camera(which), frameFirst=frame_first, frameCount=frame_count,
                                 accumulate=frame_count > 1, portableMath=portable))
    return out


def same_image(got, want, what):
    differ = int((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum())
    assert differ == 0, (what, "%d floats differ" % differ)


def batch(which):
    """4097 of the camera's rays, shuffled: (lt_hip_shade_ray records, lt_hip_ray records, pixel of each)"""
    o, d, fx, fy = reference_camera_rays(walk_camera(which), W, H)
    pix = np.random.default_rng(17).permutation(W * H)[:4097]
    return make_shade_rays(o[pix], d[pix], fx[pix], fy[pix]), make_rays(o[pix], d[pix]), pix


_plain = {}


def plain_and_poisoned(which, poison, what, call, resident=None):
    """call(context) in a context with the switch and in one without it (that result kept per `what`): (poisoned, plain).  The
    scene is walk_scene(which), or `resident` (tests/test_gpu_query_shapes.py's scenes, which it names `which`)."""
    s = walk_scene(which) if resident is None else resident
    if (which, what) not in _plain:
        r = context()
        try:
            r.set_scene(s)
            _plain[which, what] = call(r)
        finally:
            r.close()
    r = context(poison)
    try:
        r.set_scene(s)
        return call(r), _plain[which, what]
    finally:
        r.close()


@pytest.mark.parametrize("poison", WALK_POISONS, ids=hex)
@pytest.mark.parametrize("which", list(WALK_SCENES))
def test_accumulator_with_every_shadow_walk_on_poisoned_scratch(which, poison):
    def call(r):
        out = {}
        for walk in "0123":
            with environment(LT_SHADOW_PACKETS=walk):
                out[walk] = render(r, which, ACC, W, H, 0, 3)
                out[walk, "default"] = render(r, which, ACC, W, H, 0, 3, portable=False)
        return out

    got, plain = plain_and_poisoned(which, poison, "accumulator", call)
    want = oracle_fold(which, po.ACCUMULATOR, W, H, 0, 3)
    for key in got:
        same_image(got[key], plain[key], (which, hex(poison), key, "a context without the switch"))
        if "default" not in key:
            same_image(plain[key], want, (which, key, "without the switch, the oracle"))
            same_image(got[key], want, (which, hex(poison), key, "the oracle"))


@pytest.mark.parametrize("poison", WALK_POISONS, ids=hex)
@pytest.mark.parametrize("which", list(WALK_SCENES))
def test_global_illumination_in_every_form_on_poisoned_scratch(which, poison):
    def call(r):
        out = {}
        for form, env in GI_FORMS.items():
            with environment(**env):
                out[form] = render(r, which, GI, W, H, 0, 1)
        return out

    got, plain = plain_and_poisoned(which, poison, "gi", call)
    want = oracle_fold(which, po.GI, W, H, 0, 1)
    for form in GI_FORMS:
        same_image(plain[form], want, (which, form, "without the switch, the oracle"))
        same_image(got[form], want, (which, hex(poison), form, "the oracle"))
        same_image(got[form], plain[form], (which, hex(poison), form, "a context without the switch"))


_expected = {}


def expected_queries(which):
    """What the oracle says of the batch: closest hits, the first four hits, their surface records, both programs' colours."""
    if which not in _expected:
        s = walk_scene(which)
        _, rays, pix = batch(which)
        seqs = M.sequences(("scene_history", which), s, rays, po.ACCUMULATOR)
        first = M.expected_records(seqs, rays, 1)[:, 0]
        _expected[which] = dict(closest=first, first4=M.expected_records(seqs, rays, 4), surface=S.expected(s, first, "portable"),
                                shade=oracle_fold(which, po.ACCUMULATOR, W, H, 0, 3).reshape(-1, 3)[pix],
                                paths=oracle_fold(which, po.GI, W, H, 0, 1).reshape(-1, 3)[pix])
    return _expected[which]


@pytest.mark.parametrize("poison", WALK_POISONS, ids=hex)
@pytest.mark.parametrize("which", list(WALK_SCENES))
def test_ray_queries_on_poisoned_scratch(which, poison):
    shade, rays, _ = batch(which)
    assert len(rays) == 4097

    def call(r):
        return dict(closest=r.trace_rays(rays, portable_math=True), first4=r.trace_hits(rays, max_hits=4, portable_math=True),
                    surface=r.trace_surface(rays, portable_math=True),
                    shade=r.shade_rays(shade, program=C.PROGRAM_ACCUMULATOR, frame_first=0, frame_count=3, portable_math=True),
                    paths=r.shade_paths(shade, program=C.PROGRAM_GLOBAL_ILLUMINATION, frame_first=0, frame_count=1, portable_math=True),
                    closest_default=r.trace_rays(rays), packets=r.trace_rays(rays, coherent=True, portable_math=True))

    got, plain = plain_and_poisoned(which, poison, "queries", call)
    for key in got:
        assert got[key].tobytes() == plain[key].tobytes(), (which, hex(poison), key, "a context without the switch")
    want = expected_queries(which)
    assert 4 * (want["closest"]["prim"] >= 0).sum() >= len(rays)   # (the batch sees the scene)
    for tag, res in (("without the switch", plain), (hex(poison), got)):
        assert len(M.same_records(res["closest"], want["closest"])) == 0, (which, tag, "trace_rays")
        assert len(M.same_records(res["packets"], want["closest"])) == 0, (which, tag, "trace_rays, the packet kernel")
        assert len(M.same_records(res["first4"], want["first4"])) == 0, (which, tag, "trace_hits")
        assert len(S.same(res["surface"], want["surface"])) == 0, (which, tag, "trace_surface")
        for key in ("shade", "paths"):
            same_image(res[key]["rgb"], want[key], (which, tag, key))
            assert np.array_equal(res[key]["prim"], want["closest"]["prim"]), (which, tag, key, "prim")


@pytest.mark.parametrize("poison", WALK_POISONS, ids=hex)
@pytest.mark.parametrize("which", list(WALK_SCENES))
def test_a_small_call_after_a_large_one_in_the_same_context(which, poison):
    """The scratch the calls grow is kept: the small call runs in buffers that hold the large call's data (and, beyond it, poison)."""
    def small(r):
        return {path: render(r, which, path, 40, 24, 0, 1) for path in (ACC, GI)}

    def call(r):
        for path in (ACC, GI):
            render(r, which, path, W, H, 0, 4)
        return small(r)

    got, after_large = plain_and_poisoned(which, poison, "large, then small", call)
    _, alone = plain_and_poisoned(which, poison, "small alone", small)
    for path, program in ((ACC, po.ACCUMULATOR), (GI, po.GI)):
        want = oracle_fold(which, program, 40, 24, 0, 1)
        same_image(alone[path], want, (which, path, "a fresh context, the oracle"))
        same_image(after_large[path], alone[path], (which, path, "after a large call, without the switch"))
        same_image(got[path], alone[path], (which, hex(poison), path, "after a large call"))
