"""GPU (-m gpu): the point and box queries (lt_hip_nearest_points, lt_hip_nearest_k, lt_hip_overlap_boxes; lt_nearest.hip and
lt_overlap.hip) on every shape of tree the library makes and on buffers with a history.  Their own test files settle the
arithmetic on a few scenes in fresh contexts; here the same word-for-word comparison with the numpy models (tests/nearest.py,
tests/nearest_k.py, tests/overlap.py) runs where these walks differ from the ray walks: they read the per-lane records
(SceneDev::wide), whose leaf records an edit of the primitives remakes; they keep a best-first stack and a per-lane K list in
LDS; they treat the link built from nWide + n_prims as "never entered"; and they share the ray queries' work counters.
"Every kind": nearest_points, nearest_k with K = 1, 3, 8 and the count, overlap_boxes with K = 1, 3, 8, the count and any
(tests/query_shapes.py, whose models tests/test_query_shapes_cpu.py holds against the GPU-free forms).  No tolerance anywhere.

a. every scene of tests/query_shapes.py prepared by the host and by the device, some with the caller's splits (LT_RETREE=0), the
   largest with LT_TRACE_REFILL=1; lt_hip_get_stats says "own tree" or "none" as the host builder does;
b. a history of scenes in one context: small scenes in the buffers of a large one, the scanned scene between two trees;
c. an edit of the primitives: the leaf records are remade, the leaf boxes are the nodes' and stay;
d. LT_DEBUG_POISON: host and device forms, and small calls in staging buffers that hold a large call's records;
e. two device calls on two streams with nothing between them: the library orders them (begin_ray_launches);
f. 2^20 records, so that every lane takes several: the batches above are so small that a launch has a lane for every record."""
import ctypes
import functools

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from tests import nearest as nr
from tests import nearest_k as nk
from tests import query_shapes as qs
from tests import test_gpu_scene_history as hist
from tests.test_gpu_scene_history import context, environment, plain_and_poisoned

pytestmark = pytest.mark.gpu
SENTINEL = 0x5a5a5a5a


def host_kinds(r, name, note, pidx=None, bidx=None):
    """Every kind through the host forms on the batches of `name` (indexed), held against the model; returns the words."""
    pts = qs.points(name) if pidx is None else np.ascontiguousarray(qs.points(name)[pidx])
    bxs = qs.boxes(name) if bidx is None else np.ascontiguousarray(qs.boxes(name)[bidx])
    got = qs.every_kind(r.nearest_points, r.nearest_k, r.overlap_boxes, pts, bxs)
    assert qs.differing(got, qs.expected(name, pidx, bidx)) == [], note
    return qs.as_words(got)


def device_kinds(r, name, note, stream=None):
    """Every kind through the device forms, from torch tensors on `stream` (None: the current one); returns the words."""
    import torch
    pt, bt = torch.from_numpy(np.array(qs.points(name))).cuda(), torch.from_numpy(np.array(qs.boxes(name))).cuda()
    torch.cuda.synchronize()
    got = qs.every_kind(lambda p: r.nearest_points(p, stream=stream), lambda p, **kw: r.nearest_k(p, stream=stream, **kw),
                        lambda b, **kw: r.overlap_boxes(b, stream=stream, **kw), pt, bt)
    torch.cuda.synchronize()
    assert qs.differing(got, qs.expected(name)) == [], note
    return qs.as_words(got)


def same_words(a, b, note):
    assert sorted(a) == sorted(b), note
    for kind in a:
        assert np.array_equal(a[kind], b[kind]), (note, kind)


def own_tree_as_the_table_says(r, name, table=qs.OWN_TREE):
    height = r.stats()["own_tree_height"]
    assert (height > 0) if table[name] else (height == -1), (name, height)


# ---------------------------------------------------------------------------------------------------------------- a: shapes
CASES = ([(name, device, {}) for name in qs.NAMES for device in (False, True)] +
         [(name, device, {"LT_RETREE": "0"}) for name in qs.OWN_TREE_CALLERS_SPLITS for device in (False, True)] +
         [("random2049", device, {"LT_TRACE_REFILL": "1"}) for device in (False, True)])


@pytest.mark.parametrize("name,device,env", CASES, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_every_kind_on_every_shape_of_tree(name, device, env):
    with environment(LT_DEVICE_BUILD="1" if device else "0", **env):
        r = context()
        try:
            r.set_scene(qs.scene(name))
            own_tree_as_the_table_says(r, name, qs.OWN_TREE_CALLERS_SPLITS if "LT_RETREE" in env else qs.OWN_TREE)
            if name in ("random64", "random65", "random2049"):
                assert r.scene_structure(3)[3] == int(device)       # (the device prepared it when asked to)
            host_kinds(r, name, (name, device, env))
            own_tree_as_the_table_says(r, name, qs.OWN_TREE_CALLERS_SPLITS if "LT_RETREE" in env else qs.OWN_TREE)
        finally:
            r.close()


# ---------------------------------------------------------------------------------------------------------------- b: history
HISTORY = ("random2049", "random3", "random2049", "twice", "random65", "multi")
_fresh = {}


def fresh_words(name, device):
    """Every kind on scene `name` in a context of its own; kept."""
    if (name, device) not in _fresh:
        with environment(LT_DEVICE_BUILD="1" if device else "0"):
            r = context()
            try:
                r.set_scene(qs.scene(name))
                _fresh[name, device] = host_kinds(r, name, (name, device, "a fresh context"))
            finally:
                r.close()
    return _fresh[name, device]


@pytest.mark.parametrize("device", [True, False])
def test_a_history_of_scenes_in_one_context(device):
    """The pool hands each scene the buffers of the one before: the small scenes run in buffers that held the large one, and
    the scanned scene follows a tree and is followed by one."""
    with environment(LT_DEVICE_BUILD="1" if device else "0"):
        r = context()
        try:
            for step, name in enumerate(HISTORY):
                r.set_scene(qs.scene(name))
                own_tree_as_the_table_says(r, name)
                got = host_kinds(r, name, (HISTORY, step, device))
                same_words(got, fresh_words(name, device), (HISTORY, step, device, "a fresh context"))
            assert r.stats()["scene_uploads"] == len(HISTORY)
        finally:
            r.close()


# ---------------------------------------------------------------------------------------------------------------- c: an edit
@pytest.mark.parametrize("device", [True, False])
def test_an_edit_of_the_primitives_changes_the_answers_and_only_through_the_triangles(device):
    """tests/test_gpu_scene_history.py's edit (scene ("random", 4, 2049), positions moved by N(0, 0.01), the same nodes).  The
    leaf boxes are the nodes' and did not move, so d2 = max(triangle, box) and boxes_meet still use the old boxes: the models do
    that by construction, they read the boxes from the scene's nodes and the triangles from its primitives.  That the two models
    differ on more than a quarter of the points that hit -- the test would otherwise pass on stale leaf records -- is
    tests/test_query_shapes_cpu.py's test_the_edit_changes_the_answers; asserted here once more."""
    base, edited = qs.scene("edit_base"), qs.scene("edit_moved")
    assert base.nodes.tobytes() == edited.nodes.tobytes() and base.prims.tobytes() != edited.prims.tobytes()
    a, b = qs.expected("edit_base")["nearest_points"], qs.expected("edit_moved")["nearest_points"]
    hit = (a["prim"] >= 0) | (b["prim"] >= 0)
    differ = np.zeros(len(a), dtype=bool)
    differ[nr.same(a, b)] = True
    assert hit.sum() >= 256 and 4 * (differ & hit).sum() >= hit.sum()
    with environment(LT_DEVICE_BUILD="1" if device else "0"):
        r = context()
        try:
            r.set_scene(hist.scene(("random", 3, 2049)))   # (the scene before: its buffers are the ones the next one takes)
            r.set_scene(base)
            first = host_kinds(r, "edit_base", (device, "before the edit"))
            uploads = r.stats()["scene_uploads"]
            r.set_scene(edited)
            assert r.stats()["scene_uploads"] == uploads + 1
            after = host_kinds(r, "edit_moved", (device, "after the edit"))
            for kind in qs.KINDS:
                assert not np.array_equal(first[kind], after[kind]), kind
            r.set_scene(base)
            same_words(host_kinds(r, "edit_base", (device, "the base scene again")), first, (device, "the base scene again"))
        finally:
            r.close()


# ---------------------------------------------------------------------------------------------------------------- d: poison
POISON_SCENES = ("random2049", "mixed")
LARGE, SMALL = 4097, 65


def large_indices(name):
    """4097 of the scene's points and of its boxes, by repetition with a shuffle; the models are indexed the same way."""
    return qs.repeated(len(qs.points(name)), LARGE, 11), qs.repeated(len(qs.boxes(name)), LARGE, 12)


@pytest.mark.parametrize("poison", hist.WALK_POISONS, ids=hex)
@pytest.mark.parametrize("name", POISON_SCENES)
def test_every_kind_on_poisoned_scratch(name, poison):
    import torch
    side = torch.cuda.Stream()

    def call(r):
        return {"host": host_kinds(r, name, (name, "host forms")), "device": device_kinds(r, name, (name, "device forms")),
                "side stream": device_kinds(r, name, (name, "device forms, a side stream"), stream=side)}

    got, plain = plain_and_poisoned(name, poison, "query shapes: every kind", call, resident=qs.scene(name))
    for form in got:
        same_words(got[form], plain[form], (name, hex(poison), form, "a context without the switch"))
        same_words(got[form], got["host"], (name, hex(poison), form, "the host forms"))


@pytest.mark.parametrize("poison", hist.WALK_POISONS, ids=hex)
@pytest.mark.parametrize("name", POISON_SCENES)
def test_small_calls_after_large_ones_in_the_same_context(name, poison):
    """The staging buffers of the host forms are kept and shared: nearest_k (K = 8) on 4097 points leaves 128-byte records in the
    output buffer and overlap_boxes (K = 8) on 4097 boxes 32-byte records in both; the count (16 B in, 4 B out), any (32 B in,
    4 B out) and nearest_points on the first 65 then run in buffers that hold those records and, beyond them, poison."""
    pidx, bidx = large_indices(name)
    pts, bxs = np.ascontiguousarray(qs.points(name)[pidx]), np.ascontiguousarray(qs.boxes(name)[bidx])
    want = qs.expected(name, pidx, bidx)
    small_kinds = ("nearest_count", "overlap_any", "nearest_points")

    def small(r):
        return qs.as_words(qs.every_kind(r.nearest_points, r.nearest_k, r.overlap_boxes, pts[:SMALL], bxs[:SMALL], kinds=small_kinds))

    def large_then_small(r):
        large = qs.every_kind(r.nearest_points, r.nearest_k, r.overlap_boxes, pts, bxs, kinds=("nearest_k8", "overlap_k8"))
        assert qs.differing(large, want) == [], (name, "the large calls")
        return small(r)

    resident = qs.scene(name)
    got, after_large = plain_and_poisoned(name, poison, "query shapes: large, then small", large_then_small, resident=resident)
    alone_poisoned, alone = plain_and_poisoned(name, poison, "query shapes: small alone", small, resident=resident)
    first = {"nearest_count": want["nearest_count"][:SMALL], "overlap_any": want["overlap_any"][:SMALL], "nearest_points": want["nearest_points"][:SMALL]}
    assert qs.differing(alone, first) == [], (name, "a fresh context, the model")
    assert (want["nearest_count"][:SMALL] > 0).sum() >= 16 and (want["overlap_any"][:SMALL] == 0).sum() >= 8 and (want["overlap_any"][:SMALL] == 1).sum() >= 8
    same_words(after_large, alone, (name, "after the large calls, without the switch"))
    same_words(got, alone, (name, hex(poison), "after the large calls"))
    same_words(alone_poisoned, alone, (name, hex(poison), "small alone"))


# ---------------------------------------------------------------------------------------------------------------- f: a lane's next record
FULL = 2 ** 20


@pytest.mark.parametrize("name", ("random2049", "twice"))
def test_every_lane_takes_several_records(name):
    """A launch has one wave per 64 records until every wave slot of the chip is taken (lt_nearest::launch_k, lt_overlap::launch:
    at most 32 waves per CU), so in a batch of a few thousand records no lane ever takes a second one -- only a wave that starts
    late leaves its batch to another.  What a lane does when it takes its next record -- the K list in LDS reset, the stack
    pointer and the best record set back -- shows only above 64 records per wave slot: 2^20 records here, drawn from the scene's
    batches by repetition with a shuffle, through the device forms, compared on the device with the models' rows.  On the scene
    with a tree and on the scanned one."""
    import torch
    slots = torch.cuda.get_device_properties(0).multi_processor_count * 32 * 64
    assert FULL >= 2 * slots, (FULL, slots)
    pidx, bidx = qs.repeated(len(qs.points(name)), FULL, 21), qs.repeated(len(qs.boxes(name)), FULL, 22)
    want = qs.expected(name)
    r = context()
    try:
        r.set_scene(qs.scene(name))
        own_tree_as_the_table_says(r, name)
        pi, bi = torch.from_numpy(pidx).cuda(), torch.from_numpy(bidx).cuda()
        pt = torch.from_numpy(np.array(qs.points(name))).cuda()[pi].contiguous()
        bt = torch.from_numpy(np.array(qs.boxes(name))).cuda()[bi].contiguous()
        for kind in qs.KINDS:
            got = qs.every_kind(r.nearest_points, r.nearest_k, r.overlap_boxes, pt, bt, kinds=(kind,))[kind]
            rows = torch.from_numpy(qs.words(want[kind]).view(np.int32).reshape(len(want[kind]), -1).copy()).cuda()
            index = pi if kind in qs.POINT_KINDS else bi
            differ = (got.view(torch.int32).reshape(FULL, -1) != rows[index]).any(dim=1)
            assert int(differ.sum()) == 0, (name, kind, "%d of %d records differ, first at %d" % (int(differ.sum()), FULL, int(differ.nonzero()[0])))
    finally:
        torch.cuda.synchronize()
        r.close()


# ---------------------------------------------------------------------------------------------------------------- e: two streams
STREAM_SCENE = "random2049"


@functools.lru_cache(maxsize=None)
def unbounded_counts():
    """The scene's points with max_d2 = inf and the model's count of each: every leaf, for a point whose d2 stay finite."""
    s = qs.scene(STREAM_SCENE)
    pts = np.array(qs.points(STREAM_SCENE))
    pts[:, 3] = np.inf
    count = nk.sequences(s, pts).count
    with np.errstate(invalid="ignore"):
        near = np.isfinite(pts[:, 0:3]).all(axis=1) & (np.abs(pts[:, 0:3]) < 2.0 ** 40).all(axis=1)
    assert near.sum() >= 400 and (count[near] == len(nr.leaves(s)[0])).all() and (count[~near] == 0).all()
    return qs.frozen(pts), qs.frozen(count)


class Raw:
    """The raw _device calls of one context over sentinel-filled outputs with 64 words to spare."""
    def __init__(self, r):
        self.r, self.calls = r, []

    def inputs(self, records):
        import torch
        return torch.from_numpy(np.array(records)).cuda()

    def output(self, words):
        import torch
        return torch.full((words + 64,), SENTINEL, dtype=torch.int32, device="cuda")

    def enqueue(self, what, name, desc, inp, out, record_words, want, stream):
        n = inp.shape[0]
        rc = getattr(self.r._L, "lt_hip_%s_device" % name)(self.r._ctx, ctypes.byref(desc), ctypes.c_void_p(inp.data_ptr()), n,
                                                           ctypes.c_void_p(out.data_ptr()), 4 * record_words * n, ctypes.c_void_p(stream.cuda_stream))
        self.r._check(rc)
        self.calls.append((what, out, record_words * n, want))

    def check(self):
        for what, out, words, want in self.calls:
            got = out.cpu().numpy().view(np.uint32)
            assert (got[words:] == SENTINEL).all(), (what, "words behind the results")
            kept = int((got[:words] == SENTINEL).sum())
            differ = int((got[:words] != qs.words(want)).sum())
            assert kept == 0 and differ == 0, (what, "%d of %d words keep the sentinel, %d differ from the model" % (kept, words, differ))


def nearest_k_desc(k):
    return C.NearestKDesc(ctypes.sizeof(C.NearestKDesc), 0, C.NEAREST_FIRST_K if k else C.NEAREST_COUNT, k)


def overlap_desc(kind, k=0):
    return C.OverlapDesc(ctypes.sizeof(C.OverlapDesc), 0, kind, k)


@pytest.mark.parametrize("MANY", [2 ** 16, 2 ** 20], ids=["2^16", "2^20"])
@pytest.mark.parametrize("long_call", ["nearest_k", "overlap_boxes"])
def test_calls_on_two_streams_are_ordered_among_themselves(long_call, MANY):
    """The families share eight work counters (d_query_ctl), which a call zeroes and its waves then draw from: a call that
    started while the previous one was running would zero the counters under it and draw from the same ones, and records of
    either would stay unwritten.  begin_ray_launches makes the later call's stream wait for the earlier call's event.  A long
    call on stream A (records that visit every leaf), a K = 8 call on stream B at once, then a third on A; nothing synchronises
    between the enqueues.  With 2^16 records every wave of A draws once, when it starts: that call may be past its last draw
    before B's first command arrives, and with the wait taken out of the library this case passed in one run of two.  With 2^20
    records A fills every wave slot of the chip and its waves draw 64 records at a time for milliseconds: without the wait B
    zeroes the counters under them, and B's waves, which find room only when A's leave, meet counters that A has run past
    B's n and write nothing -- tried: thousands of B's words kept the sentinel."""
    import torch
    name = STREAM_SCENE
    s = qs.scene(name)
    leaves = len(nr.leaves(s)[0])
    pidx, bidx = large_indices(name)
    want = qs.expected(name, pidx, bidx)
    r = context()
    try:
        r.set_scene(s)
        raw = Raw(r)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        if long_call == "nearest_k":
            pts, count = unbounded_counts()
            many = qs.repeated(len(pts), MANY, 13)
            assert (count[many] == leaves).sum() >= MANY // 2
            ins = [raw.inputs(pts[many]), raw.inputs(qs.boxes(name)[bidx]), raw.inputs(qs.points(name)[pidx])]
            outs = [raw.output(MANY), raw.output(8 * LARGE), raw.output(4 * LARGE)]
            torch.cuda.synchronize()
            raw.enqueue("A: nearest_k, count, max_d2 = inf", "nearest_k", nearest_k_desc(0), ins[0], outs[0], 1, count[many], a)
            raw.enqueue("B: overlap_boxes, K = 8", "overlap_boxes", overlap_desc(C.OVERLAP_FIRST_K, 8), ins[1], outs[1], 8, want["overlap_k8"], b)
            raw.enqueue("A: nearest_points", "nearest_points", C.NearestDesc(ctypes.sizeof(C.NearestDesc), 0), ins[2], outs[2], 4, want["nearest_points"], a)
        else:
            # half of the boxes hold the whole scene: every leaf touches them
            whole = qs.whole_box(name)
            many = np.concatenate([qs.repeated(len(qs.boxes(name)), MANY // 2, 14), np.full(MANY // 2, whole)])
            many = many[np.random.default_rng(15).permutation(MANY)]
            count = qs.expected(name)["overlap_count"][many]
            assert (count == leaves).sum() >= MANY // 2
            ins = [raw.inputs(qs.boxes(name)[many]), raw.inputs(qs.points(name)[pidx]), raw.inputs(qs.boxes(name)[bidx])]
            outs = [raw.output(MANY), raw.output(32 * LARGE), raw.output(LARGE)]
            torch.cuda.synchronize()
            raw.enqueue("A: overlap_boxes, count", "overlap_boxes", overlap_desc(C.OVERLAP_COUNT), ins[0], outs[0], 1, count, a)
            raw.enqueue("B: nearest_k, K = 8", "nearest_k", nearest_k_desc(8), ins[1], outs[1], 32, want["nearest_k8"], b)
            raw.enqueue("A: overlap_boxes, any", "overlap_boxes", overlap_desc(C.OVERLAP_ANY), ins[2], outs[2], 1, want["overlap_any"], a)
        a.synchronize()
        b.synchronize()
        raw.check()
    finally:
        torch.cuda.synchronize()
        r.close()
