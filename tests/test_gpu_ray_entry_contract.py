"""GPU (-m gpu): what the eighteen ray entry points (lt_hip_trace_rays, lt_hip_trace_hits, lt_hip_trace_surface, lt_hip_surface_at,
lt_hip_shade_rays, lt_hip_shade_paths, lt_hip_nearest_points, lt_hip_nearest_k, lt_hip_overlap_boxes, each with its _device form)
have in common -- the part of lens_trace_amd/csrc/lt_capi.hip behind its `ray queries` banner that is host code alone.  Cornell
box, a few hundred records at the most.

1. messages and precedence: every argument check of every entry point, in the order the library makes them, with its return code
   and the text of lt_hip_last_error; every two neighbouring checks violated in one call give the earlier one's; the output keeps
   its fill pattern throughout;
2. the host and the device form of a family give the same bytes at n = 1, 63, 64, 65 and 130, and lt_hip_get_stats the same
   figures;
3. the host forms share two staging buffers: a sequence of calls with records of 4, 16, 32, 48 and 128 bytes on one context
   gives what each call gives on a fresh context;
4. the device forms of all nine families back to back on one caller stream give the host forms' results."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import HIT_DTYPE, RendererHIP, make_shade_rays, nearest_points_host, overlap_boxes_host
from tests import nearest_k as nk
from tests import overlap as ov
from tests import shade_rays as F
from tests.test_gpu_trace_rays import random_rays

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
USER_PROGRAM = os.path.join(HERE, "user_kernels", "camera_rays.hip")
SCENE = "cornell_box_O0"
FILL = 0x5a5a5a5a
INVALID, NO_SCENE, TOO_SMALL, UNKNOWN = C.LT_ERR_INVALID_ARGUMENT, C.LT_ERR_NO_SCENE, C.LT_ERR_BUFFER_TOO_SMALL, C.LT_ERR_UNKNOWN_PROGRAM
BOTH = C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_PORTABLE_MATH
USER = 1000   # LT_PROGRAM_USER_BASE: the first program a context registers


# ---------------------------------------------------------------------------------------------- 1: messages and precedence
# A call is a dict: the descriptor's fields by their names, and
#   ctx        "scene" (a context with the Cornell box), "empty" (one without a scene) or "null"
#   desc_null  pass no descriptor
#   n          records
#   inp, out   "ok", "null" or "odd" (8 bytes past a 16-byte boundary; the device forms alone mind)
#   short      out_bytes is one byte less than n results take
# A check is (label, return code, text of lt_hip_last_error, the changes that violate it alone -- one dict or several --, pairs).
# Two neighbouring checks are violated together by both their changes (the first dict of each), unless `pairs` names the other
# check's label: with a dict of changes to use instead, or with None -- no call can violate both, the comment says why.  `pairs`
# may also name a check further down that becomes the neighbour when the one between does not apply to the call's kind.
#
# Not violated alone, because of how the library spells the conditions (the call that violates the check is in the table all the
# same, and gives the check's own text):
#   * "user" of the three query families: a program >= 1000 is also outside the built-in range of "program", the next check;
#   * "kind" of lt_hip_trace_surface: a kind that is neither CLOSEST nor ANY is also not CLOSEST, the next check.
# Not violated together:
#   * "ctx" leaves no context to read a text from: with "desc" the call returns the code, and the text of the null context
#     (lt_hip_create's) stays what it was;
#   * "desc" (a null descriptor) with any descriptor field;
#   * "align" on the host forms: host pointers need no alignment, the check is not made (the table drops it there);
#   * "first_k" with "count", "unknown" with "user" with "gi" / "not_gi": they are about one field, whose values exclude each other;
#   * "small" with anything after it: there is only n == 0 after it, and 0 results fit every buffer.  n == 0 itself is no error:
#     the end of the test calls it on both contexts.
def common(noun, per, null_text, align_text, scene_text):
    return [
        ("n", INVALID, "at most 2^32 - 1 %s per %s" % (noun, per), {"n": 2 ** 32}, {}),
        ("null", INVALID, null_text, [{"inp": "null"}, {"out": "null"}], {"align": {"inp": "null", "out": "odd"}}),
        ("align", INVALID, align_text, [{"inp": "odd"}, {"out": "odd"}], {}),
        ("scene", NO_SCENE, scene_text, {"ctx": "empty"}, {}),
        ("small", TOO_SMALL, "out is smaller than n results", {"short": True}, {}),
    ]


EXCLUDE = "LT_RENDER_FLAG_PORTABLE_MATH and LT_RENDER_FLAG_STRICT_MATH exclude each other"
QUERY_USER = "ray queries take a built-in program (it selects the triangle epsilon)"
QUERY_FLAGS = "ray queries take LT_RENDER_FLAG_STRICT_MATH, LT_RENDER_FLAG_PORTABLE_MATH and LT_TRACE_FLAG_COHERENT only"
QUERY_TAIL = common("rays", "query", "rays or out is NULL", "device rays and out must be 16-byte aligned", "ray query before lt_hip_set_scene")
HEAD = [("ctx", INVALID, None, {"ctx": "null"}, {})]
# lt_hip_trace_rays and lt_hip_trace_surface with LT_TRACE_FLAG_COHERENT launch one workgroup of 64 lanes per 64 rays: 2^32 - 63 rays
# are 2^26 workgroups, 2^32 work-items, one more than a launch holds.  The first n refused, behind the check of n >= 2^32.
COHERENT_N = ("coherent_n", INVALID, "at most 2^32 - 64 rays per query with LT_TRACE_FLAG_COHERENT",
              [{"n": 2 ** 32 - 63, "flags": C.TRACE_FLAG_COHERENT}, {"n": 2 ** 32 - 1, "flags": C.TRACE_FLAG_COHERENT | C.RENDER_FLAG_PORTABLE_MATH}], {})
TRACE_TAIL = QUERY_TAIL[:1] + [COHERENT_N] + QUERY_TAIL[1:]


def trace_checks(surface):
    return HEAD + [
        # (lt_hip_trace_surface shares lt_hip_trace_rays' check, and with it this text)
        ("desc", INVALID, "lt_hip_trace_rays: desc is NULL", {"desc_null": True}, {"size": None}),
        ("size", INVALID, "bad lt_hip_trace_desc (struct_size)", {"struct_size": 12}, {}),
        ("kind", INVALID, "unknown trace kind", {"kind": 7}, {"closest": {"kind": 7}}),
    ] + ([("closest", INVALID, "surface queries take LT_TRACE_CLOSEST", {"kind": C.TRACE_ANY}, {})] if surface else []) + [
        ("user", INVALID, QUERY_USER, {"program": USER}, {"program": {"program": USER}}),
        ("program", UNKNOWN, "unknown program", [{"program": 6}, {"program": -1}], {}),
        ("flags", INVALID, QUERY_FLAGS, [{"flags": C.RENDER_FLAG_STATS}, {"flags": 0x200}], {"exclude": {"flags": BOTH | C.RENDER_FLAG_STATS}}),
        ("exclude", INVALID, EXCLUDE, {"flags": BOTH}, {}),
    ] + TRACE_TAIL


HITS_CHECKS = HEAD + [
    ("desc", INVALID, "lt_hip_trace_hits: desc is NULL", {"desc_null": True}, {"size": None}),
    ("size", INVALID, "bad lt_hip_multihit_desc (struct_size)", {"struct_size": 20}, {}),
    ("kind", INVALID, "unknown multi-hit kind", {"kind": 7}, {}),
    ("user", INVALID, QUERY_USER, {"program": USER}, {"program": {"program": USER}}),
    ("program", UNKNOWN, "unknown program", [{"program": 6}, {"program": -1}], {}),
    ("flags", INVALID, QUERY_FLAGS, [{"flags": C.RENDER_FLAG_STATS}, {"flags": 0x200}], {"exclude": {"flags": BOTH | C.RENDER_FLAG_STATS}}),
    ("exclude", INVALID, EXCLUDE, {"flags": BOTH}, {"count": {"flags": BOTH, "kind": C.TRACE_COUNT, "max_hits": 1}}),
    ("first_k", INVALID, "LT_TRACE_FIRST_K takes max_hits in 1 .. LT_TRACE_MAX_HITS",
     [{"kind": C.TRACE_FIRST_K, "max_hits": 0}, {"kind": C.TRACE_FIRST_K, "max_hits": C.TRACE_MAX_HITS + 1}],
     {"count": None, "reserved": {"kind": C.TRACE_FIRST_K, "max_hits": 0, "reserved": 1}}),
    ("count", INVALID, "LT_TRACE_COUNT takes max_hits = 0", {"kind": C.TRACE_COUNT, "max_hits": 1}, {}),
    ("reserved", INVALID, "lt_hip_multihit_desc::reserved must be 0", {"reserved": 1}, {}),
] + QUERY_TAIL

AT_CHECKS = HEAD + [
    ("desc", INVALID, "lt_hip_surface_at: desc is NULL", {"desc_null": True}, {"size": None}),
    ("size", INVALID, "bad lt_hip_surface_desc (struct_size)", {"struct_size": 4}, {}),
    ("flags", INVALID, "lt_hip_surface_at takes LT_RENDER_FLAG_STRICT_MATH and LT_RENDER_FLAG_PORTABLE_MATH only",
     [{"flags": C.TRACE_FLAG_COHERENT}, {"flags": C.RENDER_FLAG_STATS}], {"exclude": {"flags": BOTH | C.TRACE_FLAG_COHERENT}}),
    ("exclude", INVALID, EXCLUDE, {"flags": BOTH}, {}),
] + common("hit records", "call", "hits or out is NULL", "device hits and out must be 16-byte aligned", "lt_hip_surface_at before lt_hip_set_scene")


def shade_checks(name, struct, small_size, user_text, program_check, flags_noun, more):
    return HEAD + [
        ("desc", INVALID, "%s: desc is NULL" % name, {"desc_null": True}, {"size": None}),
        ("size", INVALID, "bad %s (struct_size)" % struct, {"struct_size": small_size}, {}),
        # (a user program the context has not registered is unknown, a registered one refused: ids 1001 and 1000 here)
        ("unknown", UNKNOWN, "unknown program", [{"program": 6}, {"program": -1}, {"program": USER + 1}], {"user": None, "mode": {"program": 6, "kernel_mode": 2}}),
        ("user", INVALID, user_text, {"program": USER}, {program_check[0]: None, "mode": {"program": USER, "kernel_mode": 2}}),
        program_check,
        ("mode", INVALID, "unknown kernel mode", [{"kernel_mode": 2}, {"kernel_mode": -1}], {}),
        ("flags", INVALID, "%s take LT_RENDER_FLAG_STRICT_MATH, LT_RENDER_FLAG_PORTABLE_MATH and LT_TRACE_FLAG_COHERENT only" % flags_noun,
         [{"flags": C.RENDER_FLAG_STATS}, {"flags": 0x200}], {"exclude": {"flags": BOTH | C.RENDER_FLAG_STATS}}),
        ("exclude", INVALID, EXCLUDE, {"flags": BOTH}, {}),
        ("frames", INVALID, "%s::frame_count must be at least 1" % struct, {"frame_count": 0}, {}),
    ] + more + common("rays", "call", "rays or out is NULL", "device rays and out must be 16-byte aligned", "%s before lt_hip_set_scene" % name)


SHADE_CHECKS = shade_checks(
    "lt_hip_shade_rays", "lt_hip_shade_desc", 20, "lt_hip_shade_rays does not take user programs",
    ("gi", INVALID, "lt_hip_shade_rays does not take the global-illumination programs (their pipeline is indexed by pixel)",
     [{"program": C.PROGRAM_GLOBAL_ILLUMINATION}, {"program": C.PROGRAM_GLOBAL_ILLUMINATION_25}], {}), "shaded rays", [])
PATHS_CHECKS = shade_checks(
    "lt_hip_shade_paths", "lt_hip_paths_desc", 28, "lt_hip_shade_paths does not take user programs (nor does lt_hip_shade_rays)",
    ("not_gi", INVALID, "lt_hip_shade_paths takes the global-illumination programs only: this program's entry point is lt_hip_shade_rays",
     [{"program": p} for p in (C.PROGRAM_BASIC, C.PROGRAM_BASIC_LIGHTING, C.PROGRAM_ACCUMULATOR, C.PROGRAM_CUSTOM_OPENCL)], {}), "shaded paths",
    [("depth", INVALID, "gi_max_depth out of range", [{"gi_max_depth": 65}, {"gi_max_depth": -1}], {}),
     ("reserved", INVALID, "lt_hip_paths_desc::reserved must be 0", {"reserved": 1}, {})])


# The point and box families have no program and no flags: the descriptor's own rules (one function per family, for the context's
# entry points and the GPU-free form alike) come first, in the order of the fields' dependence -- flags, kind, then max_k as the
# kind reads it.  Not violated together:
#   * "kind" with "first_k" or "count": an unknown kind is neither of the kinds whose max_k is checked; its neighbour is "n";
#   * "first_k" with "count": the two are about max_k under kinds that exclude each other; "first_k" is paired with "n" instead.
def plain_checks(name, struct, small_size, noun, more):
    return HEAD + [
        ("desc", INVALID, "%s: desc is NULL" % name, {"desc_null": True}, {"size": None}),
        ("size", INVALID, "bad %s (struct_size)" % struct, {"struct_size": small_size}, {}),
        ("flags", INVALID, "%s takes no flags" % name, [{"flags": 1}, {"flags": C.RENDER_FLAG_STRICT_MATH}, {"flags": C.TRACE_FLAG_COHERENT}], {}),
    ] + more + common(noun, "call", "%s or out is NULL" % noun, "device %s and out must be 16-byte aligned" % noun, "%s before lt_hip_set_scene" % name)


NEAREST_CHECKS = plain_checks("lt_hip_nearest_points", "lt_hip_nearest_desc", 4, "points", [])
NEAREST_K_CHECKS = plain_checks("lt_hip_nearest_k", "lt_hip_nearest_k_desc", 12, "points", [
    ("kind", INVALID, "unknown nearest kind", [{"kind": 2}, {"kind": -1}], {"first_k": None, "n": {"kind": 2, "n": 2 ** 32}}),
    ("first_k", INVALID, "LT_NEAREST_FIRST_K takes max_k in 1 .. LT_NEAREST_MAX_K",
     [{"kind": C.NEAREST_FIRST_K, "max_k": 0}, {"kind": C.NEAREST_FIRST_K, "max_k": C.NEAREST_MAX_K + 1}],
     {"count": None, "n": {"kind": C.NEAREST_FIRST_K, "max_k": 0, "n": 2 ** 32}}),
    ("count", INVALID, "LT_NEAREST_COUNT takes max_k = 0", {"kind": C.NEAREST_COUNT, "max_k": 1}, {}),
])
OVERLAP_CHECKS = plain_checks("lt_hip_overlap_boxes", "lt_hip_overlap_desc", 12, "boxes", [
    ("kind", INVALID, "unknown overlap kind", [{"kind": 3}, {"kind": -1}], {"first_k": None, "n": {"kind": 3, "n": 2 ** 32}}),
    ("first_k", INVALID, "LT_OVERLAP_FIRST_K takes max_k in 1 .. LT_OVERLAP_MAX_K",
     [{"kind": C.OVERLAP_FIRST_K, "max_k": 0}, {"kind": C.OVERLAP_FIRST_K, "max_k": C.OVERLAP_MAX_K + 1}],
     {"count": None, "n": {"kind": C.OVERLAP_FIRST_K, "max_k": 0, "n": 2 ** 32}}),
    ("count", INVALID, "LT_OVERLAP_COUNT and LT_OVERLAP_ANY take max_k = 0",
     [{"kind": C.OVERLAP_COUNT, "max_k": 1}, {"kind": C.OVERLAP_ANY, "max_k": 1}], {}),
])


def result_bytes(family, call):
    """bytes of one result record of the call"""
    if family == "nearest_points":
        return 16
    if family == "nearest_k":
        return 4 if call["kind"] == C.NEAREST_COUNT else 16 * call["max_k"]
    if family == "overlap_boxes":
        return 4 * call["max_k"] if call["kind"] == C.OVERLAP_FIRST_K else 4
    if family == "trace_rays":
        return 4 if call["kind"] == C.TRACE_ANY else 16
    if family == "trace_hits":
        return 4 if call["kind"] == C.TRACE_COUNT else 16 * call["max_hits"]
    return 48 if family in ("trace_surface", "surface_at") else 16


# family: (descriptor, a valid call's descriptor fields, bytes of an input record, checks)
FAMILIES = {
    "trace_rays": (C.TraceDesc, {"program": C.PROGRAM_ACCUMULATOR, "kind": C.TRACE_CLOSEST, "flags": 0}, 32, trace_checks(False)),
    "trace_hits": (C.MultiHitDesc, {"program": C.PROGRAM_ACCUMULATOR, "kind": C.TRACE_FIRST_K, "flags": 0, "max_hits": 2, "reserved": 0}, 32, HITS_CHECKS),
    "trace_surface": (C.TraceDesc, {"program": C.PROGRAM_ACCUMULATOR, "kind": C.TRACE_CLOSEST, "flags": 0}, 32, trace_checks(True)),
    "surface_at": (C.SurfaceDesc, {"flags": 0}, 16, AT_CHECKS),
    "shade_rays": (C.ShadeDesc, {"program": C.PROGRAM_ACCUMULATOR, "kernel_mode": C.KERNEL_MODE_LINEAR, "flags": 0, "frame_first": 0, "frame_count": 1}, 32,
                   SHADE_CHECKS),
    "shade_paths": (C.PathsDesc, {"program": C.PROGRAM_GLOBAL_ILLUMINATION, "kernel_mode": C.KERNEL_MODE_LINEAR, "flags": 0, "frame_first": 0,
                                  "frame_count": 1, "gi_max_depth": 2, "reserved": 0}, 32, PATHS_CHECKS),
    "nearest_points": (C.NearestDesc, {"flags": 0}, 16, NEAREST_CHECKS),
    "nearest_k": (C.NearestKDesc, {"flags": 0, "kind": C.NEAREST_FIRST_K, "max_k": 2}, 16, NEAREST_K_CHECKS),
    "overlap_boxes": (C.OverlapDesc, {"flags": 0, "kind": C.OVERLAP_FIRST_K, "max_k": 2}, 32, OVERLAP_CHECKS),
}
ENTRY_POINTS = [(f, device) for f in FAMILIES for device in (False, True)]


def first(changes):
    return changes[0] if isinstance(changes, list) else changes


def violations(checks):
    """(what, expected check, changes) of every call the table asks for"""
    for i, (label, code, text, alone, pairs) in enumerate(checks):
        for k, changes in enumerate(alone if isinstance(alone, list) else [alone]):
            yield "%s alone (%d)" % (label, k), checks[i], changes
        others = [checks[i + 1][0]] if i + 1 < len(checks) else []
        others += [o for o in pairs if o not in others]
        for other in others:
            theirs = [c for c in checks if c[0] == other]
            if not theirs or (other in pairs and pairs[other] is None):
                continue   # (the other check is not made by this entry point; or the two exclude each other)
            yield "%s with %s" % (label, other), checks[i], pairs[other] if other in pairs else {**first(theirs[0][3]), **first(alone)}


class Caller:
    """makes the calls of one entry point on two contexts, over buffers that keep a fill pattern"""
    N = 4

    def __init__(self, with_scene, empty, family, device):
        import torch
        self.L = with_scene._L
        self.ctx = {"scene": with_scene._ctx, "empty": empty._ctx, "null": None}
        self.family, self.device = family, device
        self.Desc, self.fields, self.in_bytes, _ = FAMILIES[family]
        self.fn = getattr(self.L, "lt_hip_" + family + ("_device" if device else ""))
        words = self.N * 16 * C.TRACE_MAX_HITS // 4 + 4
        if device:
            self.inp = torch.zeros(self.N * 8 + 4, dtype=torch.float32, device="cuda")
            self.out = torch.full((words,), FILL, dtype=torch.int32, device="cuda")
            self.inp_ptr, self.out_ptr = self.inp.data_ptr(), self.out.data_ptr()
        else:
            self.inp = np.zeros(self.N * 8 + 4, dtype=np.float32)
            self.out = np.full(words, FILL, dtype=np.uint32)
            self.inp_ptr, self.out_ptr = self.inp.ctypes.data, self.out.ctypes.data
        assert self.inp_ptr % 16 == 0 and self.out_ptr % 16 == 0
        self.out_bytes = words * 4 - 16

    def untouched(self):
        return bool(((self.out.cpu().numpy().view(np.uint32) if self.device else self.out) == FILL).all())

    def __call__(self, changes):
        call = dict(self.fields, struct_size=ctypes.sizeof(self.Desc), ctx="scene", desc_null=False, n=self.N, inp="ok", out="ok", short=False)
        assert set(changes) <= set(call), changes
        call.update(changes)
        d = self.Desc()
        for k, _ in self.Desc._fields_:
            setattr(d, k, call[k])
        where = {"ok": 0, "odd": 8}
        args = [self.ctx[call["ctx"]], None if call["desc_null"] else ctypes.byref(d),
                None if call["inp"] == "null" else ctypes.c_void_p(self.inp_ptr + where[call["inp"]]), call["n"],
                None if call["out"] == "null" else ctypes.c_void_p(self.out_ptr + where[call["out"]]),
                call["n"] * result_bytes(self.family, call) - 1 if call["short"] else self.out_bytes]
        ctx = args[0]
        if ctx is not None:   # a text no entry point gives: what is read after the call is the call's
            assert self.L.lt_hip_untile(ctx, None, 0, 0, 0, 0, 0, 0, 0, None, None) == INVALID
            assert self.L.lt_hip_last_error(ctx) == b"lt_hip_untile: bad argument"
        before = self.L.lt_hip_last_error(None)
        rc = self.fn(*args, *([None] if self.device else []))
        after = self.L.lt_hip_last_error(ctx)
        return rc, (None if ctx is None and after == before else after.decode())


@pytest.fixture(scope="module")
def contexts():
    with_scene, empty = RendererHIP(0), RendererHIP(0)
    with_scene.set_scene(F.scene(SCENE))
    assert with_scene.resolve_program(USER_PROGRAM) == USER   # (registered: the shade families tell it from 1001)
    yield with_scene, empty
    with_scene.close()
    empty.close()


@pytest.mark.parametrize("family,device", ENTRY_POINTS)
def test_every_check_gives_its_code_and_text_and_the_earlier_of_two_wins(contexts, family, device):
    import torch
    call = Caller(*contexts, family, device)
    checks = [c for c in FAMILIES[family][3] if device or c[0] != "align"]
    for what, (label, code, text, _, _), changes in violations(checks):
        assert call(changes) == (code, text), (family, device, what, changes)
        if not device:
            assert call.untouched(), (family, what)
    # n == 0 is no error and comes after every check: without a scene it is refused, with one nothing is read or written
    assert call({"n": 0, "ctx": "empty", "inp": "null", "out": "null"})[0] == NO_SCENE
    assert call({"n": 0})[0] == 0
    assert call({"n": 0, "inp": "null", "out": "null"})[0] == 0
    if device:
        assert call({"n": 0, "inp": "odd", "out": "odd"})[0] == 0
        torch.cuda.synchronize()
    assert call.untouched(), family


@pytest.mark.parametrize("device", [False, True])
def test_the_coherent_limit_narrows_the_packet_grid_alone(contexts, device):
    """n = 2^32 - 64 with LT_TRACE_FLAG_COHERENT, and n = 2^32 - 1 without it or in a family that has no packet kernel, pass every
    check about n: such a call goes on to the next thing wrong with it, the room for its results."""
    small = (TOO_SMALL, "out is smaller than n results")
    for family in ("trace_rays", "trace_surface"):
        call = Caller(*contexts, family, device)
        assert call({"n": 2 ** 32 - 64, "flags": C.TRACE_FLAG_COHERENT}) == small, family
        assert call({"n": 2 ** 32 - 1}) == small, family
        assert call({"n": 2 ** 32 - 63, "flags": C.TRACE_FLAG_COHERENT})[0] == INVALID, family
    for family in ("trace_hits", "shade_rays", "shade_paths"):
        assert Caller(*contexts, family, device)({"n": 2 ** 32 - 1, "flags": C.TRACE_FLAG_COHERENT}) == small, family
    assert Caller(*contexts, "surface_at", device)({"n": 2 ** 32 - 1}) == small


# ---------------------------------------------------------------------------------------------- 2 - 4: the calls themselves
SIZES = (1, 63, 64, 65, 130)   # one lane, one short of a wave, a wave, one over, two waves and a bit
# variant: (method, arguments, input, kernel launches -- shade_paths: test_gpu_shade_paths.py's count for one set of the LDS-scene
# form: two for the camera rays, the primary stage, gi_max_depth bounce stages, the resolve --, counter that holds n)
VARIANTS = {
    "trace_rays": ("trace_rays", {}, "rays", 1, "rays"),
    "trace_rays_any": ("trace_rays", {"any_hit": True}, "rays", 1, "shadow_rays"),
    "trace_hits": ("trace_hits", {"max_hits": 4}, "rays", 1, "rays"),
    "trace_hits_count": ("trace_hits", {"count": True}, "rays", 1, "rays"),
    "trace_surface": ("trace_surface", {}, "rays", 2, "rays"),
    "surface_at": ("surface_at", {}, "hits", 1, None),
    "shade_rays": ("shade_rays", {"frame_count": 2}, "shade", 1, "rays"),
    "shade_paths": ("shade_paths", {"gi_max_depth": 2, "frame_count": 2}, "shade", 2 + 1 + 2 + 1, "rays"),
    "nearest_points": ("nearest_points", {}, "points", 1, "rays"),
    "nearest_k": ("nearest_k", {"k": 3}, "points", 1, "rays"),
    "nearest_k_count": ("nearest_k", {"count": True}, "points", 1, "rays"),
    "overlap_boxes": ("overlap_boxes", {"k": 3}, "boxes", 1, "rays"),
    "overlap_count": ("overlap_boxes", {"count": True}, "boxes", 1, "rays"),
    "overlap_any": ("overlap_boxes", {"any": True}, "boxes", 1, "rays"),
}


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    r.set_scene(F.scene(SCENE))
    yield r
    r.close()


@pytest.fixture(scope="module")
def inputs(renderer):
    """130 records of each kind of input: lt_hip_ray, lt_hip_shade_ray, lt_hip_hit as (n, 1) of trace_hits, lt_hip_point and
    lt_hip_box (tests/nearest_k.py's and tests/overlap.py's families, shuffled: hits and misses among any 63 of them)"""
    s = F.scene(SCENE)
    rng = np.random.default_rng(5)
    q = random_rays(s, rng, 130)
    q = np.ascontiguousarray(np.concatenate([q[:98], q[-32:]]))   # (rays of every kind, then half a coherent chunk)
    shade = make_shade_rays(q[:, 0:3], q[:, 4:7], rng.uniform(-0.5, 0.5, len(q)), rng.uniform(-0.5, 0.5, len(q)))
    hits = renderer.trace_hits(q, max_hits=1)
    assert hits.shape == (130, 1) and hits.dtype == HIT_DTYPE and (hits["prim"] >= 0).any() and (hits["prim"] < 0).any()
    points = np.concatenate(list(nk.families(s, seed=5, n=48).values()))
    points = np.ascontiguousarray(points[rng.permutation(len(points))[:130]])
    boxes = np.concatenate(list(ov.families(s, seed=5, n=48).values()))
    boxes = np.ascontiguousarray(boxes[rng.permutation(len(boxes))[:130]])
    near, touched = nearest_points_host(s, points[:63])["prim"], overlap_boxes_host(s, boxes[:63], any=True)
    assert (near >= 0).sum() >= 8 and (near < 0).sum() >= 8 and (touched == 1).sum() >= 8 and (touched == 0).sum() >= 8
    return {"rays": F.frozen(q), "shade": F.frozen(shade), "hits": F.frozen(hits), "points": F.frozen(points), "boxes": F.frozen(boxes)}


def words(a):
    """the result's bytes as uint32, flat: numpy of the host forms, torch of the device forms"""
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def host_call(r, variant, inputs, n):
    method, kw, kind, _, _ = VARIANTS[variant]
    return getattr(r, method)(np.ascontiguousarray(inputs[kind][:n]), **kw)


def on_device(inputs, n):
    """the first n records of each input as float32 tensors on the GPU; the caller keeps them until its stream is done"""
    import torch
    tensors = {}
    for kind, a in inputs.items():
        a = np.array(a[:n])   # (a copy: the fixtures are read-only)
        tensors[kind] = torch.from_numpy(a.view(np.float32).reshape(a.shape + (4,)) if kind == "hits" else a).cuda()
    torch.cuda.synchronize()
    return tensors


def device_call(r, variant, tensors, stream):
    method, kw, kind, _, _ = VARIANTS[variant]
    return getattr(r, method)(tensors[kind], stream=stream, **kw)


def check_stats(r, variant, n):
    _, _, _, launches, counter = VARIANTS[variant]
    st = r.stats()
    assert st["own_tree_height"] > 0
    assert st["kernel_launches"] == launches and st["render_ms"] == 0, (variant, n, st)
    for k in ("rays", "shadow_rays"):
        assert st[k] == (n if k == counter else 0), (variant, n, k, st)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_host_and_device_forms_agree_and_report_the_same(renderer, inputs, variant):
    import torch
    side = torch.cuda.Stream()
    for n in SIZES:
        host = host_call(renderer, variant, inputs, n)
        check_stats(renderer, variant, n)
        tensors = on_device(inputs, n)
        got = device_call(renderer, variant, tensors, side)
        side.synchronize()
        check_stats(renderer, variant, n)
        assert len(host) == len(got) == n and np.array_equal(words(host), words(got)), (variant, n)
    assert (words(host) != 0).any()


SEQUENCE = (("trace_rays", 130), ("shade_rays", 1), ("trace_surface", 65), ("surface_at", 65), ("trace_hits", 64), ("shade_paths", 63), ("trace_rays", 1),
            # records of 16 bytes in with 128 out, and of 32 in with 4 out
            ("nearest_k", 130), ("overlap_any", 65), ("nearest_points", 64), ("overlap_boxes", 63), ("trace_rays", 1))
SEQUENCE_ARGS = {"trace_hits": {"max_hits": 8}, "nearest_k": {"k": 8}, "overlap_boxes": {"k": 8}}


def sequence_call(r, variant, inputs, n):
    method, kw, kind, _, _ = VARIANTS[variant]
    return getattr(r, method)(np.ascontiguousarray(inputs[kind][:n]), **SEQUENCE_ARGS.get(variant, kw))


def test_the_shared_staging_buffers_grow_and_are_reused_across_record_sizes(renderer, inputs):
    got = [sequence_call(renderer, v, inputs, n) for v, n in SEQUENCE]
    for (v, n), g in zip(SEQUENCE, got):
        fresh = RendererHIP(0)
        try:
            fresh.set_scene(F.scene(SCENE))
            want = sequence_call(fresh, v, inputs, n)
        finally:
            fresh.close()
        assert g.shape == want.shape and g.shape[0] == n and np.array_equal(words(g), words(want)), (v, n)
    assert got[3].shape == (65, 1) and got[4].shape == (64, 8)


def test_all_families_back_to_back_on_one_caller_stream(renderer, inputs):
    import torch
    side = torch.cuda.Stream()
    n = 130
    tensors = on_device(inputs, n)
    got = {v: device_call(renderer, v, tensors, side) for v in VARIANTS}
    side.synchronize()
    for v in VARIANTS:
        assert np.array_equal(words(got[v]), words(host_call(renderer, v, inputs, n))), v
