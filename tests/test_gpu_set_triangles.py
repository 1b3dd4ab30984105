"""GPU (-m gpu): scenes made resident from bare triangles (lt_hip_set_triangles / _device, RendererHIP.set_triangles).

a. The four resident buffers (scene_buffers) equal the host form of the canonical median build (tests/build_scene.py: host(name),
   which the CPU tests hold against the numpy model and the reference's builder) byte for byte on every shape, from numpy arrays
   and from torch tensors, under LT_DEVICE_BUILD=0 and =1, in a plain context and in one whose pool hands out buffers filled with
   0xFF (a few shapes also with 0x00 and 0x7F): the build reads no word it has not written.
b. Plumbing: a context that did set_triangles(T) and one that did set_scene(build_scene_host(T)) hold the same derived structures
   (scene_structure 0..5), render the same 64 x 64 accumulator picture and report the same 4096 closest hits, bit for bit.
c. History: over a resident set_scene scene and the reverse, with equal sizes -- the second scene's results both times, never the
   unchanged-scene shortcut, also through render() (lt_hip_render_scene); a rejected call leaves the scene before it in place; a
   moved mesh gives the moved mesh's hits.
No tolerance anywhere in this file."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, RenderPropertiesHIP, make_desc, make_rays
from tests import build_scene as B

pytestmark = pytest.mark.gpu

CAMERA = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 3)
ACCUMULATOR = "examples/accumulator/resources/kernels/accumulator.cl"
KINDS = (0, 1, 2, 3, 4, 5)


def ids(names):
    return [n if isinstance(n, str) else "%s%d" % n for n in names]


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


_contexts = {}


def context(poison=None):
    """One context per poison byte for the whole module (LT_DEBUG_POISON is read when a context is created)."""
    if poison not in _contexts:
        with environment(LT_DEBUG_POISON=None if poison is None else "0x%02X" % poison):
            _contexts[poison] = RendererHIP(0)
    return _contexts[poison]


def fresh():
    with environment(LT_DEBUG_POISON=None):
        return RendererHIP(0)


def teardown_module(module):
    for r in _contexts.values():
        r.close()
    _contexts.clear()


def tensors(shape):
    """A shape's arrays (its name, or the four arrays themselves) as torch tensors on the GPU, materials as their bytes."""
    import torch
    pos, nrm, mi, mats = shape if isinstance(shape, tuple) and isinstance(shape[0], np.ndarray) else B.triangles(shape)
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(np.ascontiguousarray(pos)).to(dev), torch.from_numpy(np.ascontiguousarray(nrm)).to(dev),
            None if mi is None else torch.from_numpy(np.ascontiguousarray(mi)).to(dev),
            torch.from_numpy(np.ascontiguousarray(mats).view(np.uint8).reshape(-1).copy()).to(dev))


def render_resident(r, W=64, H=64):
    """A 64 x 64 accumulator frame of whatever scene is resident (lt_hip_render: no scene is handed over)."""
    d = make_desc(C.PROGRAM_ACCUMULATOR, W, H, 3, CAMERA)
    out = np.zeros((H, W, 3), dtype=np.float32)
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def rays4096():
    rng = np.random.default_rng(77)
    n = 4096
    o = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 8, n), np.full(n, -30.0)], axis=-1)
    target = np.stack([rng.uniform(-4, 4, n), rng.uniform(-1.5, 6.5, n), rng.uniform(-6, 1, n)], axis=-1)
    return make_rays(o, target - o)


RAYS = rays4096()


def results(r):
    """What the tests compare of a resident scene: the derived structures, a picture, closest hits -- as bytes."""
    parts = [r.scene_structure(k) for k in KINDS]
    parts = [None if p is None else np.asarray(p).tobytes() for p in parts]
    return parts + [render_resident(r).tobytes(), r.trace_rays(RAYS).tobytes()]


def reference_results(scene):
    """... of `scene` handed to lt_hip_set_scene in a context of its own."""
    r = fresh()
    try:
        r.set_scene(scene)
        return results(r)
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------- a. the four buffers
@pytest.mark.parametrize("device_build", ["0", "1"])
@pytest.mark.parametrize("name", B.NAMES, ids=ids(B.NAMES))
def test_resident_buffers_equal_host_form(name, device_build, monkeypatch):
    monkeypatch.setenv("LT_DEVICE_BUILD", device_build)
    want = B.host(name)
    n = want.n_prims
    for poison in (None, 0xFF):
        r = context(poison)
        before = r.stats()["scene_uploads"]
        r.set_triangles(*B.triangles(name))
        assert B.same_bytes(r.scene_buffers(), want) == [], ("numpy", poison)
        info = r.scene_structure(3)
        if name in B.DECLINED:
            assert r.scene_structure(0) is None and info[3] == 0   # no own hierarchy: every ray walks the tree that was built
        elif n >= 64:
            assert info[3] == int(device_build) and r.scene_structure(0) is not None
        r.set_triangles(*tensors(name))
        assert B.same_bytes(r.scene_buffers(), want) == [], ("torch", poison)
        assert r.stats()["scene_uploads"] == before + 2


@pytest.mark.parametrize("poison", [0x00, 0x7F])
@pytest.mark.parametrize("name", [("random", 65), ("random", 4097), "quads300", "emissive_200"], ids=ids([("random", 65), ("random", 4097), "quads300", "emissive_200"]))
def test_other_poison_bytes(name, poison, monkeypatch):
    monkeypatch.delenv("LT_DEVICE_BUILD", raising=False)
    r = context(poison)
    r.set_triangles(*B.triangles(name))
    assert B.same_bytes(r.scene_buffers(), B.host(name)) == []


def test_size_rule_without_the_switch(monkeypatch):
    """8193 nodes: prepared on the device by default; 8191: on the host."""
    monkeypatch.delenv("LT_DEVICE_BUILD", raising=False)
    r = context()
    for n, prepared in ((4096, 0), (4097, 1)):
        r.set_triangles(*B.triangles(("random", n)))
        assert r.scene_structure(3)[3] == prepared
        assert B.same_bytes(r.scene_buffers(), B.host(("random", n))) == []


def test_scene_buffers_of_a_set_scene_scene():
    """lt_hip_read_scene_buffer reads any resident scene; size-only calls, a short buffer, no scene."""
    r = fresh()
    try:
        n = ctypes.c_uint64(0)
        assert r._L.lt_hip_read_scene_buffer(r._ctx, 0, None, 0, ctypes.byref(n)) == C.LT_ERR_NO_SCENE
        s = B.host("quads300")
        r.set_scene(s)
        assert B.same_bytes(r.scene_buffers(), s) == []
        assert r.scene_buffers(CAMERA).camera == CAMERA
        for which, size in enumerate((s.nodes.size, s.prims.size, s.materials.size, 260)):
            assert r._L.lt_hip_read_scene_buffer(r._ctx, which, None, 0, ctypes.byref(n)) == C.LT_OK and n.value == size
        buf = np.full(s.nodes.size - 1, 0xAB, np.uint8)
        assert r._L.lt_hip_read_scene_buffer(r._ctx, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, ctypes.byref(n)) == C.LT_ERR_BUFFER_TOO_SMALL
        assert (buf == 0xAB).all()
        for which in (-1, 4):
            assert r._L.lt_hip_read_scene_buffer(r._ctx, which, None, 0, ctypes.byref(n)) == C.LT_ERR_INVALID_ARGUMENT
        assert r._L.lt_hip_read_scene_buffer(r._ctx, 0, None, 0, None) == C.LT_ERR_INVALID_ARGUMENT
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------- b. plumbing
PLUMBING = [("random", 257), ("random", 4097), "quads300", "lattice", "emissive_200"]
_reference = {}


def reference(name, device_build):
    if (name, device_build) not in _reference:
        with environment(LT_DEVICE_BUILD=device_build):
            _reference[(name, device_build)] = reference_results(B.host(name))
    return _reference[(name, device_build)]


@pytest.mark.parametrize("device_build", ["0", "1"])
@pytest.mark.parametrize("name", PLUMBING, ids=ids(PLUMBING))
def test_plumbing_equals_set_scene_of_the_host_form(name, device_build, monkeypatch):
    monkeypatch.setenv("LT_DEVICE_BUILD", device_build)
    want = reference(name, device_build)
    r = context(0xFF)
    r.set_triangles(*B.triangles(name))
    got = results(r)
    assert [g == w for g, w in zip(got, want)] == [True] * len(want)
    assert any(np.frombuffer(got[-1], dtype=C.HIT_DTYPE)["prim"] >= 0)   # (the rays do hit something)


# ---------------------------------------------------------------------------------------------------------- c. history
def moved(name, by):
    pos, nrm, mi, mats = B.triangles(name)
    return (pos + np.asarray(by, np.float32)).astype(np.float32), nrm, mi, mats


@pytest.mark.parametrize("device_build", ["0", "1"])
def test_history_with_set_scene_of_equal_sizes(device_build, monkeypatch):
    monkeypatch.setenv("LT_DEVICE_BUILD", device_build)
    t1, t2 = B.triangles(("random", 257)), moved(("random", 257), (0.5, -0.25, 0.125))
    s1, s2 = sc.build_from_triangles_canonical(*t1), sc.build_from_triangles_canonical(*t2)
    assert [a.size for a in (s1.nodes, s1.prims, s1.materials, s1.lights)] == [a.size for a in (s2.nodes, s2.prims, s2.materials, s2.lights)]
    want1, want2 = reference_results(s1), reference_results(s2)
    assert want1[-1] != want2[-1] and want1[-2] != want2[-2]
    r = fresh()
    try:
        r.set_scene(s1)
        r.set_triangles(*t2)                       # over a set_scene scene
        assert results(r) == want2
        r.set_scene(s1)                            # and the reverse
        assert results(r) == want1
        r.set_triangles(*t2)
        st = r.stats()
        r.set_scene(s2)                            # the very bytes that are resident: still an upload, never "unchanged"
        after = r.stats()
        assert (after["scene_uploads"], after["scene_reused"]) == (st["scene_uploads"] + 1, st["scene_reused"])
        assert results(r) == want2
        # lt_hip_render_scene over a built scene: the picture of the scene that came with the frame, hashed first, not speculated
        r.set_triangles(*t2)
        out = np.zeros((64, 64, 3), dtype=np.float32)
        r.render(RenderPropertiesHIP(ACCUMULATOR, (64, 64, 3), out, s1, pCamera=CAMERA))
        assert out.tobytes() == want1[-2]
        assert r.stats()["scene_reused"] == st["scene_reused"]
    finally:
        r.close()


def test_moved_mesh_and_tensor_reuse():
    """set_triangles twice: the second mesh's hits; the caller's tensors may be overwritten once the call has returned."""
    t1, t2 = B.triangles(("random", 4097)), moved(("random", 4097), (-0.75, 0.5, 0.25))
    want2 = reference_results(sc.build_from_triangles_canonical(*t2))
    r = context(0xFF)
    r.set_triangles(*tensors(("random", 4097)))
    dev = tensors(t2)
    r.set_triangles(*dev)
    for t in dev:
        t.zero_()
    import torch
    torch.cuda.synchronize()
    assert results(r) == want2


@pytest.mark.parametrize("device_build", ["0", "1"])
def test_rejected_call_leaves_the_scene(device_build, monkeypatch):
    monkeypatch.setenv("LT_DEVICE_BUILD", device_build)
    name = ("random", 257)
    r = fresh()
    try:
        r.set_triangles(*B.triangles(name))
        want = results(r)
        st = r.stats()
        pos, nrm, mi, mats = B.triangles(name)
        bad_pos = pos.copy()
        bad_pos[100, 1, 2] = np.nan
        bad_mi = mi.copy()
        bad_mi[200] = 3
        for args, text in (((bad_pos, nrm, mi, mats), "non-finite vertex position"), ((pos, nrm, bad_mi, mats), "materialIndex")):
            for form in (lambda a: a, tensors):
                with pytest.raises(C.LensTraceError) as e:
                    r.set_triangles(*form(args))
                assert e.value.code == C.LT_ERR_BAD_SCENE and text in str(e.value)
        with pytest.raises(C.LensTraceError) as e:
            r.set_triangles(pos[:0], nrm[:0], mi[:0], mats)
        assert e.value.code == C.LT_ERR_INVALID_ARGUMENT
        assert r.stats()["scene_uploads"] == st["scene_uploads"]
        assert results(r) == want
    finally:
        r.close()


def test_device_form_alignment():
    """A device pointer that is not 4-byte aligned: LT_ERR_INVALID_ARGUMENT before anything is read."""
    import torch
    r = context()
    pos, nrm, mi, mats = tensors(("random", 5))
    raw = torch.zeros(pos.numel() * 4 + 4, dtype=torch.uint8, device=pos.device)
    d = C.TrianglesDesc(ctypes.sizeof(C.TrianglesDesc), 0, 5, raw.data_ptr() + 1, nrm.data_ptr(), mi.data_ptr(), mats.data_ptr(), mats.numel())
    assert r._L.lt_hip_set_triangles_device(r._ctx, ctypes.byref(d), None) == C.LT_ERR_INVALID_ARGUMENT
