"""GPU (-m gpu): nearest-point queries (lt_hip_nearest_points and its device entry point, lens_trace_amd/csrc/lt_nearest.hip).
Every comparison is of words: the answer is a function of the scene and the point alone (include/lenstrace_hip.h), restated in
numpy by tests/nearest.py -- what that module claims is checked without a GPU in tests/test_nearest_cpu.py.

1. every point family on the base scene, a height-field wall and three scenes at the magnitude limits against the model;
2. sizes 1 .. 4097 of a shuffled batch with LT_TRACE_REFILL 1 and 64;
3. scenes without an own tree (scanned leaf by leaf) and the caller's splits (LT_RETREE=0);
4. the device entry point on a side stream from torch tensors equals the host path and writes nothing behind 16 n bytes;
5. surface_at over the records gives tests/surface.py's records: the closest point and its normal;
6. the contract: every error writes nothing, calls interleave with trace_rays, a render and a scene change, stats() reports the
   call, and the GPU's answers are the host form's;
7. a batch whose points and results both pass byte 2^32 (record 2^28), against its base batch repeated."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import HIT_DTYPE, POINT_DTYPE, RendererHIP, RenderPropertiesHIP, make_points, make_rays, nearest_points_host
from tests import nearest as nr
from tests import query_edges as qe
from tests import surface as sf
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
F32 = np.float32
SCENES = ("base", "wall16", "tiny", "large", "far+")


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def base():
    return qe.base_scene(0)


def scene_of(base, name):
    if name == "base":
        return base
    if name == "wall16":
        return synth.heightfield_wall(16)
    return qe.extreme_scene(base, name)[0]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)


def check(r, scene, pts, note):
    got = r.nearest_points(pts)
    assert got.dtype == HIT_DTYPE and got.shape == (len(pts),)
    want = nr.expected(scene, pts)
    bad = nr.same(got, want)
    assert len(bad) == 0, (note, len(bad), bad[:5], pts[bad[:3]], got[bad[:3]], want[bad[:3]])
    return got


# ------------------------------------------------------------------------------------------------------------- 1: the model
@pytest.mark.parametrize("name", SCENES)
def test_against_the_model(renderer, base, name):
    s = scene_of(base, name)
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    hits = 0
    for fam, pts in nr.families(s, seed=SCENES.index(name)).items():
        got = check(renderer, s, pts, (name, fam))
        hits += int((got["prim"] >= 0).sum())
        if fam == "f_nonfinite":
            assert (got["prim"] == -1).all() and np.array_equal(got["t"].view(np.uint32), pts[:, 3].view(np.uint32))
    assert hits >= 512


# ------------------------------------------------------------------------------------------------------------- 2: sizes
@pytest.fixture(scope="module")
def shuffled(base):
    pts = np.concatenate(list(nr.families(base, seed=5, n=512).values()))
    pts = pts[np.random.default_rng(3).permutation(len(pts))][:4097]
    assert len(pts) == 4097
    return pts, nr.expected(base, pts)


@pytest.mark.parametrize("refill", (1, 64))
def test_batch_sizes_and_refill(renderer, base, shuffled, monkeypatch, refill):
    monkeypatch.setenv("LT_TRACE_REFILL", str(refill))
    pts, want = shuffled
    renderer.set_scene(base)
    for n in (1, 63, 64, 65, 511, 4097):
        got = renderer.nearest_points(pts[:n])
        bad = nr.same(got, want[:n])
        assert len(bad) == 0, (n, refill, bad[:5])
    assert (want["prim"] >= 0).sum() >= 2048 and (want["prim"] < 0).sum() >= 256


# ------------------------------------------------------------------------------------------------------------- 3: other hierarchies
@pytest.mark.parametrize("name", ("nan_bound", "bound_at_limit"))
def test_scenes_without_an_own_tree(renderer, base, name):
    s = qe.extreme_scene(base, name)[0]
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] == -1
    hits = 0
    for fam, pts in nr.families(s, seed=7, n=96).items():
        hits += int((check(renderer, s, pts, (name, fam))["prim"] >= 0).sum())
    assert hits >= 256


def test_the_callers_splits(base, monkeypatch):
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(base)
        assert r.stats()["own_tree_height"] > 0
        hits = 0
        for fam, pts in nr.families(base, seed=9, n=96).items():
            hits += int((check(r, base, pts, fam)["prim"] >= 0).sum())
        assert hits >= 256
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------- 4: the device entry point
def test_the_device_entry_point_on_a_side_stream(renderer, base, shuffled):
    import torch
    pts, want = shuffled
    renderer.set_scene(base)
    side = torch.cuda.Stream()
    for n in (1, 65, 4097):
        host = renderer.nearest_points(pts[:n])
        pt = torch.from_numpy(pts[:n]).cuda()
        with torch.cuda.stream(side):
            got = renderer.nearest_points(pt)
        side.synchronize()
        assert got.shape == (n, 4) and got.dtype == torch.float32
        assert np.array_equal(words(got.cpu().numpy()), words(host)) and len(nr.same(host, want[:n])) == 0, n
        # (n, 3) positions with a per-point max_d2 tensor: the same records
        with torch.cuda.stream(side):
            got3 = renderer.nearest_points(pt[:, 0:3].contiguous(), pt[:, 3].contiguous(), stream=side)
        side.synchronize()
        assert np.array_equal(words(got3.cpu().numpy()), words(host)), n
        buf = torch.full((4 * n + 64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        d = C.NearestDesc(ctypes.sizeof(C.NearestDesc), 0)
        assert renderer._L.lt_hip_nearest_points_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(pt.data_ptr()), n,
                                                        ctypes.c_void_p(buf.data_ptr()), 16 * n, ctypes.c_void_p(side.cuda_stream)) == 0
        side.synchronize()
        out = buf.cpu().numpy()
        assert (out[4 * n:] == 0x5a5a5a5a).all(), n
        assert np.array_equal(out[:4 * n].view(np.uint32).reshape(-1, 4), words(host)), n


# ------------------------------------------------------------------------------------------------------------- 5: surface records
def test_surface_records_of_the_closest_points(renderer, base):
    wall = synth.heightfield_wall(16)
    for s, seed in ((base, 1), (wall, 2)):
        renderer.set_scene(s)
        fam = nr.families(s, seed=seed, n=96)
        pts = np.concatenate([fam[k] for k in ("a_uniform", "b_on", "c_off", "e_max_d2")])
        near = renderer.nearest_points(pts)
        for flavour in sf.FLAVOURS:
            got = renderer.surface_at(near, **sf.FLAVOURS[flavour])
            assert len(sf.same(got, sf.expected(s, near, flavour))) == 0, flavour
        hit = near["prim"] >= 0
        assert hit.sum() >= 256 and (~hit).sum() >= 16
        # the position is the closest point: its squared distance to P is the record's t.  With m = max |P| + max |position|:
        # the interpolation is off by at most 4 ulp of the coordinates per axis, |delta| <= 4 sqrt(3) 2^-24 m, the distance is at
        # most sqrt(3) m, so the squares differ by 2 * 3 * 4 * 2^-24 m^2, and t itself by 7 * 2^-24 R^2 <= 21 * 2^-24 m^2
        # (tests/test_nearest_cpu.py): 45, asserted as 64.
        P = pts[hit, 0:3].astype(np.float64)
        d2 = ((got["position"][hit].astype(np.float64) - P) ** 2).sum(axis=1)
        scale = (np.abs(P).max(axis=1) + np.abs(got["position"][hit]).max(axis=1)) ** 2
        assert (np.abs(d2 - near["t"][hit]) <= 64 * 2.0 ** -24 * scale).all()
        assert (got["material"][hit] >= 0).all() and (got["prim"][~hit] == -1).all()


# ------------------------------------------------------------------------------------------------------------- 6: the contract
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        pts = make_points(np.zeros((4, 3)))
        out = np.full(16, 0x5a5a5a5a, dtype=np.uint32)
        P, O = (x.ctypes.data_as(ctypes.c_void_p) for x in (pts, out))

        def desc(flags=0, size=ctypes.sizeof(C.NearestDesc)):
            return ctypes.byref(C.NearestDesc(size, flags))

        assert L.lt_hip_nearest_points(r._ctx, desc(), P, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        assert (out == 0x5a5a5a5a).all()
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        cases = [
            (None, P, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(size=4), P, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=1), P, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH), P, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(flags=C.TRACE_FLAG_COHERENT), P, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), P, 2 ** 32, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), None, 4, O, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), P, 4, None, out.nbytes, C.LT_ERR_INVALID_ARGUMENT),
            (desc(), P, 4, O, 4 * 16 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
        ]
        for i, (d, pp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_nearest_points(r._ctx, d, pp, n, op, nb) == want, i
            assert (out == 0x5a5a5a5a).all(), i
        assert L.lt_hip_nearest_points(r._ctx, desc(), P, 0, O, 0) == 0 and L.lt_hip_nearest_points(r._ctx, desc(), None, 0, None, 0) == 0
        assert (out == 0x5a5a5a5a).all()
        # the device entry point: the same checks, and 16-byte alignment
        pt = torch.from_numpy(pts).cuda()
        buf = torch.full((32,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        vp = ctypes.c_void_p
        f = L.lt_hip_nearest_points_device
        for pp, op in ((pt.data_ptr() + 4, buf.data_ptr()), (pt.data_ptr(), buf.data_ptr() + 8)):
            assert f(r._ctx, desc(), vp(pp), 3, vp(op), 64, None) == C.LT_ERR_INVALID_ARGUMENT
        assert f(r._ctx, desc(), vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 63, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert f(r._ctx, desc(flags=2), vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 64, None) == C.LT_ERR_INVALID_ARGUMENT
        assert f(r._ctx, None, vp(pt.data_ptr()), 4, vp(buf.data_ptr()), 64, None) == C.LT_ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x5a5a5a5a).all()
        with pytest.raises(ValueError):
            r.nearest_points(np.zeros((4, 2), dtype=F32))
        with pytest.raises(ValueError):
            r.nearest_points(pts, max_d2=1.0)
        # a call that works, on the same context
        got = r.nearest_points(pts.view(POINT_DTYPE).reshape(-1))
        assert (got["prim"] >= 0).all()
    finally:
        r.close()


def test_calls_interleave_and_stats_report_them(base):
    import torch
    s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
    cam = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
    W, H = 96, 64

    def render(r):
        out = np.empty((H, W, 3), dtype=np.float32)
        r.render(RenderPropertiesHIP("accumulator.cl", (W, H, 3), out, s, pCamera=cam, frameCount=4, accumulate=True, portableMath=True))
        return out, r.stats()

    r1, r2 = RendererHIP(0), RendererHIP(0)
    try:
        a1, s1 = render(r1)
        b1, t1 = render(r1)
        a2, s2 = render(r2)
        pts = np.concatenate(list(nr.families(s, seed=4, n=128).values()))
        want = nr.expected(s, pts)
        rng = np.random.default_rng(9)
        rays = make_rays(rng.uniform(-5, 5, (512, 3)) + (0, 2.5, -20), rng.normal(0, 0.2, (512, 3)) + (0, 0, 1))
        hits_before = r2.trace_rays(rays)
        near = r2.nearest_points(pts)
        st = r2.stats()
        assert st["rays"] == len(pts) and st["shadow_rays"] == 0 and st["kernel_launches"] == 1 and st["kernel_ms"] > 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0 and st["node_visits"] == 0
        assert len(nr.same(near, want)) == 0
        assert np.array_equal(words(r2.trace_rays(rays)), words(hits_before))
        b2, t2 = render(r2)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for k in ("frames", "pixels", "rays", "shadow_rays", "node_visits"):
            assert t2[k] == t1[k], k
        # the GPU's answers are the host form's
        assert len(nr.same(near, nearest_points_host(s, pts))) == 0
        assert (want["prim"] >= 0).sum() >= 256
        # set_scene of another scene right behind an enqueued device call: it keeps the old scene's results
        pt = torch.from_numpy(pts).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        got = r2.nearest_points(pt, stream=stream)
        r2.set_scene(base)
        stream.synchronize()
        assert np.array_equal(words(got.cpu().numpy()), words(want))
        bpts = nr.families(base, seed=6, n=64)["c_off"]
        assert len(nr.same(r2.nearest_points(bpts), nr.expected(base, bpts))) == 0
    finally:
        r1.close()
        r2.close()


# ------------------------------------------------------------------------------------------------------------- 7: past 4 GiB
def test_points_and_results_past_4_gib():
    """16 n bytes of points and 16 n of results with n = 2^28 + 2^20 + 37: byte 2^32 is record 2^28 in both.  A base batch of 4099
    (prime) points on the Cornell box, settled by the model, repeated on the device into a sentinel-filled output: every record
    must be the base's record of the same phase and none may keep the sentinel (tests/large_offsets.py, check_periodic).  Holds
    8.6 GB of records and 1.6 GB of masks and temporaries."""
    import torch
    from tests import large_offsets as LO
    n = 2 ** 28 + 2 ** 20 + 37
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * 16 * n + LO.COMPARE_BYTES + 2 * n:
        pytest.skip("needs %d bytes of device memory, the device has %d free" % (2 * 16 * n + LO.COMPARE_BYTES + 2 * n, free))
    s = LO.scene()
    pts = np.concatenate(list(nr.families(s, seed=8, n=512).values()))
    pts = np.ascontiguousarray(pts[np.random.default_rng(8).permutation(len(pts))][:LO.B_PRIME])
    want = nr.expected(s, pts)
    assert len(pts) == LO.B_PRIME and 0.3 < (want["prim"] >= 0).mean() < 0.95
    r = RendererHIP(0)
    big = out = base_t = None
    try:
        r.set_scene(s)
        base_t = torch.from_numpy(pts).cuda()
        base_out = r.nearest_points(base_t)
        assert len(nr.same(base_out.cpu().numpy(), want)) == 0
        big = base_t.repeat(-(-n // LO.B_PRIME), 1)[:n].contiguous()
        out = torch.full((4 * n,), LO.SENTINEL, dtype=torch.int32, device="cuda")
        d = C.NearestDesc(ctypes.sizeof(C.NearestDesc), 0)
        r._check(r._L.lt_hip_nearest_points_device(r._ctx, ctypes.byref(d), ctypes.c_void_p(big.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                                   16 * n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        rep = LO.check_periodic(out.view(n, 4), base_out.contiguous().view(torch.int32))
        assert rep.ok, str(rep)
    finally:
        del big, out, base_t
        torch.cuda.synchronize()
        r.close()
        torch.cuda.empty_cache()
