"""GPU (-m gpu): multi-hit ray queries (lt_hip_trace_hits / lt_hip_trace_hits_device, lt_query_hits_kernel in
lens_trace_amd/csrc/lt_query.hip) against the peeling oracle of tests/multihit.py.

* the portable flavour equals the oracle bit for bit: the first K hits for K = 1, 3, 8 and the count, on the sheets scene (ties,
  negative t, rays of no hit beside rays of a hundred) and the Cornell box, for the three epsilon programs -- every ray, every
  record, the miss records' tmax bits included;
* in every flavour K = 1 is the closest-hit query, the K = 3 records open the K = 8 records, the count agrees with them and with
  the any-hit query;
* a scene without an own tree (every ray takes the walk in the reference's order) and the caller's splits give the same;
* host and device entry points agree at n = 0, 1, 63, 65 and the whole batch, nothing is written behind n records, and
  LT_TRACE_FLAG_COHERENT changes nothing;
* every rejected argument leaves `out` alone; the statistics report the query."""
import ctypes
import os

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import HIT_DTYPE, RendererHIP, make_rays
from tests import multihit as mh
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS_PROGRAMS = (C.PROGRAM_BASIC, C.PROGRAM_BASIC_LIGHTING, C.PROGRAM_ACCUMULATOR)
FLAVOURS = ({}, {"strict_math": True}, {"portable_math": True})
KS = (1, 3, 8)


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


def scene_and_rays(name):
    if name == "sheets":
        return mh.sheets_scene(), mh.sheet_rays()[0]
    return mh.cornell_rays()


def check_against_the_oracle(r, name, s, rays, prog):
    seqs = mh.sequences(name, s, rays, prog)
    want_n = mh.expected_counts(seqs)
    print(name, prog, "rays", len(rays), "hits per ray: max", want_n.max(), "mean %.2f" % want_n.mean())
    for k in KS:
        got = r.trace_hits(rays, max_hits=k, program=prog, portable_math=True)
        assert got.shape == (len(rays), k) and got.dtype == HIT_DTYPE
        bad = mh.same_records(got, mh.expected_records(seqs, rays, k))
        assert len(bad) == 0, (name, prog, k, len(bad), bad[:5], rays[bad[:2]], got[bad[:2]], [seqs[i][:k] for i in bad[:2]])
    n = r.trace_hits(rays, count=True, program=prog, portable_math=True)
    assert n.shape == (len(rays),) and n.dtype == np.uint32
    bad = np.flatnonzero(n != want_n)
    assert len(bad) == 0, (name, prog, len(bad), bad[:5], n[bad[:5]], want_n[bad[:5]])


# ----------------------------------------------------------------------------------------------------------- 1: the oracle
@pytest.mark.parametrize("prog", EPS_PROGRAMS)
@pytest.mark.parametrize("name", ["sheets", "cornell"])
def test_portable_flavour_equals_the_peeling_oracle(renderer, name, prog):
    s, rays = scene_and_rays(name)
    renderer.set_scene(s)
    assert renderer.stats()["own_tree_height"] > 0
    check_against_the_oracle(renderer, name, s, rays, prog)


# ----------------------------------------------------------------------------------------------------------- 2: consistency
@pytest.mark.parametrize("flavour", FLAVOURS, ids=["default", "strict", "portable"])
def test_kinds_agree_with_each_other_and_with_trace_rays(renderer, flavour):
    for name in ("sheets", "cornell"):
        s, rays = scene_and_rays(name)
        renderer.set_scene(s)
        for prog in EPS_PROGRAMS:
            first = renderer.trace_hits(rays, max_hits=1, program=prog, **flavour)
            closest = renderer.trace_rays(rays, program=prog, **flavour)
            assert first.tobytes() == closest.tobytes(), (name, prog)
            k3 = renderer.trace_hits(rays, max_hits=3, program=prog, **flavour)
            k8 = renderer.trace_hits(rays, max_hits=8, program=prog, **flavour)
            assert k3.tobytes() == np.ascontiguousarray(k8[:, :3]).tobytes(), (name, prog)
            n = renderer.trace_hits(rays, count=True, program=prog, **flavour)
            listed = (k8["prim"] >= 0).sum(axis=1)
            assert np.array_equal(n[listed < 8], listed[listed < 8]) and (n[listed == 8] >= 8).all(), (name, prog)
            anyhit = renderer.trace_rays(rays, any_hit=True, program=prog, **flavour)
            assert np.array_equal(anyhit, (n > 0).astype(np.uint32)), (name, prog)
            if name == "sheets":
                assert (n > 8).sum() >= 64 and (n == 0).sum() >= 64


# ----------------------------------------------------------------------------------------------------------- 3: the other walks
def test_the_callers_splits_give_the_same_bytes(renderer, monkeypatch):
    s, rays = scene_and_rays("sheets")
    renderer.set_scene(s)
    want = [renderer.trace_hits(rays, max_hits=k) for k in KS] + [renderer.trace_hits(rays, count=True)]
    monkeypatch.setenv("LT_RETREE", "0")
    r = RendererHIP(0)
    try:
        r.set_scene(s)
        got = [r.trace_hits(rays, max_hits=k) for k in KS] + [r.trace_hits(rays, count=True)]
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
    finally:
        r.close()


def test_a_scene_without_an_own_tree_walks_in_the_references_order(renderer):
    """Leaves that poke out of their ancestors: legal for the reference's traversal, no own tree, so every ray takes the walk over
    the caller's tree -- where equal t keep the order in which the walk meets them."""
    s0, rays = scene_and_rays("sheets")
    s = sc.Scene(s0.nodes.copy(), s0.prims.copy(), s0.materials.copy(), s0.lights.copy(), s0.camera)
    nodes = s.node_view
    leaves = np.flatnonzero(nodes["primitiveCount"] != 0)
    for k in leaves[::7]:
        nodes["boundsMax"][k] += np.float32(0.75)
        nodes["boundsMin"][k] -= np.float32(0.25)
    renderer.set_scene(s.validate())
    assert renderer.stats()["own_tree_height"] == -1
    check_against_the_oracle(renderer, "sheets_poked", s, rays, C.PROGRAM_ACCUMULATOR)


# ----------------------------------------------------------------------------------------------------------- 4: entry points
def test_device_path_equals_host_path(renderer):
    import torch
    s, rays = scene_and_rays("sheets")
    rays = np.array(rays)
    renderer.set_scene(s)
    side = torch.cuda.Stream()
    for n in (0, 1, 63, 65, len(rays)):
        part = rays[:n]
        rt = torch.from_numpy(part).cuda()
        for k in (3, 0):                                                  # 0: the count
            kw = {"count": True} if k == 0 else {"max_hits": k}
            want = renderer.trace_hits(part, **kw)
            assert want.shape == ((n,) if k == 0 else (n, k))
            assert renderer.trace_hits(part, coherent=True, **kw).tobytes() == want.tobytes()
            with torch.cuda.stream(side):
                got = renderer.trace_hits(rt, stream=None, **kw)
                coh = renderer.trace_hits(rt, coherent=True, stream=side, **kw)
            side.synchronize()
            assert got.shape == ((n,) if k == 0 else (n, k, 4))
            assert got.cpu().numpy().tobytes() == want.tobytes() and coh.cpu().numpy().tobytes() == want.tobytes(), (n, k)
            # nothing behind n * max_hits records (n words): a larger buffer full of a sentinel keeps its tail
            words = n if k == 0 else n * k * 4
            buf = torch.full((words + 280,), -7, dtype=torch.int32, device="cuda")
            d = C.MultiHitDesc(ctypes.sizeof(C.MultiHitDesc), C.PROGRAM_ACCUMULATOR, C.TRACE_COUNT if k == 0 else C.TRACE_FIRST_K, 0, k, 0)
            assert renderer._L.lt_hip_trace_hits_device(renderer._ctx, ctypes.byref(d), ctypes.c_void_p(rt.data_ptr() if n else 0), n,
                                                        ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4, None) == 0
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert (host[words:] == -7).all(), (n, k)
            assert host[:words].tobytes() == want.tobytes(), (n, k)


# ----------------------------------------------------------------------------------------------------------- 5: errors
def test_every_error_leaves_the_output_untouched():
    import torch
    r = RendererHIP(0)
    try:
        L = r._L
        rays = make_rays(np.zeros((4, 3)), np.ones((4, 3)))
        out = np.full(4 * 8 * 4, 0x5a5a5a5a, dtype=np.uint32)
        R, O = rays.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

        def desc(program=C.PROGRAM_ACCUMULATOR, kind=C.TRACE_FIRST_K, flags=0, max_hits=2, reserved=0, size=ctypes.sizeof(C.MultiHitDesc)):
            return ctypes.byref(C.MultiHitDesc(size, program, kind, flags, max_hits, reserved))

        assert L.lt_hip_trace_hits(r._ctx, desc(), R, 4, O, out.nbytes) == C.LT_ERR_NO_SCENE
        r.set_scene(sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate())
        bad = C.LT_ERR_INVALID_ARGUMENT
        cases = [
            (None, R, 4, O, out.nbytes, bad),
            (desc(), None, 4, O, out.nbytes, bad),
            (desc(), R, 4, None, out.nbytes, bad),
            (desc(kind=2), R, 4, O, out.nbytes, bad),
            (desc(kind=-1), R, 4, O, out.nbytes, bad),
            (desc(), R, 2 ** 32, O, out.nbytes, bad),
            (desc(flags=C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_PORTABLE_MATH), R, 4, O, out.nbytes, bad),
            (desc(flags=C.RENDER_FLAG_STATS), R, 4, O, out.nbytes, bad),
            (desc(flags=C.RENDER_FLAG_NO_WALK_TIMING), R, 4, O, out.nbytes, bad),
            (desc(flags=0x200), R, 4, O, out.nbytes, bad),
            (desc(size=16), R, 4, O, out.nbytes, bad),
            (desc(size=20), R, 4, O, out.nbytes, bad),
            (desc(program=1000), R, 4, O, out.nbytes, bad),
            (desc(program=6), R, 4, O, out.nbytes, C.LT_ERR_UNKNOWN_PROGRAM),
            (desc(max_hits=0), R, 4, O, out.nbytes, bad),
            (desc(max_hits=C.TRACE_MAX_HITS + 1), R, 4, O, out.nbytes, bad),
            (desc(kind=C.TRACE_COUNT, max_hits=1), R, 4, O, out.nbytes, bad),
            (desc(reserved=1), R, 4, O, out.nbytes, bad),
            (desc(kind=C.TRACE_COUNT, max_hits=0, reserved=1), R, 4, O, out.nbytes, bad),
            (desc(max_hits=2), R, 4, O, 4 * 2 * 16 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(max_hits=8), R, 4, O, 4 * 8 * 16 - 1, C.LT_ERR_BUFFER_TOO_SMALL),
            (desc(kind=C.TRACE_COUNT, max_hits=0), R, 4, O, 15, C.LT_ERR_BUFFER_TOO_SMALL),
        ]
        for i, (d, rp, n, op, nb, want) in enumerate(cases):
            assert L.lt_hip_trace_hits(r._ctx, d, rp, n, op, nb) == want, i
            assert (out == 0x5a5a5a5a).all(), i
        assert L.lt_hip_trace_hits(r._ctx, desc(), R, 0, O, 0) == 0 and (out == 0x5a5a5a5a).all()
        assert L.lt_hip_trace_hits(r._ctx, desc(), None, 0, None, 0) == 0
        # the existing query's kinds are its own: kind 2 is not a way in
        td = C.TraceDesc(ctypes.sizeof(C.TraceDesc), C.PROGRAM_ACCUMULATOR, 2, 0)
        assert L.lt_hip_trace_rays(r._ctx, ctypes.byref(td), R, 4, O, out.nbytes) == bad and (out == 0x5a5a5a5a).all()
        # device entry point: the same checks, and 16-byte alignment
        rt = torch.from_numpy(rays).cuda()
        buf = torch.full((64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        for rp, op in ((rt.data_ptr() + 4, buf.data_ptr()), (rt.data_ptr(), buf.data_ptr() + 8)):
            assert L.lt_hip_trace_hits_device(r._ctx, desc(), ctypes.c_void_p(rp), 3, ctypes.c_void_p(op), 128, None) == bad
        assert L.lt_hip_trace_hits_device(r._ctx, desc(), ctypes.c_void_p(rt.data_ptr()), 4, ctypes.c_void_p(buf.data_ptr()), 127, None) == C.LT_ERR_BUFFER_TOO_SMALL
        assert L.lt_hip_trace_hits_device(r._ctx, desc(reserved=7), ctypes.c_void_p(rt.data_ptr()), 4, ctypes.c_void_p(buf.data_ptr()), 256, None) == bad
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x5a5a5a5a).all()
        with pytest.raises(C.LensTraceError):
            r.trace_hits(rays, program=1000)
        with pytest.raises(ValueError):
            r.trace_hits(rays, max_hits=9)
    finally:
        r.close()


# ----------------------------------------------------------------------------------------------------------- 6: statistics
def test_stats_report_the_query(renderer):
    s, rays = scene_and_rays("cornell")
    renderer.set_scene(s)
    for kw in ({"max_hits": 4}, {"count": True}):
        renderer.trace_hits(rays[:1000], **kw)
        st = renderer.stats()
        assert st["rays"] == 1000 and st["shadow_rays"] == 0 and st["kernel_launches"] >= 1 and st["kernel_ms"] > 0
        assert st["frames"] == 0 and st["pixels"] == 0 and st["render_ms"] == 0
