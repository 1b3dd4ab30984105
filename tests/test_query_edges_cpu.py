"""CPU tests of tests/query_edges.py: its batches and scenes do what tests/test_gpu_query_edges.py relies on -- every chunk lines up
with a wave of lt_query_packet_kernel and has the verdict it is built to have, all eight octants reach the packet walks of both
kinds, the scaled scenes nest (or, just outside the limits, do not), rays hit, the epsilon bands change answers with the
program -- and the CPU oracle agrees with a float64 brute force on every ray whose answer is robust.  No GPU."""
import numpy as np
import pytest

from lens_trace_amd import _capi as C
from tests import octant_scenes as oc
from tests import query_edges as qe
from tests.test_gpu_trace_rays import Oracle

PROGRAMS = (C.PROGRAM_BASIC, C.PROGRAM_BASIC_LIGHTING, C.PROGRAM_ACCUMULATOR)


@pytest.fixture(scope="module")
def base():
    return qe.base_scene(0)


@pytest.fixture(scope="module")
def fams(base):
    return {b.name: b for b in qe.families(base, 0)}


def test_every_chunk_lines_up_and_qualifies_as_claimed(fams):
    for b in fams.values():
        r = b.rays
        starts = np.cumsum([0] + [len(c) for c in b.chunks])[:-1]
        assert (starts % qe.LANES == 0).all(), b.name
        got = list(zip(qe.chunk_verdicts(r, False), qe.chunk_verdicts(r, True)))
        assert got == b.claims, (b.name, [(i, c, g) for i, (c, g) in enumerate(zip(b.claims, got)) if c != g][:4])
    assert {len(fams["partial%d" % k].rays) % 64 for k in (1, 33, 63)} == {1, 33, 63}
    for k in (1, 33, 63):   # the last chunk would qualify
        assert fams["partial%d" % k].claims[-1][0] is not None


def test_every_octant_reaches_the_packet_walks_of_both_kinds(fams):
    closest = {c for b in fams.values() for c, _ in b.claims if c is not None}
    anyhit = {a for b in fams.values() for _, a in b.claims if a is not None}
    assert closest == set(range(8))
    assert anyhit == set(range(-1, 8))
    for name in ("coherent", "tmax", "ties"):
        assert {c for c, _ in fams[name].claims} == set(range(8)), name


def test_the_intruder_chunks(fams):
    b = fams["intruders"]
    assert len(b.chunks) == len(qe.INTRUDERS) * len(qe.PACKET_SLOTS)
    for i, c in enumerate(b.chunks):
        kind, lane = qe.INTRUDERS[i // len(qe.PACKET_SLOTS)], qe.PACKET_SLOTS[i % len(qe.PACKET_SLOTS)]
        clean = np.delete(c, lane, axis=0)
        # 63 lanes that qualify on their own, one that does not (or, an infinite component, one that stays)
        assert qe.verdict(clean, False) is not None and qe.verdict(clean, True) is not None, (kind, lane)
        if kind not in ("inf_d", "sign", "ignore"):
            assert not qe.own_ok(c[lane:lane + 1])[0], (kind, lane)
    kinds = [qe.INTRUDERS[i // len(qe.PACKET_SLOTS)] for i in range(len(b.chunks))]
    assert {k for k, (c, _) in zip(kinds, b.claims) if c is not None} == {"inf_d"}


def test_the_limit_rays(fams):
    r = fams["limits"].rays
    o, d = np.abs(r[:, 0:3]), np.abs(r[:, 4:7])
    inv = np.abs(qe.inverse(r[:, 4:7]))
    below = np.float32(np.nextafter(np.float32(2.0 ** 40), np.float32(0)))
    assert (o == below).any() and (o == np.float32(2.0 ** 40)).any()
    assert (d == np.nextafter(np.float32(2.0 ** -60), np.float32(np.inf))).any() and (d == np.float32(2.0 ** -60)).any()
    assert (inv[d == np.nextafter(np.float32(2.0 ** -60), np.float32(np.inf))] < 2.0 ** 60).all()
    assert (inv[d == np.float32(2.0 ** -60)] == 2.0 ** 60).all()
    assert (d == np.finfo(np.float32).max).any() and (d >= 2.0 ** 125).sum() >= 64
    sub = inv[(d > 2.0 ** 126) & np.isfinite(d)]
    assert sub.size and (sub < np.finfo(np.float32).tiny).all() and (sub > 0).all()    # subnormal inverses
    assert (inv[np.isinf(d)] == 0).all() and np.isinf(d).any()


def test_rays_hit(base, fams):
    orc = Oracle(base)
    for b in fams.values():
        h, _ = orc.trace(b.rays, C.PROGRAM_ACCUMULATOR)
        assert (h["prim"] >= 0).mean() >= 0.3, b.name
    r = fams["limits"].rays
    h, _ = orc.trace(r, C.PROGRAM_ACCUMULATOR)
    for lim in (np.float32(np.nextafter(np.float32(2.0 ** 40), np.float32(0))), np.float32(2.0 ** 40)):
        at = (np.abs(r[:, 0:3]) == lim).any(axis=1)
        assert (h["prim"][at] >= 0).mean() >= 0.5, lim
    at = (np.abs(r[:, 4:7]) == np.nextafter(np.float32(2.0 ** -60), np.float32(np.inf))).any(axis=1)
    assert (h["prim"][at] >= 0).mean() >= 0.5
    huge = (np.abs(r[:, 4:7]) >= 2.0 ** 99).any(axis=1) & (np.abs(r[:, 4:7]) < 2.0 ** 121).all(axis=1)
    assert (h["prim"][huge] >= 0).mean() >= 0.5


def test_the_epsilon_bands_separate_the_programs(base):
    rng = np.random.default_rng(11)
    r, p = qe.eps_band_rays(base, rng, 900)
    det = np.abs(qe.det_of(base, r, p)).astype(np.float64)
    eps7 = float(qe.EPS_BASIC)
    assert (det < eps7).sum() >= 100 and ((det >= eps7) & (det < 1e-4)).sum() >= 200 and (det >= 1e-4).sum() >= 100
    assert (det == eps7).sum() + (det == float(np.nextafter(qe.EPS_BASIC, np.float32(0)))).sum() >= 1
    # (the reference's double compare against 1e-7 is the float compare against 1e-7f: no float lies in [1e-7, 1e-7f))
    assert float(np.nextafter(qe.EPS_BASIC, np.float32(0))) < 1e-7 <= eps7
    assert float(np.nextafter(qe.EPS4_FLOAT, np.float32(0))) < 1e-4 <= float(qe.EPS4_FLOAT)
    orc = Oracle(base)
    got = {prog: orc.trace(r, prog)[0] for prog in PROGRAMS}
    hb, hl, ha = got[C.PROGRAM_BASIC], got[C.PROGRAM_BASIC_LIGHTING], got[C.PROGRAM_ACCUMULATOR]
    differ = hb["prim"] != ha["prim"]
    assert differ.sum() >= 150
    # where they differ, the rays are the band between the two epsilons: basic hits, accumulator's 1e-4 refuses the triangle
    assert ((det[differ] >= eps7) & (det[differ] < 1e-4)).mean() > 0.9
    assert (hb["prim"][differ] == p[differ]).mean() > 0.75
    # basic and basic_lighting: the same answers on every ray, the two sides of 1e-7f included
    assert np.array_equal(hb.view(np.uint32), hl.view(np.uint32))
    assert (hb["prim"] == p)[det >= eps7].mean() > 0.6 and (hb["prim"] != p)[det < eps7].all()


@pytest.mark.parametrize("name", sorted(qe.EXTREME))
def test_the_extreme_scenes(base, name):
    s, cam, scale, t = qe.extreme_scene(base, name)
    assert s.validate() is s and qe.inside_leaves(s)
    assert qe.nests(s) == qe.EXTREME[name][3]
    nv = s.node_view
    finite = np.isfinite(nv["boundsMin"]).all() and np.isfinite(nv["boundsMax"]).all()
    assert finite == (name != "nan_bound")
    # the triangles keep their area in float32
    P = qe.corners(s)
    area = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    a0 = np.linalg.norm(np.cross(*(qe.corners(base)[:, k] - qe.corners(base)[:, 0] for k in (1, 2))), axis=1)
    ok = a0 > 1e-3
    assert np.allclose(area[ok] / a0[ok], scale ** 2, rtol=0.1)
    # rays mapped onto the scene hit what they hit in the base scene
    rng = np.random.default_rng(3)
    rays = np.concatenate([qe.coherent_chunk(base, k, rng) for k in range(8)])
    want, _ = Oracle(base).trace(rays, C.PROGRAM_ACCUMULATOR)
    got, _ = Oracle(s).trace(qe.scale_rays(rays, scale, t), C.PROGRAM_ACCUMULATOR)
    assert (got["prim"] >= 0).mean() >= 0.6
    if qe.EXTREME[name][3]:
        assert (got["prim"] == want["prim"]).mean() >= 0.8


def test_the_camera_scenes_put_their_cameras_where_they_say(base):
    import struct
    for name, z in (("cam_inside", np.nextafter(np.float32(-2.0 ** 40), np.float32(0))), ("cam_at", np.float32(-2.0 ** 40))):
        s, cam, _, _ = qe.extreme_scene(base, name)
        assert struct.unpack("<6fI", cam)[2] == z
        lo, hi = oc.box_of(s)
        assert lo[2] > -2.0 ** 40 and hi[2] < 2.0 ** 40 and lo[2] > z


def test_the_oracle_agrees_with_float64_on_robust_rays(base, fams):
    rays = np.concatenate([fams[k].rays for k in ("coherent", "tmax", "ignore", "limits")])
    prim, t, robust = qe.brute_force(base, rays)
    assert robust.sum() >= 1000
    h, _ = Oracle(base).trace(rays[robust], C.PROGRAM_ACCUMULATOR)
    assert np.array_equal(h["prim"], prim[robust])
    assert np.allclose(h["t"], t[robust], rtol=1e-5, atol=0)
    # and on scaled scenes, with their own magnitudes
    for name in ("tiny", "large", "far+-+"):
        s, _, scale, sh = qe.extreme_scene(base, name)
        r = qe.scale_rays(fams["coherent"].rays, scale, sh)
        prim, t, robust = qe.brute_force(s, r)
        assert robust.sum() >= 100, name
        h, _ = Oracle(s).trace(r[robust], C.PROGRAM_ACCUMULATOR)
        assert np.array_equal(h["prim"], prim[robust]), name
        assert np.allclose(h["t"], t[robust], rtol=1e-4, atol=0), name
