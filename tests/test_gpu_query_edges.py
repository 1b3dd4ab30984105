"""GPU (-m gpu): the ray-query kernels (lens_trace_amd/csrc/lt_query.hip) at their edges, on the fixtures of tests/query_edges.py
(whose claims tests/test_query_edges_cpu.py checks):

* every batch family -- packet-aligned chunks in all eight octants, mixed tmax, ignoring lanes, bit-equal pairs, one intruder lane,
  partial last chunks, rays at packet_ray_ok's limits, epsilon bands -- through both kernels, both kinds and the three epsilon
  programs: the portable flavour bit for bit the oracle, any hit == (closest prim >= 0) in every flavour, and the float64 brute
  force's answer on every robust ray, whatever the flavour;
* scenes at extreme magnitudes (x -> s x + t, s from 2^-40 to 2^35, t up to just inside 2^40): an own tree exactly when every
  bound is below 2^40, the same structures and verdict from host and device preparation, queries equal to the oracle, and renders
  of basic and accumulator equal to the reference's kernels (default, strictMath) and to the oracle (portable), a camera at just
  inside and at 2^40 included."""
import numpy as np
import pytest

from lens_trace_amd.renderer import RendererHIP
from oracle import pyoracle as po
from oracle import ref_gpu
from tests import query_edges as qe
from tests.test_gpu_device_prep import same, structures
from tests.test_gpu_octants import BUILDS, assert_same, hip, need_reference
from tests.test_gpu_trace_rays import EPS_PROGRAMS, FLAVOURS, check_scene

pytestmark = pytest.mark.gpu
BASE = qe.base_scene(0)
FAMILIES = {b.name: b for b in qe.families(BASE, 0)}
SCALED_FAMILIES = ("coherent", "tmax", "ignore", "intruders", "partial33")


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no calibration launches (as tests/test_gpu_octants.py)


def check_robust(r, s, rays):
    """The GPU's own closest hits, every flavour and both kernels, on the rays whose answer float64 settles."""
    prim, t, robust = qe.brute_force(s, rays)
    assert robust.sum() >= 20
    for prog in EPS_PROGRAMS:
        for coherent in (False, True):
            for fl in FLAVOURS:
                h = r.trace_rays(rays[robust], program=prog, coherent=coherent, **fl)
                assert np.array_equal(h["prim"], prim[robust]), (prog, coherent, fl)
                assert np.allclose(h["t"], t[robust], rtol=1e-4, atol=0), (prog, coherent, fl)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_families_against_the_oracle(renderer, family):
    rays = FAMILIES[family].rays
    check_scene(renderer, BASE, rays)
    assert renderer.stats()["own_tree_height"] > 0
    if family not in ("eps", "ties"):
        check_robust(renderer, BASE, rays)


def test_the_epsilon_bands_tell_the_programs_apart(renderer):
    """On the epsilon-band rays the kernels' own answers differ between basic and accumulator (basic_lighting's double compare
    against 1e-7 is basic's float compare against 1e-7f: no float lies between the two, so those two always agree)."""
    rays = FAMILIES["eps"].rays
    renderer.set_scene(BASE)
    for coherent in (False, True):
        for fl in FLAVOURS:
            got = {p: renderer.trace_rays(rays, program=p, coherent=coherent, **fl) for p in EPS_PROGRAMS}
            b, l, a = (got[p]["prim"] for p in EPS_PROGRAMS)
            assert (b != a).sum() >= 50, (coherent, fl)
            assert np.array_equal(b, l), (coherent, fl)


# ------------------------------------------------------------------------------------------------------- extreme magnitudes
_extreme = {}


def extreme(name):
    if name not in _extreme:
        _extreme[name] = qe.extreme_scene(BASE, name)
    return _extreme[name]


@pytest.mark.parametrize("name", sorted(qe.EXTREME))
def test_extreme_scene_queries(renderer, name):
    s, _, scale, t = extreme(name)
    rays = np.concatenate([qe.scale_rays(FAMILIES[f].rays, scale, t) for f in SCALED_FAMILIES])
    check_scene(renderer, s, rays, flavours_any=name in ("tiny", "far+-+", "nan_bound"))
    h = renderer.stats()["own_tree_height"]
    assert (h > 0) if qe.EXTREME[name][3] else (h == -1), (name, h)
    assert (renderer.trace_rays(rays, portable_math=True)["prim"] >= 0).mean() >= 0.3


@pytest.mark.parametrize("name", sorted(qe.EXTREME))
def test_extreme_scene_preparation_host_equals_device(monkeypatch, name):
    s = extreme(name)[0]
    if qe.EXTREME[name][3]:
        dev = same(monkeypatch, s)
        assert dev[3][0] > 0
    else:       # the refusal verdict: no own tree from either path
        host = structures(monkeypatch, s, False)
        dev = structures(monkeypatch, s, True)
        assert host[0] is None and dev[0] is None, name
        assert host[3][:3] == dev[3][:3] and host[3][0] <= 0, (host[3], dev[3])
        assert (host[1] is None) == (dev[1] is None) and (host[1] is None or np.array_equal(host[1], dev[1]))


RENDERED = ("large", "far+", "far-", "far+-+", "cam_inside", "cam_at", "bound_at_limit", "nan_bound")


@pytest.mark.parametrize("against", ["reference", "oracle"])
@pytest.mark.parametrize("name", RENDERED)
def test_extreme_scene_renders(renderer, name, against):
    if against == "reference":
        need_reference()
    s, cam, _, _ = extreme(name)
    for prog, W, H in (("basic", 37, 29), ("accumulator", 21, 13)):
        for build in (BUILDS if against == "reference" else ("portable",)):
            got = hip(renderer, s, prog, W, H, cam, 0, build)
            assert (renderer.stats()["own_tree_height"] > 0) == qe.EXTREME[name][3]
            want = ref_gpu.render(s, cam, W, H, prog, build, 0) if against == "reference" else po.render(s, cam, W, H, po.PROGRAMS[prog])
            assert_same(got, want, "%s %s %dx%d %s vs %s" % (name, prog, W, H, build, against))
        if prog == "basic":     # something in view
            assert np.isfinite(got).all() and (np.abs(got - got[0, 0]).max() > 0), name
