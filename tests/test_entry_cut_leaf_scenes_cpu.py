"""CPU tests of the constructions in tests/entry_cut_leaf_scenes.py, with the oracle: that the scenes show what the GPU tests of the
entry cuts' leaf pass (tests/test_gpu_entry_cut_leaves.py) rely on."""
import numpy as np

from lens_trace_amd import scene as sc
from oracle import pyoracle as po
from tests import entry_cut_leaf_scenes as ls
from tests import mixed_axis_scenes as mx

W, H = 24, 16


def lit(name, frame=1):
    s, cam = ls.scene(name)
    return po.render(s, sc.camera_with_frame(cam, frame), W, H, po.ACCUMULATOR).max(axis=2) > 0.0


def forward_hits(s, o, w, own, emissive):
    """Does the segment from o to o + w (float64) meet a triangle that is neither `own` nor a light, at 1e-9 < t < 1?"""
    pv = s.prim_view
    for i in range(len(pv)):
        if i == own or i in emissive:
            continue
        a, b, c = (np.float64(pv[i][k]) for k in ("positionA", "positionB", "positionC"))
        e1, e2 = b - a, c - a
        p = np.cross(w, e2)
        det = e1 @ p
        if abs(det) < 1e-12:
            continue
        t_ = o - a
        u = (t_ @ p) / det
        q = np.cross(t_, e1)
        v = (w @ q) / det
        t = (e2 @ q) / det
        if u >= 0 and v >= 0 and u + v <= 1 and 1e-9 < t < 1:
            return True
    return False


def test_ridge_has_pixels_that_only_a_negative_t_darkens():
    """Pixels that face the light (n . l > 0), have nothing between them and their light sample, and are dark in the oracle."""
    s, cam = ls.scene("ridge")
    hits = mx.camera_hits(s, cam, W, H)
    has, pos, _, prims = hits
    d = mx.shadow_directions(s, hits, 1)
    lv = s.light_view[0]
    emissive = set(int(p) for p in lv["primitives"][:int(lv["count"])])
    dark = ~lit("ridge") & has
    found = 0
    for y, x in zip(*np.nonzero(dark)):
        n = np.float64(s.prim_view[int(prims[y, x])]["normalA"])
        if n @ d[y, x] > 0 and not forward_hits(s, np.float64(pos[y, x]), d[y, x], int(prims[y, x]), emissive):
            found += 1
    print("ridge %dx%d frame 1: %d dark casting pixels, %d of them facing the light with a free way to it" % (W, H, int(dark.sum()), found))
    assert found >= 2


def test_flat_grid_hits_lie_on_vertices_and_edges():
    s, cam = ls.scene("flat-grid")
    on_edge = 0
    for y in range(H):
        for x in range(W):
            f = np.float32
            o = np.array([f(x) / f(W) - f(0.5), f(2.5) + f(y) / f(H) - f(0.5), f(-50.0), 1], f)
            dd = np.array([-(f(x) / f(W) - f(0.5)), -(f(y) / f(H) - f(0.5)), 5.0, 0], f)
            hit, prim, tuv = po.trace(s, o, dd)
            if hit and (tuv[1] == 0 or tuv[2] == 0 or tuv[1] + tuv[2] == 1):
                on_edge += 1
    print("flat-grid %dx%d: %d of %d camera hits on an edge or a vertex" % (W, H, on_edge, W * H))
    assert on_edge > W * H // 4


def test_far_occluder_shades_a_few_pixels_in_some_frames_only():
    a, b = lit("far-occluder", 1), lit("far-occluder", 2)
    s, cam = ls.scene("far-occluder")
    has = mx.camera_hits(s, cam, W, H)[0]
    dark = [int((~m & has).sum()) for m in (a, b)]
    print("far-occluder %dx%d: dark casting pixels in frames 1, 2: %r; different in %d" % (W, H, dark, int(((a != b) & has).sum())))
    assert 0 < max(dark) < has.sum() // 8
    assert ((a != b) & has).any()
