"""CPU tests of tests/octant_scenes.py: the scenes and cameras of tests/test_gpu_octants.py have the direction-sign octants they
claim, so that the GPU tests there drive every packet-walk instance (lt_walk_asm.hpp: one per octant and walk family)."""
import math

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import octant_scenes as oc

YAWS = (0.0, math.pi, 1.2, -2.4)                 # the GPU tests' yaws
SIZES = ((37, 29), (64, 48), (5, 3))             # ... and image sizes


@pytest.mark.parametrize("octant", range(8))
def test_every_shadow_ray_has_the_octants_signs(octant):
    P, _, _, _, light = oc.octant_triangles(octant, seed=octant)
    assert light.sum() >= 2 and not light[0]
    rng = np.random.default_rng(octant)

    def points(tris, k):     # k random points on each triangle, in float32 as the kernels interpolate them
        uv = rng.uniform(0, 1, (k, 2))
        uv = np.where(uv.sum(axis=1, keepdims=True) > 1, 1 - uv, uv).astype(np.float32)
        w = np.concatenate([1 - uv.sum(axis=1, keepdims=True), uv], axis=1).astype(np.float32)
        return np.einsum("kj,njc->nkc", w, tris).reshape(-1, 3).astype(np.float32)

    geo = points(P[~light], 16)
    lit = points(P[light], 64)
    lit = np.concatenate([lit, P[light].reshape(-1, 3)])                  # the corners too
    lo, hi = oc.light_box(octant)
    assert (lit >= lo - 1e-6).all() and (lit <= hi + 1e-6).all()
    assert (np.abs(geo) <= oc.BOX).all()
    d = lit[None, :, :] - geo[:, None, :]
    assert (oc.octant_of(d) == octant).all()
    assert np.abs(d).min() >= oc.MARGIN - 1e-3 and oc.MARGIN >= 5.0      # far above any rounding


def camera_union(sizes=SIZES, yaws=YAWS):
    got = set()
    for yaw in yaws:
        for W, H in sizes:
            got |= oc.camera_octants(oc.camera_for(yaw), W, H)
    return got


def test_the_cameras_cover_every_octant():
    assert camera_union() == set(range(8))
    for yaw, want in ((0.0, {0, 1, 2, 3}), (math.pi, {4, 5, 6, 7}), (1.2, {0, 2}), (-2.4, {5, 7})):
        assert oc.camera_octants(oc.camera_for(yaw), 64, 48) == want, yaw


@pytest.mark.parametrize("yaw", YAWS + (-1.2, 2.4, 0.7))
@pytest.mark.parametrize("W,H", SIZES + ((96, 64), (8, 8), (1, 1)))
def test_camera_octants_agree_with_double_precision(yaw, W, H):
    cam = oc.camera_for(yaw)
    d32, d64 = oc.camera_directions(cam, W, H), oc.camera_directions(cam, W, H, np.float64)
    assert np.abs(d32 - d64).max() < 1e-5                                 # far below the margin
    assert oc.camera_octants(cam, W, H) == oc.camera_octants(cam, W, H, dtype=np.float64)
    # every square counted has one octant in double precision, clear of 0
    for ys, xs in oc.square_lanes(W, H):
        q = d64[ys, xs].reshape(-1, 3)
        o = oc.octant_of(q)
        if (np.abs(q) > 1e-4).all() and (o == o[0]).all():
            assert int(o[0]) in oc.camera_octants(cam, W, H)


def test_square_lanes_cover_the_image_once():
    for W, H, tile in ((37, 29, None), (5, 3, None), (64, 48, None), (50, 30, (20, 12))):
        hit = np.zeros((H, W), int)
        for ys, xs in oc.square_lanes(W, H, tile):
            assert ys.size <= 64
            hit[ys, xs] += 1
        assert (hit == 1).all()


def hit_fraction(scene, cam, W=32, H=24):
    """Share of the pixels whose camera ray hits a triangle: custom_opencl's colour is (u, v, 1 - u - v), summing to 1 on a hit."""
    img = po.render(scene, cam, W, H, po.CUSTOM)
    return float((np.abs(img.sum(axis=2) - 1.0) < 1e-3).mean())


@pytest.mark.parametrize("octant", range(8))
def test_the_scene_is_in_view(octant):
    s = oc.octant_scene(octant, seed=octant)
    for yaw in YAWS:
        assert hit_fraction(s, oc.camera_for(yaw)) >= 0.25, yaw
