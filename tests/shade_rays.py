"""Fixtures of the shaded-ray tests (tests/test_shade_rays_cpu.py, tests/test_gpu_shade_rays.py): the cameras, their ray batches
(lens_trace_amd.renderer.reference_camera_rays) and what the CPU oracle says about them.  Computed once per process."""
import functools
import math
import os

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import make_shade_rays, reference_camera_rays
from oracle import pyoracle as po
from tests.conftest import GOLDEN

SIZES = ((32, 16), (37, 29))
# (yaw, distance from the box's centre along the viewing direction): outside the box where that shows both shadow outcomes,
# inside it otherwise.  The yaws' direction-sign octants: 0: 0-3, 0.3 and 1.2: 0, 2; 2.4: 4, 6; -2.4: 5, 7; pi: 4-7.
CAMERAS = ((0.0, 50.0), (0.3, 50.0), (1.2, 50.0), (2.4, 50.0), (-2.4, 2.0), (math.pi, 2.0))
# twelve cameras around (50, 20) and inside (2) the box, 16 x 16 each
RING = tuple((k * math.pi / 6 + 0.1 - (2 * math.pi if k > 6 else 0.0), (50.0, 2.0, 20.0)[k % 3]) for k in range(12))
RING_SIZE = (16, 16)
PROGRAMS = {"basic": po.BASIC, "basic_lighting": po.BASIC_LIGHTING, "accumulator": po.ACCUMULATOR, "custom_opencl": po.CUSTOM}
CENTRE = (0.0, 2.5, 0.0)   # of the Cornell box


@functools.lru_cache(maxsize=None)
def scene(name="cornell_box_O0"):
    return sc.load_ltsb(os.path.join(GOLDEN, name + ".ltsb")).validate()


def scene_of(program):
    return "cornell_box_lens_O0" if program == "basic" else "cornell_box_O0"


def camera(yaw, dist, frame=0):
    """The 28-byte buffer of a camera that looks at the box's centre from `dist` away, turned by yaw."""
    return sc.camera_bytes(float(np.float32(CENTRE[0] - dist * math.sin(yaw))), CENTRE[1], float(np.float32(CENTRE[2] - dist * math.cos(yaw))),
                           float(np.float32(yaw)), 0.0, 0.0, frame)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def camera_batch(yaw, dist, W, H):
    """(n, 8) lt_hip_shade_ray records of the camera's W x H pixels, pixel-major"""
    return frozen(make_shade_rays(*reference_camera_rays(camera(yaw, dist), W, H)))


@functools.lru_cache(maxsize=None)
def oracle_image(name, yaw, dist, W, H, program, mode, frame):
    return frozen(po.render(scene(name), camera(yaw, dist, frame), W, H, PROGRAMS[program], mode))


@functools.lru_cache(maxsize=None)
def oracle_fold(name, yaw, dist, W, H, program, mode, frame_first, frame_count):
    """(W * H, 3): frames frame_first .. frame_first + frame_count - 1 folded by accumulator.frag's running mean from n = 0"""
    acc = np.zeros((H, W, 3), dtype=np.float32)
    for i in range(frame_count):
        po.accumulate(acc, np.ascontiguousarray(oracle_image(name, yaw, dist, W, H, program, mode, frame_first + i)), i)
    return frozen(acc.reshape(-1, 3))


def oracle_hits(name, rays, program=po.ACCUMULATOR):
    """(prim or -1, u, v) of each ray's closest hit by the oracle's lt_oracle_trace (origin.w, direction.w do not matter to it)"""
    s = scene(name)
    prim = np.full(len(rays), -1, dtype=np.int32)
    uv = np.zeros((len(rays), 2), dtype=np.float32)
    for i, r in enumerate(rays):
        hit, p, tuv = po.trace(s, np.append(r[0:3], np.float32(1)), np.append(r[4:7], np.float32(0)), program)
        if hit:
            prim[i] = p
            uv[i] = tuv[1:]
    return prim, uv


def light_prims(name):
    lv = scene(name).light_view[0]
    return lv["primitives"][:int(lv["count"])].astype(np.int64)


@functools.lru_cache(maxsize=None)
def batch_facts(name, yaw, dist, W, H):
    """What the oracle says of a camera's batch: share of rays that hit; of the hits on non-light primitives the shares whose
    accumulator sample of frame 0 is unoccluded (a colour that is not 0 in tile mode) and occluded; share of rays whose hit
    primitive has a lens material (dissolve < 1: basic's lens chain); the direction-sign octants."""
    s = scene(name)
    rays = camera_batch(yaw, dist, W, H)
    prim, _ = oracle_hits(name, rays)
    hit = prim >= 0
    nonlight = hit & ~np.isin(prim, light_prims(name))
    col = oracle_image(name, yaw, dist, W, H, "accumulator", po.MODE_TILE, 0).reshape(-1, 3)
    lit = nonlight & (col != 0).any(axis=1)
    occ = nonlight & ~(col != 0).any(axis=1)
    lens = hit & (s.material_view["dissolve"][s.prim_view["materialIndex"][np.maximum(prim, 0)]] < 1.0)
    d = rays[:, 4:7]
    octants = set(((d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4).tolist())
    return dict(n=len(rays), hit=int(hit.sum()), nonlight=int(nonlight.sum()), lit=int(lit.sum()), occluded=int(occ.sum()), lens=int(lens.sum()),
                octants=octants)


@functools.lru_cache(maxsize=None)
def ring_batch(seed=11):
    """The twelve cameras' rays, concatenated and permuted: (rays, camera of each ray, pixel of each ray)"""
    W, H = RING_SIZE
    rays = np.concatenate([camera_batch(yaw, dist, W, H) for yaw, dist in RING])
    cam = np.repeat(np.arange(len(RING)), W * H)
    pix = np.tile(np.arange(W * H), len(RING))
    perm = np.random.default_rng(seed).permutation(len(rays))
    return frozen(rays[perm]), frozen(cam[perm]), frozen(pix[perm])


def ring_oracle(program, mode, frame_first, frame_count):
    """what the oracle's renders of the twelve cameras give for ring_batch's rays, in its order"""
    W, H = RING_SIZE
    _, cam, pix = ring_batch()
    per = np.stack([oracle_fold(scene_of(program), yaw, dist, W, H, program, mode, frame_first, frame_count) for yaw, dist in RING])
    return per[cam, pix]
