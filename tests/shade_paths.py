"""Fixtures of the shaded-path tests (tests/test_shade_paths_cpu.py, tests/test_gpu_shade_paths.py): the CPU oracle's renders of the
two global-illumination programs for the cameras of tests/shade_rays.py, folded by the running mean, and what the oracle says about
the paths of those cameras' rays.  Computed once per process."""
import functools

import numpy as np

from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from oracle import pyoracle as po
from tests import shade_rays as F

PROGRAMS = {"global_illumination": po.GI, "global_illumination25": po.GI25}
DEPTHS = (1, 4, 0)     # gi_max_depth: 0 = the reference's 16
SYNTH_SIZE = (64, 48)
SCENE = "cornell_box_O0"


def depth_of(gi_max_depth):
    return gi_max_depth if gi_max_depth else 16


@functools.lru_cache(maxsize=None)
def oracle_image(yaw, dist, W, H, program, mode, frame, gi_max_depth):
    return F.frozen(po.render(F.scene(SCENE), F.camera(yaw, dist, frame), W, H, PROGRAMS[program], mode, gi_max_depth=depth_of(gi_max_depth)))


@functools.lru_cache(maxsize=None)
def oracle_fold(yaw, dist, W, H, program, mode, frame_first, frame_count, gi_max_depth):
    """(W * H, 3): frames frame_first .. frame_first + frame_count - 1 folded by accumulator.frag's running mean from n = 0"""
    acc = np.zeros((H, W, 3), dtype=np.float32)
    for i in range(frame_count):
        po.accumulate(acc, np.ascontiguousarray(oracle_image(yaw, dist, W, H, program, mode, frame_first + i, gi_max_depth)), i)
    return F.frozen(acc.reshape(-1, 3))


def ring_oracle(program, mode, frame_first, frame_count, gi_max_depth):
    """what the oracle's renders of the twelve cameras give for ring_batch's rays, in its order"""
    W, H = F.RING_SIZE
    _, cam, pix = F.ring_batch()
    per = np.stack([oracle_fold(yaw, dist, W, H, program, mode, frame_first, frame_count, gi_max_depth) for yaw, dist in F.RING])
    return per[cam, pix]


@functools.lru_cache(maxsize=None)
def extension_rays(yaw, dist, W, H):
    """(W * H,): extension rays the single-sample program traces for each pixel of frame 0 at 16 bounces: rays - shadow rays - 1"""
    c = po.pixel_counters(F.scene(SCENE), F.camera(yaw, dist), W, H, po.GI).reshape(-1, 4).astype(np.int64)
    return F.frozen(c[:, 0] - c[:, 1] - 1)


@functools.lru_cache(maxsize=None)
def synth_scene(kind):
    s = {"wall": lambda: synth.heightfield_wall(48), "soup": lambda: synth.triangle_soup(3000), "blob": lambda: synth.blob_in_box(3)}[kind]()
    return s.validate()


@functools.lru_cache(maxsize=None)
def synth_oracle(kind, program, mode, frame_first, frame_count, gi_max_depth):
    """the oracle's render of a synthetic scene from its own camera at SYNTH_SIZE, folded; (W * H, 3)"""
    W, H = SYNTH_SIZE
    s = synth_scene(kind)
    acc = np.zeros((H, W, 3), dtype=np.float32)
    for i in range(frame_count):
        cam = sc.camera_with_frame(s.camera, frame_first + i)
        po.accumulate(acc, np.ascontiguousarray(po.render(s, cam, W, H, PROGRAMS[program], mode, gi_max_depth=depth_of(gi_max_depth), threads=8)), i)
    return F.frozen(acc.reshape(-1, 3))
