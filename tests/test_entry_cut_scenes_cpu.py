"""CPU test of the wide-light scene of tests/entry_cut_scenes.py (tests/test_gpu_entry_cut.py renders it): its occluder stops shadow rays of the frames the GPU test renders,
and every ray it stops aims at the light's outer quarter, beyond x = 10 -- outside a light box half as wide.  So an entry cut made
for too small a light box, which drops the occluder, changes pixels of that test."""
import numpy as np

from oracle import pyoracle as po
from tests import mixed_axis_scenes as mx
from tests import entry_cut_scenes as t


def test_the_occluder_hides_only_the_lights_outer_quarter():
    s, cam = t.scene("wide-light")
    occluder = [i for i in range(s.n_prims) if int(s.prim_view[i]["materialIndex"]) == 1]
    assert len(occluder) == 1
    W, H = t.SIZES[0]
    hits = mx.camera_hits(s, cam, W, H)
    has, pos, _, prims = hits
    stopped = []
    for frame in (1, 2):
        d = mx.shadow_directions(s, hits, frame)
        for y, x in zip(*np.nonzero(has)):
            length = np.linalg.norm(d[y, x])
            hit, prim, _ = po.trace(s, np.append(pos[y, x], 1).astype(np.float32), np.append(d[y, x] / length, 0).astype(np.float32),
                                    tmax=np.float32(length - 0.01), ignore=int(prims[y, x]))
            if hit and prim == occluder[0]:
                stopped.append(float(pos[y, x][0] + d[y, x][0]))
    assert len(stopped) >= 3, stopped
    assert min(stopped) > 10.0 + 1.0, stopped
