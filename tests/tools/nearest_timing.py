#!/usr/bin/env python3
"""Nearest-point query timing (lt_hip_nearest_points_device, lens_trace_amd/csrc/lt_nearest.hip): HIP-event time per call on the
1 M-triangle wall (synth.heightfield_wall()) for
  * points jittered off the surface (a random point of a random triangle, moved by N(0, LT_TIMING_JITTER = 0.01) per axis),
  * points uniform in the root box,
and, beside them, lt_hip_trace_rays_device closest hit over as many random rays through the same box (the refill kernel).
One JSON line per measurement.  For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python3 <this file>`."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import synth  # noqa: E402
from lens_trace_amd.renderer import RendererHIP, make_points, make_rays  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))
N = int(os.environ.get("LT_TIMING_POINTS", str(1 << 22)))
JITTER = float(os.environ.get("LT_TIMING_JITTER", "0.01"))


def root_box(s):
    nv = s.node_view
    return nv["boundsMin"][0].astype(np.float64), nv["boundsMax"][0].astype(np.float64)


def surface_points(s, n, rng):
    pv = s.prim_view
    p = rng.integers(0, s.n_prims, n)
    b = rng.dirichlet([1, 1, 1], n).astype(np.float32)
    on = pv["positionA"][p] * b[:, 0:1] + pv["positionB"][p] * b[:, 1:2] + pv["positionC"][p] * b[:, 2:3]
    return make_points(on + rng.normal(0, JITTER, (n, 3)))


def time_call(call, arg):
    call(arg)   # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS):
        a.record()
        out = call(arg)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms)), float((out[:, 1].view(torch.int32) >= 0).float().mean())


def main():
    r = RendererHIP(0)
    s = synth.heightfield_wall()
    r.set_scene(s)
    rng = np.random.default_rng(1)
    lo, hi = root_box(s)
    batches = [("nearest", "jittered off the surface", surface_points(s, N, rng)),
               ("nearest", "uniform in the box", make_points(rng.uniform(lo, hi, (N, 3)))),
               ("trace_rays closest", "random rays through the box", make_rays(rng.uniform(lo, hi, (N, 3)), rng.normal(0, 1, (N, 3))))]
    for query, label, records in batches:
        t = torch.from_numpy(records).cuda()
        best, med, frac = time_call(r.nearest_points if query == "nearest" else r.trace_rays, t)
        print(json.dumps({"scene": "wall", "triangles": s.n_prims, "query": query, "records": label, "n": N, "ms_min": round(best, 3),
                          "ms_median": round(med, 3), "M_per_s": round(N / best / 1e3, 1), "hit_fraction": round(frac, 4)}), flush=True)
        del t
    r.close()


if __name__ == "__main__":
    main()
