#!/usr/bin/env python3
"""Box-overlap query timing (lt_hip_overlap_boxes_device, lens_trace_amd/csrc/lt_overlap.hip): HIP-event time per call on the
1 M-triangle wall (synth.heightfield_wall()) for cubes of half-width LT_TIMING_RADIUS (0.025) centred on nearest_timing.py's two
point batches
  * points jittered off the surface (a random point of a random triangle, moved by N(0, LT_TIMING_JITTER = 0.01) per axis),
  * points uniform in the root box,
for the count, any and the first K = 8 and, in the same run on the same centres, for lt_hip_nearest_k_device's count within that
radius -- the like-for-like neighbour (the sphere inscribed in the cube): every line carries its ratio to that call.
One JSON line per measurement.  For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python3 <this file>`."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import synth  # noqa: E402
from lens_trace_amd.renderer import RendererHIP, make_points  # noqa: E402
from tests.tools.nearest_timing import root_box, surface_points  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))
N = int(os.environ.get("LT_TIMING_POINTS", str(1 << 22)))
RADIUS = float(os.environ.get("LT_TIMING_RADIUS", "0.025"))


def time_call(call):
    call()   # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS):
        a.record()
        out = call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms)), out


def main():
    r = RendererHIP(0)
    s = synth.heightfield_wall()
    r.set_scene(s)
    rng = np.random.default_rng(1)
    lo, hi = root_box(s)
    batches = [("jittered off the surface", surface_points(s, N, rng)), ("uniform in the box", make_points(rng.uniform(lo, hi, (N, 3))))]
    for label, records in batches:
        within = torch.from_numpy(records).cuda()
        within[:, 3] = RADIUS * RADIUS
        boxes = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
        boxes[:, 0:3] = within[:, 0:3] - RADIUS
        boxes[:, 4:7] = within[:, 0:3] + RADIUS
        calls = [("nearest_k count, radius %g" % RADIUS, lambda: r.nearest_k(within, count=True)),
                 ("overlap_boxes count, half-width %g" % RADIUS, lambda: r.overlap_boxes(boxes, count=True)),
                 ("overlap_boxes any", lambda: r.overlap_boxes(boxes, any=True)),
                 ("overlap_boxes K=8", lambda: r.overlap_boxes(boxes, k=8))]
        reference = None
        for query, call in calls:
            best, med, out = time_call(call)
            reference = best if reference is None else reference
            line = {"scene": "wall", "triangles": s.n_prims, "query": query, "records": label, "n": N, "ms_min": round(best, 3),
                    "ms_median": round(med, 3), "M_per_s": round(N / best / 1e3, 1), "ratio_to_nearest_k_count": round(best / reference, 3)}
            if out.dim() == 1:
                line["mean_count"] = round(float(out.float().mean()), 2)
                line["max_count"] = int(out.max())
            else:
                line["filled_fraction"] = round(float((out >= 0).float().mean()), 4)
            print(json.dumps(line), flush=True)
            del out
        del within, boxes
    r.close()


if __name__ == "__main__":
    main()
