#!/usr/bin/env python3
"""Triangle-overlap query timing (lt_hip_overlap_tris_device, lens_trace_amd/csrc/lt_tritri.hip): HIP-event time per call on the
1 M-triangle wall (synth.heightfield_wall()) for query triangles of edge about LT_TIMING_EDGE (0.05) centred on nearest_timing.py's
two point batches
  * points jittered off the surface (a random point of a random triangle, moved by N(0, LT_TIMING_JITTER = 0.01) per axis),
  * points uniform in the root box,
for the count, any and the first K = 8 and, in the same run, for lt_hip_overlap_boxes_device's count on the same triangles'
bounding boxes -- the like-for-like neighbour and the broad phase a caller does today: every line carries its ratio to that call.
One JSON line per measurement, printed and written to profiles/r3/query/overlap_tris_timing.jsonl (LT_TIMING_OUT)."""
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
EDGE = float(os.environ.get("LT_TIMING_EDGE", "0.05"))
OUT = os.environ.get("LT_TIMING_OUT", os.path.join(ROOT, "profiles", "r3", "query", "overlap_tris_timing.jsonl"))


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
    lines = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    for label, records in batches:
        centre = torch.from_numpy(records).cuda()[:, 0:3]
        tris = torch.zeros((N, 12), dtype=torch.float32, device="cuda")
        for v in range(3):   # three vertices within EDGE / 2 of the centre per axis: edges of about EDGE
            tris[:, 4 * v:4 * v + 3] = centre + (torch.rand((N, 3), device="cuda", generator=gen) - 0.5) * EDGE
        corners = torch.stack([tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]])
        boxes = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
        boxes[:, 0:3] = corners.min(dim=0).values
        boxes[:, 4:7] = corners.max(dim=0).values
        del corners
        calls = [("overlap_boxes count, the triangles' boxes", lambda: r.overlap_boxes(boxes, count=True)),
                 ("overlap_tris count, edge %g" % EDGE, lambda: r.overlap_tris(tris, count=True)),
                 ("overlap_tris any", lambda: r.overlap_tris(tris, any=True)),
                 ("overlap_tris K=8", lambda: r.overlap_tris(tris, k=8))]
        reference = None
        for query, call in calls:
            best, med, out = time_call(call)
            reference = best if reference is None else reference
            line = {"scene": "wall", "triangles": s.n_prims, "query": query, "records": label, "n": N, "ms_min": round(best, 3),
                    "ms_median": round(med, 3), "M_per_s": round(N / best / 1e3, 1), "ratio_to_overlap_boxes_count": round(best / reference, 3)}
            if out.dim() == 1:
                line["mean_count"] = round(float(out.float().mean()), 2)
                line["max_count"] = int(out.max())
            else:
                line["filled_fraction"] = round(float((out >= 0).float().mean()), 4)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del out
        del centre, tris, boxes
    r.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
