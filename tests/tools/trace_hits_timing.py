#!/usr/bin/env python3
"""Multi-hit query timing (lt_hip_trace_hits_device, lt_query_hits_kernel in lens_trace_amd/csrc/lt_query.hip): HIP-event time per
query of LT_TRACE_FIRST_K for K = 1, 4, 8 and of LT_TRACE_COUNT, beside the closest-hit query (lt_hip_trace_rays_device, refill
kernel) on the same rays in the same run.  The batches are trace_rays_timing.py's: the 4K camera rays of the
1 M-triangle wall in 8x8-square order and row-major, 8.3 M random rays through the wall's bounds, the same on the 1 M-triangle
soup.  Best of LT_TIMING_REPS (10).  One JSON line per measurement."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import synth  # noqa: E402
from lens_trace_amd.renderer import RendererHIP  # noqa: E402
from tests.tools.trace_rays_timing import camera_rays, random_rays  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))


def time_call(call):
    out = call()   # warm-up
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
    for name, s in (("wall", synth.heightfield_wall()), ("soup", synth.triangle_soup())):
        r.set_scene(s)
        batches = [("random 8.3M", random_rays(s, 3840 * 2160))]
        if name == "wall":
            batches = [("camera 4K squares", camera_rays(3840, 2160, "squares")), ("camera 4K rows", camera_rays(3840, 2160, "rows"))] + batches
        for label, rays in batches:
            rt = torch.from_numpy(rays).cuda()
            base, _, _ = time_call(lambda: r.trace_rays(rt))
            kinds = [("closest", lambda: r.trace_rays(rt))] + [("first %d" % k, lambda k=k: r.trace_hits(rt, max_hits=k)) for k in (1, 4, 8)]
            kinds.append(("count", lambda: r.trace_hits(rt, count=True)))
            for kind, call in kinds:
                best, med, out = time_call(call)
                row = {"scene": name, "rays": label, "n": len(rays), "kind": kind, "ms_min": round(best, 3), "ms_median": round(med, 3),
                       "vs_closest": round(best / base, 2)}
                if kind == "count":
                    row["hits_per_ray"] = round(float(out.float().mean()), 3)
                    row["max_hits"] = int(out.max())
                print(json.dumps(row), flush=True)
                del out
            del rt
    r.close()


if __name__ == "__main__":
    main()
