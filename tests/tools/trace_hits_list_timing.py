#!/usr/bin/env python3
"""Hit-list timing (lt_hip_trace_hits_list_device, lens_trace_amd/csrc/lt_query.hip and lt_overlist.hip): HIP-event time per call
on trace_hits_timing.py's batches -- the 4K camera rays of the 1 M-triangle wall in 8x8-square order and row-major,
8.3 M random rays through the wall's bounds, the same on the 1 M-triangle soup -- for the five calls a caller chooses between:
LT_TRACE_COUNT (what the lists' count walk costs, and the baseline), the sizing call (items NULL), the
LT_TRACE_LIST_FLAG_FILL_ONLY call from its offsets, the one-shot call, and LT_TRACE_FIRST_K at K = 8.  A warm-up, then the best of
LT_TIMING_REPS (10).  Every line carries its ratio to the count of the same run.  Run with LT_HIP_LIBRARY naming a build of the
commit before the lists, the tool measures the two calls that build has.  One JSON line per measurement, printed and appended to
profiles/r3/query/trace_hits_list_timing.jsonl (LT_TIMING_OUT; LT_TIMING_RUN labels the run; LT_TIMING_SCENES: wall, soup or
both).  The kernels' own times -- walk, scan, fill walk, order -- come from a kernel trace of this tool with LT_TIMING_REPS=1, in
a run of its own."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import _capi as C  # noqa: E402
from lens_trace_amd import synth  # noqa: E402
from lens_trace_amd.renderer import RendererHIP  # noqa: E402
from tests.tools.trace_rays_timing import camera_rays, random_rays  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))
RUN = os.environ.get("LT_TIMING_RUN", "")
SCENES = os.environ.get("LT_TIMING_SCENES", "wall,soup").split(",")
OUT = os.environ.get("LT_TIMING_OUT", os.path.join(ROOT, "profiles", "r3", "query", "trace_hits_list_timing.jsonl"))
vp = ctypes.c_void_p


def time_call(call):
    call()   # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS):
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


def main():
    r = RendererHIP(0)
    lists = hasattr(r._L, "lt_hip_trace_hits_list_device")
    stream = torch.cuda.current_stream()
    lines = []
    for name, make in (("wall", synth.heightfield_wall), ("soup", synth.triangle_soup)):
        if name not in SCENES:
            continue
        s = make()
        r.set_scene(s)
        batches = [("random 8.3M", random_rays(s, 3840 * 2160))]
        if name == "wall":
            batches = [("camera 4K squares", camera_rays(3840, 2160, "squares")), ("camera 4K rows", camera_rays(3840, 2160, "rows"))] + batches
        for label, rays in batches:
            rt = torch.from_numpy(rays).cuda()
            n = len(rays)
            calls = [("count", lambda: r.trace_hits(rt, count=True))]
            info = {}
            if lists:
                f = r._L.lt_hip_trace_hits_list_device
                offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

                def raw(flags, items):
                    d = C.HitsListDesc(ctypes.sizeof(C.HitsListDesc), C.PROGRAM_ACCUMULATOR, flags, 0)
                    r._check(f(r._ctx, ctypes.byref(d), vp(rt.data_ptr()), n, vp(offsets.data_ptr()), 8 * (n + 1),
                               vp(items.data_ptr()) if items is not None else None, 16 * items.shape[0] if items is not None else 0,
                               vp(stream.cuda_stream)))

                raw(0, None)
                total = int(offsets[-1].item())
                items = torch.zeros((max(total, 1), 4), dtype=torch.float32, device="cuda")[:total]
                lengths = offsets[1:] - offsets[:-1]
                info = {"total": total, "item_bytes": 16 * total, "hits_per_ray": round(total / n, 3), "max_hits": int(lengths.max()),
                        "empty_fraction": round(float((lengths == 0).float().mean()), 4)}
                calls += [("list, sizing call", lambda: raw(0, None)), ("list, FILL_ONLY", lambda: raw(C.TRACE_LIST_FLAG_FILL_ONLY, items)),
                          ("list, one shot", lambda: raw(0, items))]
            calls.append(("first 8", lambda: r.trace_hits(rt, max_hits=8)))
            reference = None
            for query, call in calls:
                best, med = time_call(call)
                reference = best if reference is None else reference
                line = {"scene": name, "triangles": s.n_prims, "rays": label, "n": n, "query": query, "ms_min": round(best, 3),
                        "ms_median": round(med, 3), "ratio_to_count": round(best / reference, 3),
                        "library": "LT_HIP_LIBRARY" if os.environ.get("LT_HIP_LIBRARY") else "this tree", "run": RUN}
                line.update(info)
                print(json.dumps(line), flush=True)
                lines.append(line)
            del rt
    r.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
