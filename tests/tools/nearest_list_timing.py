#!/usr/bin/env python3
"""Radius-list timing (lt_hip_nearest_list_device, lens_trace_amd/csrc/lt_nearest.hip and lt_overlist.hip): HIP-event time per
call on the 1 M-triangle wall (synth.heightfield_wall(708)) for nearest_k_timing.py's near-surface batch -- LT_TIMING_POINTS
(2^22) points jittered off the surface, every max_d2 the square of LT_TIMING_RADIUS (0.025) -- and the four calls a caller chooses
between: LT_NEAREST_COUNT (what the lists' count walk costs, and the baseline: run the tool with LT_HIP_LIBRARY naming a build of
the commit before the lists and it measures that call alone), the sizing call (items NULL), the LT_NEAREST_LIST_FLAG_FILL_ONLY
call from its offsets, and the one-shot call.  Every line carries its ratio to the count of the same run.  One JSON line per
measurement, printed and appended to profiles/r3/query/nearest_list_timing.jsonl (LT_TIMING_OUT; LT_TIMING_RUN labels the run).
The kernels' own times -- the ordering kernel's share -- come from a kernel trace of this tool with LT_TIMING_REPS=1, in a run
of its own."""
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
from tests.tools.nearest_timing import surface_points  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))
N = int(os.environ.get("LT_TIMING_POINTS", str(1 << 22)))
RADIUS = float(os.environ.get("LT_TIMING_RADIUS", "0.025"))
WALL = int(os.environ.get("LT_TIMING_WALL", "708"))
RUN = os.environ.get("LT_TIMING_RUN", "")
OUT = os.environ.get("LT_TIMING_OUT", os.path.join(ROOT, "profiles", "r3", "query", "nearest_list_timing.jsonl"))
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
    lists = hasattr(r._L, "lt_hip_nearest_list_device")
    s = synth.heightfield_wall(WALL)
    r.set_scene(s)
    pts = torch.from_numpy(surface_points(s, N, np.random.default_rng(1))).cuda()
    pts[:, 3] = RADIUS * RADIUS
    stream = torch.cuda.current_stream()
    calls = [("count", lambda: r.nearest_k(pts, count=True))]
    info = {}
    if lists:
        f = r._L.lt_hip_nearest_list_device
        size = ctypes.sizeof(C.NearestListDesc)
        offsets = torch.zeros(N + 1, dtype=torch.int64, device="cuda")

        def raw(flags, items):
            r._check(f(r._ctx, ctypes.byref(C.NearestListDesc(size, flags)), vp(pts.data_ptr()), N, vp(offsets.data_ptr()), 8 * (N + 1),
                       vp(items.data_ptr()) if items is not None else None, 16 * items.shape[0] if items is not None else 0,
                       vp(stream.cuda_stream)))

        raw(0, None)
        total = int(offsets[-1].item())
        items = torch.zeros((max(total, 1), 4), dtype=torch.float32, device="cuda")[:total]
        lengths = offsets[1:] - offsets[:-1]
        info = {"total": total, "item_bytes": 16 * total, "mean_count": round(total / N, 2), "max_count": int(lengths.max()),
                "empty_fraction": round(float((lengths == 0).float().mean()), 4)}
        calls += [("list, sizing call", lambda: raw(0, None)), ("list, FILL_ONLY", lambda: raw(C.NEAREST_LIST_FLAG_FILL_ONLY, items)),
                  ("list, one shot", lambda: raw(0, items))]
    reference = None
    lines = []
    for query, call in calls:
        best, med = time_call(call)
        reference = best if reference is None else reference
        line = {"scene": "wall", "triangles": s.n_prims, "query": query, "records": "jittered off the surface, radius %g" % RADIUS, "n": N,
                "ms_min": round(best, 3), "ms_median": round(med, 3), "ratio_to_count": round(best / reference, 3),
                "library": "LT_HIP_LIBRARY" if os.environ.get("LT_HIP_LIBRARY") else "this tree", "run": RUN}
        line.update(info)
        print(json.dumps(line), flush=True)
        lines.append(line)
    r.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
