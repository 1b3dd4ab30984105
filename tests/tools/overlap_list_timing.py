#!/usr/bin/env python3
"""Overlap-list timing (lt_hip_overlap_boxes_list_device, lt_hip_overlap_tris_list_device, lens_trace_amd/csrc/lt_overlist.hip):
HIP-event time per call on the 1 M-triangle wall (synth.heightfield_wall(708)) for
  * the 64^3 cells of a regular grid over the wall's root box (LT_TIMING_GRID = 64), as boxes,
  * 100 k query triangles of edge about LT_TIMING_EDGE (0.05) round points jittered off the surface (LT_TIMING_TRIS),
and for each the four calls a caller chooses between: LT_OVERLAP_COUNT (what the lists' count walk costs, and the baseline: run the
tool with LT_HIP_LIBRARY naming a build of the commit before the lists and it measures that call alone), the sizing call (items
NULL), the LT_OVERLAP_LIST_FLAG_FILL_ONLY call from its offsets, and the one-shot call.  Every line carries its ratio to the
count of the same run.  One JSON line per measurement, printed and written to profiles/r3/query/overlap_list_timing.jsonl
(LT_TIMING_OUT).  The kernels' own times -- the ordering kernel's share -- come from a kernel trace of this tool with
LT_TIMING_REPS=1, in a run of its own."""
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
from lens_trace_amd.renderer import RendererHIP, make_boxes  # noqa: E402
from tests.tools.nearest_timing import root_box, surface_points  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))
GRID = int(os.environ.get("LT_TIMING_GRID", "64"))
TRIS = int(os.environ.get("LT_TIMING_TRIS", "100000"))
EDGE = float(os.environ.get("LT_TIMING_EDGE", "0.05"))
WALL = int(os.environ.get("LT_TIMING_WALL", "708"))
OUT = os.environ.get("LT_TIMING_OUT", os.path.join(ROOT, "profiles", "r3", "query", "overlap_list_timing.jsonl"))
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


def grid_cells(lo, hi, g):
    edges = [np.linspace(lo[a], hi[a], g + 1) for a in range(3)]
    ix = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)
    cell_lo = np.stack([edges[a][ix[:, a]] for a in range(3)], axis=1)
    cell_hi = np.stack([edges[a][ix[:, a] + 1] for a in range(3)], axis=1)
    return make_boxes(cell_lo, cell_hi)


def query_tris(s, n, rng):
    centre = torch.from_numpy(surface_points(s, n, rng)).cuda()[:, 0:3]
    gen = torch.Generator(device="cuda").manual_seed(2)
    tris = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
    for v in range(3):
        tris[:, 4 * v:4 * v + 3] = centre + (torch.rand((n, 3), device="cuda", generator=gen) - 0.5) * EDGE
    return tris


def main():
    r = RendererHIP(0)
    lists = hasattr(r._L, "lt_hip_overlap_boxes_list_device")
    s = synth.heightfield_wall(WALL)
    r.set_scene(s)
    lo, hi = root_box(s)
    batches = [("boxes", "%d^3 cells of the root box" % GRID, torch.from_numpy(grid_cells(lo, hi, GRID)).cuda()),
               ("tris", "edge %g, jittered off the surface" % EDGE, query_tris(s, TRIS, np.random.default_rng(1)))]
    stream = torch.cuda.current_stream()
    lines = []
    for shape, label, rec in batches:
        n = rec.shape[0]
        count_call = (r.overlap_boxes if shape == "boxes" else r.overlap_tris)
        calls = [("count", lambda: count_call(rec, count=True))]
        info = {}
        if lists:
            f = getattr(r._L, "lt_hip_overlap_%s_list_device" % shape)
            size = ctypes.sizeof(C.OverlapListDesc)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

            def raw(flags, items):
                r._check(f(r._ctx, ctypes.byref(C.OverlapListDesc(size, flags)), vp(rec.data_ptr()), n, vp(offsets.data_ptr()), 8 * (n + 1),
                           vp(items.data_ptr()) if items is not None else None, 4 * items.numel() if items is not None else 0,
                           vp(stream.cuda_stream)))

            raw(0, None)
            total = int(offsets[-1].item())
            items = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")[:total]
            lengths = (offsets[1:] - offsets[:-1])
            info = {"total": total, "mean_count": round(total / n, 2), "max_count": int(lengths.max()), "empty_fraction": round(float((lengths == 0).float().mean()), 4)}
            calls += [("list, sizing call", lambda: raw(0, None)), ("list, FILL_ONLY", lambda: raw(C.OVERLAP_LIST_FLAG_FILL_ONLY, items)),
                      ("list, one shot", lambda: raw(0, items))]
        reference = None
        for query, call in calls:
            best, med = time_call(call)
            reference = best if reference is None else reference
            line = {"scene": "wall", "triangles": s.n_prims, "shape": shape, "query": query, "records": label, "n": n, "ms_min": round(best, 3),
                    "ms_median": round(med, 3), "ratio_to_count": round(best / reference, 3), "library": "LT_HIP_LIBRARY" if os.environ.get("LT_HIP_LIBRARY") else "this tree"}
            line.update(info)
            print(json.dumps(line), flush=True)
            lines.append(line)
    r.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
