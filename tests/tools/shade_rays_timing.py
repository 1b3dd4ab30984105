#!/usr/bin/env python3
"""Shaded-ray timing (lt_hip_shade_rays_device, lens_trace_amd/csrc/lt_shade.hip): HIP-event time per call, best of LT_TIMING_REPS
(10) after a warm-up, accumulator with 1 and 16 frames, on
  * the 4K camera rays (3840 x 2160, camera_bytes(0, 2.5, -50), yaw 0) of the 1 M-triangle wall, in 8x8-square order and row-major,
  * 8.3 M random rays through the wall's bounds (origins inside the root box, directions uniform on the sphere; film positions
    uniform in the film square),
  * the same on the 1 M-triangle soup,
and beside each, measured in the same run, what a caller composes today without the shading -- trace_rays closest hit plus
trace_rays any hit over the same rays (the refill kernels) -- and, for the camera rays, `render` of the same frames (the packet
path, which a ray batch cannot match).  One JSON line per measurement.  For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python3 <this file>`."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import _capi as C  # noqa: E402
from lens_trace_amd import scene as sc  # noqa: E402
from lens_trace_amd import synth  # noqa: E402
from lens_trace_amd.renderer import RendererHIP, make_desc, make_rays, make_shade_rays  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))
W, H = 3840, 2160
CAM = sc.camera_bytes(0.0, 2.5, -50.0, 0.0)
FRAMES = (1, 16)


def camera_rays(order):
    f32 = np.float32
    ys, xs = np.mgrid[0:H, 0:W]
    if order == "squares":
        ys = ys.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
        xs = xs.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    fx = xs.astype(f32) / f32(W) - f32(0.5)
    fy = ys.astype(f32) / f32(H) - f32(0.5)
    o = np.stack([f32(0.0) + fx, f32(2.5) + fy, np.full_like(fx, f32(-50.0))], axis=-1)
    d = np.stack([f32(0.0) - fx, f32(0.0) - fy, np.full_like(fx, f32(5.0))], axis=-1)
    return make_shade_rays(o, d, fx, fy)


def random_rays(s, n, seed=1):
    rng = np.random.default_rng(seed)
    nv = s.node_view
    lo, hi = nv["boundsMin"][0].astype(np.float64), nv["boundsMax"][0].astype(np.float64)
    return make_shade_rays(rng.uniform(lo, hi, (n, 3)), rng.normal(0, 1, (n, 3)), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n))


def best_of(call):
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
    return round(min(ms), 3), round(float(np.median(ms)), 3)


def main():
    r = RendererHIP(0)
    image = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    for name, s in (("wall", synth.heightfield_wall()), ("soup", synth.triangle_soup())):
        r.set_scene(s)
        batches = [("random 8.3M", random_rays(s, W * H))]
        if name == "wall":
            batches = [("camera 4K squares", camera_rays("squares")), ("camera 4K rows", camera_rays("rows"))] + batches
        for label, rays in batches:
            n = len(rays)
            rt = torch.from_numpy(rays).cuda()
            qt = torch.from_numpy(make_rays(rays[:, 0:3], rays[:, 4:7])).cuda()
            closest = best_of(lambda: r.trace_rays(qt, program=C.PROGRAM_ACCUMULATOR))
            any_hit = best_of(lambda: r.trace_rays(qt, program=C.PROGRAM_ACCUMULATOR, any_hit=True))
            out = r.shade_rays(rt)
            torch.cuda.synchronize()
            hits = float((out[:, 3].view(torch.int32) >= 0).float().mean())
            for frames in FRAMES:
                row = {"scene": name, "rays": label, "n": n, "frames": frames, "hit_fraction": round(hits, 4)}
                row["shade_ms_min"], row["shade_ms_median"] = best_of(lambda: r.shade_rays(rt, program=C.PROGRAM_ACCUMULATOR, frame_count=frames))
                row["Mrays_per_s"] = round(n / row["shade_ms_min"] / 1e3, 1)
                row["trace_closest_ms_min"], row["trace_any_ms_min"] = closest[0], any_hit[0]
                row["composed_ms"] = round(closest[0] + frames * any_hit[0], 3)   # one camera walk and one shadow walk per frame, no shading
                if label.startswith("camera"):
                    d = make_desc(C.PROGRAM_ACCUMULATOR, W, H, 3, CAM, frame_first=0, frame_count=frames, accumulate=True)
                    row["render_ms_min"], row["render_ms_median"] = best_of(lambda: r.render_device(d, image.data_ptr(), image.numel() * 4))
                print(json.dumps(row), flush=True)
            del rt, qt
    r.close()


if __name__ == "__main__":
    main()
