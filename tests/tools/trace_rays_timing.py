#!/usr/bin/env python3
"""Ray-query timing (lt_hip_trace_rays_device, lens_trace_amd/csrc/lt_query.hip): HIP-event time per query, closest and any hit,
refill kernel (default) and packet kernel (coherent=True), on
  * the 4K camera rays (3840 x 2160, camera_bytes(0, 2.5, -50), yaw 0) of the 1 M-triangle wall, in 8x8-square order and row-major,
  * 8.3 M random rays through the wall's bounds (origins inside the root box, directions uniform on the sphere),
  * the same on the 1 M-triangle soup.
One JSON line per measurement.  For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python3 <this file>`."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import synth  # noqa: E402
from lens_trace_amd.renderer import RendererHIP, make_rays  # noqa: E402

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))


def camera_rays(W, H, order):
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
    return make_rays(o, d)


def random_rays(s, n, seed=1):
    rng = np.random.default_rng(seed)
    nv = s.node_view
    lo, hi = nv["boundsMin"][0].astype(np.float64), nv["boundsMax"][0].astype(np.float64)
    return make_rays(rng.uniform(lo, hi, (n, 3)), rng.normal(0, 1, (n, 3)))


def time_query(r, rays_t, **kw):
    r.trace_rays(rays_t, **kw)   # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(REPS):
        a.record()
        out = r.trace_rays(rays_t, **kw)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    hits = float((out[:, 1].view(torch.int32) >= 0).float().mean()) if out.dim() == 2 else float(out.float().mean())
    return min(ms), float(np.median(ms)), hits


def main():
    r = RendererHIP(0)
    scenes = [("wall", synth.heightfield_wall()), ("soup", synth.triangle_soup())]
    for name, s in scenes:
        r.set_scene(s)
        batches = [("random 8.3M", random_rays(s, 3840 * 2160))]
        if name == "wall":
            batches = [("camera 4K squares", camera_rays(3840, 2160, "squares")), ("camera 4K rows", camera_rays(3840, 2160, "rows"))] + batches
        for label, rays in batches:
            rt = torch.from_numpy(rays).cuda()
            for any_hit in (False, True):
                for coherent in (False, True):
                    best, med, frac = time_query(r, rt, any_hit=any_hit, coherent=coherent)
                    print(json.dumps({"scene": name, "rays": label, "n": len(rays), "kind": "any" if any_hit else "closest",
                                      "kernel": "packet" if coherent else "refill", "ms_min": round(best, 3), "ms_median": round(med, 3),
                                      "Grays_per_s": round(len(rays) / best / 1e6, 2), "hit_fraction": round(frac, 4)}), flush=True)
            del rt
    r.close()


if __name__ == "__main__":
    main()
