#!/usr/bin/env python3
"""Surface-query timing (lt_hip_trace_surface_device, lt_hip_surface_at_device, lens_trace_amd/csrc/lt_query.hip): HIP-event time,
best of LT_TIMING_REPS (10) after a warm-up, the variants alternating inside one process, on
  * the 4K camera rays (3840 x 2160, camera_bytes(0, 2.5, -50), yaw 0) of the 1 M-triangle wall, row-major and in 8x8 squares,
    refill kernel and packet kernel (coherent=True),
  * 8.3 M random rays through the wall's bounds, and through the 1 M-triangle soup's.
Per row: trace_surface, trace_rays on the same rays, the composed pair trace_rays + surface_at as a caller would enqueue it, and
surface_at alone with its achieved bytes/s (n x 64 bytes of records plus 76 gathered bytes per hit).  trace_surface and the
composed pair are each in the rotation twice: the difference of the two copies' results is the run-to-run spread.
One JSON line per row."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import synth  # noqa: E402
from lens_trace_amd.renderer import RendererHIP  # noqa: E402
from trace_rays_timing import camera_rays, random_rays  # noqa: E402  (this directory: the script's own)

REPS = int(os.environ.get("LT_TIMING_REPS", "10"))


def main():
    r = RendererHIP(0)
    for name, s in (("wall", synth.heightfield_wall()), ("soup", synth.triangle_soup())):
        r.set_scene(s)
        rows = [("random 8.3M", random_rays(s, 3840 * 2160), False)]
        if name == "wall":
            cams = [("camera 4K rows", camera_rays(3840, 2160, "rows")), ("camera 4K squares", camera_rays(3840, 2160, "squares"))]
            rows = [(label, rays, coherent) for label, rays in cams for coherent in (False, True)] + rows
        for label, rays, coherent in rows:
            rt = torch.from_numpy(rays).cuda()
            hits = r.trace_rays(rt, coherent=coherent)
            kw = {"coherent": coherent}

            def surface():
                return r.trace_surface(rt, **kw)

            def composed():
                return r.surface_at(r.trace_rays(rt, **kw))

            variants = [("trace_surface", surface), ("trace_rays", lambda: r.trace_rays(rt, **kw)), ("composed", composed),
                        ("trace_surface_again", surface), ("surface_at", lambda: r.surface_at(hits)), ("composed_again", composed)]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = {k: [] for k, _ in variants}
            for rep in range(REPS + 1):
                for k, f in variants:
                    a.record()
                    f()
                    b.record()
                    b.synchronize()
                    if rep:                      # (rep 0: warm-up)
                        ms[k].append(a.elapsed_time(b))
            best = {k: min(v) for k, v in ms.items()}
            n = len(rays)
            n_hit = int((hits[:, 1].view(torch.int32) >= 0).sum())
            line = {"scene": name, "rays": label, "n": n, "kernel": "packet" if coherent else "refill", "hit_fraction": round(n_hit / n, 4)}
            line.update({k + "_ms": round(v, 3) for k, v in best.items()})
            line.update({k + "_median_ms": round(float(np.median(v)), 3) for k, v in ms.items() if not k.endswith("_again")})
            line["spread_ms"] = round(max(abs(best["trace_surface"] - best["trace_surface_again"]), abs(best["composed"] - best["composed_again"])), 3)
            line["surface_at_GBps"] = round((n * 64 + n_hit * 76) / best["surface_at"] / 1e6, 1)
            print(json.dumps(line), flush=True)
            del rt, hits
    r.close()


if __name__ == "__main__":
    main()
