#!/usr/bin/env python3
"""Shaded-path timing (lt_hip_shade_paths_device, lens_trace_amd/csrc/lt_paths.hip): HIP-event time per call, best of LT_TIMING_REPS
(5) after a warm-up, 16 bounces, 1 and 16 frames of global_illumination (and 1 frame of the 25-sample program), on
  * the 4K camera rays (3840 x 2160, camera_bytes(0, 2.5, -50), yaw 0) of the 1 M-triangle wall, row-major and in 8x8-square order,
  * 8.3 M random rays through the wall's bounds (origins inside the root box, directions uniform on the sphere),
  * the 1080p camera rays of the Cornell box (tests/golden/cornell_box_O0.ltsb),
and beside each camera batch, measured in the same process, `render` of the same program, frames and depth (the parent commit's
function over the reference camera, which a ray batch is not expected to beat).  `slots` rows force LT_PATHS_SLOTS: how the
default set size was chosen.  One process per row, each under its own time limit; a row that fails ends the run.  One JSON line per
row.  For the kernels alone run one row under `rocprofv3 --kernel-trace --stats -- python3 <this file> --row <scene> <rays> <program>
<frames> [slots]`."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = int(os.environ.get("LT_TIMING_REPS", "5"))
ROW_SECONDS = int(os.environ.get("LT_TIMING_ROW_SECONDS", "240"))
GI, GI25 = "global_illumination", "global_illumination25"
ROWS = [("wall", "rows", GI, 1), ("wall", "rows", GI, 16), ("wall", "squares", GI, 1), ("wall", "squares", GI, 16),
        ("wall", "random", GI, 1), ("wall", "random", GI, 16), ("wall", "rows", GI25, 1),
        ("cornell", "rows", GI, 1), ("cornell", "rows", GI, 16),
        ("wall", "rows", GI, 16, 8 << 20), ("wall", "rows", GI, 16, 16 << 20), ("wall", "rows", GI, 16, 32 << 20), ("wall", "rows", GI, 16, 144 << 20)]


def camera_rays(np, make_shade_rays, cam, W, H, order):
    f32 = np.float32
    ys, xs = np.mgrid[0:H, 0:W]
    if order == "squares":
        ys = ys.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
        xs = xs.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    fx = xs.astype(f32) / f32(W) - f32(0.5)
    fy = ys.astype(f32) / f32(H) - f32(0.5)
    o = np.stack([f32(cam[0]) + fx, f32(cam[1]) + fy, np.full_like(fx, f32(cam[2]))], axis=-1)
    d = np.stack([f32(0.0) - fx, f32(0.0) - fy, np.full_like(fx, f32(5.0))], axis=-1)
    return make_shade_rays(o, d, fx, fy)


def row(scene, order, program, frames, slots=None):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from lens_trace_amd import _capi as C
    from lens_trace_amd import scene as sc
    from lens_trace_amd import synth
    from lens_trace_amd.renderer import RendererHIP, make_desc, make_shade_rays
    pos = (0.0, 2.5, -50.0)
    cam = sc.camera_bytes(*pos, 0.0)
    if scene == "wall":
        s, (W, H) = synth.heightfield_wall(), (3840, 2160)
    else:
        s, (W, H) = sc.load_ltsb(os.path.join(ROOT, "tests", "golden", "cornell_box_O0.ltsb")).validate(), (1920, 1080)
    if order == "random":
        rng = np.random.default_rng(1)
        lo, hi = s.node_view["boundsMin"][0].astype(np.float64), s.node_view["boundsMax"][0].astype(np.float64)
        n = W * H
        rays = make_shade_rays(rng.uniform(lo, hi, (n, 3)), rng.normal(0, 1, (n, 3)), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n))
    else:
        rays = camera_rays(np, make_shade_rays, pos, W, H, order)
    pid = C.PROGRAM_GLOBAL_ILLUMINATION_25 if program == GI25 else C.PROGRAM_GLOBAL_ILLUMINATION

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

    r = RendererHIP(0)
    r.set_scene(s)
    rt = torch.from_numpy(rays).cuda()
    out = {"scene": scene, "rays": order, "n": len(rays), "program": program, "frames": frames, "slots": slots or "default"}
    got = r.shade_paths(rt, program=pid, frame_count=frames)
    torch.cuda.synchronize()
    if slots:   # the same bytes however the call is cut into sets
        os.environ["LT_PATHS_SLOTS"] = str(slots)
        out["equals_default_sets"] = bool(torch.equal(got.view(torch.int32), r.shade_paths(rt, program=pid, frame_count=frames).view(torch.int32)))
    out["hit_fraction"] = round(float((got[:, 3].view(torch.int32) >= 0).float().mean()), 4)
    out["kernel_launches"] = r.stats()["kernel_launches"]
    out["paths_ms_min"], out["paths_ms_median"] = best_of(lambda: r.shade_paths(rt, program=pid, frame_count=frames))
    if order != "random" and not slots:
        image = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
        d = make_desc(pid, W, H, 3, cam, frame_first=0, frame_count=frames, accumulate=True)
        out["render_ms_min"], out["render_ms_median"] = best_of(lambda: r.render_device(d, image.data_ptr(), image.numel() * 4))
    print(json.dumps(out), flush=True)
    r.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--row":
        a = sys.argv[2:]
        row(a[0], a[1], a[2], int(a[3]), int(a[4]) if len(a) > 4 else None)
        return 0
    for spec in ROWS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--row"] + [str(x) for x in spec], timeout=ROW_SECONDS).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:   # (a row that failed or ran out of time: nothing more is started on the GPU)
            print(json.dumps({"row": spec, "exit": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
