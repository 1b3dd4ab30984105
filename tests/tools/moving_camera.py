#!/usr/bin/env python3
"""What a call costs whose camera differs from the last call's: the bench frame (1 002 530-triangle wall, 3840x2160, accumulator,
16 frames per call) with the camera moved by a millimetre before every call, so that no call can reuse the camera hits the call
before it kept (lt_capi.hip: camera_hits_key) -- each runs its camera-hit pass and has its head squares store what they walk.  Then,
for comparison, the same number of calls with the camera left alone (frame_first moving on, as a progressive caller does).
LT_HIP_LIBRARY=<another build> measures that build the same way (tests/tools/ab_libs.sh); a build without the counter prints '-'."""
import sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import torch
from lens_trace_amd import _capi as C, scene as sc, synth
from lens_trace_amd.renderer import RendererHIP, make_desc

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
s = synth.heightfield_wall(708).validate()
r = RendererHIP(0)
r.set_scene(s)
W, H = 3840, 2160
stream = torch.cuda.current_stream().cuda_stream
counted = hasattr(r._L, "lt_hip_camera_hit_passes")
buf = None
for what, step in (("moving camera", 1e-3), ("still camera", 0.0)):
    times = []
    for rep in range(3):
        p0 = r.camera_hit_passes() if counted else 0
        for i in range(-3, CALLS):   # (three calls before the clock starts)
            if i == 0:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            cam = sc.camera_bytes(step * (i + 3 + rep * (CALLS + 3)), 2.5, -50.0, 0.0)
            d = make_desc(C.PROGRAM_ACCUMULATOR, W, H, 3, cam, frame_first=1 + 16 * (i + 3), frame_count=16, accumulate=True, accumulate_base=0)
            if buf is None:
                buf = torch.zeros(r.output_floats(d), dtype=torch.float32, device="cuda:0")
            r.render_device(d, buf.data_ptr(), buf.numel() * 4, stream)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / CALLS * 1e3)
        passes = str(r.camera_hit_passes() - p0) if counted else "-"
    print("%s: %s ms per 16-sample call over %d calls, three runs (camera-hit passes in the last run's %d calls: %s; walk %s)" % (
        what, " / ".join("%.3f" % t for t in times), CALLS, CALLS + 3, passes, r.stats()["shadow_packets"]))
