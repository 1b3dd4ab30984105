"""Making a 1 M-triangle benchmark mesh (heightfield_wall, triangle_soup) resident: build_from_triangles(BVH_MEDIAN) + set_scene --
the only way before lt_hip_set_triangles -- against set_triangles from host arrays and from device tensors.  One warm-up round,
then five rounds with the three arms alternating; medians, the LT_DEBUG_SCENE_TIMING laps of one call per form (stderr), and a
check that the resident buffers equal the host canonical build.  Run on the GPU box:
python tests/tools/set_triangles_timing.py [--out FILE.json]   (--dry: no GPU, 5000 triangles, the script's own plumbing)"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lens_trace_amd import scene as sc   # noqa: E402
from lens_trace_amd import synth   # noqa: E402

DRY = "--dry" in sys.argv
ROUNDS = 5


def mesh(name):
    """The arrays the benchmark scene hands to build_from_triangles, in their input order."""
    keep = synth.build_from_triangles
    got = {}

    def capture(pos, nrm, mi, mats, camera=None, bvh=None):
        got["t"] = (np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(mi, np.int32), mats)
        return None
    synth.build_from_triangles = capture
    try:
        getattr(synth, name)()
    finally:
        synth.build_from_triangles = keep
    return got["t"]


def main():
    out = {}
    r = None
    if not DRY:
        import torch
        from lens_trace_amd.renderer import RendererHIP
        r = RendererHIP(0)
    for name in ("heightfield_wall", "triangle_soup"):
        T = mesh(name)
        n = T[0].shape[0]
        print(name, n, "triangles", flush=True)
        if DRY:
            T = tuple(None if a is None else a[:5000] if i < 3 else a for i, a in enumerate(T))
        t0 = time.perf_counter()
        want = sc.build_from_triangles_canonical(*T)
        t_canon = time.perf_counter() - t0
        print("  host canonical build %.1f ms" % (1e3 * t_canon), flush=True)
        if DRY:
            s = sc.build_from_triangles(*T, bvh=sc.BVH_MEDIAN)
            print("  dry: baseline builder ok", s.n_nodes)
            continue
        dev = (torch.from_numpy(T[0]).cuda(), torch.from_numpy(T[1]).cuda(), torch.from_numpy(T[2]).cuda(),
               torch.from_numpy(np.ascontiguousarray(T[3]).view(np.uint8).reshape(-1).copy()).cuda())
        torch.cuda.synchronize()
        times = {"baseline_build": [], "baseline_set_scene": [], "baseline": [], "host_arrays": [], "device_tensors": []}

        def baseline():
            t0 = time.perf_counter()
            s = sc.build_from_triangles(*T, bvh=sc.BVH_MEDIAN)
            t1 = time.perf_counter()
            r.set_scene(s)
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, t2 - t0

        def host_arrays():
            t0 = time.perf_counter()
            r.set_triangles(*T)
            return time.perf_counter() - t0

        def device_tensors():
            t0 = time.perf_counter()
            r.set_triangles(*dev)
            return time.perf_counter() - t0

        for rnd in range(ROUNDS + 1):   # (round 0 warms up; the arms alternate)
            b = baseline()
            h = host_arrays()
            d = device_tensors()
            if rnd:
                times["baseline_build"].append(b[0]); times["baseline_set_scene"].append(b[1]); times["baseline"].append(b[2])
                times["host_arrays"].append(h); times["device_tensors"].append(d)
        got = r.scene_buffers()
        same = all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ("nodes", "prims", "materials", "lights"))
        st = r.stats()
        row = {k: {"median_ms": 1e3 * statistics.median(v), "all_ms": [round(1e3 * x, 3) for x in v]} for k, v in times.items()}
        row.update(triangles=n, equals_host_canonical=bool(same), host_canonical_ms=1e3 * t_canon, scene_reused=st["scene_reused"],
                   scene_uploads=st["scene_uploads"], own_tree_height=st["own_tree_height"])
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        # the laps, once per form
        os.environ["LT_DEBUG_SCENE_TIMING"] = "1"
        # (in the order of the timed rounds: each form's call follows the call it followed there)
        sys.stderr.write("--- laps: %s, baseline set_scene\n" % name); sys.stderr.flush()
        r.set_scene(sc.build_from_triangles(*T, bvh=sc.BVH_MEDIAN))
        sys.stderr.write("--- laps: %s, host arrays\n" % name); sys.stderr.flush()
        r.set_triangles(*T)
        sys.stderr.write("--- laps: %s, device tensors\n" % name); sys.stderr.flush()
        r.set_triangles(*dev)
        del os.environ["LT_DEBUG_SCENE_TIMING"]
        assert same, "resident buffers differ from the host canonical build"
    if r is not None:
        r.close()
        if "--out" in sys.argv:
            with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
