// lt_paths.hpp -- the global-illumination programs over caller-supplied rays (lt_paths.hip): a second front end and a second back
// end for the wavefront pipeline of lt_kernel.hpp.  Rays in (lt_hip_shade_ray), 16-byte records out (lt_hip_shade); the bounce
// stages between them are the pipeline's own launches, which know path slots and nothing of an image.  lt_capi.hip checks the call
// (lt_hip_shade_paths, lt_hip_shade_paths_device), cuts it into sets, launches the stages and keeps the statistics; these are the
// launches of the kernels that are new.
#pragma once
#include "lt_device.hpp"

namespace lt_paths {

// One SET of a call: rays [ray0, ray0 + nRays) of the batch, frames [folded, folded + frames) of the call's frames.  Its path slots
// are SAMPLE-MAJOR: slot = j * nRays + r for ray r of the range and sample j of the set -- j = frame of the set for the
// single-sample program (perFrame = 1), frame * 25 + k for the 25-sample program (perFrame = 25) -- so that a wavefront's 64 slots
// are 64 consecutive rays of one sample: the camera hits, the per-slot direct / indirect terms and the resolve's reads coalesce.
// Slot j's sampleIndex is sample + offset(j), offset = frame (perFrame = 1) or frame * 32 + k: the path carries the offset in m.w,
// where the bounce stages expect a path's frame (GiParams::sample + m.w).
struct Params {
  const float4* rays;      // the caller's records, two 16-byte halves per ray: (origin.xyz, film_x), (direction.xyz, film_y)
  uint4* out;              // the caller's results: (r, g, b, primitive or -1)
  uint4* hits;             // camera hit of ray r of the range: (primitive, hitType, u, v) -- the payload as the shading reads it
  uint32_t ray0, nRays;
  uint32_t frames;         // frames of the set
  uint32_t perFrame;       // 1 or 25
  uint32_t sample;         // sampleIndex of the set's first slot (GiParams::sample)
  uint32_t folded;         // frames of the call folded into `out` by earlier sets: the running mean's n
  int32_t giMaxDepth;
  int32_t clampOutput;     // linearKernel clamps a frame to [0, 1], tileKernel does not
  // queue 0 of the pipeline and its per-slot terms (GiParams::q[0], direct, indirect, counts[0])
  float4 *qo, *qd, *qn;
  uint4* qm;
  float4 *direct, *indirect;
  uint32_t* count0;
  uint32_t directQueue;    // != 0: queue 0 is direct-mapped (path of slot i at i, dead slots marked kDeadSlot, *count0 = slots); 0: appended to
};

// The camera rays of the range as lt_trace_kernel reads a queue -- o[r] = (origin.xyz, -), d[r] = (direction.xyz, +0),
// m[r].y = -1 (nothing ignored) -- and their number at *count.
hipError_t launch_stage(const Params& p, float4* o, float4* d, uint4* m, uint32_t* count, hipStream_t s);
// The camera walk of a scene without an own tree: one lane per ray over the caller's tree, into p.hits.
hipError_t launch_camera(const lt::SceneDev& sc, const Params& p, hipStream_t s);
// lt_paths_primary_kernel in the math flavour `devlibm` (Config::kDevLibm): one lane per slot of the set.
hipError_t launch_primary(const lt::SceneDev& sc, const Params& p, int devlibm, hipStream_t s);
// lt_paths_resolve_kernel: one lane per ray of the set.
hipError_t launch_resolve(const Params& p, int devlibm, hipStream_t s);

}  // namespace lt_paths
