// lt_shade.hpp -- shading of caller-supplied rays (lt_shade.hip): for each ray of a batch the colour the named program's `shade`
// would return for it, had it been a pixel's camera ray at the given film position and frame (shade_pixel, lt_device.hpp), its
// frames folded by accumulator.frag's running mean.  lt_capi.hip checks the call (lt_hip_shade_rays, lt_hip_shade_rays_device)
// and keeps the statistics; this is the launch.
#pragma once
#include "lt_device.hpp"

namespace lt_shade {

// The caller's records, as the kernel reads them: two 16-byte halves per ray, (origin.xyz, film_x) and (direction.xyz, film_y)
// -- lt_hip_shade_ray.  Results: 16 bytes per ray (r, g, b, primitive or -1) -- lt_hip_shade.
struct Params {
  const float4* rays;
  uint4* out;
  uint32_t n;            // rays
  uint32_t* next;        // the kernel's work counters: eight, kQueueStride dwords apart, zeroed by launch() on the call's stream
  uint32_t refill;       // idle lanes that make a wave take new rays
  uint32_t shadeBatch;   // lanes whose walk is done that make a wave run the shading between two walks (or all that are left)
  uint32_t frameFirst;   // frames frameFirst .. frameFirst + frameCount - 1, folded in that order from n = 0
  uint32_t frameCount;   // >= 1
  int32_t clampOutput;   // linearKernel of the lighting programs clamps every frame to [0, 1], tileKernel does not
};

constexpr int kStageRows = 9;   // origin 3, direction 3, film position 2, index

// Enqueues lt_shade_rays_kernel on `s` for `program` (kBasic, kBasicLighting, kAccumulator or kCustom; anything else is
// hipErrorInvalidValue) in the math flavour `devlibm` (Config::kDevLibm).  Returns the first HIP error.
hipError_t launch(const lt::SceneDev& sc, const Params& p, int program, int devlibm, uint32_t cuCount, hipStream_t s);

}  // namespace lt_shade
