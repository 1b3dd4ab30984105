// lt_build.hpp -- the canonical median build (include/lenstrace_hip.h, lt_hip_set_triangles): the caller's LinearBVHNode tree, the
// ordered 76-byte primitives and the light container made from bare triangles -- by kernels (lt_build.hip, run) for the two context
// forms, and in plain C++ (build_host) for lt_hip_build_scene_host, the tests' and a plugin's CPU definition.  Both produce the
// same bytes: every float operation of the rule is one rounded IEEE operation, every comparison is by value with the input index
// behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lt_prep.hpp"

namespace lt_build {

enum : uint32_t {
  kFlagNonFinite = 1,   // a vertex coordinate that is NaN or infinite
  kFlagMaterial = 2,    // a materialIndex outside [0, n_mats)
};

struct Out {
  uint32_t flags = 0;          // != 0: nothing was built (kFlag*)
  void* d_nodes = nullptr;     // from the allocator, the caller's to give back: 2n - 1 nodes of 32 bytes, pre-order
  void* d_prims = nullptr;     // n primitives of 76 bytes in leaf order
  void* d_lights = nullptr;    // the 260-byte light container
  int height = 0;              // ceil(log2 n)
  float ms_sort = 0, ms_levels = 0, ms_finish = 0;   // host wall time of the stages (each ends in a synchronisation when timed)
};

// d_positions / d_normals: 9 floats per triangle; d_material_indices may be null (all 0); d_materials: n_mats 32-byte records.
// All in device memory, read on `stream`.  d_flag: a device word the checks raise their flags in.  timed: wait behind every
// stage and fill the ms_ fields.  Returns a HIP error of a runtime call, or hipSuccess with out.flags telling whether the three
// buffers were made; nothing is left allocated when flags != 0 or on an error.
hipError_t run(const float* d_positions, const float* d_normals, const int32_t* d_material_indices, const void* d_materials, uint32_t n_mats,
               uint32_t n, hipStream_t stream, uint32_t* d_flag, bool timed, const lt_prep::Allocator& al, Out& out);

void release(Out& out, const lt_prep::Allocator& al);

// The same rule on the host.  nodes: 32 (2n - 1) bytes, prims: 76 n bytes, lights: 260 bytes.  Returns 0, or kFlag* and writes nothing.
uint32_t build_host(const float* positions, const float* normals, const int32_t* material_indices, const void* materials, uint32_t n_mats,
                    uint32_t n, void* nodes, void* prims, void* lights);

}  // namespace lt_build
