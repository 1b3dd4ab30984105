// lt_query.hpp -- ray queries over the resident scene (lt_query.hip): caller-supplied rays, each traced as the reference's
// `intersect` / `intersectIgnorePrimitiveIndex` would trace it (accumulator.cl:132-217) with the triangle epsilon of one of its
// kernel files (basic.cl:77-117, basic_lighting.cl:4, accumulator.cl:84), closest hit or any hit.  lt_capi.hip checks the call
// (lt_hip_trace_rays, lt_hip_trace_rays_device) and keeps the statistics; this is the launch.
#pragma once
#include "lt_device.hpp"

namespace lt_query {

// The caller's records, as the kernels read them: two 16-byte halves per ray, (origin.xyz, tmax) and (direction.xyz, ignore as
// int32 bits) -- lt_hip_ray.  Results: 16 bytes per ray (t, primitive or -1, u, v) -- lt_hip_hit -- or one occluded word.
struct Params {
  const float4* rays;
  uint4* hits;          // closest hit
  uint32_t* occluded;   // any hit
  uint32_t n;           // rays
  uint32_t* next;       // lt_query_kernel's work counters: eight, kQueueStride dwords apart, zeroed by launch() on the call's stream
  uint32_t refill;      // idle lanes that make a wave of lt_query_kernel take new rays
};

enum Epsilon { kEpsFloat7 = 0, kEpsDouble7 = 1, kEpsDouble4 = 2 };   // basic / custom_opencl, basic_lighting, the three others

// Enqueues the query on `s`: lt_query_packet_kernel when `coherent`, else lt_query_kernel.  Returns the first HIP error.
hipError_t launch(const lt::SceneDev& sc, const Params& p, Epsilon eps, bool anyHit, bool coherent, uint32_t cuCount, hipStream_t s);

// Multi-hit queries (lt_hip_trace_hits, lt_hip_trace_hits_device): every primitive the reference's traversal would accept with
// t < tmax, in ascending t (bit-equal t: the reference's traversal order).  Results: the first maxHits of them as maxHits
// lt_hip_hit records per ray, ray-major, unused slots {tmax, -1, 0, 0}; or, maxHits == 0, their number as one word per ray.
constexpr uint32_t kMaxHits = 8;   // LT_TRACE_MAX_HITS
// The sinks of lt_query_hits_kernel.  kFirstK and kCount are the descriptor's kinds.  The hit lists (lt_hip_trace_hits_list) are
// the other two: kCountWide, kCount as one uint64 per ray into offsets[i]; kList, the whole sequence of ray i as lt_hip_hit records
// into items[offsets[i] .. min(offsets[i + 1], capacity)) -- a length that would be negative is 0, so that with any offsets at all
// no store falls outside items[0 .. capacity).  A ray the own tree takes fills its segment in the own walk's order
// (lt_overlist::order_ray_hits sorts it then); every other ray keeps its segment sorted as it fills it (own_tree_takes).
enum HitsKind { kFirstK = 0, kCount = 1, kCountWide = 2, kList = 3 };
struct HitsParams {
  const float4* rays;
  uint4* hits;          // first K: record i * maxHits + j
  uint32_t* counts;     // count
  uint32_t n;
  uint32_t maxHits;     // 1..kMaxHits; 0 = every other kind
  uint32_t* next;       // as Params::next
  uint32_t refill;      // as Params::refill
  uint32_t kind;        // HitsKind
  uint32_t oneShot;     // kList: the offsets are this stream's own scan -- when offsets[n] > capacity the launch writes nothing
  unsigned long long* offsets;   // kCountWide: written, n words; kList: read, n + 1 words
  uint4* items;                  // kList: `capacity` records
  unsigned long long capacity;
};

// Which walk a ray of the query kernels takes: the own tree's, when the scene has one (SceneDev::rank8), every component of the
// origin and of the inverse direction is finite and the magnitudes are packet_ray_ok's; the reference's order over the caller's
// tree otherwise.  ix = 1.0f / direction.x and so on, as the kernels compute them.  The hit lists' ordering asks the same
// question about the same ray (lt_overlist.hip).
__device__ __forceinline__ bool finite_ray(const lt::Ray& ray, float ix, float iy, float iz) {
  return __builtin_fabsf(ix) < __builtin_inff() && __builtin_fabsf(iy) < __builtin_inff() && __builtin_fabsf(iz) < __builtin_inff() &&
         __builtin_fabsf(ray.o.x) < __builtin_inff() && __builtin_fabsf(ray.o.y) < __builtin_inff() && __builtin_fabsf(ray.o.z) < __builtin_inff();
}
__device__ __forceinline__ bool own_tree_takes(const lt::Ray& ray, float ix, float iy, float iz) {
  return finite_ray(ray, ix, iy, iz) && lt::packet_ray_ok(ray, ix, iy, iz);
}

// Enqueues lt_query_hits_kernel on `s`, the instantiation of p.kind.  Returns the first HIP error.
hipError_t launch_hits(const lt::SceneDev& sc, const HitsParams& p, Epsilon eps, uint32_t cuCount, hipStream_t s);

// Surface queries (lt_hip_surface_at, and lt_hip_trace_surface behind its closest-hit query): lt_surface_at_kernel over n hit
// records (lt_hip_hit) gives n 48-byte records lt_hip_surface -- the hit record, then (position.xyz, material), then (normal.xyz,
// flags) -- interpolated as shipped (fused multiply-adds) or with every product and sum rounded (the strict and portable
// flavours); a record whose primitive is not the scene's gives the miss form.  Enqueues on `s`; returns the first HIP error.
hipError_t launch_surface_at(const lt::SceneDev& sc, const uint4* hits, uint4* out, uint32_t n, bool shipped, uint32_t cuCount, hipStream_t s);

}  // namespace lt_query
