// lt_paths.hip -- the global-illumination programs over caller-supplied rays: the kernels behind lt_hip_shade_paths /
// lt_hip_shade_paths_device that the wavefront pipeline (lt_kernel.hpp) does not already have.
//
// The pipeline's bounce stages read path queues, per-slot direct / indirect terms and a sample index; only its camera stage
// (lt_gi_primary_kernel: squares, camera_ray) and its back end (lt_gi_resolve_kernel, lt_gi_blend25_kernel: tile arithmetic, the
// float image) know what a pixel is.  Here are their counterparts for a batch of rays:
//   the camera walk        ONCE PER RAY of a range, whatever the frames and samples: lt_trace_kernel's lane-refill closest-hit walk
//                          over the rays staged by lt_paths_stage_kernel (a scene with an own tree), or lt_paths_camera_kernel over
//                          the caller's tree (a scene without one).  The hit -- (primitive, hitType, u, v) -- is kept per ray.
//   lt_paths_primary_kernel  one lane per slot (ray, sample): what lt_gi_primary_kernel does behind its camera walk, the same
//                          functions in the same order: is_light -> direct = 1; a surface hit -> direct_light with seeds s, s+1, s+2
//                          (its shadow ray per lane: a batch has no squares to walk as packets), uniform_sample_hemisphere /
//                          align_hemisphere with s+3, s+4; direct[slot], indirect[slot] = 0; the surviving path into queue 0.
//   (the bounce stages: lt_capi.hip launches the pipeline's own kernels, unmodified)
//   lt_paths_resolve_kernel  one lane per ray: direct + indirect of its slots in order, the clamp, the 25-sample blend and the running
//                          mean -- lt_gi_resolve_kernel's, lt_gi_blend25_kernel's and lt_running_mean_kernel's expressions -- and one
//                          16-byte record.  No intermediate image.
#include "lt_paths.hpp"

using namespace lt;

namespace {

// Waves per SIMD lt_paths_primary_kernel is compiled for: light_sample's three double-precision random() beside a per-lane walk
// (lt_shade.hip's lighting kernels: the same budget).  DESIGN.md 5.11 has the resource table.
#ifndef LT_PATHS_WAVES
#define LT_PATHS_WAVES 4
#endif

// one atomic per wave: slot of this lane among the lanes with `keep` (lt_kernel.hpp: wave_append)
__device__ __forceinline__ uint32_t append(uint32_t* counter, bool keep) {
  const unsigned long long m = __ballot(keep);
  if (m == 0ull) return 0u;
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if ((int)__lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
  return base + (uint32_t)__popcll(m & ((1ull << __lane_id()) - 1ull));
}

// accumulator.frag:10-20 with n = the frames folded so far (lt_gi_resolve_kernel's and lt_running_mean_kernel's store)
__device__ __forceinline__ float fold(float acc, float c, uint32_t n) {
  if (n == 0u) return c;
  const float nf = (float)(int32_t)n, n1 = (float)((int32_t)n + 1);
  return (c + (acc * nf)) / n1;
}

}  // namespace

__global__ __launch_bounds__(256) void lt_paths_stage_kernel(lt_paths::Params p, float4* __restrict__ o, float4* __restrict__ d, uint4* __restrict__ m,
                                                             uint32_t* __restrict__ count) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0u) *count = p.nRays;
  if (r >= p.nRays) return;
  const float4 a = p.rays[2 * (size_t)(p.ray0 + r)], b = p.rays[2 * (size_t)(p.ray0 + r) + 1];
  o[r] = make_float4(a.x, a.y, a.z, 0.0f);
  d[r] = make_float4(b.x, b.y, b.z, 0.0f);
  m[r] = make_uint4(0u, 0xffffffffu, 0u, 0u);
}

// (the reference's order over the caller's tree, the stack in private memory: traverse's form for a scene without an own tree)
__global__ __launch_bounds__(kBlock) void lt_paths_camera_kernel(SceneDev sc, lt_paths::Params p) {
  extern __shared__ int lds_stack[];
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= p.nRays) return;
  Stack<false> st;
  st.lds = lds_stack + threadIdx.x;
  st.rows = kOwnRows;
  Counters c{};
  const float4 a = p.rays[2 * (size_t)(p.ray0 + r)], b = p.rays[2 * (size_t)(p.ray0 + r) + 1];
  const Ray ray{mk4(a.x, a.y, a.z, 2.0f), mk4(b.x, b.y, b.z, 0.0f)};
  Hit pl{0, 0, kFltMax, 0.0f, 0.0f};
  traverse<kGI, false, false, false>(sc, ray, false, 0, pl, st, c);
  p.hits[r] = make_uint4((uint32_t)pl.prim, (uint32_t)pl.hitType, __float_as_uint(pl.u), __float_as_uint(pl.v));
}

template <class CFG>
__global__ __launch_bounds__(kBlock, LT_PATHS_WAVES) void lt_paths_primary_kernel(SceneDev sc, lt_paths::Params p) {
  extern __shared__ int lds_stack[];   // kOwnRows rows: the stack of the shadow ray's per-lane walk
  Stack<CFG::kDeep> st;
  st.lds = lds_stack + threadIdx.x;
  st.rows = kOwnRows;
  Counters c{};
  const uint32_t slots = p.nRays * p.frames * p.perFrame;
  const uint32_t slot = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (p.directQueue && slot == 0u) *p.count0 = slots;   // (read by the launches behind this one)
  bool alive = false;
  V4 position{}, normal{}, dir{};
  float fx = 0.0f, fy = 0.0f;
  int prim = 0;
  uint32_t offset = 0u;
  if (slot < slots) {
    const uint32_t j = slot / p.nRays, r = slot - j * p.nRays;
    const uint32_t frame = j / p.perFrame, k = j - frame * p.perFrame;
    offset = p.perFrame == 1u ? frame : frame * 32u + k;
    const uint32_t s = p.sample + offset;
    fx = p.rays[2 * (size_t)(p.ray0 + r)].w;
    fy = p.rays[2 * (size_t)(p.ray0 + r) + 1].w;
    const uint4 h = p.hits[r];
    Hit pl{(int)h.x, (int)h.y, 0.0f, __uint_as_float(h.z), __uint_as_float(h.w)};
    V3 direct{0.0f, 0.0f, 0.0f};
    if (is_light(sc.lights, pl.prim)) {
      direct = V3{1.0f, 1.0f, 1.0f};
    } else if (pl.hitType == 1) {
      const float* pr = prim_ptr(sc, pl.prim);
      const Material* m = sc.mats + prim_material(pr);
      float ndotl;
      if (direct_light<kGI, CFG>(sc, pr, pl.prim, pl.u, pl.v, fx, fy, (float)s, (float)(s + 1u), (float)(s + 2u), 1.0f, position, normal, ndotl, st, c)) {
        direct = V3{m->diffuse[0] * ndotl, m->diffuse[1] * ndotl, m->diffuse[2] * ndotl};
      }
      const V4 hemi = random_hemisphere<CFG::kDevLibm>(fx, fy, (float)(s + 3u), (float)(s + 4u));
      dir = align_hemisphere<CFG::kDevLibm>(hemi, normal);
      prim = pl.prim;
      alive = p.giMaxDepth > 0;
    }
    p.direct[slot] = make_float4(direct.x, direct.y, direct.z, 0.0f);
    p.indirect[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  uint32_t at = slot;
  if (p.directQueue) {
    if (slot < slots && !alive) p.qm[at] = make_uint4(kDeadSlot, 0u, 0u, 0u);
  } else {
    at = append(p.count0, alive);
  }
  if (alive) {
    p.qo[at] = make_float4(position.x, position.y, position.z, fx);
    p.qd[at] = make_float4(dir.x, dir.y, dir.z, dir.w);
    p.qn[at] = make_float4(normal.x, normal.y, normal.z, normal.w);
    p.qm[at] = make_uint4(slot, (uint32_t)prim, __float_as_uint(fy), offset);
  }
}

template <class CFG>
__global__ __launch_bounds__(256) void lt_paths_resolve_kernel(lt_paths::Params p) {
  using M = Math<CFG::kDevLibm>;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.nRays) return;
  const uint4 h = p.hits[r];
  V3 acc{0.0f, 0.0f, 0.0f};
  if (p.folded != 0u) {
    const uint4 o = p.out[p.ray0 + r];
    acc = V3{__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z)};
  }
  for (uint32_t f = 0u; f < p.frames; f++) {
    V3 color{0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0u; k < p.perFrame; k++) {
      const size_t slot = (size_t)(f * p.perFrame + k) * p.nRays + r;
      const float4 di = p.direct[slot], in = p.indirect[slot];
      const V3 cn{di.x + in.x, di.y + in.y, di.z + in.z};   // gi.cl:374
      if (k == 0u) {
        color = cn;
      } else {
        const float a = M::div25((float)(25 - (int)k));
        color = V3{M::mad(1.0f - a, color.x, a * cn.x), M::mad(1.0f - a, color.y, a * cn.y), M::mad(1.0f - a, color.z, a * cn.z)};
      }
    }
    if (p.clampOutput) color = V3{M::clamp01(color.x), M::clamp01(color.y), M::clamp01(color.z)};
    const uint32_t n = p.folded + f;
    acc = V3{fold(acc.x, color.x, n), fold(acc.y, color.y, n), fold(acc.z, color.z, n)};
  }
  p.out[p.ray0 + r] = make_uint4(__float_as_uint(acc.x), __float_as_uint(acc.y), __float_as_uint(acc.z), h.y == 1u ? h.x : 0xffffffffu);
}

namespace lt_paths {

hipError_t launch_stage(const Params& p, float4* o, float4* d, uint4* m, uint32_t* count, hipStream_t s) {
  hipLaunchKernelGGL(lt_paths_stage_kernel, dim3((p.nRays + 255u) / 256u), dim3(256), 0, s, p, o, d, m, count);
  return hipGetLastError();
}

hipError_t launch_camera(const SceneDev& sc, const Params& p, hipStream_t s) {
  hipLaunchKernelGGL(lt_paths_camera_kernel, dim3((p.nRays + (uint32_t)kBlock - 1u) / (uint32_t)kBlock), dim3(kBlock), (uint32_t)(kOwnRows * kBlock * sizeof(int)), s, sc, p);
  return hipGetLastError();
}

hipError_t launch_primary(const SceneDev& sc, const Params& p, int devlibm, hipStream_t s) {
  const uint64_t slots = (uint64_t)p.nRays * p.frames * p.perFrame;
  if (slots == 0 || slots > 0xffffffffull) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)((slots + kBlock - 1) / kBlock)), block(kBlock);
  const uint32_t lds = (uint32_t)(kOwnRows * kBlock * sizeof(int));
  if (devlibm == 0) hipLaunchKernelGGL((lt_paths_primary_kernel<Config<false, false, 0>>), grid, block, lds, s, sc, p);
  else if (devlibm == 1) hipLaunchKernelGGL((lt_paths_primary_kernel<Config<false, false, 1>>), grid, block, lds, s, sc, p);
  else hipLaunchKernelGGL((lt_paths_primary_kernel<Config<false, false, 2>>), grid, block, lds, s, sc, p);
  return hipGetLastError();
}

hipError_t launch_resolve(const Params& p, int devlibm, hipStream_t s) {
  const dim3 grid((p.nRays + 255u) / 256u), block(256);
  if (devlibm == 0) hipLaunchKernelGGL((lt_paths_resolve_kernel<Config<false, false, 0>>), grid, block, 0, s, p);
  else if (devlibm == 1) hipLaunchKernelGGL((lt_paths_resolve_kernel<Config<false, false, 1>>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((lt_paths_resolve_kernel<Config<false, false, 2>>), grid, block, 0, s, p);
  return hipGetLastError();
}

}  // namespace lt_paths
