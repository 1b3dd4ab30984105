// lt_shade.hip -- shading of caller-supplied rays: the kernel behind lt_hip_shade_rays / lt_hip_shade_rays_device.
//
// Every program's shading is a function of (ray, filmX, filmY, frameCount) and takes no pixel (shade_pixel, lt_device.hpp).  Here
// the ray comes from memory instead of camera_ray, with camera_ray's w components (origin.w = cameraPosition.w + film.w = 2,
// direction.w = aperture.w - film.w = +0), and the result of frames frameFirst .. frameFirst + frameCount - 1 is folded in frame
// order by accumulator.frag's running mean from n = 0 -- what lt_hip_render with accumulate = 1, accumulate_base = 0 leaves in a
// pixel (render_square's store, lt_running_mean_kernel: the same expression).
//
// lt_shade_rays_kernel is lt_query_kernel's claim / stage / refill loop (lt_query.hip) with a lane that carries a PHASE instead of
// one walk.  The walks of one ray, in the order shade_pixel runs them:
//   accumulator     the camera walk (closest hit); per frame light_sample and one shadow walk
//   basic_lighting  the same with 25 samples per frame; one camera walk serves them all, as in shade_pixel's non-counting kernels
//   basic           the camera walk and, on a lens material, the two further closest-hit walks of trace_ray_through_lens
//   custom_opencl   the camera walk
// A lane whose walk is done does the arithmetic that lies between it and the next walk (next_phase: the existing functions, in
// shade_lighting's / trace_ray_through_lens' / shade_pixel's order) -- together with the other lanes of its wave that are as far,
// see the kernel --, sets the next ray up in place and walks on; it becomes idle -- and is refilled -- only when its ray's last
// phase is done, and then writes one 16-byte result.
//
// Shadow and camera walks share ONE step function and run the same instructions, whatever the mix of phases in the wave:
// own_walk_step's closest-hit form accepts the first triangle of a walk under the any-hit form's condition (tt < payload t, the
// payload's t = tmax until then; the order table is consulted only once a hit is held), and the own walks never prune by t.  So a
// shadow-phase lane takes the closest-hit step and stops as soon as it holds a hit: the hitType it reports is the any-hit walk's.
// (The alternative, an any-hit and a closest-hit instantiation under complementary lane masks, runs each step of a mixed wave
// twice and holds the walk's code twice.)
//
// Rays the own tree does not take -- a non-finite component, beyond packet_ray_ok, every ray of a scene without an own tree --
// walk the caller's tree in the reference's order, each such phase at once in the lane that meets it.
#include "lt_shade.hpp"

using namespace lt;

namespace {

// Waves per SIMD the kernels are compiled for: the lighting programs (light_sample's three double-precision random() want
// registers) and the two others.  DESIGN.md 5.10 has the resource table and the timings these were chosen from.
#ifndef LT_SHADE_WAVES_LIGHTING
#define LT_SHADE_WAVES_LIGHTING 4
#endif
#ifndef LT_SHADE_WAVES_SIMPLE
#define LT_SHADE_WAVES_SIMPLE 6
#endif
constexpr int shade_waves(int program) { return program == kBasicLighting || program == kAccumulator ? LT_SHADE_WAVES_LIGHTING : LT_SHADE_WAVES_SIMPLE; }

constexpr int kShadeClaim = 512;  // rays a wave claims per atomic (lt_query_kernel's kQueryClaim)

__device__ __forceinline__ bool finite_ray(const Ray& ray, float ix, float iy, float iz) {
  return __builtin_fabsf(ix) < __builtin_inff() && __builtin_fabsf(iy) < __builtin_inff() && __builtin_fabsf(iz) < __builtin_inff() &&
         __builtin_fabsf(ray.o.x) < __builtin_inff() && __builtin_fabsf(ray.o.y) < __builtin_inff() && __builtin_fabsf(ray.o.z) < __builtin_inff();
}

// What a lane keeps of its ray from one phase to the next.
struct Phase {
  float fx, fy;        // film position: random()'s key
  int prim;            // the result's primitive: the camera ray's own hit, -1 on a miss
  int hprim, hhit;     // the camera hit as the shading reads it (a miss leaves primitive 0 in the payload: is_light and the lens
  float hu, hv;        // chain look at it without asking hitType)
  V3 acc;              // running mean of the frames done
  V3 color;            // basic_lighting: the blend of this frame's samples so far
  uint32_t f, k;       // frame and sample at hand
  float ndotl;         // of the sample whose shadow ray walks
  uint32_t step;       // 0: the camera walk; lighting programs 1: a shadow walk; basic 1, 2: the lens chain's walks
};

// accumulator.frag:10-20 with n = the frames folded so far: render_square's store
__device__ __forceinline__ float fold(float acc, float c, uint32_t n) {
  if (n == 0u) return c;
  const float nf = (float)(int32_t)n, n1 = (float)((int32_t)n + 1);
  return (c + (acc * nf)) / n1;
}

// Position and normal of a hit, as trace_ray_through_lens interpolates them (basic.cl:228-233).
template <class CFG>
__device__ __forceinline__ void lens_surface(const float* pr, float u, float v, V4& position, V4& normal) {
  const V3 b = barycentrics(u, v);
  const V3 p3 = bary3<CFG::kDevLibm>(pr + 0, pr + 3, pr + 6, b);
  position = mk4(p3.x, p3.y, p3.z, 1.0f);
  const V3 n3 = bary3<CFG::kDevLibm>(pr + 9, pr + 12, pr + 15, b);
  normal = mk4(n3.x, n3.y, n3.z, 0.0f);
}

// The lane's walk is done, its result in `pl`: everything up to the ray's next walk.  True: `ray`, `ign`, `shadow` and `pl` are the
// next walk's.  False: the ray is done and `rgb` is its colour.
template <int PROGRAM, class CFG>
__device__ __forceinline__ bool next_phase(const SceneDev& sc, const lt_shade::Params& sp, Phase& ph, Ray& ray, int& ign, bool& shadow, Hit& pl, V3& rgb) {
  using M = Math<CFG::kDevLibm>;
  if (PROGRAM == kCustom) {   // shade_custom
    ph.prim = pl.hitType == 1 ? pl.prim : -1;
    V3 c{0.0f, 0.0f, 0.0f};
    if (pl.hitType == 1) c = V3{pl.u, pl.v, (float)((1.0 - (double)pl.u) - (double)pl.v)};
    rgb = c;
    for (uint32_t f = 1u; f < sp.frameCount; f++) rgb = V3{fold(rgb.x, c.x, f), fold(rgb.y, c.y, f), fold(rgb.z, c.z, f)};
    return false;
  } else if (PROGRAM == kBasic) {   // shade_basic, trace_ray_through_lens
    if (ph.step == 0u) {
      ph.prim = pl.hitType == 1 ? pl.prim : -1;
      ph.hprim = pl.prim;
      ph.hhit = pl.hitType;
      if (pl.hitType == 1) {
        const float* pr = prim_ptr(sc, pl.prim);
        const Material* m = sc.mats + prim_material(pr);
        if ((double)m->dissolve < 1.0) {
          V4 position, normal;
          lens_surface<CFG>(pr, pl.u, pl.v, position, normal);
          const V4 tdir = refract_<CFG::kDevLibm>(ray.d, normal, 1.0f, m->ior);
          ray = Ray{position, tdir};
          ign = pl.prim;
          shadow = false;
          pl = Hit{0, 0, kFltMax, 0.0f, 0.0f};
          ph.step = 1u;
          return true;
        }
      }
    } else if (ph.step == 1u) {
      const float* pr = prim_ptr(sc, pl.prim);
      const Material* m = sc.mats + prim_material(pr);
      V4 position, normal;
      lens_surface<CFG>(pr, pl.u, pl.v, position, normal);
      const V4 tdir = refract_<CFG::kDevLibm>(ray.d, neg4(normal), m->ior, 1.0f);
      ray = Ray{position, tdir};
      ign = pl.prim;
      shadow = false;
      pl = Hit{0, 0, kFltMax, 0.0f, 0.0f};
      ph.step = 2u;
      return true;
    }
    V3 c{0.0f, 0.0f, 0.0f};
    if (ph.hhit == 1) {   // the last hit's material; the camera hit's where the chain ends in a miss
      const Material* m = sc.mats + prim_material(prim_ptr(sc, pl.hitType == 1 ? pl.prim : ph.hprim));
      c = V3{m->diffuse[0], m->diffuse[1], m->diffuse[2]};
    }
    rgb = c;
    for (uint32_t f = 1u; f < sp.frameCount; f++) rgb = V3{fold(rgb.x, c.x, f), fold(rgb.y, c.y, f), fold(rgb.z, c.z, f)};
    return false;
  } else {   // shade_lighting, and shade_pixel's 25-sample blend and clamp
    V3 cn{0.0f, 0.0f, 0.0f};
    bool have = false;
    if (ph.step == 0u) {
      ph.prim = pl.hitType == 1 ? pl.prim : -1;
      ph.hprim = pl.prim; ph.hhit = pl.hitType; ph.hu = pl.u; ph.hv = pl.v;
      ph.f = 0u; ph.k = 0u;
      ph.step = 1u;
    } else {   // a shadow walk: the sample's colour
      if (pl.hitType == 0) {
        const Material* m = sc.mats + prim_material(prim_ptr(sc, ph.hprim));
        cn = V3{m->diffuse[0] * ph.ndotl, m->diffuse[1] * ph.ndotl, m->diffuse[2] * ph.ndotl};
      }
      have = true;
    }
    for (;;) {
      if (!have) {   // sample k of frame f
        const uint32_t frame = sp.frameFirst + ph.f;
        const uint32_t s = PROGRAM == kBasicLighting ? frame * 32u + ph.k : frame;
        if (PROGRAM == kAccumulator && is_light(sc.lights, ph.hprim)) {
          cn = V3{1.0f, 1.0f, 1.0f};
        } else if (ph.hhit == 1) {
          V4 position, normal, toLight;
          float tmax;
          light_sample<CFG>(sc, prim_ptr(sc, ph.hprim), ph.hu, ph.hv, ph.fx, ph.fy, (float)s, (float)(s + 1u), (float)(s + 2u), 0.0f, position, normal,
                            toLight, tmax, ph.ndotl);
          ray = Ray{position, toLight};
          ign = ph.hprim;
          shadow = true;
          pl = Hit{0, 0, tmax, 0.0f, 0.0f};
          return true;
        } else {
          cn = V3{0.0f, 0.0f, 0.0f};
        }
      }
      have = false;
      V3 c = cn;
      if (PROGRAM == kBasicLighting) {
        if (ph.k != 0u) {
          const float a = M::div25((float)(25 - (int)ph.k));
          c = V3{M::mad(1.0f - a, ph.color.x, a * cn.x), M::mad(1.0f - a, ph.color.y, a * cn.y), M::mad(1.0f - a, ph.color.z, a * cn.z)};
        }
        ph.color = c;
        if (++ph.k < 25u) continue;
        ph.k = 0u;
      }
      if (sp.clampOutput) c = V3{M::clamp01(c.x), M::clamp01(c.y), M::clamp01(c.z)};
      ph.acc = V3{fold(ph.acc.x, c.x, ph.f), fold(ph.acc.y, c.y, ph.f), fold(ph.acc.z, c.z, ph.f)};
      if (++ph.f == sp.frameCount) {
        rgb = ph.acc;
        return false;
      }
    }
  }
}

}  // namespace

// Lane states: idle (takes a staged ray at the next refill), ready (a ray is set up: own_ray or the reference walk next), walking,
// and walked: the walk is done and next_phase is due.  next_phase is hundreds of instructions for the lighting programs, and
// a wave pays for it whenever ONE lane runs it: the lanes wait in `walked` until sp.shadeBatch of them do, or nobody walks
// (custom_opencl's is a few instructions: its lanes do not wait).
template <int PROGRAM, class CFG>
__global__ __launch_bounds__(kBlock, shade_waves(PROGRAM)) void lt_shade_rays_kernel(SceneDev sc, lt_shade::Params sp) {
  using u64 = unsigned long long;
  extern __shared__ int lds_stack[];   // [kTraceRows stack rows][lt_shade::kStageRows rows of staged rays], 64 lanes each
  int* const col = lds_stack + threadIdx.x;
  int* const stage = lds_stack + kTraceRows * kBlock;
  const uint32_t total = sp.n;
  const uint32_t lane = threadIdx.x;
  const u64 below = (1ull << lane) - 1ull;
  const bool ownTree = sc.rank8 != nullptr;
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kShadeClaim ? (uint32_t)kShadeClaim : share);
  enum { kIdle = 0, kReady = 1, kWalking = 2, kWalked = 3 };
  int state = kIdle;
  uint32_t stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;
  Ray ray{};
  float ix = 0.0f, iy = 0.0f, iz = 0.0f;
  OwnRay w{};
  Hit pl{0, 0, 0.0f, 0.0f, 0.0f};
  Phase ph{};
  int ign = -1;
  bool shadow = false;
  uint32_t idx = 0u, e = 0u;
  int sp_ = 0;
  int deep[kOwnRows + kOwnDeep - kTraceRows];
  // the walk at hand is done: the next one is set up, or the result goes out
  auto advance = [&]() {
    V3 rgb{0.0f, 0.0f, 0.0f};
    if (next_phase<PROGRAM, CFG>(sc, sp, ph, ray, ign, shadow, pl, rgb)) {
      state = kReady;
    } else {
      sp.out[idx] = make_uint4(__float_as_uint(rgb.x), __float_as_uint(rgb.y), __float_as_uint(rgb.z), (uint32_t)ph.prim);
      state = kIdle;
    }
  };
  for (;;) {
    const u64 walked = __builtin_amdgcn_ballot_w64(state == kWalked);
    if (walked != 0ull && (PROGRAM == kCustom || (uint32_t)__popcll(walked) >= sp.shadeBatch || __builtin_amdgcn_ballot_w64(state == kWalking) == 0ull)) {
      if (state == kWalked) advance();
    }
    const u64 idle = __builtin_amdgcn_ballot_w64(state == kIdle);
    const uint32_t nIdle = (uint32_t)__popcll(idle);
    if ((nIdle >= sp.refill || nIdle == (uint32_t)kBlock) && (stageTaken < stageCount || !drained)) {
      if (stageTaken == stageCount) {
        while (claimNext == claimEnd && sweep < 8u) {
          const uint32_t part = (home + sweep) & 7u;
          const uint32_t lo = (uint32_t)((uint64_t)total * part / 8u / kBlock * kBlock), hi = part == 7u ? total : (uint32_t)((uint64_t)total * (part + 1u) / 8u / kBlock * kBlock);
          uint32_t got = 0u;
          if (lane == 0u) got = atomicAdd(&sp.next[part * kQueueStride], claim);
          got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
          if (got >= hi - lo) { sweep++; continue; }
          claimNext = lo + got;
          claimEnd = hi - claimNext < claim ? hi : claimNext + claim;
        }
        const uint32_t base = claimNext;
        const uint32_t batch = claimEnd - base < (uint32_t)kBlock ? claimEnd - base : (uint32_t)kBlock;
        claimNext = base + batch;
        drained = claimNext == claimEnd && sweep >= 8u;
        stageTaken = 0u;
        stageCount = batch;
        if (lane < batch) {   // the caller's record: two coalesced 16-byte loads
          const float4 a = sp.rays[2 * (size_t)(base + lane)], b = sp.rays[2 * (size_t)(base + lane) + 1];
          stage[0 * kBlock + lane] = __float_as_int(a.x); stage[1 * kBlock + lane] = __float_as_int(a.y); stage[2 * kBlock + lane] = __float_as_int(a.z);
          stage[3 * kBlock + lane] = __float_as_int(b.x); stage[4 * kBlock + lane] = __float_as_int(b.y); stage[5 * kBlock + lane] = __float_as_int(b.z);
          stage[6 * kBlock + lane] = __float_as_int(a.w);   // film x
          stage[7 * kBlock + lane] = __float_as_int(b.w);   // film y
          stage[8 * kBlock + lane] = (int)(base + lane);
        }
        // (one wavefront per workgroup: its own LDS writes are visible to it once they have completed -- the reads below wait for them)
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = (uint32_t)__popcll(idle & below);
      if (state == kIdle && mine < take) {
        const uint32_t s = stageTaken + mine;
        idx = (uint32_t)stage[8 * kBlock + s];
        ray = Ray{mk4(__int_as_float(stage[0 * kBlock + s]), __int_as_float(stage[1 * kBlock + s]), __int_as_float(stage[2 * kBlock + s]), 2.0f),
                  mk4(__int_as_float(stage[3 * kBlock + s]), __int_as_float(stage[4 * kBlock + s]), __int_as_float(stage[5 * kBlock + s]), 0.0f)};
        ph = Phase{};
        ph.fx = __int_as_float(stage[6 * kBlock + s]);
        ph.fy = __int_as_float(stage[7 * kBlock + s]);
        pl = Hit{0, 0, kFltMax, 0.0f, 0.0f};   // the camera payload: ignores nothing
        ign = -1;
        shadow = false;
        state = kReady;
      }
      stageTaken += take;
    }
    if (state == kReady) {
      ix = 1.0f / ray.d.x; iy = 1.0f / ray.d.y; iz = 1.0f / ray.d.z;
      if (ownTree && finite_ray(ray, ix, iy, iz) && packet_ray_ok(ray, ix, iy, iz)) {
        w = own_ray(sc, ray, ix, iy, iz, ign);
        e = 0u;
        sp_ = 0;
        state = kWalking;
      } else {   // the reference's order over the caller's tree
        ScratchStack ss;
        Counters c{};
        if (shadow) traverse_nodes_impl<PROGRAM, ScratchStack, false, false, true, false>(sc, ray, ix, iy, iz, true, ign, pl, ss, c);
        else traverse_nodes_impl<PROGRAM, ScratchStack, false, false, false, false>(sc, ray, ix, iy, iz, true, ign, pl, ss, c);
        state = kWalked;
      }
    }
    if (__builtin_amdgcn_ballot_w64(state != kIdle) == 0ull) {
      if (drained && stageTaken == stageCount) break;
      continue;
    }
    if (state == kWalking) {
      if (own_walk_step<PROGRAM, false, kTraceRows>(sc, ray, ix, iy, iz, w, pl, col, deep, e, sp_) || (shadow && pl.hitType != 0)) state = kWalked;
    }
  }
}

namespace lt_shade {

template <int PROGRAM, int M>
static void launch_one(const SceneDev& sc, const Params& p, uint32_t cuCount, hipStream_t s) {
  const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);
  const uint32_t resident = cuCount * 4u * (uint32_t)shade_waves(PROGRAM);   // every wave slot the registers leave, once
  hipLaunchKernelGGL((lt_shade_rays_kernel<PROGRAM, Config<false, false, M>>), dim3(chunks < resident ? chunks : resident), dim3(kBlock),
                     (uint32_t)((kTraceRows + kStageRows) * kBlock * sizeof(int)), s, sc, p);
}

template <int M>
static bool launch_math(const SceneDev& sc, const Params& p, int program, uint32_t cuCount, hipStream_t s) {
  switch (program) {
    case kBasic: launch_one<kBasic, M>(sc, p, cuCount, s); return true;
    case kBasicLighting: launch_one<kBasicLighting, M>(sc, p, cuCount, s); return true;
    case kAccumulator: launch_one<kAccumulator, M>(sc, p, cuCount, s); return true;
    case kCustom: launch_one<kCustom, M>(sc, p, cuCount, s); return true;
    default: return false;
  }
}

hipError_t launch(const SceneDev& sc, const Params& p, int program, int devlibm, uint32_t cuCount, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (p.frameCount == 0u) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(p.next, 0, 8 * kQueueStride * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const bool known = devlibm == 0 ? launch_math<0>(sc, p, program, cuCount, s)
                     : devlibm == 1 ? launch_math<1>(sc, p, program, cuCount, s) : launch_math<2>(sc, p, program, cuCount, s);
  if (!known) return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace lt_shade
