// lt_kernel.hpp -- the render kernel of liblenstrace-hip.so, as a device-side header: included by lt_capi.hip for the six
// built-in programs and by the run-time compiled translation unit of a user program (lt_hip_resolve_program ->
// hipRTC), whose `user_shade` it calls (the reference JIT-compiles a user's kernel *file*,
// src/opencl/renderer_opencl.cpp:35-54; here the user supplies the shade step in HIP and gets the built-in traversal).
#pragma once
#include "lt_device.hpp"
#include "lt_entry_cut.hpp"

using namespace lt;

// One lane per pixel; a workgroup is ONE wavefront covering an 8x8 pixel square (no intra-workgroup tail: the
// LDS stack and the wave slot are released as soon as that wave's slowest ray ends).  Workgroup ids are
// remapped so that the blocks one XCD receives (ids congruent mod 8) cover one contiguous part of the
// image: each XCD's private L2 then holds the BVH subtrees of its own image region.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t n) {
  const uint32_t q = n / 8u, r = n % 8u, xcd = b % 8u;
  return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + b / 8u;
}

// A persistent launch's n squares in eight contiguous shares, one per XCD: XCD x hands out [xcd_share_start, + xcd_share_size).
__host__ __device__ inline uint32_t xcd_share_size(uint32_t n, uint32_t xcd) { return n / 8u + (xcd < n % 8u ? 1u : 0u); }
__host__ __device__ inline uint32_t xcd_share_start(uint32_t n, uint32_t xcd) {
  const uint32_t q = n / 8u, r = n % 8u;
  return xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
}
// The indices a persistent wave takes from a long queue with one atomic (render_kernel_body).  Measured on the 1 M-triangle wall at
// 4K, 16 frames: 2 is 0.2-0.3 ms faster than 1; 8 (a whole square) is 2.3 ms slower -- the launch's last items then run one
// after the other in a few waves.
constexpr uint32_t kClaimPair = 2u;
// The squares of XCD x's share that the camera-hit pass walks (lt_camera_hits_kernel): all but its head squares, which the render
// launches walk themselves.  (ensure_square_order puts at most the share at its head.)
__host__ __device__ inline uint32_t camera_hit_squares(const FrameParams& fp, uint32_t xcd) {
  return xcd_share_size(fp.totalSquares, xcd) - (fp.order ? fp.orderHead[xcd] : 0u);
}

// Pixel of this lane in square b: false outside the image or the call's tiles.
__device__ __forceinline__ bool square_pixel(const FrameParams& fp, uint32_t b, uint32_t& x, uint32_t& y, uint32_t& pix) {
  const uint32_t k = b / fp.blocksPerTile, sb = b % fp.blocksPerTile;
  const uint32_t sbx = sb % fp.blocksPerTileX, sby = sb / fp.blocksPerTileX;
  const uint32_t tile = fp.tileFirst + k * fp.tileStride;
  const uint32_t tx = tile % fp.tilesX, ty = tile / fp.tilesX;
  const uint32_t lane = threadIdx.x;
  const uint32_t lx = sbx * 8u + (lane & 7u), ly = sby * 8u + (lane >> 3);
  x = tx * fp.tileW + lx;
  y = ty * fp.tileH + ly;
  pix = (k * fp.tileH + ly) * fp.tileW + lx;
  return k < fp.tilesInCall && lx < fp.tileW && ly < fp.tileH && x < fp.width && y < fp.height;
}

// One 8x8 pixel square (logical index b, already XCD-ordered) by one wavefront.
// (pos: the square's position in the hand-out order -- what a queued shadow ray's slot is made of, SceneDev::shadowPackets == 3;
// hitRow: the square's stored camera hits, FrameParams::cameraHits, or null; frames: 2 for a work item of two frames, frame and
// frame + 1, of accumulator over stored hits -- FrameParams::shadowFrames -- else 1; cut: the square's entry cut, FrameParams::entryCuts,
// or null; folding: the item is a frame group of a square handed out whole whose samples are not stored -- FrameParams::foldMap -- but
// folded by the wave itself, frame by frame in frame order, into the running mean at fp.foldOut: the wave runs the square's groups
// one after the other, so between them the mean waits in the words it ends up in, which no one else touches during the launch)
template <int PROGRAM, class CFG>
__device__ __forceinline__ void render_square(const SceneDev& sc, const FrameParams& fp, float* __restrict__ out, uint32_t b,
                                              uint32_t frame, uint32_t frames, Stack<CFG::kDeep>& st, Counters& c, uint32_t pos,
                                              const uint4* hitRow, const uint32_t* cut, bool folding) {
  constexpr bool STATS = CFG::kStats;
  const bool fold = PROGRAM == kAccumulator && CFG::kGroups && CFG::kItems && !STATS && folding;
  const uint32_t k = b / fp.blocksPerTile, sb = b % fp.blocksPerTile;
  const uint32_t sbx = sb % fp.blocksPerTileX, sby = sb / fp.blocksPerTileX;
  const uint32_t tile = fp.tileFirst + k * fp.tileStride;
  const uint32_t tx = tile % fp.tilesX, ty = tile / fp.tilesX;
  const uint32_t lane = threadIdx.x;
  const uint32_t lx = sbx * 8u + (lane & 7u);
  const uint32_t ly = sby * 8u + (lane >> 3);
  const uint32_t x = tx * fp.tileW + lx, y = ty * fp.tileH + ly;
  const bool valid = k < fp.tilesInCall && lx < fp.tileW && ly < fp.tileH && x < fp.width && y < fp.height;
  constexpr bool queueing = PROGRAM == kAccumulatorQueue;
  const uint32_t qslot = (pos * fp.fusedFrames + frame) * (uint32_t)kBlock + lane;
  bool queued = false;
  // A head square's item of the call's first frame keeps what its camera walk finds (FrameParams::storeHeadHits): all 64 slots, as
  // camera_hit_square writes them.  Its other frames' items do not wait for that: they walk as before.
  uint4* storeRow = nullptr;
  if constexpr ((PROGRAM == kAccumulator || PROGRAM == kAccumulatorQueue) && !STATS)
    if (fp.storeHeadHits && hitRow == nullptr && frame == 0u && fp.cameraHits != nullptr) storeRow = fp.cameraHits + (size_t)pos * kBlock;
  if (storeRow != nullptr && !valid) storeRow[lane] = make_uint4(0u, 0u, 0u, 0u);
  if (valid) {
    Counters pc{};   // this pixel's own counters (diagnostic output), folded into the lane's totals below
    const uint32_t pixel = (k * fp.tileH + ly) * fp.tileW + lx;
    const size_t first = (((size_t)k * fp.tileH + ly) * fp.tileW + lx) * fp.depth;
    float* o = out + (size_t)frame * fp.frameStride + first;
    auto store = [&](uint32_t f, const V3& color) {   // the colour of frame f of the launch
      // (a folded frame: lt_running_mean4_kernel's step on the mean itself, n = foldBase + f)
      float* d = fold ? fp.foldOut + first : o + (size_t)(f - frame) * fp.frameStride;
      const int32_t n = fold ? fp.foldBase + (int32_t)f : fp.accumulateN;
      if (n <= 0) {   // overwrite, or first frame of a running mean (`if (frameCount > 0)` guard)
        d[0] = color.x; d[1] = color.y; d[2] = color.z;
      } else {        // accumulator.frag:12-18: (c + acc*n) / (n+1)
        d[0] = running_mean_step(d[0], color.x, n);
        d[1] = running_mean_step(d[1], color.y, n);
        d[2] = running_mean_step(d[2], color.z, n);
      }
    };
    bool grouped = false;
    if constexpr (PROGRAM == kAccumulator && CFG::kGroups && !STATS) {
      if (frames > 1u) {
        V3 color[2];
        grouped = shade_pixel2<CFG>(sc, fp, fp.frameCount + frame, (int)x, (int)y, st, c, hitRow, color, cut);
        if (grouped) {
          store(frame, color[0]);
          store(frame + 1u, color[1]);
        }
      }
    }
    if constexpr (PROGRAM == kAccumulator && CFG::kGroups && !STATS) {
      // one frame at a time: every item of one frame, and the lanes of a group whose shadow rays could not walk together (a loop the
      // compiler keeps: one inlined copy of shade_pixel and its walks)
#pragma unroll 1
      for (uint32_t f = frame; !grouped && f < frame + frames; f++)
        store(f, shade_pixel<PROGRAM, CFG>(sc, fp, fp.frameCount + f, (int)x, (int)y, st, c, qslot, pixel, f, queued, hitRow, storeRow));
    } else {
      const V3 color = shade_pixel<PROGRAM, CFG>(sc, fp, fp.frameCount + frame, (int)x, (int)y, st, STATS ? pc : c, qslot, pixel, frame, queued, hitRow, storeRow);
      if (STATS && fp.pixelCounters) {
        o[0] = (float)pc.rays; o[1] = (float)pc.shadow; o[2] = (float)pc.nodes; o[3] = (float)pc.tris;
      } else {
        store(frame, color);
      }
    }
    if (STATS) {
      c.rays += pc.rays; c.shadow += pc.shadow; c.nodes += pc.nodes; c.tris += pc.tris;
#ifdef LT_DEBUG_WAVE_COUNTERS
      c.wInner += pc.wInner; c.wTri += pc.wTri; c.wOuter += pc.wOuter;
#endif
    }
  }
  // (every slot of the square says what it holds -- all 16 bytes of it: a wave's dwords 16 bytes apart would be sixteen
  // partly written lines instead of four whole ones)
  if (queueing && !queued) ((uint4*)sc.shadowQueue)[2 * (size_t)sc.shadowCap + qslot] = make_uint4(kDeadSlot, 0u, 0u, 0u);
}

// A clear square handed out whole (lt_entry_cut.hpp: kItemWhole; the square b at hand-out position pos, its hits stored), all its
// two-frame groups in one pass: what render_square -> shade_pixel2 -> shade_lighting2 -> traverse_shadow2 evaluate for each group
// over again is evaluated once per square -- the pixel, fx / fy, the stored hit, what kind of lane it is, position, normal and
// diffuse colour, the cut's word 0 -- and a group draws two new randoms, its other two being the group before's last two (frame s
// draws seeds s, s + 1, s + 2: a launch of 16 frames has 18 seeds per pixel, not 32).  With `fold` the running mean waits in three
// registers from the first group to the last instead of going through fp.foldOut twice per group.  Every value is the expression
// the per-group path evaluates, in its flavour and order; no walk is called here, so nothing of this is live across one.
// Returns the first frame group it did NOT render, `groups` when none is left: a group whose frames would not have walked together
// (shadow_frames_walk_together: render_square then renders them apart), one with a light sample off the light list, a trailing group
// of one frame, all of them where the cut's word 0 is no clear mark.  render_kernel_body goes on from that group as it always did.
// count: [0] squares that got past the mark, [1] those of them that left before their last group, [2] groups rendered here.
template <class CFG>
__device__ __forceinline__ uint32_t render_clear_square(const SceneDev& sc, const FrameParams& fp, float* __restrict__ out, uint32_t b, uint32_t pos,
                                                        uint32_t groups, bool fold, uint32_t (&count)[3]) {
  if (*(const __attribute__((address_space(4))) uint32_t*)(unsigned long long)(fp.entryCuts + (size_t)pos * lt_entry_cut::kListWords) != kEntryCutClear) return 0u;
  count[0]++;
  const uint32_t k = b / fp.blocksPerTile, sb = b % fp.blocksPerTile;
  const uint32_t sbx = sb % fp.blocksPerTileX, sby = sb / fp.blocksPerTileX;
  const uint32_t tile = fp.tileFirst + k * fp.tileStride;
  const uint32_t tx = tile % fp.tilesX, ty = tile / fp.tilesX;
  const uint32_t lane = threadIdx.x;
  const uint32_t lx = sbx * 8u + (lane & 7u);
  const uint32_t ly = sby * 8u + (lane >> 3);
  const uint32_t x = tx * fp.tileW + lx, y = ty * fp.tileH + ly;
  const bool valid = k < fp.tilesInCall && lx < fp.tileW && ly < fp.tileH && x < fp.width && y < fp.height;
  const size_t first = (((size_t)k * fp.tileH + ly) * fp.tileW + lx) * fp.depth;   // (the pixel's first float, as render_square makes it)
  // once per square: the lane's kind (a light: (1, 1, 1) in every frame; no surface: black; else shaded), and a shaded lane's
  // position, normal and diffuse colour (shade_lighting2's expressions on the same stored hit)
  bool shaded = false;
  float flat = 0.0f;   // the colour of a lane that is not shaded, every channel of every frame
  float fx = 0.0f, fy = 0.0f;
  V4 position = mk4(0.0f, 0.0f, 0.0f, 1.0f), normal = mk4(0.0f, 0.0f, 0.0f, 0.0f);
  V3 diffuse{0.0f, 0.0f, 0.0f};
  if (valid) {
    (void)camera_ray<CFG::kDevLibm>(fp, (int)x, (int)y, fx, fy);
    const uint4 h = (fp.cameraHits + (size_t)pos * kBlock)[__lane_id()];
    const int prim = (int)h.x;
    if (is_light(sc.lights, prim)) flat = 1.0f;
    else shaded = (int)h.y == 1;
    if (shaded) {
      const float* pr = prim_ptr(sc, prim);
      const V3 bc = barycentrics(__uint_as_float(h.z), __uint_as_float(h.w));
      const V3 p3 = bary3<CFG::kDevLibm>(pr + 0, pr + 3, pr + 6, bc);
      position = mk4(p3.x, p3.y, p3.z, 1.0f);
      const V3 n3 = bary3<CFG::kDevLibm>(pr + 9, pr + 12, pr + 15, bc);
      normal = mk4(n3.x, n3.y, n3.z, 0.0f);
      const Material* m = sc.mats + prim_material(pr);
      diffuse = V3{m->diffuse[0], m->diffuse[1], m->diffuse[2]};
    }
  }
  const bool anyShaded = __builtin_amdgcn_ballot_w64(shaded) != 0ull;
  float mean[3] = {0.0f, 0.0f, 0.0f};
  if (fold && valid) {
    const float* d = fp.foldOut + first;
    mean[0] = d[0]; mean[1] = d[1]; mean[2] = d[2];
  }
  // (the sample of frame f of the launch: render_square's store, with the mean in `mean` where it folds)
  auto store = [&](uint32_t f, const V3& color) {
    if (fold) {
      const int32_t n = fp.foldBase + (int32_t)f;
      mean[0] = running_mean_step(mean[0], color.x, n);
      mean[1] = running_mean_step(mean[1], color.y, n);
      mean[2] = running_mean_step(mean[2], color.z, n);
    } else {
      float* d = out + (size_t)f * fp.frameStride + first;
      const int32_t n = fp.accumulateN;
      if (n <= 0) {
        d[0] = color.x; d[1] = color.y; d[2] = color.z;
      } else {
        d[0] = running_mean_step(d[0], color.x, n);
        d[1] = running_mean_step(d[1], color.y, n);
        d[2] = running_mean_step(d[2], color.z, n);
      }
    }
  };
  const uint32_t full = fp.fusedFrames / 2u;   // the groups of two frames; one frame left over is the general path's
  float carried[2] = {0.0f, 0.0f};             // the randoms of the two seeds a group shares with the next
  uint32_t g = 0u;
  // pass `it` draws seeds 2 * it and 2 * it + 1 past the launch's first -- pass 0 nothing else -- and renders group it - 1 with them and
  // the two of the pass before: one copy of random()'s code
#pragma unroll 1
  for (uint32_t it = 0u; it <= full; it++) {
    bool together = false;
    float ndotl[2] = {0.0f, 0.0f};
    if (shaded) {
      float rnd[4];
      rnd[0] = carried[0];
      rnd[1] = carried[1];
      // (behind the opaque wave-uniform branch of shade_lighting2, for its reason: the sine's coefficients are made where they are used)
      uint32_t opaque = sc.shadowPackets;
      asm volatile("" : "+s"(opaque));
      const uint32_t s = fp.frameCount + 2u * it;
      if (opaque == 0xffffffffu) {
#pragma unroll
        for (int i = 0; i < 2; i++) rnd[2 + i] = __uint_as_float(opaque + (uint32_t)i);
      } else {
        const float seed[2] = {(float)s, (float)(s + 1u)};
        float drawn[2];
        randoms_<CFG::kDevLibm, 2>(fx, fy, seed, drawn);
        rnd[2] = drawn[0];
        rnd[3] = drawn[1];
      }
      carried[0] = rnd[2];
      carried[1] = rnd[3];
      if (it != 0u) {
        V4 lightPosition[2];
        bool listed = true;
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const float* lp = light_prim(sc, rnd[j]);
          // (off the list only where random() returns exactly 1.0 -- index == count -- or the list is empty: no pixel and frame of
          // the tests draws that, so the term of `together` below that reads `listed` is the one line here no test reaches)
          listed = listed && light_index_listed(sc, rnd[j]);
          float uvx = rnd[j + 1], uvy = rnd[j + 2];
          if (uvx + uvy > 1.0f) {
            uvx = 1.0f - uvx;
            uvy = 1.0f - uvy;
          }
          const V3 l3 = bary3<CFG::kDevLibm>(lp + 0, lp + 3, lp + 6, barycentrics(uvx, uvy));
          lightPosition[j] = mk4(l3.x, l3.y, l3.z, 1.0f);
        }
        asm volatile("" ::: "memory");
        Ray ray[2];
        float tmax[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const V4 toLight = normalize4<CFG::kDevLibm>(sub4(lightPosition[j], position));
          tmax[j] = (float)((double)distance4<CFG::kDevLibm>(position, lightPosition[j]) - 0.01);
          ndotl[j] = dot4(toLight, normal);
          ray[j] = Ray{position, toLight};
        }
        asm volatile("" : "+v"(ndotl[0]), "+v"(ndotl[1]));
        float inv[2][3];
        uint32_t form;
        unsigned long long all;
        together = shadow_frames_walk_together(sc, ray, tmax, all, inv, form) && __builtin_amdgcn_ballot_w64(!listed) == 0ull;
      }
    }
    if (it == 0u) continue;
    if (anyShaded && __builtin_amdgcn_ballot_w64(together) == 0ull) break;
    if (valid) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        V3 color = shaded ? V3{diffuse.x * ndotl[j], diffuse.y * ndotl[j], diffuse.z * ndotl[j]} : V3{flat, flat, flat};
        if (fp.clampOutput) color = V3{Math<CFG::kDevLibm>::clamp01(color.x), Math<CFG::kDevLibm>::clamp01(color.y), Math<CFG::kDevLibm>::clamp01(color.z)};
        store(2u * (it - 1u) + (uint32_t)j, color);
      }
    }
    g = it;
    count[2]++;
  }
  if (fold && valid && g != 0u) {
    float* d = fp.foldOut + first;
    d[0] = mean[0]; d[1] = mean[1]; d[2] = mean[2];
  }
  if (g != groups) count[1]++;
  return g;
}

// The camera-hit pass's work on one square: the walk of render_square's camera rays (same lanes, same walk: kAccumulator's and
// kAccumulatorQueue's are one), the hits stored for every frame's render_square.  All 64 slots are written: four whole lines.
template <class CFG>
__device__ __forceinline__ void camera_hit_square(const SceneDev& sc, const FrameParams& fp, uint32_t b, uint32_t pos, Stack<CFG::kDeep>& st, Counters& c) {
  uint32_t x, y, pix;
  Hit pl{0, 0, kFltMax, 0.0f, 0.0f};
  if (square_pixel(fp, b, x, y, pix)) {
    float fx, fy;
    const Ray ray = camera_ray<CFG::kDevLibm>(fp, (int)x, (int)y, fx, fy);
    pl = camera_hit<kAccumulator, CFG>(sc, ray, nullptr, st, c);
  }
  fp.cameraHits[(size_t)pos * kBlock + threadIdx.x] = make_uint4((uint32_t)pl.prim, (uint32_t)pl.hitType, __float_as_uint(pl.u), __float_as_uint(pl.v));
}

// Registers: the traversal wants every wave slot (8 per SIMD = 64 VGPRs); the single-bounce programs fit that with a few
// spilled values in their shading code; the 16-bounce / 25-sample programs as ONE kernel would spill 85-140 values at 8 and
// run best at 5 waves per SIMD (Cornell GI 1080p, 16 bounces, 16 frames per launch: 31.5 / 30.2 / 32.8 / 45.7 ms at
// 4 / 5 / 6 / 8); the stage kernels of the wavefront GI pipeline hold one ray's state and take 8 (1 M-triangle wall, 4K,
// 16 frames: 498 / 432 / 395 / 363 ms at 4 / 5 / 6 / 8; Cornell 24.0 -> 24.9 ms).  basic_lighting (one shadow ray, 25 samples
// per pixel) sides with the single-bounce programs: 8 waves are +9 % (blob) / +13 % (wall) over 5.
#ifndef LT_GI_WAVES
#define LT_GI_WAVES 5
#endif
#ifndef LT_GI_STAGE_WAVES
#define LT_GI_STAGE_WAVES 8
#endif
#ifndef LT_ACC_WAVES
#define LT_ACC_WAVES 8
#endif
constexpr int waves_per_simd(int program) { return (program == kGI || program == kGI25) ? LT_GI_WAVES : LT_ACC_WAVES; }

// HITS: the camera-hit pass (lt_camera_hits_kernel): every square of the XCDs' shares but their head squares, once, through
// camera_hit_square, in the order and on the XCD that the render launches give them.  (The head squares' slots are filled by the
// first render launch behind the pass: render_square, FrameParams::storeHeadHits.)
template <int PROGRAM, class CFG, bool HITS = false>
__device__ __forceinline__ void render_kernel_body(const SceneDev& sc, const FrameParams& fp, float* __restrict__ out,
                                                   unsigned long long* __restrict__ stats, uint32_t* __restrict__ queues) {
  extern __shared__ int lds_stack[];   // [BVH height (<= kLdsStack)][kBlock], sized by the launch
  constexpr bool STATS = CFG::kStats;
  Stack<CFG::kDeep> st;
  st.lds = lds_stack + threadIdx.x;
  st.rows = (int)fp.ldsRows;
  Counters c{};

  // Two ways to hand out the 8x8 squares, one loop (a single inlined copy of the renderer):
  //  * one square per workgroup, the hardware dispatcher doing the scheduling (workgroup ids remapped per XCD);
  //  * persistent wavefronts: a grid just large enough to fill the chip, every wave pulling squares from the queue of the
  //    XCD it runs on (its contiguous share of the logical square list, so each XCD's L2 keeps serving one image region)
  //    and, when that is drained, from the other XCDs' queues.  Every wave reaches the exit: each queue hands out at most
  //    its share, and the loop ends after one empty sweep over all eight.
  const uint32_t home = fp.persistent ? (__builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u) : 0u;   // HW_REG_XCC_ID
  uint32_t sweep = 0;
  uint32_t claimed = 0, claimedLeft = 0;   // a claim of two indices: the next one, and how many of the claim are left (below)
  // An entry of the item table that stands for a whole square (FrameParams::itemTable): the wave runs the square's frame groups one
  // after the other, through this same loop.  One word of state, so that the walks keep their registers: the index of the square's
  // next group (never 0; a multiple of the groups per square when none is left), and in bit 31 whether its samples are folded
  // (render_square: fold).  0: no whole square in hand.
  uint32_t wholeNext = 0u;
  // ... and the kernel of the item table renders such a square's two-frame groups in one pass (render_clear_square): what this wave
  // saw of that, in three scalars, added to the launch's counters when the wave ends (kClearCountAt)
  constexpr bool kClearSquare = PROGRAM == kAccumulator && CFG::kGroups && CFG::kItems && !STATS && !HITS;
  uint32_t clearCount[3] = {0u, 0u, 0u};
  uint32_t tableLimit = 0u, tableSweep = 8u;   // the length of the queue's share of the table, loaded once per sweep (8: none yet)
  auto sload = [](const uint32_t* p) { return *(const __attribute__((address_space(4))) uint32_t*)(unsigned long long)p; };
  bool done = false;
  while (!done) {
    uint32_t b, frame = 0, frames = 1, pos = 0;
    bool stored = false;   // the item's camera hits are in fp.cameraHits
    bool folding = false;  // the item's samples are folded into the running mean by the item itself (render_square)
    if (!fp.persistent) {
      b = xcd_remap(blockIdx.x, gridDim.x);
      pos = b;
      done = true;
    } else {
      const uint32_t xcd = (home + sweep) & 7u;
      const uint32_t share = xcd_share_size(fp.totalSquares, xcd), start = xcd_share_start(fp.totalSquares, xcd);
      const uint32_t head = fp.order ? fp.orderHead[xcd] : 0u;
      // accumulator's squares with stored hits come in work items of `group` consecutive frames (FrameParams::shadowFrames), the last
      // of a square shorter when the launch's frames are not a multiple of it: `groups` items per square
      const uint32_t group = PROGRAM == kAccumulator && CFG::kGroups && !STATS && !HITS && fp.cameraHits != nullptr && fp.shadowFrames >= 2u ? 2u : 1u;
      const uint32_t groups = (fp.fusedFrames + group - 1u) / group;
      // With an item table (FrameParams::itemTable; the host sets it for launches whose every square is stored, in square-major order,
      // and built for this many groups) a claim indexes the queue's share of the table, whose length is in device memory: one scalar
      // load per sweep.
      const bool table = PROGRAM == kAccumulator && CFG::kGroups && CFG::kItems && !STATS && !HITS && group == 2u && fp.itemTable != nullptr &&
                         item_groups(fp) == groups && fp.squareMajor != 0u && head == 0u;
      if (table && tableSweep != sweep) {
        tableLimit = sload(fp.itemTable + xcd);
        tableSweep = sweep;
      }
      // (head * fusedFrames + (share - head) * groups <= share * fusedFrames < 2^32: checked by the host)
      const uint32_t limit = table ? tableLimit : HITS ? camera_hit_squares(fp, xcd) : head * fp.fusedFrames + (share - head) * groups;
      // A claim is an atomic on one of eight addresses, and those complete one after the other, some 15 ns apart: the flagship
      // launch's 129 600 claims per queue are 1.9 ms of that, which the items' work only partly hides.  So a claim
      // takes TWO consecutive indices where the queue has more than four items per wave of the launch (kClaimPair), and the wave
      // renders them one after the other -- in square-major order two neighbouring frame groups of one square.  Every index below
      // `limit` is still handed out exactly once, the second of a pair that begins at limit - 1 to nobody.  A shorter queue stays
      // at one index per claim: with few items per wave the pairs lengthen the launch's end by more than the claims they save
      // (one frame at 4K, 16 items per wave: 1.97 ms with one index per claim, 2.11 with two).  (A counter ends at most two per
      // wave and queue above `limit`, which the host keeps below 2^30 or so: no wrap.)
      uint32_t t = 0;
      if (table && wholeNext != 0u) {   // the next frame group of a whole square: no claim
        folding = (wholeNext & lt_entry_cut::kItemWhole) != 0u;
        t = wholeNext & ~lt_entry_cut::kItemWhole;
        wholeNext = (t + 1u) % groups == 0u ? 0u : wholeNext + 1u;
      } else {
        if (claimedLeft == 0u) {
          // (A table's queue goes out in pairs only while more than half of what it could hold is in it: a queue that whole squares have
          // thinned out -- the flagship's hold 3 entries per square of 8, 0.7 ms of atomics under a launch of 4 ms -- ran 0.35 ms
          // slower in pairs, and one that is mostly single frame groups, as without a table, is as claim-bound as without one: the
          // Cornell box at 4K ran 0.5 ms slower with one entry per claim)
          const uint32_t take = limit / 4u > gridDim.x && (!table || limit / share > groups / 2u) ? kClaimPair : 1u;
          if (threadIdx.x == 0) t = atomicAdd(&queues[xcd * kQueueStride], take);
          claimed = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
          claimedLeft = take;
        }
        t = claimed++;
        claimedLeft--;
        if (t >= limit) {
          claimedLeft = 0u;
          done = ++sweep >= 8u;
          continue;
        }
        if (table) {   // the entry: the index the arithmetic below takes apart, and whether it stands for the whole square
          const uint32_t entry = sload(fp.itemTable + lt_entry_cut::kItemHeader + (size_t)start * groups + t);
          t = entry & ~lt_entry_cut::kItemWhole;
          if ((entry & lt_entry_cut::kItemWhole) != 0u) {
            // Folded where the fold map says so: the word lt_running_mean4_kernel skips the square's floats by (the byte of the square's
            // first row; its rows are marked alike).
            if (fp.foldMap != nullptr) {
              const uint32_t sq = fp.order ? sload(fp.order + start + t / groups) : start + t / groups;
              const uint32_t k = sq / fp.blocksPerTile, sb = sq % fp.blocksPerTile;
              const unsigned long long seg = lt_entry_cut::fold_segment(k, fp.tileH, fp.tileW, sb / fp.blocksPerTileX * 8u, sb % fp.blocksPerTileX);
              folding = (sload(fp.foldMap + (seg >> 2)) >> (8u * (uint32_t)(seg & 3ull)) & 0xffu) != 0u;
            }
            // The square's groups of two frames in one pass (render_clear_square), as far as they go: the loop takes the square up at
            // the first group that is left, as if it had rendered the ones before it.
            if constexpr (kClearSquare) {
              if (item_one_pass(fp) && sc.groupWalks == nullptr && fp.entryCuts != nullptr) {
                const uint32_t at = start + t / groups;
                const uint32_t rendered = render_clear_square<CFG>(sc, fp, out, fp.order ? sload(fp.order + at) : at, at, groups, folding, clearCount);
                if (rendered == groups) continue;
                t += rendered;
              }
            }
            wholeNext = (t + 1u) % groups == 0u ? 0u : (t + 1u) | (folding ? lt_entry_cut::kItemWhole : 0u);
          }
        }
      }
      stored = fp.cameraHits != nullptr && t >= head * fp.fusedFrames;
      // frame-major inside the XCD's share (every frame of a square stays on its XCD), the head squares of all frames first
      if (HITS) {
        t += head;
      } else if (t < head * fp.fusedFrames) {
        frame = t / head;
        t -= frame * head;
      } else if (fp.fusedFrames > 1u) {
        t -= head * fp.fusedFrames;
        uint32_t item;   // the item's frame group
        if (fp.squareMajor) {   // the frames of a square side by side: their rays meet the same nodes while those are in the L2
          item = t % groups;
          t = head + t / groups;
        } else {
          item = t / (share - head);
          t = head + (t - item * (share - head));
        }
        frame = item * group;
        frames = fp.fusedFrames - frame < group ? fp.fusedFrames - frame : group;
      }
      b = start + t;
      pos = b;
      if (fp.order) b = (uint32_t)__builtin_amdgcn_readfirstlane((int)fp.order[b]);
    }
    if (HITS) {
      camera_hit_square<CFG>(sc, fp, b, pos, st, c);
    } else {
      render_square<PROGRAM, CFG>(sc, fp, out, b, frame, frames, st, c, pos, stored ? fp.cameraHits + (size_t)pos * kBlock : nullptr,
                                  stored && fp.entryCuts != nullptr ? fp.entryCuts + (size_t)pos * lt_entry_cut::kListWords : nullptr, folding);
    }
  }
  if constexpr (kClearSquare) {
    if (clearCount[0] != 0u && threadIdx.x == 0u) {   // (only a persistent launch has a table: `queues` is set)
      unsigned long long* const at = (unsigned long long*)(queues + home * kQueueStride + kClearCountAt);
#pragma unroll
      for (int i = 0; i < 3; i++) atomicAdd(&at[i], (unsigned long long)clearCount[i]);
    }
  }
  if (STATS) {
    atomicAdd(&stats[0], (unsigned long long)c.rays);
    atomicAdd(&stats[1], (unsigned long long)c.shadow);
    atomicAdd(&stats[2], (unsigned long long)c.nodes);
    atomicAdd(&stats[3], (unsigned long long)c.tris);
#ifdef LT_DEBUG_WAVE_COUNTERS
    atomicAdd(&stats[4], (unsigned long long)c.wInner);
    atomicAdd(&stats[5], (unsigned long long)c.wTri);
    atomicAdd(&stats[6], (unsigned long long)c.wOuter);
#endif
  }
}

template <int PROGRAM, class CFG>
__global__ __launch_bounds__(kBlock, waves_per_simd(PROGRAM)) void lt_render_kernel(SceneDev sc, FrameParams fp, float* __restrict__ out,
                                                          unsigned long long* __restrict__ stats, uint32_t* __restrict__ queues) {
  render_kernel_body<PROGRAM, CFG>(sc, fp, out, stats, queues);
}

// The camera-hit pass of a call (FrameParams::cameraHits; lt_capi.hip: render_on_stream).  Same scheduling as the render launches
// it serves, so that a square's hits are written through the L2 of the XCD that renders its frames.
template <class CFG>
__global__ __launch_bounds__(kBlock, LT_ACC_WAVES) void lt_camera_hits_kernel(SceneDev sc, FrameParams fp, uint32_t* __restrict__ queues) {
  render_kernel_body<kAccumulator, CFG, true>(sc, fp, nullptr, nullptr, queues);
}

// The entry cuts of stored camera hits (lt_entry_cut.hpp; FrameParams::entryCuts): one wave per square of the hand-out order,
// position blockIdx.x -- every square (all != 0: the hits are whole, a call that reuses them) or all but the head squares of fp's
// hand-out order (all == 0: behind a call's own camera-hit pass, whose render launches walk the head squares themselves).  A lane casts shadow rays iff its stored hit is a surface that is
// no light (shade_lighting2); the square's list starts as the root and the shallowest interior entry is replaced by those of its
// two children that some casting lane may reach (may_reach), until a replacement would make it longer than `chunks` records of
// `limit` (<= kCut) entries hold (lt_entry_cut.hpp: Chunks; chunk c at cuts[(c * totalSquares + pos) * 16]).  The empty list
// -- start at the root -- where the argument does not hold or nothing is gained: no light, a casting lane that lane_set refuses,
// no casting lane, a list that is the root alone or empty.  stats: [0] squares with a non-empty list, [1] their entries -- of the
// node cut, whatever the leaf pass below makes of the square; [2] squares the leaf pass marks clear, [3] squares it gives a list of
// leaves that fits one chunk, [4] the entries of those; [5], [6] the same for the lists of leaves that take several chunks; [7], [8]
// the squares whose list stays a node cut of several chunks, and its entries; [kEntryCutStatsChunks + k - 1] the squares whose
// list, of any kind, takes k chunks; [kEntryCutStatsPruned], [+ 1] the squares whose list is a cut over the pruned tree, and its entries.  leafBudget: the records the leaf pass may visit per square; 0: no leaf pass
// (LT_ENTRY_CUT_LEAVES=0).
constexpr uint32_t kEntryCutStatsChunks = 9u, kEntryCutStatsPruned = kEntryCutStatsChunks + (uint32_t)lt_entry_cut::kMaxChunks,
                   kEntryCutStats = kEntryCutStatsPruned + 2u;
template <class CFG>
__global__ __launch_bounds__(kBlock) void lt_entry_cut_kernel(SceneDev sc, FrameParams fp, uint32_t* __restrict__ cuts, uint32_t all,
                                                             uint32_t limit, unsigned long long* __restrict__ stats, uint32_t leafBudget, uint32_t chunks,
                                                             uint32_t nodeChunks) {
  using namespace lt_entry_cut;
  static_assert(kClearMark == kEntryCutClear && kClearMark > (unsigned)kCut, "traverse_shadow2 looks for the mark that this kernel writes; no count is one");
  static_assert(kMaxEntries + 2 <= 256, "the pick below keeps an entry's index in eight bits");
  static_assert((unsigned)kCut <= kEntryCutMaxCount, "packet_walk2 takes a further chunk's count for one only up to kEntryCutMaxCount");
  const uint32_t pos = blockIdx.x, lane = threadIdx.x;
  if (pos >= fp.totalSquares) return;
  bool head = false;
  for (uint32_t xcd = 0; xcd < 8u; xcd++) {
    const uint32_t start = xcd_share_start(fp.totalSquares, xcd);
    if (pos >= start && pos - start < xcd_share_size(fp.totalSquares, xcd)) head = fp.order != nullptr && pos - start < fp.orderHead[xcd];
  }
  if (head && all == 0u) return;
  if (limit > (uint32_t)kCut) limit = (uint32_t)kCut;
  chunks = chunks < 1u ? 1u : chunks > (uint32_t)kMaxChunks ? (uint32_t)kMaxChunks : chunks;
  const uint32_t cap = chunk_capacity(limit, chunks);   // the entries of a square's list at most: `chunks` records of `limit`
  const uint32_t nodeCap = chunk_capacity(limit, nodeChunks < chunks ? nodeChunks : chunks);   // ... and of a list of nodes
  __shared__ uint32_t refs[kMaxEntries + 2], depth[kMaxEntries + 2], leaves[kMaxEntries];
  // the light primitives' vertex box, pushed outwards
  const uint32_t nLights = sc.lights->count;
  float Llo[3], Lhi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { Llo[a] = __builtin_inff(); Lhi[a] = -__builtin_inff(); }
  if (lane < nLights && lane < 64u) {
    const float* lp = prim_ptr(sc, (int)sc.lights->primitives[lane]);
#pragma unroll
    for (int v = 0; v < 3; v++)
#pragma unroll
      for (int a = 0; a < 3; a++) {
        Llo[a] = __builtin_fminf(Llo[a], lp[3 * v + a]);
        Lhi[a] = __builtin_fmaxf(Lhi[a], lp[3 * v + a]);
      }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    for (int m = 32; m >= 1; m >>= 1) {
      Llo[a] = __builtin_fminf(Llo[a], __shfl_xor(Llo[a], m));
      Lhi[a] = __builtin_fmaxf(Lhi[a], __shfl_xor(Lhi[a], m));
    }
    light_box_pad(Llo[a], Lhi[a]);
  }
  // this lane's origin: shade_lighting2's `position`, the same operations on the same stored hit
  const uint32_t b = fp.order ? fp.order[pos] : pos;
  uint32_t x, y, pix;
  bool casts = false;
  int own = -1;   // the primitive this lane's rays start from
  LaneSet ls{};
  bool covered = true;
  if (square_pixel(fp, b, x, y, pix)) {
    const uint4 h = fp.cameraHits[(size_t)pos * kBlock + lane];
    if ((int)h.y == 1 && !is_light(sc.lights, (int)h.x)) {
      casts = true;
      own = (int)h.x;
      const float* pr = prim_ptr(sc, (int)h.x);
      const V3 p3 = bary3<CFG::kDevLibm>(pr + 0, pr + 3, pr + 6, barycentrics(__uint_as_float(h.z), __uint_as_float(h.w)));
      covered = lane_set(p3.x, p3.y, p3.z, Llo, Lhi, ls);
    }
  }
  uint32_t n = 0u;
  const bool build = nLights != 0u && nLights <= 64u && sc.ownPairs != nullptr && __builtin_amdgcn_ballot_w64(casts) != 0ull &&
                     __builtin_amdgcn_ballot_w64(casts && !covered) == 0ull;
  if (build) {
    if (lane == 0u) { refs[0] = 0u; depth[0] = 0u; }
    n = 1u;
    __syncthreads();
    const __attribute__((address_space(4))) char* const pairs = (const __attribute__((address_space(4))) char*)(unsigned long long)sc.ownPairs;
    for (;;) {
      // the shallowest interior entry, the first of several: the least (depth, index), a lane per entry and 64 entries a round
      uint32_t key = 0xffffffffu;
      for (uint32_t i = lane; i < n; i += 64u)
        if ((int)refs[i] >= 0 && (depth[i] << 8 | i) < key) key = depth[i] << 8 | i;
      for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)key, m);
        key = other < key ? other : key;
      }
      if (key == 0xffffffffu) break;
      const uint32_t pick = key & 255u;
      const F16v r = *(ConstF16)(pairs + ((size_t)refs[pick] << 6));
      const bool inL = __builtin_amdgcn_ballot_w64(casts && may_reach(ls, r.s0, r.s1, r.s2, r.s3, r.s4, r.s5)) != 0ull;
      const bool inR = __builtin_amdgcn_ballot_w64(casts && may_reach(ls, r.s8, r.s9, r.sa, r.sb, r.sc, r.sd)) != 0ull;
      const uint32_t kids = (inL ? 1u : 0u) + (inR ? 1u : 0u);
      if (n - 1u + kids > nodeCap) break;
      __syncthreads();
      if (lane == 0u) {
        const uint32_t d = depth[pick] + 1u;
        // (the picked entry's place goes to the last entry, the children to the end: the walk takes a list in any order)
        refs[pick] = refs[n - 1u]; depth[pick] = depth[n - 1u];
        uint32_t m = n - 1u;
        if (inL) { refs[m] = __float_as_uint(r.s6); depth[m] = d; m++; }
        if (inR) { refs[m] = __float_as_uint(r.se); depth[m] = d; m++; }
      }
      n = n - 1u + kids;
      __syncthreads();
      if (n == 0u) break;
    }
    if (n == 1u && refs[0] == 0u) n = 0u;   // the root alone
  }
  if (lane == 0u && n != 0u && stats != nullptr) {
    atomicAdd(&stats[0], 1ull);
    atomicAdd(&stats[1], (unsigned long long)n);
  }
  // The leaf pass: depth first from the root, a child where some casting lane may reach its box, a leaf where some casting lane that
  // does not start on it may reach its own box and may accept its triangle (may_accept).  The stack is wave-uniform and lives in one
  // register, a lane per slot (2 * height + 2 <= 62 slots: entry_cut_limit != 0); the surviving leaves go to LDS.  Finished within
  // leafBudget records and with at most `cap` leaves: those leaves are the square's list -- by the two claims no ray of the square
  // is accepted anywhere else -- and none at all is the clear mark.  Finished with more leaves than that, and within kPruneRecords
  // records: the pass has written down the tree as it saw it (the first kPruneRecords records it visits: each one's reference, the
  // record it came from and the records its children became; a second stack register carries where a waiting child came from), and
  // the list is a cut of that tree without the subtrees in which no leaf survived (lt_entry_cut.hpp: pruned_cut_select; lane 0
  // runs it).  Else the node cut above stays.
  __shared__ uint32_t seenRef[kPruneRecords];
  __shared__ unsigned short seenParent[kPruneRecords], seenKid[2 * kPruneRecords], cutEntry[kMaxEntries + 2];
  __shared__ unsigned char seenMark[kPruneRecords], cutDepth[kMaxEntries + 2];
  bool whole = false, pruned = false;
  uint32_t kept = 0u, prunedEntries = 0u;
  if (build && leafBudget != 0u) {
    const __attribute__((address_space(4))) char* const pairs = (const __attribute__((address_space(4))) char*)(unsigned long long)sc.ownPairs;
    int stackv = 0, stackFrom = 0;
    uint32_t sp = 0u, visited = 0u, cur = 0u, from = 0xffffffffu;   // from: 2 * (the record `cur` was reached from) + which child it is
    bool finished = true;
    for (;;) {
      if (++visited > leafBudget) { finished = false; break; }
      const uint32_t v = visited - 1u;
      if (v < (uint32_t)kPruneRecords && lane == 0u) {
        seenRef[v] = cur;
        seenParent[v] = from == 0xffffffffu ? kNoRecord : (unsigned short)(from >> 1);
        seenKid[2u * v] = seenKid[2u * v + 1u] = kNoRecord;
        seenMark[v] = 0;
        if (from != 0xffffffffu) seenKid[from] = (unsigned short)v;
      }
      const F16v r = *(ConstF16)(pairs + (size_t)(cur << 6));
      if ((int)cur >= 0) {
        const bool inL = __builtin_amdgcn_ballot_w64(casts && may_reach(ls, r.s0, r.s1, r.s2, r.s3, r.s4, r.s5)) != 0ull;
        const bool inR = __builtin_amdgcn_ballot_w64(casts && may_reach(ls, r.s8, r.s9, r.sa, r.sb, r.sc, r.sd)) != 0ull;
        if (sp + 2u > 64u) { finished = false; break; }
        if (inR) { stackv = lane == sp ? __float_as_int(r.se) : stackv; stackFrom = lane == sp ? (int)(2u * v + 1u) : stackFrom; sp++; }
        if (inL) { stackv = lane == sp ? __float_as_int(r.s6) : stackv; stackFrom = lane == sp ? (int)(2u * v) : stackFrom; sp++; }
      } else {
        const bool may = casts && own != __float_as_int(r.sf) && may_reach(ls, r.s9, r.sa, r.sb, r.sc, r.sd, r.se) &&
                         may_accept(ls, r.s0, r.s1, r.s2, r.s3, r.s4, r.s5, r.s6, r.s7, r.s8);
        if (__builtin_amdgcn_ballot_w64(may) != 0ull) {
          if (kept < cap && lane == 0u) leaves[kept] = cur;
          if (v < (uint32_t)kPruneRecords && lane == 0u) pruned_mark(seenParent, seenMark, v);
          kept++;   // (beyond cap: counted, not kept -- the pass goes on to see the whole tree)
        }
      }
      if (sp == 0u) break;
      --sp;
      cur = (uint32_t)__builtin_amdgcn_readlane(stackv, (int)sp);
      from = (uint32_t)__builtin_amdgcn_readlane(stackFrom, (int)sp);
    }
    whole = finished && kept <= cap;
    pruned = finished && kept > cap && visited <= (uint32_t)kPruneRecords && cap >= 2u;
    if (pruned) {
      __syncthreads();
      uint32_t count = 0u;
      if (lane == 0u) count = pruned_cut_select(seenRef, seenKid, seenMark, cap, cutEntry, cutDepth, leaves);
      prunedEntries = (uint32_t)__builtin_amdgcn_readfirstlane((int)count);
    }
  }
  __syncthreads();
  // The square's list -- the surviving leaves, the cut over the pruned tree, else the node cut -- in chunks of `limit`: chunk c in
  // plane c, a count and that many references.  Every plane's record is written, whatever the list: a count of 0 where it has
  // ended (or never began).
  const uint32_t* const list = whole || pruned ? leaves : refs;
  const uint32_t entries = whole ? kept : pruned ? prunedEntries : n;
  for (uint32_t c = 0; c < chunks; c++) {
    const uint32_t count = chunk_entries(entries, limit, c);
    const uint32_t word0 = c == 0u && whole && kept == 0u ? kClearMark : count;
    if (lane < (uint32_t)kListWords)
      cuts[((size_t)c * fp.totalSquares + pos) * kListWords + lane] = lane == 0u ? word0 : lane <= count ? list[c * limit + lane - 1u] : 0u;
  }
  if (lane == 0u && stats != nullptr) {
    const uint32_t used = chunk_count(entries, limit);
    if (whole && kept == 0u) atomicAdd(&stats[2], 1ull);
    else if (whole && used == 1u) { atomicAdd(&stats[3], 1ull); atomicAdd(&stats[4], (unsigned long long)kept); }
    else if (whole) { atomicAdd(&stats[5], 1ull); atomicAdd(&stats[6], (unsigned long long)kept); }
    else if (pruned) { atomicAdd(&stats[kEntryCutStatsPruned], 1ull); atomicAdd(&stats[kEntryCutStatsPruned + 1u], (unsigned long long)prunedEntries); }
    else if (used > 1u) { atomicAdd(&stats[7], 1ull); atomicAdd(&stats[8], (unsigned long long)n); }
    if (used != 0u) atomicAdd(&stats[kEntryCutStatsChunks + used - 1u], 1ull);
  }
}

// =====================================================================================================================
// Wavefront pipeline for the global-illumination programs (gi.cl:241-375): the 16-bounce loop of `shade` as one kernel per
// stage with ACTIVE-PATH COMPACTION between stages, instead of one lane carrying a pixel through up to 34 rays while its
// neighbours idle (a path ends at the first occluded light sample or miss; on the Cornell box the mean is 3.9 rays per pixel,
// the maximum 34).
//   lt_gi_primary_kernel : camera ray, direct term, first extension ray      -> appends the surviving paths to queue 0
//   lt_gi_bounce_kernel  : extension ray d of every path in queue d, light sample + shadow ray, indirect term d
//                                                                             -> appends the surviving paths to queue d+1
//   lt_gi_resolve_kernel : direct + indirect, the 25-sample blend of the resources/ variant, clamp, running mean, store
// Queues are structure-of-float4 arrays in HBM (64 bytes per path: origin+film.x, direction, previous normal, {pixel,
// previous primitive, film.y}); a wave appends with one atomic: ballot of the surviving lanes, popcount, prefix count
// (mbcnt) for each lane's slot.  All kernels are persistent: a chip-filling grid whose waves pull work (8x8 squares from
// per-XCD queues / 64-path chunks) with an atomic, the queue length being read from device memory, so the host never waits
// between stages.  Per pixel the arithmetic and its order are those of the reference loop: the indirect sum receives its
// terms in depth order, and a path that hits a light adds the terms of all remaining depths at once (the reference
// re-traces the identical ray each time: same hit, same term).  Used when work is not being counted; the counting variants
// run the one-lane-per-pixel kernel, which re-traces like the reference does.
struct GiQueue { float4* o; float4* d; float4* n; uint4* m; };
constexpr uint32_t kDeadPath = kDeadSlot;    // m.x of a slot of a direct-mapped queue that holds no path

struct GiParams {
  GiQueue q[2];            // ping-pong: stage d reads q[d & 1], writes q[(d + 1) & 1]
  float4* direct;          // per pixel (compact output index): direct colour
  float4* indirect;        // per pixel: indirect sum so far
  float4* blend;           // per pixel: running blend of the 25-sample variant (between chunks of its samples)
  uint32_t* counts;        // [maxDepth + 1] queue lengths, kQueueStride dwords apart (one cache line per counter)
  uint32_t* work;          // [maxDepth + 1] chunk counters of the bounce launches, likewise
  uint32_t sample;         // sampleIndex passed to shade (frameCount, or frameCount*32 + k) of the launch's first frame
  uint32_t raw;            // != 0: the resolve stage stores direct + indirect as is (25-sample variant: lt_gi_blend25_kernel
                           // blends, clamps and accumulates afterwards); 0: it clamps (the frame's own colour is final)
  // Several frames per set of launches (FrameParams::fusedFrames of them; for the 25-sample variant the "frames" are the
  // samples k of one frame): frame f uses sample + f, its pixels live at [f * pixels, (f + 1) * pixels) of direct / indirect,
  // and every path carries its frame (m.w).
  uint32_t pixels;         // compact output pixels of one frame
  uint32_t ldsRows;        // rows of each wave's LDS stack (the stage kernels with several waves per workgroup need it)
  // The extension rays of a stage traced ahead of it by lt_trace_kernel (below): hits[e] = (primitive, hitType, u, v) of path e
  // of the stage's queue, or null when the stage traces them itself (small LDS-resident scenes; scenes without an own tree).
  const uint4* hits;
  // ... and then the stage runs as three kernels with a compacted list between them instead of one (below): the paths whose
  // extension ray hit a surface (hitList, hitCount), their light samples and shadow rays (so = position + tmax, sd = direction,
  // sm = (path, primitive, n.l), sn = normal), which lt_trace_kernel walks as any-hit rays (their fate: `occluded`, by list entry).
  // Queue 0 is then not appended to but DIRECT-MAPPED: the path of lane l of square p (position in the XCD-contiguous square
  // list) and frame f sits at slot (p * frames + f) * 64 + l, dead slots (no surface hit, pixel outside the image) marked by
  // m.x = kDeadPath.  No atomic in the camera stage (its 2 M appends to one counter were a 12 ns queue of their own), and the
  // queue is in the squares' order: an eighth of it is an eighth of the image, which lt_trace_kernel hands to one XCD.
  uint32_t directQueue;
  uint32_t* hitList;
  uint32_t* hitCount;      // [maxDepth + 1], kQueueStride dwords apart
  float4* so; float4* sd; uint4* sm; float4* sn;
  const uint32_t* occluded;   // [i of the list] != 0: the shadow ray met something
};

// one atomic per wave: slot of this lane among the lanes with `keep`
__device__ __forceinline__ uint32_t wave_append(uint32_t* counter, bool keep) {
  const unsigned long long m = __ballot(keep);
  if (m == 0ull) return 0u;
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if ((int)__lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
  return base + (uint32_t)__popcll(m & ((1ull << __lane_id()) - 1ull));
}

template <class CFG>
__global__ __launch_bounds__(kBlock, LT_GI_STAGE_WAVES) void lt_gi_primary_kernel(SceneDev sc, FrameParams fp, GiParams gp, uint32_t* __restrict__ queues) {
  extern __shared__ int lds_stack[];
  Stack<CFG::kDeep> st;
  st.lds = lds_stack + threadIdx.x;
  st.rows = (int)fp.ldsRows;
  Counters c{};
  const uint32_t n = fp.totalSquares, q = n / 8u, r = n % 8u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;
  if (gp.directQueue && blockIdx.x == 0 && threadIdx.x == 0) gp.counts[0] = n * fp.fusedFrames * (uint32_t)kBlock;   // (read by the launches behind this one)
  for (uint32_t sweep = 0; sweep < 8u;) {
    const uint32_t xcd = (home + sweep) & 7u;
    const uint32_t share = q + (xcd < r ? 1u : 0u), start = xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    uint32_t t = 0;
    if (threadIdx.x == 0) t = atomicAdd(&queues[xcd * kQueueStride], 1u);
    t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    if (t >= share * fp.fusedFrames) { sweep++; continue; }
    const uint32_t frame = t / share;   // frame-major inside the XCD's share
    t -= frame * share;
    uint32_t x, y, pix;
    const bool valid = square_pixel(fp, start + t, x, y, pix);
    pix += frame * gp.pixels;
    bool alive = false;
    V4 position{}, normal{}, dir{};
    float fx = 0.0f, fy = 0.0f;
    int prim = 0;
    if (valid) {
      const Ray ray = camera_ray<CFG::kDevLibm>(fp, (int)x, (int)y, fx, fy);
      const uint32_t s = gp.sample + frame;
      V3 direct{0.0f, 0.0f, 0.0f};
      Hit pl{0, 0, kFltMax, 0.0f, 0.0f};
      traverse_camera<kGI, CFG::kDeep, false>(sc, ray, pl, st, c);
      if (is_light(sc.lights, pl.prim)) {
        direct = V3{1.0f, 1.0f, 1.0f};
      } else if (pl.hitType == 1) {
        const float* pr = prim_ptr(sc, pl.prim);
        const Material* m = sc.mats + prim_material(pr);
        float ndotl;
        if (direct_light<kGIPrimary, CFG>(sc, pr, pl.prim, pl.u, pl.v, fx, fy, (float)s, (float)(s + 1u), (float)(s + 2u), 1.0f, position,
                                          normal, ndotl, st, c)) {
          direct = V3{m->diffuse[0] * ndotl, m->diffuse[1] * ndotl, m->diffuse[2] * ndotl};
        }
        const V4 hemi = random_hemisphere<CFG::kDevLibm>(fx, fy, (float)(s + 3u), (float)(s + 4u));
        dir = align_hemisphere<CFG::kDevLibm>(hemi, normal);
        prim = pl.prim;
        alive = fp.giMaxDepth > 0;
      }
      gp.direct[pix] = make_float4(direct.x, direct.y, direct.z, 0.0f);
      gp.indirect[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    uint32_t slot;
    if (gp.directQueue) {
      slot = ((start + t) * fp.fusedFrames + frame) * (uint32_t)kBlock + threadIdx.x;
      if (!alive) gp.q[0].m[slot] = make_uint4(kDeadPath, 0u, 0u, 0u);
    } else {
      slot = wave_append(&gp.counts[0], alive);
    }
    if (alive) {
      gp.q[0].o[slot] = make_float4(position.x, position.y, position.z, fx);
      gp.q[0].d[slot] = make_float4(dir.x, dir.y, dir.z, dir.w);
      gp.q[0].n[slot] = make_float4(normal.x, normal.y, normal.z, normal.w);
      gp.q[0].m[slot] = make_uint4(pix, (uint32_t)prim, __float_as_uint(fy), frame);
    }
  }
}

// Workgroup of the kLdsScene instantiations: eight wavefronts share one LDS copy of the scene (a 4.7 KB Cornell box + eight
// 2 KB stacks = 21 KB per workgroup: the CU still holds its 32 waves).
constexpr int kLdsSceneWaves = 8;

// The workgroup's LDS: [scene copy (kLdsScene only): nodes, then traversal triangles][one stack of gp.ldsRows rows per wave].
// Copies the scene (all threads, then a barrier) and returns this thread's stack column.
template <class CFG>
__device__ __forceinline__ int* stage_lds_setup(SceneDev& sc, uint32_t ldsRows, int* lds) {
  uint32_t stackBase = 0;   // dwords
  if constexpr (CFG::kLdsScene) {
    const uint32_t nodeF4 = sc.n_nodes * 2u, triF4 = sc.n_prims * 3u;
    float4* dst = (float4*)lds;
    for (uint32_t i = threadIdx.x; i < nodeF4; i += blockDim.x) dst[i] = sc.nodes[i];
    for (uint32_t i = threadIdx.x; i < triF4; i += blockDim.x) dst[nodeF4 + i] = sc.tris[i];
    __syncthreads();
    sc.ldsNodes = (uint32_t)(size_t)(__attribute__((address_space(3))) int*)lds;
    sc.ldsTris = sc.ldsNodes + nodeF4 * 16u;
    stackBase = (nodeF4 + triF4) * 4u;
  }
  return lds + stackBase + (threadIdx.x / kBlock) * ldsRows * kBlock + (threadIdx.x % kBlock);
}

template <class CFG>
__global__ __launch_bounds__(CFG::kLdsScene ? kBlock * kLdsSceneWaves : kBlock, LT_GI_STAGE_WAVES)
void lt_gi_bounce_kernel(SceneDev sc, FrameParams fp, GiParams gp, uint32_t depth) {
  extern __shared__ int lds_stack[];
  Stack<CFG::kDeep> st;
  st.lds = stage_lds_setup<CFG>(sc, gp.ldsRows, lds_stack);
  st.rows = (int)gp.ldsRows;
  Counters c{};
  const GiQueue in = gp.q[depth & 1u], out = gp.q[(depth + 1u) & 1u];
  const uint32_t total = gp.counts[depth * kQueueStride];
  const int d = (int)depth;
  const uint32_t lane = threadIdx.x % kBlock;
  for (;;) {
    uint32_t chunk = 0;
    if (lane == 0) chunk = atomicAdd(&gp.work[depth * kQueueStride], 1u);
    chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
    if ((uint64_t)chunk * kBlock >= total) break;
    const uint32_t e = chunk * kBlock + lane;
    bool alive = false;
    V4 epos{}, enorm{}, ndir{};
    uint4 misc = make_uint4(0u, 0u, 0u, 0u);
    float fx = 0.0f;
    int hitPrim = 0;
    if (e < total) {
      const float4 o = in.o[e], dd = in.d[e], nn = in.n[e];
      misc = in.m[e];
      fx = o.w;
      const float fy = __uint_as_float(misc.z);
      const uint32_t pix = misc.x;
      const Ray ext{mk4(o.x, o.y, o.z, 1.0f), mk4(dd.x, dd.y, dd.z, dd.w)};
      const V4 previousNormal = mk4(nn.x, nn.y, nn.z, nn.w);
      Hit epl{0, 0, kFltMax, 0.0f, 0.0f};
      if (gp.hits != nullptr) {   // traced ahead of this launch by lt_trace_kernel (t is not read below)
        const uint4 h = gp.hits[e];
        epl.prim = (int)h.x; epl.hitType = (int)h.y; epl.u = __uint_as_float(h.z); epl.v = __uint_as_float(h.w);
      } else {
        traverse<kGI, CFG::kDeep, false, false, CFG::kLdsScene>(sc, ext, true, (int)misc.y, epl, st, c);
      }
      const uint32_t s = gp.sample + misc.w, sd = s + depth;
      float4 ind = gp.indirect[pix];
      if (is_light(sc.lights, epl.prim)) {
        // the reference keeps looping with the SAME ray (gi.cl:319-321): same hit, one more term per remaining depth
        const float k = dot4(previousNormal, ext.d);
        for (int dd2 = d; dd2 < fp.giMaxDepth; dd2++) {
          const float w = (float)(1.0 / (double)(dd2 + 1));
          ind.x = Math<CFG::kDevLibm>::mad(w * 1.0f, k, ind.x);
          ind.y = Math<CFG::kDevLibm>::mad(w * 1.0f, k, ind.y);
          ind.z = Math<CFG::kDevLibm>::mad(w * 1.0f, k, ind.z);
        }
        gp.indirect[pix] = ind;
      } else if (epl.hitType == 1) {
        const float w = (float)(1.0 / (double)(d + 1));
        const float* epr = prim_ptr(sc, epl.prim);
        const Material* em = sc.mats + prim_material(epr);
        float endotl;
        if (direct_light<kGI, CFG>(sc, epr, epl.prim, epl.u, epl.v, fx, fy, (float)(sd + 5u), (float)(sd + 6u), (float)(sd + 7u), 1.0f,
                                   epos, enorm, endotl, st, c)) {
          ind.x = Math<CFG::kDevLibm>::mad(w * em->diffuse[0], endotl, ind.x);
          ind.y = Math<CFG::kDevLibm>::mad(w * em->diffuse[1], endotl, ind.y);
          ind.z = Math<CFG::kDevLibm>::mad(w * em->diffuse[2], endotl, ind.z);
          gp.indirect[pix] = ind;
          const V4 hemi = random_hemisphere<CFG::kDevLibm>(fx, fy, (float)(sd + 8u), (float)(sd + 9u));
          ndir = align_hemisphere<CFG::kDevLibm>(hemi, enorm);
          hitPrim = epl.prim;
          alive = d + 1 < fp.giMaxDepth;
        }
      }
    }
    const uint32_t slot = wave_append(&gp.counts[(depth + 1u) * kQueueStride], alive);
    if (alive) {
      out.o[slot] = make_float4(epos.x, epos.y, epos.z, fx);
      out.d[slot] = make_float4(ndir.x, ndir.y, ndir.z, ndir.w);
      out.n[slot] = make_float4(enorm.x, enorm.y, enorm.z, enorm.w);
      out.m[slot] = make_uint4(misc.x, (uint32_t)hitPrim, misc.z, misc.w);
    }
  }
}

// ---- a bounce stage in pieces, around lt_trace_kernel (further down), when its extension rays were traced ahead of it:
//   lt_gi_classify_kernel : every path of the stage's queue: a light hit adds its terms (gi.cl:319-321); a surface hit joins the list
//   lt_gi_shadow_kernel   : every path of the list: the light sample (gi.cl:323-349) and its shadow ray, into the shadow queue
//   (lt_trace_kernel, any-hit, over the shadow queue)
//   lt_gi_finish_kernel   : every path of the list whose shadow ray found nothing: the indirect term, the next extension ray
//                           (gi.cl:350-366), appended to the next stage's queue
// Same arithmetic per path as lt_gi_bounce_kernel, same order of a pixel's terms (one path per pixel and frame).  What it buys:
// on the 1 M-triangle wall nine extension rays in ten hit nothing, and a wavefront of the one-kernel stage ran the light
// sampling (three double-precision random() calls) and a per-lane shadow walk for the few lanes that did; here those lanes of
// all wavefronts are packed into full wavefronts first.
// (kClassifyBatch paths per lane and list append: an atomic on ONE address completes every ~12 ns chip-wide, and one per 64 paths
// made this kernel -- 16 bytes in, at most 4 out per path -- take 33 ms for the 133 M paths of the 1 M-triangle wall's first stage)
constexpr int kClassifyBatch = 8;
template <class CFG>
__global__ __launch_bounds__(256) void lt_gi_classify_kernel(SceneDev sc, FrameParams fp, GiParams gp, uint32_t depth) {
  const GiQueue in = gp.q[depth & 1u];
  const uint32_t total = gp.counts[depth * kQueueStride];
  const uint32_t lane = threadIdx.x % kBlock, wave = (blockIdx.x * blockDim.x + threadIdx.x) / kBlock, waves = gridDim.x * blockDim.x / kBlock;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint64_t base = (uint64_t)wave * (kBlock * kClassifyBatch); base < total; base += (uint64_t)waves * (kBlock * kClassifyBatch)) {
    bool surface[kClassifyBatch];
    uint32_t before[kClassifyBatch];   // surface hits of this wave's batch in front of this lane's k-th path
    uint32_t count = 0u;
#pragma unroll
    for (int k = 0; k < kClassifyBatch; k++) {
      const uint64_t e = base + (uint64_t)k * kBlock + lane;
      surface[k] = false;
      if (e < total && !(gp.directQueue && depth == 0u && in.m[e].x == kDeadPath)) {
        const uint4 h = gp.hits[e];
        if (is_light(sc.lights, (int)h.x)) {
          // the reference keeps looping with the SAME ray (gi.cl:319-321): same hit, one more term per remaining depth
          const float4 dd = in.d[e], nn = in.n[e];
          const uint32_t pix = in.m[e].x;
          const float kk = dot4(mk4(nn.x, nn.y, nn.z, nn.w), mk4(dd.x, dd.y, dd.z, dd.w));
          float4 ind = gp.indirect[pix];
          for (int dd2 = (int)depth; dd2 < fp.giMaxDepth; dd2++) {
            const float w = (float)(1.0 / (double)(dd2 + 1));
            ind.x = Math<CFG::kDevLibm>::mad(w * 1.0f, kk, ind.x);
            ind.y = Math<CFG::kDevLibm>::mad(w * 1.0f, kk, ind.y);
            ind.z = Math<CFG::kDevLibm>::mad(w * 1.0f, kk, ind.z);
          }
          gp.indirect[pix] = ind;
        } else {
          surface[k] = h.y == 1u;
        }
      }
      const unsigned long long m = __ballot(surface[k]);
      before[k] = count + (uint32_t)__popcll(m & below);
      count += (uint32_t)__popcll(m);
    }
    if (count == 0u) continue;
    uint32_t slot0 = 0u;
    if (lane == 0u) slot0 = atomicAdd(&gp.hitCount[depth * kQueueStride], count);
    slot0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot0);
#pragma unroll
    for (int k = 0; k < kClassifyBatch; k++)
      if (surface[k]) gp.hitList[slot0 + before[k]] = (uint32_t)(base + (uint64_t)k * kBlock + lane);
  }
}

template <class CFG>
__global__ __launch_bounds__(256) void lt_gi_shadow_kernel(SceneDev sc, FrameParams fp, GiParams gp, uint32_t depth) {
  const GiQueue in = gp.q[depth & 1u];
  const uint32_t total = gp.hitCount[depth * kQueueStride];
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const uint32_t e = gp.hitList[i];
    const uint4 h = gp.hits[e], misc = in.m[e];
    const float fx = in.o[e].w, fy = __uint_as_float(misc.z);
    const uint32_t sd = gp.sample + misc.w + depth;
    V4 epos, enorm, toLight;
    float tmax, endotl;
    light_sample<CFG>(sc, prim_ptr(sc, (int)h.x), __uint_as_float(h.z), __uint_as_float(h.w), fx, fy, (float)(sd + 5u), (float)(sd + 6u), (float)(sd + 7u),
                      1.0f, epos, enorm, toLight, tmax, endotl);
    gp.so[i] = make_float4(epos.x, epos.y, epos.z, tmax);
    gp.sd[i] = make_float4(toLight.x, toLight.y, toLight.z, toLight.w);
    gp.sm[i] = make_uint4(e, h.x, __float_as_uint(endotl), 0u);
    gp.sn[i] = make_float4(enorm.x, enorm.y, enorm.z, enorm.w);
  }
}

template <class CFG>
__global__ __launch_bounds__(256) void lt_gi_finish_kernel(SceneDev sc, FrameParams fp, GiParams gp, uint32_t depth) {
  const GiQueue in = gp.q[depth & 1u], out = gp.q[(depth + 1u) & 1u];
  const uint32_t total = gp.hitCount[depth * kQueueStride];
  const uint32_t stride = gridDim.x * blockDim.x;
  const int d = (int)depth;
  for (uint32_t base = blockIdx.x * blockDim.x; base < total; base += stride) {   // (whole wavefronts take part in wave_append)
    const uint32_t i = base + threadIdx.x;
    bool alive = false;
    V4 ndir{};
    float4 so = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sn = so;
    uint4 sm = make_uint4(0u, 0u, 0u, 0u), misc = sm;
    float fx = 0.0f;
    if (i < total && gp.occluded[i] == 0u) {   // the shadow ray found nothing (gi.cl:351)
      so = gp.so[i]; sn = gp.sn[i]; sm = gp.sm[i];
      const uint32_t e = sm.x;
      misc = in.m[e];
      fx = in.o[e].w;
      const float fy = __uint_as_float(misc.z);
      const uint32_t pix = misc.x, sd = gp.sample + misc.w + depth;
      const float w = (float)(1.0 / (double)(d + 1));
      const Material* em = sc.mats + prim_material(prim_ptr(sc, (int)sm.y));
      const float endotl = __uint_as_float(sm.z);
      float4 ind = gp.indirect[pix];
      ind.x = Math<CFG::kDevLibm>::mad(w * em->diffuse[0], endotl, ind.x);
      ind.y = Math<CFG::kDevLibm>::mad(w * em->diffuse[1], endotl, ind.y);
      ind.z = Math<CFG::kDevLibm>::mad(w * em->diffuse[2], endotl, ind.z);
      gp.indirect[pix] = ind;
      const V4 hemi = random_hemisphere<CFG::kDevLibm>(fx, fy, (float)(sd + 8u), (float)(sd + 9u));
      ndir = align_hemisphere<CFG::kDevLibm>(hemi, mk4(sn.x, sn.y, sn.z, sn.w));
      alive = d + 1 < fp.giMaxDepth;
    }
    const uint32_t slot = wave_append(&gp.counts[(depth + 1u) * kQueueStride], alive);
    if (alive) {
      out.o[slot] = make_float4(so.x, so.y, so.z, fx);
      out.d[slot] = make_float4(ndir.x, ndir.y, ndir.z, ndir.w);
      out.n[slot] = sn;
      out.m[slot] = make_uint4(misc.x, sm.y, misc.z, misc.w);
    }
  }
}

// =====================================================================================================================
// lt_trace_kernel: a queue of rays through the per-lane walk over the own tree (lt_device.hpp: own_walk_step), with LANE REFILL.
// Incoherent rays differ in cost by two orders of magnitude -- a bounce ray that leaves the 1 M-triangle wall visits a handful
// of groups, one that grazes it several hundred leaves -- and a wavefront that walks 64 of them side by side runs until its
// slowest lane is done (measured on that scene's bounce stage: 14-17 % of the lanes active in the average vector instruction,
// profiles/r2/gi_wall, gpurun_out r3).  Here a lane whose ray is done takes the next ray of the queue: whenever at least
// `refill` lanes of the wave are idle (or all of them), the idle lanes claim that many rays with ONE atomic (ballot, popcount,
// prefix count) and set them up; then every lane with a ray makes one step.  A lane's state is its ray and its stack, nothing
// of the shading that produced the ray or will consume the hit: that is why this is a kernel of its own.
//   rays:   o[i] = (origin.xyz, tmax of an any-hit ray), d[i] = direction.xyzw, m[i].y = the primitive the ray starts on (ignored,
//           acc.cl:188)
//   result: hit[i] = (primitive, hitType, u, v) of a closest-hit ray (t is not kept: no caller reads it); occluded[i] = hitType of an
//           any-hit ray (its caller reads nothing else)
// Rays the walks over the own tree do not take (a non-finite component, magnitudes beyond packet_ray_ok) are walked at once, in
// the reference's order over the caller's tree, by the lane that drew them.  Every wave reaches the exit: the queue hands out
// each index once, a lane's walk ends (the stack only holds entries of a finite tree), and the loop ends when the queue is drained
// and no lane holds a ray.
constexpr int kTraceClaim = 512;   // rays a wave claims from the queue per atomic
struct TraceParams {
  const float4* o;
  const float4* d;
  const uint4* m;
  uint4* hit;              // closest-hit walks
  uint32_t* occluded;      // any-hit walks: one word per ray, != 0 when something was hit (their callers read nothing else)
  const uint32_t* count;   // rays in the queue (device memory: written by the stage that filled it)
  uint32_t* next;          // work counters (zeroed by the host): one per eighth of the queue, kQueueStride dwords apart
  uint32_t refill;         // idle lanes that trigger a refill
  uint32_t dead;           // != 0: the queue is direct-mapped, slots with m.x == kDeadPath hold no ray
};

template <int PROGRAM, bool ANYHIT>
__global__ __launch_bounds__(kBlock, 8) void lt_trace_kernel(SceneDev sc, TraceParams tp) {
  using u64 = unsigned long long;
  extern __shared__ int lds_stack[];   // [kTraceRows stack rows][kTraceStage rows of staged rays], 64 lanes each
  int* const col = lds_stack + threadIdx.x;
  int* const stage = lds_stack + kTraceRows * kBlock;
  const uint32_t total = tp.count[0];
  const uint32_t lane = threadIdx.x;
  const u64 below = (1ull << lane) - 1ull;
  // (a short queue is shared out in small claims, so that it is not a few waves' work; a long one in claims of kTraceClaim)
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kTraceClaim ? (uint32_t)kTraceClaim : share);
  bool active = false;
  // the wave's staged batch of rays: stageCount of them (each with its index in the queue), the first stageTaken handed out; they
  // come out of the wave's claim [claimNext, claimEnd) of the queue (kTraceClaim rays per atomic: one address serves an atomic
  // every ~12 ns, 80 M per second chip-wide)
  uint32_t stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;   // the queue has handed out its last ray, and the wave's claim is staged
  Ray ray{};
  float ix = 0.0f, iy = 0.0f, iz = 0.0f;
  OwnRay w{};
  Hit pl{0, 0, kFltMax, 0.0f, 0.0f};
  uint32_t idx = 0u, e = 0u;
  int sp = 0;
  int deep[kOwnRows + kOwnDeep - kTraceRows];
  for (;;) {
    const u64 idle = __builtin_amdgcn_ballot_w64(!active);
    const uint32_t nIdle = (uint32_t)__popcll(idle);
    if ((nIdle >= tp.refill || nIdle == (uint32_t)kBlock) && (stageTaken < stageCount || !drained)) {
      if (stageTaken == stageCount) {
        // the next 64 rays of the queue, one per lane (coalesced), parked in LDS: the lanes' own registers hold their walks
        // The queue in eighths, one per XCD (an eighth of a direct-mapped queue is an eighth of the image: the XCD's L2 then
        // serves the groups and leaves of one part of the scene): a wave claims from the eighth of the XCD it runs on, then from
        // the others'.
        while (claimNext == claimEnd && sweep < 8u) {
          const uint32_t part = (home + sweep) & 7u;
          const uint32_t lo = (uint32_t)((uint64_t)total * part / 8u / kBlock * kBlock), hi = part == 7u ? total : (uint32_t)((uint64_t)total * (part + 1u) / 8u / kBlock * kBlock);
          uint32_t got = 0u;
          if (lane == 0u) got = atomicAdd(&tp.next[part * kQueueStride], claim);
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
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), dd = o;
        uint32_t ign = 0u;
        bool live = lane < batch;
        if (live) {
          const uint2 mm = *(const uint2*)&tp.m[base + lane];
          ign = mm.y;
          live = !(tp.dead && mm.x == kDeadPath);
        }
        if (live) { o = tp.o[base + lane]; dd = tp.d[base + lane]; }
        const u64 lm = __builtin_amdgcn_ballot_w64(live);
        stageCount = (uint32_t)__popcll(lm);
        if (live) {
          const uint32_t at = (uint32_t)__popcll(lm & below);
          stage[0 * kBlock + at] = __float_as_int(o.x); stage[1 * kBlock + at] = __float_as_int(o.y); stage[2 * kBlock + at] = __float_as_int(o.z);
          stage[3 * kBlock + at] = __float_as_int(dd.x); stage[4 * kBlock + at] = __float_as_int(dd.y); stage[5 * kBlock + at] = __float_as_int(dd.z);
          stage[6 * kBlock + at] = __float_as_int(dd.w); stage[7 * kBlock + at] = (int)ign;
          stage[8 * kBlock + at] = __float_as_int(o.w);   // tmax of an any-hit ray
          stage[9 * kBlock + at] = (int)(base + lane);
        }
        // (one wavefront per workgroup: its own LDS writes are visible to it once they have completed -- the reads below wait for them)
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = (uint32_t)__popcll(idle & below);
      if (!active && mine < take) {
        const uint32_t s = stageTaken + mine;
        idx = (uint32_t)stage[9 * kBlock + s];
        ray = Ray{mk4(__int_as_float(stage[0 * kBlock + s]), __int_as_float(stage[1 * kBlock + s]), __int_as_float(stage[2 * kBlock + s]), 1.0f),
                  mk4(__int_as_float(stage[3 * kBlock + s]), __int_as_float(stage[4 * kBlock + s]), __int_as_float(stage[5 * kBlock + s]),
                      __int_as_float(stage[6 * kBlock + s]))};
        const int ign = stage[7 * kBlock + s];
        ix = 1.0f / ray.d.x; iy = 1.0f / ray.d.y; iz = 1.0f / ray.d.z;
        pl = Hit{0, 0, ANYHIT ? __int_as_float(stage[8 * kBlock + s]) : kFltMax, 0.0f, 0.0f};
        const bool finite = __builtin_fabsf(ix) < __builtin_inff() && __builtin_fabsf(iy) < __builtin_inff() && __builtin_fabsf(iz) < __builtin_inff() &&
                            __builtin_fabsf(ray.o.x) < __builtin_inff() && __builtin_fabsf(ray.o.y) < __builtin_inff() &&
                            __builtin_fabsf(ray.o.z) < __builtin_inff();
        if (finite && packet_ray_ok(ray, ix, iy, iz)) {
          w = own_ray(sc, ray, ix, iy, iz, ign);
          e = 0u;
          sp = 0;
          active = true;
        } else {   // (rare) the reference's order over the caller's tree, here and now
          ScratchStack ss;
          Counters c{};
          traverse_nodes_impl<PROGRAM, ScratchStack, false, false, ANYHIT, false>(sc, ray, ix, iy, iz, true, ign, pl, ss, c);
          if (ANYHIT) tp.occluded[idx] = (uint32_t)pl.hitType;
          else tp.hit[idx] = make_uint4((uint32_t)pl.prim, (uint32_t)pl.hitType, __float_as_uint(pl.u), __float_as_uint(pl.v));
        }
      }
      stageTaken += take;
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
      if (drained && stageTaken == stageCount) break;
      continue;
    }
    if (active) {
      if (own_walk_step<PROGRAM, ANYHIT, kTraceRows>(sc, ray, ix, iy, iz, w, pl, col, deep, e, sp)) {
        if (ANYHIT) tp.occluded[idx] = (uint32_t)pl.hitType;
        else tp.hit[idx] = make_uint4((uint32_t)pl.prim, (uint32_t)pl.hitType, __float_as_uint(pl.u), __float_as_uint(pl.v));
        active = false;
      }
    }
  }
}

// accumulator's shadow rays walked by lt_trace_kernel (SceneDev::shadowPackets == 3): a sample whose ray met an occluder is
// black (acc.cl:276-279: the colour is only assigned when the shadow payload's hitType is 0)
__global__ __launch_bounds__(256) void lt_shadow_resolve_kernel(const uint4* __restrict__ m, const uint32_t* __restrict__ occluded, uint32_t slots,
                                                                float* __restrict__ out, unsigned long long frameStride, uint32_t depth) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {
    const uint4 mm = m[i];
    if (mm.x == kDeadSlot || occluded[i] == 0u) continue;
    float* o = out + (size_t)mm.z * frameStride + (size_t)mm.x * depth;
    o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
  }
}

// direct + indirect (gi.cl:374), clamp (:409-411), running mean, store
template <class CFG>
__global__ void lt_gi_resolve_kernel(FrameParams fp, GiParams gp, float* __restrict__ out, uint32_t pixels) {
  const uint32_t vpix = blockIdx.x * blockDim.x + threadIdx.x;   // (frame, pixel) of a fused launch
  if (vpix >= pixels) return;
  const uint32_t frame = vpix / gp.pixels, pix = vpix - frame * gp.pixels;
  // only pixels inside the image were written by the primary stage
  const uint32_t perTile = fp.tileW * fp.tileH, k = pix / perTile, rem = pix % perTile, ly = rem / fp.tileW, lx = rem % fp.tileW;
  const uint32_t tile = fp.tileFirst + k * fp.tileStride, tx = tile % fp.tilesX, ty = tile / fp.tilesX;
  if (k >= fp.tilesInCall || tx * fp.tileW + lx >= fp.width || ty * fp.tileH + ly >= fp.height) return;
  const float4 di = gp.direct[vpix], in = gp.indirect[vpix];
  V3 color{di.x + in.x, di.y + in.y, di.z + in.z};
  if (fp.clampOutput && !gp.raw) color = V3{Math<CFG::kDevLibm>::clamp01(color.x), Math<CFG::kDevLibm>::clamp01(color.y), Math<CFG::kDevLibm>::clamp01(color.z)};
  float* o = out + (size_t)frame * fp.frameStride + (size_t)pix * fp.depth;   // fused: this frame's un-accumulated slice
  if (fp.accumulateN <= 0) {
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
  } else {
    const float n = (float)fp.accumulateN, n1 = (float)(fp.accumulateN + 1);
    o[0] = (color.x + (o[0] * n)) / n1;
    o[1] = (color.y + (o[1] * n)) / n1;
    o[2] = (color.z + (o[2] * n)) / n1;
  }
}

// The 25-sample variant (resources/kernels/opencl/global_illumination.cl:408-420): samples k0 .. k0+n-1 of one frame, stored
// un-clamped by the resolve stage at samples + j * stride, are blended in order, `c = (1-a)*c + a*c_k`, a = (25-k)/25; the
// partial blend waits in gp.blend between chunks; after sample 24 the colour is clamped (linearKernel) and stored or folded
// into the running mean like any frame.  Pixels of edge tiles outside the image are skipped.
template <class CFG>
__global__ void lt_gi_blend25_kernel(FrameParams fp, GiParams gp, const float* __restrict__ samples, uint32_t k0, uint32_t n,
                                     float* __restrict__ out, uint32_t pixels) {
  const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= pixels) return;
  const uint32_t perTile = fp.tileW * fp.tileH, k = pix / perTile, rem = pix % perTile, ly = rem / fp.tileW, lx = rem % fp.tileW;
  const uint32_t tile = fp.tileFirst + k * fp.tileStride, tx = tile % fp.tilesX, ty = tile / fp.tilesX;
  if (k >= fp.tilesInCall || tx * fp.tileW + lx >= fp.width || ty * fp.tileH + ly >= fp.height) return;
  V3 color{0.0f, 0.0f, 0.0f};
  if (k0 > 0u) {
    const float4 b = gp.blend[pix];
    color = V3{b.x, b.y, b.z};
  }
  for (uint32_t j = 0; j < n; j++) {
    const float* c = samples + (size_t)j * fp.frameStride + (size_t)pix * fp.depth;
    const V3 cn{c[0], c[1], c[2]};
    const uint32_t kk = k0 + j;
    if (kk == 0u) {
      color = cn;
    } else {
      const float a = Math<CFG::kDevLibm>::div25((float)(25 - (int)kk));
      color = V3{Math<CFG::kDevLibm>::mad(1.0f - a, color.x, a * cn.x), Math<CFG::kDevLibm>::mad(1.0f - a, color.y, a * cn.y),
                 Math<CFG::kDevLibm>::mad(1.0f - a, color.z, a * cn.z)};
    }
  }
  if (k0 + n < 25u) {
    gp.blend[pix] = make_float4(color.x, color.y, color.z, 0.0f);
    return;
  }
  if (fp.clampOutput) color = V3{Math<CFG::kDevLibm>::clamp01(color.x), Math<CFG::kDevLibm>::clamp01(color.y), Math<CFG::kDevLibm>::clamp01(color.z)};
  float* o = out + (size_t)pix * fp.depth;
  if (fp.accumulateN <= 0) {
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
  } else {
    const float nf = (float)fp.accumulateN, n1 = (float)(fp.accumulateN + 1);
    o[0] = (color.x + (o[0] * nf)) / n1;
    o[1] = (color.y + (o[1] * nf)) / n1;
    o[2] = (color.z + (o[2] * nf)) / n1;
  }
}
