// lt_capi.hip -- liblenstrace-hip.so: the C ABI of include/lenstrace_hip.h over hand-written gfx950 kernels.
// Host side of what the reference does in RendererOpenCL::render() (src/opencl/renderer_opencl.cpp:56-153).
#include "lt_kernel.hpp"
#include "lt_retree.hpp"
#include "lt_own16.hpp"
#include "lt_prep.hpp"
#include "lt_build.hpp"
#include "lt_query.hpp"
#include "lt_nearest.hpp"
#include "lt_overlap.hpp"
#include "lt_tritri.hpp"
#include "lt_overlist.hpp"
#include "lt_shade.hpp"
#include "lt_paths.hpp"

#include "../../include/lenstrace_hip.h"

#include <dlfcn.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <exception>
#include <thread>
#include <type_traits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

// Triangle re-tiling at upload: 76-byte Primitive -> 48-byte (A, B-A, C-A, 0 0 0).
__global__ void lt_retile_kernel(const float* __restrict__ prims, float4* __restrict__ tris, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = prims + 19 * (size_t)i;
  const float ax = p[0], ay = p[1], az = p[2];
  tris[3 * (size_t)i + 0] = make_float4(ax, ay, az, p[3] - ax);
  tris[3 * (size_t)i + 1] = make_float4(p[4] - ay, p[5] - az, p[6] - ax, p[7] - ay);
  tris[3 * (size_t)i + 2] = make_float4(p[8] - az, 0.0f, 0.0f, 0.0f);
}

// The records of the packet walks (lt_walk_asm.hpp, packet_walk_cpp), one 64-byte slot per node of the backend's own tree:
//   interior node i: [left child's box, its reference, -][right child's box, its reference, -], the boxes pushed outwards by
//                    2^-21 of each bound and one float more (the walks' conservative test needs lo' <= lo - 6 * 2^-24 |lo|),
//                    a reference = the child's index, with bit 31 set when the child is a leaf;
//   leaf i:          [A, e1 = B - A, e2 = C - A of its triangle (lt_retile_kernel's arithmetic)][the leaf's own box, bit for
//                    bit][the primitive offset]: what the reference's leaf test needs, in one scalar load.
__device__ __forceinline__ float lt_outwards(float b, bool up) { return lt_own16::outwards(b, up); }
__global__ void lt_own_pair_kernel(const float4* __restrict__ nodes, const float* __restrict__ prims, float4* __restrict__ pairs, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = nodes[2 * (size_t)i], b = nodes[2 * (size_t)i + 1];
  if ((__float_as_uint(b.w) & 0xffffu) != 0u) {
    const float* p = prims + 19 * (size_t)__float_as_uint(b.z);
    const float ax = p[0], ay = p[1], az = p[2];
    pairs[4 * (size_t)i + 0] = make_float4(ax, ay, az, p[3] - ax);
    pairs[4 * (size_t)i + 1] = make_float4(p[4] - ay, p[5] - az, p[6] - ax, p[7] - ay);
    pairs[4 * (size_t)i + 2] = make_float4(p[8] - az, a.x, a.y, a.z);
    pairs[4 * (size_t)i + 3] = make_float4(a.w, b.x, b.y, b.z);
    return;
  }
  const uint32_t child[2] = {i + 1u, __float_as_uint(b.z)};
  for (int k = 0; k < 2; k++) {
    const float4 ca = nodes[2 * (size_t)child[k]], cb = nodes[2 * (size_t)child[k] + 1];
    const bool leaf = (__float_as_uint(cb.w) & 0xffffu) != 0u;
    pairs[4 * (size_t)i + 2 * k] = make_float4(lt_outwards(ca.x, false), lt_outwards(ca.y, false), lt_outwards(ca.z, false), lt_outwards(ca.w, true));
    pairs[4 * (size_t)i + 2 * k + 1] = make_float4(lt_outwards(cb.x, true), lt_outwards(cb.y, true), __uint_as_float(child[k] | (leaf ? 0x80000000u : 0u)), 0.0f);
  }
}

// The per-lane walks' records (SceneDev::wide, traverse_own_lane), 64 bytes each, one array:
//   [0, groups)                          the 4-wide groups of lt_retree::collapse_wide: four 16-byte child slots -- the child's box
//                                        on a 16-bit grid over the scene's bounds, rounded outwards (lt_own16.hpp: in real
//                                        arithmetic O + ql S <= lo - 8u|lo| and O + qh S >= hi + 8u|hi|), and its link;
//   [groups, groups + n_prims]           leaf records by primitive offset: the triangle re-tiled (A, B - A, C - A: lt_retile_kernel's
//                                        arithmetic), the leaf's own box bit for bit, the offset -- what the reference's leaf test
//                                        needs -- and one more behind them whose box is NaN (the target of empty slots).
// *bad is set when a bound falls off the grid (the host sizes the grid from the root's box with room to spare; the scene then
// simply gets no hierarchy of the backend's own).
struct Own16Frame { float O[3], S[3]; };
__global__ void lt_wide_kernel(const float4* __restrict__ nodes, const uint32_t* __restrict__ children, const uint32_t* __restrict__ groupOf,
                               uint4* __restrict__ wide, uint32_t groups, uint32_t n_prims, Own16Frame fr, uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // slot
  if (i >= 4u * groups) return;
  const uint32_t child = children[i];
  lt_own16::Rec r = lt_own16::empty_slot(groups, n_prims);
  if (child != 0xffffffffu) {
    const float4 a = nodes[2 * (size_t)child], b = nodes[2 * (size_t)child + 1];
    const float lo[3] = {a.x, a.y, a.z}, hi[3] = {a.w, b.x, b.y};
    const bool leaf = (__float_as_uint(b.w) & 0xffffu) != 0u;
    const uint32_t link = leaf ? (0x80000000u | (groups + __float_as_uint(b.z))) : groupOf[child];
    if (!lt_own16::slot_record(lo, hi, link, fr.O, fr.S, r)) atomicOr(bad, 1u);
  }
  wide[i] = make_uint4(r.x, r.y, r.z, r.w);
}
__global__ void lt_wide_leaf_kernel(const float4* __restrict__ nodes, const float* __restrict__ prims, float4* __restrict__ wide, uint32_t n,
                                    uint32_t groups, uint32_t n_prims) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // node of the own tree; thread n writes the record behind the last primitive's
  if (i > n) return;
  if (i == n) {
    const float q = __uint_as_float(0x7fc00000u);
    float4* r = wide + 4 * ((size_t)groups + n_prims);
    r[0] = r[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    r[2] = make_float4(0.0f, q, q, q);
    r[3] = make_float4(q, q, q, __uint_as_float(n_prims));
    return;
  }
  const float4 a = nodes[2 * (size_t)i], b = nodes[2 * (size_t)i + 1];
  if ((__float_as_uint(b.w) & 0xffffu) == 0u) return;
  const uint32_t prim = __float_as_uint(b.z);
  const float* p = prims + 19 * (size_t)prim;
  const float ax = p[0], ay = p[1], az = p[2];
  float4* r = wide + 4 * ((size_t)groups + prim);
  r[0] = make_float4(ax, ay, az, p[3] - ax);
  r[1] = make_float4(p[4] - ay, p[5] - az, p[6] - ax, p[7] - ay);
  r[2] = make_float4(p[8] - az, a.x, a.y, a.z);
  r[3] = make_float4(a.w, b.x, b.y, b.z);
}

// Gathered per-rank tile stacks -> row-major image (root side of the one gather per frame).
__global__ void lt_untile_kernel(const float* __restrict__ gathered, uint64_t floatsPerRank, uint32_t nRanks, uint32_t W,
                                 uint32_t H, uint32_t depth, uint32_t tileW, uint32_t tileH, uint32_t tilesX,
                                 float* __restrict__ image) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)W * H) return;
  const uint32_t x = (uint32_t)(i % W), y = (uint32_t)(i / W);
  const uint32_t tx = x / tileW, ty = y / tileH, tile = ty * tilesX + tx;
  const uint32_t rank = tile % nRanks, k = tile / nRanks;
  const float* src = gathered + (uint64_t)rank * floatsPerRank +
                     (((uint64_t)k * tileH + (y - ty * tileH)) * tileW + (x - tx * tileW)) * depth;
  float* dst = image + i * depth;
  for (uint32_t ch = 0; ch < depth; ch++) dst[ch] = src[ch];
}

// Folds the n sample images of a fused launch (samples + f * stride, f < n, in frame order) into the running mean held in
// `out`: accumulator.frag:10-20, `(c + acc*n) / (n+1)` with n = base + f, the same expression in the same order as the
// read-modify-write of render_square, so the result is bit for bit what n single-sample launches leave behind.  Pixels of
// edge tiles that lie outside the image are not touched (render_square never writes them).
__global__ void lt_running_mean_kernel(const float* __restrict__ samples, uint32_t n, uint64_t stride, float* __restrict__ out,
                                       uint64_t first, uint64_t floats, int32_t base, FrameParams fp, int checkPadding) {
  const uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (this launch folds the floats [first, floats))
  if (i >= floats) return;
  if (i % fp.depth >= 3u) return;   // render_square / the GI resolve stage write channels 0..2 only; the others are the caller's
  if (checkPadding) {
    const uint64_t pix = i / fp.depth, perTile = (uint64_t)fp.tileW * fp.tileH;
    const uint32_t k = (uint32_t)(pix / perTile), rem = (uint32_t)(pix % perTile);
    const uint32_t ly = rem / fp.tileW, lx = rem % fp.tileW, tile = fp.tileFirst + k * fp.tileStride;
    if ((tile % fp.tilesX) * fp.tileW + lx >= fp.width || (tile / fp.tilesX) * fp.tileH + ly >= fp.height) return;
  }
  float acc = base > 0 ? out[i] : 0.0f;
  for (uint32_t f = 0; f < n; f++)
    acc = running_mean_step(acc, samples[(uint64_t)f * stride + i], base + (int32_t)f);
  out[i] = acc;
}

// The same fold, four consecutive floats per thread: for launches whose every float is folded (depth == 3, no padded tiles), from
// a `first` that is a multiple of four floats into an `out` aligned to 16 bytes (launch_running_mean).  A thread reads each frame's
// four floats in one load (the sample images lie `stride` floats apart, whatever that is modulo four: the loads ask for no more than
// the floats' own alignment) and has four frames' loads in flight before the first divide that depends on them; per float the
// expression and the order of the frames are lt_running_mean_kernel's.  The thread whose four floats would pass `floats` folds what
// is left of them one by one.
// map: the fold map of the launch's item table (lt_entry_cut.hpp: fold_segment), or null.  A quad lies in one 24-float segment; where
// the segment's byte is set the wave that rendered the square has folded these samples into `out` itself (render_square), and
// the sample images hold nothing for them: the thread leaves at once.
struct __attribute__((packed, aligned(4))) MeanQuad { float v[4]; };
__global__ __launch_bounds__(256) void lt_running_mean4_kernel(const float* __restrict__ samples, uint32_t n, uint64_t stride, float* __restrict__ out,
                                                               uint64_t first, uint64_t floats, int32_t base, const unsigned char* __restrict__ map) {
  const uint64_t i = first + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4u;
  if (i >= floats) return;
  if (map != nullptr && map[lt_entry_cut::fold_segment_of_float(i)] != 0) return;
  auto fold = [&](float acc, float c, int32_t N) { return running_mean_step(acc, c, N); };
  if (i + 4u > floats) {
    for (uint64_t j = i; j < floats; j++) {
      float acc = base > 0 ? out[j] : 0.0f;
      for (uint32_t f = 0; f < n; f++) acc = fold(acc, samples[(uint64_t)f * stride + j], base + (int32_t)f);
      out[j] = acc;
    }
    return;
  }
  float4 acc = base > 0 ? *(const float4*)(out + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  uint32_t f = 0;
  for (; f + 4u <= n; f += 4u) {
    MeanQuad c[4];
#pragma unroll
    for (int u = 0; u < 4; u++) c[u] = *(const MeanQuad*)(samples + (uint64_t)(f + u) * stride + i);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int32_t N = base + (int32_t)(f + u);
      acc.x = fold(acc.x, c[u].v[0], N); acc.y = fold(acc.y, c[u].v[1], N); acc.z = fold(acc.z, c[u].v[2], N); acc.w = fold(acc.w, c[u].v[3], N);
    }
  }
  for (; f < n; f++) {
    const MeanQuad c = *(const MeanQuad*)(samples + (uint64_t)f * stride + i);
    const int32_t N = base + (int32_t)f;
    acc.x = fold(acc.x, c.v[0], N); acc.y = fold(acc.y, c.v[1], N); acc.z = fold(acc.z, c.v[2], N); acc.w = fold(acc.w, c.v[3], N);
  }
  *(float4*)(out + i) = acc;
}

// The item table and the fold map of a set of entry cuts (lt_entry_cut.hpp: kItemWhole, fold_segment; FrameParams::itemTable), for
// launches of `groups` frame groups per square: workgroup x compacts the share of XCD x in the share's order -- per square its
// entries (item_entries: one where word 0 of the square's list is the clear mark), an exclusive scan of those counts 1024 squares
// at a time, item_write at the scanned place -- and leaves the share's length in word x of the table.  map, where not null: the
// byte of every segment of every square, 1 for a square handed out whole.  stats: [0] entries, [1] squares handed out whole.
constexpr uint32_t kItemThreads = 1024u;
__global__ __launch_bounds__(kItemThreads) void lt_clear_items_kernel(const uint32_t* __restrict__ cuts, FrameParams fp, uint32_t groups,
                                                                      uint32_t* __restrict__ items, unsigned char* __restrict__ map,
                                                                      unsigned long long* __restrict__ stats) {
  using namespace lt_entry_cut;
  __shared__ uint32_t waveSum[kItemThreads / kBlock], wholeSquares;
  const uint32_t xcd = blockIdx.x, tid = threadIdx.x, lane = tid % kBlock, wave = tid / kBlock;
  const uint32_t share = xcd_share_size(fp.totalSquares, xcd), start = xcd_share_start(fp.totalSquares, xcd);
  uint32_t* const dst = items + kItemHeader + (size_t)start * groups;
  if (tid == 0u) wholeSquares = 0u;
  uint32_t base = 0u;
  for (uint32_t chunk = 0u; chunk < share; chunk += kItemThreads) {
    const uint32_t local = chunk + tid;
    const bool in = local < share;
    const uint32_t word0 = in ? cuts[(size_t)(start + local) * kListWords] : 0u;
    const uint32_t count = in ? item_entries(word0, groups) : 0u;
    uint32_t incl = count;
    for (uint32_t d = 1u; d < (uint32_t)kBlock; d <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += v;
    }
    __syncthreads();   // (the sums of the chunk before have been read)
    if (lane == (uint32_t)kBlock - 1u) waveSum[wave] = incl;
    const unsigned long long wholeLanes = __builtin_amdgcn_ballot_w64(in && item_whole(word0));
    if (lane == 0u && wholeLanes != 0ull) atomicAdd(&wholeSquares, (uint32_t)__popcll(wholeLanes));
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (uint32_t w = 0u; w < kItemThreads / kBlock; w++) {
      before += w < wave ? waveSum[w] : 0u;
      total += waveSum[w];
    }
    if (in) {
      item_write(dst + base + before + incl - count, word0, local, groups);
      if (map != nullptr)
        fold_mark_square(map, fp.order ? fp.order[start + local] : start + local, fp.blocksPerTileX, fp.blocksPerTile, fp.tileW, fp.tileH,
                         item_whole(word0) ? 1 : 0);
    }
    base += total;
  }
  __syncthreads();
  if (tid == 0u) {
    items[xcd] = base;
    atomicAdd(&stats[0], (unsigned long long)base);
    atomicAdd(&stats[1], (unsigned long long)wholeSquares);
  }
}

// The walks' slab tests compare against the smallest positive float (`tExit >= max(tEnter, 0x00000001)`: "tExit > 0" in one
// instruction) and their conservative tests carry a 2^-140 margin: both need float32 denormals to be KEPT, which is hipcc's
// default for gfx950 and what this library and its run-time compiled user programs are built with.  A build with
// -fgpu-flush-denormals-to-zero would flush the constant to 0 and accept leaves the reference rejects; lt_hip_create runs this
// once and refuses such a build instead.
__global__ void lt_denormal_probe_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  const float tiny = __uint_as_float(in[0]);                       // 0x00000001
  out[0] = __float_as_uint(__builtin_fmaxf(tiny, in[1] ? 1.0f : 0.0f));   // max(denormal, 0): the denormal, unless it was flushed
  out[1] = __float_as_uint(tiny + tiny);                           // 0x00000002
}

// ---------------------------------------------------------------------------------- context
struct SceneHash {
  uint64_t buf[4] = {0, 0, 0, 0};   // nodes, primitives, materials, lights
  bool operator==(const SceneHash& o) const { return memcmp(buf, o.buf, sizeof(buf)) == 0; }
};

// LT_DEBUG_POISON=<byte>: a buffer's bytes before its first use, chosen by the caller instead of left to the allocator (fresh
// memory is zero pages, a pooled buffer holds the last scene's content).  The wait behind the fill orders it before the work of
// every stream.  A test switch: whatever reads a word that nothing wrote shows up as a difference between two byte values.
static hipError_t lt_debug_poison(void* p, size_t bytes, int byte) {
  const hipError_t e = hipMemset(p, byte, bytes);
  return e == hipSuccess ? hipDeviceSynchronize() : e;
}

// Device buffers of scenes gone by, kept for the next scene of the same shape: an animation hands over buffers of the same sizes
// frame after frame, and a hipFree / hipMalloc pair per buffer (a dozen of them, each a device-wide wait) was a tenth of
// lt_hip_set_scene.  Exact sizes only; at most kSpareCap bytes lie idle (LT_SCENE_POOL_BYTES, 0: every buffer goes straight
// back to the runtime).
struct ScenePool {
  std::multimap<size_t, void*> spare;
  std::map<void*, size_t> sizes;   // of every buffer this pool handed out
  size_t spareBytes = 0, cap = (size_t)8 << 30;
  int poison = -1;   // LT_DEBUG_POISON: every buffer handed out is filled with this byte first (lt_debug_poison)
  hipError_t get(void** p, size_t bytes) {
    if (bytes == 0) bytes = 4;
    const hipError_t e = take(p, bytes);
    return e == hipSuccess && poison >= 0 ? lt_debug_poison(*p, bytes, poison) : e;
  }
  hipError_t take(void** p, size_t bytes) {
    auto it = spare.find(bytes);
    if (it != spare.end()) {
      *p = it->second;
      spareBytes -= bytes;
      spare.erase(it);
      return hipSuccess;
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess && !spare.empty()) {   // (memory is short: the idle buffers go first)
      clear();
      e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) sizes[*p] = bytes;
    return e;
  }
  void put(void* p) {
    if (!p) return;
    auto it = sizes.find(p);
    if (it == sizes.end()) { (void)hipFree(p); return; }
    const size_t bytes = it->second;
    if (bytes > cap) { sizes.erase(it); (void)hipFree(p); return; }
    if (spareBytes + bytes > cap) clear();
    spare.emplace(bytes, p);
    spareBytes += bytes;
  }
  void clear() {
    for (auto& kv : spare) { sizes.erase(kv.second); (void)hipFree(kv.second); }
    spare.clear();
    spareBytes = 0;
  }
  hipError_t upload(void** p, const void* src, size_t bytes) {   // (a buffer from the pool holding a copy of host memory)
    const hipError_t e = get(p, bytes);
    return e == hipSuccess ? hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice) : e;
  }
  static hipError_t get_cb(void* self, void** p, size_t bytes) { return ((ScenePool*)self)->get(p, bytes); }
  static void put_cb(void* self, void* p) { ((ScenePool*)self)->put(p); }
};

struct lt_hip_context {
  int device = -1;
  ScenePool pool;
  std::string err;
  hipStream_t stream = nullptr;      // own stream for lt_hip_render
  void *d_nodes = nullptr, *d_tris = nullptr, *d_prims = nullptr, *d_mats = nullptr, *d_lights = nullptr;
  void *d_nodes2 = nullptr, *d_pairs2 = nullptr;   // the backend's own tree over the scene's leaves (lt_retree.hpp), or null
  void* d_rank8 = nullptr;                         // with it: the reference's leaf order per direction-sign octant (SceneDev::rank8)
  void* d_wide = nullptr;                          // ... and the per-lane walks' 4-wide groups and leaf records (SceneDev::wide; 64 bytes in front: the grid)
  uint32_t n_wide = 0;                             // groups
  int wide_height = 0;
  int height2 = 0;                                 // its height
  uint32_t n_nodes2 = 0;
  float retree_ms = 0.0f;                          // host time of its build
  uint32_t n_nodes = 0, n_prims = 0, n_mats = 0;
  int bvh_height = 0;
  bool has_scene = false;
  bool device_prepared = false;      // the resident scene's derived structures were made by lt_prep.hip (not by lt_retree.hpp on the host)
  uint64_t verdict_sizes[4] = {0, 0, 0, 0};   // sizes of the scene the shadow-walk verdicts below were timed on
  bool verdict_sizes_valid = false;
  bool speculate_next = true;        // lt_hip_render_scene: the last scene handed over with a frame was the resident one (render while hashing)
  SceneHash scene_hash{};                                    // content hashes (one per buffer) ...
  bool scene_hash_valid = false;     // ... of the resident scene: false for one built on the device (lt_hip_set_triangles), which no host buffers can equal
  uint64_t scene_sizes[4] = {0, 0, 0, 0};                   // ... and sizes of the resident scene (lt_hip_set_scene)
  uint32_t scene_uploads = 0, scene_reused = 0;
  float* d_out = nullptr;            // staging output for lt_hip_render
  uint64_t d_out_bytes = 0;
  void* h_out = nullptr;             // ... and its pinned host twin: the read-back lands here at the link's rate, piece by piece
  uint64_t h_out_bytes = 0;          //     (a caller's pageable buffer would be read back through the runtime's small bounce buffers)
  hipEvent_t out_ev[8] = {};         // one event per piece
  hipEvent_t fold_ev[8] = {};        // ... and one behind the fold of each piece (launch_running_mean), when the call's last fold is cut into them
  hipStream_t copy_stream = nullptr; //     the pieces travel on a stream of their own, each behind its fold
  unsigned long long* d_stats = nullptr;
  uint32_t* d_prep_flag = nullptr;   // scene preparation's flag word: the slot behind d_stats, which no render launch writes
  uint32_t* d_queues = nullptr;      // persistent mode: 8 per-XCD work counters per launch of a call, and 8 for its camera-hit pass
  uint64_t queue_frames = 0;
  int shadow_mode[6] = {-1, -1, -1, -1, -1, -1};   // per built-in program: shadow rays as any-hit packets (1) or per lane (0); -1 = not timed yet
  hipEvent_t cal_ev[12] = {};
  std::map<std::vector<uint32_t>, int> shadow_modes;
  std::map<std::vector<uint32_t>, uint32_t> shadow_groups;   // ... and the frames per work item it was timed with (launch_walk)
  unsigned long long* d_groupWalks = nullptr;   // LT_DEBUG_SHADOW_FRAMES: waves whose two frames walked together / apart / together per one-mixed-axis form (launch_walk)   // (program, W, H, tile geometry) -> the walk timed faster for it on the resident scene
  void* d_shadowq = nullptr;         // accumulator's queued shadow rays (shadow mode 3): origin+tmax, direction, (pixel, primitive, frame), occluded: 52 bytes per slot
  uint64_t shadowq_slots = 0;
  uint32_t* d_shadowCtl = nullptr;   // ... the trace launch's eight work counters (kQueueStride apart) and, behind them, the queue's length
  float* d_samples = nullptr;        // un-accumulated sample images of a fused multi-sample launch
  uint4* d_camhits = nullptr;        // the camera-hit pass's hits (FrameParams::cameraHits): 16 bytes per lane of every square of a call
  uint64_t camhits_slots = 0;
  std::vector<unsigned char> camhits_key;   // what d_camhits holds the hits of, every square's (camera_hits_key); empty: nothing to reuse
  uint64_t camhit_passes = 0;        // camera-hit passes launched so far (lt_hip_camera_hit_passes)
  // The entry cuts of the stored hits' squares (lt_entry_cut_kernel): planes of one 64-byte record per square (launch_entry_cuts),
  // kept with the hits under camhits_key.
  uint32_t* d_cuts = nullptr;
  uint64_t cuts_squares = 0;         // the records d_cuts has room for: squares times planes
  bool cuts_valid = false;           // d_cuts holds the cuts of every square of the hits that camhits_key speaks of
  unsigned long long* d_cut_stats = nullptr;   // [0] squares with a non-empty list, [1] their entries: of the cuts d_cuts holds;
                                               // [2] squares marked clear, [3] squares with a list of leaves, [4] those lists' entries;
                                               // from [5] on the lists of several records (lt_entry_cut_kernel: kEntryCutStats in all)
  uint32_t cuts_leaves = 0;          // RenderKnobs::entry_cut_leaves of the build that made them (another value: built again)
  uint32_t cuts_chunks = 0;          // RenderKnobs::entry_cut_chunks of that build, likewise: the planes of d_cuts that it wrote
  uint32_t cuts_node_chunks = 0;     // RenderKnobs::entry_cut_node_chunks of that build, likewise
  uint32_t cuts_plane_squares = 0;   // FrameParams::totalSquares of that build: a plane of d_cuts is this many records
  uint64_t cut_builds = 0;          // launches of lt_entry_cut_kernel so far (lt_hip_entry_cut_counts)
  // The item table of those cuts and its fold map (lt_clear_items_kernel; ensure_clear_items): valid while cuts_valid is and for the
  // launches they were built for -- items_groups frame groups per square (0: none built since the cuts were), items_folds: with a map.
  uint32_t* d_items = nullptr;
  uint64_t items_words = 0;
  uint32_t* d_foldmap = nullptr;     // (bytes, four to a word: render_kernel_body reads words, lt_running_mean4_kernel bytes)
  uint64_t foldmap_words = 0;
  uint32_t items_groups = 0;
  bool items_folds = false;
  unsigned long long* d_item_stats = nullptr;   // [0] the table's entries, [1] the squares it hands out whole
  uint64_t item_builds = 0;          // launches of lt_clear_items_kernel so far
  // the work counters of the context's last render launch if it rendered whole squares in one pass (render_clear_square), whose
  // counters lie in the same lines (kClearCountAt), else null: lt_hip_clear_square_counts
  const uint32_t* last_clear_queues = nullptr;
  bool last_folded = false;          // some launch of the context's last render call was told to have the whole squares fold their own samples
  bool last_tabled = false;          // ... and some launch of it took the table (lt_hip_clear_item_counts)
  // Whether the table is worth taking is a matter of how many squares are clear, which only the device knows: the build's counters
  // come back by an asynchronous copy into pinned memory with an event behind it, and a later launch that finds the event done reads
  // them (ensure_clear_items).  -1: not known yet; dropped with the cuts.
  unsigned long long* h_item_stats = nullptr;
  hipEvent_t items_ev = nullptr;
  int items_worth = -1;
  uint64_t scene_generation = 0;     // goes up whenever a resident scene buffer or an array derived from one is written or given back
  hipEvent_t render_ev = nullptr;    // behind the last launch of the last render call, on render_stream: a render on another stream waits for it
  hipStream_t render_stream = nullptr;
  bool render_ev_recorded = false;
  uint64_t d_samples_bytes = 0;
  uint32_t* d_order = nullptr;       // persistent mode: hand-out order of the squares (slow-path squares first), cached
  uint64_t order_capacity = 0;
  std::vector<uint32_t> order_key;   // what d_order was built for
  uint32_t order_head[8] = {0};      // slow-path squares at the head of each XCD's share
  int cu_count = 256;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> mean_events;   // pairs around the running-mean kernels of the last call
  uint32_t mean_pairs = 0;
  bool pending = false, pending_stats = false;
  bool pending_query = false;        // ... and it is a ray query (lt_hip_trace_rays*): no render_ms
  lt_hip_stats last{};
  // ray queries (lt_query.hip): lt_query_kernel's eight work counters (kQueueStride apart), the host entry point's device copies
  // of the rays and the results, and an event behind the last query's launch (the next one waits for it before it zeroes the
  // counters: a query enqueued on another stream may still be running)
  uint32_t* d_query_ctl = nullptr;
  void* d_query_rays = nullptr;
  uint64_t query_rays_bytes = 0;
  uint4* d_surface_hits = nullptr;   // lt_hip_trace_surface*: the closest hits between its two launches
  uint64_t surface_hits_records = 0;
  void* d_query_out = nullptr;
  uint64_t query_out_bytes = 0;
  hipEvent_t query_ev = nullptr;
  // overlap lists (lt_overlist.hip): the scan's per-tile sums and, host entry points, the device copy of the items -- the offsets
  // are staged in d_query_out, which has to outlive the growth of the items between the call's two halves
  unsigned long long* d_list_partials = nullptr;
  uint64_t list_partials_words = 0;
  void* d_list_items = nullptr;
  uint64_t list_items_bytes = 0;
  // shaded rays (lt_shade.hip): lt_shade_rays_kernel's own eight work counters and the event behind its last launch, as above
  uint32_t* d_shade_ctl = nullptr;
  hipEvent_t shade_ev = nullptr;
  // wavefront GI pipeline: path queues, per-pixel direct / indirect / blend, control block (queue lengths, work counters)
  void* d_gi[17] = {nullptr};
  uint64_t gi_pixels = 0;
  uint32_t* d_giCtl = nullptr;
  // the GI programs over caller-supplied rays (lt_paths.hip): the camera hits of a range of rays, and the event behind the last
  // call's last launch (the next call waits for it before it touches the control block or the scratch above)
  uint4* d_paths_hits = nullptr;
  uint64_t paths_hits_rays = 0;
  hipEvent_t paths_ev = nullptr;
  // user programs (hipRTC), cached by path like the reference's programMap
  struct UserProgram { hipModule_t module; hipFunction_t lds, ldsStrict, ldsPortable; };   // one kernel per math flavour
  std::vector<UserProgram> user_programs;
  std::map<std::string, int> user_program_ids;
};

static thread_local std::string g_create_error;

#define LT_HIP_CHECK(ctx, call)                                                                     \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
      return LT_ERR_HIP;                                                                            \
    }                                                                                               \
  } while (0)

static int fail(lt_hip_context* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg; else g_create_error = msg;
  return code;
}

extern "C" int lt_hip_abi_version(void) { return LT_HIP_ABI_VERSION; }

extern "C" const char* lt_hip_last_error(const lt_hip_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

extern "C" int lt_hip_create(int device_index, lt_hip_context** out_ctx) {
  if (!out_ctx) return fail(nullptr, LT_ERR_INVALID_ARGUMENT, "out_ctx is NULL");
  *out_ctx = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(nullptr, LT_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
  if (device_index < 0 || device_index >= n) return fail(nullptr, LT_ERR_INVALID_ARGUMENT, "device_index out of range");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device_index)) != hipSuccess)
    return fail(nullptr, LT_ERR_NO_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(nullptr, LT_ERR_NO_DEVICE, std::string("kernels are built for gfx950 only; device is ") + prop.gcnArchName);
  lt_hip_context* ctx = new lt_hip_context();
  ctx->device = device_index;
  ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char* e = getenv("LT_SCENE_POOL_BYTES")) ctx->pool.cap = (size_t)strtoull(e, nullptr, 10);
  if (const char* e = getenv("LT_DEBUG_POISON")) ctx->pool.poison = (int)(strtoul(e, nullptr, 0) & 0xffu);
  auto bail = [&](const char* what, hipError_t er) {
    std::string m = std::string(what) + ": " + hipGetErrorString(er);
    delete ctx;
    return fail(nullptr, LT_ERR_HIP, m);
  };
  if ((e = hipSetDevice(device_index)) != hipSuccess) return bail("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
  if ((e = hipEventCreate(&ctx->ev0)) != hipSuccess) return bail("hipEventCreate", e);
  if ((e = hipEventCreate(&ctx->ev1)) != hipSuccess) return bail("hipEventCreate", e);
  if ((e = hipMalloc((void**)&ctx->d_stats, 9 * sizeof(unsigned long long))) != hipSuccess) return bail("hipMalloc", e);
  ctx->d_prep_flag = (uint32_t*)(ctx->d_stats + 8);
  {   // float32 denormals must be kept (lt_denormal_probe_kernel)
    const uint32_t in[2] = {1u, 0u};
    uint32_t out[2] = {0u, 0u};
    uint32_t* d = (uint32_t*)ctx->d_stats;
    if ((e = hipMemcpy(d, in, sizeof(in), hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy", e);
    hipLaunchKernelGGL(lt_denormal_probe_kernel, dim3(1), dim3(1), 0, ctx->stream, (const uint32_t*)d, d + 2);
    if ((e = hipGetLastError()) != hipSuccess) return bail("kernel launch (is this library built for gfx950?)", e);
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail("hipStreamSynchronize", e);
    if ((e = hipMemcpy(out, d + 2, sizeof(out), hipMemcpyDeviceToHost)) != hipSuccess) return bail("hipMemcpy", e);
    if (out[0] != 1u || out[1] != 2u) {
      (void)hipFree(ctx->d_stats);
      (void)hipEventDestroy(ctx->ev0);
      (void)hipEventDestroy(ctx->ev1);
      (void)hipStreamDestroy(ctx->stream);
      delete ctx;
      return fail(nullptr, LT_ERR_NO_DEVICE, "this build flushes float32 denormals to zero (-fgpu-flush-denormals-to-zero?): the walks' slab tests need them kept");
    }
  }
  *out_ctx = ctx;
  return LT_OK;
}

static void free_scene(lt_hip_context* ctx) {
  ctx->scene_generation++;
  for (void** p : {&ctx->d_nodes, &ctx->d_tris, &ctx->d_prims, &ctx->d_mats, &ctx->d_lights, &ctx->d_nodes2, &ctx->d_pairs2, &ctx->d_rank8, &ctx->d_wide}) {
    if (*p) ctx->pool.put(*p);
    *p = nullptr;
  }
  ctx->has_scene = false;
  ctx->device_prepared = false;
  ctx->height2 = 0;
  ctx->retree_ms = 0.0f;
}

extern "C" int lt_hip_destroy(lt_hip_context* ctx) {
  if (!ctx) return LT_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  free_scene(ctx);
  ctx->pool.clear();
  if (ctx->d_out) (void)hipFree(ctx->d_out);
  if (ctx->h_out) (void)hipHostFree(ctx->h_out);
  for (hipEvent_t e : ctx->out_ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->fold_ev) if (e) (void)hipEventDestroy(e);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->d_stats) (void)hipFree(ctx->d_stats);
  if (ctx->d_queues) (void)hipFree(ctx->d_queues);
  if (ctx->d_samples) (void)hipFree(ctx->d_samples);
  if (ctx->d_camhits) (void)hipFree(ctx->d_camhits);
  if (ctx->d_cuts) (void)hipFree(ctx->d_cuts);
  if (ctx->d_cut_stats) (void)hipFree(ctx->d_cut_stats);
  if (ctx->d_items) (void)hipFree(ctx->d_items);
  if (ctx->d_foldmap) (void)hipFree(ctx->d_foldmap);
  if (ctx->d_item_stats) (void)hipFree(ctx->d_item_stats);
  if (ctx->h_item_stats) (void)hipHostFree(ctx->h_item_stats);
  if (ctx->items_ev) (void)hipEventDestroy(ctx->items_ev);
  if (ctx->render_ev) (void)hipEventDestroy(ctx->render_ev);
  if (ctx->d_groupWalks) (void)hipFree(ctx->d_groupWalks);
  if (ctx->d_shadowq) (void)hipFree(ctx->d_shadowq);
  if (ctx->d_shadowCtl) (void)hipFree(ctx->d_shadowCtl);
  if (ctx->d_query_ctl) (void)hipFree(ctx->d_query_ctl);
  if (ctx->d_query_rays) (void)hipFree(ctx->d_query_rays);
  if (ctx->d_surface_hits) (void)hipFree(ctx->d_surface_hits);
  if (ctx->d_query_out) (void)hipFree(ctx->d_query_out);
  if (ctx->query_ev) (void)hipEventDestroy(ctx->query_ev);
  if (ctx->d_list_partials) (void)hipFree(ctx->d_list_partials);
  if (ctx->d_list_items) (void)hipFree(ctx->d_list_items);
  if (ctx->d_shade_ctl) (void)hipFree(ctx->d_shade_ctl);
  if (ctx->shade_ev) (void)hipEventDestroy(ctx->shade_ev);
  if (ctx->d_order) (void)hipFree(ctx->d_order);
  for (auto& up : ctx->user_programs) (void)hipModuleUnload(up.module);
  for (void*& b : ctx->d_gi) if (b) (void)hipFree(b);
  if (ctx->d_giCtl) (void)hipFree(ctx->d_giCtl);
  if (ctx->d_paths_hits) (void)hipFree(ctx->d_paths_hits);
  if (ctx->paths_ev) (void)hipEventDestroy(ctx->paths_ev);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  for (hipEvent_t e : ctx->mean_events) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->cal_ev) if (e) (void)hipEventDestroy(e);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return LT_OK;
}

extern "C" int lt_hip_program_from_path(const char* path, int* out_program) {
  if (!path || !out_program) return LT_ERR_INVALID_ARGUMENT;
  std::string p(path);
  size_t slash = p.find_last_of('/');
  std::string base = slash == std::string::npos ? p : p.substr(slash + 1);
  size_t dot = base.find_last_of('.');
  if (dot != std::string::npos) base = base.substr(0, dot);
  if (base == "basic") *out_program = LT_PROGRAM_BASIC;
  else if (base == "basic_lighting") *out_program = LT_PROGRAM_BASIC_LIGHTING;
  else if (base == "accumulator") *out_program = LT_PROGRAM_ACCUMULATOR;
  else if (base == "custom_opencl") *out_program = LT_PROGRAM_CUSTOM_OPENCL;
  else if (base == "global_illumination25") *out_program = LT_PROGRAM_GLOBAL_ILLUMINATION_25;
  else if (base == "global_illumination") {
    const bool shipped25 = p.find("resources/kernels/opencl/") != std::string::npos && p.find("examples/") == std::string::npos;
    *out_program = shipped25 ? LT_PROGRAM_GLOBAL_ILLUMINATION_25 : LT_PROGRAM_GLOBAL_ILLUMINATION;
  } else return LT_ERR_UNKNOWN_PROGRAM;
  return LT_OK;
}

// ---------------------------------------------------------------------------------- user programs (hipRTC)
// hipRTC is loaded on first use (dlopen), so the library has no link-time dependency on it.
namespace {
struct Hiprtc {
  void* lib = nullptr;
  int (*createProgram)(void**, const char*, const char*, int, const char**, const char**) = nullptr;
  int (*compileProgram)(void*, int, const char**) = nullptr;
  int (*getProgramLogSize)(void*, size_t*) = nullptr;
  int (*getProgramLog)(void*, char*) = nullptr;
  int (*getCodeSize)(void*, size_t*) = nullptr;
  int (*getCode)(void*, char*) = nullptr;
  int (*destroyProgram)(void**) = nullptr;
  bool load(std::string& err) {
    if (lib) return true;
    for (const char* name : {"libhiprtc.so.7", "libhiprtc.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) { err = "hipRTC library not found (libhiprtc.so)"; return false; }
#define LT_SYM(field, sym) field = reinterpret_cast<decltype(field)>(dlsym(lib, sym)); if (!field) { err = std::string("hipRTC symbol missing: ") + sym; return false; }
    LT_SYM(createProgram, "hiprtcCreateProgram") LT_SYM(compileProgram, "hiprtcCompileProgram")
    LT_SYM(getProgramLogSize, "hiprtcGetProgramLogSize") LT_SYM(getProgramLog, "hiprtcGetProgramLog")
    LT_SYM(getCodeSize, "hiprtcGetCodeSize") LT_SYM(getCode, "hiprtcGetCode") LT_SYM(destroyProgram, "hiprtcDestroyProgram")
#undef LT_SYM
    return true;
  }
};
Hiprtc g_hiprtc;

// directory of the device headers: <this library>/../csrc, or $LT_CSRC_DIR
std::string csrc_dir() {
  if (const char* e = getenv("LT_CSRC_DIR")) return e;
  Dl_info info;
  if (dladdr((const void*)&lt_hip_abi_version, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    const size_t slash = p.find_last_of('/');
    return (slash == std::string::npos ? std::string(".") : p.substr(0, slash)) + "/../csrc";
  }
  return "lens_trace_amd/csrc";
}
}  // namespace

static int compile_user_program(lt_hip_context* ctx, const std::string& path, int* out_program) {
  std::ifstream in(path);
  if (!in) return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "cannot read user program " + path);
  std::stringstream user;
  user << in.rdbuf();
  std::string err;
  if (!g_hiprtc.load(err)) return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, err);
  const std::string src = "#define LT_USER_PROGRAM 1\n#include \"lt_kernel.hpp\"\n#line 1 \"" + path + "\"\n" + user.str() +
      "\n#define LT_USER_KERNEL(name, DEEP, DEVLIBM) extern \"C\" __global__ __launch_bounds__(64) void name(SceneDev sc, FrameParams fp, float* out, unsigned long long* stats, uint32_t* queues) { render_kernel_body<kUser, Config<DEEP, false, DEVLIBM>>(sc, fp, out, stats, queues); }\n"
      "LT_USER_KERNEL(lt_user_kernel_lds, false, 2)\n"
      "LT_USER_KERNEL(lt_user_kernel_lds_strict, false, 1)\n"
      "LT_USER_KERNEL(lt_user_kernel_lds_portable, false, 0)\n";
  void* prog = nullptr;
  if (g_hiprtc.createProgram(&prog, src.c_str(), "lt_user_program.hip", 0, nullptr, nullptr) != 0)
    return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "hiprtcCreateProgram failed");
  const std::string inc = "-I" + csrc_dir();
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", inc.c_str()};
  const int rc = g_hiprtc.compileProgram(prog, 5, opts);
  size_t n = 0;
  std::string log;
  if (g_hiprtc.getProgramLogSize(prog, &n) == 0 && n > 1) {
    log.resize(n);
    g_hiprtc.getProgramLog(prog, &log[0]);
  }
  if (rc != 0) {
    g_hiprtc.destroyProgram(&prog);
    return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "user program " + path + " failed to compile:\n" + log);
  }
  std::vector<char> code;
  if (g_hiprtc.getCodeSize(prog, &n) != 0 || n == 0) { g_hiprtc.destroyProgram(&prog); return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "hiprtcGetCodeSize failed"); }
  code.resize(n);
  g_hiprtc.getCode(prog, code.data());
  g_hiprtc.destroyProgram(&prog);
  lt_hip_context::UserProgram up{};
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LT_HIP_CHECK(ctx, hipModuleLoadData(&up.module, code.data()));
  LT_HIP_CHECK(ctx, hipModuleGetFunction(&up.lds, up.module, "lt_user_kernel_lds"));
  LT_HIP_CHECK(ctx, hipModuleGetFunction(&up.ldsStrict, up.module, "lt_user_kernel_lds_strict"));
  LT_HIP_CHECK(ctx, hipModuleGetFunction(&up.ldsPortable, up.module, "lt_user_kernel_lds_portable"));
  ctx->user_programs.push_back(up);
  *out_program = LT_PROGRAM_USER_BASE + (int)ctx->user_programs.size() - 1;
  ctx->user_program_ids[path] = *out_program;
  return LT_OK;
}

extern "C" int lt_hip_resolve_program(lt_hip_context* ctx, const char* path, int* out_program) {
  if (!ctx || !path || !out_program) return LT_ERR_INVALID_ARGUMENT;
  if (lt_hip_program_from_path(path, out_program) == LT_OK) return LT_OK;
  const std::string p(path);
  if (p.size() < 5 || p.compare(p.size() - 4, 4, ".hip") != 0)
    return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "no built-in program for " + p + " (user programs are .hip files)");
  auto it = ctx->user_program_ids.find(p);
  if (it != ctx->user_program_ids.end()) { *out_program = it->second; return LT_OK; }
  return compile_user_program(ctx, p, out_program);
}

// The checks of the primitives' materials and of the light list (validate_scene, the edit path, the device path's pre-check): the
// error text, or nullptr.
static const char kTooManyLights[] = "more than 64 emissive triangles";
static const char* check_material_indices(const uint8_t* prims, uint32_t n_prims, uint32_t n_mats) {
  for (uint32_t i = 0; i < n_prims; i++) {
    int32_t m;
    memcpy(&m, prims + 76 * (size_t)i + 72, 4);
    if (m < 0 || (uint32_t)m >= n_mats) return "materialIndex out of range";
  }
  return nullptr;
}
static const char* check_lights(const uint8_t* lights, uint32_t n_prims) {
  uint32_t lc;
  memcpy(&lc, lights, 4);
  if (lc > 64) return kTooManyLights;
  for (uint32_t i = 0; i < lc; i++) {
    uint32_t p;
    memcpy(&p, lights + 4 + 4 * i, 4);
    if (p >= n_prims) return "light primitive out of range";
  }
  return nullptr;
}

// Host-side validation: nothing with an out-of-range index or a cycle may reach a kernel.
// Returns the BVH height (max number of interior ancestors of a node) or -1 with msg set.
static int validate_scene(const uint8_t* nodes, uint32_t n_nodes, const uint8_t* prims, uint32_t n_prims, uint32_t n_mats,
                          const uint8_t* lights, std::string& msg) {
  struct N { float lo[3], hi[3]; int32_t off; uint16_t cnt; uint8_t axis, pad; };
  static_assert(sizeof(N) == 32, "LinearBVHNode is 32 bytes");
  const N* nd = reinterpret_cast<const N*>(nodes);
  for (uint32_t i = 0; i < n_nodes; i++) {
    if (nd[i].cnt > 0) {
      if (nd[i].off < 0 || (uint32_t)nd[i].off >= n_prims) { msg = "leaf primitivesOffset out of range"; return -1; }
    } else {
      // pre-order layout: left child = i+1, right child = secondChildOffset > i+1; forward-only => no cycles
      if (i + 1 >= n_nodes || nd[i].off <= (int32_t)i + 1 || (uint32_t)nd[i].off >= n_nodes) { msg = "interior node children out of range"; return -1; }
      if (nd[i].axis > 2) { msg = "split axis out of range"; return -1; }
    }
  }
  const char* why = check_material_indices(prims, n_prims, n_mats);
  if (!why) why = check_lights(lights, n_prims);
  if (why) { msg = why; return -1; }
  // height by forward propagation (children always have larger indices than their parent)
  std::vector<int> depth(n_nodes, -1);
  depth[0] = 0;
  int height = 0;
  for (uint32_t i = 0; i < n_nodes; i++) {
    if (depth[i] < 0) continue;   // unreachable node: harmless
    if (depth[i] > height) height = depth[i];
    if (nd[i].cnt == 0) {   // (max: a malformed buffer may share a child between parents; the LDS stack is sized by this height)
      depth[i + 1] = std::max(depth[i + 1], depth[i] + 1);
      depth[nd[i].off] = std::max(depth[nd[i].off], depth[i] + 1);
    }
  }
  return height;
}

// Host threads for the memory-bound host passes of lt_hip_set_scene (content hash): what the process may run on
// (sched_getaffinity: a container's CPU share, not the machine's core count), at most 16 unless LT_HOST_THREADS says otherwise
// (140 MB on the GPU box's host: 2.5 ms on 2 threads, 0.85 on 8, 0.70 on 12-16, 1.1 on 32 -- starting a thread costs what it
// hashes in 30 microseconds; tests/tools/hash_threads.py).
static int host_threads() {
  cpu_set_t set;
  int n = 1;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(16, CPU_COUNT(&set));
  if (const char* e = getenv("LT_HOST_THREADS")) n = atoi(e);
  return std::max(1, std::min(64, n));
}

// 64-bit content hash of a host buffer: four independent multiply-rotate lanes over 32-byte blocks, per 4 MiB piece; the pieces'
// hashes are folded in order, so the value does not depend on how many threads computed them (one pass over host memory at the
// memory system's rate: the four scene buffers of the 1 M-triangle scene, 140 MB, take a few milliseconds on the GPU box's
// host; bench.py's e2e figures measure it).  Used to tell "the same scene again" from "a buffer was edited in place" without an upload.
static uint64_t hash_piece(const uint8_t* b, uint64_t n, uint64_t seed) {
  constexpr uint64_t K = 0x9E3779B97F4A7C15ull;
  uint64_t h[4] = {seed ^ K, seed + 0xC2B2AE3D27D4EB4Full, seed ^ 0x165667B19E3779F9ull, seed + 0x27D4EB2F165667C5ull};
  auto block = [&](const uint8_t* q) {
    uint64_t w[4];
    memcpy(w, q, 32);
    for (int k = 0; k < 4; k++) {
      h[k] = (h[k] ^ w[k]) * K;
      h[k] = (h[k] << 29) | (h[k] >> 35);
    }
  };
  uint64_t i = 0;
  for (; i + 32 <= n; i += 32) block(b + i);
  if (i < n) {
    uint8_t tail[32] = {0};
    memcpy(tail, b + i, (size_t)(n - i));
    block(tail);
  }
  uint64_t r = n * K;
  for (int k = 0; k < 4; k++) {
    r = (r ^ h[k]) * K;
    r ^= r >> 32;
  }
  return r;
}

// The four scene buffers as one list of pieces, hashed by up to host_threads() threads (fewer when threads cannot be had: the
// pieces left are hashed by this one).
static SceneHash hash_scene(const void* const bufs[4], const uint64_t sizes[4]) {
  constexpr uint64_t kPiece = 4ull << 20;
  struct Piece { const uint8_t* p; uint64_t n; int of; };
  std::vector<Piece> pieces;
  for (int k = 0; k < 4; k++)
    for (uint64_t off = 0; off < sizes[k]; off += kPiece) pieces.push_back({(const uint8_t*)bufs[k] + off, std::min(kPiece, sizes[k] - off), k});
  std::vector<uint64_t> hashes(pieces.size());
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < pieces.size();) hashes[i] = hash_piece(pieces[i].p, pieces[i].n, (uint64_t)i);
  };
  std::vector<std::thread> pool;
  const int threads = (int)std::min<size_t>((size_t)host_threads(), pieces.size());
  try {
    for (int t = 1; t < threads; t++) pool.emplace_back(work);
  } catch (...) {   // (no more threads to be had: whoever exists does the work)
  }
  work();
  for (std::thread& th : pool) th.join();
  SceneHash r;
  for (int k = 0; k < 4; k++) r.buf[k] = 0x243F6A8885A308D3ull + (uint64_t)k;
  for (size_t i = 0; i < pieces.size(); i++) {
    uint64_t& b = r.buf[pieces[i].of];
    b = (b ^ hashes[i]) * 0x9E3779B97F4A7C15ull;
    b ^= b >> 29;
  }
  return r;
}

extern "C" int lt_hip_own_hierarchy(const void* nodes, uint64_t node_bytes, int height_slack, void* out_nodes, uint64_t out_bytes,
                                    uint32_t* rank8, uint32_t n_prims) {
  if (!nodes || node_bytes == 0 || node_bytes % 32 || node_bytes > 0xffffffffull) return -1;
  const uint32_t n_nodes = (uint32_t)(node_bytes / 32);
  {   // the same structural checks lt_hip_set_scene makes before it looks at a buffer (indices in range, forward-only children)
    const lt_retree::Node* nd = (const lt_retree::Node*)nodes;
    for (uint32_t i = 0; i < n_nodes; i++) {
      if (nd[i].cnt != 0) { if (nd[i].off < 0 || (rank8 && (uint32_t)nd[i].off >= n_prims)) return -1; }
      else if (i + 1 >= n_nodes || nd[i].off <= (int32_t)i + 1 || (uint32_t)nd[i].off >= n_nodes || nd[i].axis > 2) return -1;
    }
  }
  std::vector<lt_retree::Node> own;
  const int h = height_slack < 0 ? lt_retree::copy(nodes, n_nodes, 30, own) : lt_retree::build(nodes, n_nodes, 30, height_slack, own);
  if (h < 0) return -1;
  if (out_nodes) {
    if (out_bytes < own.size() * sizeof(lt_retree::Node)) return -1;
    memcpy(out_nodes, own.data(), own.size() * sizeof(lt_retree::Node));
  }
  if (rank8) {
    std::vector<uint32_t> r;
    lt_retree::reference_order(nodes, n_nodes, n_prims, r);
    memcpy(rank8, r.data(), r.size() * sizeof(uint32_t));
  }
  return h;
}

extern "C" int lt_hip_own_wide(const void* own_nodes, uint64_t node_bytes, uint32_t n_prims, float* origin_step, void* out_slots, uint64_t out_bytes,
                               uint32_t* out_groups) {
  if (!own_nodes || !origin_step || !out_slots || !out_groups || node_bytes == 0 || node_bytes % 32 || node_bytes > 0xffffffffull) return -1;
  const uint32_t n = (uint32_t)(node_bytes / 32);
  const lt_retree::Node* src = (const lt_retree::Node*)own_nodes;
  if (n < 3 || src[0].cnt != 0) return -1;
  for (uint32_t i = 0; i < n; i++)   // (a pre-order tree: children behind their parent, in range)
    if (src[i].cnt == 0 && (i + 1 >= n || src[i].off <= (int32_t)i + 1 || (uint32_t)src[i].off >= n)) return -1;
  const std::vector<lt_retree::Node> own(src, src + n);
  std::vector<uint32_t> children, groupOf;
  const int height = lt_retree::collapse_wide(own, n_prims, children, groupOf);
  if (height < 0) return -1;
  const uint32_t groups = (uint32_t)(children.size() / 4);
  if (out_bytes < (uint64_t)groups * 64) return -1;
  for (int a = 0; a < 3; a++) lt_own16::frame(own[0].lo[a], own[0].hi[a], origin_step[a], origin_step[3 + a]);
  lt_own16::Rec* out = (lt_own16::Rec*)out_slots;
  bool ok = true;
  for (size_t i = 0; i < children.size(); i++) {
    const uint32_t c = children[i];
    out[i] = lt_own16::empty_slot(groups, n_prims);
    if (c == 0xffffffffu) continue;
    const uint32_t link = own[c].cnt != 0 ? (0x80000000u | (groups + (uint32_t)own[c].off)) : groupOf[c];
    ok = lt_own16::slot_record(own[c].lo, own[c].hi, link, origin_step, origin_step + 3, out[i]) && ok;
  }
  *out_groups = groups;
  return ok ? height : -1;
}

// Set, to a number that reads 0: how most switches are turned off.
static bool env_off(const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; }

// The knobs of scene preparation, read once at the top of every public call that may install a scene (tests change them between
// the calls on one context).
struct SceneKnobs {
  int device = -1;          // LT_DEVICE_BUILD=0 / 1: prepare on the device never / whenever possible; unset (-1): by the scene's size
  bool own_splits = !env_off("LT_RETREE");   // off: the own structures keep the caller's splits
  int slack = 2;            // LT_RETREE_SLACK: levels the own tree may have beyond the least height possible
  bool always_upload = getenv("LT_SCENE_ALWAYS_UPLOAD") != nullptr;   // the resident scene is uploaded again when it is handed over
  bool retime = getenv("LT_RETIME_EVERY_SCENE") != nullptr;           // every scene forgets the shadow-walk verdicts (adopt_scene)
  bool timing = getenv("LT_DEBUG_SCENE_TIMING") != nullptr;           // SceneLaps
  SceneKnobs() {
    if (const char* e = getenv("LT_DEVICE_BUILD")) device = atoi(e) != 0;
    if (const char* e = getenv("LT_RETREE_SLACK")) slack = atoi(e);
  }
};

// The lap timer of one set_scene_impl call: LT_DEBUG_SCENE_TIMING prints the host time of every step, and of the whole call, to stderr.
struct SceneLaps {
  const bool timing;
  std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now(), mark = start;
  ~SceneLaps() { mark = start; lap("lt_hip_set_scene, all of it"); }
  void lap(const char* what) {
    const auto now = std::chrono::steady_clock::now();
    if (timing) fprintf(stderr, "[lt set_scene] %-28s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(now - mark).count());
    mark = now;
  }
};

// The own structures as either build leaves them, in device memory from the pool: the own tree and the leaf order table, which
// install_own_structures hands to the context, and collapse_wide's `children` / `groupOf`, which the builder gives back.
struct OwnBuild {
  void *d_nodes2, *d_rank8;
  const void *d_children, *d_groupOf;
  uint32_t n_nodes2, groups;
  int height, wide_height;              // of the own tree; of its 4-wide groups (-1: none)
  const float *root_lo, *root_hi;       // the own tree's root box: the grid of the per-lane walks' records
};

// Makes the per-lane walks' group records and the own structures resident -- or, when the walks cannot use them, gives all of them
// back (the renderer takes them all or none): the scene then walks the caller's tree.  The leaf records are remake_leaf_records'.
static int install_own_structures(lt_hip_context* ctx, const OwnBuild& b, uint32_t n_prims) {
  ctx->scene_generation++;
  ctx->d_nodes2 = b.d_nodes2;
  ctx->d_rank8 = b.d_rank8;
  // (the walk's stack: at most three waiting entries per level of groups and the four of the last one; the records' links: 31 bits)
  bool ok = b.wide_height >= 0 && b.groups > 0 && 3 * b.wide_height + 4 <= kOwnRows + kOwnDeep && (uint64_t)b.groups + n_prims + 1 < 0x7fffffffull;
  if (ok) {
    Own16Frame fr;
    for (int a = 0; a < 3; a++) lt_own16::frame(b.root_lo[a], b.root_hi[a], fr.O[a], fr.S[a]);
    LT_HIP_CHECK(ctx, ctx->pool.get(&ctx->d_pairs2, (size_t)b.n_nodes2 * 64));
    LT_HIP_CHECK(ctx, ctx->pool.get(&ctx->d_wide, ((size_t)b.groups + n_prims + 1) * 64 + 64));   // (64 bytes in front: the grid, read by the walks themselves)
    const float head[16] = {0, 0, 0, 0, 0, 0, 0, 0, fr.O[0], fr.O[1], fr.O[2], 0.0f, fr.S[0], fr.S[1], fr.S[2], 0.0f};
    LT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_wide, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_prep_flag, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(lt_wide_kernel, dim3((4 * b.groups + 255) / 256), dim3(256), 0, ctx->stream, (const float4*)ctx->d_nodes2,
                       (const uint32_t*)b.d_children, (const uint32_t*)b.d_groupOf, (uint4*)ctx->d_wide + 4, b.groups, n_prims, fr, ctx->d_prep_flag);
    LT_HIP_CHECK(ctx, hipGetLastError());
    uint32_t bad = 0;
    LT_HIP_CHECK(ctx, hipMemcpyAsync(&bad, ctx->d_prep_flag, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ok = bad == 0;   // (a bound off the grid cannot happen for a grid sized from the root's box)
  }
  if (!ok) {
    for (void** p : {&ctx->d_nodes2, &ctx->d_pairs2, &ctx->d_wide, &ctx->d_rank8}) { ctx->pool.put(*p); *p = nullptr; }
    return LT_OK;
  }
  ctx->n_nodes2 = b.n_nodes2;
  ctx->height2 = b.height;
  ctx->n_wide = b.groups;
  ctx->wide_height = b.wide_height;
  return LT_OK;
}

// What is made from the resident primitives: the traversal triangles and, with the own structures, the leaf records of both walks
// (the packet walks' pairs, the per-lane walks' records behind the groups).  Both builds run it, and an edit of the primitives.
static int remake_leaf_records(lt_hip_context* ctx, uint32_t n_prims) {
  ctx->scene_generation++;
  hipLaunchKernelGGL(lt_retile_kernel, dim3((n_prims + 255) / 256), dim3(256), 0, ctx->stream, (const float*)ctx->d_prims, (float4*)ctx->d_tris, n_prims);
  if (ctx->d_nodes2 && ctx->d_pairs2 && ctx->d_wide) {
    const uint32_t n2 = ctx->n_nodes2;
    hipLaunchKernelGGL(lt_own_pair_kernel, dim3((n2 + 255) / 256), dim3(256), 0, ctx->stream, (const float4*)ctx->d_nodes2, (const float*)ctx->d_prims,
                       (float4*)ctx->d_pairs2, n2);
    hipLaunchKernelGGL(lt_wide_leaf_kernel, dim3((n2 + 1 + 255) / 256), dim3(256), 0, ctx->stream, (const float4*)ctx->d_nodes2, (const float*)ctx->d_prims,
                       (float4*)((uint4*)ctx->d_wide + 4), n2, ctx->n_wide, n_prims);
  }
  LT_HIP_CHECK(ctx, hipGetLastError());
  return LT_OK;
}

// The scene is resident: its sizes and hash (what the next call is compared with), the caller's tree's height, who prepared it.
static void adopt_scene(lt_hip_context* ctx, const uint64_t sizes[4], const SceneHash& hash, int bvh_height, bool device_prepared, const SceneKnobs& k) {
  ctx->n_nodes = (uint32_t)(sizes[0] / 32);
  ctx->n_prims = (uint32_t)(sizes[1] / 76);
  ctx->n_mats = (uint32_t)(sizes[2] / 32);
  ctx->bvh_height = bvh_height;
  ctx->has_scene = true;
  ctx->device_prepared = device_prepared;
  ctx->scene_hash = hash;
  ctx->scene_hash_valid = true;
  memcpy(ctx->scene_sizes, sizes, sizeof(ctx->scene_sizes));
  ctx->scene_uploads++;
  ctx->scene_generation++;   // (every path that wrote a scene buffer ends here; those that write without it -- a failed edit -- count below)
  // The shadow-ray walk timed fastest for a scene (render_on_stream) is kept for a scene of the same shape -- the next pose of an
  // animation, an edited material: it is a matter of speed, never of pixels, and timing it again costs five frames -- and forgotten
  // when the sizes change (another scene).
  if (ctx->verdict_sizes_valid && memcmp(sizes, ctx->verdict_sizes, sizeof(ctx->verdict_sizes)) == 0 && !k.retime) return;
  for (int& m : ctx->shadow_mode) m = -1;
  ctx->shadow_modes.clear();
  ctx->shadow_groups.clear();
  memcpy(ctx->verdict_sizes, sizes, sizeof(ctx->verdict_sizes));
  ctx->verdict_sizes_valid = true;
}

// The device path of lt_hip_set_scene.  kDeviceDeclined: nothing of ctx was touched, the host path decides.
constexpr int kDeviceDeclined = -1000;
template <class Arrived>
static int prepare_resident(lt_hip_context* ctx, void*& d_nodes, void*& d_prims, const void* materials, const void* lights, hipMemcpyKind kind,
                            const uint64_t sizes[4], const SceneHash& hash, const SceneKnobs& k, SceneLaps& laps, Arrived primsArrived);

static int set_scene_on_device(lt_hip_context* ctx, const void* nodes, const void* prims, const void* materials, const void* lights,
                               const uint64_t sizes[4], const SceneHash& hash, const SceneKnobs& k, SceneLaps& laps) {
  const uint32_t n_prims = (uint32_t)(sizes[1] / 76);
  if (check_lights((const uint8_t*)lights, n_prims)) return kDeviceDeclined;   // (the light list is 260 bytes: checked here; the host words the error)
  void *d_nodes = nullptr, *d_prims = nullptr;
  struct Guard {   // (whatever is still set when this returns goes back)
    ScenePool& pool; void** a; void** b;
    ~Guard() { pool.put(*a); pool.put(*b); }
  };
  Guard guard{ctx->pool, &d_nodes, &d_prims};
  LT_HIP_CHECK(ctx, ctx->pool.upload(&d_nodes, nodes, sizes[0]));
  LT_HIP_CHECK(ctx, ctx->pool.get(&d_prims, sizes[1]));
  laps.lap("upload nodes");
  // The hierarchy is built from the nodes alone: the primitives (the larger buffer) travel meanwhile, sent by a thread of their
  // own (a copy from pageable memory keeps its caller until it is done) -- or, if that thread cannot be had, right here.
  std::thread primThread;
  hipError_t primError = hipSuccess;
  try {
    primThread = std::thread([&]() {
      primError = hipSetDevice(ctx->device);
      if (primError == hipSuccess) primError = hipMemcpy(d_prims, prims, sizes[1], hipMemcpyHostToDevice);
    });
  } catch (...) {
    primError = hipMemcpy(d_prims, prims, sizes[1], hipMemcpyHostToDevice);
  }
  struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{primThread};   // (every exit below waits for it)
  return prepare_resident(ctx, d_nodes, d_prims, materials, lights, hipMemcpyHostToDevice, sizes, hash, k, laps, [&]() {
    if (primThread.joinable()) primThread.join();
    return primError;
  });
}

// The second half of the device path: d_nodes and d_prims are pool buffers on the device (the primitives may still be on their
// way: primsArrived waits for them), materials and lights are copied from wherever `kind` says they are.  On success the two
// buffers are the context's and the pointers null; kDeviceDeclined: nothing of ctx was touched and they are still the caller's.
template <class Arrived>
static int prepare_resident(lt_hip_context* ctx, void*& d_nodes, void*& d_prims, const void* materials, const void* lights, hipMemcpyKind kind,
                            const uint64_t sizes[4], const SceneHash& hash, const SceneKnobs& k, SceneLaps& laps, Arrived primsArrived) {
  const uint32_t n_nodes = (uint32_t)(sizes[0] / 32), n_prims = (uint32_t)(sizes[1] / 76), n_mats = (uint32_t)(sizes[2] / 32);
  const lt_prep::Allocator al{&ctx->pool, &ScenePool::get_cb, &ScenePool::put_cb};
  struct Guard { const lt_prep::Allocator& al; lt_prep::Out* o; ~Guard() { lt_prep::release(*o, al); } };
  lt_prep::Out prep;
  Guard guard{al, &prep};
  const auto t0 = std::chrono::steady_clock::now();
  // (height <= 30: the packet walks' stack, one VGPR, holds 2 * height + 2 entries at most; LT_RETREE=0: the caller's splits)
  LT_HIP_CHECK(ctx, lt_prep::run(d_nodes, n_nodes, nullptr, n_prims, n_mats, 30, k.slack, k.own_splits, ctx->stream, al, prep));
  if (k.timing) fprintf(stderr, "[lt set_scene] device: checks + leaf order %.2f ms, own hierarchy %.2f ms (%d levels), 4-wide groups %.2f ms, flags %u\n",
                        prep.ms_check, prep.ms_build, prep.levels, prep.ms_wide, prep.flags);
  if (prep.flags != 0 || prep.bvh_height > kMaxStack) return kDeviceDeclined;
  laps.lap("device preparation");
  LT_HIP_CHECK(ctx, primsArrived());
  bool primsOk = false;
  LT_HIP_CHECK(ctx, lt_prep::check_primitives(d_prims, n_prims, n_mats, ctx->stream, ctx->d_prep_flag, primsOk));
  if (!primsOk) return kDeviceDeclined;
  laps.lap("primitives arrived, checked");
  // from here on the scene is good: it replaces the resident one
  LT_HIP_CHECK(ctx, hipDeviceSynchronize());
  free_scene(ctx);
  ctx->d_nodes = d_nodes; d_nodes = nullptr;
  ctx->d_prims = d_prims; d_prims = nullptr;
  LT_HIP_CHECK(ctx, ctx->pool.get(&ctx->d_tris, (size_t)n_prims * 48));
  LT_HIP_CHECK(ctx, ctx->pool.get(&ctx->d_mats, sizes[2]));
  LT_HIP_CHECK(ctx, ctx->pool.get(&ctx->d_lights, sizes[3]));
  LT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_mats, materials, sizes[2], kind, ctx->stream));
  LT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_lights, lights, sizes[3], kind, ctx->stream));
  const OwnBuild own{prep.d_nodes2, prep.d_rank8, prep.d_children, prep.d_groupOf, prep.n_own, prep.groups, prep.own_height, prep.wide_height,
                     prep.root_lo, prep.root_hi};
  prep.d_nodes2 = prep.d_rank8 = nullptr;   // (the context's from here on; the guard gives back the rest)
  int rc = install_own_structures(ctx, own, n_prims);
  if (rc == LT_OK) rc = remake_leaf_records(ctx, n_prims);
  if (rc) return rc;
  LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->retree_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  laps.lap("own structures, leaf records");
  adopt_scene(ctx, sizes, hash, prep.bvh_height, true, k);
  return LT_OK;
}

static int set_scene_impl(lt_hip_context* ctx, const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes, const void* materials,
                          uint64_t material_bytes, const void* lights, uint64_t light_bytes, const SceneKnobs& k, const SceneHash* known_hash) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  if (!nodes || !prims || !materials || !lights) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "NULL scene buffer");
  if (node_bytes == 0 || node_bytes % 32 || prim_bytes == 0 || prim_bytes % 76 || material_bytes == 0 || material_bytes % 32 ||
      light_bytes != 260)
    return fail(ctx, LT_ERR_BAD_SCENE, "scene buffer sizes are not whole multiples of LinearBVHNode(32) / Primitive(76) / Material(32) / LightContainer(260)");
  if (node_bytes > 0xffffffffull || prim_bytes / 76 > 0x7fffffffull / 48) return fail(ctx, LT_ERR_BAD_SCENE, "scene too large for 32-bit byte offsets (4 GiB of nodes / 2 GiB of traversal triangles)");
  SceneLaps laps{k.timing};
  const uint32_t n_nodes = (uint32_t)(node_bytes / 32), n_prims = (uint32_t)(prim_bytes / 76), n_mats = (uint32_t)(material_bytes / 32);
  // The reference uploads all buffers on every render() (renderer_opencl.cpp:107-120); here the resident copy is kept when the
  // caller hands over the same content again: sizes and a hash of EVERY byte (so an in-place edit of any vertex, node or
  // material is honoured).  LT_SCENE_ALWAYS_UPLOAD=1 turns the shortcut off.
  const uint64_t sizes[4] = {node_bytes, prim_bytes, material_bytes, light_bytes};
  const void* const bufs[4] = {nodes, prims, materials, lights};
  const SceneHash hash = known_hash ? *known_hash : hash_scene(bufs, sizes);
  laps.lap(known_hash ? "hash (known)" : "hash");
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (ctx->has_scene && ctx->scene_hash_valid && memcmp(sizes, ctx->scene_sizes, sizeof(sizes)) == 0 && !k.always_upload) {
    if (hash == ctx->scene_hash) {
      ctx->scene_reused++;
      return LT_OK;
    }
    // An edit that left the nodes alone -- a material, a light, a primitive's normals or material index -- leaves the hierarchies
    // alone too: the buffers that changed are uploaded, and what is derived from the primitives (traversal triangles, the leaf
    // records of both walks) is made again by the kernels that made it: no host-side build, no second copy of the tree.
    if (hash.buf[0] == ctx->scene_hash.buf[0]) {
      const bool primsChanged = hash.buf[1] != ctx->scene_hash.buf[1];
      // (of several defects, this path has always named a light count over 64 first, then a materialIndex, then a light's primitive)
      const char* why = check_lights((const uint8_t*)lights, n_prims);
      const char* badMaterial = primsChanged ? check_material_indices((const uint8_t*)prims, n_prims, n_mats) : nullptr;
      if (badMaterial && why != kTooManyLights) why = badMaterial;
      if (why) return fail(ctx, LT_ERR_BAD_SCENE, why);
      LT_HIP_CHECK(ctx, hipDeviceSynchronize());   // (nothing of an earlier call may still be reading what is about to change)
      ctx->scene_generation++;
      if (primsChanged) {
        LT_HIP_CHECK(ctx, hipMemcpy(ctx->d_prims, prims, prim_bytes, hipMemcpyHostToDevice));
        const int rc = remake_leaf_records(ctx, n_prims);
        if (rc) return rc;
      }
      LT_HIP_CHECK(ctx, hipMemcpy(ctx->d_mats, materials, material_bytes, hipMemcpyHostToDevice));
      LT_HIP_CHECK(ctx, hipMemcpy(ctx->d_lights, lights, light_bytes, hipMemcpyHostToDevice));
      LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
      adopt_scene(ctx, sizes, hash, ctx->bvh_height, ctx->device_prepared, k);
      return LT_OK;
    }
  }
  // Scene preparation on the device (lt_prep.hip): nodes and primitives go up first, kernels check them, make the leaf order
  // table, build the own hierarchy and collapse it; the host passes below are what remains for scenes that path declines
  // (a malformed buffer -- the host words the error --, a tree that is not in the scene builder's pre-order, boxes that do not
  // nest) and for small ones, where a host build costs less than the launches.
  if (k.device < 0 ? n_nodes >= 8192u : k.device != 0) {
    const int rc = set_scene_on_device(ctx, nodes, prims, materials, lights, sizes, hash, k, laps);
    if (rc != kDeviceDeclined) return rc;
    laps.lap("device preparation declined");
  }
  std::string msg;
  const int height = validate_scene((const uint8_t*)nodes, n_nodes, (const uint8_t*)prims, n_prims, n_mats, (const uint8_t*)lights, msg);
  laps.lap("validate");
  if (height < 0) return fail(ctx, LT_ERR_BAD_SCENE, msg);
  if (height > kMaxStack) return fail(ctx, LT_ERR_BAD_SCENE, "BVH deeper than the reference's 64-entry traversal stack");
  LT_HIP_CHECK(ctx, hipDeviceSynchronize());
  free_scene(ctx);
  LT_HIP_CHECK(ctx, ctx->pool.upload(&ctx->d_nodes, nodes, node_bytes));
  LT_HIP_CHECK(ctx, ctx->pool.upload(&ctx->d_prims, prims, prim_bytes));
  LT_HIP_CHECK(ctx, ctx->pool.get(&ctx->d_tris, (size_t)n_prims * 48));
  LT_HIP_CHECK(ctx, ctx->pool.upload(&ctx->d_mats, materials, material_bytes));
  LT_HIP_CHECK(ctx, ctx->pool.upload(&ctx->d_lights, lights, light_bytes));
  laps.lap("free, malloc, upload scene");
  // The backend's own hierarchy over the same leaves (lt_retree.hpp says why the pixels cannot change), for every finite ray of
  // the non-counting kernels.  LT_RETREE=0 keeps the caller's splits (same structures, same walks).  A scene whose boxes do not
  // nest gets none: its rays walk the caller's tree one by one, in the reference's order.
  {
    const auto t0 = std::chrono::steady_clock::now();
    // (the leaf order table depends on the caller's tree alone: it is made by a thread of its own beside the build -- or, if that
    // thread cannot be had, after it)
    std::vector<uint32_t> rank8;
    std::thread rankThread;
    std::atomic<bool> rankMade{false};
    try {
      rankThread = std::thread([&]() {
        try { lt_retree::reference_order(nodes, n_nodes, n_prims, rank8); rankMade = true; } catch (...) {}   // (nothing escapes a thread)
      });
    } catch (...) {
    }
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{rankThread};   // (every exit below waits for it)
    std::vector<lt_retree::Node> own;
    // (height <= 30: the packet walks' stack, one VGPR, holds 2 * height + 2 entries at most; LT_RETREE=0: the caller's splits)
    const int h2 = k.own_splits ? lt_retree::build(nodes, n_nodes, 30, k.slack, own) : lt_retree::copy(nodes, n_nodes, 30, own);
    laps.lap("own hierarchy (host build)");
    if (h2 >= 0) {
      std::vector<uint32_t> children, groupOf;
      const int hw = lt_retree::collapse_wide(own, n_prims, children, groupOf);
      if (rankThread.joinable()) rankThread.join();
      if (!rankMade) lt_retree::reference_order(nodes, n_nodes, n_prims, rank8);
      laps.lap("4-wide groups, leaf order");
      void *d_children = nullptr, *d_groupOf = nullptr;
      LT_HIP_CHECK(ctx, ctx->pool.upload(&ctx->d_nodes2, own.data(), own.size() * sizeof(lt_retree::Node)));
      LT_HIP_CHECK(ctx, ctx->pool.upload(&ctx->d_rank8, rank8.data(), rank8.size() * sizeof(uint32_t)));
      LT_HIP_CHECK(ctx, ctx->pool.upload(&d_children, children.data(), children.size() * sizeof(uint32_t)));
      LT_HIP_CHECK(ctx, ctx->pool.upload(&d_groupOf, groupOf.data(), groupOf.size() * sizeof(uint32_t)));
      const OwnBuild b{ctx->d_nodes2, ctx->d_rank8, d_children, d_groupOf, (uint32_t)own.size(), (uint32_t)(children.size() / 4), h2, hw,
                       own[0].lo, own[0].hi};
      const int rc = install_own_structures(ctx, b, n_prims);
      ctx->pool.put(d_children);
      ctx->pool.put(d_groupOf);
      if (rc) return rc;
      ctx->retree_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
      laps.lap("own structures (upload, groups)");
    }
  }
  const int rc = remake_leaf_records(ctx, n_prims);
  if (rc) return rc;
  LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  adopt_scene(ctx, sizes, hash, height, false, k);
  return LT_OK;
}

extern "C" int lt_hip_set_scene(lt_hip_context* ctx, const void* nodes, uint64_t node_bytes, const void* prims,
                                uint64_t prim_bytes, const void* materials, uint64_t material_bytes, const void* lights,
                                uint64_t light_bytes) {
  try {
    return set_scene_impl(ctx, nodes, node_bytes, prims, prim_bytes, materials, material_bytes, lights, light_bytes, SceneKnobs(), nullptr);
  } catch (const std::exception& e) {   // (std::bad_alloc, std::system_error of a thread: nothing may cross the C ABI)
    return fail(ctx, LT_ERR_HIP, std::string("lt_hip_set_scene: ") + e.what());
  }
}

// ---------------------------------------------------------------------------------- scenes from bare triangles
// lt_hip_set_triangles / _device: the caller's tree, the ordered primitives and the light container are built on the device by the
// canonical median rule (lt_build.hip) and handed to the second half of the device path; lt_hip_build_scene_host is the same rule
// on the host, lt_hip_read_scene_buffer reads the four resident buffers back.
static_assert(sizeof(lt_hip_triangles_desc) == 56, "triangle descriptor (include/lenstrace_hip.h)");

// The argument rules of the three forms, in the header's order.
static int check_triangles_desc(lt_hip_context* ctx, const lt_hip_triangles_desc* d, bool device, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, w + "NULL desc");
  if (d->struct_size < sizeof(lt_hip_triangles_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, w + "struct_size too small");
  if (d->flags != 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, w + "unknown flags");
  if (d->n == 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, w + "no triangles");
  if (!d->positions || !d->normals || !d->materials) return fail(ctx, LT_ERR_INVALID_ARGUMENT, w + "NULL positions, normals or materials");
  if (d->material_bytes == 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, w + "zero materials");
  if (device && (((uintptr_t)d->positions | (uintptr_t)d->normals | (uintptr_t)d->material_indices | (uintptr_t)d->materials) & 3u))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, w + "device pointers must be 4-byte aligned");
  if (d->material_bytes % 32 || d->material_bytes / 32 > 0x7fffffffull)
    return fail(ctx, LT_ERR_BAD_SCENE, "scene buffer sizes are not whole multiples of LinearBVHNode(32) / Primitive(76) / Material(32) / LightContainer(260)");
  if (d->n > 0x7fffffffull / 48 || 32 * (2 * d->n - 1) > 0xffffffffull)
    return fail(ctx, LT_ERR_BAD_SCENE, "scene too large for 32-bit byte offsets (4 GiB of nodes / 2 GiB of traversal triangles)");
  return LT_OK;
}

static int triangles_flags_error(lt_hip_context* ctx, uint32_t flags) {
  return fail(ctx, LT_ERR_BAD_SCENE, (flags & lt_build::kFlagNonFinite) ? "non-finite vertex position" : "materialIndex out of range");
}

static int set_triangles_impl(lt_hip_context* ctx, const lt_hip_triangles_desc* d, bool device, void* hip_stream) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  const char* who = device ? "lt_hip_set_triangles_device" : "lt_hip_set_triangles";
  if (const int rc = check_triangles_desc(ctx, d, device, who)) return rc;
  const SceneKnobs k;
  SceneLaps laps{k.timing};
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint32_t n = (uint32_t)d->n, n_nodes = 2 * n - 1, n_mats = (uint32_t)(d->material_bytes / 32);
  const uint64_t sizes[4] = {32ull * n_nodes, 76ull * n, d->material_bytes, 260};
  const lt_prep::Allocator al{&ctx->pool, &ScenePool::get_cb, &ScenePool::put_cb};
  struct Staged {   // (the host form's device copies of the caller's arrays, and what the build made: back to the pool on every exit)
    ScenePool& pool; const lt_prep::Allocator& al; void* p[4] = {nullptr, nullptr, nullptr, nullptr}; lt_build::Out built;
    ~Staged() { for (void* q : p) pool.put(q); lt_build::release(built, al); }
  } st{ctx->pool, al};
  const void* src[4] = {d->positions, d->normals, d->material_indices, d->materials};
  if (device) {
    LT_HIP_CHECK(ctx, hipStreamSynchronize((hipStream_t)hip_stream));   // (what wrote the caller's tensors is done)
  } else {
    const uint64_t bytes[4] = {36ull * n, 36ull * n, 4ull * n, d->material_bytes};
    for (int i = 0; i < 4; i++) {
      if (!src[i]) continue;
      LT_HIP_CHECK(ctx, ctx->pool.upload(&st.p[i], src[i], bytes[i]));
      src[i] = st.p[i];
    }
  }
  laps.lap("triangles on the device");
  LT_HIP_CHECK(ctx, lt_build::run((const float*)src[0], (const float*)src[1], (const int32_t*)src[2], src[3], n_mats, n, ctx->stream, ctx->d_prep_flag,
                                  k.timing, al, st.built));
  if (st.built.flags) return triangles_flags_error(ctx, st.built.flags);
  if (k.timing) fprintf(stderr, "[lt set_scene] build: checks + sorts %.2f ms, %d levels %.2f ms, gather + boxes + lights %.2f ms\n", st.built.ms_sort,
                        st.built.height, st.built.ms_levels, st.built.ms_finish);
  laps.lap("canonical median build");
  // What follows is lt_hip_set_scene's from its uploaded buffers on, by the same size rule.
  int rc = kDeviceDeclined;
  if (k.device < 0 ? n_nodes >= 8192u : k.device != 0)
    rc = prepare_resident(ctx, st.built.d_nodes, st.built.d_prims, src[3], st.built.d_lights, hipMemcpyDeviceToDevice, sizes, SceneHash(), k, laps,
                          []() { return hipSuccess; });
  if (rc == kDeviceDeclined) {   // (a small scene, or a tree lt_prep declines -- a bound beyond 2^40: the host path, from a copy of the four buffers)
    std::vector<uint8_t> host[4];
    const void* from[4] = {st.built.d_nodes, st.built.d_prims, src[3], st.built.d_lights};
    for (int i = 0; i < 4; i++) {
      host[i].resize(sizes[i]);
      if (i == 2 && !device) memcpy(host[i].data(), d->materials, sizes[i]);
      else LT_HIP_CHECK(ctx, hipMemcpy(host[i].data(), from[i], sizes[i], hipMemcpyDeviceToHost));
    }
    laps.lap("read back for the host path");
    SceneKnobs hk = k;
    hk.device = 0;
    hk.always_upload = true;   // (whatever is resident, this is a new scene)
    rc = set_scene_impl(ctx, host[0].data(), sizes[0], host[1].data(), sizes[1], host[2].data(), sizes[2], host[3].data(), sizes[3], hk, nullptr);
  }
  if (rc == LT_OK) ctx->scene_hash_valid = false;   // (no host image: host buffers handed over later are never "the resident scene")
  return rc;
}

extern "C" int lt_hip_set_triangles(lt_hip_context* ctx, const lt_hip_triangles_desc* desc) {
  try {
    return set_triangles_impl(ctx, desc, false, nullptr);
  } catch (const std::exception& e) {
    return fail(ctx, LT_ERR_HIP, std::string("lt_hip_set_triangles: ") + e.what());
  }
}

extern "C" int lt_hip_set_triangles_device(lt_hip_context* ctx, const lt_hip_triangles_desc* desc, void* hip_stream) {
  try {
    return set_triangles_impl(ctx, desc, true, hip_stream);
  } catch (const std::exception& e) {
    return fail(ctx, LT_ERR_HIP, std::string("lt_hip_set_triangles_device: ") + e.what());
  }
}

extern "C" int lt_hip_build_scene_host(const lt_hip_triangles_desc* desc, void* nodes, uint64_t node_bytes, void* prims, uint64_t prim_bytes, void* lights) {
  if (const int rc = check_triangles_desc(nullptr, desc, false, "lt_hip_build_scene_host")) return rc;
  if (!nodes || !prims || !lights) return fail(nullptr, LT_ERR_INVALID_ARGUMENT, "lt_hip_build_scene_host: NULL output buffer");
  if (node_bytes < 32 * (2 * desc->n - 1) || prim_bytes < 76 * desc->n) return fail(nullptr, LT_ERR_BUFFER_TOO_SMALL, "lt_hip_build_scene_host: output buffer too small");
  try {
    const uint32_t flags = lt_build::build_host(desc->positions, desc->normals, desc->material_indices, desc->materials, (uint32_t)(desc->material_bytes / 32),
                                                (uint32_t)desc->n, nodes, prims, lights);
    return flags ? triangles_flags_error(nullptr, flags) : LT_OK;
  } catch (const std::exception& e) {
    return fail(nullptr, LT_ERR_HIP, std::string("lt_hip_build_scene_host: ") + e.what());
  }
}

extern "C" int lt_hip_read_scene_buffer(lt_hip_context* ctx, int which, void* out, uint64_t capacity, uint64_t* out_bytes) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  if (!out_bytes || which < 0 || which > 3) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_read_scene_buffer: bad arguments");
  if (!ctx->has_scene) return fail(ctx, LT_ERR_NO_SCENE, "no scene uploaded");
  const void* const src[4] = {ctx->d_nodes, ctx->d_prims, ctx->d_mats, ctx->d_lights};
  const uint64_t bytes = ctx->scene_sizes[which];
  *out_bytes = bytes;
  if (!out) return LT_OK;
  if (capacity < bytes) return fail(ctx, LT_ERR_BUFFER_TOO_SMALL, "lt_hip_read_scene_buffer: buffer too small");
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LT_HIP_CHECK(ctx, hipDeviceSynchronize());
  LT_HIP_CHECK(ctx, hipMemcpy(out, src[which], bytes, hipMemcpyDeviceToHost));
  return LT_OK;
}

// ---------------------------------------------------------------------------------- render
// The render switches, read once at the top of every public render call (tests and bench.py change them between the calls on one
// context): A/B measurements, tests, debugging.  None of them changes a pixel.
struct RenderKnobs {
  int shadow_packets = -1;              // LT_SHADOW_PACKETS=0..3: the shadow-ray walk, forced (choose_shadow_walk); -1: timed or remembered
  float shadow_spread = 0.02f;          // LT_SHADOW_SPREAD: walk 2's threshold (SceneDev::shadowSpread is its square)
  bool square_major = !env_off("LT_SQUARE_MAJOR");
  bool persistent = !env_off("LT_PERSISTENT");       // off: one square per workgroup instead of persistent wavefronts
  bool square_order = !getenv("LT_NATURAL_ORDER");   // (set to anything, "0" included: the natural hand-out order)
  int gi_wavefront = -1;                // LT_GI_MEGAKERNEL=1 / =0: the GI programs' one-lane-per-pixel kernel / wavefront pipeline; -1: plan_fusion decides
  bool gi_lds_scene = !env_off("LT_GI_LDS_SCENE");   // (gi_lds_scene())
  bool gi_trace = !env_off("LT_GI_TRACE");           // off: a GI bounce stage in one kernel (launch_gi_sample)
  uint32_t trace_refill = 24;           // LT_TRACE_REFILL=1..64: lt_trace_kernel's TraceParams::refill
  bool fused_frames = !env_off("LT_FUSED_FRAMES");   // off: one launch per sample (plan_fusion)
  uint64_t fused_bytes = 16ull << 30;   // LT_FUSED_BYTES: the scratch memory of fused launches
  uint32_t debug_lds_rows = 0;          // LT_DEBUG_LDS_ROWS=1..160: LDS rows of every render launch (render_on_stream); 0: what it needs
  bool debug_calibration = getenv("LT_DEBUG_CALIBRATION") != nullptr;   // calibrate_shadow_walk prints its timings to stderr
  bool debug_camera_hits = getenv("LT_DEBUG_CAMERA_HITS") != nullptr;   // launch_camera_hits prints the squares of its pass to stderr
  bool pinned_readback = !env_off("LT_PINNED_READBACK");   // off: lt_hip_render reads back in one copy (readback_piece)
  bool camera_hits = !env_off("LT_CAMERA_HITS");   // off: every launch walks its camera rays (launch_camera_hits)
  bool camera_hits_keep = !env_off("LT_CAMERA_HITS_KEEP");   // off: a call's camera hits are not kept for the next one (camera_hits_key)
  bool entry_cut = !env_off("LT_ENTRY_CUT");   // off: every square's entry cut is the empty list (launch_entry_cuts)
  uint32_t entry_cut_leaves = 512;      // LT_ENTRY_CUT_LEAVES=0: node cuts only, no leaf pass (lt_entry_cut_kernel); =N >= 2: the records its
                                        // leaf pass may visit per square, for measurements (1, or unset: 512)
  uint32_t entry_cut_chunks = (uint32_t)lt_entry_cut::kDefaultChunks;   // LT_ENTRY_CUT_CHUNKS=1..16: the 64-byte records a square's list may take (lt_entry_cut.hpp: Chunks)
  uint32_t entry_cut_node_chunks = (uint32_t)lt_entry_cut::kDefaultNodeChunks;   // LT_ENTRY_CUT_NODE_CHUNKS=1..16: the records of a list of nodes at most
  bool clear_items = !env_off("LT_CLEAR_ITEMS");   // off: no item table -- a clear square is `groups` claims and stores its samples (ensure_clear_items)
  bool clear_items_fold = true;         // LT_CLEAR_ITEMS=2: the table's hand-out alone -- whole squares store their samples, the fold reads them
  bool clear_items_force = false;       // LT_CLEAR_ITEMS=1 or 2: the table however few squares are clear (unset: only where a third of them are)
  bool clear_square = !env_off("LT_CLEAR_SQUARE");   // off: a clear square handed out whole renders its frame groups one by one (render_clear_square)
  uint32_t shadow_frames = 2;           // LT_SHADOW_FRAMES=1..2: frames per work item whose shadow rays walk together (launch_walk)
  bool debug_shadow_frames = getenv("LT_DEBUG_SHADOW_FRAMES") != nullptr;   // launch_walk prints the frame groups of every render launch
                                                                            // and, where there are groups, how many waves walked them together
  RenderKnobs() {
    if (const char* e = getenv("LT_SHADOW_PACKETS")) shadow_packets = std::max(0, std::min(3, atoi(e)));
    if (const char* e = getenv("LT_SHADOW_SPREAD")) shadow_spread = (float)atof(e);
    if (const char* e = getenv("LT_GI_MEGAKERNEL")) gi_wavefront = atoi(e) == 0;
    if (const char* e = getenv("LT_TRACE_REFILL")) trace_refill = (uint32_t)std::max(1, std::min(64, atoi(e)));
    if (const char* e = getenv("LT_FUSED_BYTES")) fused_bytes = strtoull(e, nullptr, 10);
    if (const char* e = getenv("LT_DEBUG_LDS_ROWS")) debug_lds_rows = (uint32_t)std::max(1, std::min(160, atoi(e)));
    if (const char* e = getenv("LT_ENTRY_CUT_LEAVES")) {
      const int v = atoi(e);
      entry_cut_leaves = v <= 0 ? 0u : v == 1 ? 512u : (uint32_t)std::min(v, 1 << 20);
    }
    if (const char* e = getenv("LT_ENTRY_CUT_CHUNKS")) entry_cut_chunks = (uint32_t)std::max(1, std::min(lt_entry_cut::kMaxChunks, atoi(e)));
    if (const char* e = getenv("LT_ENTRY_CUT_NODE_CHUNKS")) entry_cut_node_chunks = (uint32_t)std::max(1, std::min(lt_entry_cut::kMaxChunks, atoi(e)));
    entry_cut_node_chunks = std::min(entry_cut_node_chunks, entry_cut_chunks);   // (a list of nodes takes no more records than a list may)
    if (const char* e = getenv("LT_CLEAR_ITEMS")) {
      clear_items_fold = atoi(e) != 2;
      clear_items_force = atoi(e) != 0;
    }
    if (const char* e = getenv("LT_SHADOW_FRAMES")) shadow_frames = (uint32_t)std::max(1, std::min(2, atoi(e)));
  }
};

// Grows a scratch buffer of the context to `need` units (`bytes` bytes): frees the old one, allocates, records the capacity
// (0 while there is no buffer).
template <class T>
static hipError_t grow_scratch(const lt_hip_context* ctx, T*& buf, uint64_t& capacity, uint64_t need, uint64_t bytes) {
  if (capacity >= need) return hipSuccess;
  hipError_t e = buf ? hipFree(buf) : hipSuccess;
  if (e != hipSuccess) return e;
  buf = nullptr;
  e = hipMalloc((void**)&buf, bytes);
  capacity = e == hipSuccess ? need : 0;
  if (e == hipSuccess && ctx->pool.poison >= 0) e = lt_debug_poison(buf, bytes, ctx->pool.poison);
  return e;
}

struct TilePlan {
  uint32_t tileW, tileH, tilesX, tilesY, tileFirst, tileStride, tilesInCall, bptx, bpty;
  uint64_t floats;
  uint64_t squares() const { return (uint64_t)tilesInCall * (bptx * bpty); }   // 8x8 squares of one frame
};

static int plan_tiles(const lt_hip_render_desc* d, TilePlan& p, std::string& msg) {
  if (!d || d->struct_size != sizeof(lt_hip_render_desc)) { msg = "bad lt_hip_render_desc (struct_size)"; return LT_ERR_INVALID_ARGUMENT; }
  if (d->width == 0 || d->height == 0 || d->depth < 3) { msg = "image dimensions must be W>0, H>0, depth>=3"; return LT_ERR_INVALID_ARGUMENT; }
  if ((uint64_t)d->width * d->height > 0x7fffffffull) { msg = "image too large"; return LT_ERR_INVALID_ARGUMENT; }
  if (d->tile_w == 0) {
    p.tileW = d->width; p.tileH = d->height; p.tileFirst = 0; p.tileStride = 1;
  } else {
    if (d->tile_h == 0 || d->tile_stride == 0) { msg = "tile_h and tile_stride must be > 0 when tile_w > 0"; return LT_ERR_INVALID_ARGUMENT; }
    p.tileW = d->tile_w; p.tileH = d->tile_h; p.tileFirst = d->tile_first; p.tileStride = d->tile_stride;
  }
  p.tilesX = (d->width + p.tileW - 1) / p.tileW;
  p.tilesY = (d->height + p.tileH - 1) / p.tileH;
  const uint32_t total = p.tilesX * p.tilesY;
  // (in 64 bits: a tile_stride near 2^32 -- "this tile alone" -- would wrap the sum to a count of 0)
  p.tilesInCall = p.tileFirst < total ? (uint32_t)(((uint64_t)total - p.tileFirst + p.tileStride - 1) / p.tileStride) : 0;
  p.bptx = (p.tileW + 7) / 8;
  p.bpty = (p.tileH + 7) / 8;
  p.floats = (uint64_t)p.tilesInCall * p.tileW * p.tileH * d->depth;
  return LT_OK;
}

extern "C" int lt_hip_output_floats(const lt_hip_render_desc* desc, uint64_t* out_floats) {
  TilePlan p;
  std::string msg;
  if (!out_floats) return LT_ERR_INVALID_ARGUMENT;
  if (const int rc = plan_tiles(desc, p, msg)) return rc;
  *out_floats = p.floats;
  return LT_OK;
}

// Every argument error of a render call past its tile plan, in the order they have always been reported.
static int check_render_desc(lt_hip_context* ctx, const lt_hip_render_desc* d, const TilePlan& p, const float* out, uint64_t out_bytes) {
  const bool userProgram = d->program >= LT_PROGRAM_USER_BASE;
  if (userProgram ? (size_t)(d->program - LT_PROGRAM_USER_BASE) >= ctx->user_programs.size()
                  : (d->program < LT_PROGRAM_BASIC || d->program > LT_PROGRAM_CUSTOM_OPENCL))
    return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "unknown program");
  if (userProgram && (d->flags & (LT_RENDER_FLAG_STATS | LT_RENDER_FLAG_PIXEL_COUNTERS)))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, "user programs are compiled without the counting variants");
  if (d->kernel_mode != LT_KERNEL_MODE_LINEAR && d->kernel_mode != LT_KERNEL_MODE_TILE) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "unknown kernel mode");
  if (!out) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "output pointer is NULL");
  if (out_bytes < p.floats * sizeof(float)) return fail(ctx, LT_ERR_BUFFER_TOO_SMALL, "output buffer smaller than the image/tile stack");
  if (d->gi_max_depth < 0 || d->gi_max_depth > 64) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "gi_max_depth out of range");
  if ((d->flags & LT_RENDER_FLAG_PIXEL_COUNTERS) && d->depth < 4) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "LT_RENDER_FLAG_PIXEL_COUNTERS needs depth >= 4");
  if ((d->flags & LT_RENDER_FLAG_PORTABLE_MATH) && (d->flags & LT_RENDER_FLAG_STRICT_MATH))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, "LT_RENDER_FLAG_PORTABLE_MATH and LT_RENDER_FLAG_STRICT_MATH exclude each other");
  if (p.squares() > 0x7fffffffull) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "too many workgroups");
  return LT_OK;
}

// The resident scene as the kernels see it, no shadow-ray walk chosen yet.  The default math flavour (2) is bit-identical to the
// reference's OpenCL kernels as RendererOpenCL builds them on this GPU; LT_RENDER_FLAG_STRICT_MATH / _PORTABLE_MATH select the
// other two (include/lenstrace_hip.h).
static SceneDev scene_dev(const lt_hip_context* ctx, const RenderKnobs& k, int devlibm) {
  SceneDev sc{};
  sc.nodes = (const float4*)ctx->d_nodes;
  sc.wide = ctx->d_wide ? (const uint4*)ctx->d_wide + 4 : nullptr;   // (behind the 64 bytes that hold the grid)
  sc.ownPairs = (const float4*)ctx->d_pairs2;
  sc.rank8 = (const uint32_t*)ctx->d_rank8;
  sc.nWide = ctx->d_rank8 ? ctx->n_wide : 0u;
  sc.tris = (const float4*)ctx->d_tris; sc.prims = (const float*)ctx->d_prims;
  sc.mats = (const Material*)ctx->d_mats; sc.lights = (const Lights*)ctx->d_lights;
  sc.n_nodes = ctx->n_nodes; sc.n_prims = ctx->n_prims; sc.n_mats = ctx->n_mats;
  sc.shadowSpread = k.shadow_spread * k.shadow_spread;
  sc.fastRcp = devlibm == 2 ? 1u : 0u;
  return sc;
}

// What is the same for every frame of a call; the frame loop of render_on_stream fills in the rest.
static FrameParams frame_params(const lt_hip_render_desc* d, const TilePlan& p, const RenderKnobs& k) {
  float cam[7];
  memcpy(cam, d->camera, 28);
  FrameParams fp{};
  fp.camx = cam[0]; fp.camy = cam[1]; fp.camz = cam[2];
  fp.apx = 0.0f; fp.apy = 0.0f; fp.apz = 5.0f;
  fp.cosYaw = (float)std::cos((double)cam[3]);
  fp.sinYaw = (float)std::sin((double)cam[3]);
  fp.yaw = cam[3];
  fp.width = d->width; fp.height = d->height; fp.depth = d->depth;
  fp.clampOutput = d->kernel_mode == LT_KERNEL_MODE_LINEAR;
  fp.squareMajor = k.square_major ? 1u : 0u;
  fp.giMaxDepth = d->gi_max_depth ? d->gi_max_depth : 16;
  fp.tileW = p.tileW; fp.tileH = p.tileH; fp.tilesX = p.tilesX; fp.tileFirst = p.tileFirst; fp.tileStride = p.tileStride;
  fp.tilesInCall = p.tilesInCall; fp.totalSquares = (uint32_t)p.squares();
  fp.blocksPerTileX = p.bptx; fp.blocksPerTile = p.bptx * p.bpty;
  fp.pixelCounters = (d->flags & LT_RENDER_FLAG_PIXEL_COUNTERS) != 0;
  fp.persistent = k.persistent;
  fp.shadowFrames = 1;
  return fp;
}

// What the launches of one render call share: render_on_stream fills it in once, before its frame loop.
struct RenderCall {
  const lt_hip_render_desc* d; const RenderKnobs& k; hipStream_t s;
  bool deep, stats;       // the counting kernels, in their deep-tree form
  int devlibm;            // the math flavour, Math<0 / 1 / 2> (lt_device.hpp)
  uint32_t lds;           // LDS of a render launch's workgroup
  uint32_t ldsRefBytes;   // LDS of a wave whose per-lane stack follows the caller's tree (the LDS-scene GI launches)
  uint64_t nblocks;       // 8x8 squares of one frame
  uint32_t launches;      // lt_hip_stats::kernel_launches
};

// f(std::integral_constant<int, M>) for the math flavour M of a launch.
template <class F>
static auto with_math(int devlibm, F&& f) {
  return devlibm == 2 ? f(std::integral_constant<int, 2>{}) : devlibm == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}

template <int PROGRAM>
static void launch_program(const RenderCall& c, const SceneDev& sc, const FrameParams& fp, dim3 grid, float* out, unsigned long long* st, uint32_t* queues) {
  with_math(c.devlibm, [&](auto m) {
    constexpr int M = decltype(m)::value;
    auto launch = [&](auto cfg) { hipLaunchKernelGGL((lt_render_kernel<PROGRAM, decltype(cfg)>), grid, dim3(kBlock), c.lds, c.s, sc, fp, out, st, queues); };
    // (DEEP -- LDS stack rows beyond kLdsStack spilled to scratch -- concerns the counting kernels only: the others keep no per-lane
    // stack in LDS, whatever the height of the caller's tree; kAccumulatorQueue is never a counting launch)
    if constexpr (PROGRAM == kAccumulatorQueue) launch(Config<false, false, M>{});
    else if (c.stats && c.deep) launch(Config<true, true, M>{});
    else if (c.stats) launch(Config<false, true, M>{});
    else if constexpr (PROGRAM == kAccumulator) {
      if (fp.shadowFrames > 1u && fp.itemTable != nullptr) launch(Config<false, false, M, false, true, true>{});   // (... from an item table: likewise)
      else if (fp.shadowFrames > 1u) launch(Config<false, false, M, false, true>{});   // (frame groups: a kernel of their own)
      else launch(Config<false, false, M>{});
    } else launch(Config<false, false, M>{});
  });
}

// 8 per-XCD square queues, queue lengths, bounce work counters, trace work counters (extension rays, shadow rays), hit-list lengths:
// every counter in a cache line of its own
constexpr uint32_t kGiCtlWords = (8 + 19 * (kMaxStack + 2)) * kQueueStride;   // (the trace launches' counters come in eights: one per eighth of their queue)

static int ensure_gi_buffers(lt_hip_context* ctx, uint64_t pixels) {
  const int poison = ctx->pool.poison;
  if (!ctx->d_giCtl) {
    LT_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_giCtl, kGiCtlWords * sizeof(uint32_t)));
    if (poison >= 0) LT_HIP_CHECK(ctx, lt_debug_poison(ctx->d_giCtl, kGiCtlWords * sizeof(uint32_t), poison));
  }
  if (ctx->gi_pixels >= pixels) return LT_OK;
  for (void*& b : ctx->d_gi) { if (b) LT_HIP_CHECK(ctx, hipFree(b)); b = nullptr; }
  ctx->gi_pixels = 0;
  for (int i = 0; i < 17; i++) {
    LT_HIP_CHECK(ctx, hipMalloc(&ctx->d_gi[i], pixels * 16));
    if (poison >= 0) LT_HIP_CHECK(ctx, lt_debug_poison(ctx->d_gi[i], pixels * 16, poison));
  }
  ctx->gi_pixels = pixels;
  return LT_OK;
}

// A scene of a few hundred triangles rides in LDS for the GI bounce stages' per-lane walks (Config::kLdsScene): workgroups of
// eight waves share one copy.  LT_GI_LDS_SCENE=0 turns it off (A/B measurements).
static uint64_t scene_lds_bytes(const lt_hip_context* ctx) { return (uint64_t)ctx->n_nodes * 32 + (uint64_t)ctx->n_prims * 48; }
static bool gi_lds_scene(const lt_hip_context* ctx, const RenderKnobs& k) {
  return ctx->bvh_height <= kLdsStack && scene_lds_bytes(ctx) <= 16384 && k.gi_lds_scene;   // (its walks keep the LDS stack)
}

// fp.fusedFrames samples of a global-illumination program through one set of stage launches of the wavefront pipeline
// (lt_kernel.hpp): frames sample, sample + 1, ... of the single-sample program (blend25Out == nullptr: the resolve stage
// writes each frame's clamped colour to out + frame * fp.frameStride, or straight to the image when there is one frame), or
// samples k0 .. k0 + fusedFrames - 1 of ONE frame of the 25-sample variant (blend25Out = the image: the resolve stage
// writes raw colours to `out`, lt_gi_blend25_kernel blends them in order and finishes the pixel with accumulateN).
template <class CFG>
static int launch_gi_sample(lt_hip_context* ctx, RenderCall& c, const SceneDev& sc, const FrameParams& fp, float* out, uint64_t pixels,
                            uint32_t sample, uint32_t k0, float* blend25Out, int32_t accumulateN) {
  // `pixels` = compact output pixels of ONE frame
  const hipStream_t s = c.s;
  GiParams gp{};
  for (int k = 0; k < 2; k++) {
    gp.q[k].o = (float4*)ctx->d_gi[4 * k + 0]; gp.q[k].d = (float4*)ctx->d_gi[4 * k + 1];
    gp.q[k].n = (float4*)ctx->d_gi[4 * k + 2]; gp.q[k].m = (uint4*)ctx->d_gi[4 * k + 3];
  }
  gp.direct = (float4*)ctx->d_gi[8]; gp.indirect = (float4*)ctx->d_gi[9]; gp.blend = (float4*)ctx->d_gi[10];
  // the control block behind the 8 square queues: runs of kMaxStack + 2 counters, one per stage (the trace launches' in eights)
  auto ctl = [&](uint32_t run) { return ctx->d_giCtl + (8 + run * (kMaxStack + 2)) * kQueueStride; };
  uint32_t* queues = ctx->d_giCtl;
  gp.counts = ctl(0); gp.work = ctl(1); gp.hitCount = ctl(2);
  uint32_t* const traceWork = ctl(3);     // 8 per stage
  uint32_t* const shadowWork = ctl(11);   // 8 per stage
  gp.sample = sample;
  gp.raw = blend25Out ? 1u : 0u;
  gp.pixels = (uint32_t)pixels;
  const uint64_t vpixels = pixels * fp.fusedFrames;
  LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_giCtl, 0, kGiCtlWords * sizeof(uint32_t), s));
  const uint32_t resident = (uint32_t)ctx->cu_count * 4u * LT_GI_STAGE_WAVES;
  const uint32_t gridA = (uint32_t)std::min<uint64_t>((uint64_t)fp.totalSquares * fp.fusedFrames, resident);
  // the primary stage's shadow rays are accumulator's (same light samples from the same camera hits): any-hit packets unless this
  // scene's accumulator frames were timed faster per lane (calibrate_shadow_walk) or LT_SHADOW_PACKETS says otherwise; the bounce
  // stages' shadow rays start on scattered bounce hits and stay per lane
  SceneDev scPrimary = sc;
  {
    const int timed = ctx->shadow_mode[LT_PROGRAM_ACCUMULATOR];
    const int mode = c.k.shadow_packets >= 0 ? c.k.shadow_packets : timed < 0 ? 1 : timed;
    scPrimary.shadowPackets = mode == 3 ? 0u : (uint32_t)mode;   // (queued is accumulator's own; where it won, the rays are not packets)
  }
  const bool ldsScene = gi_lds_scene(ctx, c.k);
  // With a tree of the backend's own to walk, a bounce stage is five launches instead of one (lt_kernel.hpp): its extension rays
  // through lt_trace_kernel, whose lanes take a new ray when theirs is done; the paths sorted into light hits, misses and
  // surface hits; the surface hits' light samples; their shadow rays through lt_trace_kernel; the survivors' next rays.
  // LT_GI_TRACE=0: the one-kernel stage (A/B measurements).
  const bool pretrace = !ldsScene && ctx->d_rank8 != nullptr && c.k.gi_trace;
  gp.directQueue = pretrace ? 1u : 0u;
  hipLaunchKernelGGL((lt_gi_primary_kernel<CFG>), dim3(gridA), dim3(kBlock), c.lds, s, scPrimary, fp, gp, queues);
  LT_HIP_CHECK(ctx, hipGetLastError());
  c.launches++;
  gp.ldsRows = c.ldsRefBytes / (kBlock * sizeof(int));   // (read by the multi-wave workgroups of the LDS-scene launches only)
  gp.hitList = (uint32_t*)ctx->d_gi[12];
  gp.so = (float4*)ctx->d_gi[13]; gp.sd = (float4*)ctx->d_gi[14]; gp.sm = (uint4*)ctx->d_gi[15]; gp.sn = (float4*)ctx->d_gi[16];
  const uint32_t traceLds = (uint32_t)((kTraceRows + kTraceStage) * kBlock * sizeof(int));
  const dim3 streamGrid((uint32_t)ctx->cu_count * 8u), streamBlock(256);
  for (int d = 0; d < fp.giMaxDepth; d++) {
    gp.hits = nullptr;
    if (pretrace) {
      TraceParams tp{};
      const GiQueue& q = gp.q[d & 1];
      tp.o = q.o; tp.d = q.d; tp.m = q.m;
      tp.hit = (uint4*)ctx->d_gi[11];
      tp.count = gp.counts + (size_t)d * kQueueStride;
      tp.next = traceWork + (size_t)d * 8 * kQueueStride;
      tp.refill = c.k.trace_refill;
      tp.dead = d == 0 ? 1u : 0u;
      gp.hits = tp.hit;
      hipLaunchKernelGGL((lt_trace_kernel<kGI, false>), dim3(resident), dim3(kBlock), traceLds, s, sc, tp);
      hipLaunchKernelGGL((lt_gi_classify_kernel<CFG>), streamGrid, streamBlock, 0, s, sc, fp, gp, (uint32_t)d);
      hipLaunchKernelGGL((lt_gi_shadow_kernel<CFG>), streamGrid, streamBlock, 0, s, sc, fp, gp, (uint32_t)d);
      tp.o = gp.so; tp.d = gp.sd; tp.m = gp.sm;
      tp.occluded = (uint32_t*)ctx->d_gi[11];   // (the extension rays' hits have been read by then: lt_gi_shadow_kernel is behind us in the stream)
      gp.occluded = tp.occluded;
      tp.count = gp.hitCount + (size_t)d * kQueueStride;
      tp.next = shadowWork + (size_t)d * 8 * kQueueStride;
      tp.dead = 0u;
      hipLaunchKernelGGL((lt_trace_kernel<kGI, true>), dim3(resident), dim3(kBlock), traceLds, s, sc, tp);
      hipLaunchKernelGGL((lt_gi_finish_kernel<CFG>), streamGrid, streamBlock, 0, s, sc, fp, gp, (uint32_t)d);
      LT_HIP_CHECK(ctx, hipGetLastError());
      c.launches += 5;
      continue;
    }
    if (ldsScene) {
      using CFGL = Config<false, false, CFG::kDevLibm, true>;
      hipLaunchKernelGGL((lt_gi_bounce_kernel<CFGL>), dim3((resident + kLdsSceneWaves - 1) / kLdsSceneWaves), dim3(kBlock * kLdsSceneWaves),
                         (uint32_t)scene_lds_bytes(ctx) + kLdsSceneWaves * c.ldsRefBytes, s, sc, fp, gp, (uint32_t)d);
    } else {
      hipLaunchKernelGGL((lt_gi_bounce_kernel<CFG>), dim3(resident), dim3(kBlock), c.lds, s, sc, fp, gp, (uint32_t)d);
    }
    LT_HIP_CHECK(ctx, hipGetLastError());
    c.launches++;
  }
  hipLaunchKernelGGL((lt_gi_resolve_kernel<CFG>), dim3((uint32_t)((vpixels + 255) / 256)), dim3(256), 0, s, fp, gp, out, (uint32_t)vpixels);
  LT_HIP_CHECK(ctx, hipGetLastError());
  c.launches++;
  if (blend25Out) {
    FrameParams fb = fp;
    fb.accumulateN = accumulateN;
    hipLaunchKernelGGL((lt_gi_blend25_kernel<CFG>), dim3((uint32_t)((pixels + 255) / 256)), dim3(256), 0, s, fb, gp, out, k0, fp.fusedFrames,
                       blend25Out, (uint32_t)pixels);
    LT_HIP_CHECK(ctx, hipGetLastError());
  }
  return LT_OK;
}

// Hand-out order of the 8x8 squares in persistent mode.  Each XCD keeps its contiguous share of the logical square list
// (render_kernel_body); inside a share, the squares holding a pixel of the image's centre row (direction.y == 0 exactly) or,
// with an unrotated camera, centre column (direction.x == 0) come first, the others follow in Z order over 64x64-pixel blocks.  Those wavefronts cannot use the packet walk or the
// NaN-free box test, and where scene geometry lies in the camera's axis planes (x = camera.x on the 1 M-triangle wall) the
// reference's NaN semantics make their rays visit every box touching the plane: 1.9 ms for such a square against 0.3 ms
// for its neighbours.  Started last they are a launch's tail; started first they overlap with everything else.
static int ensure_square_order(lt_hip_context* ctx, const lt_hip_render_desc* d, const TilePlan& p, bool unrotated, hipStream_t s,
                               const uint32_t** order, uint32_t head[8]) {
  *order = nullptr;
  for (int i = 0; i < 8; i++) head[i] = 0;
  const int64_t cx = (unrotated && d->width % 2 == 0) ? d->width / 2 : -1, cy = d->height % 2 == 0 ? d->height / 2 : -1;
  const uint32_t bpt = p.bptx * p.bpty;
  const uint64_t n = (uint64_t)p.tilesInCall * bpt;
  if (n == 0) return LT_OK;
  const std::vector<uint32_t> key = {d->width, d->height, p.tileW, p.tileH, p.tileFirst, p.tileStride, (uint32_t)cx, (uint32_t)cy};
  auto hand_out = [&]() { *order = ctx->d_order; for (int i = 0; i < 8; i++) head[i] = ctx->order_head[i]; return LT_OK; };
  if (key == ctx->order_key) return hand_out();
  std::vector<uint32_t> ord((size_t)n);
  const uint64_t q = n / 8, r = n % 8;
  for (uint32_t xcd = 0; xcd < 8; xcd++) {
    const uint64_t share = q + (xcd < r ? 1 : 0), start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    size_t pos = (size_t)start;
    std::vector<uint32_t> rest;
    rest.reserve((size_t)share);
    for (uint64_t b = start; b < start + share; b++) {
      const uint32_t k = (uint32_t)(b / bpt), sb = (uint32_t)(b % bpt);
      const uint32_t tile = p.tileFirst + k * p.tileStride;
      const int64_t x0 = (int64_t)(tile % p.tilesX) * p.tileW + (sb % p.bptx) * 8, y0 = (int64_t)(tile / p.tilesX) * p.tileH + (sb / p.bptx) * 8;
      // (a square is clipped to its tile: an 8-pixel span that crosses the tile edge does not reach the next tile's pixels)
      const int64_t x1 = std::min<int64_t>(x0 + 8, (int64_t)(tile % p.tilesX) * p.tileW + p.tileW);
      const int64_t y1 = std::min<int64_t>(y0 + 8, (int64_t)(tile / p.tilesX) * p.tileH + p.tileH);
      if ((cx >= x0 && cx < x1) || (cy >= y0 && cy < y1)) ord[pos++] = (uint32_t)b; else rest.push_back((uint32_t)b);
    }
    ctx->order_head[xcd] = (uint32_t)(pos - (size_t)start);
    // the rest in Z order over blocks of 8 x 8 squares (64 x 64 pixels): the ~1000 squares an XCD works on at any moment
    // then cover a compact image region instead of two full-width rows of squares, and its L2 a smaller part of the tree
    // (+3.6 % on the 1 M-triangle soup, neutral on the wall)
    {
      constexpr uint32_t B = 8;
      auto keyOf = [&](uint32_t b) {
        const uint32_t k = b / bpt, sb = b % bpt, tile = p.tileFirst + k * p.tileStride;
        const uint32_t sx = ((tile % p.tilesX) * p.tileW) / 8 + sb % p.bptx, sy = ((tile / p.tilesX) * p.tileH) / 8 + sb / p.bptx;
        const uint32_t bx = sx / B, by = sy / B;
        uint64_t z = 0;
        for (int i = 0; i < 16; i++) z |= ((uint64_t)((bx >> i) & 1u) << (2 * i)) | ((uint64_t)((by >> i) & 1u) << (2 * i + 1));
        return (z << 32) | ((uint64_t)(sy % B) << 16) | (sx % B);
      };
      std::vector<std::pair<uint64_t, uint32_t>> keyed;
      keyed.reserve(rest.size());
      for (uint32_t b : rest) keyed.emplace_back(keyOf(b), b);
      std::sort(keyed.begin(), keyed.end());
      for (size_t i = 0; i < keyed.size(); i++) rest[i] = keyed[i].second;
    }
    std::copy(rest.begin(), rest.end(), ord.begin() + pos);
  }
  ctx->order_key.clear();
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_order, ctx->order_capacity, n, n * sizeof(uint32_t)));
  // (rare path: image size, tiling or camera rotation changed)  No launch of an earlier call, on whatever stream, may still
  // be reading the old order; and `ord` must outlive the copy.
  LT_HIP_CHECK(ctx, hipDeviceSynchronize());
  LT_HIP_CHECK(ctx, hipMemcpy(ctx->d_order, ord.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  ctx->order_key = key;
  return hand_out();
}

// The wavefront GI pipeline for one iteration of render_on_stream's frame loop: one set of stage launches for the
// fp.fusedFrames frames of the single-sample program (samplesPerSet == 0; colours go to stageOut), or ceil(25 / samplesPerSet)
// sets for the 25 samples of the one frame of the 25-sample variant (raw colours to ctx->d_samples, blended into `image`).
static int launch_gi_sets(lt_hip_context* ctx, RenderCall& c, const SceneDev& sc, const FrameParams& fp, uint64_t giPixels, uint32_t samplesPerSet,
                          uint64_t floats, float* stageOut, float* image) {
  const bool gi25 = samplesPerSet != 0u;
  const uint32_t sets = gi25 ? (25u + samplesPerSet - 1u) / samplesPerSet : 1u;
  for (uint32_t set = 0; set < sets; set++) {
    const uint32_t k0 = set * samplesPerSet;
    FrameParams fs = fp;
    float* blendOut = nullptr;
    float* out = stageOut;
    uint32_t sample = fp.frameCount;
    if (gi25) {
      fs.fusedFrames = std::min(samplesPerSet, 25u - k0);
      fs.frameStride = floats;
      fs.accumulateN = -1;
      blendOut = image;
      out = ctx->d_samples;
      sample = fp.frameCount * 32u + k0;
    }
    const int rc = with_math(c.devlibm, [&](auto m) {   // (never a counting launch: no deep-tree form)
      return launch_gi_sample<Config<false, false, decltype(m)::value>>(ctx, c, sc, fs, out, giPixels, sample, k0, blendOut, fp.accumulateN);
    });
    if (rc) return rc;
  }
  return LT_OK;
}

// lt_hip_render's read-back of `need` bytes: eight pieces of this many bytes each (enqueue_readback), and the call's last fold cut
// into the same pieces (launch_running_mean); 0 (LT_PINNED_READBACK=0, a small image): one copy, one fold launch.
static uint64_t readback_piece(const RenderKnobs& k, uint64_t need) {
  return k.pinned_readback && need >= (1u << 20) ? ((need + 7) / 8 + 4095) / 4096 * 4096 : 0;
}

// One lt_hip_render call's read-back of ctx->d_out.
struct ReadBack {
  uint64_t need = 0, piece = 0;   // bytes of the image; readback_piece (0 once enqueue_readback has no pinned buffer to stage in)
  bool foldPieced = false;        // the call's last fold came in the pieces, an event behind each (launch_running_mean)
};

// The fold of a fused launch runs four floats per thread (lt_running_mean4_kernel) where every float of the range is folded and `out`
// takes 16-byte stores.  (Every range launch_running_mean cuts begins at a multiple of four floats: the pieces' bounds are multiples
// of 4096 bytes.)
static bool mean_in_quads(uint32_t depth, bool paddedTiles, const float* out) { return depth == 3u && !paddedTiles && (uintptr_t)out % 16u == 0u; }

// Folds the nf sample images a fused launch left in ctx->d_samples into `out` (timed by its own event pair, so that
// lt_hip_stats::render_ms can leave it out).  map: the fold map the launch folded its whole squares by (ensure_clear_items: only
// where the quads run), or null.
static int launch_running_mean(lt_hip_context* ctx, hipStream_t s, const FrameParams& fp, uint64_t floats, uint32_t nf, int32_t base,
                               bool paddedTiles, float* out, ReadBack* rb, const unsigned char* map) {
  const uint32_t threads = 256;
  const bool quads = mean_in_quads(fp.depth, paddedTiles, out);
  // (what the render launch folded is skipped by the quads alone: every range below then begins at a multiple of four floats)
  if (map != nullptr && (!quads || (rb && rb->piece % 16u != 0u))) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "a fold map without the four-float fold");
  auto launch = [&](uint64_t lo, uint64_t hi) {
    if (quads && lo % 4u == 0u)
      lt_running_mean4_kernel<<<dim3((uint32_t)((hi - lo + 4u * threads - 1) / (4u * threads))), dim3(threads), 0, s>>>(ctx->d_samples, nf, floats, out, lo, hi, base, map);
    else
      lt_running_mean_kernel<<<dim3((uint32_t)((hi - lo + threads - 1) / threads)), dim3(threads), 0, s>>>(ctx->d_samples, nf, floats, out, lo, hi, base, fp,
                                                                                                       paddedTiles ? 1 : 0);
  };
  while (ctx->mean_events.size() < 2 * (size_t)(ctx->mean_pairs + 1)) {
    hipEvent_t e;
    LT_HIP_CHECK(ctx, hipEventCreate(&e));
    ctx->mean_events.push_back(e);
  }
  LT_HIP_CHECK(ctx, hipEventRecord(ctx->mean_events[2 * ctx->mean_pairs], s));
  if (rb && rb->piece != 0) {
    // lt_hip_render: the call's last fold in the eight pieces of the read-back, an event behind each, so that piece k travels
    // (enqueue_readback, on the copy stream) while piece k + 1 is folded
    for (hipEvent_t& e : ctx->fold_ev) if (!e) LT_HIP_CHECK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const uint64_t per = rb->piece / sizeof(float);
    for (int k = 0; k < 8; k++) {
      const uint64_t lo = std::min(floats, (uint64_t)k * per), hi = std::min(floats, lo + per);
      if (hi > lo) launch(lo, hi);
      LT_HIP_CHECK(ctx, hipEventRecord(ctx->fold_ev[k], s));
    }
    rb->foldPieced = true;
  } else {
    launch(0ull, floats);
  }
  LT_HIP_CHECK(ctx, hipGetLastError());
  LT_HIP_CHECK(ctx, hipEventRecord(ctx->mean_events[2 * ctx->mean_pairs + 1], s));
  ctx->mean_pairs++;
  return LT_OK;
}

// How a call is cut into launches (render_on_stream): which execution path the global-illumination programs take, how many
// frames (or, for the 25-sample variant, samples of one frame) travel through one launch, and the scratch memory for them.
struct FusionPlan {
  bool giWavefront = false;     // wavefront pipeline instead of the one-lane-per-pixel kernel
  uint32_t chunk = 1;           // frames per launch (> 1: fused; lt_running_mean_kernel folds them)
  uint32_t samplesPerSet = 0;   // 25-sample variant through the pipeline: samples per set of stage launches (0: another program)
  uint64_t giPixels = 0;        // compact output pixels of one frame
};

static int plan_fusion(lt_hip_context* ctx, const RenderKnobs& k, const lt_hip_render_desc* d, const TilePlan& p, uint32_t frames, bool stats,
                       int giMaxDepth, FusionPlan& out) {
  const uint64_t nblocks = p.squares();
  // The global-illumination programs run as a wavefront pipeline with path compaction when the scene is big enough for the
  // traversal to dominate the ~18 launches and the queue traffic per sample (1 M-triangle wall at 4K, 16 bounces: 31 ms
  // against 52 ms for the one-lane-per-pixel kernel; 42-triangle Cornell box at 1080p: 3.5 ms against 2.7 ms), or when the
  // launches serve many frames at once and paths are long (Cornell 1080p, 16 frames per call: 1.55 ms against 1.89 ms per
  // sample at 16 bounces, but 1.12 against 0.78 ms at 4; the 25 samples of one frame of the 25-sample variant count as many:
  // 37 against 55 ms at 16 bounces, 27.5 against 21 ms at 4), and never when work is being counted (the counting kernels
  // re-trace like the reference does).  LT_GI_MEGAKERNEL=1 / =0 force one or the other (A/B measurements, tests of both
  // paths on small scenes).
  const bool giProgram = d->program == LT_PROGRAM_GLOBAL_ILLUMINATION || d->program == LT_PROGRAM_GLOBAL_ILLUMINATION_25;
  // (a scene small enough to ride in LDS through the bounce stages, launch_gi_sample, takes the pipeline from 2 bounces on:
  // Cornell 1080p, 16 frames per call, 4 bounces: 8.6 against 10.9 ms; 25-sample variant 12.9 against 19.9 ms)
  const bool giManyLongPaths = giMaxDepth > (gi_lds_scene(ctx, k) ? 1 : 8) && (d->program == LT_PROGRAM_GLOBAL_ILLUMINATION_25 ||
                                                                               (d->program == LT_PROGRAM_GLOBAL_ILLUMINATION && frames > 1 && d->accumulate));
  const bool giWavefront = giProgram && !stats && nblocks > 0 && (k.gi_wavefront >= 0 ? k.gi_wavefront != 0 : (ctx->n_prims >= 1024u || giManyLongPaths));
  const uint64_t giPixels = (uint64_t)p.tilesInCall * p.tileW * p.tileH;
  const uint64_t giSlots = std::max<uint64_t>(giPixels, nblocks * kBlock);   // (a direct-mapped path queue has a slot per lane of every square)
  // (the stages' grids round the slots of a launch up to whole blocks of 256: 2^32 - 256 slots are the most a launch holds)
  if (giWavefront && giSlots > 0xffffff00ull) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "too many pixels for the GI path queues");
  // Several samples of a running mean in ONE launch.  A launch cannot end before its slowest wavefront does -- one 8x8 square
  // is a dependent chain of several hundred node fetches, ~0.3-0.6 ms on the 1 M-triangle scene, 1.9 ms for the squares on
  // the image's centre column -- so a launch per sample pays that drain once per sample: 0.65 ms of a 4.5 ms launch for the
  // whole 4K frame, and of a 1.2 ms launch for one GPU's eighth of it.  Fused, the work items are (frame, square) pairs, all
  // independent: each stores its un-accumulated colour in its frame's slice of a scratch buffer and lt_running_mean_kernel
  // folds the slices in frame order afterwards (same arithmetic, same order: bit-identical).  LT_FUSED_FRAMES=0 turns it
  // off (A/B measurements), LT_FUSED_BYTES caps the scratch memory (default 16 GiB of the 288; tests use it to force chunks).
  // The wavefront GI pipeline fuses the same way (single-sample program only: the 25-sample blend is sequential per pixel):
  // its ~18 stage launches then serve all frames of a chunk, each path carrying its frame; its per-frame scratch is the path
  // queues and the direct / indirect images (11 arrays of 16 bytes per pixel) besides the sample image.
  // The 25-sample variant fuses the samples of ONE frame instead (its frames stay sequential): `chunk` is then the number of
  // samples k per set of launches, and lt_gi_blend25_kernel replaces the running mean.
  uint32_t chunk = 1;
  const bool giFusable = giWavefront && d->program == LT_PROGRAM_GLOBAL_ILLUMINATION;
  const bool gi25Sets = giWavefront && d->program == LT_PROGRAM_GLOBAL_ILLUMINATION_25;
  if (gi25Sets || ((giFusable || (k.persistent && !giWavefront)) && !stats && frames > 1 && d->accumulate && nblocks > 0)) {
    const uint64_t frameBytes = p.floats * sizeof(float);
    const uint64_t scratchPerFrame = frameBytes + (giWavefront ? giSlots * 16 * 17 : 0);
    // (lt_running_mean_kernel runs one thread per float of a sample image, 256 to a block: 2^32 - 256 floats are the most one
    // launch holds.  Under the default LT_FUSED_BYTES two such images do not fit the scratch anyway; a larger cap must not fuse them.)
    if (k.fused_frames && frameBytes > 0 && p.floats <= 0xffffff00ull)
      chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)(gi25Sets ? 25u : frames), k.fused_bytes / scratchPerFrame, 0xffffffffull / nblocks,
                                                                  giWavefront ? 0xffffff00ull / std::max<uint64_t>(giSlots, 1) : ~0ull}));
    // a device that cannot spare the scratch memory gets shorter launches, down to one sample per launch
    while ((chunk > 1 || gi25Sets) && grow_scratch(ctx, ctx->d_samples, ctx->d_samples_bytes, chunk * frameBytes, chunk * frameBytes) != hipSuccess) {
      (void)hipGetLastError();
      if (chunk == 1) return fail(ctx, LT_ERR_HIP, "out of device memory for one sample image");
      chunk /= 2;
    }
  }
  if (giWavefront) {
    int erc;
    while ((erc = ensure_gi_buffers(ctx, giSlots * chunk)) != LT_OK && chunk > 1) chunk /= 2;   // (frees what it got, retries smaller)
    if (erc) return erc;
  }
  out.giWavefront = giWavefront;
  out.giPixels = giPixels;
  out.samplesPerSet = gi25Sets ? chunk : 0u;   // 25-sample variant: samples k per set of stage launches
  out.chunk = gi25Sets ? 1u : chunk;           // ... and its frames stay one per iteration of the caller's loop
  return LT_OK;
}

// Shadow rays as any-hit packets (1), per lane (0), chosen per wavefront (2: traverse(), lt_device.hpp) or queued for
// lt_trace_kernel (3: accumulator): which is fastest depends on the scene (wall: packets; soup: the queue), so each (scene,
// program, image geometry, frames per launch) is timed once, on the first launch that can be repeated without changing the
// result (calibrate_shadow_walk), and the fastest walk kept.  LT_SHADOW_PACKETS=0/1/2/3 forces one (tests, A/B measurements).
// -1: to be timed.  `queueOk`: the call's launches can queue their shadow rays (or there are none).
static int choose_shadow_walk(lt_hip_context* ctx, const RenderKnobs& k, const lt_hip_render_desc* d, const std::vector<uint32_t>& key, bool queueOk) {
  const bool hasShadowRays = d->program == LT_PROGRAM_ACCUMULATOR || d->program == LT_PROGRAM_BASIC_LIGHTING;   // (the GI programs' kernels hold the per-lane walk only)
  int mode = k.shadow_packets >= 0 ? k.shadow_packets : hasShadowRays ? -1 : 0;
  if (mode < 0 && ctx->shadow_modes.count(key)) mode = ctx->shadow_modes[key];
  if (mode < 0 && (d->flags & LT_RENDER_FLAG_NO_WALK_TIMING))   // the caller wants no timing launches in this call
    mode = ctx->shadow_mode[d->program] >= 0 ? ctx->shadow_mode[d->program] : 1;
  if (mode == 3 && d->program != LT_PROGRAM_ACCUMULATOR) mode = 0;   // (queued shadow rays are accumulator's)
  if (mode == 3 && !queueOk) mode = k.shadow_packets >= 0 ? 0 : -1;   // (a forced or remembered mode 3 where it cannot run)
  return mode;
}

// One launch of a built-in program through the one-lane-per-pixel kernels.
static void launch_builtin(const RenderCall& c, const SceneDev& sc, const FrameParams& fp, dim3 grid, float* out, unsigned long long* st,
                           uint32_t* queues) {
  switch (c.d->program) {
    case LT_PROGRAM_BASIC: launch_program<kBasic>(c, sc, fp, grid, out, st, queues); break;
    case LT_PROGRAM_BASIC_LIGHTING: launch_program<kBasicLighting>(c, sc, fp, grid, out, st, queues); break;
    case LT_PROGRAM_ACCUMULATOR:
      if (sc.shadowPackets == 3u) launch_program<kAccumulatorQueue>(c, sc, fp, grid, out, st, queues);
      else launch_program<kAccumulator>(c, sc, fp, grid, out, st, queues);
      break;
    case LT_PROGRAM_GLOBAL_ILLUMINATION: launch_program<kGI>(c, sc, fp, grid, out, st, queues); break;
    case LT_PROGRAM_GLOBAL_ILLUMINATION_25: launch_program<kGI25>(c, sc, fp, grid, out, st, queues); break;
    default: launch_program<kCustom>(c, sc, fp, grid, out, st, queues); break;
  }
}

// One frame-set of the call with a given shadow-ray walk: the render launch and, when the shadow rays are queued (mode 3:
// accumulator, a tree of the backend's own, a launch that overwrites what it writes), lt_trace_kernel over the queue and the
// kernel that blacks out the occluded samples.  With the packet walks (1, 2) accumulator's squares whose camera hits are stored
// are rendered `group` frames at a time (at most LT_SHADOW_FRAMES), their shadow rays walking together (FrameParams::shadowFrames).
static int launch_walk(lt_hip_context* ctx, RenderCall& c, SceneDev& sc, uint32_t mode, uint32_t group, const FrameParams& fp0, dim3 grid, float* out,
                       uint32_t* queues) {
  sc.shadowPackets = mode;
  FrameParams fp = fp0;
  fp.shadowFrames = (mode == 1u || mode == 2u) && c.d->program == LT_PROGRAM_ACCUMULATOR && !c.stats && fp.cameraHits != nullptr
                        ? std::min(std::min(group, c.k.shadow_frames), fp.fusedFrames) : 1u;
  if (mode != 3u) {
    if (c.k.debug_shadow_frames && fp.shadowFrames > 1u) {   // (a debugging aid: counts the waves of each kind, and waits for them)
      if (!ctx->d_groupWalks) LT_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_groupWalks, 14 * sizeof(unsigned long long)));
      LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_groupWalks, 0, 14 * sizeof(unsigned long long), c.s));
      SceneDev sd = sc;
      sd.groupWalks = ctx->d_groupWalks;
      launch_builtin(c, sd, fp, grid, out, ctx->d_stats, queues);
      unsigned long long h[14];   // together, apart, then the together-walks of each one-mixed-axis form (traverse_shadow2)
      LT_HIP_CHECK(ctx, hipMemcpyAsync(h, ctx->d_groupWalks, sizeof(h), hipMemcpyDeviceToHost, c.s));
      LT_HIP_CHECK(ctx, hipStreamSynchronize(c.s));
      fprintf(stderr, "shadow-ray frame groups: %u (walk %u, %u frames): %llu waves walked both frames together, %llu apart; of those together, "
              "one mixed axis: x %llu %llu %llu %llu, y %llu %llu %llu %llu, z %llu %llu %llu %llu\n", fp.shadowFrames, mode, fp.fusedFrames, h[0],
              h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12], h[13]);
      return LT_OK;
    }
    if (c.k.debug_shadow_frames) fprintf(stderr, "shadow-ray frame groups: %u (walk %u, %u frames)\n", fp.shadowFrames, mode, fp.fusedFrames);
    launch_builtin(c, sc, fp, grid, out, ctx->d_stats, queues);
    return LT_OK;
  }
  if (c.k.debug_shadow_frames) fprintf(stderr, "shadow-ray frame groups: %u (walk %u, %u frames)\n", fp.shadowFrames, mode, fp.fusedFrames);
  const uint64_t slots = c.nblocks * fp.fusedFrames * kBlock;
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_shadowq, ctx->shadowq_slots, slots, slots * 52));   // (origin + tmax, direction, pixel / primitive / frame: 48 bytes; its fate: 4)
  if (!ctx->d_shadowCtl) LT_HIP_CHECK(ctx, hipMalloc((void**)&ctx->d_shadowCtl, 9 * kQueueStride * sizeof(uint32_t)));
  LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_shadowCtl, 0, 8 * kQueueStride * sizeof(uint32_t), c.s));
  LT_HIP_CHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)(ctx->d_shadowCtl + 8 * kQueueStride), (int)(uint32_t)slots, 1, c.s));
  sc.shadowQueue = (float4*)ctx->d_shadowq;
  sc.shadowCap = (uint32_t)ctx->shadowq_slots;
  launch_builtin(c, sc, fp, grid, out, ctx->d_stats, queues);
  TraceParams tp{};
  tp.o = sc.shadowQueue; tp.d = sc.shadowQueue + sc.shadowCap; tp.m = (const uint4*)(sc.shadowQueue + 2 * (size_t)sc.shadowCap);
  tp.occluded = (uint32_t*)(sc.shadowQueue + 3 * (size_t)sc.shadowCap);
  tp.count = ctx->d_shadowCtl + 8 * kQueueStride; tp.next = ctx->d_shadowCtl;
  tp.refill = c.k.trace_refill; tp.dead = 1u;
  hipLaunchKernelGGL((lt_trace_kernel<kGI, true>), dim3((uint32_t)ctx->cu_count * 32u), dim3(kBlock), (uint32_t)((kTraceRows + kTraceStage) * kBlock * sizeof(int)),
                     c.s, sc, tp);
  hipLaunchKernelGGL(lt_shadow_resolve_kernel, dim3((uint32_t)ctx->cu_count * 8u), dim3(256), 0, c.s, tp.m, (const uint32_t*)tp.occluded, (uint32_t)slots, out,
                     fp.frameStride, fp.depth);
  LT_HIP_CHECK(ctx, hipGetLastError());
  c.launches += 2;
  return LT_OK;
}

// Times the shadow-ray walks (any-hit packets, per lane, chosen per wavefront, queued for lt_trace_kernel) once per (scene,
// program, image geometry, frames per launch), ahead of a launch whose output they may scribble on (it overwrites what it
// writes, as every fused launch does): the launch as it is -- a verdict on fewer frames is another launch's verdict: a
// launch pays a fixed price for its slowest squares, which the walks share out differently -- once per walk after one
// untimed run.  The fastest wins, unless the walk an earlier verdict on this scene picked is within 3 % of it: two walks
// that close must not take turns from call to call.  Frame groups (launch_walk) are a matter of speed too, and they do not win
// everywhere (colonnade: 16.0 ms with one frame per work item, 16.6 with two): walk 1 is timed with groups, walk 2 without, so
// that a scene where groups lose keeps the packets of single frames (walk 2 takes them where its rays are coherent); `group` is
// the frames per work item of the winner, remembered with it.
static int calibrate_shadow_walk(lt_hip_context* ctx, RenderCall& c, SceneDev& sc, const FrameParams& fp, dim3 grid, float* out, uint32_t* queues,
                                 bool queueOk, const std::vector<uint32_t>& key, int& mode, uint32_t& group) {
  for (hipEvent_t& e : ctx->cal_ev) if (!e) LT_HIP_CHECK(ctx, hipEventCreate(&e));
  const uint32_t kOrder[4] = {1u, 0u, 2u, 3u}, kGroup[4] = {c.k.shadow_frames, 1u, 1u, 1u};
  const int candidates = queueOk ? 4 : 3;
  for (int pass = -1; pass < candidates; pass++) {
    if (pass >= 0) LT_HIP_CHECK(ctx, hipEventRecord(ctx->cal_ev[2 * pass], c.s));
    if (const int rc = launch_walk(ctx, c, sc, kOrder[pass < 0 ? 0 : pass], kGroup[pass < 0 ? 0 : pass], fp, grid, out, queues)) return rc;
    if (pass >= 0) LT_HIP_CHECK(ctx, hipEventRecord(ctx->cal_ev[2 * pass + 1], c.s));
    LT_HIP_CHECK(ctx, hipMemsetAsync(queues, 0, 8 * kQueueStride * sizeof(uint32_t), c.s));
  }
  float t[4] = {0, 0, 0, 0};
  LT_HIP_CHECK(ctx, hipEventSynchronize(ctx->cal_ev[2 * candidates - 1]));
  for (int k = 0; k < candidates; k++) LT_HIP_CHECK(ctx, hipEventElapsedTime(&t[k], ctx->cal_ev[2 * k], ctx->cal_ev[2 * k + 1]));
  if (c.k.debug_calibration)
    fprintf(stderr, "shadow-walk timing (ms, %u frames): packets %.3f, per lane %.3f, per wavefront %.3f, queued %.3f\n", fp.fusedFrames, t[0], t[1], t[2], t[3]);
  int best = 0;
  for (int k = 1; k < candidates; k++) if (t[k] < t[best]) best = k;
  int kept = best;
  const int earlier = ctx->shadow_mode[c.d->program];
  for (int k = 0; k < candidates; k++)
    if ((int)kOrder[k] == earlier && t[k] <= 1.03f * t[best]) kept = k;
  mode = (int)kOrder[kept];
  group = kGroup[kept];
  ctx->shadow_modes[key] = mode;
  ctx->shadow_groups[key] = group;
  ctx->shadow_mode[c.d->program] = mode;
  c.launches += (uint32_t)candidates + 1u;
  return LT_OK;
}

// What the stored camera hits are a function of, and nothing else: every input that camera_hit_square and square_pixel read.  Made
// from the FrameParams the pass is launched with -- not from the desc, so that a field added later is in it without being asked --
// with what changes from frame to frame or launch to launch cleared; the camera's bytes as frame_params takes them, without the frame
// counter at byte 24; the hand-out order the hits are indexed by (ensure_square_order's key and head counts); the math flavour; the
// scene generation; and the allocation the hits live in.
// FrameParams, field by field: camx .. yaw, width, height (camera_ray), tileW .. totalSquares (square_pixel), order, orderHead and
// persistent (the hand-out), ldsRows (the walk's stack) are in the key; depth, clampOutput, giMaxDepth, pixelCounters and squareMajor do
// not reach a camera hit and are in it all the same; frameCount, accumulateN, fusedFrames, frameStride, shadowFrames, storeHeadHits,
// the cameraHits and entryCuts pointers and entryCutPlane and entryCutChunks, which say how to read entryCuts, and the item table's and the
// fold's fields (itemTable .. itemGroups), which are set per launch, are cleared.  (The
// entry cuts kept with the hits are a function of the hits, of the scene's primitives, lights and own tree -- the scene generation
// -- and of the knobs of their build, which launch_camera_hits compares by themselves.)
static_assert(sizeof(FrameParams) == 232 && offsetof(FrameParams, entryCutChunks) + sizeof(uint32_t) == offsetof(FrameParams, itemTable) &&
                  offsetof(FrameParams, itemTable) + 8 == offsetof(FrameParams, foldMap) && offsetof(FrameParams, foldMap) + 8 == offsetof(FrameParams, foldOut) &&
                  offsetof(FrameParams, foldOut) + 8 == offsetof(FrameParams, foldBase) && offsetof(FrameParams, foldBase) + 4 == offsetof(FrameParams, itemGroups) &&
                  offsetof(FrameParams, itemGroups) + sizeof(uint32_t) == sizeof(FrameParams) &&
                  offsetof(FrameParams, entryCuts) + sizeof(const uint32_t*) == offsetof(FrameParams, entryCutPlane) &&
                  offsetof(FrameParams, entryCutPlane) + sizeof(uint32_t) == offsetof(FrameParams, entryCutChunks) &&
                  offsetof(FrameParams, storeHeadHits) + sizeof(uint32_t) == offsetof(FrameParams, entryCuts),
              "FrameParams changed: say in camera_hits_key whether the new field is part of the key or cleared");
static std::vector<unsigned char> camera_hits_key(const lt_hip_context* ctx, const FrameParams& pass, const lt_hip_render_desc* d, int devlibm) {
  FrameParams f = pass;
  f.frameCount = 0; f.accumulateN = 0; f.fusedFrames = 0; f.frameStride = 0; f.shadowFrames = 0; f.storeHeadHits = 0; f.cameraHits = nullptr;
  f.entryCuts = nullptr; f.entryCutPlane = 0; f.entryCutChunks = 0;
  f.itemTable = nullptr; f.foldMap = nullptr; f.foldOut = nullptr; f.foldBase = 0; f.itemGroups = 0;
  std::vector<unsigned char> key;
  auto put = [&](const void* p, size_t n) { key.insert(key.end(), (const unsigned char*)p, (const unsigned char*)p + n); };
  put(&f, sizeof(f));   // (no padding inside: the assertion above and the fields' natural alignment)
  put(d->camera, 24);
  const uint64_t words[4] = {(uint64_t)devlibm, ctx->scene_generation, (uint64_t)(uintptr_t)ctx->d_camhits, ctx->order_key.size()};
  put(words, sizeof(words));
  put(ctx->order_key.data(), ctx->order_key.size() * sizeof(uint32_t));
  put(ctx->order_head, sizeof(ctx->order_head));
  return key;
}

// The camera-hit pass (lt_camera_hits_kernel, FrameParams::cameraHits): a camera ray is the same in every frame of a call, and so is
// its walk -- 1 002 530-triangle wall, 4K, 16 frames: 6.4 of the 17 ms of accumulator's launch were its 16 walks of each camera
// ray (`basic`, nothing but those walks).  So a call of accumulator that renders two or more frames walks each camera ray once,
// before its render launches, which read the hits and shade from them; its head squares (ensure_square_order: 1.9 ms for one on the
// wall, a floor under the pass's length) stay out and are walked by the render launches, where they start first and overlap.  A
// one-frame call keeps the walk in its launch (the pass would add a launch and its drain).
// The hits are kept from one call to the next: a progressive caller leaves the camera where it is and moves frame_first on, and the
// hits do not depend on the frame.  The first launch of a call whose pass ran has its head squares' first-frame items store what they
// walk (FrameParams::storeHeadHits), and once that launch is enqueued the context remembers what the hits belong to (camera_hits_key;
// `pendingKey`: the caller records it then).  A later call with the same key launches no pass and hands its render launches orderHead
// all zero: every square, the head squares too, is then a stored item in frame groups, at the position it always had -- fp.order is
// unchanged, and so are the XCDs' shares.  Anything else in the key -- another camera, image, tile set, scene, math flavour, a
// reallocation -- and the call runs its pass as before; a call that fails after it has begun to overwrite the hits leaves nothing to
// reuse.  Calls that take no hits (one frame, the counting kernels, other programs, LT_PERSISTENT=0, LT_CAMERA_HITS=0) neither read
// nor disturb them.  LT_CAMERA_HITS_KEEP=0: nothing is kept, every call runs its pass.
// Not the counting kernels: their walks are what their ray, node and triangle counts count.  Run after ev0 (render_ms holds it),
// not counted in kernel_launches (lt_hip_camera_hit_passes counts the passes).  LT_CAMERA_HITS=0: every launch walks its camera rays.
// The entry cuts of the squares whose camera hits are stored (lt_entry_cut.hpp, lt_entry_cut_kernel): where the two-frame shadow
// walks of those squares start instead of the root.  Built on the render's stream by the first call that REUSES a set of hits, for
// every square (`all`), and kept with the hits from then on: later reusing calls launch nothing.  A call that runs its own
// camera-hit pass builds none -- a caller whose camera moves with every call would pay the build (4.0 ms on the 1 M-triangle wall
// at 4K: a chain of dependent record fetches per square) for walks that save 2.8 ms in their one call -- unless it is the call that times the shadow walks, which then times the
// packet walk as it will run: with the cuts of the squares its pass walked (`all` false; not kept).  LT_ENTRY_CUT=0, a scene
// without an own tree or with one so high that no list fits the walk's stack beside its own entries (entry_cut_limit): no cuts.
// The same launch then runs the leaf pass (lt_entry_cut_kernel; lt_entry_cut.hpp: may_accept) with RenderKnobs::entry_cut_leaves
// records per square: squares marked clear, squares whose list becomes a few leaves (lt_hip_entry_cut_leaf_counts); 0: none.
// Not in the timing call (`all` false): there the packet walk is timed from the node lists, as it was before there was a leaf pass.
// On bench.py's mixed scene the timed packets and the timed queued walk are within 0.1 - 0.3 ms of each other as it is (27.2 - 27.5
// against 26.4 - 27.3 ms: the queued walk's timed launch includes the first allocation of its queue), while in the calls that reuse
// their hits the queue wins clearly (23.8 against 26.2 ms per step): a faster timed packet launch would tip that toss the wrong way.
// A list takes up to RenderKnobs::entry_cut_chunks records (LT_ENTRY_CUT_CHUNKS; lt_entry_cut.hpp: Chunks): d_cuts holds that many
// planes of one record per square, and the launch writes every plane's record of every square it builds.
static void set_entry_cuts(const lt_hip_context* ctx, FrameParams& fp, uint32_t chunks) {
  fp.entryCuts = ctx->d_cuts;
  fp.entryCutPlane = fp.totalSquares * (uint32_t)lt_entry_cut::kListWords;
  fp.entryCutChunks = chunks;
}
static int launch_entry_cuts(lt_hip_context* ctx, const RenderCall& c, const SceneDev& sc, const FrameParams& fh, bool all) {
  ctx->cuts_valid = false;
  ctx->items_groups = 0;   // (the item table is of the cuts that were: ensure_clear_items builds it again behind this launch)
  ctx->items_worth = -1;
  // (the timing call builds lists of nodes alone: its planes are those a list of nodes may take)
  const uint32_t chunks = all ? c.k.entry_cut_chunks : c.k.entry_cut_node_chunks;
  const uint64_t lists = c.nblocks * chunks;   // (cuts_squares counts records: squares times planes)
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_cuts, ctx->cuts_squares, lists, lists * lt_entry_cut::kListWords * sizeof(uint32_t)));
  if (!ctx->d_cut_stats) LT_HIP_CHECK(ctx, hipMalloc(&ctx->d_cut_stats, kEntryCutStats * sizeof(unsigned long long)));
  LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_cut_stats, 0, kEntryCutStats * sizeof(unsigned long long), c.s));
  with_math(c.devlibm, [&](auto m) {
    hipLaunchKernelGGL((lt_entry_cut_kernel<Config<false, false, decltype(m)::value>>), dim3((uint32_t)c.nblocks), dim3(kBlock), 0, c.s, sc, fh, ctx->d_cuts,
                       all ? 1u : 0u, (uint32_t)lt_entry_cut::entry_cut_limit(ctx->height2), ctx->d_cut_stats, all ? c.k.entry_cut_leaves : 0u, chunks, c.k.entry_cut_node_chunks);
    return 0;
  });
  LT_HIP_CHECK(ctx, hipGetLastError());
  ctx->cuts_valid = all;
  ctx->cuts_leaves = c.k.entry_cut_leaves;
  ctx->cuts_chunks = chunks;
  ctx->cuts_node_chunks = c.k.entry_cut_node_chunks;
  ctx->cuts_plane_squares = fh.totalSquares;
  ctx->cut_builds++;
  return LT_OK;
}

// The item table of the cuts a reusing call reads (lt_entry_cut.hpp: kItemWhole; lt_clear_items_kernel), for a launch of `groups`
// frame groups per square: built on the render's stream behind the cuts -- by the first launch that reads them, which is where the
// number of groups is known, and again by a launch of another number (a call's last, shorter chunk; a call of other frames) -- and
// kept with them: launch_entry_cuts drops it with the cuts it was made from, and a launch takes it only while cuts_valid holds.  No
// host synchronisation: the queues' lengths stay in device memory.  fold: the launch is a fused one whose fold runs in quads over a
// map that is exact for it (render_on_stream); the map is then built with the table and the launch's whole squares fold their
// own samples into `out` from n = base on.  LT_CLEAR_ITEMS=0: never called.
// Worth taking only where enough squares are clear.  Where few are -- the Cornell box at 4K -- nearly every entry is a single frame
// group, as without a table, and each pays the entry's scalar load behind its claim, which items that short cannot hide, and the
// table kernel's larger code: 0.15 ms on that launch of 1.9.  The count is the device's: the first build's counters
// are copied back asynchronously, and from the first launch that finds them there a set of cuts with fewer than a third of its
// squares clear is rendered without the table -- the kernel and the hand-out it had before there was one.  Until then, and under
// LT_CLEAR_ITEMS=1, the table is taken.  (The pixels are the same either way.)
static int ensure_clear_items(lt_hip_context* ctx, const RenderCall& c, FrameParams& fp, uint32_t groups, bool fold, uint64_t floats, float* out, int32_t base) {
  const uint64_t words = lt_entry_cut::kItemHeader + c.nblocks * groups;
  const uint64_t mapWords = (lt_entry_cut::fold_segment_of_float(floats) + 3u) / 4u;
  if (ctx->items_worth < 0 && ctx->items_groups != 0u && ctx->items_ev && hipEventQuery(ctx->items_ev) == hipSuccess)
    ctx->items_worth = 3ull * ctx->h_item_stats[1] >= c.nblocks ? 1 : 0;
  (void)hipGetLastError();   // (hipErrorNotReady of the query is no error)
  if (ctx->items_worth == 0 && !c.k.clear_items_force) return LT_OK;
  if (ctx->items_groups != groups || (fold && !ctx->items_folds)) {
    ctx->items_groups = 0;
    LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_items, ctx->items_words, words, words * sizeof(uint32_t)));
    if (fold) LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_foldmap, ctx->foldmap_words, mapWords, mapWords * sizeof(uint32_t)));
    if (!ctx->d_item_stats) LT_HIP_CHECK(ctx, hipMalloc(&ctx->d_item_stats, 2 * sizeof(unsigned long long)));
    LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_item_stats, 0, 2 * sizeof(unsigned long long), c.s));
    hipLaunchKernelGGL(lt_clear_items_kernel, dim3(8), dim3(kItemThreads), 0, c.s, (const uint32_t*)ctx->d_cuts, fp, groups, ctx->d_items,
                       fold ? (unsigned char*)ctx->d_foldmap : nullptr, ctx->d_item_stats);
    LT_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->items_worth < 0) {
      if (!ctx->h_item_stats) LT_HIP_CHECK(ctx, hipHostMalloc((void**)&ctx->h_item_stats, 2 * sizeof(unsigned long long), hipHostMallocDefault));
      if (!ctx->items_ev) LT_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->items_ev, hipEventDisableTiming));
      LT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_item_stats, ctx->d_item_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.s));
      LT_HIP_CHECK(ctx, hipEventRecord(ctx->items_ev, c.s));
    }
    ctx->items_groups = groups;
    ctx->items_folds = fold;
    ctx->item_builds++;
  }
  fp.itemTable = ctx->d_items;
  fp.itemGroups = groups;
  if (fold) {
    fp.foldMap = ctx->d_foldmap;
    fp.foldOut = out;
    fp.foldBase = base;
  }
  return LT_OK;
}

static int launch_camera_hits(lt_hip_context* ctx, const RenderCall& c, const SceneDev& sc, FrameParams& fp, uint32_t* queues, uint32_t resident,
                              std::vector<unsigned char>& pendingKey, bool wantCuts, bool timingCall) {
  uint64_t squares = 0;   // those of the pass: every square but the head squares (the kernel's own count, lt_kernel.hpp)
  for (uint32_t xcd = 0; xcd < 8; xcd++) squares += camera_hit_squares(fp, xcd);
  if (squares == 0) {
    if (c.k.debug_camera_hits) fprintf(stderr, "camera-hit pass: none (every square is a head square)\n");
    return LT_OK;
  }
  FrameParams fh = fp;
  fh.fusedFrames = 1;
  if (c.k.camera_hits_keep && !ctx->camhits_key.empty() && ctx->camhits_slots >= c.nblocks * kBlock &&
      ctx->camhits_key == camera_hits_key(ctx, fh, c.d, c.devlibm)) {
    // (the same words as below for the pass these hits came from, so that a reader of the log sees which squares it walked)
    if (c.k.debug_camera_hits)
      fprintf(stderr, "camera-hit pass: %llu of %llu squares, kept from an earlier call (no pass launched: %llu so far)\n", (unsigned long long)squares,
              (unsigned long long)c.nblocks, (unsigned long long)ctx->camhit_passes);
    fp.cameraHits = ctx->d_camhits;
    for (uint32_t& h : fp.orderHead) h = 0u;
    if (wantCuts) {
      if (!ctx->cuts_valid || ctx->cuts_squares < c.nblocks * c.k.entry_cut_chunks || ctx->cuts_leaves != c.k.entry_cut_leaves ||
          ctx->cuts_chunks != c.k.entry_cut_chunks || ctx->cuts_node_chunks != c.k.entry_cut_node_chunks) {
        fh.cameraHits = ctx->d_camhits;
        if (const int rc = launch_entry_cuts(ctx, c, sc, fh, true)) return rc;
      }
      set_entry_cuts(ctx, fp, ctx->cuts_chunks);
    }
    return LT_OK;
  }
  if (c.k.debug_camera_hits) fprintf(stderr, "camera-hit pass: %llu of %llu squares\n", (unsigned long long)squares, (unsigned long long)c.nblocks);
  ctx->camhits_key.clear();   // (from here on the hits are being overwritten, or their buffer replaced)
  ctx->cuts_valid = false;
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_camhits, ctx->camhits_slots, c.nblocks * kBlock, c.nblocks * kBlock * sizeof(uint4)));
  fp.cameraHits = fh.cameraHits = ctx->d_camhits;
  with_math(c.devlibm, [&](auto m) {
    hipLaunchKernelGGL((lt_camera_hits_kernel<Config<false, false, decltype(m)::value>>), dim3((uint32_t)std::min<uint64_t>(squares, resident)), dim3(kBlock),
                       c.lds, c.s, sc, fh, queues);
    return 0;
  });
  LT_HIP_CHECK(ctx, hipGetLastError());
  ctx->camhit_passes++;
  if (wantCuts && timingCall) {
    if (const int rc = launch_entry_cuts(ctx, c, sc, fh, false)) return rc;
    set_entry_cuts(ctx, fp, ctx->cuts_chunks);
  }
  if (c.k.camera_hits_keep) {
    fp.storeHeadHits = 1u;
    pendingKey = camera_hits_key(ctx, fh, c.d, c.devlibm);
  }
  return LT_OK;
}

// `rb`: lt_hip_render's read-back of out_device (= ctx->d_out, on ctx->stream), whose pieces the call's last fold follows; null
// for lt_hip_render_device.
static int render_on_stream(lt_hip_context* ctx, const lt_hip_render_desc* d, const TilePlan& p, float* out_device, uint64_t out_bytes,
                            hipStream_t s, const RenderKnobs& k, ReadBack* rb) {
  if (const int rc = check_render_desc(ctx, d, p, out_device, out_bytes)) return rc;
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool stats = (d->flags & (LT_RENDER_FLAG_STATS | LT_RENDER_FLAG_PIXEL_COUNTERS)) != 0;
  const int devlibm = (d->flags & LT_RENDER_FLAG_PORTABLE_MATH) ? 0 : (d->flags & LT_RENDER_FLAG_STRICT_MATH) ? 1 : 2;
  SceneDev sc = scene_dev(ctx, k, devlibm);
  FrameParams fp = frame_params(d, p, k);
  uint32_t camFrame;
  memcpy(&camFrame, d->camera + 24, 4);
  const uint32_t frames = d->frame_count ? d->frame_count : 1;
  const uint64_t nblocks = p.squares();

  // The scratch of a render -- work counters, sample images, shadow queue, the camera hits and what they are kept for -- is the
  // context's: a render enqueued on another stream than the one before it waits for that one's last launch (the writer of the hits a
  // reusing call reads; the last reader of hits about to be overwritten).  One stream: no waits.
  if (!ctx->render_ev) LT_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->render_ev, hipEventDisableTiming));
  if (ctx->render_ev_recorded && s != ctx->render_stream) LT_HIP_CHECK(ctx, hipStreamWaitEvent(s, ctx->render_ev, 0));
  if (stats) LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_stats, 0, 8 * sizeof(unsigned long long), s));
  ctx->last_clear_queues = nullptr;   // (it points into d_queues, which may move below)
  if (k.persistent) {   // (persistent wavefronts by default; LT_PERSISTENT=0 selects one-square-per-workgroup dispatch: A/B measurements)
    const uint64_t queueBytes = ((uint64_t)frames + 1) * 8 * kQueueStride * sizeof(uint32_t);   // (the last eight: the camera-hit pass's)
    LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_queues, ctx->queue_frames, (uint64_t)frames + 1, queueBytes));
    LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_queues, 0, queueBytes, s));
    if (k.square_order)
      if (const int rc = ensure_square_order(ctx, d, p, fp.sinYaw == 0.0f, s, &fp.order, fp.orderHead)) return rc;
  }
  FusionPlan fu;
  if (const int rc = plan_fusion(ctx, k, d, p, frames, stats, fp.giMaxDepth, fu)) return rc;
  const bool fused = fu.chunk > 1, meanInLaunch = d->frame_count && d->accumulate && !fused;
  const uint32_t firstFrames = fused ? std::min(fu.chunk, frames) : 1u;   // frames of the first (and largest) launch
  // (keyed on the image geometry too: how coherent a wavefront's 64 shadow rays are depends on how large its 8x8 pixels are in the
  // scene; and on the frames per launch in three classes: a launch pays a fixed price for its slowest squares, which the walks share
  // out differently.  shadow_mode[program] keeps the most recent verdict for callers without a geometry of their own: the GI pipeline)
  const std::vector<uint32_t> shadowKey = {(uint32_t)d->program, d->width, d->height, p.tileW, p.tileH, p.tileFirst, p.tileStride,
                                           firstFrames == 1u ? 1u : firstFrames < 8u ? 2u : 8u};
  // (the slots: a 32-bit index, and lt_shadow_resolve_kernel strides over them with `i += stride` in 32 bits -- its grid of 8 blocks
  // of 256 threads per CU: the count stays one stride below 2^32, or the sum would wrap and the loop never end)
  const bool queueOk = d->program == LT_PROGRAM_ACCUMULATOR && k.persistent && !stats && ctx->d_rank8 != nullptr && !meanInLaunch &&
                       nblocks * firstFrames * kBlock + (uint64_t)ctx->cu_count * 2048u <= 0xffffffffull;
  int shadowMode = choose_shadow_walk(ctx, k, d, shadowKey, queueOk || nblocks == 0);
  // frames per work item of walks 1 and 2 (launch_walk): LT_SHADOW_FRAMES where the walk is forced, else what it was timed with
  uint32_t shadowGroup = k.shadow_frames;
  if (k.shadow_packets < 0 && ctx->shadow_groups.count(shadowKey)) shadowGroup = ctx->shadow_groups[shadowKey];
  sc.shadowPackets = shadowMode > 0 ? (uint32_t)shadowMode : 0u;
  const bool calibrate = k.persistent && !stats && ctx->bvh_height <= kLdsStack && !meanInLaunch;

  // LDS stack rows: a lane never holds more entries than a node has interior ancestors (= bvh_height, validate_scene).  The counting
  // kernels (and the LDS-resident small scenes of the GI bounce stage: launch_gi_sample) keep one stack entry per lane and level of
  // the caller's tree in LDS; the others the kOwnRows rows of the per-lane walks over the own tree (the packet walks park their
  // stack register in the first of them).  LT_DEBUG_LDS_ROWS (occupancy experiments, tests): more rows than the launch needs, for
  // every kernel; FEWER only for the counting kernels, whose deep-tree form keeps what does not fit in private memory (the others
  // index their rows with compile-time bounds).  The kernel is told what it got (FrameParams::ldsRows) and the form is chosen from that.
  const uint32_t rowBytes = (uint32_t)(kBlock * sizeof(int));
  const uint32_t ldsRefBytes = (uint32_t)std::max(kPacketRows, std::min(ctx->bvh_height, kLdsStack)) * rowBytes;
  uint32_t lds = stats ? ldsRefBytes : (uint32_t)std::max(kPacketRows, kOwnRows) * rowBytes;
  if (k.debug_lds_rows) lds = stats ? k.debug_lds_rows * rowBytes : std::max(lds, k.debug_lds_rows * rowBytes);
  fp.ldsRows = lds / rowBytes;
  // (the non-counting kernels have no deep-tree form: they keep no per-lane stack of the caller's tree in LDS)
  RenderCall call{d, k, s, stats && (uint32_t)ctx->bvh_height > fp.ldsRows, stats, devlibm, lds, ldsRefBytes, nblocks, 0u};
  const bool paddedTiles = d->width % p.tileW != 0 || d->height % p.tileH != 0;
  const uint32_t resident = (uint32_t)ctx->cu_count * 32u;   // every wave slot of the chip, once
  ctx->mean_pairs = 0;
  LT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, s));
  // entry cuts: for the walks that take them (the two-frame packet walk of shadow walks 1 and 2; a walk yet to be timed is timed with them)
  const bool wantCuts = k.entry_cut && ctx->d_pairs2 != nullptr && lt_entry_cut::entry_cut_limit(ctx->height2) != 0 && shadowGroup >= 2u &&
                        (shadowMode < 0 || shadowMode == 1 || shadowMode == 2);
  std::vector<unsigned char> hitsKey;   // (launch_camera_hits: what the hits will belong to once the first launch has stored the head squares')
  if (k.camera_hits && k.persistent && !stats && frames > 1 && nblocks > 0 && d->program == LT_PROGRAM_ACCUMULATOR)
    if (const int rc = launch_camera_hits(ctx, call, sc, fp, ctx->d_queues + (size_t)frames * 8 * kQueueStride, resident, hitsKey, wantCuts, shadowMode < 0 && calibrate)) return rc;
  for (uint32_t f = 0, launchIndex = 0; f < frames && nblocks > 0; launchIndex++) {
    const uint32_t nf = fused ? std::min(fu.chunk, frames - f) : 1u;   // frames of this launch
    fp.frameCount = d->frame_count ? d->frame_first + f : camFrame;
    fp.accumulateN = meanInLaunch ? (int32_t)(d->accumulate_base + f) : -1;
    fp.fusedFrames = nf;
    fp.frameStride = fused ? p.floats : 0;
    float* const out = fused ? ctx->d_samples : out_device;
    const dim3 grid(k.persistent ? (uint32_t)std::min<uint64_t>(nblocks * nf, resident) : (uint32_t)nblocks);
    uint32_t* queues = k.persistent ? ctx->d_queues + (size_t)launchIndex * 8 * kQueueStride : nullptr;
    const unsigned char* foldMap = nullptr;   // the map this launch folds its whole squares by, and its fold skips them by
    bool tabled = false;                      // this launch hands out from the item table
    if (fu.giWavefront) {
      SceneDev scGi = sc;
      scGi.shadowPackets = k.shadow_packets >= 0 ? sc.shadowPackets : 0u;   // the pipeline's bounce stages cast incoherent shadow rays: per lane
      if (const int rc = launch_gi_sets(ctx, call, scGi, fp, fu.giPixels, fu.samplesPerSet, p.floats, out, out_device)) return rc;
      call.launches--;   // (counted again below)
    } else if (d->program >= LT_PROGRAM_USER_BASE) {
      const lt_hip_context::UserProgram& up = ctx->user_programs[d->program - LT_PROGRAM_USER_BASE];
      unsigned long long* statsPtr = ctx->d_stats;
      float* outPtr = out;
      void* args[] = {(void*)&sc, (void*)&fp, (void*)&outPtr, (void*)&statsPtr, (void*)&queues};
      const hipFunction_t fn = devlibm == 2 ? up.lds : devlibm == 1 ? up.ldsStrict : up.ldsPortable;
      LT_HIP_CHECK(ctx, hipModuleLaunchKernel(fn, grid.x, 1, 1, kBlock, 1, 1, lds, s, args, nullptr));
    } else {
      // The item table (ensure_clear_items): for a launch of frame groups over the kept cuts of a reusing call -- every square stored
      // (launch_camera_hits has cleared orderHead), square-major, walk 1 or 2 as forced or remembered (not the launch that times the
      // walks: its candidates run one after the other into the same output) -- whose entries fit 31 bits.  Folding by the items themselves on
      // top of it: a fused launch whose fold runs in quads over whole 8-pixel segments.
      FrameParams fl = fp;
      const uint32_t groups = (nf + 1u) / 2u;
      if (k.clear_items && k.persistent && !stats && d->program == LT_PROGRAM_ACCUMULATOR && (shadowMode == 1 || shadowMode == 2) && fp.entryCuts != nullptr && ctx->cuts_valid && fp.cameraHits != nullptr &&
          std::all_of(fp.orderHead, fp.orderHead + 8, [](uint32_t h) { return h == 0u; }) && std::min(shadowGroup, k.shadow_frames) >= 2u &&
          nf >= 2u && fp.squareMajor != 0u && nblocks * groups < 0x80000000ull) {
        const bool fold = k.clear_items_fold && fused && mean_in_quads(fp.depth, paddedTiles, out_device) && p.tileW % 8u == 0u;
        if (const int rc = ensure_clear_items(ctx, call, fl, groups, fold, p.floats, out_device, (int32_t)(d->accumulate_base + f))) return rc;
      }
      foldMap = (const unsigned char*)fl.foldMap;
      tabled = fl.itemTable != nullptr;
      // (a whole square's frame groups in one pass, render_clear_square; not where the launch counts its groups' walks, launch_walk)
      const bool onePass = tabled && k.clear_square && !k.debug_shadow_frames;
      if (onePass) fl.itemGroups |= kItemGroupsOnePass;
      ctx->last_clear_queues = onePass ? queues : nullptr;
      if (shadowMode < 0 && calibrate)
        if (const int rc = calibrate_shadow_walk(ctx, call, sc, fp, grid, out, queues, queueOk, shadowKey, shadowMode, shadowGroup)) return rc;
      if (const int rc = launch_walk(ctx, call, sc, (uint32_t)std::max(0, shadowMode), shadowGroup, fl, grid, out, queues)) return rc;
    }
    LT_HIP_CHECK(ctx, hipGetLastError());
    call.launches++;
    if (fp.storeHeadHits) {   // the pass and the launch that stores the head squares' hits are enqueued: the hits are whole
      ctx->camhits_key.swap(hitsKey);
      fp.storeHeadHits = 0u;
    }
    if (fused)
      if (const int rc = launch_running_mean(ctx, s, fp, p.floats, nf, (int32_t)(d->accumulate_base + f), paddedTiles, out_device, f + nf >= frames ? rb : nullptr, foldMap))
        return rc;
    ctx->last_folded = (launchIndex != 0 && ctx->last_folded) || foldMap != nullptr;
    ctx->last_tabled = (launchIndex != 0 && ctx->last_tabled) || tabled;
    f += nf;
  }
  LT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, s));
  LT_HIP_CHECK(ctx, hipEventRecord(ctx->render_ev, s));
  ctx->render_stream = s;
  ctx->render_ev_recorded = true;
  ctx->last = lt_hip_stats{};
  ctx->last.frames = frames;
  ctx->last.kernel_launches = call.launches;
  ctx->last.shadow_packets = shadowMode;
  // pixels actually inside the image for this call's tiles
  uint64_t px = 0;
  for (uint32_t t = 0; t < p.tilesInCall; t++) {
    const uint32_t tile = p.tileFirst + t * p.tileStride, tx = tile % p.tilesX, ty = tile / p.tilesX;
    const uint32_t w = std::min(p.tileW, d->width - tx * p.tileW), h = std::min(p.tileH, d->height - ty * p.tileH);
    px += (uint64_t)w * h;
  }
  ctx->last.pixels = px;
  ctx->pending = true;
  ctx->pending_stats = stats;
  ctx->pending_query = false;
  return LT_OK;
}

static int finish_pending(lt_hip_context* ctx) {
  if (!ctx->pending) return LT_OK;
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LT_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
  float ms = 0.0f;
  LT_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  ctx->last.kernel_ms = ms;
  float meanMs = 0.0f;
  for (uint32_t i = 0; i < ctx->mean_pairs; i++) {
    float m = 0.0f;
    LT_HIP_CHECK(ctx, hipEventElapsedTime(&m, ctx->mean_events[2 * i], ctx->mean_events[2 * i + 1]));
    meanMs += m;
  }
  ctx->last.render_ms = ctx->pending_query ? 0.0f : ms - meanMs;
  if (ctx->pending_stats) {
    unsigned long long h[8];
    LT_HIP_CHECK(ctx, hipMemcpy(h, ctx->d_stats, sizeof(h), hipMemcpyDeviceToHost));
#ifdef LT_DEBUG_WAVE_COUNTERS
    fprintf(stderr, "[lt debug] wave-level: node steps %llu (lane-level %llu, utilisation %.3f), triangle blocks %llu (lane-level %llu, utilisation %.3f), outer iterations %llu\n",
            h[4], h[2], (double)h[2] / (64.0 * (double)h[4]), h[5], h[3], (double)h[3] / (64.0 * (double)h[5]), h[6]);
#endif
    ctx->last.rays = h[0]; ctx->last.shadow_rays = h[1]; ctx->last.node_visits = h[2]; ctx->last.tri_tests = h[3];
  }
  ctx->pending = false;
  return LT_OK;
}

extern "C" int lt_hip_render_device(lt_hip_context* ctx, const lt_hip_render_desc* desc, float* out_device, uint64_t out_bytes,
                                    void* hip_stream) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  if (!ctx->has_scene) return fail(ctx, LT_ERR_NO_SCENE, "lt_hip_render before lt_hip_set_scene");
  TilePlan p;
  std::string msg;
  if (const int rc = plan_tiles(desc, p, msg)) return fail(ctx, rc, msg);
  return render_on_stream(ctx, desc, p, out_device, out_bytes, (hipStream_t)hip_stream, RenderKnobs(), nullptr);
}

// The read-back of lt_hip_render: device -> the context's pinned buffer in eight pieces (enqueued behind the kernels), each piece
// copied on to the caller's buffer by a few host threads as soon as it has arrived, so that the link and the host's copy overlap.
// LT_PINNED_READBACK=0: one hipMemcpyAsync into the caller's (pageable) buffer, as round 2 did it.
static int enqueue_readback(lt_hip_context* ctx, float* out_host, ReadBack& rb) {
  if (rb.piece && ctx->h_out_bytes < rb.need) {
    if (ctx->h_out) (void)hipHostFree(ctx->h_out);
    ctx->h_out_bytes = 0;
    if (hipHostMalloc(&ctx->h_out, rb.need, hipHostMallocDefault) == hipSuccess) ctx->h_out_bytes = rb.need;
    else { (void)hipGetLastError(); ctx->h_out = nullptr; rb.piece = 0; }
  }
  if (!rb.piece) {
    LT_HIP_CHECK(ctx, hipMemcpyAsync(out_host, ctx->d_out, rb.need, hipMemcpyDeviceToHost, ctx->stream));
    return LT_OK;
  }
  for (hipEvent_t& e : ctx->out_ev) if (!e) LT_HIP_CHECK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipStream_t cs = ctx->stream;
  if (rb.foldPieced) {   // (the frame's last fold came in these pieces: each travels behind its own)
    if (!ctx->copy_stream) LT_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    cs = ctx->copy_stream;
  }
  for (int k = 0; k < 8; k++) {
    const uint64_t off = std::min(rb.need, (uint64_t)k * rb.piece), n = std::min(rb.piece, rb.need - off);
    if (cs != ctx->stream) LT_HIP_CHECK(ctx, hipStreamWaitEvent(cs, ctx->fold_ev[k], 0));
    if (n) LT_HIP_CHECK(ctx, hipMemcpyAsync((char*)ctx->h_out + off, (const char*)ctx->d_out + off, n, hipMemcpyDeviceToHost, cs));
    LT_HIP_CHECK(ctx, hipEventRecord(ctx->out_ev[k], cs));
  }
  return LT_OK;
}
static int finish_readback(lt_hip_context* ctx, float* out_host, const ReadBack& rb) {
  if (!rb.piece) {
    LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return LT_OK;
  }
  const int threads = std::max(1, std::min(8, host_threads()));
  std::atomic<int> failed{0};
  auto work = [&](int t, int of) {
    (void)hipSetDevice(ctx->device);
    for (int k = 0; k < 8; k++) {
      if (hipEventSynchronize(ctx->out_ev[k]) != hipSuccess) { failed = 1; return; }
      const uint64_t off = std::min(rb.need, (uint64_t)k * rb.piece), n = std::min(rb.piece, rb.need - off);
      const uint64_t lo = off + n * (uint64_t)t / (uint64_t)of, hi = off + n * (uint64_t)(t + 1) / (uint64_t)of;
      memcpy((char*)out_host + lo, (const char*)ctx->h_out + lo, (size_t)(hi - lo));
    }
  };
  std::vector<std::thread> pool;
  int started = 1;
  try {
    for (; started < threads; started++) pool.emplace_back(work, started, threads);
  } catch (...) {
  }
  work(0, threads);
  for (std::thread& th : pool) th.join();
  for (int t = started; t < threads; t++) work(t, threads);   // (the slices of the threads that could not be had)
  LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->copy_stream) LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->copy_stream));
  if (failed) return fail(ctx, LT_ERR_HIP, "read-back failed");
  return LT_OK;
}

// lt_hip_render up to the enqueued read-back: the image is rendered into ctx->d_out and travels to out_host (finish_readback).
static int render_to_host(lt_hip_context* ctx, const lt_hip_render_desc* desc, float* out_host, uint64_t out_bytes, const RenderKnobs& k, ReadBack& rb) {
  if (!out_host) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "output pointer is NULL");
  TilePlan p;
  std::string msg;
  if (const int rc = plan_tiles(desc, p, msg)) return fail(ctx, rc, msg);
  rb = ReadBack{};
  rb.need = p.floats * sizeof(float);
  if (out_bytes < rb.need) return fail(ctx, LT_ERR_BUFFER_TOO_SMALL, "outputBufferSize smaller than W*H*depth floats");
  if (!ctx->has_scene) return fail(ctx, LT_ERR_NO_SCENE, "lt_hip_render before lt_hip_set_scene");
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_out, ctx->d_out_bytes, rb.need, rb.need ? rb.need : 4));
  // a running mean continues from the caller's buffer when accumulate_base > 0
  if (desc->frame_count && desc->accumulate && desc->accumulate_base > 0)
    LT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_out, out_host, rb.need, hipMemcpyHostToDevice, ctx->stream));
  else
    LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_out, 0, rb.need, ctx->stream));
  rb.piece = readback_piece(k, rb.need);
  const int rc = render_on_stream(ctx, desc, p, ctx->d_out, rb.need, ctx->stream, k, &rb);
  return rc == LT_OK ? enqueue_readback(ctx, out_host, rb) : rc;
}

// lt_hip_render, its host time counted from t0 (lt_hip_stats::total_ms)
static int render_host(lt_hip_context* ctx, const lt_hip_render_desc* desc, float* out_host, uint64_t out_bytes, const RenderKnobs& k,
                       std::chrono::steady_clock::time_point t0) {
  ReadBack rb;
  int rc = render_to_host(ctx, desc, out_host, out_bytes, k, rb);
  if (rc == LT_OK) rc = finish_readback(ctx, out_host, rb);
  if (rc == LT_OK) rc = finish_pending(ctx);
  if (rc == LT_OK) ctx->last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

extern "C" int lt_hip_render(lt_hip_context* ctx, const lt_hip_render_desc* desc, float* out_host, uint64_t out_bytes) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  return render_host(ctx, desc, out_host, out_bytes, RenderKnobs(), t0);
}

// lt_hip_set_scene + lt_hip_render in one call, as the plugin's render() needs them (the reference hands over its scene on every
// call, renderer_opencl.cpp:107-120): when the buffers have the resident scene's sizes, the frame is rendered and read back ON
// THE ASSUMPTION that nothing changed while this thread hashes the buffers; the hash decides whether the frame stands.  It
// nearly always does -- and then the hash of 140 MB of scene has cost nothing, hidden behind the frame's 17 ms -- or the scene
// is uploaded and the frame rendered again.
extern "C" int lt_hip_render_scene(lt_hip_context* ctx, const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                                   const void* materials, uint64_t material_bytes, const void* lights, uint64_t light_bytes,
                                   const lt_hip_render_desc* desc, float* out_host, uint64_t out_bytes) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  if (!nodes || !prims || !materials || !lights) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "NULL scene buffer");
  try {
    const auto t0 = std::chrono::steady_clock::now();
    const SceneKnobs sk;
    const RenderKnobs rk;
    const uint64_t sizes[4] = {node_bytes, prim_bytes, material_bytes, light_bytes};
    const void* const bufs[4] = {nodes, prims, materials, lights};
    const bool continues = desc && desc->frame_count && desc->accumulate && desc->accumulate_base > 0;   // (reads the caller's buffer: no second try)
    // Rendering from the resident copy while the host hashes what came with the frame pays when the scene is the resident one --
    // a still scene, every call but the first.  A caller whose scene changed last time (an animation) gets the hash first: a
    // millisecond in front of the frame instead of a whole frame rendered for nothing.
    const bool speculate = ctx->has_scene && ctx->scene_hash_valid && ctx->speculate_next && memcmp(sizes, ctx->scene_sizes, sizeof(sizes)) == 0 &&
                           !sk.always_upload && !continues;
    int rc;
    if (speculate) {
      ReadBack rb;
      rc = render_to_host(ctx, desc, out_host, out_bytes, rk, rb);
      if (rc) return rc;
      const SceneHash hash = hash_scene(bufs, sizes);   // (while the GPU renders)
      if ((rc = finish_readback(ctx, out_host, rb))) return rc;
      const bool stands = hash == ctx->scene_hash;
      if (stands) ctx->scene_reused++;
      if ((rc = finish_pending(ctx))) return rc;
      if (stands) {
        ctx->last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return LT_OK;
      }
      ctx->speculate_next = false;
      rc = set_scene_impl(ctx, nodes, node_bytes, prims, prim_bytes, materials, material_bytes, lights, light_bytes, sk, &hash);
    } else {
      const uint32_t reused = ctx->scene_reused;
      rc = set_scene_impl(ctx, nodes, node_bytes, prims, prim_bytes, materials, material_bytes, lights, light_bytes, sk, nullptr);
      ctx->speculate_next = rc == LT_OK && ctx->scene_reused != reused;   // (the resident scene again: the next frame may start at once)
    }
    if (rc) return rc;
    return render_host(ctx, desc, out_host, out_bytes, rk, t0);
  } catch (const std::exception& e) {
    return fail(ctx, LT_ERR_HIP, std::string("lt_hip_render_scene: ") + e.what());
  }
}

// ---------------------------------------------------------------------------------- ray queries
// Ten families of entry points take caller-supplied records against the resident scene, each in a host and a _device form:
// lt_hip_trace_rays, lt_hip_trace_hits, lt_hip_trace_surface, lt_hip_surface_at (lt_query.hip), lt_hip_shade_rays (lt_shade.hip),
// lt_hip_shade_paths (lt_paths.hip), lt_hip_nearest_points and lt_hip_nearest_k (lt_nearest.hip), lt_hip_overlap_boxes
// (lt_overlap.hip), lt_hip_overlap_tris (lt_tritri.hip).  (The lists, lt_hip_overlap_boxes_list, lt_hip_overlap_tris_list,
// lt_hip_nearest_list and lt_hip_trace_hits_list -- lt_overlist.hip --, have two result buffers and a course of their own: run_list_call, behind the triangle queries.)  Every argument error is found before anything is enqueued, so that a failed call writes nothing to `out`.  What the families share is written once: the rules about flags and buffers (check_ray_flags,
// check_ray_buffers), the course of an entry point with the host form's staging (run_ray_call) and the events and statistics
// around the launches (begin_ray_launches, end_ray_launches).  A family has its check (the rules about its descriptor, at their
// place in the order), its launches (enqueue_*) and two one-line entry points.
static_assert(sizeof(lt_hip_ray) == 32 && sizeof(lt_hip_hit) == 16 && sizeof(lt_hip_trace_desc) == 16, "ray query records (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_multihit_desc) == 24 && LT_TRACE_MAX_HITS == lt_query::kMaxHits, "multi-hit records (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_surface) == 48 && sizeof(lt_hip_surface_desc) == 8, "surface records (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_shade_ray) == 32 && sizeof(lt_hip_shade) == 16 && sizeof(lt_hip_shade_desc) == 24, "shaded-ray records (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_paths_desc) == 32, "path-shading descriptor (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_point) == 16 && sizeof(lt_hip_nearest_desc) == 8, "nearest-point records (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_nearest_k_desc) == 16 && LT_NEAREST_MAX_K == lt_nearest::kMaxK && LT_NEAREST_FIRST_K == lt_nearest::kFirstK &&
                  LT_NEAREST_COUNT == lt_nearest::kCount,
              "k-nearest records (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_box) == 32 && sizeof(lt_hip_overlap_desc) == 16 && LT_OVERLAP_MAX_K == lt_overlap::kMaxK &&
                  LT_OVERLAP_FIRST_K == lt_overlap::kFirstK && LT_OVERLAP_COUNT == lt_overlap::kCount && LT_OVERLAP_ANY == lt_overlap::kAny,
              "box-overlap records (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_tri) == 48, "triangle-overlap records (include/lenstrace_hip.h)");

// What every family's check leaves for its launches: the math flavour (SceneDev: 0 portable, 1 strict, 2 as shipped) and the bytes
// of one result.
struct RayCall {
  int devlibm;
  uint64_t outRecord;
  bool chunkGrid = false;   // the call launches one 64-lane workgroup per 64 records (lt_query_packet_kernel)
};

// The nouns of a family's error texts: the call, its records, what a batch of them is, the input pointer.
struct RayWording { const char *call, *records, *batch, *in; };
constexpr RayWording kQueryWording{"ray query", "rays", "query", "rays"};
constexpr RayWording kSurfaceAtWording{"lt_hip_surface_at", "hit records", "call", "hits"};
constexpr RayWording kShadeWording{"lt_hip_shade_rays", "rays", "call", "rays"};
constexpr RayWording kPathsWording{"lt_hip_shade_paths", "rays", "call", "rays"};
constexpr RayWording kNearestWording{"lt_hip_nearest_points", "points", "call", "points"};
constexpr RayWording kNearestKWording{"lt_hip_nearest_k", "points", "call", "points"};
constexpr RayWording kOverlapWording{"lt_hip_overlap_boxes", "boxes", "call", "boxes"};
constexpr RayWording kOverlapTrisWording{"lt_hip_overlap_tris", "triangles", "call", "tris"};

// The flags of a call: the two math flags and, `coherent`, LT_TRACE_FLAG_COHERENT; `who`: the family's "... take(s)".
static int check_ray_flags(lt_hip_context* ctx, uint32_t flags, bool coherent, const char* who, RayCall& call) {
  const uint32_t allowed = LT_RENDER_FLAG_STRICT_MATH | LT_RENDER_FLAG_PORTABLE_MATH | (coherent ? LT_TRACE_FLAG_COHERENT : 0u);
  if (flags & ~allowed)
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string(who) + (coherent ? " LT_RENDER_FLAG_STRICT_MATH, LT_RENDER_FLAG_PORTABLE_MATH and LT_TRACE_FLAG_COHERENT only"
                                                                        : " LT_RENDER_FLAG_STRICT_MATH and LT_RENDER_FLAG_PORTABLE_MATH only"));
  if ((flags & LT_RENDER_FLAG_PORTABLE_MATH) && (flags & LT_RENDER_FLAG_STRICT_MATH))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, "LT_RENDER_FLAG_PORTABLE_MATH and LT_RENDER_FLAG_STRICT_MATH exclude each other");
  call.devlibm = (flags & LT_RENDER_FLAG_PORTABLE_MATH) ? 0 : (flags & LT_RENDER_FLAG_STRICT_MATH) ? 1 : 2;
  return LT_OK;
}

// The records of a call and the room for its results (call.outRecord bytes each), once the descriptor has passed.
static int check_ray_buffers(lt_hip_context* ctx, const RayWording& w, const void* in, uint64_t n, const void* out, uint64_t out_bytes, bool device,
                             const RayCall& call) {
  if (n > 0xffffffffull) return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string("at most 2^32 - 1 ") + w.records + " per " + w.batch);
  // A grid of ceil(n / 64) workgroups of 64 lanes has 2^32 work-items from n = 2^32 - 63 on, one more than a dispatch's 32-bit
  // grid size holds: the launch would fail.  Every other kernel of these calls runs a grid of the chip's size.
  if (call.chunkGrid && n > 0xffffffc0ull)
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string("at most 2^32 - 64 ") + w.records + " per " + w.batch + " with LT_TRACE_FLAG_COHERENT");
  if (n > 0 && (!in || !out)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string(w.in) + " or out is NULL");
  if (device && n > 0 && (((uintptr_t)in | (uintptr_t)out) & 15u))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string("device ") + w.in + " and out must be 16-byte aligned");
  if (!ctx->has_scene) return fail(ctx, LT_ERR_NO_SCENE, std::string(w.call) + " before lt_hip_set_scene");
  if (out_bytes < n * call.outRecord) return fail(ctx, LT_ERR_BUFFER_TOO_SMALL, "out is smaller than n results");
  return LT_OK;
}

// The program of a query: a built-in one, for the triangle epsilon of its intersect.
static int query_epsilon(lt_hip_context* ctx, int program, lt_query::Epsilon& eps) {
  if (program >= LT_PROGRAM_USER_BASE) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "ray queries take a built-in program (it selects the triangle epsilon)");
  if (program < LT_PROGRAM_BASIC || program > LT_PROGRAM_CUSTOM_OPENCL) return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "unknown program");
  eps = (program == LT_PROGRAM_BASIC || program == LT_PROGRAM_CUSTOM_OPENCL) ? lt_query::kEpsFloat7
        : program == LT_PROGRAM_BASIC_LIGHTING ? lt_query::kEpsDouble7 : lt_query::kEpsDouble4;
  return LT_OK;
}

// The program of a shade family: a built-in one; `noUserPrograms`: the family's text for a user program the context knows.
static int check_shade_program(lt_hip_context* ctx, int program, const char* noUserPrograms) {
  const bool userProgram = program >= LT_PROGRAM_USER_BASE;
  if (userProgram ? (size_t)(program - LT_PROGRAM_USER_BASE) >= ctx->user_programs.size()
                  : (program < LT_PROGRAM_BASIC || program > LT_PROGRAM_CUSTOM_OPENCL))
    return fail(ctx, LT_ERR_UNKNOWN_PROGRAM, "unknown program");
  if (userProgram) return fail(ctx, LT_ERR_INVALID_ARGUMENT, noUserPrograms);
  return LT_OK;
}

// Every entry point: the family's check, then -- n > 0 -- its launches.  The device form enqueues them on the caller's stream.
// The host form stages the records and the results in two buffers of the context that all the families share, runs on the
// context's stream and waits.
template <class Call, class Desc, class Record>
static int run_ray_call(lt_hip_context* ctx, const Desc* desc, const Record* in, uint64_t n, void* out, uint64_t out_bytes, bool device,
                        void* hip_stream,
                        int (*check)(lt_hip_context*, const Desc*, const Record*, uint64_t, const void*, uint64_t, bool, Call&),
                        int (*enqueue)(lt_hip_context*, const Call&, const void*, uint64_t, void*, hipStream_t)) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  Call call{};
  if (const int rc = check(ctx, desc, in, n, out, out_bytes, device, call)) return rc;
  if (n == 0) return LT_OK;
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (device) return enqueue(ctx, call, in, n, out, (hipStream_t)hip_stream);
  const uint64_t inBytes = n * sizeof(Record), outBytes = n * call.outRecord;
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_query_rays, ctx->query_rays_bytes, inBytes, inBytes));
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_query_out, ctx->query_out_bytes, outBytes, outBytes));
  LT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_query_rays, in, inBytes, hipMemcpyHostToDevice, ctx->stream));
  if (const int rc = enqueue(ctx, call, ctx->d_query_rays, n, ctx->d_query_out, ctx->stream)) return rc;
  LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (const int rc = finish_pending(ctx)) return rc;
  LT_HIP_CHECK(ctx, hipMemcpy(out, ctx->d_query_out, outBytes, hipMemcpyDeviceToHost));
  return LT_OK;
}

// The eight work counters of a family's kernels (kQueueStride apart), allocated at its first call.
static hipError_t ensure_ray_counters(uint32_t*& ctl) {
  return ctl ? hipSuccess : hipMalloc((void**)&ctl, 8 * kQueueStride * sizeof(uint32_t));
}

// Around the launches of a call on `s`.  `ev`: the event behind the family's last call, or null (lt_hip_surface_at: it has no
// state of its own) -- the counters and the scratch are the previous call's until it is done, on whichever stream that was.  The
// context's timing events bracket the launches; lt_hip_get_stats reports them (finish_pending).
static int begin_ray_launches(lt_hip_context* ctx, hipEvent_t* ev, hipStream_t s) {
  if (ev && !*ev) LT_HIP_CHECK(ctx, hipEventCreateWithFlags(ev, hipEventDisableTiming));
  else if (ev) LT_HIP_CHECK(ctx, hipStreamWaitEvent(s, *ev, 0));
  ctx->mean_pairs = 0;
  LT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, s));
  return LT_OK;
}

static int end_ray_launches(lt_hip_context* ctx, hipEvent_t ev, hipStream_t s, uint32_t launches, uint64_t rays, uint64_t shadowRays) {
  LT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, s));
  if (ev) LT_HIP_CHECK(ctx, hipEventRecord(ev, s));
  ctx->last = lt_hip_stats{};
  ctx->last.kernel_launches = launches;
  ctx->last.rays = rays;
  ctx->last.shadow_rays = shadowRays;
  ctx->pending = true;
  ctx->pending_stats = false;
  ctx->pending_query = true;
  return LT_OK;
}

// lt_hip_trace_rays*: closest or any hit of each ray.  lt_hip_trace_surface* (`surface`): closest hits with the surface record
// behind them -- lt_hip_trace_rays' launch into a scratch buffer of the context, then lt_hip_surface_at's over it.  By definition
// the call equals those two, and the one-kernel form -- the query kernels writing the record themselves -- was slower than the pair
// on incoherent rays.
struct TraceCall : RayCall {
  lt_query::Epsilon eps;
  bool anyHit, coherent, surface;
};

template <bool SURFACE>
static int check_trace(lt_hip_context* ctx, const lt_hip_trace_desc* d, const lt_hip_ray* rays, uint64_t n, const void* out, uint64_t out_bytes,
                       bool device, TraceCall& tc) {
  tc.surface = SURFACE;
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_trace_rays: desc is NULL");
  if (d->struct_size < sizeof(lt_hip_trace_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "bad lt_hip_trace_desc (struct_size)");
  if (d->kind != LT_TRACE_CLOSEST && d->kind != LT_TRACE_ANY) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "unknown trace kind");
  if (tc.surface && d->kind != LT_TRACE_CLOSEST) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "surface queries take LT_TRACE_CLOSEST");
  if (const int rc = query_epsilon(ctx, d->program, tc.eps)) return rc;
  if (const int rc = check_ray_flags(ctx, d->flags, true, "ray queries take", tc)) return rc;
  tc.anyHit = d->kind == LT_TRACE_ANY;
  tc.coherent = (d->flags & LT_TRACE_FLAG_COHERENT) != 0;
  tc.chunkGrid = tc.coherent;
  tc.outRecord = tc.surface ? sizeof(lt_hip_surface) : tc.anyHit ? sizeof(uint32_t) : sizeof(lt_hip_hit);
  return check_ray_buffers(ctx, kQueryWording, rays, n, out, out_bytes, device, tc);
}

static int enqueue_trace(lt_hip_context* ctx, const TraceCall& tc, const void* rays, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_query_ctl));
  // (growing frees the old buffer, which waits for the calls that use it)
  if (tc.surface) LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_surface_hits, ctx->surface_hits_records, n, n * sizeof(lt_hip_hit)));
  lt_query::Params qp{};
  qp.rays = (const float4*)rays;
  qp.hits = tc.surface ? ctx->d_surface_hits : tc.anyHit ? nullptr : (uint4*)out;
  qp.occluded = tc.anyHit ? (uint32_t*)out : nullptr;
  qp.n = (uint32_t)n;
  qp.next = ctx->d_query_ctl;
  qp.refill = k.trace_refill;
  const SceneDev sc = scene_dev(ctx, k, tc.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->query_ev, s)) return rc;
  LT_HIP_CHECK(ctx, lt_query::launch(sc, qp, tc.eps, tc.anyHit, tc.coherent, (uint32_t)ctx->cu_count, s));
  if (tc.surface)
    LT_HIP_CHECK(ctx, lt_query::launch_surface_at(sc, ctx->d_surface_hits, (uint4*)out, (uint32_t)n, tc.devlibm == 2, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, ctx->query_ev, s, tc.surface ? 2 : 1, tc.anyHit ? 0 : n, tc.anyHit ? n : 0);
}

extern "C" int lt_hip_trace_rays(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n, void* out,
                                 uint64_t out_bytes) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, false, nullptr, check_trace<false>, enqueue_trace);
}

extern "C" int lt_hip_trace_rays_device(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n, void* out,
                                        uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, true, hip_stream, check_trace<false>, enqueue_trace);
}

extern "C" int lt_hip_trace_surface(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n, lt_hip_surface* out,
                                    uint64_t out_bytes) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, false, nullptr, check_trace<true>, enqueue_trace);
}

extern "C" int lt_hip_trace_surface_device(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n, lt_hip_surface* out,
                                           uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, true, hip_stream, check_trace<true>, enqueue_trace);
}

// lt_hip_trace_hits*: the first K hits of each ray, or their number (lt_query_hits_kernel).
struct HitsCall : RayCall {
  lt_query::Epsilon eps;
  uint32_t maxHits;    // 0: count
};

static int check_hits(lt_hip_context* ctx, const lt_hip_multihit_desc* d, const lt_hip_ray* rays, uint64_t n, const void* out, uint64_t out_bytes,
                      bool device, HitsCall& hc) {
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_trace_hits: desc is NULL");
  if (d->struct_size < sizeof(lt_hip_multihit_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "bad lt_hip_multihit_desc (struct_size)");
  if (d->kind != LT_TRACE_FIRST_K && d->kind != LT_TRACE_COUNT) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "unknown multi-hit kind");
  if (const int rc = query_epsilon(ctx, d->program, hc.eps)) return rc;
  if (const int rc = check_ray_flags(ctx, d->flags, true, "ray queries take", hc)) return rc;
  if (d->kind == LT_TRACE_FIRST_K && (d->max_hits < 1 || d->max_hits > LT_TRACE_MAX_HITS))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, "LT_TRACE_FIRST_K takes max_hits in 1 .. LT_TRACE_MAX_HITS");
  if (d->kind == LT_TRACE_COUNT && d->max_hits != 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "LT_TRACE_COUNT takes max_hits = 0");
  if (d->reserved != 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_multihit_desc::reserved must be 0");
  hc.maxHits = d->max_hits;
  hc.outRecord = d->kind == LT_TRACE_COUNT ? sizeof(uint32_t) : d->max_hits * sizeof(lt_hip_hit);
  return check_ray_buffers(ctx, kQueryWording, rays, n, out, out_bytes, device, hc);
}

static int enqueue_hits(lt_hip_context* ctx, const HitsCall& hc, const void* rays, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_query_ctl));
  lt_query::HitsParams qp{};
  qp.rays = (const float4*)rays;
  qp.hits = hc.maxHits ? (uint4*)out : nullptr;
  qp.counts = hc.maxHits ? nullptr : (uint32_t*)out;
  qp.n = (uint32_t)n;
  qp.maxHits = hc.maxHits;
  qp.kind = hc.maxHits ? lt_query::kFirstK : lt_query::kCount;
  qp.next = ctx->d_query_ctl;
  qp.refill = k.trace_refill;
  const SceneDev sc = scene_dev(ctx, k, hc.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->query_ev, s)) return rc;
  LT_HIP_CHECK(ctx, lt_query::launch_hits(sc, qp, hc.eps, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, ctx->query_ev, s, 1, n, 0);
}

extern "C" int lt_hip_trace_hits(lt_hip_context* ctx, const lt_hip_multihit_desc* desc, const lt_hip_ray* rays, uint64_t n, void* out,
                                 uint64_t out_bytes) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, false, nullptr, check_hits, enqueue_hits);
}

extern "C" int lt_hip_trace_hits_device(lt_hip_context* ctx, const lt_hip_multihit_desc* desc, const lt_hip_ray* rays, uint64_t n, void* out,
                                        uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, true, hip_stream, check_hits, enqueue_hits);
}

// lt_hip_surface_at*: the surface record of hit records the caller has (lt_surface_at_kernel).  The kernel keeps nothing in the
// context: the call waits for no event and records none.
static int check_surface_at(lt_hip_context* ctx, const lt_hip_surface_desc* d, const lt_hip_hit* hits, uint64_t n, const void* out, uint64_t out_bytes,
                            bool device, RayCall& call) {
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_surface_at: desc is NULL");
  if (d->struct_size < sizeof(lt_hip_surface_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "bad lt_hip_surface_desc (struct_size)");
  if (const int rc = check_ray_flags(ctx, d->flags, false, "lt_hip_surface_at takes", call)) return rc;
  call.outRecord = sizeof(lt_hip_surface);
  return check_ray_buffers(ctx, kSurfaceAtWording, hits, n, out, out_bytes, device, call);
}

static int enqueue_surface_at(lt_hip_context* ctx, const RayCall& call, const void* hits, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  const bool shipped = call.devlibm == 2;
  const SceneDev sc = scene_dev(ctx, k, shipped ? 2 : 1);
  if (const int rc = begin_ray_launches(ctx, nullptr, s)) return rc;
  LT_HIP_CHECK(ctx, lt_query::launch_surface_at(sc, (const uint4*)hits, (uint4*)out, (uint32_t)n, shipped, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, nullptr, s, 1, 0, 0);
}

extern "C" int lt_hip_surface_at(lt_hip_context* ctx, const lt_hip_surface_desc* desc, const lt_hip_hit* hits, uint64_t n, lt_hip_surface* out,
                                 uint64_t out_bytes) {
  return run_ray_call(ctx, desc, hits, n, out, out_bytes, false, nullptr, check_surface_at, enqueue_surface_at);
}

extern "C" int lt_hip_surface_at_device(lt_hip_context* ctx, const lt_hip_surface_desc* desc, const lt_hip_hit* hits, uint64_t n, lt_hip_surface* out,
                                        uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, hits, n, out, out_bytes, true, hip_stream, check_surface_at, enqueue_surface_at);
}

// lt_hip_nearest_points*: the closest primitive of each point (lt_nearest_kernel).  The work counters are the ray queries': the
// call takes its turn behind them (ctx->query_ev).
static int check_nearest(lt_hip_context* ctx, const lt_hip_nearest_desc* d, const lt_hip_point* points, uint64_t n, const void* out, uint64_t out_bytes,
                         bool device, RayCall& call) {
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_nearest_points: desc is NULL");
  if (d->struct_size < sizeof(lt_hip_nearest_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "bad lt_hip_nearest_desc (struct_size)");
  if (d->flags != 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_nearest_points takes no flags");
  call.devlibm = 2;
  call.outRecord = sizeof(lt_hip_hit);
  return check_ray_buffers(ctx, kNearestWording, points, n, out, out_bytes, device, call);
}

static int enqueue_nearest(lt_hip_context* ctx, const RayCall& call, const void* points, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_query_ctl));
  lt_nearest::Params qp{};
  qp.points = (const float4*)points;
  qp.hits = (uint4*)out;
  qp.n = (uint32_t)n;
  qp.next = ctx->d_query_ctl;
  qp.refill = k.trace_refill;
  const SceneDev sc = scene_dev(ctx, k, call.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->query_ev, s)) return rc;
  LT_HIP_CHECK(ctx, lt_nearest::launch(sc, qp, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, ctx->query_ev, s, 1, n, 0);
}

extern "C" int lt_hip_nearest_points(lt_hip_context* ctx, const lt_hip_nearest_desc* desc, const lt_hip_point* points, uint64_t n, lt_hip_hit* out,
                                     uint64_t out_bytes) {
  return run_ray_call(ctx, desc, points, n, out, out_bytes, false, nullptr, check_nearest, enqueue_nearest);
}

extern "C" int lt_hip_nearest_points_device(lt_hip_context* ctx, const lt_hip_nearest_desc* desc, const lt_hip_point* points, uint64_t n,
                                            lt_hip_hit* out, uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, points, n, out, out_bytes, true, hip_stream, check_nearest, enqueue_nearest);
}

// The same answers without a context or a GPU: every leaf of `nodes` (LinearBVHNode) with its one primitive of `prims` (Primitive,
// 76 bytes), the arithmetic of lt_nearest.hpp on the traversal triangle A, fl(B - A), fl(C - A).  Nothing is written unless
// every leaf's offset lies inside `prims`.
extern "C" int lt_hip_nearest_points_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes, const lt_hip_point* points,
                                          uint64_t n, lt_hip_hit* out, uint64_t out_bytes) {
  if (!nodes || !prims || node_bytes == 0 || node_bytes % 32 || node_bytes > 0xffffffffull * 32 || prim_bytes % 76) return LT_ERR_INVALID_ARGUMENT;
  if (n > 0xffffffffull || (n > 0 && (!points || !out))) return LT_ERR_INVALID_ARGUMENT;
  const lt_retree::Node* nd = (const lt_retree::Node*)nodes;
  const uint64_t n_nodes = node_bytes / 32, n_prims = prim_bytes / 76;
  for (uint64_t i = 0; i < n_nodes; i++)
    if (nd[i].cnt != 0 && (nd[i].off < 0 || (uint64_t)nd[i].off >= n_prims)) return LT_ERR_BAD_SCENE;
  if (out_bytes < n * sizeof(lt_hip_hit)) return LT_ERR_BUFFER_TOO_SMALL;
  const float* pr = (const float*)prims;
  for (uint64_t j = 0; j < n; j++) {
    const float px = points[j].p[0], py = points[j].p[1], pz = points[j].p[2];
    lt_nearest::Best best{points[j].max_d2, 0.0f, 0.0f, -1};
    if (!lt_nearest::no_walk(px, py, pz, best.t)) {
      for (uint64_t i = 0; i < n_nodes; i++) {
        if (nd[i].cnt == 0) continue;
        const float* p = pr + 19 * (size_t)nd[i].off;
        const lt_nearest::Tri t = lt_nearest::tri(px, py, pz, p[0], p[1], p[2], p[3] - p[0], p[4] - p[1], p[5] - p[2], p[6] - p[0], p[7] - p[1], p[8] - p[2]);
        const float box = lt_nearest::box_d2(px, py, pz, nd[i].lo[0], nd[i].lo[1], nd[i].lo[2], nd[i].hi[0], nd[i].hi[1], nd[i].hi[2]);
        best.offer(lt_nearest::candidate_d2(t.d2, box), t.u, t.v, nd[i].off);
      }
    }
    memcpy(&out[j].t, &best.t, sizeof(float));   // (max_d2's bits on a miss, a NaN's payload included)
    out[j].prim = best.prim;
    out[j].u = best.u;
    out[j].v = best.v;
  }
  return LT_OK;
}

// lt_hip_nearest_k*: the first K entries of each point's candidate sequence, or its length (lt_nearest_k_kernel).  The descriptor's
// rules, for the context's entry points and the host form alike; null when it passes.
static const char* nearest_k_desc_error(const lt_hip_nearest_k_desc* d) {
  if (!d) return "lt_hip_nearest_k: desc is NULL";
  if (d->struct_size < sizeof(lt_hip_nearest_k_desc)) return "bad lt_hip_nearest_k_desc (struct_size)";
  if (d->flags != 0) return "lt_hip_nearest_k takes no flags";
  if (d->kind != LT_NEAREST_FIRST_K && d->kind != LT_NEAREST_COUNT) return "unknown nearest kind";
  if (d->kind == LT_NEAREST_FIRST_K && (d->max_k < 1 || d->max_k > LT_NEAREST_MAX_K)) return "LT_NEAREST_FIRST_K takes max_k in 1 .. LT_NEAREST_MAX_K";
  if (d->kind == LT_NEAREST_COUNT && d->max_k != 0) return "LT_NEAREST_COUNT takes max_k = 0";
  return nullptr;
}

struct NearestKCall : RayCall {
  uint32_t maxK;   // 0: count
};

static int check_nearest_k(lt_hip_context* ctx, const lt_hip_nearest_k_desc* d, const lt_hip_point* points, uint64_t n, const void* out,
                           uint64_t out_bytes, bool device, NearestKCall& call) {
  if (const char* why = nearest_k_desc_error(d)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, why);
  call.devlibm = 2;
  call.maxK = d->max_k;
  call.outRecord = d->kind == LT_NEAREST_COUNT ? sizeof(uint32_t) : (uint64_t)d->max_k * sizeof(lt_hip_hit);
  return check_ray_buffers(ctx, kNearestKWording, points, n, out, out_bytes, device, call);
}

static int enqueue_nearest_k(lt_hip_context* ctx, const NearestKCall& call, const void* points, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_query_ctl));
  lt_nearest::KParams qp{};
  qp.points = (const float4*)points;
  qp.hits = call.maxK ? (uint4*)out : nullptr;
  qp.counts = call.maxK ? nullptr : (uint32_t*)out;
  qp.n = (uint32_t)n;
  qp.maxK = call.maxK;
  qp.kind = call.maxK ? lt_nearest::kFirstK : lt_nearest::kCount;
  qp.next = ctx->d_query_ctl;
  qp.refill = k.trace_refill;
  const SceneDev sc = scene_dev(ctx, k, call.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->query_ev, s)) return rc;
  LT_HIP_CHECK(ctx, lt_nearest::launch_k(sc, qp, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, ctx->query_ev, s, 1, n, 0);
}

extern "C" int lt_hip_nearest_k(lt_hip_context* ctx, const lt_hip_nearest_k_desc* desc, const lt_hip_point* points, uint64_t n, void* out,
                                uint64_t out_bytes) {
  return run_ray_call(ctx, desc, points, n, out, out_bytes, false, nullptr, check_nearest_k, enqueue_nearest_k);
}

extern "C" int lt_hip_nearest_k_device(lt_hip_context* ctx, const lt_hip_nearest_k_desc* desc, const lt_hip_point* points, uint64_t n, void* out,
                                       uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, points, n, out, out_bytes, true, hip_stream, check_nearest_k, enqueue_nearest_k);
}

// The same answers without a context or a GPU: lt_hip_nearest_points_host's scan of the caller's leaves in node order into the
// kernel's sinks (lt_nearest.hpp: KList, KCount), u and v from the same tri() once more for the survivors.
extern "C" int lt_hip_nearest_k_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes, const lt_hip_nearest_k_desc* desc,
                                     const lt_hip_point* points, uint64_t n, void* out, uint64_t out_bytes) {
  if (nearest_k_desc_error(desc)) return LT_ERR_INVALID_ARGUMENT;
  if (!nodes || !prims || node_bytes == 0 || node_bytes % 32 || node_bytes > 0xffffffffull * 32 || prim_bytes % 76) return LT_ERR_INVALID_ARGUMENT;
  if (n > 0xffffffffull || (n > 0 && (!points || !out))) return LT_ERR_INVALID_ARGUMENT;
  const lt_retree::Node* nd = (const lt_retree::Node*)nodes;
  const uint64_t n_nodes = node_bytes / 32, n_prims = prim_bytes / 76;
  for (uint64_t i = 0; i < n_nodes; i++)
    if (nd[i].cnt != 0 && (nd[i].off < 0 || (uint64_t)nd[i].off >= n_prims)) return LT_ERR_BAD_SCENE;
  const uint32_t maxK = desc->max_k;
  if (out_bytes < n * (maxK ? (uint64_t)maxK * sizeof(lt_hip_hit) : sizeof(uint32_t))) return LT_ERR_BUFFER_TOO_SMALL;
  const float* pr = (const float*)prims;
  auto triangle = [&](float px, float py, float pz, int32_t off) {
    const float* p = pr + 19 * (size_t)off;
    return lt_nearest::tri(px, py, pz, p[0], p[1], p[2], p[3] - p[0], p[4] - p[1], p[5] - p[2], p[6] - p[0], p[7] - p[1], p[8] - p[2]);
  };
  for (uint64_t j = 0; j < n; j++) {
    const float px = points[j].p[0], py = points[j].p[1], pz = points[j].p[2];
    int entries[2 * LT_NEAREST_MAX_K];
    lt_nearest::KList<1> list{entries, maxK};
    lt_nearest::KCount count{points[j].max_d2, 0u};
    list.reset(points[j].max_d2);
    if (!lt_nearest::no_walk(px, py, pz, points[j].max_d2)) {
      for (uint64_t i = 0; i < n_nodes; i++) {
        if (nd[i].cnt == 0) continue;
        const float d2 = lt_nearest::candidate_d2(triangle(px, py, pz, nd[i].off).d2,
                                                  lt_nearest::box_d2(px, py, pz, nd[i].lo[0], nd[i].lo[1], nd[i].lo[2], nd[i].hi[0], nd[i].hi[1], nd[i].hi[2]));
        if (maxK) list.offer(d2, 0.0f, 0.0f, nd[i].off); else count.offer(d2, 0.0f, 0.0f, nd[i].off);
      }
    }
    if (!maxK) { ((uint32_t*)out)[j] = count.n; continue; }
    lt_hip_hit* rec = (lt_hip_hit*)out + j * maxK;
    for (uint32_t e = 0; e < maxK; e++) {
      const int bits = list.d2_bits(e);
      memcpy(&rec[e].t, &bits, sizeof(float));   // (max_d2's bits in an unused slot, a NaN's payload included)
      rec[e].prim = list.prim(e);
      rec[e].u = rec[e].v = 0.0f;
      if (rec[e].prim >= 0) {
        const lt_nearest::Tri t = triangle(px, py, pz, rec[e].prim);
        rec[e].u = t.u;
        rec[e].v = t.v;
      }
    }
  }
  return LT_OK;
}

// lt_hip_overlap_boxes*: the primitives each box touches -- the first K offsets, their number, or any (lt_overlap_kernel).  The
// descriptor's rules, for the context's entry points and the host form alike; null when it passes.  The work counters are the ray
// queries': the call takes its turn behind them (ctx->query_ev).
static const char* overlap_desc_error(const lt_hip_overlap_desc* d) {
  if (!d) return "lt_hip_overlap_boxes: desc is NULL";
  if (d->struct_size < sizeof(lt_hip_overlap_desc)) return "bad lt_hip_overlap_desc (struct_size)";
  if (d->flags != 0) return "lt_hip_overlap_boxes takes no flags";
  if (d->kind != LT_OVERLAP_FIRST_K && d->kind != LT_OVERLAP_COUNT && d->kind != LT_OVERLAP_ANY) return "unknown overlap kind";
  if (d->kind == LT_OVERLAP_FIRST_K && (d->max_k < 1 || d->max_k > LT_OVERLAP_MAX_K)) return "LT_OVERLAP_FIRST_K takes max_k in 1 .. LT_OVERLAP_MAX_K";
  if (d->kind != LT_OVERLAP_FIRST_K && d->max_k != 0) return "LT_OVERLAP_COUNT and LT_OVERLAP_ANY take max_k = 0";
  return nullptr;
}

struct OverlapCall : RayCall {
  uint32_t kind, maxK;
};

static int check_overlap(lt_hip_context* ctx, const lt_hip_overlap_desc* d, const lt_hip_box* boxes, uint64_t n, const void* out, uint64_t out_bytes,
                         bool device, OverlapCall& call) {
  if (const char* why = overlap_desc_error(d)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, why);
  call.devlibm = 2;
  call.kind = (uint32_t)d->kind;
  call.maxK = d->max_k;
  call.outRecord = d->kind == LT_OVERLAP_FIRST_K ? (uint64_t)d->max_k * sizeof(int32_t) : sizeof(uint32_t);
  return check_ray_buffers(ctx, kOverlapWording, boxes, n, out, out_bytes, device, call);
}

static int enqueue_overlap(lt_hip_context* ctx, const OverlapCall& call, const void* boxes, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_query_ctl));
  lt_overlap::Params qp{};
  qp.boxes = (const float4*)boxes;
  qp.out = (uint32_t*)out;
  qp.n = (uint32_t)n;
  qp.kind = call.kind;
  qp.maxK = call.maxK;
  qp.next = ctx->d_query_ctl;
  qp.refill = k.trace_refill;
  const SceneDev sc = scene_dev(ctx, k, call.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->query_ev, s)) return rc;
  LT_HIP_CHECK(ctx, lt_overlap::launch(sc, qp, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, ctx->query_ev, s, 1, n, 0);
}

extern "C" int lt_hip_overlap_boxes(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_box* boxes, uint64_t n, void* out,
                                    uint64_t out_bytes) {
  return run_ray_call(ctx, desc, boxes, n, out, out_bytes, false, nullptr, check_overlap, enqueue_overlap);
}

extern "C" int lt_hip_overlap_boxes_device(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_box* boxes, uint64_t n, void* out,
                                           uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, boxes, n, out, out_bytes, true, hip_stream, check_overlap, enqueue_overlap);
}

// The scan behind the host forms: f(offset) for every leaf of the caller's array that touches the box, in node order, until f
// returns false.
template <class F>
static void for_touching_box(const lt_retree::Node* nd, uint64_t n_nodes, const float* pr, const lt_hip_box& box, F&& f) {
  const float* lo = box.lo;
  const float* hi = box.hi;
  if (lt_overlap::empty_box(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])) return;
  for (uint64_t i = 0; i < n_nodes; i++) {
    if (nd[i].cnt == 0) continue;
    if (!lt_overlap::boxes_meet(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], nd[i].lo[0], nd[i].lo[1], nd[i].lo[2], nd[i].hi[0], nd[i].hi[1], nd[i].hi[2]))
      continue;
    const float* p = pr + 19 * (size_t)nd[i].off;
    const float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    if (!lt_overlap::tri_meets_box(lo, hi, p, e1, e2)) continue;
    if (!f(nd[i].off)) return;
  }
}

// The same answers without a context or a GPU: lt_hip_nearest_k_host's scan of the caller's leaves in node order over
// lt_overlap.hpp's boxes_meet, tri_meets_box and KList.
extern "C" int lt_hip_overlap_boxes_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes, const lt_hip_overlap_desc* desc,
                                         const lt_hip_box* boxes, uint64_t n, void* out, uint64_t out_bytes) {
  if (overlap_desc_error(desc)) return LT_ERR_INVALID_ARGUMENT;
  if (!nodes || !prims || node_bytes == 0 || node_bytes % 32 || node_bytes > 0xffffffffull * 32 || prim_bytes % 76) return LT_ERR_INVALID_ARGUMENT;
  if (n > 0xffffffffull || (n > 0 && (!boxes || !out))) return LT_ERR_INVALID_ARGUMENT;
  const lt_retree::Node* nd = (const lt_retree::Node*)nodes;
  const uint64_t n_nodes = node_bytes / 32, n_prims = prim_bytes / 76;
  for (uint64_t i = 0; i < n_nodes; i++)
    if (nd[i].cnt != 0 && (nd[i].off < 0 || (uint64_t)nd[i].off >= n_prims)) return LT_ERR_BAD_SCENE;
  const uint32_t maxK = desc->max_k;
  if (out_bytes < n * (maxK ? (uint64_t)maxK * sizeof(int32_t) : sizeof(uint32_t))) return LT_ERR_BUFFER_TOO_SMALL;
  for (uint64_t j = 0; j < n; j++) {
    int entries[LT_OVERLAP_MAX_K];
    lt_overlap::KList<1> list{entries, maxK};
    list.reset();
    uint32_t count = 0;
    for_touching_box(nd, n_nodes, (const float*)prims, boxes[j], [&](int32_t off) {
      count++;
      if (maxK) list.offer(off);
      return maxK != 0 || desc->kind != LT_OVERLAP_ANY;
    });
    if (maxK) for (uint32_t e = 0; e < maxK; e++) ((int32_t*)out)[j * maxK + e] = list.at(e);
    else ((uint32_t*)out)[j] = desc->kind == LT_OVERLAP_ANY ? (count != 0 ? 1u : 0u) : count;
  }
  return LT_OK;
}

// lt_hip_overlap_tris*: the primitives each query triangle meets (lt_overlap_tris_kernel).  The descriptor, its rules and their
// order are lt_hip_overlap_boxes', word for word; the records are 48 bytes, so sizes are (size_t)idx * 48.
static int check_overlap_tris(lt_hip_context* ctx, const lt_hip_overlap_desc* d, const lt_hip_tri* tris, uint64_t n, const void* out, uint64_t out_bytes,
                              bool device, OverlapCall& call) {
  if (const char* why = overlap_desc_error(d)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, why);
  call.devlibm = 2;
  call.kind = (uint32_t)d->kind;
  call.maxK = d->max_k;
  call.outRecord = d->kind == LT_OVERLAP_FIRST_K ? (uint64_t)d->max_k * sizeof(int32_t) : sizeof(uint32_t);
  return check_ray_buffers(ctx, kOverlapTrisWording, tris, n, out, out_bytes, device, call);
}

static int enqueue_overlap_tris(lt_hip_context* ctx, const OverlapCall& call, const void* tris, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_query_ctl));
  lt_overlap::Params qp{};
  qp.boxes = (const float4*)tris;   // three float4 per record
  qp.out = (uint32_t*)out;
  qp.n = (uint32_t)n;
  qp.kind = call.kind;
  qp.maxK = call.maxK;
  qp.next = ctx->d_query_ctl;
  qp.refill = k.trace_refill;
  const SceneDev sc = scene_dev(ctx, k, call.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->query_ev, s)) return rc;
  LT_HIP_CHECK(ctx, lt_tritri::launch(sc, qp, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, ctx->query_ev, s, 1, n, 0);
}

extern "C" int lt_hip_overlap_tris(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_tri* tris, uint64_t n, void* out,
                                   uint64_t out_bytes) {
  return run_ray_call(ctx, desc, tris, n, out, out_bytes, false, nullptr, check_overlap_tris, enqueue_overlap_tris);
}

extern "C" int lt_hip_overlap_tris_device(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_tri* tris, uint64_t n, void* out,
                                          uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, tris, n, out, out_bytes, true, hip_stream, check_overlap_tris, enqueue_overlap_tris);
}

// lt_hip_overlap_tris_host's scan, as for_touching_box: f(offset) for every leaf that touches the query triangle, in node order.
template <class F>
static void for_touching_tri(const lt_retree::Node* nd, uint64_t n_nodes, const float* pr, const lt_hip_tri& tri, F&& f) {
  using lt_tritri::Vec;
  const Vec P{tri.a[0], tri.a[1], tri.a[2]}, Q{tri.b[0], tri.b[1], tri.b[2]}, R{tri.c[0], tri.c[1], tri.c[2]};
  if (lt_tritri::empty_tri(P, Q, R)) return;
  float lo[3], hi[3];
  lt_tritri::query_box(P, Q, R, lo, hi);
  lt_tritri::Table table;
  lt_tritri::put_query(table, P, Q, R);
  for (uint64_t i = 0; i < n_nodes; i++) {
    if (nd[i].cnt == 0) continue;
    if (!lt_overlap::boxes_meet(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], nd[i].lo[0], nd[i].lo[1], nd[i].lo[2], nd[i].hi[0], nd[i].hi[1], nd[i].hi[2]))
      continue;
    const float* p = pr + 19 * (size_t)nd[i].off;
    const Vec A{p[0], p[1], p[2]}, e1{p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2{p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    if (!lt_tritri::tri_meets_tri(table, A, e1, e2)) continue;
    if (!f(nd[i].off)) return;
  }
}

// The same answers without a context or a GPU: lt_hip_overlap_boxes_host's scan of the caller's leaves in node order over
// lt_tritri.hpp's query_box and tri_meets_tri and lt_overlap.hpp's boxes_meet and KList.
extern "C" int lt_hip_overlap_tris_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes, const lt_hip_overlap_desc* desc,
                                        const lt_hip_tri* tris, uint64_t n, void* out, uint64_t out_bytes) {
  if (overlap_desc_error(desc)) return LT_ERR_INVALID_ARGUMENT;
  if (!nodes || !prims || node_bytes == 0 || node_bytes % 32 || node_bytes > 0xffffffffull * 32 || prim_bytes % 76) return LT_ERR_INVALID_ARGUMENT;
  if (n > 0xffffffffull || (n > 0 && (!tris || !out))) return LT_ERR_INVALID_ARGUMENT;
  const lt_retree::Node* nd = (const lt_retree::Node*)nodes;
  const uint64_t n_nodes = node_bytes / 32, n_prims = prim_bytes / 76;
  for (uint64_t i = 0; i < n_nodes; i++)
    if (nd[i].cnt != 0 && (nd[i].off < 0 || (uint64_t)nd[i].off >= n_prims)) return LT_ERR_BAD_SCENE;
  const uint32_t maxK = desc->max_k;
  if (out_bytes < n * (maxK ? (uint64_t)maxK * sizeof(int32_t) : sizeof(uint32_t))) return LT_ERR_BUFFER_TOO_SMALL;
  for (uint64_t j = 0; j < n; j++) {
    int entries[LT_OVERLAP_MAX_K];
    lt_overlap::KList<1> list{entries, maxK};
    list.reset();
    uint32_t count = 0;
    for_touching_tri(nd, n_nodes, (const float*)prims, tris[j], [&](int32_t off) {
      count++;
      if (maxK) list.offer(off);
      return maxK != 0 || desc->kind != LT_OVERLAP_ANY;
    });
    if (maxK) for (uint32_t e = 0; e < maxK; e++) ((int32_t*)out)[j * maxK + e] = list.at(e);
    else ((uint32_t*)out)[j] = desc->kind == LT_OVERLAP_ANY ? (count != 0 ? 1u : 0u) : count;
  }
  return LT_OK;
}

// ---------------------------------------------------------------------------------- lists
// lt_hip_overlap_boxes_list*, lt_hip_overlap_tris_list*, lt_hip_nearest_list* and lt_hip_trace_hits_list*: the whole sequence of every query as CSR
// (lt_overlist.hpp) -- the family's walk with its kCountWide into offsets, the scan, the walk again with its kList into items, the
// ordering.  A sibling of run_ray_call: the results are two buffers and the second one's size is known only after the scan, so
// the host form runs in two halves with a look at offsets[n] between them.  The work counters are the ray queries'
// (ctx->query_ev).  What the four families share is written once -- the buffers' rules, the course, the staging; a family is a
// ListFamily -- its nouns, the bytes of an item and its two walks -- and the check of its descriptor, which leaves a ListCall.
static_assert(sizeof(lt_hip_overlap_list_desc) == 8, "overlap-list descriptor (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_nearest_list_desc) == 8 && LT_NEAREST_LIST_FLAG_FILL_ONLY == LT_OVERLAP_LIST_FLAG_FILL_ONLY,
              "radius-list descriptor (include/lenstrace_hip.h)");
static_assert(sizeof(lt_hip_hits_list_desc) == 16 &&
                  (LT_TRACE_LIST_FLAG_FILL_ONLY & (LT_RENDER_FLAG_STRICT_MATH | LT_RENDER_FLAG_PORTABLE_MATH | LT_TRACE_FLAG_COHERENT)) == 0,
              "hit-list descriptor (include/lenstrace_hip.h)");
constexpr uint32_t kListFillOnly = LT_OVERLAP_LIST_FLAG_FILL_ONLY;

// What the check of a family's descriptor leaves for the course and the launches: FILL_ONLY, and -- the hit lists -- the math
// flavour (SceneDev's) and the triangle epsilon.  The overlap and radius lists have neither choice.
struct ListCall {
  bool fillOnly = false;
  int devlibm = 2;
  lt_query::Epsilon eps = lt_query::kEpsDouble4;
};

// One walk of a list call over device memory: the count into `offsets` (fill == false), or the fill of `items` and its ordering.
struct ListPass {
  const void* records;
  uint32_t n;
  uint32_t* next;
  uint32_t refill;
  bool fill, oneShot;
  unsigned long long* offsets;
  void* items;
  unsigned long long capacity;   // items
  lt_query::Epsilon eps;         // the hit lists' triangle epsilon
};
using ListWalk = hipError_t (*)(const SceneDev&, const ListPass&, uint32_t, hipStream_t);

struct ListFamily {
  const char *lists, *desc, *fillOnly;   // the nouns of the error texts: "overlap lists", the descriptor's and the flag's name
  const char* call;                      // the entry point
  const char* in;                        // the input pointer
  const char* items;                     // what items holds: "words", "records"
  uint64_t itemBytes;
  ListWalk walk;
  bool rankOrder = false;                // the ordering is a launch only in a scene with an own tree (lt_overlist::order_ray_hits)
};

using OverlapLaunch = hipError_t (*)(const SceneDev&, const lt_overlap::Params&, uint32_t, hipStream_t);
template <OverlapLaunch LAUNCH>
static hipError_t overlap_list_walk(const SceneDev& sc, const ListPass& p, uint32_t cuCount, hipStream_t s) {
  lt_overlap::Params qp{};
  qp.boxes = (const float4*)p.records;
  qp.n = p.n;
  qp.next = p.next;
  qp.refill = p.refill;
  if (!p.fill) {
    qp.kind = lt_overlap::kCountWide;
    qp.out = (uint32_t*)p.offsets;
    return LAUNCH(sc, qp, cuCount, s);
  }
  qp.kind = lt_overlap::kList;
  qp.offsets = p.offsets;
  qp.items = (int32_t*)p.items;
  qp.capacity = p.capacity;
  qp.oneShot = p.oneShot ? 1u : 0u;
  const hipError_t e = LAUNCH(sc, qp, cuCount, s);
  return e != hipSuccess ? e : lt_overlist::order(p.offsets, p.n, qp.items, p.capacity, p.oneShot, cuCount, s);
}

static hipError_t nearest_list_walk(const SceneDev& sc, const ListPass& p, uint32_t cuCount, hipStream_t s) {
  lt_nearest::KParams qp{};
  qp.points = (const float4*)p.records;
  qp.n = p.n;
  qp.next = p.next;
  qp.refill = p.refill;
  qp.offsets = p.offsets;
  if (!p.fill) {
    qp.kind = lt_nearest::kCountWide;
    return lt_nearest::launch_k(sc, qp, cuCount, s);
  }
  qp.kind = lt_nearest::kList;
  qp.items = (uint4*)p.items;
  qp.capacity = p.capacity;
  qp.oneShot = p.oneShot ? 1u : 0u;
  const hipError_t e = lt_nearest::launch_k(sc, qp, cuCount, s);
  return e != hipSuccess ? e : lt_overlist::order_hits(p.offsets, p.n, qp.items, p.capacity, p.oneShot, cuCount, s);
}

static hipError_t hits_list_walk(const SceneDev& sc, const ListPass& p, uint32_t cuCount, hipStream_t s) {
  lt_query::HitsParams qp{};
  qp.rays = (const float4*)p.records;
  qp.n = p.n;
  qp.next = p.next;
  qp.refill = p.refill;
  qp.offsets = p.offsets;
  if (!p.fill) {
    qp.kind = lt_query::kCountWide;
    return lt_query::launch_hits(sc, qp, p.eps, cuCount, s);
  }
  qp.kind = lt_query::kList;
  qp.items = (uint4*)p.items;
  qp.capacity = p.capacity;
  qp.oneShot = p.oneShot ? 1u : 0u;
  const hipError_t e = lt_query::launch_hits(sc, qp, p.eps, cuCount, s);
  return e != hipSuccess ? e : lt_overlist::order_ray_hits(p.offsets, p.n, qp.items, p.capacity, p.oneShot, qp.rays, sc.rank8, sc.n_prims, cuCount, s);
}

constexpr ListFamily kOverlapBoxesList{"overlap lists", "lt_hip_overlap_list_desc", "LT_OVERLAP_LIST_FLAG_FILL_ONLY", "lt_hip_overlap_boxes_list",
                                       "boxes", "words", sizeof(int32_t), overlap_list_walk<lt_overlap::launch>};
constexpr ListFamily kOverlapTrisList{"overlap lists", "lt_hip_overlap_list_desc", "LT_OVERLAP_LIST_FLAG_FILL_ONLY", "lt_hip_overlap_tris_list",
                                      "tris", "words", sizeof(int32_t), overlap_list_walk<lt_tritri::launch>};
constexpr ListFamily kNearestList{"radius lists", "lt_hip_nearest_list_desc", "LT_NEAREST_LIST_FLAG_FILL_ONLY", "lt_hip_nearest_list",
                                  "points", "records", sizeof(lt_hip_hit), nearest_list_walk};
constexpr ListFamily kHitsList{"hit lists", "lt_hip_hits_list_desc", "LT_TRACE_LIST_FLAG_FILL_ONLY", "lt_hip_trace_hits_list",
                               "rays", "records", sizeof(lt_hip_hit), hits_list_walk, true};

// The descriptor's rules -- the two descriptors are the same two words --; empty when it passes.
template <class Desc>
static std::string list_desc_error(const ListFamily& f, const Desc* d) {
  if (!d) return std::string(f.lists) + ": desc is NULL";
  if (d->struct_size < sizeof(Desc)) return std::string("bad ") + f.desc + " (struct_size)";
  if (d->flags & ~kListFillOnly) return std::string(f.lists) + " take " + f.fillOnly + " only";
  return std::string();
}

// The check of the overlap and radius lists' descriptors.
template <class Desc>
static int check_list_desc(lt_hip_context* ctx, const ListFamily& f, const Desc* d, ListCall& lc) {
  const std::string why = list_desc_error(f, d);
  if (!why.empty()) return fail(ctx, LT_ERR_INVALID_ARGUMENT, why);
  lc.fillOnly = (d->flags & kListFillOnly) != 0;
  return LT_OK;
}

// ... and of the hit lists': the program and the flags by lt_hip_trace_hits' rules (check_hits), FILL_ONLY beside them.
static int check_hits_list_desc(lt_hip_context* ctx, const ListFamily& f, const lt_hip_hits_list_desc* d, ListCall& lc) {
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string(f.lists) + ": desc is NULL");
  if (d->struct_size < sizeof(lt_hip_hits_list_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string("bad ") + f.desc + " (struct_size)");
  if (const int rc = query_epsilon(ctx, d->program, lc.eps)) return rc;
  RayCall rc{};
  if (d->flags & ~(LT_RENDER_FLAG_STRICT_MATH | LT_RENDER_FLAG_PORTABLE_MATH | LT_TRACE_FLAG_COHERENT | LT_TRACE_LIST_FLAG_FILL_ONLY))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT,
                std::string(f.lists) + " take LT_RENDER_FLAG_STRICT_MATH, LT_RENDER_FLAG_PORTABLE_MATH, LT_TRACE_FLAG_COHERENT and " + f.fillOnly + " only");
  if (const int e = check_ray_flags(ctx, d->flags & ~LT_TRACE_LIST_FLAG_FILL_ONLY, true, "hit lists take", rc)) return e;
  if (d->reserved != 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string(f.desc) + "::reserved must be 0");
  lc.devlibm = rc.devlibm;
  lc.fillOnly = (d->flags & LT_TRACE_LIST_FLAG_FILL_ONLY) != 0;
  return LT_OK;
}

// The rules about the records and the two buffers that the context's entry points and the host forms share, in their order.
static std::string list_buffers_error(const ListFamily& f, uint32_t flags, const void* in, uint64_t n, const void* offsets, const void* items,
                                      uint64_t items_bytes) {
  if (n > 0xffffffffull) return "at most 2^32 - 1 queries per call";
  if (n > 0 && (!in || !offsets)) return "the records or offsets are NULL";
  if (!items && items_bytes != 0) return "items is NULL and items_bytes is not 0";
  if ((flags & kListFillOnly) && !items) return std::string(f.fillOnly) + " takes items";
  return std::string();
}

// One half of a call, or both, on `s`, over device memory: `sized` runs the count and the scan, `fill` the fill and the ordering
// over `capacity` items (`oneShot`: behind this stream's own scan, and nothing is written when its total is larger).
static int enqueue_list(lt_hip_context* ctx, const ListFamily& f, const ListCall& lc, const void* records, uint64_t n, uint64_t* offsets, void* items,
                        uint64_t capacity, bool sized, bool fill, bool oneShot, hipStream_t s) {
  const RenderKnobs k;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_query_ctl));
  if (sized) {
    const uint64_t words = lt_overlist::scan_partials(n);
    LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_list_partials, ctx->list_partials_words, words, words * sizeof(uint64_t)));
  }
  ListPass p{records, (uint32_t)n, ctx->d_query_ctl, k.trace_refill, false, oneShot, (unsigned long long*)offsets, items, capacity, lc.eps};
  const SceneDev sc = scene_dev(ctx, k, lc.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->query_ev, s)) return rc;
  uint32_t launches = 0;
  if (sized) {
    LT_HIP_CHECK(ctx, f.walk(sc, p, (uint32_t)ctx->cu_count, s));
    LT_HIP_CHECK(ctx, lt_overlist::scan(p.offsets, p.n, ctx->d_list_partials, s));
    launches += 1 + lt_overlist::kScanLaunches;
  }
  if (fill) {
    p.fill = true;
    LT_HIP_CHECK(ctx, f.walk(sc, p, (uint32_t)ctx->cu_count, s));
    launches += 1 + (f.rankOrder && sc.rank8 == nullptr ? 0u : lt_overlist::kOrderLaunches);
  }
  return end_ray_launches(ctx, ctx->query_ev, s, launches, n, 0);
}

template <class Desc, class Record>
static int run_list_call(lt_hip_context* ctx, const ListFamily& f, const Desc* desc, const Record* in, uint64_t n, uint64_t* offsets,
                         uint64_t offsets_bytes, void* items, uint64_t items_bytes, bool device, void* hip_stream,
                         int (*check)(lt_hip_context*, const ListFamily&, const Desc*, ListCall&) = check_list_desc<Desc>) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  ListCall lc{};
  if (const int rc = check(ctx, f, desc, lc)) return rc;
  {
    const std::string why = list_buffers_error(f, lc.fillOnly ? kListFillOnly : 0u, in, n, offsets, items, items_bytes);
    if (!why.empty()) return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string(f.call) + ": " + why);
  }
  if (device && n > 0 && (((uintptr_t)in | (uintptr_t)offsets | (uintptr_t)items) & 15u))
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, std::string("device ") + f.in + ", offsets and items must be 16-byte aligned");
  if (!ctx->has_scene) return fail(ctx, LT_ERR_NO_SCENE, std::string(f.call) + " before lt_hip_set_scene");
  if (offsets_bytes < (n + 1) * sizeof(uint64_t)) return fail(ctx, LT_ERR_BUFFER_TOO_SMALL, "offsets is smaller than n + 1 words");
  const bool fillOnly = lc.fillOnly;
  const uint64_t capacity = items_bytes / f.itemBytes;
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n == 0) {
    if (fillOnly || !offsets) return LT_OK;
    if (device) LT_HIP_CHECK(ctx, hipMemsetAsync(offsets, 0, sizeof(uint64_t), (hipStream_t)hip_stream));
    else offsets[0] = 0;
    return LT_OK;
  }
  if (device) return enqueue_list(ctx, f, lc, in, n, offsets, items, capacity, !fillOnly, items != nullptr, !fillOnly, (hipStream_t)hip_stream);
  // The host form: the records and the offsets in the two staging buffers of the ray families, the items in a buffer of their own
  // -- growing a buffer frees what it held, and the offsets have to outlive the growth of the items.
  const uint64_t inBytes = n * sizeof(Record), offBytes = (n + 1) * sizeof(uint64_t);
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_query_rays, ctx->query_rays_bytes, inBytes, inBytes));
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_query_out, ctx->query_out_bytes, offBytes, offBytes));
  uint64_t* const dOffsets = (uint64_t*)ctx->d_query_out;
  LT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_query_rays, in, inBytes, hipMemcpyHostToDevice, ctx->stream));
  uint64_t total = 0;
  float sizedMs = 0.0f;
  uint32_t sizedLaunches = 0;
  if (fillOnly) {
    LT_HIP_CHECK(ctx, hipMemcpyAsync(dOffsets, offsets, offBytes, hipMemcpyHostToDevice, ctx->stream));
    total = offsets[n] < capacity ? offsets[n] : capacity;   // the items that can be written at all
  } else {
    if (const int rc = enqueue_list(ctx, f, lc, ctx->d_query_rays, n, dOffsets, nullptr, 0, true, false, false, ctx->stream)) return rc;
    LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (const int rc = finish_pending(ctx)) return rc;
    sizedMs = ctx->last.kernel_ms;
    sizedLaunches = ctx->last.kernel_launches;
    LT_HIP_CHECK(ctx, hipMemcpy(offsets, dOffsets, offBytes, hipMemcpyDeviceToHost));
    total = offsets[n];
    if (!items) return LT_OK;
    if (capacity < total) return fail(ctx, LT_ERR_BUFFER_TOO_SMALL, std::string("items is smaller than offsets[n] ") + f.items + " (offsets is written)");
  }
  if (total == 0) return LT_OK;
  const uint64_t itemBytes = total * f.itemBytes;
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_list_items, ctx->list_items_bytes, itemBytes, itemBytes));
  if (const int rc = enqueue_list(ctx, f, lc, ctx->d_query_rays, n, dOffsets, ctx->d_list_items, total, false, true, false, ctx->stream)) return rc;
  LT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (const int rc = finish_pending(ctx)) return rc;
  ctx->last.kernel_ms += sizedMs;
  ctx->last.kernel_launches += sizedLaunches;
  LT_HIP_CHECK(ctx, hipMemcpy(items, ctx->d_list_items, itemBytes, hipMemcpyDeviceToHost));
  return LT_OK;
}

extern "C" int lt_hip_overlap_boxes_list(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_box* boxes, uint64_t n,
                                         uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes) {
  return run_list_call(ctx, kOverlapBoxesList, desc, boxes, n, offsets, offsets_bytes, items, items_bytes, false, nullptr);
}

extern "C" int lt_hip_overlap_boxes_list_device(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_box* boxes, uint64_t n,
                                                uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes, void* hip_stream) {
  return run_list_call(ctx, kOverlapBoxesList, desc, boxes, n, offsets, offsets_bytes, items, items_bytes, true, hip_stream);
}

extern "C" int lt_hip_overlap_tris_list(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_tri* tris, uint64_t n,
                                        uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes) {
  return run_list_call(ctx, kOverlapTrisList, desc, tris, n, offsets, offsets_bytes, items, items_bytes, false, nullptr);
}

extern "C" int lt_hip_overlap_tris_list_device(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_tri* tris, uint64_t n,
                                               uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes, void* hip_stream) {
  return run_list_call(ctx, kOverlapTrisList, desc, tris, n, offsets, offsets_bytes, items, items_bytes, true, hip_stream);
}

extern "C" int lt_hip_nearest_list(lt_hip_context* ctx, const lt_hip_nearest_list_desc* desc, const lt_hip_point* points, uint64_t n,
                                   uint64_t* offsets, uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes) {
  return run_list_call(ctx, kNearestList, desc, points, n, offsets, offsets_bytes, items, items_bytes, false, nullptr);
}

extern "C" int lt_hip_nearest_list_device(lt_hip_context* ctx, const lt_hip_nearest_list_desc* desc, const lt_hip_point* points, uint64_t n,
                                          uint64_t* offsets, uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes, void* hip_stream) {
  return run_list_call(ctx, kNearestList, desc, points, n, offsets, offsets_bytes, items, items_bytes, true, hip_stream);
}

extern "C" int lt_hip_trace_hits_list(lt_hip_context* ctx, const lt_hip_hits_list_desc* desc, const lt_hip_ray* rays, uint64_t n, uint64_t* offsets,
                                      uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes) {
  return run_list_call(ctx, kHitsList, desc, rays, n, offsets, offsets_bytes, items, items_bytes, false, nullptr, check_hits_list_desc);
}

extern "C" int lt_hip_trace_hits_list_device(lt_hip_context* ctx, const lt_hip_hits_list_desc* desc, const lt_hip_ray* rays, uint64_t n,
                                             uint64_t* offsets, uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes, void* hip_stream) {
  return run_list_call(ctx, kHitsList, desc, rays, n, offsets, offsets_bytes, items, items_bytes, true, hip_stream, check_hits_list_desc);
}

// The same lists without a context or a GPU.  `sequence(nd, n_nodes, prims, record, seq)` fills `seq` with the whole sequence of
// one query, in order: the host forms' scan of the caller's leaves in node order, then a sort.  LT_ERR_BAD_SCENE stands where the
// context's entry points have LT_ERR_NO_SCENE.
template <class Item, class Desc, class Record, class Sequence>
static int list_host(const ListFamily& f, const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes, const Desc* desc,
                     const Record* in, uint64_t n, uint64_t* offsets, uint64_t offsets_bytes, Item* items, uint64_t items_bytes, Sequence sequence) {
  if (!list_desc_error(f, desc).empty()) return LT_ERR_INVALID_ARGUMENT;
  if (!nodes || !prims || node_bytes == 0 || node_bytes % 32 || node_bytes > 0xffffffffull * 32 || prim_bytes % 76) return LT_ERR_INVALID_ARGUMENT;
  if (!list_buffers_error(f, desc->flags, in, n, offsets, items, items_bytes).empty()) return LT_ERR_INVALID_ARGUMENT;
  const lt_retree::Node* nd = (const lt_retree::Node*)nodes;
  const uint64_t n_nodes = node_bytes / 32, n_prims = prim_bytes / 76;
  for (uint64_t i = 0; i < n_nodes; i++)
    if (nd[i].cnt != 0 && (nd[i].off < 0 || (uint64_t)nd[i].off >= n_prims)) return LT_ERR_BAD_SCENE;
  if (offsets_bytes < (n + 1) * sizeof(uint64_t)) return LT_ERR_BUFFER_TOO_SMALL;
  const bool fillOnly = (desc->flags & kListFillOnly) != 0;
  const uint64_t capacity = items_bytes / sizeof(Item);
  std::vector<Item> seq, all;
  if (fillOnly) {   // query j's items go to [offsets[j], min(offsets[j + 1], capacity)), whatever the offsets hold
    for (uint64_t j = 0; j < n; j++) {
      const uint64_t begin = offsets[j], end = offsets[j + 1] < capacity ? offsets[j + 1] : capacity;
      if (end <= begin) continue;
      seq.clear();
      sequence(nd, n_nodes, (const float*)prims, in[j], seq);
      const uint64_t room = end - begin;
      std::copy(seq.begin(), seq.begin() + (size_t)(room < seq.size() ? room : seq.size()), items + begin);
    }
    return LT_OK;
  }
  if (n == 0) {
    if (offsets) offsets[0] = 0;
    return LT_OK;
  }
  uint64_t total = 0;
  for (uint64_t j = 0; j < n; j++) {
    seq.clear();
    sequence(nd, n_nodes, (const float*)prims, in[j], seq);
    offsets[j] = total;
    total += seq.size();
    if (items && total <= capacity) all.insert(all.end(), seq.begin(), seq.end());
  }
  offsets[n] = total;
  if (!items) return LT_OK;
  if (capacity < total) return LT_ERR_BUFFER_TOO_SMALL;
  std::copy(all.begin(), all.end(), items);
  return LT_OK;
}

extern "C" int lt_hip_overlap_boxes_list_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                                              const lt_hip_overlap_list_desc* desc, const lt_hip_box* boxes, uint64_t n, uint64_t* offsets,
                                              uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes) {
  return list_host(kOverlapBoxesList, nodes, node_bytes, prims, prim_bytes, desc, boxes, n, offsets, offsets_bytes, items, items_bytes,
                   [](const lt_retree::Node* nd, uint64_t n_nodes, const float* pr, const lt_hip_box& q, std::vector<int32_t>& seq) {
                     for_touching_box(nd, n_nodes, pr, q, [&](int32_t off) { seq.push_back(off); return true; });
                     std::sort(seq.begin(), seq.end());
                   });
}

extern "C" int lt_hip_overlap_tris_list_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                                             const lt_hip_overlap_list_desc* desc, const lt_hip_tri* tris, uint64_t n, uint64_t* offsets,
                                             uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes) {
  return list_host(kOverlapTrisList, nodes, node_bytes, prims, prim_bytes, desc, tris, n, offsets, offsets_bytes, items, items_bytes,
                   [](const lt_retree::Node* nd, uint64_t n_nodes, const float* pr, const lt_hip_tri& q, std::vector<int32_t>& seq) {
                     for_touching_tri(nd, n_nodes, pr, q, [&](int32_t off) { seq.push_back(off); return true; });
                     std::sort(seq.begin(), seq.end());
                   });
}

// lt_hip_nearest_k_host's scan with every accepted candidate kept, then a STABLE sort by lt_nearest::record_before: node order is
// the third key.
extern "C" int lt_hip_nearest_list_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                                        const lt_hip_nearest_list_desc* desc, const lt_hip_point* points, uint64_t n, uint64_t* offsets,
                                        uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes) {
  static_assert(sizeof(lt_nearest::Record) == sizeof(lt_hip_hit), "a radius list's record is lt_hip_hit");
  return list_host(kNearestList, nodes, node_bytes, prims, prim_bytes, desc, points, n, offsets, offsets_bytes, (lt_nearest::Record*)items, items_bytes,
                   [](const lt_retree::Node* nd, uint64_t n_nodes, const float* pr, const lt_hip_point& q, std::vector<lt_nearest::Record>& seq) {
                     const float px = q.p[0], py = q.p[1], pz = q.p[2];
                     if (lt_nearest::no_walk(px, py, pz, q.max_d2)) return;
                     for (uint64_t i = 0; i < n_nodes; i++) {
                       if (nd[i].cnt == 0) continue;
                       const float* p = pr + 19 * (size_t)nd[i].off;
                       const lt_nearest::Tri t = lt_nearest::tri(px, py, pz, p[0], p[1], p[2], p[3] - p[0], p[4] - p[1], p[5] - p[2], p[6] - p[0],
                                                                 p[7] - p[1], p[8] - p[2]);
                       const float d2 = lt_nearest::candidate_d2(
                           t.d2, lt_nearest::box_d2(px, py, pz, nd[i].lo[0], nd[i].lo[1], nd[i].lo[2], nd[i].hi[0], nd[i].hi[1], nd[i].hi[2]));
                       if (d2 < q.max_d2) seq.push_back(lt_nearest::Record{d2, nd[i].off, t.u, t.v});
                     }
                     std::stable_sort(seq.begin(), seq.end(), lt_nearest::record_before);
                   });
}

// lt_hip_shade_rays*: the colour a program's `shade` returns for caller-supplied rays (lt_shade.hip).
struct ShadeCall : RayCall {
  int program;         // lt::Program
  const lt_hip_shade_desc* desc;
};

static int check_shade(lt_hip_context* ctx, const lt_hip_shade_desc* d, const lt_hip_shade_ray* rays, uint64_t n, const void* out, uint64_t out_bytes,
                       bool device, ShadeCall& sc) {
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_shade_rays: desc is NULL");
  if (d->struct_size < sizeof(lt_hip_shade_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "bad lt_hip_shade_desc (struct_size)");
  if (const int rc = check_shade_program(ctx, d->program, "lt_hip_shade_rays does not take user programs")) return rc;
  if (d->program == LT_PROGRAM_GLOBAL_ILLUMINATION || d->program == LT_PROGRAM_GLOBAL_ILLUMINATION_25)
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_shade_rays does not take the global-illumination programs (their pipeline is indexed by pixel)");
  if (d->kernel_mode != LT_KERNEL_MODE_LINEAR && d->kernel_mode != LT_KERNEL_MODE_TILE) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "unknown kernel mode");
  if (const int rc = check_ray_flags(ctx, d->flags, true, "shaded rays take", sc)) return rc;
  if (d->frame_count == 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_shade_desc::frame_count must be at least 1");
  sc.program = d->program == LT_PROGRAM_BASIC ? kBasic : d->program == LT_PROGRAM_BASIC_LIGHTING ? kBasicLighting
               : d->program == LT_PROGRAM_ACCUMULATOR ? kAccumulator : kCustom;
  sc.desc = d;
  sc.outRecord = sizeof(lt_hip_shade);
  return check_ray_buffers(ctx, kShadeWording, rays, n, out, out_bytes, device, sc);
}

static int enqueue_shade(lt_hip_context* ctx, const ShadeCall& call, const void* rays, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  const lt_hip_shade_desc* const d = call.desc;
  LT_HIP_CHECK(ctx, ensure_ray_counters(ctx->d_shade_ctl));
  lt_shade::Params sp{};
  sp.rays = (const float4*)rays;
  sp.out = (uint4*)out;
  sp.n = (uint32_t)n;
  sp.next = ctx->d_shade_ctl;
  sp.refill = k.trace_refill;
  sp.shadeBatch = 16;   // LT_SHADE_BATCH=1..64 (A/B measurements; no result depends on it)
  if (const char* e = getenv("LT_SHADE_BATCH")) sp.shadeBatch = (uint32_t)std::max(1, std::min(64, atoi(e)));
  sp.frameFirst = d->frame_first;
  sp.frameCount = d->frame_count;
  sp.clampOutput = d->kernel_mode == LT_KERNEL_MODE_LINEAR;
  const SceneDev sc = scene_dev(ctx, k, call.devlibm);
  if (const int rc = begin_ray_launches(ctx, &ctx->shade_ev, s)) return rc;
  LT_HIP_CHECK(ctx, lt_shade::launch(sc, sp, call.program, call.devlibm, (uint32_t)ctx->cu_count, s));
  return end_ray_launches(ctx, ctx->shade_ev, s, 1, n, 0);
}

extern "C" int lt_hip_shade_rays(lt_hip_context* ctx, const lt_hip_shade_desc* desc, const lt_hip_shade_ray* rays, uint64_t n, lt_hip_shade* out,
                                 uint64_t out_bytes) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, false, nullptr, check_shade, enqueue_shade);
}

extern "C" int lt_hip_shade_rays_device(lt_hip_context* ctx, const lt_hip_shade_desc* desc, const lt_hip_shade_ray* rays, uint64_t n, lt_hip_shade* out,
                                        uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, true, hip_stream, check_shade, enqueue_shade);
}

// lt_hip_shade_paths*: the global-illumination programs over caller-supplied rays (lt_paths.hip).  check_shade's rules and order.
struct PathsCall : RayCall {
  bool gi25;
  const lt_hip_paths_desc* desc;
};

static int check_paths(lt_hip_context* ctx, const lt_hip_paths_desc* d, const lt_hip_shade_ray* rays, uint64_t n, const void* out, uint64_t out_bytes,
                       bool device, PathsCall& pc) {
  if (!d) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_shade_paths: desc is NULL");
  if (d->struct_size < sizeof(lt_hip_paths_desc)) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "bad lt_hip_paths_desc (struct_size)");
  if (const int rc = check_shade_program(ctx, d->program, "lt_hip_shade_paths does not take user programs (nor does lt_hip_shade_rays)")) return rc;
  if (d->program != LT_PROGRAM_GLOBAL_ILLUMINATION && d->program != LT_PROGRAM_GLOBAL_ILLUMINATION_25)
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_shade_paths takes the global-illumination programs only: this program's entry point is lt_hip_shade_rays");
  if (d->kernel_mode != LT_KERNEL_MODE_LINEAR && d->kernel_mode != LT_KERNEL_MODE_TILE) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "unknown kernel mode");
  if (const int rc = check_ray_flags(ctx, d->flags, true, "shaded paths take", pc)) return rc;
  if (d->frame_count == 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_paths_desc::frame_count must be at least 1");
  if (d->gi_max_depth < 0 || d->gi_max_depth > 64) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "gi_max_depth out of range");
  if (d->reserved != 0) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_paths_desc::reserved must be 0");
  pc.gi25 = d->program == LT_PROGRAM_GLOBAL_ILLUMINATION_25;
  pc.desc = d;
  pc.outRecord = sizeof(lt_hip_shade);
  return check_ray_buffers(ctx, kPathsWording, rays, n, out, out_bytes, device, pc);
}

// Path slots of one set when neither LT_PATHS_SLOTS nor LT_FUSED_BYTES says otherwise (DESIGN.md 5.11 has the timings of the
// candidates): 272 bytes of scratch each.
constexpr uint64_t kPathsSlots = 64ull << 20;

// One set of a call (lt_paths::Params) through the pipeline: lt_paths_primary_kernel, the bounce stages -- launch_gi_sample's
// launches in its three forms, over path slots instead of pixels -- and lt_paths_resolve_kernel.
template <class CFG>
static int launch_paths_set(lt_hip_context* ctx, const RenderKnobs& k, const SceneDev& sc, lt_paths::Params pp, hipStream_t s, uint32_t& launches) {
  GiParams gp{};
  for (int q = 0; q < 2; q++) {
    gp.q[q].o = (float4*)ctx->d_gi[4 * q + 0]; gp.q[q].d = (float4*)ctx->d_gi[4 * q + 1];
    gp.q[q].n = (float4*)ctx->d_gi[4 * q + 2]; gp.q[q].m = (uint4*)ctx->d_gi[4 * q + 3];
  }
  gp.direct = (float4*)ctx->d_gi[8]; gp.indirect = (float4*)ctx->d_gi[9]; gp.blend = (float4*)ctx->d_gi[10];
  auto ctl = [&](uint32_t run) { return ctx->d_giCtl + (8 + run * (kMaxStack + 2)) * kQueueStride; };
  gp.counts = ctl(0); gp.work = ctl(1); gp.hitCount = ctl(2);
  uint32_t* const traceWork = ctl(3);
  uint32_t* const shadowWork = ctl(11);
  gp.sample = pp.sample;
  gp.pixels = pp.nRays * pp.frames * pp.perFrame;   // (the slots of the set; every path's m.w is its sample's offset from gp.sample)
  FrameParams fp{};
  fp.giMaxDepth = pp.giMaxDepth;
  fp.clampOutput = pp.clampOutput;
  fp.fusedFrames = 1;
  LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_giCtl, 0, kGiCtlWords * sizeof(uint32_t), s));
  const uint32_t resident = (uint32_t)ctx->cu_count * 4u * LT_GI_STAGE_WAVES;
  // the LDS of the stage launches, as render_on_stream computes it for its non-counting launches
  const uint32_t rowBytes = (uint32_t)(kBlock * sizeof(int));
  const uint32_t ldsRefBytes = (uint32_t)std::max(kPacketRows, std::min(ctx->bvh_height, kLdsStack)) * rowBytes;
  uint32_t lds = (uint32_t)std::max(kPacketRows, kOwnRows) * rowBytes;
  if (k.debug_lds_rows) lds = std::max(lds, k.debug_lds_rows * rowBytes);
  const bool ldsScene = gi_lds_scene(ctx, k);
  const bool pretrace = !ldsScene && ctx->d_rank8 != nullptr && k.gi_trace;
  gp.directQueue = pretrace ? 1u : 0u;
  pp.qo = gp.q[0].o; pp.qd = gp.q[0].d; pp.qn = gp.q[0].n; pp.qm = gp.q[0].m;
  pp.direct = gp.direct; pp.indirect = gp.indirect;
  pp.count0 = gp.counts;
  pp.directQueue = gp.directQueue;
  LT_HIP_CHECK(ctx, lt_paths::launch_primary(sc, pp, CFG::kDevLibm, s));
  launches++;
  gp.ldsRows = ldsRefBytes / rowBytes;
  gp.hitList = (uint32_t*)ctx->d_gi[12];
  gp.so = (float4*)ctx->d_gi[13]; gp.sd = (float4*)ctx->d_gi[14]; gp.sm = (uint4*)ctx->d_gi[15]; gp.sn = (float4*)ctx->d_gi[16];
  const uint32_t traceLds = (uint32_t)((kTraceRows + kTraceStage) * kBlock * sizeof(int));
  const dim3 streamGrid((uint32_t)ctx->cu_count * 8u), streamBlock(256);
  for (int d = 0; d < fp.giMaxDepth; d++) {
    gp.hits = nullptr;
    if (pretrace) {
      TraceParams tp{};
      const GiQueue& q = gp.q[d & 1];
      tp.o = q.o; tp.d = q.d; tp.m = q.m;
      tp.hit = (uint4*)ctx->d_gi[11];
      tp.count = gp.counts + (size_t)d * kQueueStride;
      tp.next = traceWork + (size_t)d * 8 * kQueueStride;
      tp.refill = k.trace_refill;
      tp.dead = d == 0 ? 1u : 0u;
      gp.hits = tp.hit;
      hipLaunchKernelGGL((lt_trace_kernel<kGI, false>), dim3(resident), dim3(kBlock), traceLds, s, sc, tp);
      hipLaunchKernelGGL((lt_gi_classify_kernel<CFG>), streamGrid, streamBlock, 0, s, sc, fp, gp, (uint32_t)d);
      hipLaunchKernelGGL((lt_gi_shadow_kernel<CFG>), streamGrid, streamBlock, 0, s, sc, fp, gp, (uint32_t)d);
      tp.o = gp.so; tp.d = gp.sd; tp.m = gp.sm;
      tp.occluded = (uint32_t*)ctx->d_gi[11];
      gp.occluded = tp.occluded;
      tp.count = gp.hitCount + (size_t)d * kQueueStride;
      tp.next = shadowWork + (size_t)d * 8 * kQueueStride;
      tp.dead = 0u;
      hipLaunchKernelGGL((lt_trace_kernel<kGI, true>), dim3(resident), dim3(kBlock), traceLds, s, sc, tp);
      hipLaunchKernelGGL((lt_gi_finish_kernel<CFG>), streamGrid, streamBlock, 0, s, sc, fp, gp, (uint32_t)d);
      LT_HIP_CHECK(ctx, hipGetLastError());
      launches += 5;
      continue;
    }
    if (ldsScene) {
      using CFGL = Config<false, false, CFG::kDevLibm, true>;
      hipLaunchKernelGGL((lt_gi_bounce_kernel<CFGL>), dim3((resident + kLdsSceneWaves - 1) / kLdsSceneWaves), dim3(kBlock * kLdsSceneWaves),
                         (uint32_t)scene_lds_bytes(ctx) + kLdsSceneWaves * ldsRefBytes, s, sc, fp, gp, (uint32_t)d);
    } else {
      hipLaunchKernelGGL((lt_gi_bounce_kernel<CFG>), dim3(resident), dim3(kBlock), lds, s, sc, fp, gp, (uint32_t)d);
    }
    LT_HIP_CHECK(ctx, hipGetLastError());
    launches++;
  }
  LT_HIP_CHECK(ctx, lt_paths::launch_resolve(pp, CFG::kDevLibm, s));
  launches++;
  return LT_OK;
}

// Enqueues the call on `s` between the context's timing events; lt_hip_get_stats reports it (finish_pending).  The call is cut
// into SETS of at most `cap` path slots: ranges of rays with all their frames, or -- one ray's frames alone exceed the cap --
// ranges of frames as well; a frame's 25 samples stay together.  A range of rays walks its camera rays once, ahead of its sets;
// between the sets of a range the running mean waits in the caller's record (lt_paths::Params::folded).
static int enqueue_paths(lt_hip_context* ctx, const PathsCall& call, const void* rays, uint64_t n, void* out, hipStream_t s) {
  const RenderKnobs k;
  const lt_hip_paths_desc* const d = call.desc;
  const uint32_t perFrame = call.gi25 ? 25u : 1u, frames = d->frame_count;
  uint64_t cap = std::min<uint64_t>(kPathsSlots, k.fused_bytes / (17 * 16));
  if (const char* e = getenv("LT_PATHS_SLOTS")) cap = strtoull(e, nullptr, 10);   // (tests, A/B measurements; no result depends on it)
  // (lt_paths_primary_kernel runs one lane per slot, 64 to a block, the stage and resolve kernels one per ray, 256 to a block: a
  // launch holds 2^32 - 1 work-items, so a set has at most 2^32 - 256 slots)
  cap = std::min<uint64_t>(std::max<uint64_t>(cap, perFrame), 0xffffff00ull);
  const uint64_t perRay = (uint64_t)frames * perFrame;
  const uint32_t framesPerSet = perRay <= cap ? frames : (uint32_t)(cap / perFrame);
  const uint64_t raysAtMost = std::min<uint64_t>(n, std::max<uint64_t>(1, cap / ((uint64_t)framesPerSet * perFrame)));
  const uint64_t ranges = (n + raysAtMost - 1) / raysAtMost;
  const uint32_t raysPerSet = (uint32_t)((n + ranges - 1) / ranges);   // (ranges of equal size: a short last one costs its launches all the same)
  if (const int rc = ensure_gi_buffers(ctx, (uint64_t)raysPerSet * framesPerSet * perFrame)) return rc;
  LT_HIP_CHECK(ctx, grow_scratch(ctx, ctx->d_paths_hits, ctx->paths_hits_rays, (uint64_t)raysPerSet, (uint64_t)raysPerSet * sizeof(uint4)));
  SceneDev sc = scene_dev(ctx, k, call.devlibm);
  sc.shadowPackets = 0u;   // (every shadow ray of these launches walks per lane)
  lt_paths::Params pp{};
  pp.rays = (const float4*)rays;
  pp.out = (uint4*)out;
  pp.hits = ctx->d_paths_hits;
  pp.perFrame = perFrame;
  pp.giMaxDepth = d->gi_max_depth ? d->gi_max_depth : 16;
  pp.clampOutput = d->kernel_mode == LT_KERNEL_MODE_LINEAR;
  uint32_t launches = 0;
  if (const int rc = begin_ray_launches(ctx, &ctx->paths_ev, s)) return rc;   // (waits for the previous call: the control block and the scratch are its)
  for (uint64_t r0 = 0; r0 < n; r0 += raysPerSet) {
    pp.ray0 = (uint32_t)r0;
    pp.nRays = (uint32_t)std::min<uint64_t>(raysPerSet, n - r0);
    if (ctx->d_rank8 != nullptr) {   // lt_trace_kernel over the staged rays; its counters: the control block's first eight, its length: a spare one
      uint32_t* const count = ctx->d_giCtl + (8 + kMaxStack + 1) * kQueueStride;
      LT_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_giCtl, 0, kGiCtlWords * sizeof(uint32_t), s));
      LT_HIP_CHECK(ctx, lt_paths::launch_stage(pp, (float4*)ctx->d_gi[0], (float4*)ctx->d_gi[1], (uint4*)ctx->d_gi[3], count, s));
      TraceParams tp{};
      tp.o = (const float4*)ctx->d_gi[0]; tp.d = (const float4*)ctx->d_gi[1]; tp.m = (const uint4*)ctx->d_gi[3];
      tp.hit = ctx->d_paths_hits;
      tp.count = count;
      tp.next = ctx->d_giCtl;
      tp.refill = k.trace_refill;
      hipLaunchKernelGGL((lt_trace_kernel<kGI, false>), dim3((uint32_t)ctx->cu_count * 4u * LT_GI_STAGE_WAVES), dim3(kBlock),
                         (uint32_t)((kTraceRows + kTraceStage) * kBlock * sizeof(int)), s, sc, tp);
      LT_HIP_CHECK(ctx, hipGetLastError());
      launches += 2;
    } else {
      LT_HIP_CHECK(ctx, lt_paths::launch_camera(sc, pp, s));
      launches++;
    }
    for (uint32_t f0 = 0; f0 < frames; f0 += framesPerSet) {
      pp.frames = std::min(framesPerSet, frames - f0);
      pp.folded = f0;
      pp.sample = call.gi25 ? (d->frame_first + f0) * 32u : d->frame_first + f0;
      const int rc = with_math(call.devlibm, [&](auto m) { return launch_paths_set<Config<false, false, decltype(m)::value>>(ctx, k, sc, pp, s, launches); });
      if (rc) return rc;
    }
  }
  return end_ray_launches(ctx, ctx->paths_ev, s, launches, n, 0);
}

extern "C" int lt_hip_shade_paths(lt_hip_context* ctx, const lt_hip_paths_desc* desc, const lt_hip_shade_ray* rays, uint64_t n, lt_hip_shade* out,
                                  uint64_t out_bytes) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, false, nullptr, check_paths, enqueue_paths);
}

extern "C" int lt_hip_shade_paths_device(lt_hip_context* ctx, const lt_hip_paths_desc* desc, const lt_hip_shade_ray* rays, uint64_t n, lt_hip_shade* out,
                                         uint64_t out_bytes, void* hip_stream) {
  return run_ray_call(ctx, desc, rays, n, out, out_bytes, true, hip_stream, check_paths, enqueue_paths);
}

extern "C" int lt_hip_untile(lt_hip_context* ctx, const float* gathered, uint64_t floats_per_rank, uint32_t n_ranks, uint32_t width,
                             uint32_t height, uint32_t depth, uint32_t tile_w, uint32_t tile_h, float* image_out, void* hip_stream) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  if (!gathered || !image_out || !n_ranks || !width || !height || depth < 1 || !tile_w || !tile_h)
    return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_untile: bad argument");
  // (the images the render calls take, plan_tiles: lt_untile_kernel's tile index and its grid of one thread per pixel are 32-bit)
  if ((uint64_t)width * height > 0x7fffffffull) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_untile: image too large");
  const uint32_t tilesX = (width + tile_w - 1) / tile_w, tilesY = (height + tile_h - 1) / tile_h;
  const uint64_t maxTilesPerRank = ((uint64_t)tilesX * tilesY + n_ranks - 1) / n_ranks;
  if (floats_per_rank < maxTilesPerRank * tile_w * tile_h * depth) return fail(ctx, LT_ERR_BUFFER_TOO_SMALL, "lt_hip_untile: floats_per_rank too small");
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint64_t n = (uint64_t)width * height;
  hipLaunchKernelGGL(lt_untile_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, gathered,
                     floats_per_rank, n_ranks, width, height, depth, tile_w, tile_h, tilesX, image_out);
  LT_HIP_CHECK(ctx, hipGetLastError());
  return LT_OK;
}

extern "C" int lt_hip_synchronize(lt_hip_context* ctx, void* hip_stream) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LT_HIP_CHECK(ctx, hipStreamSynchronize((hipStream_t)hip_stream));
  return LT_OK;
}

extern "C" int lt_hip_read_scene_structure(lt_hip_context* ctx, int what, void* out, uint64_t capacity, uint64_t* out_bytes) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  if (!out_bytes || what < 0 || what > 5) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_read_scene_structure: bad arguments");
  if (!ctx->has_scene) return fail(ctx, LT_ERR_NO_SCENE, "no scene uploaded");
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool own = ctx->d_nodes2 && ctx->d_wide && ctx->d_rank8;
  uint32_t info[4] = {(uint32_t)ctx->height2, (uint32_t)ctx->wide_height, ctx->n_wide, ctx->device_prepared ? 1u : 0u};
  const void* src = nullptr;
  uint64_t bytes = 0;
  if (what == 3) { bytes = sizeof(info); }
  else if (own && what == 0) { src = ctx->d_nodes2; bytes = (uint64_t)ctx->n_nodes2 * 32; }
  else if (own && what == 1) { src = ctx->d_rank8; bytes = (uint64_t)ctx->n_prims * 32; }
  else if (own && what == 2) { src = ctx->d_wide; bytes = ((uint64_t)ctx->n_wide + ctx->n_prims + 1) * 64 + 64; }
  else if (own && what == 4 && ctx->d_pairs2) { src = ctx->d_pairs2; bytes = (uint64_t)ctx->n_nodes2 * 64; }
  else if (what == 5) { src = ctx->d_tris; bytes = (uint64_t)ctx->n_prims * 48; }
  *out_bytes = bytes;
  if (!out || bytes == 0) return LT_OK;
  if (capacity < bytes) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_read_scene_structure: buffer too small");
  if (what == 3) { memcpy(out, info, sizeof(info)); return LT_OK; }
  LT_HIP_CHECK(ctx, hipDeviceSynchronize());
  LT_HIP_CHECK(ctx, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
  return LT_OK;
}

// The entry cuts the context holds now, as the two-frame walk reads them: cuts_chunks planes of one record per square; none held:
// 0 bytes.
extern "C" int lt_hip_read_entry_cuts(lt_hip_context* ctx, void* out, uint64_t capacity, uint64_t* out_bytes) {
  if (!ctx) return LT_ERR_INVALID_ARGUMENT;
  if (!out_bytes) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_read_entry_cuts: bad arguments");
  uint64_t bytes = 0;
  if (ctx->cuts_valid && ctx->d_cuts && (uint64_t)ctx->cuts_plane_squares * ctx->cuts_chunks <= ctx->cuts_squares)
    bytes = (uint64_t)ctx->cuts_plane_squares * ctx->cuts_chunks * lt_entry_cut::kListWords * sizeof(uint32_t);
  *out_bytes = bytes;
  if (!out || bytes == 0) return LT_OK;
  if (capacity < bytes) return fail(ctx, LT_ERR_INVALID_ARGUMENT, "lt_hip_read_entry_cuts: buffer too small");
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LT_HIP_CHECK(ctx, hipDeviceSynchronize());
  LT_HIP_CHECK(ctx, hipMemcpy(out, ctx->d_cuts, bytes, hipMemcpyDeviceToHost));
  return LT_OK;
}

extern "C" uint64_t lt_hip_camera_hit_passes(const lt_hip_context* ctx) { return ctx ? ctx->camhit_passes : 0; }

// lt_entry_cut.hpp's interval test as the host compiles it, case by case: what lt_entry_cut_kernel asks of a lane and a box
// (light_box_pad, lane_set, may_reach).  out[i]: 0 the box is excluded, 1 it may be reached, 2 lane_set refuses the lane.
extern "C" int lt_hip_entry_cut_test_host(const float* origins, const float* light_boxes, const float* boxes, uint64_t n, uint8_t* out) {
  if ((!origins || !light_boxes || !boxes || !out) && n) return LT_ERR_INVALID_ARGUMENT;
  for (uint64_t i = 0; i < n; i++) {
    const float *o = origins + 3 * i, *L = light_boxes + 6 * i, *b = boxes + 6 * i;
    float Llo[3] = {L[0], L[1], L[2]}, Lhi[3] = {L[3], L[4], L[5]};
    for (int a = 0; a < 3; a++) lt_entry_cut::light_box_pad(Llo[a], Lhi[a]);
    lt_entry_cut::LaneSet ls;
    if (!lt_entry_cut::lane_set(o[0], o[1], o[2], Llo, Lhi, ls)) out[i] = 2;
    else out[i] = lt_entry_cut::may_reach(ls, b[0], b[1], b[2], b[3], b[4], b[5]) ? 1 : 0;
  }
  return LT_OK;
}

// lt_entry_cut.hpp's triangle test as the host compiles it: what the leaf pass of lt_entry_cut_kernel asks of a lane and a leaf's
// traversal triangle (A, v0v1, v0v2: nine floats).  out[i]: 0 the triangle is excluded, 1 it is kept, 2 lane_set refuses the lane.
extern "C" int lt_hip_entry_cut_triangle_test_host(const float* origins, const float* light_boxes, const float* triangles, uint64_t n, uint8_t* out) {
  if ((!origins || !light_boxes || !triangles || !out) && n) return LT_ERR_INVALID_ARGUMENT;
  for (uint64_t i = 0; i < n; i++) {
    const float *o = origins + 3 * i, *L = light_boxes + 6 * i, *t = triangles + 9 * i;
    float Llo[3] = {L[0], L[1], L[2]}, Lhi[3] = {L[3], L[4], L[5]};
    for (int a = 0; a < 3; a++) lt_entry_cut::light_box_pad(Llo[a], Lhi[a]);
    lt_entry_cut::LaneSet ls;
    if (!lt_entry_cut::lane_set(o[0], o[1], o[2], Llo, Lhi, ls)) out[i] = 2;
    else out[i] = lt_entry_cut::may_accept(ls, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]) ? 1 : 0;
  }
  return LT_OK;
}

// lt_device.hpp's random_fast_r as the host compiles it (the same operations: every fma spelled out, no contraction).
extern "C" int lt_hip_random_fast_test_host(int flavour, const float* args3, const double* r, uint64_t n, const double* params10, double* r_out,
                                            double* p, uint8_t* determined, float* a) {
  if ((!args3 && !r && n) || flavour < 0 || flavour > 2) return LT_ERR_INVALID_ARGUMENT;
  lt::RandomFastParams k;
  if (params10) {
    for (int i = 0; i < 8; i++) k.c[i] = params10[i];
    k.pi_lo = params10[8];
    k.delta = params10[9];
  }
  for (uint64_t i = 0; i < n; i++) {
    double ri;
    if (r) ri = r[i];
    else {
      const float* q = args3 + 3 * i;
      const double x = flavour == 2 ? lt::random_arg_<2>(q[0], q[1], q[2]) : lt::random_arg_<0>(q[0], q[1], q[2]);
      ri = lt::fmod_pi(x);
    }
    double pi;
    float ai;
    const bool det = params10 ? lt::random_fast_r_with(ri, k, pi, ai) : lt::random_fast_r(ri, pi, ai);
    if (r_out) r_out[i] = ri;
    if (p) p[i] = pi;
    if (determined) determined[i] = det ? 1 : 0;
    if (a) a[i] = ai;
  }
  return LT_OK;
}

extern "C" int lt_hip_entry_cut_leaf_counts(lt_hip_context* ctx, uint64_t* out3) {
  if (!ctx || !out3) return LT_ERR_INVALID_ARGUMENT;
  out3[0] = out3[1] = out3[2] = 0;
  if (ctx->cuts_valid && ctx->d_cut_stats) {
    LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->render_ev_recorded) LT_HIP_CHECK(ctx, hipEventSynchronize(ctx->render_ev));
    unsigned long long h[5];
    LT_HIP_CHECK(ctx, hipMemcpy(h, ctx->d_cut_stats, sizeof(h), hipMemcpyDeviceToHost));
    out3[0] = h[2];
    out3[1] = h[3];
    out3[2] = h[4];
  }
  return LT_OK;
}

extern "C" int lt_hip_entry_cut_chunk_counts(lt_hip_context* ctx, uint64_t* out23) {
  uint64_t* const out21 = out23;
  if (!ctx || !out23) return LT_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 7 + lt_entry_cut::kMaxChunks; i++) out23[i] = 0;
  if (ctx->cuts_valid && ctx->d_cut_stats) {
    LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->render_ev_recorded) LT_HIP_CHECK(ctx, hipEventSynchronize(ctx->render_ev));
    unsigned long long h[kEntryCutStats];
    LT_HIP_CHECK(ctx, hipMemcpy(h, ctx->d_cut_stats, sizeof(h), hipMemcpyDeviceToHost));
    out21[0] = ctx->cuts_chunks;
    out21[1] = h[5]; out21[2] = h[6];
    out21[3] = h[kEntryCutStatsPruned]; out21[4] = h[kEntryCutStatsPruned + 1];
    out21[5] = h[7]; out21[6] = h[8];
    for (int k = 0; k < lt_entry_cut::kMaxChunks; k++) out21[7 + k] = h[kEntryCutStatsChunks + k];
  }
  return LT_OK;
}

// lt_entry_cut.hpp's chunk arithmetic as the host compiles it: for n cases of (tree height, chunks asked for, entries of a list),
// out[4 * i ..]: entry_cut_limit of the height, the entries a list may have, the chunks this one takes, and the count of chunk
// `which[i]` of it.
extern "C" int lt_hip_entry_cut_chunks_test_host(const int32_t* heights, const uint32_t* chunks, const uint32_t* entries, const uint32_t* which,
                                                 uint64_t n, uint32_t* out) {
  if ((!heights || !chunks || !entries || !which || !out) && n) return LT_ERR_INVALID_ARGUMENT;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t limit = (uint32_t)lt_entry_cut::entry_cut_limit(heights[i]);
    out[4 * i + 0] = limit;
    out[4 * i + 1] = lt_entry_cut::chunk_capacity(limit, chunks[i]);
    out[4 * i + 2] = lt_entry_cut::chunk_count(entries[i], limit);
    out[4 * i + 3] = lt_entry_cut::chunk_entries(entries[i], limit, which[i]);
  }
  return LT_OK;
}

// lt_entry_cut.hpp's cut over the pruned tree as the host compiles it, on a recorded tree of n records (refs, parents, kids[2 n] as
// the leaf pass writes them down; survives[v] != 0: leaf record v survives): marks with pruned_mark in the order of the records,
// selects with pruned_cut_select.  out: room for cap references; *count: their number.
extern "C" int lt_hip_entry_cut_pruned_test_host(const uint32_t* refs, const uint16_t* parents, const uint16_t* kids, const uint8_t* survives,
                                                 uint32_t n, uint32_t cap, uint32_t* out, uint32_t* count) {
  if (!refs || !parents || !kids || !survives || !out || !count || n == 0 || n > (uint32_t)lt_entry_cut::kPruneRecords || cap < 2 ||
      cap > (uint32_t)lt_entry_cut::kMaxEntries)
    return LT_ERR_INVALID_ARGUMENT;
  std::vector<unsigned char> mark(n, 0), depth(cap + 2);
  std::vector<unsigned short> entry(cap + 2);
  for (uint32_t v = 0; v < n; v++)
    if ((int)refs[v] < 0 && survives[v]) lt_entry_cut::pruned_mark(parents, mark.data(), v);
  *count = lt_entry_cut::pruned_cut_select(refs, kids, mark.data(), cap, entry.data(), depth.data(), out);
  return LT_OK;
}

// Of the item table the context holds now (ensure_clear_items): out5[0] its entries and out5[1] the squares it hands out whole, as
// lt_clear_items_kernel counted them; out5[2] those of them that the host told some launch of the context's last render call to fold
// by their own wave (all or none: the host's decision, not a count by the render kernel -- that a launch did as told is what the
// pixels show); out5[3] the tables built so far; out5[4] 1 if some launch of the last render call took the table.
extern "C" int lt_hip_clear_item_counts(lt_hip_context* ctx, uint64_t* out5) {
  uint64_t* const out4 = out5;
  if (!ctx || !out5) return LT_ERR_INVALID_ARGUMENT;
  out4[0] = out4[1] = out4[2] = 0;
  out5[4] = ctx->last_tabled ? 1 : 0;
  out4[3] = ctx->item_builds;
  if (ctx->cuts_valid && ctx->items_groups != 0u && ctx->d_item_stats) {
    LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->render_ev_recorded) LT_HIP_CHECK(ctx, hipEventSynchronize(ctx->render_ev));
    unsigned long long h[2];
    LT_HIP_CHECK(ctx, hipMemcpy(h, ctx->d_item_stats, sizeof(h), hipMemcpyDeviceToHost));
    out4[0] = h[0];
    out4[1] = h[1];
    out4[2] = ctx->last_folded ? h[1] : 0;
  }
  return LT_OK;
}

// Of the context's last render launch, what its waves counted in render_clear_square (lt_kernel.hpp): out3[0] the clear squares that
// entered the one-pass path, out3[1] those of them that left it before their last frame group (the general path rendered the rest),
// out3[2] the frame groups rendered inside it.  All zero where the launch had no such path: no item table, LT_CLEAR_SQUARE=0,
// LT_DEBUG_SHADOW_FRAMES.  Waits for the context's last render.
extern "C" int lt_hip_clear_square_counts(lt_hip_context* ctx, uint64_t* out3) {
  if (!ctx || !out3) return LT_ERR_INVALID_ARGUMENT;
  out3[0] = out3[1] = out3[2] = 0;
  if (ctx->last_clear_queues == nullptr) return LT_OK;
  LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (ctx->render_ev_recorded) LT_HIP_CHECK(ctx, hipEventSynchronize(ctx->render_ev));
  uint32_t h[8 * kQueueStride];
  LT_HIP_CHECK(ctx, hipMemcpy(h, ctx->last_clear_queues, sizeof(h), hipMemcpyDeviceToHost));
  for (uint32_t xcd = 0; xcd < 8u; xcd++)
    for (uint32_t i = 0; i < 3u; i++) {
      uint64_t v;
      memcpy(&v, h + xcd * kQueueStride + kClearCountAt + 2u * i, sizeof(v));
      out3[i] += v;
    }
  return LT_OK;
}

// lt_entry_cut.hpp's item table and fold map as the host compiles them (item_entries, item_write, fold_mark_square), share by share
// as lt_clear_items_kernel lays them out: marks[p] is word 0 of the list of the square at hand-out position p < n, order[p] its
// square index (null: p).  table: room for 16 + n * groups words; map (null: none): a byte per segment of tiles_in_call stacked
// tiles of tile_w x tile_h pixels, tile_w a multiple of 8.
extern "C" int lt_hip_clear_items_test_host(const uint32_t* marks, const uint32_t* order, uint32_t n, uint32_t groups, uint32_t tile_w, uint32_t tile_h,
                                            uint32_t tiles_in_call, uint32_t* table, uint8_t* map) {
  if (!marks || !table || groups == 0 || (uint64_t)n * groups >= 0x80000000ull) return LT_ERR_INVALID_ARGUMENT;
  const uint32_t bptx = (tile_w + 7u) / 8u, bpty = (tile_h + 7u) / 8u;
  if (map && (tile_w == 0 || tile_w % 8u != 0 || tile_h == 0 || (uint64_t)tiles_in_call * bptx * bpty != n)) return LT_ERR_INVALID_ARGUMENT;
  for (uint32_t xcd = 0; xcd < 8u; xcd++) {
    const uint32_t share = xcd_share_size(n, xcd), start = xcd_share_start(n, xcd);
    uint32_t* const dst = table + lt_entry_cut::kItemHeader + (size_t)start * groups;
    uint32_t at = 0;
    for (uint32_t local = 0; local < share; local++) {
      const uint32_t word0 = marks[start + local];
      lt_entry_cut::item_write(dst + at, word0, local, groups);
      at += lt_entry_cut::item_entries(word0, groups);
      if (map) {
        const uint32_t b = order ? order[start + local] : start + local;
        if (b >= n) return LT_ERR_INVALID_ARGUMENT;
        lt_entry_cut::fold_mark_square(map, b, bptx, bptx * bpty, tile_w, tile_h, lt_entry_cut::item_whole(word0) ? 1 : 0);
      }
    }
    table[xcd] = at;
  }
  return LT_OK;
}

extern "C" int lt_hip_entry_cut_counts(lt_hip_context* ctx, uint64_t* out3) {
  if (!ctx || !out3) return LT_ERR_INVALID_ARGUMENT;
  out3[0] = ctx->cut_builds;
  out3[1] = out3[2] = 0;
  if (ctx->cuts_valid && ctx->d_cut_stats) {
    LT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->render_ev_recorded) LT_HIP_CHECK(ctx, hipEventSynchronize(ctx->render_ev));
    unsigned long long h[2];
    LT_HIP_CHECK(ctx, hipMemcpy(h, ctx->d_cut_stats, sizeof(h), hipMemcpyDeviceToHost));
    out3[1] = h[0];
    out3[2] = h[1];
  }
  return LT_OK;
}

extern "C" int lt_hip_get_stats(lt_hip_context* ctx, lt_hip_stats* out) {
  if (!ctx || !out) return LT_ERR_INVALID_ARGUMENT;
  int rc = finish_pending(ctx);
  if (rc) return rc;
  *out = ctx->last;
  out->scene_uploads = ctx->scene_uploads;
  out->scene_reused = ctx->scene_reused;
  out->own_tree_height = ctx->d_rank8 ? ctx->height2 : -1;
  out->own_tree_ms = ctx->retree_ms;
  return LT_OK;
}
