// lt_build.hip -- the canonical median build on the device (gfx950) and on the host: see lt_build.hpp and, for the rule itself,
// include/lenstrace_hip.h (lt_hip_set_triangles).
//
// The tree's shape depends on n alone (every leaf holds one triangle, the left child takes floor(count / 2)), so the build never
// moves a node: it only has to find, level by level, which triangles go left.
//   * one thread per triangle: the box, the centre 0.5f * lo + 0.5f * hi (two products, one sum), a monotone integer key of the
//     centre per axis with -0 merged into +0, the non-finite and material checks;
//   * three index lists, one per axis, sorted once by (key, input index): hipCUB's device radix sort over the keys with the input
//     indices as values -- it is stable, and the values go in ascending;
//   * per level, over the ranges of that level (kept per position: start, count, node): the extent of a range on an axis is the
//     centre of its last entry minus the centre of its first in that axis' list, so `dim` needs no reduction; the first
//     floor(count / 2) entries of the dim list go left; all three lists are then stably partitioned inside their ranges -- a flag per
//     entry, one exclusive scan over the 3n flags, one scatter.  A stable partition keeps each list sorted by (key, index) inside
//     both halves, which is the invariant the next level needs;
//   * a range that reaches one triangle writes its leaf; after ceil(log2 n) levels any list is the leaf order;
//   * the 76-byte primitives are gathered one thread per word (stores are contiguous, the reads are 36-byte runs);
//   * interior boxes are folded bottom-up, one launch per level, with IEEE minimum / maximum (min(-0, +0) = -0, max = +0);
//   * the lights: a flag per position, the same scan, the first 64 ranks write their position.
// The scan is three launches (tile sums, one workgroup over the sums, tiles again): no kernel waits for another workgroup, every
// loop is bounded by a count known when it starts.  All stores are vector stores of plain C++.
#include "lt_build.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <numeric>
#include <vector>

#include <hipcub/hipcub.hpp>

namespace lt_build {

constexpr uint32_t kThreads = 256, kPerThread = 4, kTile = kThreads * kPerThread;

__host__ __device__ inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
__host__ __device__ inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
// IEEE 754-2019 minimum / maximum of two numbers: equal values differ at most in the sign of a zero, which OR / AND of the bits settle
__host__ __device__ inline float ieee_min(float a, float b) { return a < b ? a : b < a ? b : u2f(f2u(a) | f2u(b)); }
__host__ __device__ inline float ieee_max(float a, float b) { return a > b ? a : b > a ? b : u2f(f2u(a) & f2u(b)); }
__host__ __device__ inline float centre(float lo, float hi) {
#ifdef __HIP_DEVICE_COMPILE__
  return __fadd_rn(__fmul_rn(0.5f, lo), __fmul_rn(0.5f, hi));
#else
  const volatile float a = 0.5f * lo, b = 0.5f * hi;   // (two rounded products whatever the host compiler's contraction rule is)
  return a + b;
#endif
}
__host__ __device__ inline bool finite_bits(float f) { return (f2u(f) & 0x7f800000u) != 0x7f800000u; }
// ascending keys for ascending floats, -0 and +0 on one key
__device__ inline uint32_t sort_key(float c) {
  uint32_t u = f2u(c);
  if ((u << 1) == 0) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline int pick_dim(float d0, float d1, float d2) { return (d0 > d1 && d0 > d2) ? 0 : (d1 > d2 ? 1 : 2); }

// -------------------------------------------------------------------------------------------------- kernels
__global__ void lt_build_centres_kernel(const float* __restrict__ pos, const int32_t* __restrict__ mi, uint32_t n, uint32_t n_mats,
                                        float* __restrict__ cen, uint32_t* __restrict__ keys, uint32_t* __restrict__ iota, uint32_t* flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v[9];
  uint32_t bad = 0;
  for (int k = 0; k < 9; k++) {
    v[k] = pos[(size_t)i * 9 + k];
    if (!finite_bits(v[k])) bad |= kFlagNonFinite;
  }
  if (mi) {
    const int32_t m = mi[i];
    if (m < 0 || (uint32_t)m >= n_mats) bad |= kFlagMaterial;
  }
  if (bad) atomicOr(flag, bad);
  for (int a = 0; a < 3; a++) {
    const float lo = ieee_min(ieee_min(v[a], v[3 + a]), v[6 + a]), hi = ieee_max(ieee_max(v[a], v[3 + a]), v[6 + a]);
    const float c = centre(lo, hi);
    cen[(size_t)a * n + i] = c;
    keys[(size_t)a * n + i] = sort_key(c);
  }
  iota[i] = i;
}

// a leaf: its triangle's box, its position in the ordered buffer, primitiveCount 1, axis 0, pad 0
__device__ inline void write_leaf(uint4* nodes, uint8_t* depth, uint32_t node, uint32_t p, uint32_t tri, const float* __restrict__ pos, uint32_t d) {
  float v[9];
  for (int k = 0; k < 9; k++) v[k] = pos[(size_t)tri * 9 + k];
  uint32_t lo[3], hi[3];
  for (int a = 0; a < 3; a++) {
    lo[a] = f2u(ieee_min(ieee_min(v[a], v[3 + a]), v[6 + a]));
    hi[a] = f2u(ieee_max(ieee_max(v[a], v[3 + a]), v[6 + a]));
  }
  nodes[2 * (size_t)node] = make_uint4(lo[0], lo[1], lo[2], hi[0]);
  nodes[2 * (size_t)node + 1] = make_uint4(hi[1], hi[2], p, 1u);
  depth[node] = (uint8_t)d;
}

// seg: start[n], count[n], node[n] of the range every position lies in
__global__ void lt_build_init_kernel(uint32_t* __restrict__ seg, uint32_t n, uint4* nodes, uint8_t* depth, const float* __restrict__ pos) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  seg[p] = 0;
  seg[(size_t)n + p] = n;
  seg[2 * (size_t)n + p] = 0;
  if (n == 1) write_leaf(nodes, depth, 0, 0, 0, pos, 0);
}

__global__ void lt_build_split_kernel(const uint32_t* __restrict__ seg, const uint32_t* __restrict__ lists, const float* __restrict__ cen, uint32_t n,
                                      uint32_t level, uint8_t* __restrict__ goLeft, uint4* nodes, uint8_t* depth) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t s = seg[p], c = seg[(size_t)n + p];
  if (c < 2) return;
  const uint32_t e = s + c - 1;
  float d[3];
  for (int a = 0; a < 3; a++) {
    const size_t base = (size_t)a * n;
    d[a] = __fsub_rn(cen[base + lists[base + e]], cen[base + lists[base + s]]);
  }
  const int dim = pick_dim(d[0], d[1], d[2]);
  const uint32_t lc = c >> 1;
  goLeft[lists[(size_t)dim * n + p]] = (p - s < lc) ? 1 : 0;
  if (p == s) {
    const uint32_t node = seg[2 * (size_t)n + p];
    // (the box words are the fold's; secondChildOffset = node + 1 + (2 lc - 1), primitiveCount 0, axis, pad 0)
    ((uint2*)nodes)[4 * (size_t)node + 3] = make_uint2(node + 2 * lc, (uint32_t)dim << 16);
    depth[node] = (uint8_t)level;
  }
}

// t runs over the three lists laid end to end
__global__ void lt_build_flag_kernel(const uint32_t* __restrict__ seg, const uint32_t* __restrict__ lists, const uint8_t* __restrict__ goLeft, uint32_t n,
                                     uint32_t* __restrict__ flags) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const uint32_t p = t % n;
  flags[t] = seg[(size_t)n + p] >= 2 ? (uint32_t)goLeft[lists[t]] : 0u;
}

__global__ void __launch_bounds__(kThreads) lt_build_tile_sum_kernel(const uint32_t* __restrict__ flags, uint32_t N, uint32_t* __restrict__ partial) {
  typedef hipcub::BlockReduce<uint32_t, kThreads> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint32_t base = blockIdx.x * kTile + threadIdx.x * kPerThread;
  uint32_t sum = 0;
  for (uint32_t k = 0; k < kPerThread; k++)
    if (base + k < N) sum += flags[base + k];
  const uint32_t total = Reduce(tmp).Sum(sum);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: partial[0 .. B) becomes its exclusive prefix sum
__global__ void __launch_bounds__(kThreads) lt_build_partial_scan_kernel(uint32_t* partial, uint32_t B) {
  typedef hipcub::BlockScan<uint32_t, kThreads> Scan;
  __shared__ typename Scan::TempStorage tmp;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < B; base += kThreads) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < B ? partial[i] : 0u;
    uint32_t excl, total;
    Scan(tmp).ExclusiveSum(v, excl, total);
    if (i < B) partial[i] = carry + excl;
    carry += total;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kThreads) lt_build_tile_scan_kernel(const uint32_t* __restrict__ flags, uint32_t N, const uint32_t* __restrict__ partial,
                                                                      uint32_t* __restrict__ scan) {
  typedef hipcub::BlockScan<uint32_t, kThreads> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const uint32_t base = blockIdx.x * kTile + threadIdx.x * kPerThread;
  uint32_t v[kPerThread], sum = 0;
  for (uint32_t k = 0; k < kPerThread; k++) {
    v[k] = base + k < N ? flags[base + k] : 0u;
    sum += v[k];
  }
  uint32_t excl;
  Scan(tmp).ExclusiveSum(sum, excl);
  uint32_t run = partial[blockIdx.x] + excl;
  for (uint32_t k = 0; k < kPerThread; k++) {
    if (base + k < N) scan[base + k] = run;
    run += v[k];
  }
}

// the stable partition of every range of every list: the lefts keep their order in front, the rights theirs behind
__global__ void lt_build_scatter_kernel(const uint32_t* __restrict__ seg, const uint32_t* __restrict__ lists, const uint32_t* __restrict__ flags,
                                        const uint32_t* __restrict__ scan, uint32_t n, uint32_t* __restrict__ listsOut) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * n) return;
  const uint32_t a = t / n, p = t - a * n;
  const uint32_t s = seg[p], c = seg[(size_t)n + p];
  const uint32_t tri = lists[t];
  if (c < 2) { listsOut[t] = tri; return; }
  const uint32_t lc = c >> 1;
  const uint32_t leftsBefore = scan[t] - scan[a * n + s];
  const uint32_t dst = flags[t] ? s + leftsBefore : s + lc + (p - s - leftsBefore);
  listsOut[a * n + dst] = tri;
}

// every position moves on to its child range; a range of one triangle writes its leaf
__global__ void lt_build_advance_kernel(uint32_t* __restrict__ seg, const uint32_t* __restrict__ lists, uint32_t n, uint32_t level, uint4* nodes,
                                        uint8_t* depth, const float* __restrict__ pos) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t s = seg[p], c = seg[(size_t)n + p], node = seg[2 * (size_t)n + p];
  if (c < 2) return;
  const uint32_t lc = c >> 1;
  const bool left = p - s < lc;
  const uint32_t ns = left ? s : s + lc, nc = left ? lc : c - lc, nn = left ? node + 1 : node + 2 * lc;
  seg[p] = ns;
  seg[(size_t)n + p] = nc;
  seg[2 * (size_t)n + p] = nn;
  if (nc == 1) write_leaf(nodes, depth, nn, p, lists[p], pos, level + 1);
}

__global__ void lt_build_fold_kernel(uint4* nodes, const uint8_t* __restrict__ depth, uint32_t n_nodes, uint32_t level) {
  const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n_nodes || depth[node] != level) return;
  const uint4 w = nodes[2 * (size_t)node + 1];
  if ((w.w & 0xffffu) != 0) return;   // a leaf
  const uint32_t l = node + 1, r = w.z;
  const uint4 l0 = nodes[2 * (size_t)l], l1 = nodes[2 * (size_t)l + 1], r0 = nodes[2 * (size_t)r], r1 = nodes[2 * (size_t)r + 1];
  nodes[2 * (size_t)node] = make_uint4(f2u(ieee_min(u2f(l0.x), u2f(r0.x))), f2u(ieee_min(u2f(l0.y), u2f(r0.y))), f2u(ieee_min(u2f(l0.z), u2f(r0.z))),
                                       f2u(ieee_max(u2f(l0.w), u2f(r0.w))));
  nodes[2 * (size_t)node + 1] = make_uint4(f2u(ieee_max(u2f(l1.x), u2f(r1.x))), f2u(ieee_max(u2f(l1.y), u2f(r1.y))), w.z, w.w);
}

// t runs over the 19 words of every ordered primitive: positions, normals, materialIndex
__global__ void lt_build_gather_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ nrm,
                                       const int32_t* __restrict__ mi, uint32_t n, uint32_t* __restrict__ prims) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 19u * n) return;
  const uint32_t p = t / 19u, w = t - 19u * p;
  const uint32_t tri = order[p];
  prims[t] = w < 9 ? pos[(size_t)tri * 9 + w] : w < 18 ? nrm[(size_t)tri * 9 + (w - 9)] : mi ? (uint32_t)mi[tri] : 0u;
}

__global__ void lt_build_light_flag_kernel(const uint32_t* __restrict__ order, const int32_t* __restrict__ mi, const float* __restrict__ mats, uint32_t n,
                                           uint32_t* __restrict__ flags) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float* m = mats + 8 * (size_t)(mi ? mi[order[p]] : 0);
  flags[p] = (m[5] > 0.0f || m[6] > 0.0f || m[7] > 0.0f) ? 1u : 0u;
}

__global__ void lt_build_lights_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ scan, uint32_t n, uint32_t* __restrict__ lights) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  if (flags[p] && scan[p] < 64u) lights[1 + scan[p]] = p;
  if (p == n - 1) lights[0] = min(64u, scan[p] + flags[p]);
}

// -------------------------------------------------------------------------------------------------- the device build
static int ceil_log2(uint32_t n) {
  int l = 0;
  while (((uint64_t)1 << l) < n) l++;
  return l;
}

void release(Out& out, const lt_prep::Allocator& al) {
  for (void** p : {&out.d_nodes, &out.d_prims, &out.d_lights}) {
    if (*p) al.put(al.self, *p);
    *p = nullptr;
  }
}

namespace {
struct Temps {   // (whatever it handed out goes back when it leaves scope)
  const lt_prep::Allocator& al;
  std::vector<void*> held;
  ~Temps() { for (void* p : held) al.put(al.self, p); }
  hipError_t get(void** p, size_t bytes) {
    const hipError_t e = al.get(al.self, p, bytes);
    if (e == hipSuccess) held.push_back(*p);
    return e;
  }
};
}  // namespace

#define LT_BUILD_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { release(out, al); return e_; } } while (0)

// flags[0 .. N) -> scan[0 .. N), exclusive
static hipError_t exclusive_scan(const uint32_t* flags, uint32_t N, uint32_t* partial, uint32_t* scan, hipStream_t stream) {
  const uint32_t tiles = (N + kTile - 1) / kTile;
  hipLaunchKernelGGL(lt_build_tile_sum_kernel, dim3(tiles), dim3(kThreads), 0, stream, flags, N, partial);
  hipLaunchKernelGGL(lt_build_partial_scan_kernel, dim3(1), dim3(kThreads), 0, stream, partial, tiles);
  hipLaunchKernelGGL(lt_build_tile_scan_kernel, dim3(tiles), dim3(kThreads), 0, stream, flags, N, (const uint32_t*)partial, scan);
  return hipGetLastError();
}

hipError_t run(const float* d_pos, const float* d_nrm, const int32_t* d_mi, const void* d_mats, uint32_t n_mats, uint32_t n, hipStream_t stream,
               uint32_t* d_flag, bool timed, const lt_prep::Allocator& al, Out& out) {
  out = Out();
  Temps tmp{al, {}};
  const size_t N = n;
  const uint32_t n_nodes = 2 * n - 1, blocksN = (n + kThreads - 1) / kThreads, blocks3N = (3 * n + kThreads - 1) / kThreads;
  const uint32_t tiles = (3 * n + kTile - 1) / kTile;
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](float& ms) -> hipError_t {
    if (!timed) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(stream);
    const auto now = std::chrono::steady_clock::now();
    ms = std::chrono::duration<float, std::milli>(now - t0).count();
    t0 = now;
    return e;
  };

  float* cen = nullptr;
  uint32_t *keys = nullptr, *keysOut = nullptr, *iota = nullptr, *lists = nullptr, *lists2 = nullptr;
  LT_BUILD_TRY(tmp.get((void**)&cen, 12 * N));
  LT_BUILD_TRY(tmp.get((void**)&keys, 12 * N));
  LT_BUILD_TRY(tmp.get((void**)&keysOut, 4 * N));
  LT_BUILD_TRY(tmp.get((void**)&iota, 4 * N));
  LT_BUILD_TRY(tmp.get((void**)&lists, 12 * N));
  LT_BUILD_TRY(tmp.get((void**)&lists2, 12 * N));
  LT_BUILD_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), stream));
  hipLaunchKernelGGL(lt_build_centres_kernel, dim3(blocksN), dim3(kThreads), 0, stream, d_pos, d_mi, n, n_mats, cen, keys, iota, d_flag);
  LT_BUILD_TRY(hipGetLastError());
  uint32_t flags = 0;
  LT_BUILD_TRY(hipMemcpyAsync(&flags, d_flag, sizeof(flags), hipMemcpyDeviceToHost, stream));
  LT_BUILD_TRY(hipStreamSynchronize(stream));
  if (flags) { out.flags = flags; return hipSuccess; }

  {   // the three lists
    size_t sortBytes = 0;
    LT_BUILD_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, keys, keysOut, iota, lists, (int)n, 0, 32, stream));
    void* sortTmp = nullptr;
    LT_BUILD_TRY(tmp.get(&sortTmp, sortBytes));
    for (int a = 0; a < 3; a++)
      LT_BUILD_TRY(hipcub::DeviceRadixSort::SortPairs(sortTmp, sortBytes, keys + a * N, keysOut, iota, lists + a * N, (int)n, 0, 32, stream));
  }
  LT_BUILD_TRY(lap(out.ms_sort));

  uint32_t *seg = nullptr, *flagWords = nullptr, *scan = nullptr, *partial = nullptr;
  uint8_t *goLeft = nullptr, *depth = nullptr;
  LT_BUILD_TRY(tmp.get((void**)&seg, 12 * N));
  LT_BUILD_TRY(tmp.get((void**)&flagWords, 12 * N));
  LT_BUILD_TRY(tmp.get((void**)&scan, 12 * N));
  LT_BUILD_TRY(tmp.get((void**)&partial, 4 * (size_t)tiles));
  LT_BUILD_TRY(tmp.get((void**)&goLeft, N));
  LT_BUILD_TRY(tmp.get((void**)&depth, n_nodes));
  LT_BUILD_TRY(al.get(al.self, &out.d_nodes, 32 * (size_t)n_nodes));
  LT_BUILD_TRY(al.get(al.self, &out.d_prims, 76 * N));
  LT_BUILD_TRY(al.get(al.self, &out.d_lights, 260));
  uint4* nodes = (uint4*)out.d_nodes;
  out.height = ceil_log2(n);

  hipLaunchKernelGGL(lt_build_init_kernel, dim3(blocksN), dim3(kThreads), 0, stream, seg, n, nodes, depth, d_pos);
  for (int level = 0; level < out.height; level++) {
    hipLaunchKernelGGL(lt_build_split_kernel, dim3(blocksN), dim3(kThreads), 0, stream, (const uint32_t*)seg, (const uint32_t*)lists, (const float*)cen, n,
                       (uint32_t)level, goLeft, nodes, depth);
    hipLaunchKernelGGL(lt_build_flag_kernel, dim3(blocks3N), dim3(kThreads), 0, stream, (const uint32_t*)seg, (const uint32_t*)lists,
                       (const uint8_t*)goLeft, n, flagWords);
    LT_BUILD_TRY(exclusive_scan(flagWords, 3 * n, partial, scan, stream));
    hipLaunchKernelGGL(lt_build_scatter_kernel, dim3(blocks3N), dim3(kThreads), 0, stream, (const uint32_t*)seg, (const uint32_t*)lists,
                       (const uint32_t*)flagWords, (const uint32_t*)scan, n, lists2);
    hipLaunchKernelGGL(lt_build_advance_kernel, dim3(blocksN), dim3(kThreads), 0, stream, seg, (const uint32_t*)lists2, n, (uint32_t)level, nodes, depth,
                       d_pos);
    LT_BUILD_TRY(hipGetLastError());
    std::swap(lists, lists2);
  }
  LT_BUILD_TRY(lap(out.ms_levels));

  const uint32_t* order = lists;   // (at the leaves the three lists agree)
  hipLaunchKernelGGL(lt_build_gather_kernel, dim3((19u * n + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, order, (const uint32_t*)d_pos,
                     (const uint32_t*)d_nrm, d_mi, n, (uint32_t*)out.d_prims);
  for (int level = out.height - 1; level >= 0; level--)
    hipLaunchKernelGGL(lt_build_fold_kernel, dim3((n_nodes + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, nodes, (const uint8_t*)depth, n_nodes,
                       (uint32_t)level);
  LT_BUILD_TRY(hipGetLastError());
  LT_BUILD_TRY(hipMemsetAsync(out.d_lights, 0, 260, stream));
  hipLaunchKernelGGL(lt_build_light_flag_kernel, dim3(blocksN), dim3(kThreads), 0, stream, order, d_mi, (const float*)d_mats, n, flagWords);
  LT_BUILD_TRY(exclusive_scan(flagWords, n, partial, scan, stream));
  hipLaunchKernelGGL(lt_build_lights_kernel, dim3(blocksN), dim3(kThreads), 0, stream, (const uint32_t*)flagWords, (const uint32_t*)scan, n,
                     (uint32_t*)out.d_lights);
  LT_BUILD_TRY(hipGetLastError());
  LT_BUILD_TRY(hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind this)
  LT_BUILD_TRY(lap(out.ms_finish));
  return hipSuccess;
}

// -------------------------------------------------------------------------------------------------- the host build
uint32_t build_host(const float* pos, const float* nrm, const int32_t* mi, const void* materials, uint32_t n_mats, uint32_t n, void* nodesOut,
                    void* primsOut, void* lightsOut) {
  uint32_t bad = 0;
  for (size_t k = 0; k < 9 * (size_t)n; k++)
    if (!finite_bits(pos[k])) { bad |= kFlagNonFinite; break; }
  if (mi)
    for (uint32_t i = 0; i < n; i++)
      if (mi[i] < 0 || (uint32_t)mi[i] >= n_mats) { bad |= kFlagMaterial; break; }
  if (bad) return bad;

  struct Node { float lo[3], hi[3]; int32_t off; uint16_t cnt; uint8_t axis, pad; };
  static_assert(sizeof(Node) == 32, "LinearBVHNode");
  std::vector<float> cen[3];
  for (int a = 0; a < 3; a++) cen[a].resize(n);
  auto box = [&](uint32_t i, float* lo, float* hi) {
    const float* v = pos + 9 * (size_t)i;
    for (int a = 0; a < 3; a++) {
      lo[a] = ieee_min(ieee_min(v[a], v[3 + a]), v[6 + a]);
      hi[a] = ieee_max(ieee_max(v[a], v[3 + a]), v[6 + a]);
    }
  };
  for (uint32_t i = 0; i < n; i++) {
    float lo[3], hi[3];
    box(i, lo, hi);
    for (int a = 0; a < 3; a++) cen[a][i] = centre(lo[a], hi[a]);
  }
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::vector<Node> nodes(2 * (size_t)n - 1);
  memset(nodes.data(), 0, nodes.size() * sizeof(Node));
  struct Range { uint32_t start, end, node; };
  std::vector<Range> work{{0, n, 0}};
  while (!work.empty()) {
    const Range r = work.back();
    work.pop_back();
    Node& node = nodes[r.node];
    const uint32_t count = r.end - r.start;
    if (count == 1) {
      box(order[r.start], node.lo, node.hi);
      node.off = (int32_t)r.start;
      node.cnt = 1;
      continue;
    }
    float d[3];
    for (int a = 0; a < 3; a++) {
      float cmin = cen[a][order[r.start]], cmax = cmin;
      for (uint32_t i = r.start + 1; i < r.end; i++) {
        const float c = cen[a][order[i]];
        if (c < cmin) cmin = c;
        if (c > cmax) cmax = c;
      }
      const volatile float ext = cmax - cmin;
      d[a] = ext;
    }
    const int dim = pick_dim(d[0], d[1], d[2]);
    const uint32_t lc = count / 2;
    const std::vector<float>& c = cen[dim];
    // (c[dim], input index) is a total order, so which triangles are the first lc does not depend on how they are found
    std::nth_element(order.begin() + r.start, order.begin() + r.start + lc, order.begin() + r.end,
                     [&](uint32_t x, uint32_t y) { return c[x] < c[y] || (c[x] == c[y] && x < y); });
    node.axis = (uint8_t)dim;
    node.off = (int32_t)(r.node + 2 * lc);
    work.push_back({r.start + lc, r.end, r.node + 2 * lc});
    work.push_back({r.start, r.start + lc, r.node + 1});
  }
  for (size_t i = nodes.size(); i-- > 0;) {   // (pre-order: both children lie behind their parent)
    Node& node = nodes[i];
    if (node.cnt) continue;
    const Node &l = nodes[i + 1], &r = nodes[node.off];
    for (int a = 0; a < 3; a++) {
      node.lo[a] = ieee_min(l.lo[a], r.lo[a]);
      node.hi[a] = ieee_max(l.hi[a], r.hi[a]);
    }
  }
  memcpy(nodesOut, nodes.data(), nodes.size() * sizeof(Node));
  uint32_t lights[65];
  memset(lights, 0, sizeof(lights));
  uint8_t* prims = (uint8_t*)primsOut;
  const float* mats = (const float*)materials;
  for (uint32_t p = 0; p < n; p++) {
    const uint32_t i = order[p];
    const int32_t m = mi ? mi[i] : 0;
    memcpy(prims + 76 * (size_t)p, pos + 9 * (size_t)i, 36);
    memcpy(prims + 76 * (size_t)p + 36, nrm + 9 * (size_t)i, 36);
    memcpy(prims + 76 * (size_t)p + 72, &m, 4);
    const float* e = mats + 8 * (size_t)m + 5;
    if ((e[0] > 0.0f || e[1] > 0.0f || e[2] > 0.0f) && lights[0] < 64) lights[1 + lights[0]++] = p;
  }
  memcpy(lightsOut, lights, 260);
  return 0;
}

}  // namespace lt_build
