// lt_overlist.hip -- the two steps of an overlap list (lt_overlist.hpp) that are not a walk: the exclusive scan that turns the
// queries' counts into the segments' bounds, and the ordering of each segment.  The count and the fill are lt_overlap.hip's and
// lt_tritri.hip's kernels with the sinks kCountWide and kList (lt_overlap.hpp).  The radius lists (lt_hip_nearest_list) share both
// steps: their count and fill are lt_nearest.hip's kernel with its kCountWide and kList, and their segments are 16-byte records.
// So do the hit lists (lt_hip_trace_hits_list), with lt_query_hits_kernel's kinds of the same names; their order needs the rays.
//
// Neither step waits for another workgroup.  The scan is three launches -- per-tile sums, one workgroup over those sums, per-tile
// scans plus the tile's base -- and the stream orders them.  A segment is sorted by one wave alone.
#include "lt_overlist.hpp"
#include "lt_device.hpp"
#include "lt_nearest.hpp"
#include "lt_query.hpp"

using namespace lt;

namespace {

using u64 = unsigned long long;

constexpr uint32_t kScanLanes = 256;
constexpr uint32_t kScanPer = lt_overlist::kListScanTile / kScanLanes;   // consecutive words per lane
static_assert(kScanPer * kScanLanes == lt_overlist::kListScanTile && (kScanLanes & (kScanLanes - 1)) == 0, "the scan's tile");

// The exclusive prefix of `v` over the workgroup's lanes, and the sum over all of them.  `row`: kScanLanes words of LDS, free
// to be reused when the call returns.
__device__ __forceinline__ u64 lanes_exclusive(u64 v, u64* row, u64& sum) {
  const uint32_t t = threadIdx.x;
  row[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kScanLanes; d <<= 1) {
    const u64 below = t >= d ? row[t - d] : 0ull;
    __syncthreads();
    row[t] += below;
    __syncthreads();
  }
  const u64 inclusive = row[t];
  sum = row[kScanLanes - 1];
  __syncthreads();
  return inclusive - v;
}

// A lane's kScanPer consecutive words from word `first` on; words from `count` on read as 0.
__device__ __forceinline__ u64 load_words(const u64* a, u64 first, u64 count, u64 (&v)[kScanPer]) {
  u64 sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; k++) {
    v[k] = first + k < count ? a[first + k] : 0ull;
    sum += v[k];
  }
  return sum;
}

}  // namespace

// Scan, first launch: partials[tile] = the sum of the tile's words.  The words are offsets[0 .. n); word n counts as 0.
__global__ __launch_bounds__(kScanLanes) void lt_list_tile_sums_kernel(const u64* offsets, uint32_t n, u64* partials) {
  __shared__ u64 row[kScanLanes];
  u64 v[kScanPer], sum;
  const u64 mine = load_words(offsets, (u64)blockIdx.x * lt_overlist::kListScanTile + (u64)threadIdx.x * kScanPer, n, v);
  lanes_exclusive(mine, row, sum);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// Scan, second launch: one workgroup turns the `tiles` sums into the tiles' bases, a tile of them at a time with the sum so far.
__global__ __launch_bounds__(kScanLanes) void lt_list_scan_partials_kernel(u64* partials, uint32_t tiles) {
  __shared__ u64 row[kScanLanes];
  u64 carry = 0;
  for (u64 base = 0; base < tiles; base += lt_overlist::kListScanTile) {
    const u64 first = base + (u64)threadIdx.x * kScanPer;
    u64 v[kScanPer], sum;
    const u64 mine = load_words(partials, first, tiles, v);
    u64 at = carry + lanes_exclusive(mine, row, sum);
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; k++) {
      if (first + k < tiles) partials[first + k] = at;
      at += v[k];
    }
    carry += sum;
  }
}

// Scan, third launch: every tile's own exclusive scan plus its base, written over offsets[0 .. n].
__global__ __launch_bounds__(kScanLanes) void lt_list_tile_scan_kernel(u64* offsets, uint32_t n, const u64* partials) {
  __shared__ u64 row[kScanLanes];
  const u64 first = (u64)blockIdx.x * lt_overlist::kListScanTile + (u64)threadIdx.x * kScanPer;
  u64 v[kScanPer], sum;
  const u64 mine = load_words(offsets, first, n, v);
  u64 at = partials[blockIdx.x] + lanes_exclusive(mine, row, sum);
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; k++) {
    if (first + k <= n) offsets[first + k] = at;
    at += v[k];
  }
}

namespace {

// The two elements a segment is made of, the order of each and the longest segment of them that is sorted in LDS: an overlap
// list's int32 offsets by `<`, a radius list's 16-byte records by lt_nearest::record_before on (d2, prim).
__device__ __forceinline__ bool smaller(int32_t a, int32_t b) { return a < b; }
__device__ __forceinline__ bool smaller(const uint4& a, const uint4& b) {
  return lt_nearest::record_before(lt_nearest::Record{__uint_as_float(a.x), (int32_t)a.y, 0.0f, 0.0f},
                                   lt_nearest::Record{__uint_as_float(b.x), (int32_t)b.y, 0.0f, 0.0f});
}
template <class T> struct Span;
template <> struct Span<int32_t> { static constexpr uint32_t kWords = lt_overlist::kListSortSpan; };
template <> struct Span<uint4> { static constexpr uint32_t kWords = lt_overlist::kListSortSpanHits; };

// An order, as the ordering kernel asks for it: take(q, key) -- is query q's segment this kernel's to sort, and the word its
// comparator wants to know about the query --, and before(a, b, key).  The overlap and the radius lists: every segment, by
// `smaller`, no word.
template <class T>
struct PlainOrder {
  __device__ __forceinline__ bool take(u64, uint32_t&) const { return true; }
  __device__ __forceinline__ bool before(const T& a, const T& b, uint32_t) const { return smaller(a, b); }
};

// The hit lists' records {t, prim, u, v} of the rays the own tree takes (lt_query::own_tree_takes: the kernel's own predicate on
// the same ray), which fill their segments in the own hierarchy's order: t by the float `<`, bit-equal t (-0 == +0) by the
// reference's leaf order for the ray's octant -- rank8, read on ties only; the octant is the word, from the signs of 1 / direction
// as own_ray computes it.  In a scene with an own tree a primitive has one leaf, so this is a strict total order over the distinct
// records of a segment, and the network's result is the sequence although the network is not stable.  The other rays' segments
// are sorted when they are filled (lt_query.hip, HitInsert) and are left as they are.  (A segment the caller's offsets made longer
// than the ray's sequence ends in whatever the caller's buffer held: a primitive that is none of the scene's has no row in the
// table and goes behind those that have, by its own bits.)
struct RayHitOrder {
  const float4* rays;
  const uint32_t* rank8;
  uint32_t nPrims;
  __device__ __forceinline__ u64 rank(uint32_t prim, uint32_t octant) const {
    return prim < nPrims ? (u64)rank8[8 * (size_t)prim + octant] : (1ull << 32) | prim;
  }
  __device__ __forceinline__ bool take(u64 q, uint32_t& octant) const {
    const float4 a = rays[2 * q], b = rays[2 * q + 1];
    const Ray ray{mk4(a.x, a.y, a.z, 1.0f), mk4(b.x, b.y, b.z, 0.0f)};
    const float ix = 1.0f / ray.d.x, iy = 1.0f / ray.d.y, iz = 1.0f / ray.d.z;
    octant = (ix < 0.0f ? 1u : 0u) | (iy < 0.0f ? 2u : 0u) | (iz < 0.0f ? 4u : 0u);
    return lt_query::own_tree_takes(ray, ix, iy, iz);
  }
  __device__ __forceinline__ bool before(const uint4& a, const uint4& b, uint32_t octant) const {
    const float ta = __uint_as_float(a.x), tb = __uint_as_float(b.x);
    return ta < tb || (ta == tb && rank(a.y, octant) < rank(b.y, octant));
  }
};

template <class T, class ORDER>
__device__ __forceinline__ void put_smaller_first(T* w, u64 lo, u64 hi, const ORDER& order, uint32_t key) {
  const T a = w[lo], b = w[hi];
  if (order.before(b, a, key)) { w[lo] = b; w[hi] = a; }
}

// Sorts w[0 .. L) ascending, L >= 2, by the normalised bitonic network over P = the power of two at or above L: every comparator
// puts the smaller word at the lower index, so the words behind L may be thought of as +inf, a comparator whose upper index is
// >= L would change nothing, and leaving it out sorts any length exactly.  Stage k = 2, 4 .. P: one step that compares i with
// its mirror image in its block of k, then steps at distance k / 4, k / 8 .. 1.  The wave's lanes share a step's comparators,
// which touch disjoint pairs; between steps the words pass from lane to lane through memory, LDS or global alike, so each step
// ends in __syncthreads(): the workgroup is this one wave, and the call carries the workgroup-scope release and acquire fences
// that order one lane's stores before another's loads.  A comparator's lower index grows with its number t, so a lane stops
// at the first one that starts at or behind L.
template <class T, class ORDER>
__device__ __forceinline__ void sort_segment(T* w, u64 L, const ORDER& order, uint32_t key) {
  const u64 lane = threadIdx.x;
  for (uint32_t lk = 1; (1ull << (lk - 1)) < L; lk++) {     // k = 1 << lk
    const u64 half = 1ull << (lk - 1);
    for (u64 t = lane;; t += kBlock) {
      const u64 block = (t >> (lk - 1)) << lk, r = t & (half - 1);
      const u64 lo = block + r, hi = block + (2 * half - 1 - r);
      if (lo >= L) break;
      if (hi < L) put_smaller_first(w, lo, hi, order, key);
    }
    __syncthreads();
    for (uint32_t lj = lk - 1; lj-- > 0;) {                  // j = 1 << lj = k / 4 .. 1
      const u64 j = 1ull << lj;
      for (u64 t = lane;; t += kBlock) {
        const u64 lo = ((t >> lj) << (lj + 1)) | (t & (j - 1)), hi = lo + j;
        if (lo >= L) break;
        if (hi < L) put_smaller_first(w, lo, hi, order, key);
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ u64 lane_word(u64 v, uint32_t lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
  return ((u64)hi << 32) | lo;
}

}  // namespace

// Order: a wave takes 64 consecutive queries, each lane reads one's clamped bounds (lt_overlap::Sink's), and the wave sorts the
// segments longer than one element one after another: up to Span<T> elements in LDS (16 KB either way), longer ones where they
// lie.  T: int32_t, an overlap list's offsets, or uint4, a radius list's records -- or, ORDER = RayHitOrder, a hit list's, where
// the order leaves out the segments it does not take and every comparator knows the segment's ray's octant.
template <class T, class ORDER = PlainOrder<T>>
__global__ __launch_bounds__(kBlock) void lt_list_order_kernel(const u64* offsets, uint32_t n, T* items, u64 capacity, uint32_t oneShot, ORDER order) {
  __shared__ T seg[Span<T>::kWords];
  if (oneShot != 0u && offsets[n] > capacity) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t chunks = (uint32_t)(((u64)n + kBlock - 1) / kBlock);
  for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const u64 q = (u64)c * kBlock + lane;
    u64 begin = 0, length = 0;
    uint32_t key = 0u;
    if (q < n) {
      const u64 to = offsets[q + 1];
      const u64 end = to < capacity ? to : capacity;
      begin = offsets[q];
      length = end > begin ? end - begin : 0ull;
      if (length > 1ull && !order.take(q, key)) length = 0ull;
    }
    u64 todo = __builtin_amdgcn_ballot_w64(length > 1ull);
    while (todo != 0ull) {
      const uint32_t j = (uint32_t)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      const u64 L = lane_word(length, j);
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)j);
      T* const w = items + lane_word(begin, j);
      if (L <= Span<T>::kWords) {
        for (u64 i = lane; i < L; i += kBlock) seg[i] = w[i];
        __syncthreads();
        sort_segment(seg, L, order, k);
        for (u64 i = lane; i < L; i += kBlock) w[i] = seg[i];
        __syncthreads();   // (the next segment's words overwrite these)
      } else {
        sort_segment(w, L, order, k);
      }
    }
  }
}

namespace lt_overlist {

hipError_t scan(unsigned long long* offsets, uint32_t n, unsigned long long* partials, hipStream_t s) {
  const uint32_t tiles = (uint32_t)scan_partials(n);
  hipLaunchKernelGGL(lt_list_tile_sums_kernel, dim3(tiles), dim3(kScanLanes), 0, s, offsets, n, partials);
  hipLaunchKernelGGL(lt_list_scan_partials_kernel, dim3(1), dim3(kScanLanes), 0, s, partials, tiles);
  hipLaunchKernelGGL(lt_list_tile_scan_kernel, dim3(tiles), dim3(kScanLanes), 0, s, offsets, n, partials);
  return hipGetLastError();
}

namespace {

template <class T, class ORDER = PlainOrder<T>>
hipError_t order_elements(const unsigned long long* offsets, uint32_t n, T* items, unsigned long long capacity, bool oneShot, uint32_t cuCount,
                          hipStream_t s, ORDER order = ORDER{}) {
  if (n == 0) return hipSuccess;
  const uint32_t chunks = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
  // 16 KB of LDS per wave: ten waves per CU
  const uint32_t resident = cuCount * 10u;
  hipLaunchKernelGGL((lt_list_order_kernel<T, ORDER>), dim3(chunks < resident ? chunks : resident), dim3(kBlock), 0, s, offsets, n, items,
                     capacity, oneShot ? 1u : 0u, order);
  return hipGetLastError();
}

}  // namespace

hipError_t order(const unsigned long long* offsets, uint32_t n, int32_t* items, unsigned long long capacity, bool oneShot, uint32_t cuCount,
                 hipStream_t s) {
  return order_elements(offsets, n, items, capacity, oneShot, cuCount, s);
}

hipError_t order_hits(const unsigned long long* offsets, uint32_t n, uint4* items, unsigned long long capacity, bool oneShot, uint32_t cuCount,
                      hipStream_t s) {
  return order_elements(offsets, n, items, capacity, oneShot, cuCount, s);
}

hipError_t order_ray_hits(const unsigned long long* offsets, uint32_t n, uint4* items, unsigned long long capacity, bool oneShot,
                          const float4* rays, const uint32_t* rank8, uint32_t nPrims, uint32_t cuCount, hipStream_t s) {
  if (rank8 == nullptr) return hipSuccess;   // every ray walked in the reference's order and filled its segment sorted
  return order_elements(offsets, n, items, capacity, oneShot, cuCount, s, RayHitOrder{rays, rank8, nPrims});
}

}  // namespace lt_overlist
