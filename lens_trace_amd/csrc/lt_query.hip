// lt_query.hip -- ray queries over the resident scene: the kernels behind lt_hip_trace_rays / lt_hip_trace_rays_device.
//
// A query traces caller-supplied rays as the reference traces one of its own (acc.cl:132-217: `intersect`, and
// `intersectIgnorePrimitiveIndex` for a ray with ignore >= 0) from a payload {t = tmax, primitiveIndex = hitType = 0}, with
// the triangle epsilon of one of the reference's kernel files (basic.cl:77-117 compares 1e-7f in float, basic_lighting.cl:4
// 1e-7 in double, accumulator.cl:84 and the others 1e-4 in double: three instantiations).  What the reference does not do, the
// query does not do either: no t > 0 test, no tmin, `t < tmax` as given (0, negative, inf and NaN included).  Ray w components
// are the kernel's: origin.w = 1, direction.w = +0 (dot4 reads them).
//
// Which hierarchy a ray walks does not change its result (lt_retree.hpp): the walks over the backend's own tree, with the
// reference's leaf order settling equal-t ties (SceneDev::rank8), for rays the own tree takes (finite, of packet_ray_ok's
// magnitudes, a scene that has one); the caller's tree in the reference's order for the others.  Two kernels:
//   lt_query_kernel         the default: lt_trace_kernel's per-lane walk with lane refill (lt_kernel.hpp says why), reading the
//                           caller's records and keeping t;
//   lt_query_packet_kernel  LT_TRACE_FLAG_COHERENT: one wave per 64 consecutive rays, walked as one packet (packet_walk) when
//                           the 64 qualify, per lane otherwise.
// And the multi-hit queries (lt_hip_trace_hits): lt_query_hits_kernel, lt_query_kernel's loop with another leaf action -- every
// accepted primitive goes into a per-lane list sorted by t (the first K hits), or is counted.  The hit lists
// (lt_hip_trace_hits_list; lt_overlist.hpp has the four steps) are that kernel with two more sinks: the count as one uint64 per
// ray, and every accepted hit stored into the ray's segment of the CSR items.
// And the surface queries (lt_hip_surface_at; lt_hip_trace_surface is a closest-hit query and this): lt_surface_at_kernel turns hit
// records into what every `shade` of the reference computes first at a hit.  Nothing is walked.
#include "lt_query.hpp"

using namespace lt;

namespace {

constexpr int kQueryClaim = 512;   // rays a wave of lt_query_kernel claims per atomic (lt_trace_kernel's kTraceClaim)

// The result of one ray: one 16-byte store (closest hit) or one word (any hit).
template <bool ANYHIT>
__device__ __forceinline__ void put_result(const lt_query::Params& qp, uint32_t idx, const Hit& pl) {
  if (ANYHIT) qp.occluded[idx] = pl.hitType != 0 ? 1u : 0u;
  else qp.hits[idx] = make_uint4(__float_as_uint(pl.t), pl.hitType != 0 ? (uint32_t)pl.prim : 0xffffffffu, __float_as_uint(pl.u), __float_as_uint(pl.v));
}

using lt_query::finite_ray;

// A ray the own tree does not take, or any ray of a scene without one: the reference's order over the caller's tree.
template <int PROGRAM, bool ANYHIT>
__device__ __forceinline__ void walk_reference(const SceneDev& sc, const Ray& ray, float ix, float iy, float iz, int ign, Hit& pl) {
  ScratchStack ss;
  Counters c{};
  traverse_nodes_impl<PROGRAM, ScratchStack, false, false, ANYHIT, false>(sc, ray, ix, iy, iz, true, ign, pl, ss, c);
}

// The packet walk of a chunk whose 64 rays the own tree takes: false (nothing walked) for closest-hit rays of mixed octants.
template <int PROGRAM, bool ANYHIT>
__device__ __forceinline__ bool packet_query(const SceneDev& sc, const Ray& ray, float ix, float iy, float iz, int ign, Hit& pl, int* row) {
  const unsigned long long all = __builtin_amdgcn_ballot_w64(true), bx = __builtin_amdgcn_ballot_w64(ix < 0.0f),
                           by = __builtin_amdgcn_ballot_w64(iy < 0.0f), bz = __builtin_amdgcn_ballot_w64(iz < 0.0f);
  if ((bx == 0ull || bx == all) && (by == 0ull || by == all) && (bz == 0ull || bz == all)) {
    switch ((bx != 0ull ? 1 : 0) | (by != 0ull ? 2 : 0) | (bz != 0ull ? 4 : 0)) {   // one specialisation per sign octant
      case 0: packet_walk<PROGRAM, 0, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
      case 1: packet_walk<PROGRAM, 1, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
      case 2: packet_walk<PROGRAM, 2, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
      case 3: packet_walk<PROGRAM, 3, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
      case 4: packet_walk<PROGRAM, 4, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
      case 5: packet_walk<PROGRAM, 5, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
      case 6: packet_walk<PROGRAM, 6, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
      default: packet_walk<PROGRAM, 7, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, row); return true;
    }
  }
  if constexpr (ANYHIT) {
    packet_walk<PROGRAM, -1, true>(sc, ray, ix, iy, iz, ign, pl, row);   // (the sign-generic form of the walk)
    return true;
  }
  return false;
}

// ---------------------------------------------------------------------------------------------------- multi-hit queries
// The hits of one ray, nearest first: K entries {t, primitive} in the lane's column of 2 K LDS rows behind the stage (entry j:
// rows 2 j and 2 j + 1).  Only what the order needs is kept while the ray walks -- u and v are computed again for the K
// survivors when it is done (finish) -- so a wave of the K = 8 kernel takes 36 rows, not 52.  An empty entry is the miss record's
// {tmax, -1}: every accepted hit has t < tmax and sorts in front of it.  Order: t by the float `<`; equal t (-0 == +0) by the
// reference's leaf order for the ray's octant (rank8), or, for a walk that follows the reference's own order (rank8 null), behind
// what is there (insert's rank8 / octant).  An entry pushed past the end is dropped.
struct HitList {
  int* col;
  uint32_t k;
  __device__ __forceinline__ void reset(float tmax) {
    for (uint32_t j = 0; j < k; j++) { col[2 * j * kBlock] = __float_as_int(tmax); col[(2 * j + 1) * kBlock] = -1; }
  }
  __device__ __forceinline__ void insert(float tt, int prim, const uint32_t* rank8, uint32_t octant) {
    uint32_t j = k;
    while (j > 0u) {
      const float ti = __int_as_float(col[(2 * j - 2) * kBlock]);
      const int pi = col[(2 * j - 1) * kBlock];
      bool before = tt < ti;
      if (tt == ti && rank8 != nullptr && pi >= 0) before = rank8[8 * (size_t)prim + octant] < rank8[8 * (size_t)pi + octant];
      if (!before) break;
      if (j < k) { col[2 * j * kBlock] = __float_as_int(ti); col[(2 * j + 1) * kBlock] = pi; }
      j--;
    }
    if (j < k) { col[2 * j * kBlock] = __float_as_int(tt); col[(2 * j + 1) * kBlock] = prim; }
  }
  // The ray's K records: t and the primitive from the list, u and v from the triangle test run once more on the same triangle
  // from the same payload {t = tmax} -- the same function on the same operands, hence the bits the walk saw.
  template <int PROGRAM>
  __device__ __forceinline__ void finish(const SceneDev& sc, const Ray& ray, float tmax, uint4* out) const {
    for (uint32_t j = 0; j < k; j++) {
      const int tb = col[2 * j * kBlock], prim = col[(2 * j + 1) * kBlock];
      Hit trial{0, 0, tmax, 0.0f, 0.0f};
      if (prim >= 0) intersect_triangle<PROGRAM>(sc.tris, prim, ray, trial, sc.fastRcp != 0u);
      out[j] = make_uint4((uint32_t)tb, (uint32_t)prim, __float_as_uint(trial.u), __float_as_uint(trial.v));
    }
  }
};

struct HitCount {
  uint32_t n;
  __device__ __forceinline__ void operator()(float, int, float, float) { n++; }
};

// The hit lists (lt_hip_trace_hits_list): the clamped end of ray i's segment, and the records it has room for -- a length that
// would be negative is 0, so with any offsets at all no store falls outside items[0 .. capacity).
__device__ __forceinline__ unsigned long long segment_end(const lt_query::HitsParams& qp, uint32_t i) {
  const unsigned long long to = qp.offsets[(size_t)i + 1];
  return to < qp.capacity ? to : qp.capacity;
}
__device__ __forceinline__ uint32_t segment_room(const lt_query::HitsParams& qp, uint32_t i) {
  const unsigned long long begin = qp.offsets[i], to = segment_end(qp, i);
  const unsigned long long room = to > begin ? to - begin : 0ull;
  return room > 0xffffffffull ? 0xffffffffu : (uint32_t)room;
}

// The fill of a ray that walks in the reference's order: that order is the sequence's among bit-equal t, and no sort that comes
// later could know it, so the lane keeps its segment sorted while it fills it -- a stable insertion in device memory over the
// lane's own loads and stores, a hit of equal t going behind what is there, one pushed past the segment's end dropped.  Quadratic
// in the segment's length, on the path that is the slow one already.
struct HitInsert {
  uint4* seg;
  uint32_t room, filled;
  __device__ __forceinline__ void operator()(float t, int prim, float u, float v) {
    uint32_t j = filled;
    while (j > 0u) {
      const uint4 r = seg[j - 1u];
      if (!(t < __uint_as_float(r.x))) break;
      if (j < room) seg[j] = r;
      j--;
    }
    if (j < room) seg[j] = make_uint4(__float_as_uint(t), (uint32_t)prim, __float_as_uint(u), __float_as_uint(v));
    if (filled < room) filled++;
  }
};

// walk_reference for these queries: the caller's tree in the reference's order (acc.cl:132-217: near child first by
// dirIsNeg[axis], its box test compare for compare, a leaf's one primitive tested once, the ignored leaf never entered), every
// accepted triangle handed to `sink` in that order.
template <int PROGRAM, class SINK>
__device__ __forceinline__ void walk_reference_all(const SceneDev& sc, const Ray& ray, float ix, float iy, float iz, int ign, float tmax, SINK& sink) {
  const bool nx = ix < 0.0f, ny = iy < 0.0f, nz = iz < 0.0f;
  const uint32_t negBits = (nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u);
  int todo[kMaxStack];   // (set_scene refuses trees deeper than the reference's nodesToVisit[64])
  int sp = 0, cur = 0;
  for (;;) {
    const float4* n = (const float4*)((const char*)sc.nodes + ((uint32_t)cur << 5));
    const float4 a = n[0], b = n[1];
    const uint32_t meta = __float_as_uint(b.w);
    const int off = __float_as_int(b.z);
    if (box_test_reference(a.x, a.y, a.z, a.w, b.x, b.y, ray, ix, iy, iz, nx, ny, nz)) {
      if ((meta & 0xffffu) == 0u) {
        const bool neg = (negBits >> ((meta >> 16) & 0xffu)) & 1u;
        todo[sp++] = neg ? cur + 1 : off;
        cur = neg ? off : cur + 1;
        continue;
      }
      if (off != ign) {
        Hit trial{0, 0, tmax, 0.0f, 0.0f};
        if (intersect_triangle<PROGRAM>(sc.tris, off, ray, trial, sc.fastRcp != 0u)) sink(trial.t, off, trial.u, trial.v);
      }
    }
    if (sp == 0) break;
    cur = todo[--sp];
  }
}

// A ray's count: one uint32 (LT_TRACE_COUNT) or, kCountWide, one uint64 into the list's offsets.
template <int KIND>
__device__ __forceinline__ void put_hit_count(const lt_query::HitsParams& qp, uint32_t idx, uint32_t n) {
  if (KIND == lt_query::kCountWide) qp.offsets[idx] = n; else qp.counts[idx] = n;
}

}  // namespace

// lt_trace_kernel (lt_kernel.hpp) over the caller's records: waves claim rays from the eighth of the batch of the XCD they run on
// (then from the others'), 64 at a time into an LDS stage, and a lane whose ray is done takes the next staged one whenever
// `refill` lanes (or all) are idle.  Rays the own tree does not take are walked at once by the lane that drew them.
template <int PROGRAM, bool ANYHIT>
__global__ __launch_bounds__(kBlock, 8) void lt_query_kernel(SceneDev sc, lt_query::Params qp) {
  using u64 = unsigned long long;
  extern __shared__ int lds_stack[];   // [kTraceRows stack rows][kTraceStage rows of staged rays], 64 lanes each
  int* const col = lds_stack + threadIdx.x;
  int* const stage = lds_stack + kTraceRows * kBlock;
  const uint32_t total = qp.n;
  const uint32_t lane = threadIdx.x;
  const u64 below = (1ull << lane) - 1ull;
  const bool ownTree = sc.rank8 != nullptr;
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kQueryClaim ? (uint32_t)kQueryClaim : share);
  bool active = false;
  uint32_t stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;
  Ray ray{};
  float ix = 0.0f, iy = 0.0f, iz = 0.0f;
  OwnRay w{};
  Hit pl{0, 0, 0.0f, 0.0f, 0.0f};
  uint32_t idx = 0u, e = 0u;
  int sp = 0;
  int deep[kOwnRows + kOwnDeep - kTraceRows];
  for (;;) {
    const u64 idle = __builtin_amdgcn_ballot_w64(!active);
    const uint32_t nIdle = (uint32_t)__popcll(idle);
    if ((nIdle >= qp.refill || nIdle == (uint32_t)kBlock) && (stageTaken < stageCount || !drained)) {
      if (stageTaken == stageCount) {
        while (claimNext == claimEnd && sweep < 8u) {
          const uint32_t part = (home + sweep) & 7u;
          const uint32_t lo = (uint32_t)((uint64_t)total * part / 8u / kBlock * kBlock), hi = part == 7u ? total : (uint32_t)((uint64_t)total * (part + 1u) / 8u / kBlock * kBlock);
          uint32_t got = 0u;
          if (lane == 0u) got = atomicAdd(&qp.next[part * kQueueStride], claim);
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
          const float4 a = qp.rays[2 * (size_t)(base + lane)], b = qp.rays[2 * (size_t)(base + lane) + 1];
          stage[0 * kBlock + lane] = __float_as_int(a.x); stage[1 * kBlock + lane] = __float_as_int(a.y); stage[2 * kBlock + lane] = __float_as_int(a.z);
          stage[3 * kBlock + lane] = __float_as_int(b.x); stage[4 * kBlock + lane] = __float_as_int(b.y); stage[5 * kBlock + lane] = __float_as_int(b.z);
          stage[6 * kBlock + lane] = __float_as_int(b.w);   // ignore
          stage[7 * kBlock + lane] = __float_as_int(a.w);   // tmax
          stage[8 * kBlock + lane] = (int)(base + lane);
        }
        // (one wavefront per workgroup: its own LDS writes are visible to it once they have completed -- the reads below wait for them)
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = (uint32_t)__popcll(idle & below);
      if (!active && mine < take) {
        const uint32_t s = stageTaken + mine;
        idx = (uint32_t)stage[8 * kBlock + s];
        ray = Ray{mk4(__int_as_float(stage[0 * kBlock + s]), __int_as_float(stage[1 * kBlock + s]), __int_as_float(stage[2 * kBlock + s]), 1.0f),
                  mk4(__int_as_float(stage[3 * kBlock + s]), __int_as_float(stage[4 * kBlock + s]), __int_as_float(stage[5 * kBlock + s]), 0.0f)};
        const int ignRaw = stage[6 * kBlock + s];
        const int ign = ignRaw >= 0 ? ignRaw : -1;
        ix = 1.0f / ray.d.x; iy = 1.0f / ray.d.y; iz = 1.0f / ray.d.z;
        pl = Hit{0, 0, __int_as_float(stage[7 * kBlock + s]), 0.0f, 0.0f};
        if (ownTree && finite_ray(ray, ix, iy, iz) && packet_ray_ok(ray, ix, iy, iz)) {
          w = own_ray(sc, ray, ix, iy, iz, ign);
          e = 0u;
          sp = 0;
          active = true;
        } else {
          walk_reference<PROGRAM, ANYHIT>(sc, ray, ix, iy, iz, ign, pl);
          put_result<ANYHIT>(qp, idx, pl);
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
        put_result<ANYHIT>(qp, idx, pl);
        active = false;
      }
    }
  }
}

// LT_TRACE_FLAG_COHERENT: workgroup b takes rays [64 b, 64 b + 64).  They walk as ONE packet when every one of them is finite and
// passes packet_ray_ok on a scene with an own tree, and -- closest hit -- they share a direction-sign octant (the leaf order that
// settles ties is the octant's) and none ignores a primitive (the closest-hit packet walk applies no `ignore`); any-hit rays of
// mixed octants take the sign-generic packet walk.  Otherwise each lane walks its own ray.  Lanes past the end of the batch walk a
// copy of the chunk's first ray and store nothing, so that every walk runs with the whole wave.
template <int PROGRAM, bool ANYHIT>
__global__ __launch_bounds__(kBlock, 8) void lt_query_packet_kernel(SceneDev sc, lt_query::Params qp) {
  extern __shared__ int lds_stack[];   // kOwnRows rows: the per-lane walks' stacks; the packet walks use the first two
  const uint32_t base = blockIdx.x * (uint32_t)kBlock;
  const uint32_t idx = base + threadIdx.x;
  const bool valid = idx < qp.n;
  const size_t src = valid ? idx : base;
  const float4 a = qp.rays[2 * src], b = qp.rays[2 * src + 1];
  const Ray ray{mk4(a.x, a.y, a.z, 1.0f), mk4(b.x, b.y, b.z, 0.0f)};
  const int ignRaw = __float_as_int(b.w);
  const int ign = ignRaw >= 0 ? ignRaw : -1;
  const float ix = 1.0f / ray.d.x, iy = 1.0f / ray.d.y, iz = 1.0f / ray.d.z;
  Hit pl{0, 0, a.w, 0.0f, 0.0f};
  const bool ownOk = sc.rank8 != nullptr && finite_ray(ray, ix, iy, iz) && packet_ray_ok(ray, ix, iy, iz);
  if (!(__all(ownOk) && (ANYHIT || __all(ign < 0)) && packet_query<PROGRAM, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, lds_stack))) {
    if (ownOk) traverse_own_lane<PROGRAM, ANYHIT>(sc, ray, ix, iy, iz, ign, pl, lds_stack + threadIdx.x);
    else walk_reference<PROGRAM, ANYHIT>(sc, ray, ix, iy, iz, ign, pl);
  }
  if (valid) put_result<ANYHIT>(qp, idx, pl);
}

// lt_query_kernel's claim, stage and refill loop with the multi-hit leaf action (own_walk_step_all): COUNT counts a ray's accepted
// primitives in a register; kFirstK puts them into the lane's HitList of qp.maxHits entries, 2 maxHits LDS rows behind the stage,
// which the lane resets when it takes a new ray -- its neighbours' lists stay as they are -- and writes out when its walk is done.
// The hit lists (lt_hip_trace_hits_list) are two more sinks, neither with LDS list rows, so their layout and occupancy are the
// count's: kCountWide is the count stored as one uint64 into offsets[idx]; kList stores each accepted hit {t, prim, u, v} -- u and v
// arrive with it -- behind the last in the ray's segment while records are left of it (`left`; the segment's end is read again
// beside the store, lt_nearest.hip's ListSink says why), or, for a ray that walks in the reference's order, by HitInsert.
template <int PROGRAM, int KIND>
__global__ __launch_bounds__(kBlock, 8) void lt_query_hits_kernel(SceneDev sc, lt_query::HitsParams qp) {
  using u64 = unsigned long long;
  constexpr bool COUNT = KIND == lt_query::kCount || KIND == lt_query::kCountWide, LIST = KIND == lt_query::kList;
  extern __shared__ int lds_stack[];   // [kTraceRows stack rows][kTraceStage rows of staged rays][2 maxHits list rows], 64 lanes each
  if (LIST && qp.oneShot != 0u && qp.offsets[qp.n] > qp.capacity) return;   // (every lane reads the same word)
  int* const col = lds_stack + threadIdx.x;
  int* const stage = lds_stack + kTraceRows * kBlock;
  const uint32_t total = qp.n;
  const uint32_t lane = threadIdx.x;
  const u64 below = (1ull << lane) - 1ull;
  const bool ownTree = sc.rank8 != nullptr;
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kQueryClaim ? (uint32_t)kQueryClaim : share);
  bool active = false;
  uint32_t stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;
  Ray ray{};
  float ix = 0.0f, iy = 0.0f, iz = 0.0f, tmax = 0.0f;
  OwnRay w{};
  HitList list{lds_stack + (kTraceRows + kTraceStage) * kBlock + threadIdx.x, COUNT || LIST ? 0u : qp.maxHits};
  HitCount count{0u};
  uint32_t idx = 0u, e = 0u, left = 0u;
  auto ranked = [&](float t, int prim, float, float) { list.insert(t, prim, sc.rank8, w.octant); };   // the own tree's order is not the reference's
  auto inOrder = [&](float t, int prim, float, float) { list.insert(t, prim, nullptr, 0u); };
  auto behind = [&](float t, int prim, float u, float v) {   // kList, the own walk: its order is left to the ordering kernel
    if (left != 0u) {
      const u64 to = segment_end(qp, idx);
      // (left <= to holds while the offsets are what the lane read when it took the ray; were they changed under the launch, the store is dropped)
      if (left <= to) qp.items[to - left] = make_uint4(__float_as_uint(t), (uint32_t)prim, __float_as_uint(u), __float_as_uint(v));
      left--;
    }
  };
  int sp = 0;
  int deep[kOwnRows + kOwnDeep - kTraceRows];
  for (;;) {
    const u64 idle = __builtin_amdgcn_ballot_w64(!active);
    const uint32_t nIdle = (uint32_t)__popcll(idle);
    if ((nIdle >= qp.refill || nIdle == (uint32_t)kBlock) && (stageTaken < stageCount || !drained)) {
      if (stageTaken == stageCount) {
        while (claimNext == claimEnd && sweep < 8u) {
          const uint32_t part = (home + sweep) & 7u;
          const uint32_t lo = (uint32_t)((uint64_t)total * part / 8u / kBlock * kBlock), hi = part == 7u ? total : (uint32_t)((uint64_t)total * (part + 1u) / 8u / kBlock * kBlock);
          uint32_t got = 0u;
          if (lane == 0u) got = atomicAdd(&qp.next[part * kQueueStride], claim);
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
        if (lane < batch) {
          const float4 a = qp.rays[2 * (size_t)(base + lane)], b = qp.rays[2 * (size_t)(base + lane) + 1];
          stage[0 * kBlock + lane] = __float_as_int(a.x); stage[1 * kBlock + lane] = __float_as_int(a.y); stage[2 * kBlock + lane] = __float_as_int(a.z);
          stage[3 * kBlock + lane] = __float_as_int(b.x); stage[4 * kBlock + lane] = __float_as_int(b.y); stage[5 * kBlock + lane] = __float_as_int(b.z);
          stage[6 * kBlock + lane] = __float_as_int(b.w);   // ignore
          stage[7 * kBlock + lane] = __float_as_int(a.w);   // tmax
          stage[8 * kBlock + lane] = (int)(base + lane);
        }
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = (uint32_t)__popcll(idle & below);
      if (!active && mine < take) {
        const uint32_t s = stageTaken + mine;
        idx = (uint32_t)stage[8 * kBlock + s];
        ray = Ray{mk4(__int_as_float(stage[0 * kBlock + s]), __int_as_float(stage[1 * kBlock + s]), __int_as_float(stage[2 * kBlock + s]), 1.0f),
                  mk4(__int_as_float(stage[3 * kBlock + s]), __int_as_float(stage[4 * kBlock + s]), __int_as_float(stage[5 * kBlock + s]), 0.0f)};
        const int ignRaw = stage[6 * kBlock + s];
        const int ign = ignRaw >= 0 ? ignRaw : -1;
        ix = 1.0f / ray.d.x; iy = 1.0f / ray.d.y; iz = 1.0f / ray.d.z;
        tmax = __int_as_float(stage[7 * kBlock + s]);
        if (COUNT) count.n = 0u; else if (LIST) left = segment_room(qp, idx); else list.reset(tmax);
        if (ownTree && finite_ray(ray, ix, iy, iz) && packet_ray_ok(ray, ix, iy, iz)) {
          w = own_ray(sc, ray, ix, iy, iz, ign);
          e = 0u;
          sp = 0;
          active = true;
        } else {
          if (COUNT) {
            walk_reference_all<PROGRAM>(sc, ray, ix, iy, iz, ign, tmax, count);
            put_hit_count<KIND>(qp, idx, count.n);
          } else if (LIST) {
            HitInsert sorted{qp.items + qp.offsets[idx], left, 0u};
            walk_reference_all<PROGRAM>(sc, ray, ix, iy, iz, ign, tmax, sorted);
          } else {
            walk_reference_all<PROGRAM>(sc, ray, ix, iy, iz, ign, tmax, inOrder);
            list.template finish<PROGRAM>(sc, ray, tmax, qp.hits + (size_t)idx * qp.maxHits);
          }
        }
      }
      stageTaken += take;
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
      if (drained && stageTaken == stageCount) break;
      continue;
    }
    if (active) {
      const bool done = COUNT  ? own_walk_step_all<PROGRAM, kTraceRows>(sc, ray, ix, iy, iz, w, tmax, count, col, deep, e, sp)
                        : LIST ? own_walk_step_all<PROGRAM, kTraceRows>(sc, ray, ix, iy, iz, w, tmax, behind, col, deep, e, sp)
                               : own_walk_step_all<PROGRAM, kTraceRows>(sc, ray, ix, iy, iz, w, tmax, ranked, col, deep, e, sp);
      if (done) {
        if (COUNT) put_hit_count<KIND>(qp, idx, count.n);
        else if (!LIST) list.template finish<PROGRAM>(sc, ray, tmax, qp.hits + (size_t)idx * qp.maxHits);
        active = false;
      }
    }
  }
}

// lt_hip_surface from lt_hip_hit: one record per lane -- a 16-byte load, the primitive's 76 bytes gathered, three 16-byte stores --
// in a grid-stride loop.  The reference's own steps (acc.cl:233-247): the primitive, b = (1.0 - u - v in double, u, v),
// A*b.x + B*b.y + C*b.z of the positions and of the normals -- as shipped (Math<2>: fused) or with every product and sum rounded
// (strict and portable: bary3 knows no other difference) --, the material, the scan of the light list.  A primitive that is none of
// the scene's (one unsigned compare: -1 included) gives the miss form.
template <bool SHIPPED>
__global__ __launch_bounds__(256) void lt_surface_at_kernel(SceneDev sc, const uint4* __restrict__ hits, uint4* __restrict__ out, uint32_t n) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint4 hit = hits[i];
    uint4 pos = make_uint4(0u, 0u, 0u, 0xffffffffu), nrm = make_uint4(0u, 0u, 0u, 0u);
    if (hit.y >= sc.n_prims) {
      hit = make_uint4(hit.x, 0xffffffffu, 0u, 0u);
    } else {
      const int prim = (int)hit.y;
      const float* pr = prim_ptr(sc, prim);
      const V3 b = barycentrics(__uint_as_float(hit.z), __uint_as_float(hit.w));
      const V3 p3 = bary3<SHIPPED ? 2 : 0>(pr + 0, pr + 3, pr + 6, b);
      const V3 n3 = bary3<SHIPPED ? 2 : 0>(pr + 9, pr + 12, pr + 15, b);
      pos = make_uint4(__float_as_uint(p3.x), __float_as_uint(p3.y), __float_as_uint(p3.z), (uint32_t)prim_material(pr));
      nrm = make_uint4(__float_as_uint(n3.x), __float_as_uint(n3.y), __float_as_uint(n3.z), is_light(sc.lights, prim) ? 1u : 0u);
    }
    uint4* const o = out + 3 * (size_t)i;
    o[0] = hit;
    o[1] = pos;
    o[2] = nrm;
    if (n - i <= stride) break;   // (i + stride may wrap: n goes up to 2^32 - 1)
  }
}

namespace lt_query {

template <int PROGRAM, bool ANYHIT>
static void launch_one(const SceneDev& sc, const Params& p, bool coherent, uint32_t cuCount, hipStream_t s) {
  const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);
  if (coherent) {
    hipLaunchKernelGGL((lt_query_packet_kernel<PROGRAM, ANYHIT>), dim3(chunks), dim3(kBlock), (uint32_t)(kOwnRows * kBlock * sizeof(int)), s, sc, p);
  } else {
    const uint32_t resident = cuCount * 32u;   // every wave slot of the chip, once
    hipLaunchKernelGGL((lt_query_kernel<PROGRAM, ANYHIT>), dim3(chunks < resident ? chunks : resident), dim3(kBlock),
                       (uint32_t)((kTraceRows + kTraceStage) * kBlock * sizeof(int)), s, sc, p);
  }
}

hipError_t launch(const SceneDev& sc, const Params& p, Epsilon eps, bool anyHit, bool coherent, uint32_t cuCount, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (!coherent) {
    const hipError_t e = hipMemsetAsync(p.next, 0, 8 * kQueueStride * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
  }
  switch (eps) {
    case kEpsFloat7: anyHit ? launch_one<kBasic, true>(sc, p, coherent, cuCount, s) : launch_one<kBasic, false>(sc, p, coherent, cuCount, s); break;
    case kEpsDouble7:
      anyHit ? launch_one<kBasicLighting, true>(sc, p, coherent, cuCount, s) : launch_one<kBasicLighting, false>(sc, p, coherent, cuCount, s);
      break;
    default:
      anyHit ? launch_one<kAccumulator, true>(sc, p, coherent, cuCount, s) : launch_one<kAccumulator, false>(sc, p, coherent, cuCount, s);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_surface_at(const SceneDev& sc, const uint4* hits, uint4* out, uint32_t n, bool shipped, uint32_t cuCount, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t blocks = (uint32_t)(((uint64_t)n + 255u) / 256u), resident = cuCount * 8u;   // 2048 lanes per CU
  const dim3 grid(blocks < resident ? blocks : resident);
  if (shipped) hipLaunchKernelGGL((lt_surface_at_kernel<true>), grid, dim3(256), 0, s, sc, hits, out, n);
  else hipLaunchKernelGGL((lt_surface_at_kernel<false>), grid, dim3(256), 0, s, sc, hits, out, n);
  return hipGetLastError();
}

template <int PROGRAM>
static void launch_hits_one(const SceneDev& sc, const HitsParams& p, uint32_t cuCount, hipStream_t s) {
  const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);
  const uint32_t rows = (uint32_t)(kTraceRows + kTraceStage) + 2u * p.maxHits;
  // every wave slot the list rows leave: 160 KB of LDS per CU, at most 32 waves
  const uint32_t fit = 160u * 1024u / (rows * kBlock * (uint32_t)sizeof(int)), perCu = fit < 32u ? fit : 32u;
  const uint32_t resident = cuCount * perCu;
  const dim3 grid(chunks < resident ? chunks : resident);
  const uint32_t bytes = rows * kBlock * (uint32_t)sizeof(int);
  if (p.kind == (uint32_t)kCount) hipLaunchKernelGGL((lt_query_hits_kernel<PROGRAM, kCount>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kCountWide) hipLaunchKernelGGL((lt_query_hits_kernel<PROGRAM, kCountWide>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kList) hipLaunchKernelGGL((lt_query_hits_kernel<PROGRAM, kList>), grid, dim3(kBlock), bytes, s, sc, p);
  else hipLaunchKernelGGL((lt_query_hits_kernel<PROGRAM, kFirstK>), grid, dim3(kBlock), bytes, s, sc, p);
}

hipError_t launch_hits(const SceneDev& sc, const HitsParams& p, Epsilon eps, uint32_t cuCount, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (p.kind > (uint32_t)kList || p.maxHits > kMaxHits || (p.kind == (uint32_t)kFirstK) != (p.maxHits != 0u)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(p.next, 0, 8 * kQueueStride * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  switch (eps) {
    case kEpsFloat7: launch_hits_one<kBasic>(sc, p, cuCount, s); break;
    case kEpsDouble7: launch_hits_one<kBasicLighting>(sc, p, cuCount, s); break;
    default: launch_hits_one<kAccumulator>(sc, p, cuCount, s); break;
  }
  return hipGetLastError();
}

}  // namespace lt_query
