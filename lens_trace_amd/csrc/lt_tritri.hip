// lt_tritri.hip -- triangle-overlap queries over the resident scene: the kernels behind lt_hip_overlap_tris /
// lt_hip_overlap_tris_device.  For each query triangle: the candidates (a leaf of the caller's tree with its one primitive) that
// touch it -- the leaf's own box meets the query's box and none of the 17 axes of lt_tritri.hpp separates the two triangles --
// as the first K primitive offsets in ascending order, as their number, or as "any".  The answer is a function of the scene and
// the query alone and the walk only has to find it.  The overlap lists (lt_overlist.hpp) run the same kernels with the sinks
// kCountWide and kList of lt_overlap.hpp.
//
// The walk is lt_overlap_kernel's (lt_overlap.hip): depth-first over the per-lane walks' records, a group's four child slots put
// back on the grid (slot_box) and tested against the query's box with boxes_meet, links only on the stack.  Nothing is dropped
// that could hold a touching leaf: touching requires boxes_meet on the leaf's own box, a slot's box encloses every leaf box
// beneath it as floats and boxes_meet is monotone in enclosure.  A lane holds the query's box in registers and
// the query's own terms (P, h_j, m) in LDS rows, computed once per query; the 17 axes are one rolled loop over those rows and the
// scene triangle's, put beside them at each leaf.  A scene without an own tree is
// scanned leaf by leaf in the caller's node order, by a kernel of its own.
#include "lt_tritri.hpp"

using namespace lt;
using lt_tritri::Vec;

namespace {

constexpr int kTtClaim = 512;       // queries a wave claims per atomic (lt_overlap_kernel's kOvClaim)
constexpr int kTtEntries = 12;      // stack entries per lane in LDS, one row each (the link) ...
constexpr int kTtDeep = kOwnRows + kOwnDeep - kTtEntries;   // ... and the entries beyond them, in private memory
constexpr int kTtQuery = 3 * lt_tritri::kRows;   // rows of the lanes' tables of operands (lt_tritri.hpp): 27

struct Grid { float O[3], S[3]; };   // the 16-bit grid of the group slots (wide[-2], wide[-1])
// A lane's query: its box in registers, for the slot tests, and lt_tritri.hpp's table of the test's operands in the lane's column
// of kTtQuery LDS rows -- the query's own terms put when the lane takes the query, the scene triangle's at each leaf.
struct Query {
  float lo[3], hi[3];
  int* rows;
  __device__ __forceinline__ Vec row(int v) const {
    return Vec{__int_as_float(rows[(3 * v) * kBlock]), __int_as_float(rows[(3 * v + 1) * kBlock]), __int_as_float(rows[(3 * v + 2) * kBlock])};
  }
  __device__ __forceinline__ void put(int v, const Vec& a) {
    rows[(3 * v) * kBlock] = __float_as_int(a.x); rows[(3 * v + 1) * kBlock] = __float_as_int(a.y); rows[(3 * v + 2) * kBlock] = __float_as_int(a.z);
  }
  // Takes the caller's record: false when the query is empty.
  __device__ __forceinline__ bool take(const float4* rec) {
    const float4 a = rec[0], b = rec[1], c = rec[2];   // three 16-byte loads, the pads ignored
    const Vec P{a.x, a.y, a.z}, Q{b.x, b.y, b.z}, R{c.x, c.y, c.z};
    if (lt_tritri::empty_tri(P, Q, R)) return false;
    lt_tritri::query_box(P, Q, R, lo, hi);
    lt_tritri::put_query(*this, P, Q, R);
    return true;
  }
};

using lt_overlap::Sink;          // what takes a query's touching candidates (lt_overlap.hpp)
using lt_overlap::put_overlap;

__device__ __forceinline__ bool meets_query_box(const Query& q, float blx, float bly, float blz, float bhx, float bhy, float bhz) {
  return lt_overlap::boxes_meet(q.lo[0], q.lo[1], q.lo[2], q.hi[0], q.hi[1], q.hi[2], blx, bly, blz, bhx, bhy, bhz);
}

__device__ __forceinline__ bool leaf_meets(Query& q, Vec A, Vec e1, Vec e2) {
  return lt_tritri::tri_meets_tri(q, A, e1, e2);
}

// One step of the walk for one lane: the record `e` (a group, or a leaf: bit 31) is fetched and dealt with, the next entry popped
// into `e`.  Returns true when the walk is over: the stack is empty or, kAny, a candidate touched.
template <int KIND>
__device__ __forceinline__ bool tris_step(const SceneDev& sc, uint32_t emptyLink, Query& q, Sink<KIND>& sink, int* col, int* deep, uint32_t& e,
                                          int& sp) {
  const uint4* rec = (const uint4*)((const char*)sc.wide + ((size_t)(e & 0x7fffffffu) << 6));
  const uint4 s0 = rec[0], s1 = rec[1], s2 = rec[2], s3 = rec[3];
  int32_t touched = -1;   // (the sink takes it behind the test, as in lt_overlap.hip)
  if ((int)e < 0) {   // a leaf: A e1.x | e1.yz e2.xy | e2.z lo | hi prim
    if (meets_query_box(q, __uint_as_float(s2.y), __uint_as_float(s2.z), __uint_as_float(s2.w), __uint_as_float(s3.x), __uint_as_float(s3.y),
                        __uint_as_float(s3.z)) &&
        leaf_meets(q, Vec{__uint_as_float(s0.x), __uint_as_float(s0.y), __uint_as_float(s0.z)},
                   Vec{__uint_as_float(s0.w), __uint_as_float(s1.x), __uint_as_float(s1.y)},
                   Vec{__uint_as_float(s1.z), __uint_as_float(s1.w), __uint_as_float(s2.x)}))
      touched = (int32_t)s3.w;
  } else {
    // the slots whose box meets the query's (an empty slot's link is the record behind the last primitive's: never entered)
    const F8v fr = *(ConstF8)((unsigned long long)sc.wide - 32ull);   // origin.xyz - step.xyz -
    const Grid g{{fr.s0, fr.s1, fr.s2}, {fr.s4, fr.s5, fr.s6}};
    const uint4 slot[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int k = 3; k >= 0; k--) {
      float lo[3], hi[3];
      lt_overlap::slot_box(slot[k].x, slot[k].y, slot[k].z, g.O, g.S, lo, hi);
      if (slot[k].w != emptyLink && meets_query_box(q, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])) {
        if (sp < kTtEntries) col[sp * kBlock] = (int)slot[k].w;
        else deep[sp - kTtEntries] = (int)slot[k].w;
        sp++;
      }
    }
  }
  if (touched >= 0) {
    sink.touch(touched);
    if (KIND == lt_overlap::kAny) return true;
  }
  if (sp == 0) return true;
  sp--;
  e = (uint32_t)(sp < kTtEntries ? col[sp * kBlock] : deep[sp - kTtEntries]);
  return false;
}

// A scene without an own tree: every leaf of the caller's node array in index order.
template <int KIND>
__device__ __forceinline__ void tris_scan(const SceneDev& sc, Query& q, Sink<KIND>& sink) {
  for (uint32_t i = 0; i < sc.n_nodes; i++) {
    const float4 a = sc.nodes[2 * (size_t)i], b = sc.nodes[2 * (size_t)i + 1];
    if ((__float_as_uint(b.w) & 0xffffu) == 0u) continue;
    if (!meets_query_box(q, a.x, a.y, a.z, a.w, b.x, b.y)) continue;
    const int32_t prim = __float_as_int(b.z);
    const float4 t0 = sc.tris[3 * (size_t)prim], t1 = sc.tris[3 * (size_t)prim + 1], t2 = sc.tris[3 * (size_t)prim + 2];
    if (leaf_meets(q, Vec{t0.x, t0.y, t0.z}, Vec{t0.w, t1.x, t1.y}, Vec{t1.z, t1.w, t2.x})) {
      sink.touch(prim);
      if (KIND == lt_overlap::kAny) return;
    }
  }
}

}  // namespace

// lt_overlap_kernel's claim, stage and refill loop over query triangles: waves claim queries from the eighth of the batch of the
// XCD they run on (then from the others'), stage 64 at a time, and a lane whose query is done takes the next staged one whenever
// `refill` lanes (or all) are idle.  The stage is a range of indices and no copy: lanes that take together take consecutive
// records, so each reads its own from the caller's array (three 16-byte loads that coalesce), keeps the box in registers and puts
// the query's own terms into its column of kTtQuery LDS rows -- a staged copy would be ten more rows per wave beside those.  Empty
// queries (lt_tritri::empty_tri) are answered at once by the lane that drew them.  kFirstK: the lane's list is qp.maxK LDS rows
// behind the table.  A step pops one stack entry and pushes at most four, so kOwnRows + kOwnDeep entries suffice.
template <int KIND>
__global__ __launch_bounds__(kBlock, 8) void lt_overlap_tris_kernel(SceneDev sc, lt_overlap::Params qp) {
  using u64 = unsigned long long;
  extern __shared__ int lds_stack[];   // [kTtEntries stack rows][kTtQuery rows of the test's operands][maxK list rows], 64 lanes each
  if (lt_overlap::list_overflows<KIND>(qp)) return;
  int* const col = lds_stack + threadIdx.x;
  const uint32_t total = qp.n;
  const uint32_t lane = threadIdx.x;
  const uint32_t emptyLink = 0x80000000u | (sc.nWide + sc.n_prims);
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kTtClaim ? (uint32_t)kTtClaim : share);
  bool active = false;
  uint32_t stageBase = 0u, stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;
  Query q{{}, {}, col + kTtEntries * kBlock};
  Sink<KIND> sink{{col + (kTtEntries + kTtQuery) * kBlock, KIND == lt_overlap::kFirstK ? qp.maxK : 0u}, -1, 0u};
  uint32_t idx = 0u, e = 0u;
  int sp = 0;
  int deep[kTtDeep];
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
        stageBase = claimNext;
        const uint32_t batch = claimEnd - stageBase < (uint32_t)kBlock ? claimEnd - stageBase : (uint32_t)kBlock;
        claimNext = stageBase + batch;   // (<= claimEnd <= total: every index taken below names a record of the batch)
        drained = claimNext == claimEnd && sweep >= 8u;
        stageTaken = 0u;
        stageCount = batch;
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));   // idle lanes below this one
      if (!active && mine < take) {
        idx = stageBase + stageTaken + mine;
        sink.reset(qp, idx);
        if (!q.take(qp.boxes + 3 * (size_t)idx)) {
          put_overlap(qp, idx, sink);
        } else {
          e = 0u;   // the root's group
          sp = 0;
          active = true;
        }
      }
      stageTaken += take;
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
      if (drained && stageTaken == stageCount) break;
      continue;
    }
    if (active) {
      if (tris_step(sc, emptyLink, q, sink, col, deep, e, sp)) {
        put_overlap(qp, idx, sink);
        active = false;
      }
    }
  }
}

// A scene without an own tree (boxes that do not nest, bounds >= 2^40): each lane scans the caller's leaves for its queries --
// slow, correct, and only for the scenes that already fall back.  The lane's table of operands is its column of kTtQuery LDS rows and,
// kFirstK, its list the qp.maxK rows behind them.
template <int KIND>
__global__ __launch_bounds__(kBlock, 8) void lt_overlap_tris_scan_kernel(SceneDev sc, lt_overlap::Params qp) {
  extern __shared__ int lds_stack[];   // [kTtQuery rows of the test's operands][maxK list rows], 64 lanes each
  if (lt_overlap::list_overflows<KIND>(qp)) return;
  Query q{{}, {}, lds_stack + threadIdx.x};
  Sink<KIND> sink{{lds_stack + kTtQuery * kBlock + threadIdx.x, KIND == lt_overlap::kFirstK ? qp.maxK : 0u}, -1, 0u};
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < qp.n; i += (uint64_t)gridDim.x * kBlock) {
    sink.reset(qp, (uint32_t)i);
    if (q.take(qp.boxes + 3 * (size_t)i)) tris_scan(sc, q, sink);
    put_overlap(qp, (uint32_t)i, sink);
  }
}

namespace lt_tritri {

using lt_overlap::kAny;
using lt_overlap::kCount;
using lt_overlap::kCountWide;
using lt_overlap::kFirstK;
using lt_overlap::kList;

hipError_t launch(const SceneDev& sc, const lt_overlap::Params& p, uint32_t cuCount, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (p.kind > (uint32_t)kCountWide || p.maxK > lt_overlap::kMaxK || (p.kind == (uint32_t)kFirstK) != (p.maxK != 0u)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(p.next, 0, 8 * kQueueStride * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);
  const uint32_t rows = (uint32_t)(kTtEntries + kTtQuery) + p.maxK;
  // every wave slot the rows leave: 160 KB of LDS per CU (39 rows: 16 waves; with eight list rows 13)
  const uint32_t bytes = rows * kBlock * (uint32_t)sizeof(int);
  const uint32_t fit = 160u * 1024u / bytes, perCu = fit < 32u ? fit : 32u;
  const uint32_t resident = cuCount * perCu;
  const dim3 grid(chunks < resident ? chunks : resident);
  if (sc.wide == nullptr || sc.rank8 == nullptr) {   // no own tree
    const dim3 all(chunks < cuCount * 32u ? chunks : cuCount * 32u);
    const uint32_t list = ((uint32_t)kTtQuery + p.maxK) * kBlock * (uint32_t)sizeof(int);
    if (p.kind == (uint32_t)kFirstK) hipLaunchKernelGGL((lt_overlap_tris_scan_kernel<kFirstK>), all, dim3(kBlock), list, s, sc, p);
    else if (p.kind == (uint32_t)kCount) hipLaunchKernelGGL((lt_overlap_tris_scan_kernel<kCount>), all, dim3(kBlock), list, s, sc, p);
    else if (p.kind == (uint32_t)kList) hipLaunchKernelGGL((lt_overlap_tris_scan_kernel<kList>), all, dim3(kBlock), list, s, sc, p);
    else if (p.kind == (uint32_t)kCountWide) hipLaunchKernelGGL((lt_overlap_tris_scan_kernel<kCountWide>), all, dim3(kBlock), list, s, sc, p);
    else hipLaunchKernelGGL((lt_overlap_tris_scan_kernel<kAny>), all, dim3(kBlock), list, s, sc, p);
    return hipGetLastError();
  }
  if (p.kind == (uint32_t)kFirstK) hipLaunchKernelGGL((lt_overlap_tris_kernel<kFirstK>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kCount) hipLaunchKernelGGL((lt_overlap_tris_kernel<kCount>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kList) hipLaunchKernelGGL((lt_overlap_tris_kernel<kList>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kCountWide) hipLaunchKernelGGL((lt_overlap_tris_kernel<kCountWide>), grid, dim3(kBlock), bytes, s, sc, p);
  else hipLaunchKernelGGL((lt_overlap_tris_kernel<kAny>), grid, dim3(kBlock), bytes, s, sc, p);
  return hipGetLastError();
}

}  // namespace lt_tritri
