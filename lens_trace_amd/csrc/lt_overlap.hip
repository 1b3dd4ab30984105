// lt_overlap.hip -- box-overlap queries over the resident scene: the kernel behind lt_hip_overlap_boxes /
// lt_hip_overlap_boxes_device.  For each box: the candidates (a leaf of the caller's tree with its one primitive) that touch it --
// the leaf's own box meets the box and the traversal triangle passes the 13-axis test, both as lt_overlap.hpp defines them -- as
// the first K primitive offsets in ascending order, as their number, or as "any".  The answer is a function of the scene and
// the box alone and the walk only has to find it.  The overlap lists (lt_overlist.hpp) run the same kernels with two more sinks:
// the number as uint64 (kCountWide) and every offset into the box's segment of a CSR array (kList).
//
// The walk is depth-first over the per-lane walks' records (SceneDev::wide): a group's four child slots are put back on the grid
// (slot_box) and the ones that meet the box go on the lane's stack, links only.  A leaf record holds the triangle, the leaf's own
// box and the offset.  Nothing is dropped that could hold a touching leaf: a slot's box encloses every leaf box beneath it as
// floats and boxes_meet is monotone in enclosure, without margins.  A scene without an own tree is scanned leaf
// by leaf in the caller's node order, by a kernel of its own (lt_overlap_scan_kernel).
#include "lt_overlap.hpp"

using namespace lt;

namespace {

constexpr int kOvClaim = 512;       // boxes a wave claims per atomic (lt_nearest_kernel's kNearClaim)
constexpr int kOvEntries = 12;      // stack entries per lane in LDS, one row each (the link) ...
constexpr int kOvDeep = kOwnRows + kOwnDeep - kOvEntries;   // ... and the entries beyond them, in private memory
constexpr int kOvStage = 7;         // rows of staged boxes (lo.xyz, hi.xyz, index): 19 rows = 4.75 KB, 32 waves per CU

struct Grid { float O[3], S[3]; };   // the 16-bit grid of the group slots (wide[-2], wide[-1])
struct Box { float lo[3], hi[3]; };

using lt_overlap::Sink;          // what takes a box's touching candidates (lt_overlap.hpp)
using lt_overlap::put_overlap;

// Whether the candidate of a leaf -- its own box, its traversal triangle -- touches q.
__device__ __forceinline__ bool leaf_touches(const Box& q, float ax, float ay, float az, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z,
                                             float blx, float bly, float blz, float bhx, float bhy, float bhz) {
  if (!lt_overlap::boxes_meet(q.lo[0], q.lo[1], q.lo[2], q.hi[0], q.hi[1], q.hi[2], blx, bly, blz, bhx, bhy, bhz)) return false;
  const float A[3] = {ax, ay, az}, e1[3] = {e1x, e1y, e1z}, e2[3] = {e2x, e2y, e2z};
  return lt_overlap::tri_meets_box(q.lo, q.hi, A, e1, e2);
}

// One step of the walk for one lane: the record `e` (a group, or a leaf: bit 31) is fetched and dealt with, the next entry popped
// into `e`.  Returns true when the walk is over: the stack is empty or, kAny, a candidate touched.
template <int KIND>
__device__ __forceinline__ bool overlap_step(const SceneDev& sc, uint32_t emptyLink, const Box& q, Sink<KIND>& sink, int* col, int* deep,
                                             uint32_t& e, int& sp) {
  const uint4* rec = (const uint4*)((const char*)sc.wide + ((size_t)(e & 0x7fffffffu) << 6));
  const uint4 s0 = rec[0], s1 = rec[1], s2 = rec[2], s3 = rec[3];
  int32_t touched = -1;   // (the sink takes it behind the test, not inside it: the list's insertion then sits outside the test's branches)
  if ((int)e < 0) {   // a leaf: A e1.x | e1.yz e2.xy | e2.z lo | hi prim
    if (leaf_touches(q, __uint_as_float(s0.x), __uint_as_float(s0.y), __uint_as_float(s0.z), __uint_as_float(s0.w), __uint_as_float(s1.x),
                     __uint_as_float(s1.y), __uint_as_float(s1.z), __uint_as_float(s1.w), __uint_as_float(s2.x), __uint_as_float(s2.y),
                     __uint_as_float(s2.z), __uint_as_float(s2.w), __uint_as_float(s3.x), __uint_as_float(s3.y), __uint_as_float(s3.z)))
      touched = (int32_t)s3.w;
  } else {
    // the slots whose box meets q (an empty slot's link is the record behind the last primitive's: never entered)
    // (the grid comes from the scalar cache at every group, beside the record's own load: held across the leaf test instead, its
    // six words are six more wave-uniform registers parked in the lanes of a vector register the test needs)
    const F8v fr = *(ConstF8)((unsigned long long)sc.wide - 32ull);   // origin.xyz - step.xyz -
    const Grid g{{fr.s0, fr.s1, fr.s2}, {fr.s4, fr.s5, fr.s6}};
    const uint4 slot[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int k = 3; k >= 0; k--) {
      float lo[3], hi[3];
      lt_overlap::slot_box(slot[k].x, slot[k].y, slot[k].z, g.O, g.S, lo, hi);
      if (slot[k].w != emptyLink && lt_overlap::boxes_meet(q.lo[0], q.lo[1], q.lo[2], q.hi[0], q.hi[1], q.hi[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])) {
        if (sp < kOvEntries) col[sp * kBlock] = (int)slot[k].w;
        else deep[sp - kOvEntries] = (int)slot[k].w;
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
  e = (uint32_t)(sp < kOvEntries ? col[sp * kBlock] : deep[sp - kOvEntries]);
  return false;
}

// A scene without an own tree: every leaf of the caller's node array in index order.
template <int KIND>
__device__ __forceinline__ void overlap_scan(const SceneDev& sc, const Box& q, Sink<KIND>& sink) {
  for (uint32_t i = 0; i < sc.n_nodes; i++) {
    const float4 a = sc.nodes[2 * (size_t)i], b = sc.nodes[2 * (size_t)i + 1];
    if ((__float_as_uint(b.w) & 0xffffu) == 0u) continue;
    if (!lt_overlap::boxes_meet(q.lo[0], q.lo[1], q.lo[2], q.hi[0], q.hi[1], q.hi[2], a.x, a.y, a.z, a.w, b.x, b.y)) continue;
    const int32_t prim = __float_as_int(b.z);
    const float4 t0 = sc.tris[3 * (size_t)prim], t1 = sc.tris[3 * (size_t)prim + 1], t2 = sc.tris[3 * (size_t)prim + 2];
    const float A[3] = {t0.x, t0.y, t0.z}, e1[3] = {t0.w, t1.x, t1.y}, e2[3] = {t1.z, t1.w, t2.x};
    if (lt_overlap::tri_meets_box(q.lo, q.hi, A, e1, e2)) {
      sink.touch(prim);
      if (KIND == lt_overlap::kAny) return;
    }
  }
}

}  // namespace

// lt_nearest_kernel's claim, stage and refill loop (lt_nearest.hip) over boxes: waves claim boxes from the eighth of the batch of
// the XCD they run on (then from the others'), 64 at a time into an LDS stage, and a lane whose box is done takes the next staged
// one whenever `refill` lanes (or all) are idle.  Empty boxes (lt_overlap::empty_box) are answered at once by the lane that drew
// them.  kFirstK: the lane's list is qp.maxK LDS rows behind the stage, which the
// lane resets when it takes a new box -- its neighbours' lists stay as they are -- and writes out when its walk is done.  A step
// pops one stack entry and pushes at most four, so kOwnRows + kOwnDeep entries suffice.
template <int KIND>
__global__ __launch_bounds__(kBlock, 8) void lt_overlap_kernel(SceneDev sc, lt_overlap::Params qp) {
  using u64 = unsigned long long;
  extern __shared__ int lds_stack[];   // [kOvEntries stack rows][kOvStage rows of staged boxes][maxK list rows], 64 lanes each
  if (lt_overlap::list_overflows<KIND>(qp)) return;
  int* const col = lds_stack + threadIdx.x;
  int* const stage = lds_stack + kOvEntries * kBlock;
  const uint32_t total = qp.n;
  const uint32_t lane = threadIdx.x;
  const uint32_t emptyLink = 0x80000000u | (sc.nWide + sc.n_prims);
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kOvClaim ? (uint32_t)kOvClaim : share);
  bool active = false;
  uint32_t stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;
  Box q{};
  Sink<KIND> sink{{col + (kOvEntries + kOvStage) * kBlock, KIND == lt_overlap::kFirstK ? qp.maxK : 0u}, -1, 0u};
  uint32_t idx = 0u, e = 0u;
  int sp = 0;
  int deep[kOvDeep];
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
        if (lane < batch) {   // the caller's record: two 16-byte loads, the pads ignored
          const float4 a = qp.boxes[2 * (size_t)(base + lane)], b = qp.boxes[2 * (size_t)(base + lane) + 1];
          stage[0 * kBlock + lane] = __float_as_int(a.x); stage[1 * kBlock + lane] = __float_as_int(a.y); stage[2 * kBlock + lane] = __float_as_int(a.z);
          stage[3 * kBlock + lane] = __float_as_int(b.x); stage[4 * kBlock + lane] = __float_as_int(b.y); stage[5 * kBlock + lane] = __float_as_int(b.z);
          stage[6 * kBlock + lane] = (int)(base + lane);
        }
        // (one wavefront per workgroup: its own LDS writes are visible to it once they have completed -- the reads below wait for them)
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));   // idle lanes below this one
      if (!active && mine < take) {
        const uint32_t s = stageTaken + mine;
        idx = (uint32_t)stage[6 * kBlock + s];
        q.lo[0] = __int_as_float(stage[0 * kBlock + s]); q.lo[1] = __int_as_float(stage[1 * kBlock + s]); q.lo[2] = __int_as_float(stage[2 * kBlock + s]);
        q.hi[0] = __int_as_float(stage[3 * kBlock + s]); q.hi[1] = __int_as_float(stage[4 * kBlock + s]); q.hi[2] = __int_as_float(stage[5 * kBlock + s]);
        sink.reset(qp, idx);
        if (lt_overlap::empty_box(q.lo[0], q.lo[1], q.lo[2], q.hi[0], q.hi[1], q.hi[2])) {
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
      if (overlap_step(sc, emptyLink, q, sink, col, deep, e, sp)) {
        put_overlap(qp, idx, sink);
        active = false;
      }
    }
  }
}

// A scene without an own tree (boxes that do not nest, bounds >= 2^40): each lane scans the caller's leaves for its boxes --
// slow, correct, and only for the scenes that already fall back.  A kernel of its own: inlined into lt_overlap_kernel as
// nearest_scan is into lt_nearest_kernel, the second copy of the 13-axis test cost the walk two spilled VGPRs.  kFirstK: the
// lane's list is its column of qp.maxK LDS rows.
template <int KIND>
__global__ __launch_bounds__(kBlock, 8) void lt_overlap_scan_kernel(SceneDev sc, lt_overlap::Params qp) {
  extern __shared__ int lds_stack[];   // [maxK list rows], 64 lanes each
  if (lt_overlap::list_overflows<KIND>(qp)) return;
  Sink<KIND> sink{{lds_stack + threadIdx.x, KIND == lt_overlap::kFirstK ? qp.maxK : 0u}, -1, 0u};
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < qp.n; i += (uint64_t)gridDim.x * kBlock) {
    const float4 a = qp.boxes[2 * (size_t)i], b = qp.boxes[2 * (size_t)i + 1];
    const Box q{{a.x, a.y, a.z}, {b.x, b.y, b.z}};
    sink.reset(qp, (uint32_t)i);
    if (!lt_overlap::empty_box(q.lo[0], q.lo[1], q.lo[2], q.hi[0], q.hi[1], q.hi[2])) overlap_scan(sc, q, sink);
    put_overlap(qp, (uint32_t)i, sink);
  }
}

namespace lt_overlap {

hipError_t launch(const SceneDev& sc, const Params& p, uint32_t cuCount, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (p.kind > (uint32_t)kCountWide || p.maxK > kMaxK || (p.kind == (uint32_t)kFirstK) != (p.maxK != 0u)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(p.next, 0, 8 * kQueueStride * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);
  const uint32_t rows = (uint32_t)(kOvEntries + kOvStage) + p.maxK;
  // every wave slot the list rows leave: 160 KB of LDS per CU, at most 32 waves
  const uint32_t bytes = rows * kBlock * (uint32_t)sizeof(int);
  const uint32_t fit = 160u * 1024u / bytes, perCu = fit < 32u ? fit : 32u;
  const uint32_t resident = cuCount * perCu;
  const dim3 grid(chunks < resident ? chunks : resident);
  if (sc.wide == nullptr || sc.rank8 == nullptr) {   // no own tree
    const dim3 all(chunks < cuCount * 32u ? chunks : cuCount * 32u);
    const uint32_t list = p.maxK * kBlock * (uint32_t)sizeof(int);
    if (p.kind == (uint32_t)kFirstK) hipLaunchKernelGGL((lt_overlap_scan_kernel<kFirstK>), all, dim3(kBlock), list, s, sc, p);
    else if (p.kind == (uint32_t)kCount) hipLaunchKernelGGL((lt_overlap_scan_kernel<kCount>), all, dim3(kBlock), list, s, sc, p);
    else if (p.kind == (uint32_t)kList) hipLaunchKernelGGL((lt_overlap_scan_kernel<kList>), all, dim3(kBlock), list, s, sc, p);
    else if (p.kind == (uint32_t)kCountWide) hipLaunchKernelGGL((lt_overlap_scan_kernel<kCountWide>), all, dim3(kBlock), list, s, sc, p);
    else hipLaunchKernelGGL((lt_overlap_scan_kernel<kAny>), all, dim3(kBlock), list, s, sc, p);
    return hipGetLastError();
  }
  if (p.kind == (uint32_t)kFirstK) hipLaunchKernelGGL((lt_overlap_kernel<kFirstK>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kCount) hipLaunchKernelGGL((lt_overlap_kernel<kCount>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kList) hipLaunchKernelGGL((lt_overlap_kernel<kList>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kCountWide) hipLaunchKernelGGL((lt_overlap_kernel<kCountWide>), grid, dim3(kBlock), bytes, s, sc, p);
  else hipLaunchKernelGGL((lt_overlap_kernel<kAny>), grid, dim3(kBlock), bytes, s, sc, p);
  return hipGetLastError();
}

}  // namespace lt_overlap
