// lt_nearest.hip -- nearest-point queries over the resident scene: the kernel behind lt_hip_nearest_points /
// lt_hip_nearest_points_device.  For each point: the candidate (a leaf of the caller's tree with its one primitive) of the smallest
// d2 below the point's max_d2, the lowest primitive offset among equal d2 -- d2, u and v as lt_nearest.hpp defines them, so the
// answer is a function of the scene and the point alone and the walk only has to find it.
//
// The walk is best-first over the per-lane walks' records (SceneDev::wide): a group's four child slots get their bound
// (slot_bound), the ones that can still hold the answer go on the lane's stack far to near WITH their bound, and an entry that
// comes off is tested against the running best once more before its record is fetched.  A leaf record holds the triangle, the
// leaf's own box and the offset.  Nothing is dropped that could hold a candidate with d2 <= best (or, before the first one, with
// d2 < max_d2): every bound on the way to a leaf is <= that leaf's box_d2 <= its d2, as floats, without margins.
// A scene without an own tree is scanned leaf by leaf in the caller's node order.
//
// And the k-nearest queries (lt_hip_nearest_k): lt_nearest_k_kernel, the same loop and step with another sink -- the first K
// candidates by (d2, offset) in a per-lane list in LDS, or their number -- and "best" read as "K-th best" (DESIGN 5.15).
//
// And the count and the fill of the radius lists (lt_hip_nearest_list; the scan and the ordering are lt_overlist.hip's): that
// kernel with two more sinks, the number as one uint64 and every accepted candidate as a record into the point's segment of a CSR
// array.
#include "lt_nearest.hpp"

using namespace lt;

namespace {

constexpr int kNearClaim = 512;      // points a wave claims per atomic (lt_query_kernel's kQueryClaim)
constexpr int kNearEntries = 7;      // stack entries per lane in LDS, two rows each (link, bound) ...
constexpr int kNearDeep = kOwnRows + kOwnDeep - kNearEntries;   // ... and the entries beyond them, in private memory
constexpr int kNearStage = 5;        // rows of staged points (p.xyz, max_d2, index): 19 rows = 4.75 KB, 32 waves per CU

__device__ __forceinline__ void put_nearest(const lt_nearest::Params& qp, uint32_t idx, const lt_nearest::Best& b) {
  qp.hits[(size_t)idx] = make_uint4(__float_as_uint(b.t), (uint32_t)b.prim, __float_as_uint(b.u), __float_as_uint(b.v));
}

struct Grid { float O[3], S[3]; };   // the 16-bit grid of the group slots (wide[-2], wide[-1])

// One step of the walk for one lane: the record `e` (a group, or a leaf: bit 31) is fetched and dealt with, the next entry that
// can still hold the answer popped into `e`.  Returns true when the stack is empty.  SINK: what takes the candidates and says
// which bounds it still reaches -- lt_nearest::Best, lt_hip_nearest_k's LaneList (the first K) and lt_nearest::KCount, or the
// radius lists' ListSink.
template <class SINK>
__device__ __forceinline__ bool nearest_step(const SceneDev& sc, const Grid& g, uint32_t emptyLink, float px, float py, float pz, SINK& best,
                                             int* col, int* deep, uint32_t& e, int& sp) {
  const uint4* rec = (const uint4*)((const char*)sc.wide + ((size_t)(e & 0x7fffffffu) << 6));
  const uint4 s0 = rec[0], s1 = rec[1], s2 = rec[2], s3 = rec[3];
  if ((int)e < 0) {   // a leaf: A e1.x | e1.yz e2.xy | e2.z lo | hi prim
    const lt_nearest::Tri t = lt_nearest::tri(px, py, pz, __uint_as_float(s0.x), __uint_as_float(s0.y), __uint_as_float(s0.z), __uint_as_float(s0.w),
                                              __uint_as_float(s1.x), __uint_as_float(s1.y), __uint_as_float(s1.z), __uint_as_float(s1.w),
                                              __uint_as_float(s2.x));
    const float box = lt_nearest::box_d2(px, py, pz, __uint_as_float(s2.y), __uint_as_float(s2.z), __uint_as_float(s2.w), __uint_as_float(s3.x),
                                         __uint_as_float(s3.y), __uint_as_float(s3.z));
    best.offer(lt_nearest::candidate_d2(t.d2, box), t.u, t.v, (int32_t)s3.w);
  } else {
    // the slots that can still hold the answer, sorted by bound, the farthest pushed first (an empty slot's link is the record
    // behind the last primitive's: never entered).  -1 marks a slot that is dropped: every bound is >= +0.
    const uint4 slot[4] = {s0, s1, s2, s3};
    float key[4];
    uint32_t link[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float b = lt_nearest::slot_bound(slot[k].x, slot[k].y, slot[k].z, g.O, g.S, px, py, pz);
      link[k] = slot[k].w;
      key[k] = (slot[k].w != emptyLink && best.reaches(b)) ? b : -1.0f;
    }
#define LT_NEAR_ORDER(i, j)                                                    \
  if (key[i] < key[j]) {                                                       \
    const float tk = key[i]; key[i] = key[j]; key[j] = tk;                     \
    const uint32_t tl = link[i]; link[i] = link[j]; link[j] = tl;              \
  }
    LT_NEAR_ORDER(0, 1) LT_NEAR_ORDER(2, 3) LT_NEAR_ORDER(0, 2) LT_NEAR_ORDER(1, 3) LT_NEAR_ORDER(1, 2)
#undef LT_NEAR_ORDER
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (key[k] >= 0.0f) {
        if (sp < kNearEntries) { col[2 * sp * kBlock] = (int)link[k]; col[(2 * sp + 1) * kBlock] = __float_as_int(key[k]); }
        else { deep[2 * (sp - kNearEntries)] = (int)link[k]; deep[2 * (sp - kNearEntries) + 1] = __float_as_int(key[k]); }
        sp++;
      }
    }
  }
  while (sp > 0) {
    sp--;
    const uint32_t l = (uint32_t)(sp < kNearEntries ? col[2 * sp * kBlock] : deep[2 * (sp - kNearEntries)]);
    const float b = __int_as_float(sp < kNearEntries ? col[(2 * sp + 1) * kBlock] : deep[2 * (sp - kNearEntries) + 1]);
    if (best.reaches(b)) { e = l; return false; }
  }
  return true;
}

// A scene without an own tree: every leaf of the caller's node array in index order; the triangle may be skipped when the leaf's
// box alone is already beyond what the sink still takes (d2 >= box_d2).
template <class SINK>
__device__ __forceinline__ void nearest_scan(const SceneDev& sc, float px, float py, float pz, SINK& best) {
  for (uint32_t i = 0; i < sc.n_nodes; i++) {
    const float4 a = sc.nodes[2 * (size_t)i], b = sc.nodes[2 * (size_t)i + 1];
    if ((__float_as_uint(b.w) & 0xffffu) == 0u) continue;
    const float box = lt_nearest::box_d2(px, py, pz, a.x, a.y, a.z, a.w, b.x, b.y);
    if (!best.reaches(box)) continue;
    const int32_t prim = __float_as_int(b.z);
    const float4 t0 = sc.tris[3 * (size_t)prim], t1 = sc.tris[3 * (size_t)prim + 1], t2 = sc.tris[3 * (size_t)prim + 2];
    const lt_nearest::Tri t = lt_nearest::tri(px, py, pz, t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x);
    best.offer(lt_nearest::candidate_d2(t.d2, box), t.u, t.v, prim);
  }
}

}  // namespace

// lt_query_kernel's claim, stage and refill loop (lt_query.hip) over points: waves claim points from the eighth of the batch of the
// XCD they run on (then from the others'), 64 at a time into an LDS stage, and a lane whose point is done takes the next staged
// one whenever `refill` lanes (or all) are idle.  Points that need no walk (lt_nearest::no_walk) and every point of a scene
// without an own tree are answered at once by the lane that drew them.
__global__ __launch_bounds__(kBlock, 8) void lt_nearest_kernel(SceneDev sc, lt_nearest::Params qp) {
  using u64 = unsigned long long;
  extern __shared__ int lds_stack[];   // [2 kNearEntries stack rows][kNearStage rows of staged points], 64 lanes each
  int* const col = lds_stack + threadIdx.x;
  int* const stage = lds_stack + 2 * kNearEntries * kBlock;
  const uint32_t total = qp.n;
  const uint32_t lane = threadIdx.x;
  const bool ownTree = sc.wide != nullptr && sc.rank8 != nullptr;
  const uint32_t emptyLink = 0x80000000u | (sc.nWide + sc.n_prims);
  Grid g{};
  if (ownTree) {
    const F8v fr = *(ConstF8)((unsigned long long)sc.wide - 32ull);   // origin.xyz - step.xyz -
    g = Grid{{fr.s0, fr.s1, fr.s2}, {fr.s4, fr.s5, fr.s6}};
  }
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kNearClaim ? (uint32_t)kNearClaim : share);
  bool active = false;
  uint32_t stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  lt_nearest::Best best{0.0f, 0.0f, 0.0f, -1};
  uint32_t idx = 0u, e = 0u;
  int sp = 0;
  int deep[2 * kNearDeep];
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
        if (lane < batch) {   // the caller's record: one coalesced 16-byte load
          const float4 a = qp.points[(size_t)(base + lane)];
          stage[0 * kBlock + lane] = __float_as_int(a.x); stage[1 * kBlock + lane] = __float_as_int(a.y); stage[2 * kBlock + lane] = __float_as_int(a.z);
          stage[3 * kBlock + lane] = __float_as_int(a.w);   // max_d2
          stage[4 * kBlock + lane] = (int)(base + lane);
        }
        // (one wavefront per workgroup: its own LDS writes are visible to it once they have completed -- the reads below wait for them)
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));   // idle lanes below this one
      if (!active && mine < take) {
        const uint32_t s = stageTaken + mine;
        idx = (uint32_t)stage[4 * kBlock + s];
        px = __int_as_float(stage[0 * kBlock + s]); py = __int_as_float(stage[1 * kBlock + s]); pz = __int_as_float(stage[2 * kBlock + s]);
        best = lt_nearest::Best{__int_as_float(stage[3 * kBlock + s]), 0.0f, 0.0f, -1};
        if (lt_nearest::no_walk(px, py, pz, best.t)) {
          put_nearest(qp, idx, best);
        } else if (ownTree) {
          e = 0u;   // the root's group
          sp = 0;
          active = true;
        } else {
          nearest_scan(sc, px, py, pz, best);
          put_nearest(qp, idx, best);
        }
      }
      stageTaken += take;
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
      if (drained && stageTaken == stageCount) break;
      continue;
    }
    if (active) {
      if (nearest_step(sc, g, emptyLink, px, py, pz, best, col, deep, e, sp)) {
        put_nearest(qp, idx, best);
        active = false;
      }
    }
  }
}

namespace {

// The lane's KList with its last entry in registers: every slot and every popped entry asks reaches(), and a candidate enters
// the list iff it comes before that entry -- the others never touch LDS.
struct LaneList {
  lt_nearest::KList<kBlock> list;
  float lastD2;
  int32_t lastPrim;
  __device__ __forceinline__ void reset(float max_d2) { list.reset(max_d2); lastD2 = max_d2; lastPrim = -1; }
  __device__ __forceinline__ void offer(float d2, float u, float v, int32_t p) {
    if (!lt_nearest::before(d2, p, lastD2, lastPrim)) return;
    list.offer(d2, u, v, p);
    lastD2 = list.d2(list.k - 1u);
    lastPrim = list.prim(list.k - 1u);
  }
  __device__ __forceinline__ bool reaches(float bound) const { return lt_nearest::last_reaches(bound, lastD2, lastPrim); }
};

// A point's K records: d2 and the primitive from the list, u and v from lt_nearest::tri run once more on the traversal triangle
// and the same point -- the same function on the same operands as in the walk's leaf record, hence the same bits.  Empty entries
// are the miss record already (max_d2's bits, -1); their u and v are +0.
__device__ __forceinline__ void put_nearest_k(const SceneDev& sc, const lt_nearest::KList<kBlock>& list, float px, float py, float pz, uint4* out) {
  for (uint32_t j = 0; j < list.k; j++) {
    const int prim = list.prim(j);
    float u = 0.0f, v = 0.0f;
    if (prim >= 0) {
      const float4 t0 = sc.tris[3 * (size_t)prim], t1 = sc.tris[3 * (size_t)prim + 1], t2 = sc.tris[3 * (size_t)prim + 2];
      const lt_nearest::Tri t = lt_nearest::tri(px, py, pz, t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x);
      u = t.u; v = t.v;
    }
    out[j] = make_uint4((uint32_t)list.d2_bits(j), (uint32_t)prim, __float_as_uint(u), __float_as_uint(v));
  }
}

// The radius lists' fill: a point's accepted candidates, each stored behind the last in the point's segment while records are
// left of it, no LDS rows.  u and v arrive with the offer, so nothing is computed again.  The pruning bound never moves: reaches
// is KCount's.  In registers the sink is KCount's two words, the radius and the records left: u and v stay live across tri() here,
// which the count lets die, and a pointer on top of them does not fit 64 VGPRs -- so an offer reads the segment's end again (one
// cached 8-byte load beside a 16-byte store) and stores at end - left.
struct ListSink {
  float max_d2;
  uint32_t left;   // the records left of the segment
  uint32_t idx;    // the point (the kernel's own register)
  const lt_nearest::KParams* qp;
  __device__ __forceinline__ unsigned long long end() const {
    const unsigned long long to = qp->offsets[(size_t)idx + 1];
    return to < qp->capacity ? to : qp->capacity;
  }
  // The lane takes point i: the clamped bounds -- a length that would be negative is 0, so with any offsets at all no store
  // falls outside items[0 .. capacity).
  __device__ __forceinline__ void reset(uint32_t i, float maxD2) {
    idx = i;
    const unsigned long long begin = qp->offsets[i], to = end();
    const unsigned long long room = to > begin ? to - begin : 0ull;
    max_d2 = maxD2;
    left = room > 0xffffffffull ? 0xffffffffu : (uint32_t)room;
  }
  __device__ __forceinline__ void offer(float d2, float u, float v, int32_t p) {
    if (d2 < max_d2 && left != 0u) {
      const unsigned long long to = end();
      // (left <= to holds while the offsets are what reset() read; were they changed under the launch, the store is dropped)
      if (left <= to) qp->items[to - left] = make_uint4(__float_as_uint(d2), (uint32_t)p, __float_as_uint(u), __float_as_uint(v));
      left--;
    }
  }
  __device__ __forceinline__ bool reaches(float bound) const { return bound < max_d2; }
};

// A point's count: one uint32 (LT_NEAREST_COUNT) or, kCountWide, one uint64 into the list's offsets.
template <int KIND>
__device__ __forceinline__ void put_count(const lt_nearest::KParams& qp, uint32_t idx, uint32_t n) {
  if (KIND == lt_nearest::kCountWide) qp.offsets[idx] = n; else qp.counts[idx] = n;
}

}  // namespace

// lt_hip_nearest_k: lt_nearest_kernel's claim, stage and refill loop with another sink.  COUNT counts a point's accepted
// candidates in a register and keeps every subtree whose bound is below max_d2.  Otherwise the candidates go into the lane's
// KList of qp.maxK entries, 2 maxK LDS rows behind the stage, which the lane resets when it takes a new point -- its neighbours'
// lists stay as they are -- and writes out when its walk is done; a subtree is kept while its bound reaches the list's last
// entry (KList::reaches).  A step pops one stack entry and pushes at most four whatever the sink keeps, so the
// stack is lt_nearest_kernel's.
// The radius lists (lt_hip_nearest_list) are two more sinks: kCountWide is COUNT stored as one uint64 into offsets[idx]; kList is
// ListSink above -- no LDS list rows, so its layout and occupancy are the count's -- and points that take no walk write nothing.
template <int KIND>
__global__ __launch_bounds__(kBlock, 8) void lt_nearest_k_kernel(SceneDev sc, lt_nearest::KParams qp) {
  using u64 = unsigned long long;
  constexpr bool COUNT = KIND == lt_nearest::kCount || KIND == lt_nearest::kCountWide, LIST = KIND == lt_nearest::kList;
  extern __shared__ int lds_stack[];   // [2 kNearEntries stack rows][kNearStage rows of staged points][2 maxK list rows], 64 lanes each
  if (LIST && qp.oneShot != 0u && qp.offsets[qp.n] > qp.capacity) return;   // (every lane reads the same word)
  int* const col = lds_stack + threadIdx.x;
  int* const stage = lds_stack + 2 * kNearEntries * kBlock;
  const uint32_t total = qp.n;
  const uint32_t lane = threadIdx.x;
  const bool ownTree = sc.wide != nullptr && sc.rank8 != nullptr;
  const uint32_t emptyLink = 0x80000000u | (sc.nWide + sc.n_prims);
  Grid g{};
  if (ownTree) {
    const F8v fr = *(ConstF8)((unsigned long long)sc.wide - 32ull);   // origin.xyz - step.xyz -
    g = Grid{{fr.s0, fr.s1, fr.s2}, {fr.s4, fr.s5, fr.s6}};
  }
  const uint32_t share = total / (gridDim.x * 4u) / (uint32_t)kBlock * (uint32_t)kBlock;
  const uint32_t claim = share < (uint32_t)kBlock ? (uint32_t)kBlock : (share > (uint32_t)kNearClaim ? (uint32_t)kNearClaim : share);
  bool active = false;
  uint32_t stageCount = 0u, stageTaken = 0u, claimNext = 0u, claimEnd = 0u, sweep = 0u;
  const uint32_t home = __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 7u;   // HW_REG_XCC_ID
  bool drained = false;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  LaneList list{{col + (2 * kNearEntries + kNearStage) * kBlock, COUNT || LIST ? 0u : qp.maxK}, 0.0f, -1};
  lt_nearest::KCount count{0.0f, 0u};
  ListSink fill{0.0f, 0u, 0u, &qp};
  uint32_t idx = 0u, e = 0u;
  int sp = 0;
  int deep[2 * kNearDeep];
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
        if (lane < batch) {   // the caller's record: one coalesced 16-byte load
          const float4 a = qp.points[(size_t)(base + lane)];
          stage[0 * kBlock + lane] = __float_as_int(a.x); stage[1 * kBlock + lane] = __float_as_int(a.y); stage[2 * kBlock + lane] = __float_as_int(a.z);
          stage[3 * kBlock + lane] = __float_as_int(a.w);   // max_d2
          stage[4 * kBlock + lane] = (int)(base + lane);
        }
      }
      const uint32_t take = nIdle < stageCount - stageTaken ? nIdle : stageCount - stageTaken;
      const uint32_t mine = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));   // idle lanes below this one
      if (!active && mine < take) {
        const uint32_t s = stageTaken + mine;
        idx = (uint32_t)stage[4 * kBlock + s];
        px = __int_as_float(stage[0 * kBlock + s]); py = __int_as_float(stage[1 * kBlock + s]); pz = __int_as_float(stage[2 * kBlock + s]);
        const float maxD2 = __int_as_float(stage[3 * kBlock + s]);
        if (COUNT) count = lt_nearest::KCount{maxD2, 0u}; else if (LIST) fill.reset(idx, maxD2); else list.reset(maxD2);
        if (lt_nearest::no_walk(px, py, pz, maxD2)) {
          if (COUNT) put_count<KIND>(qp, idx, 0u); else if (!LIST) put_nearest_k(sc, list.list, px, py, pz, qp.hits + (size_t)idx * qp.maxK);
        } else if (ownTree) {
          e = 0u;   // the root's group
          sp = 0;
          active = true;
        } else if (COUNT) {
          nearest_scan(sc, px, py, pz, count);
          put_count<KIND>(qp, idx, count.n);
        } else if (LIST) {
          nearest_scan(sc, px, py, pz, fill);
        } else {
          nearest_scan(sc, px, py, pz, list);
          put_nearest_k(sc, list.list, px, py, pz, qp.hits + (size_t)idx * qp.maxK);
        }
      }
      stageTaken += take;
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
      if (drained && stageTaken == stageCount) break;
      continue;
    }
    if (active) {
      const bool done = COUNT  ? nearest_step(sc, g, emptyLink, px, py, pz, count, col, deep, e, sp)
                        : LIST ? nearest_step(sc, g, emptyLink, px, py, pz, fill, col, deep, e, sp)
                               : nearest_step(sc, g, emptyLink, px, py, pz, list, col, deep, e, sp);
      if (done) {
        if (COUNT) put_count<KIND>(qp, idx, count.n); else if (!LIST) put_nearest_k(sc, list.list, px, py, pz, qp.hits + (size_t)idx * qp.maxK);
        active = false;
      }
    }
  }
}

namespace lt_nearest {

hipError_t launch_k(const SceneDev& sc, const KParams& p, uint32_t cuCount, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (p.kind > (uint32_t)kCountWide || p.maxK > kMaxK || (p.kind == (uint32_t)kFirstK) != (p.maxK != 0u)) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(p.next, 0, 8 * kQueueStride * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);
  const uint32_t rows = (uint32_t)(2 * kNearEntries + kNearStage) + 2u * p.maxK;
  // every wave slot the list rows leave: 160 KB of LDS per CU, at most 32 waves
  const uint32_t fit = 160u * 1024u / (rows * kBlock * (uint32_t)sizeof(int)), perCu = fit < 32u ? fit : 32u;
  const uint32_t resident = cuCount * perCu;
  const dim3 grid(chunks < resident ? chunks : resident);
  const uint32_t bytes = rows * kBlock * (uint32_t)sizeof(int);
  if (p.kind == (uint32_t)kCount) hipLaunchKernelGGL((lt_nearest_k_kernel<kCount>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kCountWide) hipLaunchKernelGGL((lt_nearest_k_kernel<kCountWide>), grid, dim3(kBlock), bytes, s, sc, p);
  else if (p.kind == (uint32_t)kList) hipLaunchKernelGGL((lt_nearest_k_kernel<kList>), grid, dim3(kBlock), bytes, s, sc, p);
  else hipLaunchKernelGGL((lt_nearest_k_kernel<kFirstK>), grid, dim3(kBlock), bytes, s, sc, p);
  return hipGetLastError();
}

hipError_t launch(const SceneDev& sc, const Params& p, uint32_t cuCount, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(p.next, 0, 8 * kQueueStride * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint32_t chunks = (uint32_t)(((uint64_t)p.n + kBlock - 1) / kBlock);
  const uint32_t resident = cuCount * 32u;   // every wave slot of the chip, once
  hipLaunchKernelGGL(lt_nearest_kernel, dim3(chunks < resident ? chunks : resident), dim3(kBlock),
                     (uint32_t)((2 * kNearEntries + kNearStage) * kBlock * sizeof(int)), s, sc, p);
  return hipGetLastError();
}

}  // namespace lt_nearest
