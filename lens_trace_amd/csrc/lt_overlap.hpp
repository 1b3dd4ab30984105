// lt_overlap.hpp -- box-overlap queries over the resident scene (lt_overlap.hip; lt_hip_overlap_boxes in lt_capi.hip): the
// arithmetic of the definition in include/lenstrace_hip.h, shared by the kernel, by the host form (lt_hip_overlap_boxes_host) and,
// restated in numpy, by tests/overlap.py.  Every operation below is one IEEE float32 operation, rounded once, in the order
// written: the build contracts nothing (-ffp-contract=off), subnormals are kept.  Only slot_box fuses, and says so
// (__builtin_fmaf).  Compares with a NaN are false, which everywhere below reads "not separated"; minima and maxima are chains
// of compares (no fmin / fmax, whose NaN rules differ between processors).
//
// A candidate (a leaf of the caller's tree with its one primitive) touches a box q iff
//     boxes_meet(q, the leaf's own box)  and  tri_meets_box(q; A, e1, e2),
// where (A, e1, e2) is the traversal triangle as the scene stores it (A, fl(B - A), fl(C - A)).  The walk prunes with boxes_meet
// alone, which is monotone in enclosure, so it needs no margins.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define LT_OV_HD __host__ __device__
#else
#define LT_OV_HD
#endif

namespace lt_overlap {

constexpr uint32_t kMaxK = 8;   // LT_OVERLAP_MAX_K

// A box that touches nothing: a bound that is not finite, or lo <= hi failing on an axis.  lo == hi is a point box.
LT_OV_HD inline bool empty_box(float lx, float ly, float lz, float hx, float hy, float hz) {
  const float inf = __builtin_inff();
  const bool finite = __builtin_fabsf(lx) < inf && __builtin_fabsf(ly) < inf && __builtin_fabsf(lz) < inf && __builtin_fabsf(hx) < inf &&
                      __builtin_fabsf(hy) < inf && __builtin_fabsf(hz) < inf;
  return !(finite && lx <= hx && ly <= hy && lz <= hz);
}

// Per axis q.lo <= b.hi && b.lo <= q.hi; a NaN bound makes it false.  Compares only: if a box B encloses a box b as floats
// (B.lo <= b.lo, B.hi >= b.hi) then boxes_meet(q, b) implies boxes_meet(q, B).
LT_OV_HD inline bool boxes_meet(float qlx, float qly, float qlz, float qhx, float qhy, float qhz, float blx, float bly, float blz, float bhx,
                                float bhy, float bhz) {
  return qlx <= bhx && blx <= qhx && qly <= bhy && bly <= qhy && qlz <= bhz && blz <= qhz;
}

// The smallest and the largest of three by compares, the first operand kept at ties and against a NaN.
LT_OV_HD inline float min3(float a, float b, float c) {
  float m = a;
  if (b < m) m = b;
  if (c < m) m = c;
  return m;
}
LT_OV_HD inline float max3(float a, float b, float c) {
  float m = a;
  if (b > m) m = b;
  if (c > m) m = c;
  return m;
}

// One edge axis (a unit axis crossed with an edge f): the three vertices' projections p = a b' - a' b in that order, the box's
// radius r = ha |fb| + hb |fa| in the two-term form; separated iff min(p) > r or max(p) < -r.
//   v?a, v?b: the two coordinates of the centred vertices that the axis sees; fa, fb: the edge's; ha, hb: the half-sizes.
//   p_i = v_i.a * fb - v_i.b * fa,  r = ha * |fb| + hb * |fa|.
LT_OV_HD inline bool edge_separates(float v0a, float v0b, float v1a, float v1b, float v2a, float v2b, float fa, float fb, float ha, float hb) {
  const float p0 = v0a * fb - v0b * fa, p1 = v1a * fb - v1b * fa, p2 = v2a * fb - v2b * fa;
  const float r = ha * __builtin_fabsf(fb) + hb * __builtin_fabsf(fa);
  return min3(p0, p1, p2) > r || max3(p0, p1, p2) < -r;
}

// The three axes of one edge f, in the order x, y, z of the unit axis: the projections are
//   x:  v.z f.y - v.y f.z    (a = z, b = y),   r = h.z |f.y| + h.y |f.z|
//   y:  v.x f.z - v.z f.x    (a = x, b = z),   r = h.x |f.z| + h.z |f.x|
//   z:  v.y f.x - v.x f.y    (a = y, b = x),   r = h.y |f.x| + h.x |f.y|
LT_OV_HD inline bool edge_axes_separate(const float* v0, const float* v1, const float* v2, float fx, float fy, float fz, const float* h) {
  return edge_separates(v0[2], v0[1], v1[2], v1[1], v2[2], v2[1], fz, fy, h[2], h[1]) ||
         edge_separates(v0[0], v0[2], v1[0], v1[2], v2[0], v2[2], fx, fz, h[0], h[2]) ||
         edge_separates(v0[1], v0[0], v1[1], v1[0], v2[1], v2[0], fy, fx, h[1], h[0]);
}

// The three classes of the 13 axes, each on its own (tests/overlap.py counts them one by one; tri_meets_box is "none of them").
//
// Box axes: un-centred, on the vertices A, fl(A + e1), fl(A + e2): axis k separates iff min > hi[k] or max < lo[k].  Compares
// only, so a vertex exactly on a face touches the cells on both sides of it.
LT_OV_HD inline bool box_axes_separate(const float* lo, const float* hi, const float* A, const float* e1, const float* e2) {
  for (int k = 0; k < 3; k++) {
    const float b = A[k] + e1[k], c = A[k] + e2[k];
    if (min3(A[k], b, c) > hi[k] || max3(A[k], b, c) < lo[k]) return true;
  }
  return false;
}

// The other ten axes see the triangle from the box's centre: c = 0.5 lo + 0.5 hi, h = 0.5 hi - 0.5 lo (>= 0: rounding is
// monotone), v0 = A - c, v1 = v0 + e1, v2 = v0 + e2.
struct Centred { float h[3], v0[3], v1[3], v2[3]; };
LT_OV_HD inline Centred centre(const float* lo, const float* hi, const float* A, const float* e1, const float* e2) {
  Centred t;
  for (int k = 0; k < 3; k++) {
    const float c = 0.5f * lo[k] + 0.5f * hi[k];
    t.h[k] = 0.5f * hi[k] - 0.5f * lo[k];
    t.v0[k] = A[k] - c;
    t.v1[k] = t.v0[k] + e1[k];
    t.v2[k] = t.v0[k] + e2[k];
  }
  return t;
}

// The plane: n = e1 x e2 (n.x = e1.y e2.z - e1.z e2.y, n.y = e1.z e2.x - e1.x e2.z, n.z = e1.x e2.y - e1.y e2.x),
// d = (n.x v0.x + n.y v0.y) + n.z v0.z, r = (|n.x| h.x + |n.y| h.y) + |n.z| h.z; separated iff d > r or d < -r.
LT_OV_HD inline bool plane_separates(const Centred& t, const float* e1, const float* e2) {
  const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
  const float d = (nx * t.v0[0] + ny * t.v0[1]) + nz * t.v0[2];
  const float r = (__builtin_fabsf(nx) * t.h[0] + __builtin_fabsf(ny) * t.h[1]) + __builtin_fabsf(nz) * t.h[2];
  return d > r || d < -r;
}

// The nine edge axes: the edges f0 = e1, f1 = e2 - e1, f2 = -e2 in that order, each with the unit axes x, y, z.  A point
// triangle or a needle gives zero axes (p = 0, r = 0), which separate nothing: the other axes decide.
LT_OV_HD inline bool edges_separate(const Centred& t, const float* e1, const float* e2) {
  return edge_axes_separate(t.v0, t.v1, t.v2, e1[0], e1[1], e1[2], t.h) ||
         edge_axes_separate(t.v0, t.v1, t.v2, e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2], t.h) ||
         edge_axes_separate(t.v0, t.v1, t.v2, -e2[0], -e2[1], -e2[2], t.h);
}

// The 13-axis test, in the order box axes, plane, edge axes.  Each class is a pure function of the operands, so the verdict does
// not depend on where the evaluation stops.  (It stops at the first axis that separates.  Evaluated without branches the ten
// centred axes kept the kernel's every operand alive at once and spilled more than a hundred registers per lane.)
LT_OV_HD inline bool tri_meets_box(const float* lo, const float* hi, const float* A, const float* e1, const float* e2) {
  if (box_axes_separate(lo, hi, A, e1, e2)) return false;
  const Centred t = centre(lo, hi, A, e1, e2);
  if (plane_separates(t, e1, e2)) return false;
  return !edges_separate(t, e1, e2);
}

// A 4-wide group's child slot (lt_own16.hpp) put back on the grid: lo = fma(ql, S, O), hi = fma(qh, S, O) per axis, ONE rounding
// each as in lt_nearest::slot_bound, so that O + ql S <= lo' in reals gives lo <= lo' in floats for every leaf box beneath the
// slot (and hi >= hi').  q: the slot's first three words (lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16).
LT_OV_HD inline void slot_box(uint32_t q0, uint32_t q1, uint32_t q2, const float* O, const float* S, float* lo, float* hi) {
  lo[0] = __builtin_fmaf((float)(q0 & 0xffffu), S[0], O[0]); lo[1] = __builtin_fmaf((float)(q0 >> 16), S[1], O[1]);
  lo[2] = __builtin_fmaf((float)(q1 & 0xffffu), S[2], O[2]);
  hi[0] = __builtin_fmaf((float)(q1 >> 16), S[0], O[0]); hi[1] = __builtin_fmaf((float)(q2 & 0xffffu), S[1], O[1]);
  hi[2] = __builtin_fmaf((float)(q2 >> 16), S[2], O[2]);
}

// The first k entries of a box's sequence: the touching candidates' primitive offsets in ascending order, -1 behind the end.
// Entry j is col[j STRIDE] -- the kernel's lists are columns of LDS rows (STRIDE = 64 lanes), the host form's an array
// (STRIDE = 1).  An offset equal to one in the list goes behind it: in a scan in node order that is the sequence's second key.
// No subtree can be pruned by offset -- a hierarchy knows nothing of the offsets beneath a node -- so LT_OVERLAP_FIRST_K visits
// what LT_OVERLAP_COUNT visits.
template <int STRIDE>
struct KList {
  int* col;
  uint32_t k;   // 1 .. LT_OVERLAP_MAX_K
  LT_OV_HD int32_t at(uint32_t j) const { return col[j * STRIDE]; }
  LT_OV_HD void reset() { for (uint32_t j = 0; j < k; j++) col[j * STRIDE] = -1; }
  LT_OV_HD void offer(int32_t p) {
    uint32_t j = k;
    while (j > 0u) {
      const int32_t e = at(j - 1u);
      if (!(e < 0 || p < e)) break;
      if (j < k) col[j * STRIDE] = e;
      j--;
    }
    if (j < k) col[j * STRIDE] = p;
  }
};

}  // namespace lt_overlap

#if defined(__HIPCC__) || defined(__HIP__)
#include "lt_device.hpp"

namespace lt_overlap {

// LT_OVERLAP_FIRST_K, LT_OVERLAP_COUNT, LT_OVERLAP_ANY, and the two kinds of the overlap lists (lt_overlist.hpp), which no
// descriptor names: kList, the whole sequence into the query's segment of `items`; kCountWide, kCount as one uint64 per query.
enum Kind { kFirstK = 0, kCount = 1, kAny = 2, kList = 3, kCountWide = 4 };

// The caller's records as the kernel reads them: 32 bytes per box (lo.xyz, pad, hi.xyz, pad) -- lt_hip_box -- and per box maxK
// int32 offsets (kFirstK), one uint32 (kCount, kAny) or one uint64 (kCountWide).  kList writes nothing to `out`: query i's
// touching offsets go, in walk order, to items[offsets[i] .. min(offsets[i + 1], capacity)) and whatever is beyond that is dropped.
struct Params {
  const float4* boxes;
  uint32_t* out;
  uint32_t n;
  uint32_t kind;
  uint32_t maxK;      // kFirstK: 1 .. kMaxK; else 0
  uint32_t* next;     // the work counters: eight, kQueueStride dwords apart, zeroed by launch() on the call's stream
  uint32_t refill;    // idle lanes that make a wave take new boxes
  uint32_t oneShot;   // kList: the offsets are this stream's own scan -- when offsets[n] > capacity the launch writes nothing
  const unsigned long long* offsets;   // kList: n + 1 words
  int32_t* items;                      // kList: `capacity` words
  unsigned long long capacity;
};

// What takes a query's touching candidates, for the box and the triangle kernels alike.  kCount, kCountWide and kAny count in a
// register (kAny's walk ends at the first).  kFirstK keeps the K smallest offsets in the lane's column of LDS rows and the list's
// last entry in a register: once the list is full, an offset that is not below that entry never touches LDS.  kList stores each
// offset behind the last in the query's segment while words are left of it: a pointer and the words left, no LDS rows.
template <int KIND>
struct Sink {
  KList<lt::kBlock> list;
  int32_t last;    // kFirstK: the list's last entry (-1: not full)
  uint32_t n;      // kList: the words left of the segment
  int32_t* at;     // kList: where the next offset goes
  // The lane takes query idx.  kList: the clamped bounds -- a length that would be negative is 0, so with any offsets at all no
  // store falls outside items[0 .. capacity).
  __device__ __forceinline__ void reset(const Params& qp, uint32_t idx) {
    n = 0u;
    if (KIND == kFirstK) { list.reset(); last = -1; }
    if (KIND == kList) {
      const unsigned long long begin = qp.offsets[idx], to = qp.offsets[(size_t)idx + 1];
      const unsigned long long end = to < qp.capacity ? to : qp.capacity;
      const unsigned long long room = end > begin ? end - begin : 0ull;
      n = room > 0xffffffffull ? 0xffffffffu : (uint32_t)room;
      at = qp.items + begin;   // (never dereferenced when n == 0)
    }
  }
  __device__ __forceinline__ void touch(int32_t p) {
    if (KIND == kList) {
      if (n != 0u) { *at++ = p; n--; }
      return;
    }
    n++;
    if (KIND == kFirstK) {
      if (last >= 0 && p >= last) return;
      list.offer(p);
      last = list.at(list.k - 1u);
    }
  }
};

template <int KIND>
__device__ __forceinline__ void put_overlap(const Params& qp, uint32_t idx, const Sink<KIND>& sink) {
  if (KIND == kFirstK) {
    int32_t* out = (int32_t*)qp.out + (size_t)idx * qp.maxK;
    for (uint32_t j = 0; j < sink.list.k; j++) out[j] = sink.list.at(j);
  } else if (KIND == kCountWide) {
    ((unsigned long long*)qp.out)[idx] = sink.n;
  } else if (KIND != kList) {
    qp.out[idx] = KIND == kAny ? (sink.n != 0u ? 1u : 0u) : sink.n;
  }
}

// kList in its one-shot form: whether the launch has to write nothing (every lane reads the same word).
template <int KIND>
__device__ __forceinline__ bool list_overflows(const Params& qp) {
  return KIND == kList && qp.oneShot != 0u && qp.offsets[qp.n] > qp.capacity;
}

// Enqueues lt_overlap_kernel<kind> on `s`.  Returns the first HIP error.
hipError_t launch(const lt::SceneDev& sc, const Params& p, uint32_t cuCount, hipStream_t s);

}  // namespace lt_overlap
#endif
