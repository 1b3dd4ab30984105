// lt_nearest.hpp -- nearest-point queries over the resident scene (lt_nearest.hip; lt_hip_nearest_points in lt_capi.hip): the
// arithmetic of the definition in include/lenstrace_hip.h, shared by the kernel, by the host form (lt_hip_nearest_points_host) and,
// restated in numpy, by tests/nearest.py.  Every operation below is one IEEE float32 operation, rounded once, in the order
// written: the build contracts nothing (-ffp-contract=off), `/` is the correctly rounded quotient, subnormals are kept.  Only
// slot_bound fuses, and says so (__builtin_fmaf).  Compares with a NaN are false; no fmin / fmax, whose NaN rules differ between
// processors.
//
// The distance of a point P to a candidate (a leaf of the caller's tree with its one primitive) is
//     d2 = max(tri(P; A, e1, e2), box_d2(P; the leaf's box)),   a NaN tri staying a NaN,
// where (A, e1, e2) is the traversal triangle as the scene stores it (A, fl(B - A), fl(C - A)).  The true distance to a triangle
// is never below the true distance to a box that holds it, so the max only lifts an underestimate of a few ulp -- and makes
// d2 >= box_d2 hold IN FLOATS, which is all the walk's pruning needs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define LT_NEAR_HD __host__ __device__
#else
#define LT_NEAR_HD
#endif

namespace lt_nearest {

LT_NEAR_HD inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// A segment parameter held to [0, 1]; a NaN (a segment of no length: 0 / 0) counts as 0.
LT_NEAR_HD inline float unit_clamp(float t) {
  if (!(t > 0.0f)) t = 0.0f;
  if (t > 1.0f) t = 1.0f;
  return t;
}

// Squared length of ap - u e1 - v e2.
LT_NEAR_HD inline float residual2(float apx, float apy, float apz, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float u, float v) {
  const float rx = (apx - u * e1x) - v * e2x, ry = (apy - u * e1y) - v * e2y, rz = (apz - u * e1z) - v * e2z;
  return (rx * rx + ry * ry) + rz * rz;
}

// The closest point of the triangle A, A + e1, A + e2 to P as A + u e1 + v e2, and its squared distance.  Four candidates, each a
// point OF the triangle whatever the rounding, the first of the smallest d2 (by `<`) kept: the closest point of edge AB
// (u, v) = (t, 0), of edge AC (0, t), of edge BC (1 - t, t) -- t the projection's parameter held to [0, 1], so the vertices are the
// edges' ends -- and the foot of the perpendicular on the plane where its (u, v) lie inside (u >= 0, v >= 0, u + v <= 1).  The foot
// comes from e2's part at right angles to e1, g = e2 - k e1 with k = (e1.e2) / (e1.e1): v = (ap.g) / (g.g), u = (e1.ap) / (e1.e1) - v k
// -- no product of more than two lengths anywhere, so scenes of size 2^-40 and 2^40 neither underflow nor overflow.  A needle or
// a point triangle has a g of 0 or of rounding noise: the face candidate is then absent (a NaN fails the compares) or some point
// of the triangle, and the edges decide.  region: 0 a vertex (t was held), 1 an edge, 2 the face.
struct Tri { float d2, u, v; int region; };
LT_NEAR_HD inline Tri tri(float px, float py, float pz, float ax, float ay, float az, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
  const float apx = px - ax, apy = py - ay, apz = pz - az;
  const float a = dot3(e1x, e1y, e1z, e1x, e1y, e1z), b = dot3(e1x, e1y, e1z, e2x, e2y, e2z), c = dot3(e2x, e2y, e2z, e2x, e2y, e2z);
  const float d = dot3(e1x, e1y, e1z, apx, apy, apz), e = dot3(e2x, e2y, e2z, apx, apy, apz);
  // (the four parameter pairs first, then the four distances: what is written is the order of the compares, not of the arithmetic)
  const float qab = d / a;
  const float tab = unit_clamp(qab), tac = unit_clamp(e / c);     // edges AB, AC
  const float k = b / a;                                          // the face
  const float gx = e2x - k * e1x, gy = e2y - k * e1y, gz = e2z - k * e1z;
  const float vf = dot3(apx, apy, apz, gx, gy, gz) / dot3(gx, gy, gz, gx, gy, gz);
  const float uf = qab - vf * k;
  const float fx = e2x - e1x, fy = e2y - e1y, fz = e2z - e1z;     // edge BC: B + t (C - B)
  const float bpx = apx - e1x, bpy = apy - e1y, bpz = apz - e1z;
  const float tbc = unit_clamp(dot3(bpx, bpy, bpz, fx, fy, fz) / dot3(fx, fy, fz, fx, fy, fz));
  const float ubc = 1.0f - tbc;
  Tri r;
  r.u = tab; r.v = 0.0f;
  r.d2 = residual2(apx, apy, apz, e1x, e1y, e1z, e2x, e2y, e2z, tab, 0.0f);
  r.region = (tab > 0.0f && tab < 1.0f) ? 1 : 0;
  float d2 = residual2(apx, apy, apz, e1x, e1y, e1z, e2x, e2y, e2z, 0.0f, tac);
  if (d2 < r.d2) { r.d2 = d2; r.u = 0.0f; r.v = tac; r.region = (tac > 0.0f && tac < 1.0f) ? 1 : 0; }
  d2 = residual2(apx, apy, apz, e1x, e1y, e1z, e2x, e2y, e2z, ubc, tbc);
  if (d2 < r.d2) { r.d2 = d2; r.u = ubc; r.v = tbc; r.region = (tbc > 0.0f && tbc < 1.0f) ? 1 : 0; }
  if (uf >= 0.0f && vf >= 0.0f && uf + vf <= 1.0f) {
    d2 = residual2(apx, apy, apz, e1x, e1y, e1z, e2x, e2y, e2z, uf, vf);
    if (d2 < r.d2) { r.d2 = d2; r.u = uf; r.v = vf; r.region = 2; }
  }
  return r;
}

// Squared distance from P to the box [lo, hi]: per axis g = max(lo - p, p - hi, +0) (a NaN bound takes no part), then
// (g.x g.x + g.y g.y) + g.z g.z.  Rounding is monotone and this is one fixed expression, so the value for a box that encloses
// another is <= the other's, as floats.
LT_NEAR_HD inline float axis_gap(float lo, float hi, float p) {
  float g = 0.0f;
  const float below = lo - p, above = p - hi;
  if (below > g) g = below;
  if (above > g) g = above;
  return g;
}
LT_NEAR_HD inline float box_d2(float px, float py, float pz, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const float gx = axis_gap(lox, hix, px), gy = axis_gap(loy, hiy, py), gz = axis_gap(loz, hiz, pz);
  return (gx * gx + gy * gy) + gz * gz;
}

// d2 of a candidate: the larger of the two, a NaN tri staying a NaN (it is never accepted).
LT_NEAR_HD inline float candidate_d2(float tri_d2, float box) { return tri_d2 < box ? box : tri_d2; }

// The bound of a 4-wide group's child slot (lt_own16.hpp): its 16-bit box put back on the grid, qlo = fma(ql, S, O) and
// qhi = fma(qh, S, O) per axis -- ONE rounding each, so that O + ql S <= lo in reals gives qlo <= lo in floats (and qhi >= hi) --
// then box_d2's expression.  Hence slot_bound <= box_d2 of every leaf box beneath the slot.
// q: the slot's first three words (lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16); O, S: the grid's origin and step.
LT_NEAR_HD inline float slot_bound(uint32_t q0, uint32_t q1, uint32_t q2, const float* O, const float* S, float px, float py, float pz) {
  const float lx = __builtin_fmaf((float)(q0 & 0xffffu), S[0], O[0]), ly = __builtin_fmaf((float)(q0 >> 16), S[1], O[1]),
              lz = __builtin_fmaf((float)(q1 & 0xffffu), S[2], O[2]);
  const float hx = __builtin_fmaf((float)(q1 >> 16), S[0], O[0]), hy = __builtin_fmaf((float)(q2 & 0xffffu), S[1], O[1]),
              hz = __builtin_fmaf((float)(q2 >> 16), S[2], O[2]);
  return box_d2(px, py, pz, lx, ly, lz, hx, hy, hz);
}

// The running best of one point.  A candidate is accepted iff d2 < max_d2; among the accepted the smallest d2 wins, the lowest
// primitive offset among equal d2.  `t` starts as max_d2 with the bits given and is what a miss reports.
struct Best {
  float t, u, v;
  int32_t prim;   // -1: none yet
  LT_NEAR_HD void offer(float d2, float cu, float cv, int32_t p) {
    if (d2 < t || (d2 == t && prim >= 0 && p < prim)) { t = d2; u = cu; v = cv; prim = p; }
  }
  // Whether a subtree (or leaf) whose every candidate has d2 >= bound may still hold the answer.  Strict, so that ties stay reachable.
  LT_NEAR_HD bool reaches(float bound) const { return bound < t || (prim >= 0 && bound == t); }
};

// The order of a point's candidate sequence (lt_hip_nearest_k): ascending d2 by `<`, ascending primitive offset among equal d2.
// Whether the candidate {d2, p} comes before the list entry {ed2, ep}; ep = -1 is the miss entry {max_d2, -1}, which every
// accepted candidate (d2 < max_d2) comes before and nothing else does -- so the order is the acceptance too.  Best::offer is
// this with a list of one.  Equal d2 and equal offset: not before, i.e. behind what is there.
LT_NEAR_HD inline bool before(float d2, int32_t p, float ed2, int32_t ep) { return d2 < ed2 || (d2 == ed2 && ep >= 0 && p < ep); }

// KList::reaches from the list's last entry {lastD2, lastPrim}, for a walk that keeps that entry in registers.
LT_NEAR_HD inline bool last_reaches(float bound, float lastD2, int32_t lastPrim) { return bound < lastD2 || (lastPrim >= 0 && bound == lastD2); }

// The first k entries of a point's candidate sequence, sorted by `before`: entry j is the two words col[2 j STRIDE] (d2's bits) and
// col[(2 j + 1) STRIDE] (the primitive offset) -- the kernel's lists are columns of LDS rows (STRIDE = 64 lanes), the host form's
// an array (STRIDE = 1).  Empty entries are the miss entry.  u and v are not kept: tri() gives them again for the survivors.
template <int STRIDE>
struct KList {
  int* col;
  uint32_t k;   // 1 .. LT_NEAREST_MAX_K
  LT_NEAR_HD int d2_bits(uint32_t j) const { return col[2 * j * STRIDE]; }
  LT_NEAR_HD float d2(uint32_t j) const { return __builtin_bit_cast(float, col[2 * j * STRIDE]); }
  LT_NEAR_HD int32_t prim(uint32_t j) const { return col[(2 * j + 1) * STRIDE]; }
  LT_NEAR_HD void reset(float max_d2) {
    for (uint32_t j = 0; j < k; j++) { col[2 * j * STRIDE] = __builtin_bit_cast(int, max_d2); col[(2 * j + 1) * STRIDE] = -1; }
  }
  // Inserts from the end; the entry pushed past the end is dropped.  (Best::offer's signature: u and v are not kept.)
  LT_NEAR_HD void offer(float cd2, float, float, int32_t p) {
    uint32_t j = k;
    while (j > 0u) {
      const int eb = d2_bits(j - 1u);
      const int32_t ep = prim(j - 1u);
      if (!before(cd2, p, __builtin_bit_cast(float, eb), ep)) break;
      if (j < k) { col[2 * j * STRIDE] = eb; col[(2 * j + 1) * STRIDE] = ep; }
      j--;
    }
    if (j < k) { col[2 * j * STRIDE] = __builtin_bit_cast(int, cd2); col[(2 * j + 1) * STRIDE] = p; }
  }
  // Whether a subtree (or leaf) whose every candidate has d2 >= bound may still hold one of the first k: while the list is not
  // full (its last entry is the miss entry), bound < max_d2; once it is, bound <= the k-th d2 -- equality stays reachable, a
  // lower offset at the same d2 displaces the k-th entry.  Best::reaches with the k-th best.
  LT_NEAR_HD bool reaches(float bound) const { return last_reaches(bound, d2(k - 1u), prim(k - 1u)); }
};

// The length of the whole sequence: the candidates within the radius.
struct KCount {
  float max_d2;
  uint32_t n;
  LT_NEAR_HD void offer(float cd2, float, float, int32_t) { if (cd2 < max_d2) n++; }
  LT_NEAR_HD bool reaches(float bound) const { return bound < max_d2; }
};

// A record of a radius list (lt_hip_nearest_list): lt_hip_hit's four words.  The ordering of a segment (lt_overlist.hip) and the
// host form sort by this alone: two records of one point with equal d2 and equal offset come from the same tri() on the same
// operands and are bit-identical, so the multiset sorted by (d2, offset) IS the sequence; accepted d2 are never NaN.
struct Record { float d2; int32_t prim; float u, v; };
LT_NEAR_HD inline bool record_before(const Record& a, const Record& b) { return before(a.d2, a.prim, b.d2, b.prim); }

// A point that needs no walk: a component that is not finite, or a max_d2 nothing is below (0, -0, negative, NaN).
LT_NEAR_HD inline bool no_walk(float px, float py, float pz, float max_d2) {
  const float inf = __builtin_inff();
  return !(__builtin_fabsf(px) < inf && __builtin_fabsf(py) < inf && __builtin_fabsf(pz) < inf) || !(max_d2 > 0.0f);
}

}  // namespace lt_nearest

#if defined(__HIPCC__) || defined(__HIP__)
#include "lt_device.hpp"

namespace lt_nearest {

// The caller's records as the kernel reads them: 16 bytes per point (p.xyz, max_d2) -- lt_hip_point -- and 16 bytes per result
// (d2, primitive or -1, u, v) -- lt_hip_hit.
struct Params {
  const float4* points;
  uint4* hits;
  uint32_t n;
  uint32_t* next;     // the work counters: eight, kQueueStride dwords apart, zeroed by launch() on the call's stream
  uint32_t refill;    // idle lanes that make a wave take new points
};

// Enqueues lt_nearest_kernel on `s`.  Returns the first HIP error.
hipError_t launch(const lt::SceneDev& sc, const Params& p, uint32_t cuCount, hipStream_t s);

constexpr uint32_t kMaxK = 8;   // LT_NEAREST_MAX_K

// LT_NEAREST_FIRST_K, LT_NEAREST_COUNT, and the two kinds of the radius lists (lt_hip_nearest_list; lt_overlist.hpp), which no
// descriptor names: kList, the whole sequence into the point's segment of `items`; kCountWide, kCount as one uint64 per point.
enum Kind { kFirstK = 0, kCount = 1, kList = 2, kCountWide = 3 };

// lt_hip_nearest_k: the first maxK entries of each point's candidate sequence as maxK lt_hip_hit records per point, or -- kCount --
// the sequence's length, one uint32 per point.  kCountWide writes that length as one uint64 into offsets[i].  kList writes
// neither `hits` nor `counts`: point i's accepted candidates go, in walk order, to items[offsets[i] .. min(offsets[i + 1], capacity))
// as {d2, prim, u, v}, and whatever is beyond that is dropped.
struct KParams {
  const float4* points;
  uint4* hits;        // kFirstK: [n * maxK], point-major
  uint32_t* counts;   // kCount: [n]
  uint32_t n;
  uint32_t maxK;      // kFirstK: 1 .. kMaxK; else 0
  uint32_t* next;
  uint32_t refill;
  uint32_t kind;
  uint32_t oneShot;   // kList: the offsets are this stream's own scan -- when offsets[n] > capacity the launch writes nothing
  unsigned long long* offsets;   // kCountWide: written, n words; kList: read, n + 1 words
  uint4* items;                  // kList: `capacity` records
  unsigned long long capacity;
};

// Enqueues lt_nearest_k_kernel on `s`.  Returns the first HIP error.
hipError_t launch_k(const lt::SceneDev& sc, const KParams& p, uint32_t cuCount, hipStream_t s);

}  // namespace lt_nearest
#endif
