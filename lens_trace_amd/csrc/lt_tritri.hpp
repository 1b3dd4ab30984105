// lt_tritri.hpp -- triangle-overlap queries over the resident scene (lt_tritri.hip; lt_hip_overlap_tris in lt_capi.hip): the
// arithmetic of the definition in include/lenstrace_hip.h, shared by the kernel, by the host form (lt_hip_overlap_tris_host) and,
// restated in numpy, by tests/overlap_tris.py.  The rules are lt_overlap.hpp's: every operation below is one IEEE float32
// operation, rounded once, in the order written (-ffp-contract=off), subnormals are kept, compares with a NaN are false, minima
// and maxima are that header's chains of compares.
//
// A candidate (a leaf of the caller's tree with its one primitive) touches a query triangle (P, Q, R) iff
//     boxes_meet(qbox, the leaf's own box)  and  tri_meets_tri(P, Q, R; A, e1, e2),
// where qbox is the query's bounding box (query_box) and (A, e1, e2) the traversal triangle as the scene stores it.  The walk
// prunes with boxes_meet alone, as the box queries do.
#pragma once
#include "lt_overlap.hpp"

namespace lt_tritri {

using lt_overlap::max3;
using lt_overlap::min3;

struct Vec { float x, y, z; };

LT_OV_HD inline Vec sub(const Vec& a, const Vec& b) { return Vec{a.x - b.x, a.y - b.y, a.z - b.z}; }
LT_OV_HD inline Vec add(const Vec& a, const Vec& b) { return Vec{a.x + b.x, a.y + b.y, a.z + b.z}; }
LT_OV_HD inline Vec cross(const Vec& a, const Vec& b) { return Vec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
LT_OV_HD inline float dot(const Vec& a, const Vec& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
LT_OV_HD inline bool finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

// A query that meets nothing: one of its nine coordinates is not finite.  A needle and a point (P = Q = R) are valid.
LT_OV_HD inline bool empty_tri(const Vec& P, const Vec& Q, const Vec& R) {
  return !(finite(P.x) && finite(P.y) && finite(P.z) && finite(Q.x) && finite(Q.y) && finite(Q.z) && finite(R.x) && finite(R.y) && finite(R.z));
}

// The query's box: per axis min3 / max3 of P, Q, R in that order.
LT_OV_HD inline void query_box(const Vec& P, const Vec& Q, const Vec& R, float* lo, float* hi) {
  lo[0] = min3(P.x, Q.x, R.x); lo[1] = min3(P.y, Q.y, R.y); lo[2] = min3(P.z, Q.z, R.z);
  hi[0] = max3(P.x, Q.x, R.x); hi[1] = max3(P.y, Q.y, R.y); hi[2] = max3(P.z, Q.z, R.z);
}

LT_OV_HD inline Vec neg(const Vec& a) { return Vec{-a.x, -a.y, -a.z}; }

// The test reads its operands from a table of nine vectors, by row, so that one loop with one body walks the 17 axes and the
// kernel can keep the table in LDS and index it with the loop's counter.  Rows 0 .. 4 are the query's own terms,
// computed once per query and held; rows 5 .. 8 are the scene triangle's, computed once per candidate.
//   0  P                       5  f0 = e1
//   1  h0 = g1 = Q - P         6  f1 = e2 - e1
//   2  h1 = g2 - g1            7  f2 = -e2
//   3  h2 = -g2, g2 = R - P    8  n = cross(e1, e2)
//   4  m = cross(g1, g2)
// (g2 and e2 are read back as -h2 and -f2: a negation is exact.)  A table is anything with Vec row(int) const and
// void put(int, const Vec&); Table is the one in plain memory.
enum Row { kP = 0, kH0 = 1, kM = 4, kF0 = 5, kN = 8, kRows = 9, kQueryRows = 5 };
struct Table {
  Vec v[kRows];
  LT_OV_HD Vec row(int i) const { return v[i]; }
  LT_OV_HD void put(int i, const Vec& a) { v[i] = a; }
};
template <class T>
LT_OV_HD inline void put_query(T& t, const Vec& P, const Vec& Q, const Vec& R) {
  const Vec g1 = sub(Q, P), g2 = sub(R, P);
  t.put(kP, P); t.put(kH0, g1); t.put(kH0 + 1, sub(g2, g1)); t.put(kH0 + 2, neg(g2)); t.put(kM, cross(g1, g2));
}
template <class T>
LT_OV_HD inline void put_scene(T& t, const Vec& e1, const Vec& e2) {
  t.put(kF0, e1); t.put(kF0 + 1, sub(e2, e1)); t.put(kF0 + 2, neg(e2)); t.put(kN, cross(e1, e2));
}

// Axis k of the 17, in the definition's order: n; m; the nine cross(f_i, h_j), i-major; cross(n, f_i); cross(m, h_j).
template <class T>
LT_OV_HD inline Vec axis(const T& t, int k) {
  if (k == 0) return t.row(kN);
  if (k == 1) return t.row(kM);
  if (k < 11) return cross(t.row(kF0 + (k - 2) / 3), t.row(kH0 + (k - 2) % 3));
  if (k < 14) return cross(t.row(kN), t.row(kF0 + (k - 11)));
  return cross(t.row(kM), t.row(kH0 + (k - 14)));
}

// Whether axis `a` separates.  Everything is seen from P: the scene's vertices s0 = A - P, s1 = s0 + e1, s2 = s0 + e2 give
// ps = (a.s0, a.s1, a.s2), the query's +0, g1, g2 give pq = (+0, a.g1, a.g2); separated iff min3(ps) > max3(pq) or
// max3(ps) < min3(pq), and all five dot products are finite.  A separating axis proves the triangles apart whatever its
// direction, so a cross product that lost bits, or underflowed to zero (every projection 0: nothing separates), costs sharpness
// only.  One that overflowed does not: its projections are inf or NaN, the compare chains keep their first operand against a NaN,
// and the finiteness test is what makes "separates nothing" true of it.
LT_OV_HD inline bool axis_separates(const Vec& a, const Vec& s0, const Vec& s1, const Vec& s2, const Vec& g1, const Vec& g2) {
  const float p0 = dot(a, s0), p1 = dot(a, s1), p2 = dot(a, s2), q1 = dot(a, g1), q2 = dot(a, g2);
  const bool apart = min3(p0, p1, p2) > max3(0.0f, q1, q2) || max3(p0, p1, p2) < min3(0.0f, q1, q2);
  return apart && finite(p0) && finite(p1) && finite(p2) && finite(q1) && finite(q2);
}

// The 17-axis test on a table whose query rows are put (put_query): puts the scene's rows, then walks the axes and stops at the
// first that separates.  Every axis is a pure function of the operands, so the verdict does not depend on where the walk stops.
// If P equals a vertex of the scene's triangle bit for bit, that vertex's s is 0 exactly (s1 = fl(fl(A - B) + fl(B - A))), both
// projection sets hold 0 on every axis and nothing separates.
template <class T>
LT_OV_HD inline bool tri_meets_tri(T& t, const Vec& A, const Vec& e1, const Vec& e2) {
  put_scene(t, e1, e2);
  const Vec s0 = sub(A, t.row(kP)), s1 = add(s0, e1), s2 = add(s0, e2);
  const Vec g1 = t.row(kH0), g2 = neg(t.row(kH0 + 2));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int k = 0; k < 17; k++)
    if (axis_separates(axis(t, k), s0, s1, s2, g1, g2)) return false;
  return true;
}

}  // namespace lt_tritri

#if defined(__HIPCC__) || defined(__HIP__)

namespace lt_tritri {

// The caller's records as the kernel reads them: 48 bytes per triangle (a.xyz, pad, b.xyz, pad, c.xyz, pad) -- lt_hip_tri -- and
// per triangle maxK int32 offsets (kFirstK) or one uint32 (kCount, kAny): lt_overlap::Params with `boxes` naming the triangles.
// Enqueues lt_overlap_tris_kernel<kind> (or the scan kernel, for a scene without an own tree) on `s`.  Returns the first HIP error.
hipError_t launch(const lt::SceneDev& sc, const lt_overlap::Params& p, uint32_t cuCount, hipStream_t s);

}  // namespace lt_tritri
#endif
