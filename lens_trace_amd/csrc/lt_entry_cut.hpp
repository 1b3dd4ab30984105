// lt_entry_cut.hpp -- the entry cut of a square's shadow walks (lt_entry_cut_kernel in lt_kernel.hpp; LT_ASM_WALK2's prologue in
// lt_walk_asm.hpp): the interval test that says which nodes of the own tree the shadow rays of a square's stored camera hits can
// reach at all, whatever the frame.  Compiled for the device (the kernel) and for the host (tests/test_entry_cut_cpu.py holds it
// against a float32 restatement of the reference's slab test).  Every operation below is one IEEE float32 operation, rounded once,
// in the order written (-ffp-contract=off); compares with a NaN are false, and every exclusion below needs a compare to be TRUE,
// so a NaN never excludes.
//
// The ray set of a lane.  The lane's camera hit has the position o (shade_lighting2's `position`, the same bits).  In any frame its
// shadow ray is  d = normalize4(fl(l - o)),  l = bary3(light primitive, barycentrics(u, v)),  with u, v, 1 - u - v in [0, 1] and
// the primitive one of the light list's.  L = [Llo, Lhi] is the box of all light primitives' vertices pushed outwards by
// 2^-14 max|bound| + 2^-100 per axis (light_box_pad): a convex combination of three vertices evaluated in floats (two fmas and a
// product, or three products and two sums, weights within an ulp of summing to 1) leaves the vertices' box by less than
// 8u max|vertex| (u = 2^-24), so l lies in L.  The set is  { o + s w : s >= 0, w_a in [Llo_a - o_a, Lhi_a - o_a] for every axis a },
// unbounded beyond the light (the slab test has no tmax).
//
// The interval test of a box A = [lo, hi] (may_reach), per axis a, R = 2^-16:
//     pad = R (max(|lo_a|, |hi_a|) + |o_a|) + 2^-100,  slo = fl(lo_a - pad),  shi = fl(hi_a + pad)        (the slab, pushed outwards)
//     wl = fl(fl(Llo_a - o_a) - m), wh = fl(fl(Lhi_a - o_a) + m'), m = R (|Llo_a| + |o_a|) + 2^-100, m' likewise   (lane_set)
//     where the ray enters:  o_a in [slo, shi]: at 0;  o_a < slo: wh > 0 or the box is excluded, at (slo - o_a) / wh;
//                            o_a > shi: wl < 0 or the box is excluded, at (o_a - shi) / -wl
//     where it leaves, wherever the origin is:  wl > 0 (every direction goes up): at (shi - o_a) / wl;  wh < 0: at
//                            (o_a - slo) / -wh;  else (some direction stays): never, inf
//     S_a = [enters, leaves]
//   each quotient one float division, then the lower bounds times (1 - 4R) minus 2^-100, the upper bounds times (1 + 4R) plus
//   2^-100; the box is excluded iff max_a lower(S_a) > min_a upper(S_a).
//
// CLAIM.  Let the lane be one that lane_set accepts (o and L finite, below 2^40 in magnitude), let its ray (o, d) be one that
// traverse_shadow2 sends through a packet walk (inv_a = 1.0f / d_a finite, |inv_a| < 2^60: packet_ray_ok), let B be a leaf's own
// box and A any box with A.lo_a <= B.lo_a and B.hi_a <= A.hi_a as floats -- an ancestor's box, or the pushed-out copy of it in a
// pair record.  If the ray passes the reference's slab test of B,
//     tn_a = fl(fl(near_a - o_a) inv_a),  tf_a = fl(fl(far_a - o_a) inv_a),  T = min_a tf_a >= t* = max(max_a tn_a, 0+),
// (near_a = B.lo_a where inv_a > 0, else B.hi_a; 0+ the smallest positive float) then may_reach(A) is true.
//
// PROOF.  normalize4 multiplies every component of p = fl(l - o) by ONE float, after scaling p by a power of two at most: d_a =
// fl(q p_a) for a common real q > 0.  |d_a| > 2^-61, so none of these products underflowed and d_a = q p_a (1 + e1), |e1| <= u;
// p_a = (l_a - o_a)(1 + e2), of the sign of l_a - o_a; inv_a = (1 + e3) / d_a with |e3| <= 4u whichever division the math flavour
// has.  Put s = t* q, a positive real, ONE number for the three axes, and w_a = l_a - o_a, which lies in [Llo_a - o_a, Lhi_a - o_a].
// We show o_a + s w_a in [slo, shi] for every axis, i.e. s in every S_a as a set of reals:
//   * o_a in [slo, shi] as floats: S_a begins at 0.  Its end, where wl > 0 (then w_a > 0, d_a > 0, inv_a > 0, far_a = B.hi_a): h =
//     B.hi_a - o_a is not negative -- else tf_a, a negative or zero float times a positive one, were at most -0 and T below 0+ --
//     and t* <= T <= tf_a <= fl(h) inv_a (1 + u) + 2^-149 (fl(h) is within u of h, and exact where subnormal), hence
//     s w_a <= h (1 + 9u) + 2^-147 <= A.hi_a - o_a + 9u (|hi_a| + |o_a|) + 2^-147 <= shi - o_a (the 2^-100 in pad), and
//     s <= (shi - o_a) / w_a <= (shi - o_a) / wl.  Where wh < 0: the mirror image.
//   * o_a < slo.  Then g = B.lo_a - o_a >= A.lo_a - o_a >= pad (1 - 2u) - u |lo_a| > 2^-101, and fl(g) is a normal positive float.
//     Were inv_a < 0, tf_a = fl(fl(B.lo_a - o_a) inv_a) would be at most -2^-102 (|inv_a| > 1/2), T negative, and the test failed.
//     So inv_a > 0, d_a > 0, w_a > 0, near_a = B.lo_a, and from tn_a <= t*:  g (1 + e)(1 + e') inv_a <= t*  (no underflow: the
//     product is above 2^-102), hence g <= t* d_a (1 + 7u) <= s w_a (1 + 9u) and
//         s w_a >= g - 9u g >= A.lo_a - o_a - 9u (|lo_a| + |o_a|) >= slo - o_a,
//     as slo <= lo_a - pad (1 - u) + u |lo_a| and pad >= 250u (|lo_a| + |o_a|).  From t* <= T <= tf_a with h = B.hi_a - o_a >= g
//     in the same way s w_a <= h (1 + 9u) <= A.hi_a - o_a + 9u (|hi_a| + |o_a|) <= shi - o_a.  And wh >= Lhi_a - o_a >= w_a > 0
//     (m' outweighs the two roundings of wh), so the axis does not exclude the box.
//   * o_a > shi: the mirror image (inv_a < 0, near_a = B.hi_a).
// So the real intervals S_a (over the real quotients) share the point s.  The floats: wh is at least and wl at most the real bound
// of w_a, so (slo - o_a) / wh is at most, and (shi - o_a) / wl -- taken only when wl > 0, which makes the real bound positive
// too -- at least the real end of S_a; the subtraction and the division round by 3u in all, far inside 4R; a quotient that
// underflows is off by at most 2^-149, inside the 2^-100; one that overflows to +inf stands for a real above 2^127, which every
// finite upper bound is below.  Hence lower(S_a) <= s <= upper(S_a) for every a and the box is not excluded.  QED
//
// With the nesting argument of lt_retree.hpp and the conservative interior test of lt_walk_asm.hpp this gives what the walks need.
// The cut is built by replacing a node by those of its children that some casting lane of the square may reach, so a leaf that is
// below no entry of the list has an ancestor that no lane may reach, and by the claim no lane's ray, in any frame, passes the slab
// test of that leaf's own box: no lane accepts a hit there in a walk from the root either.  A leaf below an entry E is reached
// from E as it is from the root: the tests between E and the leaf are the same.  The accepts are decided by the same exact tests
// of the same leaves, and an any-hit caller reads nothing else.
// What the claim does NOT cover gets the empty list (start at the root): a non-finite or huge origin or light box, no light, a
// light sample whose index falls on the list's zero tail (index == count: shade_lighting2 looks at its own samples and drops the
// list for that work item), a stack that could overflow (entry_cut_limit).
//
// Chunks.  A square's list may be longer than one record holds: it is then cut into up to `chunks` records of at most
// entry_cut_limit entries each (chunk_count, chunk_entries), chunk c in plane c of the buffer, and packet_walk2 runs the walk once
// per chunk (a list of leaves up to `chunks` records, a list of nodes up to the smaller nodeChunks), each time from an empty stack, with the lanes still open after the chunk before (it stops when none is).  The argument
// above goes through per chunk: every leaf that some ray of the square could be accepted in lies below an entry of exactly one
// chunk, and the walk of that chunk reaches it from that entry as a walk from the root would -- the tests between the entry and
// the leaf are the same.  A lane that an earlier chunk closed found an accepted hit there, which a walk from the root finds too (in
// another order); a lane open to the end was accepted in no leaf below any entry.  The accepts are those of the same leaves under
// the same tests in another order, and an any-hit caller reads nothing else.  Word 0 of every chunk after the first is a plain
// count, 0 .. limit, written for every square by every build: 0 ends the list, and a chunk of count 0 is never handed to a walk
// (nor is a word that is no count, 1 .. kCut: packet_walk2 ends the list there).
//
// The cut over the pruned tree.  Where the leaf pass (lt_entry_cut_kernel) finishes -- it has visited every record that some casting
// lane may reach and tested every leaf among them -- but more leaves survive than a list holds, the square's list is a cut of the
// tree AS THE PASS SAW IT (pruned_cut_select over the records the pass wrote down): an interior record below which no leaf survived
// is dropped, a surviving leaf stands for itself, and the cut is deepened shallowest first as the node cut is.  It leans on the
// claim that justifies the lists of leaves: no ray of the square is accepted in a leaf that did not survive -- a leaf the pass did
// not visit has an ancestor that no casting lane may reach (the first claim), a leaf it visited and dropped accepts no ray of the
// square (the second) -- so every leaf in which some ray could be accepted is a surviving leaf, lies below exactly one entry of
// the cut (pruned_mark marks every record above a survivor, and an entry is replaced by ALL its marked children or not at all), and
// is reached from that entry by the same tests as from the root.  A pass that does not finish, or one that visits more records
// than are written down (kPruneRecords), knows no such tree: the square keeps the node cut chosen by box reach.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define LT_EC_HD __host__ __device__
#else
#define LT_EC_HD
#endif

#ifndef LT_ENTRY_CUT_K
#define LT_ENTRY_CUT_K 15
#endif

namespace lt_entry_cut {

constexpr int kCut = LT_ENTRY_CUT_K;   // entries of a list at most; a list's 64 bytes hold a count and up to 15 references
static_assert(kCut >= 2 && kCut <= 15, "a list is one count and at most 15 references");
constexpr int kListWords = 16;
// Word 0 of a list is its count, 0 .. kCut, or kClearMark: no leaf of the tree can occlude a shadow ray of the square (the leaf pass
// of lt_entry_cut_kernel; may_accept below), so its two-frame walks are not run at all (traverse_shadow2 -- the mark never reaches
// a walk, which would take it for a count).
constexpr unsigned kClearMark = 0xffffffffu;

constexpr float kRel = 0x1p-16f;       // R
constexpr float kAbs = 0x1p-100f;
constexpr float kLightRel = 0x1p-14f;
constexpr float kMaxMagnitude = 0x1p+40f;

// The walk's stack register has 64 slots: 2 * height + 2 under the deepest path from the root (lt_walk_asm.hpp), and the entries
// of the list wait below whichever subtree is being walked.  So a scene's lists hold at most entry_cut_limit entries: kCut, fewer
// under a high tree, and below 2 there is nothing to build.
LT_EC_HD inline int entry_cut_limit(int ownHeight) {
  if (ownHeight < 0) return 0;
  const int room = 64 - (2 * ownHeight + 2);
  const int limit = room < kCut ? room : kCut;
  return limit >= 2 ? limit : 0;
}

// A list of `entries` references in chunks of at most `limit` (entry_cut_limit's, 0: no lists), at most kMaxChunks of them: every
// chunk but the last is full.
constexpr int kMaxChunks = 16;
constexpr int kDefaultChunks = 16;  // LT_ENTRY_CUT_CHUNKS unset (1, 2, 4, 8, 12 and 16 timed on the 1 M-triangle wall)
// LT_ENTRY_CUT_NODE_CHUNKS unset: a list of NODES takes no more records than this.  A deeper cut by box reach alone is not always
// a better one -- every entry is a record fetched and two boxes tested by every work item, where a node higher up lets the rays
// themselves cull both -- DESIGN 5.1: the colonnade gains with 2 and loses with 4 and 8, the wall gains with all.
constexpr int kDefaultNodeChunks = 2;
constexpr int kMaxEntries = kMaxChunks * kCut;
LT_EC_HD inline unsigned chunk_capacity(unsigned limit, unsigned chunks) {   // the entries a square's list may have
  const unsigned c = chunks < 1u ? 1u : chunks > (unsigned)kMaxChunks ? (unsigned)kMaxChunks : chunks;
  return limit * c;
}
LT_EC_HD inline unsigned chunk_count(unsigned entries, unsigned limit) { return limit == 0u ? 0u : (entries + limit - 1u) / limit; }
LT_EC_HD inline unsigned chunk_entries(unsigned entries, unsigned limit, unsigned chunk) {   // the count of chunk `chunk`
  const unsigned first = chunk * limit;
  return entries <= first ? 0u : entries - first < limit ? entries - first : limit;
}

// One axis of the light primitives' vertex box, pushed outwards (in place).
LT_EC_HD inline void light_box_pad(float& lo, float& hi) {
  const float alo = __builtin_fabsf(lo), ahi = __builtin_fabsf(hi);
  const float m = (alo > ahi ? alo : ahi) * kLightRel + kAbs;
  lo = lo - m;
  hi = hi + m;
}

struct LaneSet {
  float o[3];
  float wl[3], wh[3];   // w_a in [wl, wh], rounded outwards
};

// False: the claim does not cover this lane (the square then starts at the root).
LT_EC_HD inline bool lane_set(float ox, float oy, float oz, const float (&Llo)[3], const float (&Lhi)[3], LaneSet& ls) {
  ls.o[0] = ox; ls.o[1] = oy; ls.o[2] = oz;
  bool ok = true;
  for (int a = 0; a < 3; a++) {
    const float o = ls.o[a], ao = __builtin_fabsf(o);
    ok = ok && ao < kMaxMagnitude && __builtin_fabsf(Llo[a]) < kMaxMagnitude && __builtin_fabsf(Lhi[a]) < kMaxMagnitude && Llo[a] <= Lhi[a];
    ls.wl[a] = (Llo[a] - o) - ((__builtin_fabsf(Llo[a]) + ao) * kRel + kAbs);
    ls.wh[a] = (Lhi[a] - o) + ((__builtin_fabsf(Lhi[a]) + ao) * kRel + kAbs);
  }
  return ok;
}

// The interval test: false only if no half-line of the lane's ray set meets the box [lo, hi].
LT_EC_HD inline bool may_reach(const LaneSet& ls, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const float lo[3] = {lox, loy, loz}, hi[3] = {hix, hiy, hiz};
  const float inf = __builtin_inff();
  float tLo = 0.0f, tHi = inf;
  for (int a = 0; a < 3; a++) {
    const float o = ls.o[a], alo = __builtin_fabsf(lo[a]), ahi = __builtin_fabsf(hi[a]);
    const float pad = ((alo > ahi ? alo : ahi) + __builtin_fabsf(o)) * kRel + kAbs;
    const float slo = lo[a] - pad, shi = hi[a] + pad;
    float lower = 0.0f, upper = inf;
    if (o < slo) {
      if (ls.wh[a] <= 0.0f) return false;
      lower = ((slo - o) / ls.wh[a]) * (1.0f - 4.0f * kRel) - kAbs;
    } else if (o > shi) {
      if (ls.wl[a] >= 0.0f) return false;
      lower = ((o - shi) / -ls.wl[a]) * (1.0f - 4.0f * kRel) - kAbs;
    }
    if (ls.wl[a] > 0.0f) upper = ((shi - o) / ls.wl[a]) * (1.0f + 4.0f * kRel) + kAbs;            // (o <= shi here)
    else if (ls.wh[a] < 0.0f) upper = ((o - slo) / -ls.wh[a]) * (1.0f + 4.0f * kRel) + kAbs;     // (o >= slo here)
    if (lower > tLo) tLo = lower;
    if (upper < tHi) tHi = upper;
  }
  return !(tLo > tHi);
}

// ---- The triangle test (may_accept): which LEAVES the lane's rays can be occluded by.  A leaf's own box contains or touches the
// origins of a square that lies on its neighbours, so no box test removes it; the triangle itself does.
//
// The walk's leaf (LT_ASM_TRI2_*, leaf2_frame; the reference's intersect_triangle_data) of the traversal triangle (A, e1 = v0v1,
// e2 = v0v2) and a ray (o, d), T = fl(o - A) -- ONE subtraction per axis, the same in every flavour, and the T of this file:
//     det^ = e1 . (d x e2),  U^ = T . (d x e2),  V^ = d . (T x e1),  inv^ = 1 / det^  (a division, or the as-shipped rcp),
//     u^ = fl(U^ inv^),  v^ = fl(V^ inv^);  accepted only if  !(|det^| < 1e-4), !(u^ < 0), !(u^ > 1), !(v^ < 0), !(fl(u^ + v^) > 1),
// then t^ = fl(N^ inv^) < tmax, N^ = e2 . (T x e1), and the leaf's own slab test.  There is NO test of t^ > 0: a triangle behind the
// origin occludes.  So the ray counts as the whole LINE through o along d up to tmax, and nothing below looks at the slab or at
// the 1e-4 gate: leaving a test out only keeps more.  tmax is shade_lighting2's: fl((double)dist^ - 0.01), dist^ = distance4(o, l)
// within 8u of |l - o| in every flavour (a difference, three squares, two sums: 5u under the root, which halves it; the root 2u).
// Without it no square were ever clear: the shaft ends on the light's own triangles.  As functions of the direction the three
// numerators are LINEAR and N does not depend on it:  for any real vector w
//     D(w) = w . cD,  U(w) = w . cU,  V(w) = w . cV,  N = e2 . cV,   cD = e2 x e1,  cU = e2 x T,  cV = T x e1   (scalar triple products),
// and a linear function over the box W = [wl, wh] of lane_set takes its extremes at corners: min f = sum_a min(c_a wl_a, c_a wh_a).
//
// What is rounded, u = 2^-24.  Write S_f(w) = sum over the six products x_i y_j w_k of f of their magnitudes (S_D: e2, e1; S_U: e2,
// T; S_V: T, e1; S_N: the products of N, no w), S_f = its largest value over W = sum_a M_a P_a with M_a = max(|wl_a|, |wh_a|) and P the cross product of the
// magnitudes with a plus.
//   (a) The walk.  Every product of det^, U^, V^ passes at most five roundings whatever the flavour -- the product inside the cross
//       product, its difference, the product with the third vector, two additions; a contracted form (fma) has fewer, the order of
//       the additions does not matter to the bound, dot4's `w` terms are exact zeros -- so |f^ - f(d)| <= 5.01 u S_f(d), plus at most
//       sixteen flushed or subnormal results of 2^-126 each times a factor, below 2^-121 (1 + |T|_1 + |e1|_1 + |e2|_1).
//       inv^ = (1 + e) / det^ with |e| <= 4u in either flavour, and the product with it rounds once more: u^ det^ = U^ (1 + e'),
//       |e'| <= 5.01 u (and 2^-126 |det^| where it underflows), v^ likewise.
//   (b) This file (-ffp-contract=off: one rounding per operation).  A component of cD, cU, cV: two products and a difference, off by
//       at most 2.01 u P_a; the combined vectors cU - cD and cU + cV - cD: one and two more roundings of at most the sum of the
//       magnitudes; the range sum: a product and two additions, 3.01 u sum_a |c_a| M_a.  In all below 8 u (S_U + S_V + S_D) for every
//       range used, plus underflows of 2^-126 each, at most 2^-122 (1 + M_1).
//   (c) The direction.  As in the proof above d_a = q w''_a for ONE real q > 0, w''_a = (l_a - o_a)(1 + e1)(1 + e2), which differs from
//       w_a = l_a - o_a by at most 2.01 u |w_a| towards or away from 0, and wl / wh keep (R - 3u)(|L_a| + |o_a|) >= 2.01 u |w_a| of
//       their margin after their own roundings: w'' lies in W.  |d| is within 4u of 1, so q >= 0.99 / M_1.
// With G = 64 u = 2^-18 and Z = 2^-100 (1 + M_1 (1 + |cD|_1 bound P_D,1 + |T|_1 + |e1|_1 + |e2|_1)) every test below compares a range
// bound with a margin  m_f = G S_f + Z  (S over the functions the range is made of).  G is (a) + (b) + the slack of the `> 1` tests
// with room to spare (the largest sums: for u + v 11.1 u + 8 u, for t 30.5 u + 16 u); Z times q >= 0.99 Z / M_1 outweighs every absolute term of (a), and
// Z every one of (b).
//
// CLAIM.  Let the lane be one that lane_set accepts and its ray (o, d) one that traverse_shadow2 sends through a packet walk, as in
// the claim above.  If the ray passes the float triangle test of the traversal triangle (A, e1, e2) in any flavour, t^ < tmax included, may_accept is true.
//
// PROOF.  Suppose may_accept is false.  Then its values are finite and below 2^40 and one sign s holds for D: the computed range of
// D lies beyond m_D on one side, so by (b) s D(w) > (G - 8u) S_D + Z' for every w in W, in particular for w'' (c), and
// s D(d) = q s D(w'') > q (56 u S_D(w'') + Z') >= 5.01 u S_D(d) + (the absolute term of (a)): det^ is not zero and has the sign s.
// Say s = + (else negate cD, cU, cV: the code does, and every statement below mirrors).  One of five holds:
//   * U < -m_U over W.  Then U^ <= U(d) + 5.01 u S_U(d) + abs < -q (56 u S_U + Z') + ... < 0, and by the absolute part of Z
//     |U^| > 2^-101 q (1 + P_D,1) M_1 >= 2^-102 |det^|, so U^ inv^, a negative number of magnitude above 2^-103, does not round to -0:
//     u^ < 0 and the ray is rejected.   * V < -m_V: the same for v^.
//   * U - D > m over W (m of U and D).  Then U^ (1 - 5.01 u) - det^ >= U(d) - D(d) - 10.1 u (S_U(d) + S_D(d)) - abs > 2u det^ (as
//     det^ <= 1.01 S_D(d)), so U^ inv^ (1 + e') >= 1 + 2u, a float, and rounding is monotone: u^ >= 1 + 2u > 1, rejected.
//   * U + V - D > m over W (m of all three).  (u^ + v^) det^ >= U^ + V^ - 5.01 u (|U^| + |V^|) - 2^-125 det^ >= U(d) + V(d) -
//     10.1 u (S_U(d) + S_V(d)) - abs, and that exceeds (1 + 2u) det^ <= D(d) + 8.1 u S_D(d) by the margin: u^ + v^ >= 1 + 2u as reals,
//     fl(u^ + v^) >= 1 + 2u > 1 (also when the sum was contracted into an fma: one rounding fewer), rejected.
//   * N - max D + k min D > m over W (m of N and D), k = min(1, 0.0098 / M_1) <= 0.0099 / |w''|: the plane is met beyond the light
//     point, or less than 0.01 in front of it.  t^ det^ >= N^ (1 - 5.01 u) >= N - 10.1 u S_N and det^ <= D(d) + 5.01 u S_D(d), so with
//     1 / q = |w''| / |d| >= (1 - 4u) |w''|:  t^ >= (1 - 4u) |w''| X,  X = (N - 10.1 u S_N) / (D(w'') + 5.01 u S_D(w'')).  And
//     tmax <= (1 + 9.1 u) |l - o| - 0.0099 <= (1 + 11.2 u) |w''| - 0.0099.  So t^ >= tmax follows from X >= 1 + 15.3 u - k, i.e. from
//     N - D(w'') >= -k D(w'') + 10.1 u S_N + 20.4 u S_D, and that from the range: D(w'') lies between min D and max D, the computed
//     ones are off by 8 u S_D each and N by 8 u S_N (b), k <= 1:  46.5 u in all.  t^ < tmax is false, rejected.
// In every case the ray does not pass.  QED.  Every exclusion needs a compare to be TRUE: a NaN or an infinity (a margin that
// overflows) excludes nothing, and a D whose range contains 0 -- among them every lane whose light box contains its origin --
// keeps the triangle.  The caller leaves out the lanes that START on the triangle (the walk ignores that primitive and no other).
// The cull is per lane and per triangle, for all frames: lt_entry_cut_kernel keeps a leaf that any casting lane may accept.
constexpr float kTriRel = 0x1p-18f;    // G

LT_EC_HD inline void cross_signed_abs(const float (&x)[3], const float (&y)[3], float (&c)[3], float (&p)[3]) {
  for (int a = 0; a < 3; a++) {
    const int b = (a + 1) % 3, d = (a + 2) % 3;
    c[a] = x[b] * y[d] - x[d] * y[b];
    p[a] = __builtin_fabsf(x[b]) * __builtin_fabsf(y[d]) + __builtin_fabsf(x[d]) * __builtin_fabsf(y[b]);
  }
}
// The range of w . c over the lane's direction box.
LT_EC_HD inline void range_over_box(const LaneSet& ls, const float (&c)[3], float& lo, float& hi) {
  lo = 0.0f; hi = 0.0f;
  for (int a = 0; a < 3; a++) {
    const float p = c[a] * ls.wl[a], q = c[a] * ls.wh[a];
    lo = lo + (p < q ? p : q);
    hi = hi + (p < q ? q : p);
  }
}

// The triangle test: false only if no line through the lane's origin along a direction of its ray set passes the float triangle
// test of the traversal triangle (A, e1, e2) -- in any math flavour, whatever t.
LT_EC_HD inline bool may_accept(const LaneSet& ls, float ax, float ay, float az, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
  const float A[3] = {ax, ay, az}, e1[3] = {e1x, e1y, e1z}, e2[3] = {e2x, e2y, e2z};
  float T[3], M[3];
  float norm1 = 1.0f, M1 = 0.0f;
  bool sane = true;
  for (int a = 0; a < 3; a++) {
    T[a] = ls.o[a] - A[a];
    const float wl = __builtin_fabsf(ls.wl[a]), wh = __builtin_fabsf(ls.wh[a]);
    M[a] = wl > wh ? wl : wh;
    M1 = M1 + M[a];
    sane = sane && __builtin_fabsf(T[a]) < kMaxMagnitude && __builtin_fabsf(e1[a]) < kMaxMagnitude && __builtin_fabsf(e2[a]) < kMaxMagnitude;
    norm1 = norm1 + ((__builtin_fabsf(T[a]) + __builtin_fabsf(e1[a])) + __builtin_fabsf(e2[a]));
  }
  if (!sane) return true;
  float cD[3], cU[3], cV[3], pD[3], pU[3], pV[3];
  cross_signed_abs(e2, e1, cD, pD);
  cross_signed_abs(e2, T, cU, pU);
  cross_signed_abs(T, e1, cV, pV);
  float SD = 0.0f, SU = 0.0f, SV = 0.0f, SN = 0.0f, N = 0.0f;
  for (int a = 0; a < 3; a++) {
    SD = SD + M[a] * pD[a];
    SU = SU + M[a] * pU[a];
    SV = SV + M[a] * pV[a];
    SN = SN + __builtin_fabsf(e2[a]) * pV[a];
    N = N + e2[a] * cV[a];
    norm1 = norm1 + pD[a];
  }
  const float Z = (M1 * norm1) * kAbs + kAbs;
  float lo, hi;
  range_over_box(ls, cD, lo, hi);
  const float mD = kTriRel * SD + Z;
  float s, minD, maxD;
  if (lo > mD) { s = 1.0f; minD = lo; maxD = hi; }
  else if (hi < -mD) { s = -1.0f; minD = -hi; maxD = -lo; }
  else return true;
  const float k = 0.0098f / M1;
  if ((s * N - maxD) + (k < 1.0f ? k : 1.0f) * minD > kTriRel * (SN + SD) + Z) return false;   // t >= tmax
  float cUD[3], cUVD[3];
  for (int a = 0; a < 3; a++) {   // (times s: exact)
    cD[a] = s * cD[a]; cU[a] = s * cU[a]; cV[a] = s * cV[a];
    cUD[a] = cU[a] - cD[a];
    cUVD[a] = (cU[a] + cV[a]) - cD[a];
  }
  range_over_box(ls, cU, lo, hi);
  if (hi < -(kTriRel * SU + Z)) return false;                    // u < 0
  range_over_box(ls, cV, lo, hi);
  if (hi < -(kTriRel * SV + Z)) return false;                    // v < 0
  range_over_box(ls, cUD, lo, hi);
  if (lo > kTriRel * (SU + SD) + Z) return false;                // u > 1
  range_over_box(ls, cUVD, lo, hi);
  if (lo > kTriRel * ((SU + SV) + SD) + Z) return false;         // u + v > 1
  return true;
}

// ---- The tree as the leaf pass saw it: record v (the v-th it visited, the root first) has the reference ref[v] (negative: a leaf),
// the record it was reached from, parent[v] (kNoRecord for the root), and the records its two children became, kid[2 v], kid[2 v + 1]
// (kNoRecord: not reached).  mark[v]: a surviving leaf, or a record above one.
constexpr int kPruneRecords = 512;
constexpr unsigned short kNoRecord = 0xffffu;

// Leaf record v survives: marks it and every record above it (stops at the first that is marked already).
LT_EC_HD inline void pruned_mark(const unsigned short* parent, unsigned char* mark, unsigned v) {
  while (v != (unsigned)kNoRecord && mark[v] == 0) {
    mark[v] = 1;
    v = parent[v];
  }
}

// The cut: starts as the root record, and the shallowest interior entry -- the first of several -- is replaced by its marked
// children, until a replacement would make it longer than cap or every entry is a leaf.  entry / depth: room for cap + 2 each.
// Writes the references of the cut to out (cap at least 2) and returns their number; 0 when the root is not marked.
LT_EC_HD inline unsigned pruned_cut_select(const unsigned* ref, const unsigned short* kid, const unsigned char* mark, unsigned cap,
                                           unsigned short* entry, unsigned char* depth, unsigned* out) {
  if (mark[0] == 0) return 0u;
  unsigned n = 1u;
  entry[0] = 0;
  depth[0] = 0;
  for (;;) {
    unsigned pick = n, best = 0xffffffffu;
    for (unsigned i = 0; i < n; i++)
      if ((int)ref[entry[i]] >= 0 && depth[i] < best) { best = depth[i]; pick = i; }
    if (pick == n) break;
    const unsigned v = entry[pick];
    unsigned short kids[2];
    unsigned k = 0u;
    for (unsigned s = 0; s < 2u; s++)
      if (kid[2u * v + s] != kNoRecord && mark[kid[2u * v + s]] != 0) kids[k++] = kid[2u * v + s];
    if (n - 1u + k > cap) break;
    const unsigned char d = (unsigned char)(depth[pick] + 1);
    entry[pick] = entry[n - 1u]; depth[pick] = depth[n - 1u];
    unsigned m = n - 1u;
    for (unsigned s = 0; s < k; s++) { entry[m] = kids[s]; depth[m] = d; m++; }
    n = m;
    if (n == 0u) break;   // (a marked interior record has a marked child: not reached)
  }
  for (unsigned i = 0; i < n; i++) out[i] = ref[entry[i]];
  return n;
}

// The item table of a kept set of cuts (lt_clear_items_kernel; render_kernel_body).  A launch of `groups` frame groups per stored
// square hands out, per XCD share and in the share's order, ONE entry for a square marked clear -- the wave that takes it runs the
// square's frame groups one after the other -- and `groups` entries for any other square, one per frame group.  An entry is the
// index the square-major hand-out without a table gives that item, local * groups + group (local: the square's place in its
// share), with kItemWhole set for a whole square; a share's entries lie from word kItemHeader + share start * groups of the table,
// and words 0 .. 7 hold the eight shares' entry counts.
constexpr unsigned kItemWhole = 0x80000000u;
constexpr unsigned kItemHeader = 16u;
LT_EC_HD inline bool item_whole(unsigned word0) { return word0 == kClearMark; }
LT_EC_HD inline unsigned item_entries(unsigned word0, unsigned groups) { return item_whole(word0) ? 1u : groups; }
// Writes a square's entries at dst (item_entries of them).
LT_EC_HD inline void item_write(unsigned* dst, unsigned word0, unsigned local, unsigned groups) {
  if (item_whole(word0)) {
    dst[0] = (local * groups) | kItemWhole;
    return;
  }
  for (unsigned g = 0; g < groups; g++) dst[g] = local * groups + g;
}

// The fold map that goes with a table: one byte per 8-pixel row segment of the tile-stacked output (tileW a multiple of 8, three
// floats per pixel: a segment is 24 floats, six whole quads of lt_running_mean4_kernel), 1 where the segment's square is handed
// out whole -- its samples are then folded into the running mean by the wave that renders it and never stored -- else 0.  Row ly of the
// stacked tile k, square column sbx; and the segment a float of the output lies in.
constexpr unsigned kFoldSegmentFloats = 24u;
LT_EC_HD inline unsigned long long fold_segment(unsigned k, unsigned tileH, unsigned tileW, unsigned ly, unsigned sbx) {
  return ((unsigned long long)k * tileH + ly) * (tileW / 8u) + sbx;
}
LT_EC_HD inline unsigned long long fold_segment_of_float(unsigned long long i) { return i / kFoldSegmentFloats; }
// Marks the (up to eight) segments of square b = (tile k, square sb of the tile) with `mark`.
LT_EC_HD inline void fold_mark_square(unsigned char* map, unsigned b, unsigned blocksPerTileX, unsigned blocksPerTile, unsigned tileW,
                                      unsigned tileH, unsigned char mark) {
  const unsigned k = b / blocksPerTile, sb = b % blocksPerTile, sbx = sb % blocksPerTileX, sby = sb / blocksPerTileX;
  for (unsigned r = 0; r < 8u && sby * 8u + r < tileH; r++) map[fold_segment(k, tileH, tileW, sby * 8u + r, sbx)] = mark;
}

}  // namespace lt_entry_cut
