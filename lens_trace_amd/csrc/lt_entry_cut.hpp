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

}  // namespace lt_entry_cut
