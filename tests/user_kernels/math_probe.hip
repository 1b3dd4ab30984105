// A user program used as a probe of lt_device.hpp's leaf layer: Math<>::{mad, rcp, fdiv, div25, sqrt_user, rsqrt, sin, cos, clamp01} (and,
// through distance4, sqrt_in_distance), normalize4, distance4, dot4, dot2, cross4 and bary3's contraction
// shape, each in the flavour its kernel was compiled for (CFG::kDevLibm).  tests/math_edges.py packs one record per pixel into the
// primitives' normals (nine words per primitive that nothing else reads): the word stream starts with a header primitive
// (width, height, records), then 18 words per record: the operation's id, up to 8 input words, up to 4 expected result words.
// The pixel evaluates the lt:: function on its record's inputs and compares bit patterns -- two NaNs are equal whatever their
// payload.  The colour is (mismatching values, values checked, id of the mismatching operation); with frameCount = 1 + k it is
// the raw result words k .. k + 2 instead, which the test prints when a comparison fails.
namespace lt {
__device__ inline uint32_t probe_word(const SceneDev& sc, uint32_t j) { return __float_as_uint(sc.prims[19u * (size_t)(j / 9u) + 9u + j % 9u]); }
__device__ inline bool probe_nan(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
template <class CFG>
__device__ V3 user_shade(const SceneDev& sc, const Ray& cameraRay, float filmX, float filmY, uint32_t frameCount,
                         Stack<CFG::kDeep>& st, Counters& c) {
  constexpr int M = CFG::kDevLibm;
  const uint32_t W = probe_word(sc, 0), H = probe_word(sc, 1), records = probe_word(sc, 2);
  // the pixel from its film position x / W - 0.5 (any flavour's division is within ulps: rounding recovers x)
  const uint32_t x = (uint32_t)__builtin_rintf((filmX + 0.5f) * (float)W), y = (uint32_t)__builtin_rintf((filmY + 0.5f) * (float)H);
  const uint32_t idx = y * W + x;
  if (idx >= records || (size_t)(2u * idx + 3u) > sc.n_prims) return V3{0.0f, 0.0f, 0.0f};
  uint32_t w[18];
  for (uint32_t j = 0; j < 18u; j++) w[j] = probe_word(sc, 9u + 18u * idx + j);
  const uint32_t op = w[0];
  float f[8];
  for (int j = 0; j < 8; j++) f[j] = __uint_as_float(w[1 + j]);
  const V4 a = mk4(f[0], f[1], f[2], f[3]), b = mk4(f[4], f[5], f[6], f[7]);
  uint32_t got[4] = {0u, 0u, 0u, 0u}, words = 1u;
  auto put4 = [&](V4 v) { got[0] = __float_as_uint(v.x); got[1] = __float_as_uint(v.y); got[2] = __float_as_uint(v.z); got[3] = __float_as_uint(v.w); words = 4u; };
  switch (op) {
    case 1: put4(normalize4<M>(a)); break;
    case 2: got[0] = __float_as_uint(distance4<M>(a, b)); break;
    case 3: got[0] = __float_as_uint(dot4(a, b)); break;
    case 4: got[0] = __float_as_uint(dot2(f[0], f[1], f[2], f[3])); break;
    case 5: put4(cross4(a, b)); break;
    case 6: got[0] = __float_as_uint(Math<M>::clamp01(f[0])); break;
    case 7: got[0] = __float_as_uint(Math<M>::sin(f[0])); break;
    case 8: got[0] = __float_as_uint(Math<M>::cos(f[0])); break;
    case 9: got[0] = __float_as_uint(Math<M>::fdiv(f[0], f[1])); break;
    case 10: got[0] = __float_as_uint(Math<M>::rcp(f[0])); break;
    case 11: got[0] = __float_as_uint(Math<M>::div25(f[0])); break;
    case 12: got[0] = __float_as_uint(Math<M>::sqrt_user(f[0])); break;
    case 13: got[0] = __float_as_uint(Math<M>::mad(f[0], f[1], f[2])); break;                    // a*b + c
    case 14: got[0] = __float_as_uint(Math<M>::mad(f[0], f[1], f[2] * f[3])); break;             // a*b + c*d: the left product fuses
    case 15: {                                                                                  // a*b + c*d + e*f: bary3's shape
      const float A[3] = {f[0], 0.0f, 0.0f}, B[3] = {f[2], 0.0f, 0.0f}, C[3] = {f[4], 0.0f, 0.0f};
      got[0] = __float_as_uint(bary3<M>(A, B, C, V3{f[1], f[3], f[5]}).x);
      break;
    }
    case 16: {                                                                                  // a*b + c in double (random()'s shape)
      double d[3];
      for (int j = 0; j < 3; j++) d[j] = __longlong_as_double((long long)(((unsigned long long)w[2 + 2 * j] << 32) | w[1 + 2 * j]));
      const unsigned long long v = (unsigned long long)__double_as_longlong(Math<M>::mad(d[0], d[1], d[2]));
      got[0] = (uint32_t)v; got[1] = (uint32_t)(v >> 32); words = 2u;
      break;
    }
    case 17: got[0] = __float_as_uint(Math<M>::rsqrt(f[0])); break;   // (normalize4 never hands rsqrt an argument below FLT_MIN)
    default: return V3{1.0f, 0.0f, (float)op};   // an unknown operation is a mismatch, not a pass
  }
  if (frameCount) {
    const uint32_t k = frameCount - 1u;
    return V3{__uint_as_float(k < 4u ? got[k] : 0u), __uint_as_float(k + 1u < 4u ? got[k + 1u] : 0u), __uint_as_float(k + 2u < 4u ? got[k + 2u] : 0u)};
  }
  uint32_t bad = 0u, values = words;
  if (op == 16u) {   // one double in two words
    const bool nanGot = (got[1] & 0x7ff00000u) == 0x7ff00000u && ((got[1] & 0xfffffu) | got[0]) != 0u;
    const bool nanWant = (w[10] & 0x7ff00000u) == 0x7ff00000u && ((w[10] & 0xfffffu) | w[9]) != 0u;
    bad = ((got[0] == w[9] && got[1] == w[10]) || (nanGot && nanWant)) ? 0u : 1u;
    values = 1u;
  } else {
    for (uint32_t j = 0; j < words; j++) bad += (got[j] == w[9 + j] || (probe_nan(got[j]) && probe_nan(w[9 + j]))) ? 0u : 1u;
  }
  return V3{(float)bad, (float)values, bad ? (float)op : 0.0f};
}
}  // namespace lt
