// A user program used as a probe: do lt::random_ / lt::randoms_ / lt::random_x_ (lt_device.hpp: the short sine, the library's only
// where the float is not proved) return lt::random_library_'s bits?  Every pixel checks, in the kernel's math flavour,
//   * the 96 seeds from frameCount * 96 on, and the negated argument of each (-uv, -seed: the dot and the product are odd), one
//     random at a time, and the same seeds four at a time through randoms_<M, 4>;
//   * arguments built to sit on a tie: r = asin(m / 43758.5453) for a float midpoint m that depends on the pixel, its +-3
//     neighbouring doubles, and their negatives;
//   * edge values of the fmod's argument.
// The colour is (mismatches, values checked, fallbacks), fallbacks = those among the seeds' 192 + 1024 * those among the rest.
namespace lt {
__device__ inline bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
template <class CFG>
__device__ V3 user_shade(const SceneDev& sc, const Ray& cameraRay, float filmX, float filmY, uint32_t frameCount,
                         Stack<CFG::kDeep>& st, Counters& c) {
  constexpr int M = CFG::kDevLibm;
  uint32_t bad = 0, n = 0, fellSeeds = 0, fellRest = 0;
  for (uint32_t k = 0; k < 96; k++) {
    const float seed = (float)(frameCount * 96u + k);
    bad += same_bits(random_<M>(filmX, filmY, seed, &fellSeeds), random_library_<M>(filmX, filmY, seed)) ? 0u : 1u;
    bad += same_bits(random_<M>(-filmX, -filmY, -seed, &fellSeeds), random_library_<M>(-filmX, -filmY, -seed)) ? 0u : 1u;
    n += 2;
  }
  for (uint32_t k = 0; k < 96; k += 4) {
    const uint32_t s = frameCount * 96u + k;
    const float seed[4] = {(float)s, (float)(s + 1u), (float)(s + 2u), (float)(s + 3u)};
    float rnd[4];
    uint32_t fell = 0;   // (the same seeds as above: not counted twice)
    randoms_<M, 4>(filmX, filmY, seed, rnd, &fell);
#pragma unroll
    for (int i = 0; i < 4; i++) bad += same_bits(rnd[i], random_library_<M>(filmX, filmY, seed[i])) ? 0u : 1u;
    n += 4;
  }
  auto check = [&](double x) {
    const float lib = random_library_a(x);
    bad += same_bits(random_x_(x, &fellRest), lib - __builtin_floorf(lib)) ? 0u : 1u;
    n++;
  };
  {
    const uint32_t h = (__float_as_uint(filmX) * 2654435761u) ^ (__float_as_uint(filmY) * 40503u) ^ (frameCount * 97u);
    const float f = 1.0f + (float)(h >> 8) * (43000.0f / 16777216.0f);
    const double mid = 0.5 * ((double)f + (double)__uint_as_float(__float_as_uint(f) + 1u));
    const double r = asin(mid / 43758.5453);
    for (int d = -3; d <= 3; d++) {
      const double rd = __longlong_as_double(__double_as_longlong(r) + (long long)d);
      check(rd);
      check(-rd);
    }
  }
  const double edge[] = {0.0, -0.0, M_PI, -M_PI, 3.1415926535897927, 3.1415926535897936, -3.1415926535897927, 1.5707963267948966, 1.5707963267948963,
                         1.5707963267948968, -1.5707963267948966, 2.0 * M_PI, 1e-310, -1e-310, 5e-324, 0x1p+39, 0x1p+40, -0x1p+40, 0x1.fffffffffffffp+39,
                         1e300, __builtin_inf(), -__builtin_inf(), __builtin_nan(""), 355.0, 103993.0};
  for (double e : edge) check(e);
  return V3{(float)bad, (float)n, (float)(fellSeeds + 1024u * fellRest)};
}
}  // namespace lt
