// A user program that exposes the render path's own hit position: colour = A*b.x + B*b.y + C*b.z of the camera ray's hit, in the
// render's math flavour (bary3<CFG::kDevLibm>, what every built-in shade starts its next ray from); 0 on a miss.
namespace lt {
template <class CFG>
__device__ V3 user_shade(const SceneDev& sc, const Ray& cameraRay, float filmX, float filmY, uint32_t frameCount,
                         Stack<CFG::kDeep>& st, Counters& c) {
  Hit pl{0, 0, kFltMax, 0.0f, 0.0f};
  traverse_camera<kAccumulator, CFG::kDeep, CFG::kStats>(sc, cameraRay, pl, st, c);
  if (pl.hitType != 1) return V3{0.0f, 0.0f, 0.0f};
  const float* pr = prim_ptr(sc, pl.prim);
  return bary3<CFG::kDevLibm>(pr + 0, pr + 3, pr + 6, barycentrics(pl.u, pl.v));
}
}  // namespace lt
