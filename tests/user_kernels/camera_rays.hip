// A user program that renders the kernel's own camera rays: the colour is the ray's origin (frameCount % 3 == 0), its direction
// (1) or its film position and origin.w + direction.w (2).  Nothing is walked.
namespace lt {
template <class CFG>
__device__ V3 user_shade(const SceneDev& sc, const Ray& cameraRay, float filmX, float filmY, uint32_t frameCount,
                         Stack<CFG::kDeep>& st, Counters& c) {
  const uint32_t what = frameCount % 3u;
  if (what == 0u) return V3{cameraRay.o.x, cameraRay.o.y, cameraRay.o.z};
  if (what == 1u) return V3{cameraRay.d.x, cameraRay.d.y, cameraRay.d.z};
  return V3{filmX, filmY, cameraRay.o.w + cameraRay.d.w};
}
}  // namespace lt
