// rtg_trace_s.hip — instantiates the trace kernels for ONE stack capacity,
// RTG_S (set by the Makefile: one object per S = 1..16, built in parallel):
// the render kernels (trace_fn), the batch ray tracer's (raytrace_fn) and the
// posed camera's fused render kernel (camera_fn).
#include "rtg_camera_kernels.h"
#include "rtg_raytrace_kernels.h"
#include "rtg_trace_kernels.h"

#ifndef RTG_S
#error "RTG_S (stack capacity) must be defined"
#endif
#define RTG_CAT2(a, b) a##b
#define RTG_CAT(a, b) RTG_CAT2(a, b)

namespace rtg {
TraceFn RTG_CAT(trace_fn_s, RTG_S)(int variant, bool bvh, int list) {
  return trace_fn<RTG_S>(variant, bvh, list);
}
RayTraceFn RTG_CAT(raytrace_fn_s, RTG_S)(bool bvh, bool cl) {
  return raytrace_fn<RTG_S>(bvh, cl);
}
CameraFn RTG_CAT(camera_fn_s, RTG_S)(bool bvh, bool cl) {
  return camera_fn<RTG_S>(bvh, cl);
}
}  // namespace rtg
