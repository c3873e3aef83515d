// rtg_trace_s.hip — instantiates the trace kernels for ONE stack capacity,
// RTG_S (set by the Makefile: one object per S = 1..16, built in parallel),
// and exports them as one record, stack_kernels_s<S> (StackKernels,
// rtg_trace_kernels.h): the render kernels (trace_fn), the batch ray tracer's
// (raytrace_fn) and the posed camera's fused render kernels (camera_fn,
// views_fn, views_fold_fn) and the gather's (gather_fn).
#include "rtg_camera_kernels.h"
#include "rtg_gather_kernels.h"
#include "rtg_raytrace_kernels.h"
#include "rtg_trace_kernels.h"

#ifndef RTG_S
#error "RTG_S (stack capacity) must be defined"
#endif
#define RTG_CAT2(a, b) a##b
#define RTG_CAT(a, b) RTG_CAT2(a, b)

namespace rtg {
// (a function, not a constant: a constant at namespace scope would be emitted
// for the device too, where the host pickers it names do not exist)
const StackKernels* RTG_CAT(stack_kernels_s, RTG_S)() {
  static const StackKernels k = {trace_fn<RTG_S>, raytrace_fn<RTG_S>, camera_fn<RTG_S>,
                                 views_fn<RTG_S>, views_fold_fn<RTG_S>,
                                 gather_fn<RTG_S>};
  return &k;
}
}  // namespace rtg
