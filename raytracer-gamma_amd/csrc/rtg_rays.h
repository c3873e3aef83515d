// rtg_rays.h — what the batch ray queries (rtg_rays.hip) share with the
// context (rtg_kernel.hip): the BVH's origin box as a kernel argument of the
// ray kernels alone (KernelArgs and the trace kernels do not know it).
#pragma once

#include <math.h>

#include "rtg_trace_kernels.h"

namespace rtg {

// The origin box B* of a BVH scene (origin_box, rtg_scene_pack.h) in floats,
// rounded INWARD (lo up, hi down, omax down): the distance from a point to
// this box is then an upper bound of its distance to B*, and a coordinate
// magnitude within `omax` is within B*'s.  All zero without a BVH (unused).
struct RayBox {
  float lo[3], hi[3], omax;
};

inline RayBox ray_box(const double ob[7]) {
  RayBox b;
  auto up = [](double v) {
    float f = (float)v;
    return (double)f < v ? nextafterf(f, __builtin_inff()) : f;
  };
  auto down = [](double v) {
    float f = (float)v;
    return (double)f > v ? nextafterf(f, -__builtin_inff()) : f;
  };
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = up(ob[a]);
    b.hi[a] = down(ob[3 + a]);
  }
  b.omax = down(ob[6]);
  return b;
}

}  // namespace rtg
