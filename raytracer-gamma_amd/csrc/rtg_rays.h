// rtg_rays.h — what the batch ray queries (rtg_rays.hip) and the batch ray
// tracer (rtg_raytrace.hip, the per-S raytrace kernels) share with each other
// and with the context (rtg_kernel.hip): the BVH's origin box as a kernel
// argument of the ray kernels alone (KernelArgs and the trace kernels do not
// know it), the two queries that are exact for any origin (the argument is
// at the head of rtg_rays.hip), and the one call that runs rayTrace over them
// for a caller's own ray (trace_ray, with its plain-loop twin).
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

// The device scene of the ray kernels (the queries', the batch ray tracer's,
// the posed camera's): one-wave workgroups over the context's tables.
template <bool kBvh>
using RayScene = DevScene<false, 64, kBvh, 0>;

// The extra half-width every BVH box gets for a ray from o (rtg_rays.hip's
// header); `odd`: the origin is outside the slab arithmetic's range.
RTG_HD float ray_delta(const RayBox& B, V3 o, bool& odd) {
  const float ax = fabsf(o.x), ay = fabsf(o.y), az = fabsf(o.z);
  odd = !(ax <= 0x1p56f && ay <= 0x1p56f && az <= 0x1p56f);  // NaN: odd
  const float M = fmaxf(ax, fmaxf(ay, az));
  const float ex = fmaxf(fmaxf(B.lo[0] - o.x, o.x - B.hi[0]), 0.f);
  const float ey = fmaxf(fmaxf(B.lo[1] - o.y, o.y - B.hi[1]), 0.f);
  const float ez = fmaxf(fmaxf(B.lo[2] - o.z, o.z - B.hi[2]), 0.f);
  const float D = sqrt_hw(ex * ex + ey * ey + ez * ez);
  const float Mo = M > B.omax ? M : 0.f;
  return (0x1p-8f * D + 0x1p-18f * Mo) * (1.0f + 0x1p-10f);
}

// calcIntersection for ray (o, d) of an `active` lane; the whole wave enters
// (kBvh: the walk is wave-uniform).  Inactive lanes get a miss.
template <bool kBvh, class Scene>
RTG_HD int ray_closest(const Scene& sc, const RayBox& box, V3 o, V3 d, bool active, float& t) {
  if constexpr (kBvh) {
    const RayQ q = make_query(o, d);
    bool odd;
    const float delta = ray_delta(box, o, odd);
    odd = active && (odd || !q.fast);
    int id = closest_bvh<true>(sc, q, t, delta, active && !odd);
    if (sc.any(odd)) {
      if (odd) id = closest_hit4(sc, o, d, t);
    }
    return id;
  } else {
    t = 1000.f;
    if (!active) return -1;
    if (sc.n4 <= 64) return closest_hit64(sc, o, d, t);
    return closest_hit4(sc, o, d, t);
  }
}

// A segment's shadow ray (raytracer.h:279-286): gap before normalising.
RTG_HD V3 segment_ray(V3 a, V3 b, float& gap) {
  const V3 dist = vsub(b, a);
  gap = vdot(dist, dist);
  return vnorm(dist);
}

// hasClearLineOfSight's blocker search for the ray (o, d) with gap |b - a|^2,
// for a caller that asks many rays from one origin (the K probes of an
// ambient-occlusion point, rtg_ao.hip): delta and oddOrigin are ray_delta(box,
// o, oddOrigin), taken once per origin (a scene without a BVH reads neither).
// Nothing else of a query depends on the origin alone: make_query's origin
// half is a copy of o.
template <bool kBvh, class Scene>
RTG_HD bool ray_blocked(const Scene& sc, V3 o, V3 d, float gap, bool active, float delta,
                        bool oddOrigin) {
  if constexpr (kBvh) {
    const RayQ q = make_query(o, d);
    const bool odd = active && (oddOrigin || !q.fast);
    bool blk = blocked_bvh<true>(sc, q, gap, delta, active && !odd);
    if (sc.any(odd)) {
      if (odd) blk = blocked(sc, o, d, gap);
    }
    return blk;
  } else {
    if (!active) return false;
    if (sc.n4 <= 64) return blocked64(sc, o, d, gap);
    return blocked(sc, o, d, gap);
  }
}

// The same for one ray: the delta of its own origin.
template <bool kBvh, class Scene>
RTG_HD bool ray_blocked(const Scene& sc, const RayBox& box, V3 o, V3 d, float gap, bool active) {
  if constexpr (kBvh) {
    const RayQ q = make_query(o, d);
    bool odd;
    const float delta = ray_delta(box, o, odd);
    odd = active && (odd || !q.fast);
    // (active lanes have 2 a in the Markstein range: the walk's reach in ray
    // units is sqrt(gap / a) rounded up)
    bool blk = blocked_bvh<true>(sc, q, gap, delta, active && !odd);
    if (sc.any(odd)) {
      if (odd) blk = blocked(sc, o, d, gap);
    }
    return blk;
  } else {
    if (!active) return false;
    if (sc.n4 <= 64) return blocked64(sc, o, d, gap);
    return blocked(sc, o, d, gap);
  }
}

// The query path of a caller's own ray tree (trace_sample's RP, rtg_trace.h):
// every node's closest hit and every shadow ray is one of the two queries
// above, with the delta of that query's own origin.  The lanes of a wave in
// trace_sample's loop are the ones still tracing, all of them querying.
template <bool kBvh>
struct RayPath {
  static constexpr bool kOn = true;
  RayBox box;
  template <class Scene>
  RTG_HD int closest(const Scene& sc, V3 o, V3 d, float& t) const {
    return ray_closest<kBvh>(sc, box, o, d, true, t);
  }
  template <class Scene>
  RTG_HD bool blocked(const Scene& sc, V3 o, V3 d, float gap) const {
    return ray_blocked<kBvh>(sc, box, o, d, gap, true);
  }
  RTG_HD void lit(unsigned) const {}  // matte_light's note of a lit light: not kept
};

// rayTrace of a caller's own ray (o, d): THE call of the batch ray tracer and
// the posed camera, kernels and walk-1 host forms alike.  Its constants are
// what makes such a ray exact, whatever its origin and direction:
//  * Q == 2 and RayPath: the shading path that asks no table keyed to the
//    renderer's own rays (guardOK stays false, so no cone, shadow or overlap
//    mask and no sphere list is read), every query ray_closest / ray_blocked
//    with the delta of its own origin (rtg_raytrace.hip's header has the table
//    of shortcuts this leaves out);
//  * usePrim false, primSel ~0: no primary-ray mask, which holds only for a
//    camera at 0 inside the wave's direction bundle.
// Forced inline, so each caller keeps the code it had with the call written out.
template <int S, bool kCL, bool kBvh, class Scene>
RTG_HD V3 trace_ray(const Scene& sc, const RayBox& box, V3 o, V3 d) {
  return trace_sample<S, 2, kCL, RayPath<kBvh>>(sc, d, sc.frames(), false, ~0ull, o,
                                                RayPath<kBvh>{box});
}

// Its plain-loop twin, the yardstick of the host forms' walk 0: Q == 0, every
// query a loop over every sphere (closest_hit, blocked, the flat
// primary_container), no table, no BVH.
template <int S, bool kCL, class Scene>
RTG_HD V3 trace_ray_plain(const Scene& sc, V3 o, V3 d) {
  return trace_sample<S, 0, kCL>(sc, d, sc.frames(), false, ~0ull, o);
}

}  // namespace rtg
