// rtg_raytrace.hip — the batch ray tracer of librtg.so (rtg_raytrace*, rtg.h):
// rayTrace (raytracer.h:410-636) for a caller's own rays against the resident
// scene, bit for bit: dst[k] = rayTrace(spheres, n, lights, m, {origin_k,
// dir_k, (1,1,1)}, bgMaterial, 0) for stack capacity S.  The third member of
// the query family after rtg_intersect / rtg_visible (rtg_rays.hip).  This
// file holds the launcher, the argument checks and the host forms; the kernel
// (raytrace_kernel, rtg_raytrace_kernels.h: one lane per ray, one-wave
// workgroups, 24 bytes in, 12 bytes out) is instantiated per stack size next
// to the render kernels (rtg_trace_s.hip), for BVH or not and CPU or OpenCL
// semantics.  The stack machine is the renders' trace_sample (rtg_trace.h)
// with a start origin and the query path RayPath switched on: trace_ray
// (rtg_rays.h).
//
// WHICH RAYS TAKE WHICH PATH.  The render kernels shorten their queries with
// tables that were proved for the renderer's own rays: a camera at 0, hit
// points and their 0.01 offsets inside the origin box B* (origin_box,
// rtg_scene_pack.h), directions of about unit length.  A caller's ray promises
// none of that, and not only at level 0: the reference's accepted root of a
// ray from a distant origin lies up to mu = 2^-8 (|o - c| + r) off its sphere,
// so the hit point P, the shadow rays from P and both children's origins can
// leave B* too, and a refraction child keeps the caller's |d|.  Each shortcut
// of the shading path, what it assumes, and where that comes from:
//
//   shortcut (rtg_trace.h)            assumes                     checked on the values?
//   --------------------------------  --------------------------  ----------------------
//   BVH boxes, closest_bvh<false> /   every query origin in B*:   no: taken from "the
//     blocked_bvh<false>                |p_i| <= P_i, |o| <= omax    origin is in B*"
//   primary masks (usePrim, group_    a ray from 0 inside the     no: the camera's
//     sel, closest_hit_sel)             wave's direction bundle      geometry
//   shadow / overlap masks (shadow_   P in the hit sphere's guard  guardOK is, on P; but
//     union, contain_union)             ball g = r + 2^-8 (diam      g's mu bound is the
//                                       B* + r) and |D| <= 3         B* one (|p| bounded)
//   cone masks (cone_union)           origin in a guard ball       guardOK of the parent
//                                       + 0.0101, |rd| ~ 1           hit, same g
//   capsule and overlap lists         as the masks, per cell       guardOK, same g
//     (blocked_cap_lanes, container_
//     lanes, closest_enter[_list])
//   no_root skip of the origin sphere b, cc of the ray itself      yes (the ray's own
//                                                                   values), but only
//                                                                   reached through a
//                                                                   cone mask
//   facing-away light skip            relative rounding of N.dist  m >= 2^-100 is; that
//     (matte_light, masked scenes)      with no underflow            |dist| is moderate
//                                                                   is not
//   container_bvh (refraction target) the point alone: a sphere's  needs none (below)
//                                       containment ball lies in
//                                       its grown box
//
// guardOK is a run-time test on the computed P, and a P that passes it is in
// the ball the masks and lists were built for.  But the tables say more than
// "P is in the ball": the cone masks and the entering-ray lists also bound the
// child's direction (|rd| ~ 1, |D| <= 3 for the 0.01 D test point), which a
// refraction child of a caller's ray (it keeps the caller's |d|) does not
// meet, and every table path falls back to the unwidened BVH walk, which
// needs the origin in B*.  A per-lane `trusted` flag (origin in B*: ray_delta
// gives delta == 0, not odd; |d| bounded) with a wave-uniform gate would let
// such rays take the tables; it needs each row above re-proved for "origin in
// B*, any direction" and is left as follow-up.  This version takes NONE of
// the table paths for ANY ray of the batch (RayPath::kOn, a compile-time
// switch: the render kernels compile none of this and are the code they
// were):
//
//   * every node's closest hit is ray_closest (rtg_rays.h): the widened BVH
//     walk with the delta of THAT query's own origin (0 inside B*, so a tree
//     that stays in B* walks the boxes the renders walk), the flat pass for
//     its `odd` lanes, closest_hit64 / closest_hit4 without a BVH;
//   * every shadow ray is ray_blocked, the same way (the origin is P);
//   * the refraction target is primary_container: flat over every sphere
//     without a BVH; container_bvh with one.  container_bvh needs no origin
//     precondition: it descends into a child when the POINT is inside the
//     child's stored box (exact comparisons, no slab arithmetic, NaN and
//     infinity fail them as they fail the reference's <=), and a sphere's
//     containment ball (r + 1e-6, accepted at most a few ulps of |pt - c|^2
//     outside, a bound in r alone) lies inside its grown box of half-width
//     >= r + 2^-8 r + 2^-20;
//   * guardOK stays false, so no frame records an origin or entered sphere,
//     has_cone / has_smask / has_lists are never asked, and the facing-away
//     light skip is compiled out.
// ray_closest and ray_blocked are exact for any origin and any direction:
// the argument is at the head of rtg_rays.hip, and it is per query, so it
// holds at every level of the tree whatever the levels above did.  What is
// left of trace_sample is the reference's own arithmetic on the hit
// (raytracer.h:454-636 in the same float operations), shared with the renders.
// The price is measured, not guessed: tools/bench_rays.py puts the batch call
// next to rtg_render_device of the same rays (README).
//
// In a wave, the lanes in trace_sample's loop are those still tracing; a lane
// whose tree is done has left, and the wave-level tests of the queries
// (all / any, the wave-uniform BVH walk and its LDS stack) are over the lanes
// present, as in the render kernels.  Lanes past the end of the batch leave
// before the trace.  rtg_raytrace_indexed_device (the ray order, rtg.h) is the
// same kernel with an index list: lane k traces ray order[k] and writes
// dst[order[k]]; a lane whose entry is not an index of the batch leaves too.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
//
// The one call that takes this path is trace_ray (rtg_rays.h, where its
// constants are explained); the kernel and walk 1 of the host form make it.
//
// rtg_raytrace_host: walk 0 = trace_ray_plain, plain loops over every sphere
// for every query, the yardstick; walk 1 = the kernel's own path (trace_ray)
// over the packed tables (HostScene), one ray per "wave".  Its instantiation
// per stack size comes from host_trace_fn (rtg_host_scene.h), the kernel's
// from stack_kernels (rtg_trace_kernels.h); the argument checks shared with
// the other entry points are rtg_entry.h's.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_entry.h"
#include "rtg_host_scene.h"
#include "rtg_raytrace_kernels.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"

static_assert(sizeof(rtg_ray) == 24 && sizeof(rtg_vec) == 12, "24 B in, 12 B out");

namespace rtg {

// ---- host forms ----

// Rays [k0, k1) of the batch; kWalk 1: the kernel's path, else plain loops.
template <int S, bool kCL, bool kWalk, bool kBvh>
static void raytrace_host_range(const PackedScene& ps, const RayBox& box, const rtg_ray* rays,
                                size_t k0, size_t k1, rtg_vec* dst) {
  const HostScene<kBvh> sc(ps, kWalk);  // walk 0: no masks, no BVH, no lists
  for (size_t k = k0; k < k1; ++k) {
    const V3 o = v3(rays[k].origin.x, rays[k].origin.y, rays[k].origin.z);
    const V3 d = v3(rays[k].dir.x, rays[k].dir.y, rays[k].dir.z);
    if constexpr (kWalk) store_colour(dst + k, trace_ray<S, kCL, kBvh>(sc, box, o, d));
    else store_colour(dst + k, trace_ray_plain<S, kCL>(sc, o, d));
  }
}

typedef void (*HostRangeFn)(const PackedScene&, const RayBox&, const rtg_ray*, size_t, size_t,
                            rtg_vec*);

}  // namespace rtg

using namespace rtg;

// Argument checks of the host and one-shot forms (no HIP call).
static int check_raytrace_args(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                               unsigned lgtNum, const void* rays, const void* dst, int stackSize) {
  if (!rays || !dst) {
    rtg_set_error("raytrace: null %s buffer", rays ? "colour" : "ray");
    return RTG_ERR_INVALID;
  }
  const int rc = check_scene_arrays("raytrace", spheres, sphNum, lights, lgtNum);
  return rc ? rc : check_stack("raytrace", stackSize);
}

extern "C" {

int rtg_raytrace_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                      unsigned lgtNum, const rtg_ray* rays, size_t n, int stackSize, int semantics,
                      rtg_vec* dstHost, int walk, int nthreads) {
  rtg_clear_error();
  int rc = check_raytrace_args(spheres, sphNum, lights, lgtNum, rays, dstHost, stackSize);
  if (!rc) rc = check_semantics("raytrace", semantics);
  if (!rc) rc = check_walk("raytrace", walk);
  if (!rc) rc = check_sphere_count("raytrace", sphNum);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  PackedScene ps;
  pack_scene(spheres, sphNum, lights, lgtNum, &ps);  // as rtg_context_set_scene
  const bool bvh = walk == 1 && !ps.bvhNodes.empty();
  const RayBox box = bvh ? ray_box(ps.originBox) : RayBox{};
  const HostRangeFn fn = host_trace_fn(
      stackSize, semantics == RTG_SEMANTICS_OPENCL, walk == 1, bvh,
      [](auto s, auto cl, auto wk, auto bv) -> HostRangeFn {
        return raytrace_host_range<s.value, cl.value, wk.value, bv.value>;
      });
  host_bands(n, nthreads, [&](size_t k0, size_t k1) { fn(ps, box, rays, k0, k1, dstHost); });
  return RTG_OK;
}

// The device launch of rtg_raytrace_device (order null) and of its _indexed form.
static int raytrace_launch(rtg_context* ctx, const rtg_ray* raysDevice, const unsigned* order,
                           bool indexed, size_t n, int stackSize, rtg_vec* dstDevice,
                           void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0, semantics = RTG_SEMANTICS_CPU;
  if (!rtg_context_scene(ctx, &a, &device, &box, &semantics)) {
    rtg_set_error("raytrace: no context/scene");
    return RTG_ERR_INVALID;
  }
  if (!raysDevice || !dstDevice) {
    rtg_set_error("raytrace: null %s buffer", raysDevice ? "colour" : "ray");
    return RTG_ERR_INVALID;
  }
  int rc = check_stack("raytrace", stackSize);
  if (rc) return rc;
  if (indexed && !order) {
    rtg_set_error("raytrace: null order buffer");
    return RTG_ERR_INVALID;
  }
  if (n == 0) return RTG_OK;
  unsigned blocks;
  rc = ray_blocks("raytrace", "batch", n, &blocks);
  if (rc) return rc;
  const bool bvh = a.bvhNodes != nullptr;
  const StackKernels* sk = stack_kernels(stackSize);
  const RayTraceFn fn = sk ? sk->raytrace(bvh, semantics == RTG_SEMANTICS_OPENCL) : nullptr;
  if (!fn) {  // a missing kernel is an error, never another path
    rtg_set_error("raytrace: no kernel for stackSize %d", stackSize);
    return RTG_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), raytrace_lds_bytes(stackSize, bvh),
                     (hipStream_t)stream, a, box, raysDevice, order, n, dstDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_raytrace_device(rtg_context* ctx, const rtg_ray* raysDevice, size_t n, int stackSize,
                        rtg_vec* dstDevice, void* stream) {
  return raytrace_launch(ctx, raysDevice, nullptr, false, n, stackSize, dstDevice, stream);
}

int rtg_raytrace_indexed_device(rtg_context* ctx, const rtg_ray* raysDevice,
                                const unsigned* orderDevice, size_t n, int stackSize,
                                rtg_vec* dstDevice, void* stream) {
  return raytrace_launch(ctx, raysDevice, orderDevice, true, n, stackSize, dstDevice, stream);
}

int rtg_raytrace(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                 unsigned lgtNum, const rtg_ray* rays, size_t n, int stackSize,
                 rtg_vec* dstHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  const int rc = check_raytrace_args(spheres, sphNum, lights, lgtNum, rays, dstHost, stackSize);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  return one_shot("raytrace", device, {spheres, sphNum, lights, lgtNum}, rays,
                  n * sizeof(rtg_ray), dstHost, n * sizeof(rtg_vec),
                  [&](rtg_context* ctx, const void* in, void* out) {
                    return rtg_raytrace_device(ctx, (const rtg_ray*)in, n, stackSize,
                                               (rtg_vec*)out, nullptr);
                  });
}

}  // extern "C"
