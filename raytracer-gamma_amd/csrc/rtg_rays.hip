// rtg_rays.hip — batch ray queries of librtg.so (rtg_intersect*, rtg_visible*,
// rtg.h): calcIntersection (raytracer.h:145-194) and hasClearLineOfSight
// (raytracer.h:272-309) for a caller's own rays against the resident scene,
// bit for bit.  One lane per ray, one-wave workgroups, the wave's 64-entry BVH
// stack in LDS (the G-buffer kernel's mapping, rtg_gbuffer.hip); a ray is 24
// bytes in, a hit two 16-byte stores out, a visibility one byte.  Lanes past
// the end of the batch stay in the wave as inactive queries (they load the
// batch's last ray, store nothing): the BVH walk is wave-uniform, no lane
// returns early from it.  One translation unit, no instantiation per stack
// size; the launches take none of rtg_context's render scratch.  The _indexed
// forms (rtg.h, the ray order) are the same kernel bodies with an index list:
// lane k works on record order[k] (ray_slot).  They are kernels of their own
// (two more instantiations each, in this one translation unit), so that the
// un-indexed kernels keep the code they had (DESIGN).
//
// The two queries themselves (ray_delta, ray_closest, ray_blocked) and a
// segment's shadow ray (segment_ray) are in rtg_rays.h, shared with the batch
// ray tracer (rtg_raytrace.hip), which asks them at every level of a ray's
// tree, and with the ambient occlusion (rtg_ao.hip); the argument below is
// theirs.
//
// Query per scene kind, all with the device functions of rtg_trace.h:
//   BVH scene (SceneTables::bvhNodes)  the render kernels' walk, widened
//                                      (closest_bvh<true> / blocked_bvh<true>)
//   n4 <= 64                           closest_hit64 / blocked64
//   anything else                      closest_hit4 / blocked (every sphere)
// The primary-ray masks (group_sel), the shadow, overlap and cone masks and
// the capsule lists are keyed to the renderer's own rays and are not used:
// bind_scene binds them like every table, and none of these queries reads
// them (has_smask / has_cone / has_lists are asked by the shading code only).
//
// ORIGINS OUTSIDE B*: the path taken is INFLATION (no flat fallback for finite
// origins).  The BVH's boxes (build_bvh, bvh_grow, rtg_scene_pack.h) keep every
// sphere the reference accepts only for ray origins inside the scene's origin
// box B* (rtg_trace.h, "Why a box keeps every sphere"): sphere i's box has the
// half-width
//   w_i = r_i + 2^-8 (P_i + r_i) + 2^-18 (|c_i|_inf + r_i + omax) + 2^-20,
// P_i = the distance from c_i to B*'s farthest corner >= |p_i| = |o - c_i|.
// The first margin is mu_i = 2^-8 (|p_i| + r_i), the bound of an accepted
// root's exact point X = o + t* d around the sphere, a statement about the
// ray's own p_i and d whatever they are (it comes from the radicand's
// relative rounding error, <= ~60 eps a (|p_i|^2 + r_i^2)); the second is the
// slab test's rounding, 3 eps (|plane| + |o|) per axis.  For an origin o
// anywhere, with
//   D >= dist(o, B*)  (0 inside),   M = |o|_inf,
// the nearest point q of B* to o has |q - c_i| <= P_i (q in B*, a box is
// convex and the farthest corner maximises the distance), so
//   |p_i| <= P_i + D,   mu_i <= 2^-8 (P_i + r_i) + 2^-8 D,
// and the slab rounding is at most 3 eps (|plane| + M), of which the builder's
// term covers 3 eps (|plane| + omax).  Every sphere box therefore needs at
// most
//   delta = 2^-8 D + 2^-18 [M > omax] M
// more half-width (ray_delta rounds it up by 1 + 2^-10), and the walk (kWide,
// bvh_ray_node in rtg_trace.h: the one walk there is, with the render kernels'
// prune order, slot passes and push order) tests every child box as [lo -
// delta, hi + delta].  A child box is the union of its spheres' grown boxes;
// the union inflated by delta contains each member inflated by delta, so
// inner nodes need nothing else.  Roundings on the way:
//  * D is taken to RayBox, B* rounded inward, so it can only grow; its
//    subtractions, squares, sum and v_sqrt_f32 are each within 2^-23
//    relative, and the factor 1 + 2^-10 on delta covers them;
//  * lo - delta and hi + delta round by 2^-24 (|plane| + delta): the plane
//    part is a third of the slab's own 3 eps |plane| allowance, for which the
//    builder's 2^-18 = 64 eps term leaves a factor 20; the delta part (and
//    the slab rounding 3 eps delta of the moved plane) is inside 2^-10 delta;
//  * for M > omax the whole 2^-18 M is added, 64 eps M against the 3 eps M
//    needed.
// delta is exactly 0 for an origin inside B* (the renderer's own kind: D = 0,
// M <= omax), so such rays walk the tree the render kernels walk.
// tests/test_rays_host.py (walk 1 against walk 0) checks it on near-tangent
// rays from 1e2 .. 1e5 scene units away.
//
// Lanes outside the range arguments take the flat loop (closest_hit4 /
// blocked) in a second pass that the wave skips when it has none (`odd`):
//  * an origin with a non-finite component or M > 2^56: the slab products
//    o / d stay finite only below 2^57 (build_bvh);
//  * a direction with 2 a = 2 d.d outside [2^-60, 2^60] (RayQ::fast false;
//    NaN, infinite, zero and a == b segments are among them): every
//    threshold below that multiplies a (75 a, 2^20 a, a (1 - K), sqrt(gap /
//    a)) is then free of overflow and underflow, and 1 / d_k is normal.
//
// The sphere-slot prunes are stated for the ray's own p = o - c (the
// reference's float subtraction) and d, and need nothing of where o is:
//  * pass-1 screen (pass1_rad): a slack of K = 2^-16 relative to a (|p|^2 +
//    r^2) against ~40 ulps of rounding of both evaluations: relative in p and
//    d, any origin, any |d| in the range above.  Where x^2 or a cs overflow
//    (|p| up to 2^58): x^2 = inf gives +inf or NaN, kept; a cs = +inf with
//    x^2 finite gives -inf, and the reference's a4 cc >= a (1 - K) cs is +inf
//    too, its radicand -inf or NaN, rejected as well;
//  * behind: proves b > 0, cc >= 0 and b < 150 a in the reference's own
//    values from the fused x and cs; the dot products' error bounds are
//    AM-GM bounds in a + |p|^2, any p and d;
//  * beyond: an accepted root has t |d| = |X - o| >= |p| - |X - c| >= |p| (1 -
//    2^-8) - r (1 + 2^-8), with mu_i in terms of the ray's own p; the reach is
//    minT |d| rounded up (closest) or sqrt(gap) rounded up (shadow), any o;
//  * the box reach: tn <= t* needs t* > 0 (the 1e-5 window) and t* <= minT,
//    or |t* d|^2 < gap, so t* < sqrt(gap / a) (1 + 2^-18), at most 1000.
// The 64-sphere path has no origin precondition at all: candidate_masks64
// evaluates the reference's own radicand (same operations, same value), and
// pass2's Markstein quotient (ray_sphere_k<true>) is chosen by all(q.fast), a
// condition on 2 a alone; the quotient's proof (tests/fpcheck/
// markstein_check.c) is about the float pair (x, den), any numerator: a
// quotient in the (1e-5, 10000) window has x >= 2^-77, far from underflow,
// and one whose product overflows is rejected by both forms (inf or NaN).
//
// FP contract: the Makefile's FPFLAGS; fused multiply-adds only inside the
// culls of rtg_trace.h (slab_pass, the screen); the root test is the shared
// ray_sphere*.
//
// rtg_intersect_host / rtg_visible_host: walk 0 = plain loops (closest_hit /
// blocked over the caller's array), the yardstick; walk 1 = the functions the
// kernels call (ray_closest / ray_blocked) over the packed scene tables
// (HostScene, rtg_host_scene.h: the scene of every walk-1 host form), one ray
// per "wave".  The argument checks shared with the other entry points, and
// the batch grid (ray_blocks), are rtg_entry.h's.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_entry.h"
#include "rtg_host_scene.h"
#include "rtg_trace_kernels.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"

static_assert(sizeof(rtg_ray) == 24 && sizeof(rtg_segment) == 24, "rays are 24 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, t) == 4 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout (two 16-byte halves)");

namespace rtg {

// The hit record of ray (o, d) with closest hit (id, t) as two 16-byte
// halves; point and normal of the winner (raytracer.h:172-177), c its centre.
RTG_HD void hit_record(V3 o, V3 d, int id, float t, V3 c, unsigned* w) {
  V3 P = v3(0.f, 0.f, 0.f), N = v3(0.f, 0.f, 0.f);
  if (id >= 0) {
    P = vadd(o, vsmul(t, d));
    N = vnorm(vsub(P, c));
  }
  w[0] = (unsigned)id;
  w[1] = nan_bits(t);
  w[2] = nan_bits(P.x);
  w[3] = nan_bits(P.y);
  w[4] = nan_bits(P.z);
  w[5] = nan_bits(N.x);
  w[6] = nan_bits(N.y);
  w[7] = nan_bits(N.z);
}

// ---- host forms ----

// A host query's scene: the caller's array for the plain loops (walk 0), or
// the packed tables with the origin box of their BVH, if any (walk 1).
struct HostRayJob {
  const rtg_sphere* spheres;
  unsigned n;
  const PackedScene* ps;  // walk 1
  RayBox box;
};

static V3 host_centre(const HostRayJob& j, int id) {
  if (id < 0) return v3(0.f, 0.f, 0.f);
  return v3(j.spheres[id].pos.x, j.spheres[id].pos.y, j.spheres[id].pos.z);
}

// The two queries over either scene: the plain loops, or the functions the
// kernels call, with every lane of the one-ray "wave" active.
static int host_closest(const HostSpheres& sc, const RayBox&, V3 o, V3 d, float& t) {
  return closest_hit(sc, o, d, t);
}
template <bool kBvh>
static int host_closest(const HostScene<kBvh>& sc, const RayBox& box, V3 o, V3 d, float& t) {
  return ray_closest<kBvh>(sc, box, o, d, true, t);
}
static bool host_blocked(const HostSpheres& sc, const RayBox&, V3 o, V3 d, float gap) {
  return blocked(sc, o, d, gap);
}
template <bool kBvh>
static bool host_blocked(const HostScene<kBvh>& sc, const RayBox& box, V3 o, V3 d, float gap) {
  return ray_blocked<kBvh>(sc, box, o, d, gap, true);
}

// body(sc) with the job's scene: the setup of both range functions.
template <class Body>
static void with_host_scene(const HostRayJob& j, Body&& body) {
  if (!j.ps) body(HostSpheres{j.spheres, j.n});
  else if (!j.ps->bvhNodes.empty()) body(HostScene<true>(*j.ps, true));
  else body(HostScene<false>(*j.ps, true));
}

static void intersect_host_range(const HostRayJob& j, const rtg_ray* rays, size_t k0, size_t k1,
                                 rtg_hit* hits) {
  with_host_scene(j, [&](const auto& sc) {
    for (size_t k = k0; k < k1; ++k) {
      const V3 o = v3(rays[k].origin.x, rays[k].origin.y, rays[k].origin.z);
      const V3 d = v3(rays[k].dir.x, rays[k].dir.y, rays[k].dir.z);
      float t;
      const int id = host_closest(sc, j.box, o, d, t);
      unsigned w[8];
      hit_record(o, d, id, t, host_centre(j, id), w);
      memcpy(&hits[k], w, sizeof w);
    }
  });
}

static void visible_host_range(const HostRayJob& j, const rtg_segment* segs, size_t k0, size_t k1,
                               unsigned char* out) {
  with_host_scene(j, [&](const auto& sc) {
    for (size_t k = k0; k < k1; ++k) {
      const V3 a = v3(segs[k].a.x, segs[k].a.y, segs[k].a.z);
      const V3 b = v3(segs[k].b.x, segs[k].b.y, segs[k].b.z);
      float gap;
      const V3 d = segment_ray(a, b, gap);
      out[k] = host_blocked(sc, j.box, a, d, gap) ? 0 : 1;
    }
  });
}

// ---- device side ----

// Which record lane k of a launch works on: k itself (order null, a constant
// of the un-indexed kernels), or order[k] of an _indexed launch.
// Lanes past n, and lanes whose entry is not an index of the batch (>= n:
// never dereferenced), are not `active`: they take the last record and store
// nothing.
__device__ __forceinline__ size_t ray_slot(const unsigned* __restrict__ order, size_t k, size_t n,
                                           bool& active) {
  active = k < n;
  size_t at = active ? k : n - 1;
  if (order) {
    const unsigned e = order[at];  // at < n: inside the index list
    active = active && e < n;
    at = active ? (size_t)e : n - 1;
  }
  return at;
}

// One lane per ray; n > 0.  Inactive lanes (ray_slot) take the last ray.
template <bool kBvh>
__device__ __forceinline__ void intersect_body(const SceneTables& a, const RayBox& box,
                                               const rtg_ray* __restrict__ rays,
                                               const unsigned* __restrict__ order, size_t n,
                                               rtg_hit* __restrict__ hits, int* stk) {
  RayScene<kBvh> sc;
  bind_scene_no_frames(sc, a, stk);  // stk: the wave's BVH traversal stack
  bool active;
  const size_t k = ray_slot(order, (size_t)blockIdx.x * 64 + threadIdx.x, n, active);
  const float* r = reinterpret_cast<const float*>(rays + k);  // k < n: 24 B of the batch
  const V3 o = v3(r[0], r[1], r[2]);
  const V3 d = v3(r[3], r[4], r[5]);
  float t;
  const int id = ray_closest<kBvh>(sc, box, o, d, active, t);
  if (active) {  // k < n: inside the batch's records
    V3 c = v3(0.f, 0.f, 0.f);
    float r2;
    if (id >= 0) c = sc.sphere_lane((unsigned)id, r2);  // id < n: a scene record
    unsigned w[8];
    hit_record(o, d, id, t, c, w);
    store_record(hits + k, w);
  }
}

template <bool kBvh>
__global__ __launch_bounds__(64) void intersect_kernel(const SceneTables a, const RayBox box,
                                                       const rtg_ray* __restrict__ rays, size_t n,
                                                       rtg_hit* __restrict__ hits) {
  __shared__ int stk[kBvh ? 64 : 1];
  intersect_body<kBvh>(a, box, rays, nullptr, n, hits, stk);
}

template <bool kBvh>
__global__ __launch_bounds__(64) void intersect_indexed_kernel(
    const SceneTables a, const RayBox box, const rtg_ray* __restrict__ rays,
    const unsigned* __restrict__ order, size_t n, rtg_hit* __restrict__ hits) {
  __shared__ int stk[kBvh ? 64 : 1];
  intersect_body<kBvh>(a, box, rays, order, n, hits, stk);
}

template <bool kBvh>
__device__ __forceinline__ void visible_body(const SceneTables& a, const RayBox& box,
                                             const rtg_segment* __restrict__ segs,
                                             const unsigned* __restrict__ order, size_t n,
                                             unsigned char* __restrict__ out, int* stk) {
  RayScene<kBvh> sc;
  bind_scene_no_frames(sc, a, stk);  // stk: the wave's BVH traversal stack
  bool active;
  const size_t k = ray_slot(order, (size_t)blockIdx.x * 64 + threadIdx.x, n, active);
  const float* r = reinterpret_cast<const float*>(segs + k);  // k < n: 24 B of the batch
  const V3 pa = v3(r[0], r[1], r[2]);
  const V3 pb = v3(r[3], r[4], r[5]);
  float gap;
  const V3 d = segment_ray(pa, pb, gap);
  const bool blk = ray_blocked<kBvh>(sc, box, pa, d, gap, active);
  if (active) out[k] = blk ? 0 : 1;  // k < n
}

template <bool kBvh>
__global__ __launch_bounds__(64) void visible_kernel(const SceneTables a, const RayBox box,
                                                     const rtg_segment* __restrict__ segs,
                                                     size_t n, unsigned char* __restrict__ out) {
  __shared__ int stk[kBvh ? 64 : 1];
  visible_body<kBvh>(a, box, segs, nullptr, n, out, stk);
}

template <bool kBvh>
__global__ __launch_bounds__(64) void visible_indexed_kernel(
    const SceneTables a, const RayBox box, const rtg_segment* __restrict__ segs,
    const unsigned* __restrict__ order, size_t n, unsigned char* __restrict__ out) {
  __shared__ int stk[kBvh ? 64 : 1];
  visible_body<kBvh>(a, box, segs, order, n, out, stk);
}

}  // namespace rtg

using namespace rtg;

// Argument checks of the host and one-shot forms (no HIP call).
static int check_ray_args(const char* what, const rtg_sphere* spheres, unsigned sphNum,
                          const void* in, const void* out) {
  if (!in || !out) {
    rtg_set_error("%s: null %s buffer", what, in ? "output" : "input");
    return RTG_ERR_INVALID;
  }
  return check_scene_arrays(what, spheres, sphNum);
}

static int host_job(const char* what, const rtg_sphere* spheres, unsigned sphNum, int walk,
                    PackedScene* ps, HostRayJob* job) {
  int rc = check_walk(what, walk);
  if (rc) return rc;
  job->spheres = spheres;
  job->n = sphNum;
  job->ps = nullptr;
  job->box = RayBox{};
  if (walk == 1) {
    rc = check_sphere_count(what, sphNum);
    if (rc) return rc;
    pack_scene(spheres, sphNum, nullptr, 0, ps);  // as rtg_context_set_scene
    job->ps = ps;
    job->box = ray_box(ps->originBox);
  }
  return RTG_OK;
}

extern "C" {

int rtg_intersect_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_ray* rays, size_t n,
                       rtg_hit* hitsHost, int walk, int nthreads) {
  rtg_clear_error();
  int rc = check_ray_args("intersect", spheres, sphNum, rays, hitsHost);
  if (rc) return rc;
  PackedScene ps;
  HostRayJob job;
  rc = host_job("intersect", spheres, sphNum, walk, &ps, &job);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  host_bands(n, nthreads,
             [&](size_t k0, size_t k1) { intersect_host_range(job, rays, k0, k1, hitsHost); });
  return RTG_OK;
}

int rtg_visible_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_segment* segs, size_t n,
                     unsigned char* outHost, int walk, int nthreads) {
  rtg_clear_error();
  int rc = check_ray_args("visible", spheres, sphNum, segs, outHost);
  if (rc) return rc;
  PackedScene ps;
  HostRayJob job;
  rc = host_job("visible", spheres, sphNum, walk, &ps, &job);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  host_bands(n, nthreads,
             [&](size_t k0, size_t k1) { visible_host_range(job, segs, k0, k1, outHost); });
  return RTG_OK;
}

// The device launch of rtg_intersect_device (order null) and of its _indexed form.
static int intersect_launch(rtg_context* ctx, const rtg_ray* raysDevice, const unsigned* order,
                            bool indexed, size_t n, rtg_hit* hitsDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0;
  if (!rtg_context_scene(ctx, &a, &device, &box)) {
    rtg_set_error("intersect: no context/scene");
    return RTG_ERR_INVALID;
  }
  if (!raysDevice || !hitsDevice) {
    rtg_set_error("intersect: null %s buffer", raysDevice ? "hit" : "ray");
    return RTG_ERR_INVALID;
  }
  if (((uintptr_t)hitsDevice & 15u) != 0) {
    rtg_set_error("intersect: hits not 16-byte aligned");
    return RTG_ERR_INVALID;
  }
  if (indexed && !order) {
    rtg_set_error("intersect: null order buffer");
    return RTG_ERR_INVALID;
  }
  if (n == 0) return RTG_OK;
  unsigned blocks;
  const int rc = ray_blocks("intersect", "batch", n, &blocks);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  if (indexed) {
    void (*fn)(const SceneTables, const RayBox, const rtg_ray*, const unsigned*, size_t,
               rtg_hit*) = a.bvhNodes ? intersect_indexed_kernel<true> : intersect_indexed_kernel<false>;
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, box, raysDevice,
                       order, n, hitsDevice);
  } else {
    void (*fn)(const SceneTables, const RayBox, const rtg_ray*, size_t, rtg_hit*) =
        a.bvhNodes ? intersect_kernel<true> : intersect_kernel<false>;
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, box, raysDevice, n,
                       hitsDevice);
  }
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

static int visible_launch(rtg_context* ctx, const rtg_segment* segsDevice, const unsigned* order,
                          bool indexed, size_t n, unsigned char* outDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0;
  if (!rtg_context_scene(ctx, &a, &device, &box)) {
    rtg_set_error("visible: no context/scene");
    return RTG_ERR_INVALID;
  }
  if (!segsDevice || !outDevice) {
    rtg_set_error("visible: null %s buffer", segsDevice ? "output" : "segment");
    return RTG_ERR_INVALID;
  }
  if (indexed && !order) {
    rtg_set_error("visible: null order buffer");
    return RTG_ERR_INVALID;
  }
  if (n == 0) return RTG_OK;
  unsigned blocks;
  const int rc = ray_blocks("visible", "batch", n, &blocks);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  if (indexed) {
    void (*fn)(const SceneTables, const RayBox, const rtg_segment*, const unsigned*, size_t,
               unsigned char*) =
        a.bvhNodes ? visible_indexed_kernel<true> : visible_indexed_kernel<false>;
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, box, segsDevice,
                       order, n, outDevice);
  } else {
    void (*fn)(const SceneTables, const RayBox, const rtg_segment*, size_t, unsigned char*) =
        a.bvhNodes ? visible_kernel<true> : visible_kernel<false>;
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, box, segsDevice, n,
                       outDevice);
  }
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_intersect_device(rtg_context* ctx, const rtg_ray* raysDevice, size_t n,
                         rtg_hit* hitsDevice, void* stream) {
  return intersect_launch(ctx, raysDevice, nullptr, false, n, hitsDevice, stream);
}

int rtg_intersect_indexed_device(rtg_context* ctx, const rtg_ray* raysDevice,
                                 const unsigned* orderDevice, size_t n, rtg_hit* hitsDevice,
                                 void* stream) {
  return intersect_launch(ctx, raysDevice, orderDevice, true, n, hitsDevice, stream);
}

int rtg_visible_device(rtg_context* ctx, const rtg_segment* segsDevice, size_t n,
                       unsigned char* outDevice, void* stream) {
  return visible_launch(ctx, segsDevice, nullptr, false, n, outDevice, stream);
}

int rtg_visible_indexed_device(rtg_context* ctx, const rtg_segment* segsDevice,
                               const unsigned* orderDevice, size_t n, unsigned char* outDevice,
                               void* stream) {
  return visible_launch(ctx, segsDevice, orderDevice, true, n, outDevice, stream);
}

int rtg_intersect(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_ray* rays,
                  size_t n, rtg_hit* hitsHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  const int rc = check_ray_args("intersect", spheres, sphNum, rays, hitsHost);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  return one_shot("intersect", device, {spheres, sphNum, nullptr, 0}, rays, n * sizeof(rtg_ray),
                  hitsHost, n * sizeof(rtg_hit), [&](rtg_context* ctx, const void* in, void* out) {
                    return rtg_intersect_device(ctx, (const rtg_ray*)in, n, (rtg_hit*)out, nullptr);
                  });
}

int rtg_visible(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_segment* segs,
                size_t n, unsigned char* outHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  const int rc = check_ray_args("visible", spheres, sphNum, segs, outHost);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  return one_shot("visible", device, {spheres, sphNum, nullptr, 0}, segs, n * sizeof(rtg_segment),
                  outHost, n,
                  [&](rtg_context* ctx, const void* in, void* out) {
                    return rtg_visible_device(ctx, (const rtg_segment*)in, n, (unsigned char*)out,
                                              nullptr);
                  });
}

}  // extern "C"
