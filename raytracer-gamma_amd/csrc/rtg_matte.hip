// rtg_matte.hip — direct lighting and containment of librtg.so for a caller's
// own points (rtg_matte*, rtg_contains*, rtg.h): the two scene functions of the
// reference that lived only inside the trace kernels, as batch calls.
//
// rtg_matte: calculateMatte (raytracer.h:313-367) of hit record i, the sum over
// the context's lights of incidence / gap * colour for every light the point
// faces and sees, and a 64-bit mask of those lights.  The arithmetic is
// matte_light's (rtg_trace.h), the ONE definition the render and raytrace
// kernels shade with; no copy of the light loop lives here.  What this file
// adds is the query path it runs over, MattePath: every shadow ray is
// ray_blocked (rtg_rays.h), exact for any origin (the argument is at the head
// of rtg_rays.hip), with ray_delta of the point taken once, since the m
// shadow rays of a point share their origin (the overload written for the K
// probes of an ambient-occlusion point).  matte_light is instantiated with
// Q == 2 and a path that is kOn, as trace_ray instantiates it: no shadow mask,
// no capsule list and no facing-away pre-test, which rest on guard-ball and
// range arguments (rtg_raytrace.hip's table) that a caller's record does not
// promise; `id` is read for its sign and never used as an index.
//
// matte_kernel: one lane per point in one-wave workgroups, the wave's BVH
// stack in LDS (ao_kernel's mapping, rtg_ao.hip).  The loop over the lights is
// wave-uniform and a light's 24-byte record comes through the scalar path
// (sc.light with the loop's index).  matte_light tests incidence > 0 ahead of
// the query (the visibility test has no side effect): lanes that fail it are
// not in the walk, and a light no lane of the wave faces makes no walk.
// Lanes past n and records with id < 0 enter as inactive queries (never
// blocked) and store zeros, or nothing.  Bounds: a record index is < n (lanes
// past n read record n - 1 and store nothing), a light index < m, an output
// index < n.
//
// contains_kernel: primaryContainer (raytracer.h:245-270) of point i, one lane
// per point: primary_container (rtg_trace.h) on the same scene, four
// containment records per step without a BVH, container_bvh with one.
// container_bvh needs no origin treatment: it descends into a child when the
// POINT is inside the child's stored box (plain comparisons, no slab
// arithmetic; NaN and infinity fail them as they fail the reference's <=), and
// a sphere's containment ball (r + 1e-6, accepted at most a few ulps of
// |pt - c|^2 outside, a bound in r alone) lies inside its grown box of
// half-width >= r + 2^-8 r + 2^-20 (rtg_raytrace.hip's header).
//
// Host forms: walk 0 = the plain loops, the yardstick (matte_light<0> with
// blocked over every sphere, the scene rtg_raytrace_host's walk 0 shades on;
// for containment the literal loop over the caller's array); walk 1 = the
// kernels' own path over the packed tables, one point per "wave".
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_entry.h"
#include "rtg_host_scene.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"
#include "rtg_trace_kernels.h"

static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");
static_assert(sizeof(rtg_vec) == 12 && sizeof(unsigned long long) == 8, "12 + 8 B per point");

namespace rtg {

// A hit record's sign, point and normal (32 B, read as words: no alignment
// beyond a float's is asked of the caller's buffer).
struct MattePoint {
  int id;
  V3 P, N;
};

RTG_HD MattePoint matte_point(const rtg_hit* hit) {
  const float* w = reinterpret_cast<const float*>(hit);
  MattePoint p;
  memcpy(&p.id, w, 4);
  p.P = v3(w[2], w[3], w[4]);
  p.N = v3(w[5], w[6], w[7]);
  return p;
}

// The lights matte_light found lit, as the mask of the first 64.
struct LitMask {
  mutable unsigned long long mask = 0;
  RTG_HD void lit(unsigned l) const {
    if (l < 64) mask |= 1ull << l;
  }
};

// matte_light's query path for a caller's point: ray_blocked with the delta of
// the point, taken once (a scene without a BVH reads neither member).
template <bool kBvh>
struct MattePath : LitMask {
  static constexpr bool kOn = true;
  float delta = 0.f;
  bool oddOrigin = false, active = true;
  template <class Scene>
  RTG_HD bool blocked(const Scene& sc, V3 o, V3 d, float gap) const {
    return ray_blocked<kBvh>(sc, o, d, gap, active, delta, oddOrigin);
  }
};

// The same for the plain loops: every sphere for every shadow ray.
struct MattePlainPath : LitMask {
  static constexpr bool kOn = true;
  template <class Scene>
  RTG_HD bool blocked(const Scene& sc, V3 o, V3 d, float gap) const {
    return rtg::blocked(sc, o, d, gap);
  }
};

// calculateMatte of (P, N) over path rp: matte_light with no hit sphere, no
// guard ball and no cell, as a caller's record has none.
template <int Q, class Path, class Scene>
RTG_HD V3 matte_of(const Scene& sc, V3 P, V3 N, const Path& rp) {
  return matte_light<Q, Path>(sc, P, N, -1, false, kCapFull, V3{}, 0.f, rp);
}

// One lane per point; n > 0.
template <bool kBvh>
__global__ __launch_bounds__(64) void matte_kernel(const SceneTables a, const RayBox box,
                                                   const rtg_hit* __restrict__ hits, size_t n,
                                                   rtg_vec* __restrict__ out,
                                                   unsigned long long* __restrict__ lit) {
  __shared__ int stk[kBvh ? 64 : 1];
  RayScene<kBvh> sc;
  bind_scene_no_frames(sc, a, stk);  // stk: the wave's BVH traversal stack
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool inside = i < n;
  const MattePoint pt = matte_point(hits + (inside ? i : n - 1));  // < n: a batch record
  MattePath<kBvh> rp;
  rp.active = inside && pt.id >= 0;
  if constexpr (kBvh) rp.delta = ray_delta(box, pt.P, rp.oddOrigin);
  const V3 sum = matte_of<2>(sc, pt.P, pt.N, rp);
  if (inside) {  // i < n; a record without a point: zeros
    unsigned* o = reinterpret_cast<unsigned*>(out + i);
    o[0] = rp.active ? nan_bits(sum.x) : 0u;
    o[1] = rp.active ? nan_bits(sum.y) : 0u;
    o[2] = rp.active ? nan_bits(sum.z) : 0u;
  }
  if (lit) {  // wave-uniform: a kernel argument
    if (inside) lit[i] = rp.active ? rp.mask : 0ull;
  }
}

// One lane per point; n > 0.  Lanes past n take the last point.
template <bool kBvh>
__global__ __launch_bounds__(64) void contains_kernel(const SceneTables a,
                                                      const rtg_vec* __restrict__ pts, size_t n,
                                                      int* __restrict__ out) {
  __shared__ int stk[kBvh ? 64 : 1];
  RayScene<kBvh> sc;
  bind_scene_no_frames(sc, a, stk);  // stk: the wave's BVH traversal stack
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool inside = i < n;
  const float* w = reinterpret_cast<const float*>(pts + (inside ? i : n - 1));  // < n
  const int id = primary_container(sc, v3(w[0], w[1], w[2]));
  if (inside) out[i] = id;  // i < n
}

// ---- host forms ----

static void store_matte(rtg_vec* out, unsigned long long* lit, size_t i, bool real, V3 sum,
                        unsigned long long mask) {
  store_colour(out + i, real ? sum : v3(0.f, 0.f, 0.f));
  if (lit) lit[i] = real ? mask : 0ull;
}

// Points [i0, i1): kWalk the kernel's path over the packed tables, else the
// plain loops.
template <bool kWalk, bool kBvh>
static void matte_host_range(const PackedScene& ps, const RayBox& box, const rtg_hit* hits,
                             size_t i0, size_t i1, rtg_vec* out, unsigned long long* lit) {
  const HostScene<kBvh> sc(ps, kWalk);  // walk 0: no masks, no BVH, no lists
  for (size_t i = i0; i < i1; ++i) {
    const MattePoint pt = matte_point(hits + i);
    if (pt.id < 0) {
      store_matte(out, lit, i, false, V3{}, 0);
    } else if constexpr (kWalk) {
      MattePath<kBvh> rp;
      if constexpr (kBvh) rp.delta = ray_delta(box, pt.P, rp.oddOrigin);
      const V3 sum = matte_of<2>(sc, pt.P, pt.N, rp);
      store_matte(out, lit, i, true, sum, rp.mask);
    } else {
      const MattePlainPath rp;
      const V3 sum = matte_of<0>(sc, pt.P, pt.N, rp);
      store_matte(out, lit, i, true, sum, rp.mask);
    }
  }
}

// raytracer.h:245-270 over the caller's array.
static int contains_plain(const rtg_sphere* s, unsigned n, V3 p) {
  for (unsigned k = 0; k < n; ++k) {
    const float r = s[k].radius + 1.0e-6f;
    const V3 d = vsub(p, v3(s[k].pos.x, s[k].pos.y, s[k].pos.z));
    if (vdot(d, d) <= r * r) return (int)k;
  }
  return -1;
}

static V3 host_point(const rtg_vec* pts, size_t i) {
  const float* w = reinterpret_cast<const float*>(pts + i);
  return v3(w[0], w[1], w[2]);
}

}  // namespace rtg

using namespace rtg;

// The checks every form shares, in the order they are reported in; `in`: what
// the input buffer holds ("hit", "point").
static int check_points(const char* what, const char* in, const void* src, const void* dst,
                        size_t n) {
  if (!src || !dst) {
    rtg_set_error("%s: null %s buffer", what, src ? "output" : in);
    return RTG_ERR_INVALID;
  }
  if (n > 0xFFFFFFFFull) {
    rtg_set_error("%s: %zu points (at most 2^32 - 1)", what, n);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// The context's scene and the grid of a device call; *blocks == 0: nothing to
// launch (n == 0).
static int device_job(const char* what, const char* in, rtg_context* ctx, const void* src,
                      const void* dst, size_t n, SceneTables* a, RayBox* box, int* device,
                      unsigned* blocks) {
  rtg_clear_error();
  if (!rtg_context_scene(ctx, a, device, box)) {
    rtg_set_error("%s: no context/scene", what);
    return RTG_ERR_INVALID;
  }
  const int rc = check_points(what, in, src, dst, n);
  if (rc) return rc;
  *blocks = 0;
  return n ? ray_blocks(what, "batch", n, blocks) : RTG_OK;
}

// The scene of a host form: packed for walk 1 (as rtg_context_set_scene), and
// for matte's walk 0, whose plain loops read the lights from it.
static int host_scene(const char* what, const rtg_sphere* spheres, unsigned sphNum,
                      const rtg_light* lights, unsigned lgtNum, int walk, bool pack, size_t n,
                      PackedScene* ps, RayBox* box) {
  int rc = check_scene_arrays(what, spheres, sphNum, lights, lgtNum);
  if (!rc) rc = check_walk(what, walk);
  if (!rc && pack) rc = check_sphere_count(what, sphNum);
  if (rc || n == 0 || !pack) return rc;
  pack_scene(spheres, sphNum, lights, lgtNum, ps);
  *box = walk == 1 && !ps->bvhNodes.empty() ? ray_box(ps->originBox) : RayBox{};
  return RTG_OK;
}

extern "C" {

int rtg_matte_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n, rtg_vec* outDevice,
                     unsigned long long* litDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  SceneTables a{};
  RayBox box{};
  int device = 0;
  unsigned blocks = 0;
  const int rc = device_job("matte", "hit", ctx, hitsDevice, outDevice, n, &a, &box, &device,
                            &blocks);
  if (rc || !blocks) return rc;
  void (*fn)(const SceneTables, const RayBox, const rtg_hit*, size_t, rtg_vec*,
             unsigned long long*) = a.bvhNodes ? matte_kernel<true> : matte_kernel<false>;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, box, hitsDevice, n,
                     outDevice, litDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_matte_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                   unsigned lgtNum, const rtg_hit* hits, size_t n, rtg_vec* outHost,
                   unsigned long long* litHost, int walk, int nthreads) {
  rtg_clear_error();
  PackedScene ps;
  RayBox box{};
  int rc = check_points("matte", "hit", hits, outHost, n);
  if (!rc) rc = host_scene("matte", spheres, sphNum, lights, lgtNum, walk, true, n, &ps, &box);
  if (rc || n == 0) return rc;
  void (*fn)(const PackedScene&, const RayBox&, const rtg_hit*, size_t, size_t, rtg_vec*,
             unsigned long long*) =
      walk == 0 ? matte_host_range<false, false>
                : !ps.bvhNodes.empty() ? matte_host_range<true, true>
                                       : matte_host_range<true, false>;
  host_bands(n, nthreads,
             [&](size_t i0, size_t i1) { fn(ps, box, hits, i0, i1, outHost, litHost); });
  return RTG_OK;
}

int rtg_matte(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
              unsigned lgtNum, const rtg_hit* hits, size_t n, rtg_vec* outHost,
              unsigned long long* litHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int rc = check_points("matte", "hit", hits, outHost, n);
  if (!rc) rc = check_scene_arrays("matte", spheres, sphNum, lights, lgtNum);
  if (rc || n == 0) return rc;
  const StageScene scene{spheres, sphNum, lights, lgtNum};
  return one_shot("matte", device, &scene,
                  {{n * sizeof(rtg_hit), hits, nullptr},
                   {n * sizeof(rtg_vec), nullptr, outHost},
                   {litHost ? n * sizeof(unsigned long long) : 0, nullptr, litHost}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_matte_device(ctx, (const rtg_hit*)d[0], n, (rtg_vec*)d[1],
                                            (unsigned long long*)d[2], nullptr);
                  });
}

int rtg_contains_device(rtg_context* ctx, const rtg_vec* pointsDevice, size_t n, int* outDevice,
                        void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  SceneTables a{};
  RayBox box{};
  int device = 0;
  unsigned blocks = 0;
  const int rc = device_job("contains", "point", ctx, pointsDevice, outDevice, n, &a, &box,
                            &device, &blocks);
  if (rc || !blocks) return rc;
  void (*fn)(const SceneTables, const rtg_vec*, size_t, int*) =
      a.bvhNodes ? contains_kernel<true> : contains_kernel<false>;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, pointsDevice, n,
                     outDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_contains_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_vec* points, size_t n,
                      int* outHost, int walk, int nthreads) {
  rtg_clear_error();
  PackedScene ps;
  RayBox box{};
  int rc = check_points("contains", "point", points, outHost, n);
  if (!rc) rc = host_scene("contains", spheres, sphNum, nullptr, 0, walk, walk == 1, n, &ps, &box);
  if (rc || n == 0) return rc;
  auto run = [&](auto&& container) {
    host_bands(n, nthreads, [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; ++i) outHost[i] = container(host_point(points, i));
    });
  };
  if (walk == 0) {
    run([&](V3 p) { return contains_plain(spheres, sphNum, p); });
  } else if (!ps.bvhNodes.empty()) {
    const HostScene<true> sc(ps, true);
    run([&](V3 p) { return primary_container(sc, p); });
  } else {
    const HostScene<false> sc(ps, true);
    run([&](V3 p) { return primary_container(sc, p); });
  }
  return RTG_OK;
}

int rtg_contains(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_vec* points,
                 size_t n, int* outHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int rc = check_points("contains", "point", points, outHost, n);
  if (!rc) rc = check_scene_arrays("contains", spheres, sphNum);
  if (rc || n == 0) return rc;
  return one_shot("contains", device, {spheres, sphNum, nullptr, 0}, points, n * sizeof(rtg_vec),
                  outHost, n * sizeof(int), [&](rtg_context* ctx, const void* in, void* out) {
                    return rtg_contains_device(ctx, (const rtg_vec*)in, n, (int*)out, nullptr);
                  });
}

}  // extern "C"
