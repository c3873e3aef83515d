// rtg_ao.hip — ambient occlusion of librtg.so (rtg_ao*, rtg.h): hit points in,
// one count of unoccluded probes per point out.
//
// Point i has K probe segments from a = P + bias N to b = a + radius w_k, w_k
// the caller's local direction dirs[j] turned into the frame of the normal
// (ao_point, ao_end, rtg_ao.h: one definition for every form below), and its
// count is the number of k with hasClearLineOfSight(a, b), the line of sight
// of rtg_visible (segment_ray and ray_blocked, rtg_rays.h).  The fused count
// is therefore, word for word, the per-point sum of rtg_visible_host(walk 0)
// over rtg_ao_segments_host's segments: no segment buffer (24 K bytes per
// point), no sort and no fold on the caller's side.
//
// ao_kernel: one lane per point in one-wave workgroups, the wave's BVH stack
// in LDS (visible_kernel's mapping, rtg_rays.hip).  The K probes of a point
// share their origin, so a wave's 64 lanes stay on neighbouring origins for
// the whole loop, and what depends on the origin alone is taken once per
// point: the frame, a, and ray_delta (the BVH boxes' widening for that origin;
// ray_blocked's overload takes it).  The loop over k is wave-uniform: every
// lane runs all K iterations and the whole wave enters every BVH walk, lanes
// past n and records with id < 0 as inactive queries (never blocked: their
// count comes out as K).  Without RTG_AO_JITTER the direction index is k for
// the whole wave and the table is read through the scalar path; with it each
// lane gathers from its own window of a table of at most 768 KiB, 12 K bytes
// of it live per lane.  The two are kernels of their own (kJitter), as the
// BVH and the flat scene are (kBvh).  Bounds: a record index is < n (lanes
// past n read record n - 1 and store nothing), a table index < nDirs
// (ao_dir_index), an output index < n.
//
// The segment generator is rtg_probes.h's, with the far end as its tail.
//
// rtg_ao_host: walk 0 = plain loops (blocked over the caller's array), the
// yardstick; walk 1 = the kernel's own path (ray_blocked with the hoisted
// delta) over the packed tables, one point per "wave".
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_ao.h"
#include "rtg_entry.h"
#include "rtg_host_scene.h"
#include "rtg_probes.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"
#include "rtg_trace_kernels.h"

static_assert(sizeof(rtg_ao_params) == 20, "rtg_ao_params is 20 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");
static_assert(sizeof(rtg_segment) == 24 && sizeof(rtg_vec) == 12, "24 B per segment");
static_assert(RTG_AO_MAX_SAMPLES <= 0xFFFF, "a count fits an unsigned short");

namespace rtg {

// A probe segment's last three words: its far end.
struct AoEnd {
  float radius;
  RTG_HD V3 operator()(const AoPoint& pt, V3 l) const { return ao_end(pt, l, radius); }
};
static AoEnd ao_end_of(const rtg_ao_params& p) { return AoEnd{p.radius}; }

// One lane per point; n > 0.
template <bool kBvh, bool kJitter>
__global__ __launch_bounds__(64) void ao_kernel(const SceneTables a, const RayBox box,
                                                const rtg_hit* __restrict__ hits, size_t n,
                                                const rtg_ao_params p,
                                                const rtg_vec* __restrict__ dirs, unsigned nDirs,
                                                unsigned short* __restrict__ out) {
  __shared__ int stk[kBvh ? 64 : 1];
  RayScene<kBvh> sc;
  bind_scene_no_frames(sc, a, stk);  // stk: the wave's BVH traversal stack
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool inside = i < n;
  const AoPoint pt = ao_point(hits + (inside ? i : n - 1), p.bias);  // < n: a batch record
  const bool active = inside && pt.id >= 0;
  float delta = 0.f;
  bool oddOrigin = false;
  if constexpr (kBvh) delta = ray_delta(box, pt.a, oddOrigin);
  const unsigned s = kJitter ? ao_window(p, i, nDirs) : 0u;
  unsigned count = 0;
  for (unsigned k = 0; k < p.samples; ++k) {
    // (not kJitter: k for the whole wave, a scalar load; k < K <= nDirs)
    const V3 l = ao_dir(dirs, kJitter ? ao_dir_index(s, k, nDirs) : k);
    float gap;
    const V3 d = segment_ray(pt.a, ao_end(pt, l, p.radius), gap);
    count += ray_blocked<kBvh>(sc, pt.a, d, gap, active, delta, oddOrigin) ? 0u : 1u;
  }
  if (inside) out[i] = (unsigned short)count;  // i < n; an inactive lane's count is K
}

// ---- host forms ----

static bool ao_blocked(const HostSpheres& sc, V3 o, V3 d, float gap, float, bool) {
  return blocked(sc, o, d, gap);
}
template <bool kBvh>
static bool ao_blocked(const HostScene<kBvh>& sc, V3 o, V3 d, float gap, float delta,
                       bool oddOrigin) {
  return ray_blocked<kBvh>(sc, o, d, gap, true, delta, oddOrigin);
}
static float ao_delta(const HostSpheres&, const RayBox&, V3, bool&) { return 0.f; }
template <bool kBvh>
static float ao_delta(const HostScene<kBvh>&, const RayBox& box, V3 o, bool& oddOrigin) {
  if constexpr (kBvh) return ray_delta(box, o, oddOrigin);
  return 0.f;
}

// Points [i0, i1) over the plain loops' scene or the packed tables.
template <class Scene>
static void ao_host_range(const Scene& sc, const RayBox& box, const rtg_hit* hits, size_t i0,
                          size_t i1, const rtg_ao_params& p, const rtg_vec* dirs, unsigned nDirs,
                          unsigned short* out) {
  for (size_t i = i0; i < i1; ++i) {
    const AoPoint pt = ao_point(hits + i, p.bias);
    unsigned count = p.samples;
    if (pt.id >= 0) {
      bool oddOrigin = false;
      const float delta = ao_delta(sc, box, pt.a, oddOrigin);
      const unsigned s = ao_window(p, i, nDirs);
      count = 0;
      for (unsigned k = 0; k < p.samples; ++k) {
        const V3 l = ao_dir(dirs, ao_dir_index(s, k, nDirs));
        float gap;
        const V3 d = segment_ray(pt.a, ao_end(pt, l, p.radius), gap);
        count += ao_blocked(sc, pt.a, d, gap, delta, oddOrigin) ? 0u : 1u;
      }
    }
    out[i] = (unsigned short)count;
  }
}

}  // namespace rtg

using namespace rtg;

// The checks every form shares, in the order they are reported in.
static int check_ao(const rtg_hit* hits, const rtg_ao_params* p, const rtg_vec* dirs,
                    unsigned nDirs, const void* out, size_t n) {
  const int rc = check_probes("ao", RTG_AO_JITTER, hits, p, dirs, false, nullptr, nDirs, out);
  return rc ? rc : check_probe_points("ao", n);
}

extern "C" {

int rtg_ao_directions(unsigned nDirs, rtg_vec* out) {
  rtg_clear_error();
  if (!out || nDirs < 1 || nDirs > RTG_AO_MAX_DIRS) {
    rtg_set_error(out ? "ao_directions: %u directions outside [1, %d]"
                      : "ao_directions: null table (%u directions, at most %d)",
                  nDirs, RTG_AO_MAX_DIRS);
    return RTG_ERR_INVALID;
  }
  const double kTwoPi = 6.283185307179586476925286766559;
  for (unsigned k = 0; k < nDirs; ++k) {
    const double u = ((double)k + 0.5) / (double)nDirs;
    const double g = (double)k * 0.6180339887498949;
    const double phi = kTwoPi * (g - floor(g));
    const double r = sqrt(u);
    out[k].x = (float)(r * cos(phi));
    out[k].y = (float)(r * sin(phi));
    out[k].z = (float)sqrt(1.0 - u);
  }
  return RTG_OK;
}

int rtg_ao_segments_host(const rtg_hit* hits, size_t n, const rtg_ao_params* params,
                         const rtg_vec* dirs, unsigned nDirs, rtg_segment* segsHost,
                         int nthreads) {
  return probes_host("ao_segments", RTG_AO_JITTER, hits, n, params, ao_end_of, dirs, nDirs,
                     segsHost, nthreads);
}

int rtg_ao_segments_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                           const rtg_ao_params* params, const rtg_vec* dirsDevice,
                           unsigned nDirs, rtg_segment* segsDevice, void* stream) {
  return probes_device("ao_segments", RTG_AO_JITTER, ctx, hitsDevice, n, params, ao_end_of,
                       dirsDevice, nDirs, segsDevice, stream);
}

int rtg_ao_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                  const rtg_ao_params* params, const rtg_vec* dirsDevice, unsigned nDirs,
                  unsigned short* outDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0;
  if (!rtg_context_scene(ctx, &a, &device, &box)) {
    rtg_set_error("ao: no context/scene");
    return RTG_ERR_INVALID;
  }
  int rc = check_ao(hitsDevice, params, dirsDevice, nDirs, outDevice, n);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  unsigned blocks;
  rc = ray_blocks("ao", "batch", n, &blocks);
  if (rc) return rc;
  const bool bvh = a.bvhNodes != nullptr, jitter = (params->flags & RTG_AO_JITTER) != 0;
  void (*fn)(const SceneTables, const RayBox, const rtg_hit*, size_t, const rtg_ao_params,
             const rtg_vec*, unsigned, unsigned short*) =
      bvh ? (jitter ? ao_kernel<true, true> : ao_kernel<true, false>)
          : (jitter ? ao_kernel<false, true> : ao_kernel<false, false>);
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, box, hitsDevice, n,
                     *params, dirsDevice, nDirs, outDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_ao_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits, size_t n,
                const rtg_ao_params* params, const rtg_vec* dirs, unsigned nDirs,
                unsigned short* outHost, int walk, int nthreads) {
  rtg_clear_error();
  int rc = check_ao(hits, params, dirs, nDirs, outHost, n);
  if (!rc) rc = check_scene_arrays("ao", spheres, sphNum);
  if (!rc) rc = check_walk("ao", walk);
  if (!rc && walk == 1) rc = check_sphere_count("ao", sphNum);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  const rtg_ao_params p = *params;
  PackedScene ps;
  RayBox box{};
  if (walk == 1) {
    pack_scene(spheres, sphNum, nullptr, 0, &ps);  // as rtg_context_set_scene
    box = ray_box(ps.originBox);
  }
  auto run = [&](const auto& sc) {
    host_bands(n, nthreads, [&](size_t i0, size_t i1) {
      ao_host_range(sc, box, hits, i0, i1, p, dirs, nDirs, outHost);
    });
  };
  if (walk == 0) run(HostSpheres{spheres, sphNum});
  else if (!ps.bvhNodes.empty()) run(HostScene<true>(ps, true));
  else run(HostScene<false>(ps, true));
  return RTG_OK;
}

int rtg_ao(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits, size_t n,
           const rtg_ao_params* params, const rtg_vec* dirs, unsigned nDirs,
           unsigned short* outHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int rc = check_ao(hits, params, dirs, nDirs, outHost, n);
  if (!rc) rc = check_scene_arrays("ao", spheres, sphNum);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  const StageScene scene{spheres, sphNum, nullptr, 0};
  return one_shot("ao", device, &scene,
                  {{n * sizeof(rtg_hit), hits, nullptr},
                   {(size_t)nDirs * sizeof(rtg_vec), dirs, nullptr},
                   {n * sizeof(unsigned short), nullptr, outHost}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_ao_device(ctx, (const rtg_hit*)d[0], n, params,
                                         (const rtg_vec*)d[1], nDirs, (unsigned short*)d[2],
                                         nullptr);
                  });
}

}  // extern "C"
