// rtg_gather.hip — the gather of librtg.so (rtg_gather*, rtg.h): hit points in,
// one colour per point out, the weighted sum of rayTrace along K directions of
// the point's hemisphere.
//
// Probe k of point i starts at a = P + bias N and runs along vnorm(w_k), w_k
// the caller's local direction dirs[j] turned into the frame of the normal
// (ao_point, ao_window, ao_dir_index, ao_world, rtg_ao.h: rtg_ao's own, and
// gather_dir, rtg_gather_kernels.h).  Its colour is rtg_raytrace's (trace_ray,
// rtg_rays.h: exact for any origin and direction, rtg_raytrace.hip's header),
// and the K colours are added in order with the caller's weights (gather_add).
// The fused sum is therefore, word for word, that sum over
// rtg_raytrace_host(walk 0) of rtg_gather_rays_host's rays: no ray buffer (24 K
// bytes per point), no colour buffer (12 K), no sort and no fold on the
// caller's side.
//
// gather_kernel (rtg_gather_kernels.h, instantiated per stack size in
// rtg_trace_s<S>.hip): one lane per point in one-wave workgroups.
// The ray generator is rtg_probes.h's, with the direction as its tail.
//
// rtg_gather_host: walk 0 = trace_ray_plain, plain loops over every sphere for
// every query, the yardstick; walk 1 = the kernel's own path (trace_ray) over
// the packed tables, one point per "wave".  Its instantiation per stack size
// comes from host_trace_fn (rtg_host_scene.h), as rtg_raytrace_host's.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_ao.h"
#include "rtg_entry.h"
#include "rtg_gather_kernels.h"
#include "rtg_host_scene.h"
#include "rtg_probes.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"

static_assert(sizeof(rtg_gather_params) == 16, "rtg_gather_params is 16 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");
static_assert(sizeof(rtg_ray) == 24 && sizeof(rtg_vec) == 12, "24 B per ray, 12 B per colour");
static_assert(RTG_GATHER_MAX_SAMPLES <= 0xFFFF, "a skip count fits an unsigned short");

namespace rtg {

// A probe ray's last three words: its direction.
struct GatherDir {
  RTG_HD V3 operator()(const AoPoint& pt, V3 l) const { return gather_dir(pt, l); }
};
static GatherDir gather_dir_of(const rtg_gather_params&) { return GatherDir{}; }

// ---- host forms ----

// Points [i0, i1) of the batch; kWalk 1: the kernel's path, else plain loops.
template <int S, bool kCL, bool kWalk, bool kBvh>
static void gather_host_range(const PackedScene& ps, const RayBox& box, const GatherArgs& g,
                              size_t i0, size_t i1) {
  const HostScene<kBvh> sc(ps, kWalk);  // walk 0: no masks, no BVH, no lists
  const bool skip = (g.p.flags & RTG_GATHER_SKIP_NONFINITE) != 0;
  for (size_t i = i0; i < i1; ++i) {
    const AoPoint pt = ao_point(g.hits + i, g.p.bias);
    V3 acc = v3(0.f, 0.f, 0.f);
    unsigned skipped = 0;
    if (pt.id >= 0) {
      const unsigned s = ao_window(g.p.flags, g.p.seed, i, g.nDirs);
      for (unsigned k = 0; k < g.p.samples; ++k) {
        const unsigned j = ao_dir_index(s, k, g.nDirs);
        const V3 d = gather_dir(pt, ao_dir(g.dirs, j));
        V3 c;
        if constexpr (kWalk) c = trace_ray<S, kCL, kBvh>(sc, box, pt.a, d);
        else c = trace_ray_plain<S, kCL>(sc, pt.a, d);
        gather_add(acc, skipped, g.weights[j], c, skip);
      }
    }
    store_colour(g.out + i, acc);
    if (g.skipped) g.skipped[i] = (unsigned short)skipped;
  }
}

typedef void (*HostGatherFn)(const PackedScene&, const RayBox&, const GatherArgs&, size_t, size_t);

}  // namespace rtg

using namespace rtg;

constexpr unsigned kGatherFlags = RTG_GATHER_JITTER | RTG_GATHER_SKIP_NONFINITE;

// The checks the fused forms share, in the order they are reported in.
static int check_gather(const rtg_hit* hits, const rtg_gather_params* p, const rtg_vec* dirs,
                        const float* weights, unsigned nDirs, const void* out, int stackSize) {
  const int rc = check_probes("gather", kGatherFlags, hits, p, dirs, true, weights, nDirs, out);
  return rc ? rc : check_stack("gather", stackSize);
}

extern "C" {

int rtg_gather_rays_host(const rtg_hit* hits, size_t n, const rtg_gather_params* params,
                         const rtg_vec* dirs, unsigned nDirs, rtg_ray* raysHost, int nthreads) {
  return probes_host("gather_rays", kGatherFlags, hits, n, params, gather_dir_of, dirs, nDirs,
                     raysHost, nthreads);
}

int rtg_gather_rays_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                           const rtg_gather_params* params, const rtg_vec* dirsDevice,
                           unsigned nDirs, rtg_ray* raysDevice, void* stream) {
  return probes_device("gather_rays", kGatherFlags, ctx, hitsDevice, n, params, gather_dir_of,
                       dirsDevice, nDirs, raysDevice, stream);
}

int rtg_gather_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                      const rtg_gather_params* params, const rtg_vec* dirsDevice,
                      const float* weightsDevice, unsigned nDirs, int stackSize,
                      rtg_vec* outDevice, unsigned short* skippedDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0, semantics = RTG_SEMANTICS_CPU;
  if (!rtg_context_scene(ctx, &a, &device, &box, &semantics)) {
    rtg_set_error("gather: no context/scene");
    return RTG_ERR_INVALID;
  }
  int rc = check_gather(hitsDevice, params, dirsDevice, weightsDevice, nDirs, outDevice,
                        stackSize);
  if (!rc) rc = check_probe_points("gather", n);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  unsigned blocks;
  rc = ray_blocks("gather", "batch", n, &blocks);
  if (rc) return rc;
  const bool bvh = a.bvhNodes != nullptr;
  const StackKernels* sk = stack_kernels(stackSize);
  const GatherFn fn = sk ? sk->gather(bvh, semantics == RTG_SEMANTICS_OPENCL) : nullptr;
  if (!fn) {  // a missing kernel is an error, never another path
    rtg_set_error("gather: no kernel for stackSize %d", stackSize);
    return RTG_ERR_INVALID;
  }
  const GatherArgs g{hitsDevice, n, *params, dirsDevice, weightsDevice, nDirs, outDevice,
                     skippedDevice};
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), raytrace_lds_bytes(stackSize, bvh),
                     (hipStream_t)stream, a, box, g);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_gather_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                    unsigned lgtNum, const rtg_hit* hits, size_t n,
                    const rtg_gather_params* params, const rtg_vec* dirs, const float* weights,
                    unsigned nDirs, int stackSize, int semantics, rtg_vec* outHost,
                    unsigned short* skippedHost, int walk, int nthreads) {
  rtg_clear_error();
  int rc = check_gather(hits, params, dirs, weights, nDirs, outHost, stackSize);
  if (!rc) rc = check_semantics("gather", semantics);
  if (!rc) rc = check_walk("gather", walk);
  if (!rc) rc = check_probe_points("gather", n);
  if (!rc) rc = check_scene_arrays("gather", spheres, sphNum, lights, lgtNum);
  if (!rc) rc = check_sphere_count("gather", sphNum);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  PackedScene ps;
  pack_scene(spheres, sphNum, lights, lgtNum, &ps);  // as rtg_context_set_scene
  const bool bvh = walk == 1 && !ps.bvhNodes.empty();
  const RayBox box = bvh ? ray_box(ps.originBox) : RayBox{};
  const HostGatherFn fn = host_trace_fn(
      stackSize, semantics == RTG_SEMANTICS_OPENCL, walk == 1, bvh,
      [](auto s, auto cl, auto wk, auto bv) -> HostGatherFn {
        return gather_host_range<s.value, cl.value, wk.value, bv.value>;
      });
  const GatherArgs g{hits, n, *params, dirs, weights, nDirs, outHost, skippedHost};
  host_bands(n, nthreads, [&](size_t i0, size_t i1) { fn(ps, box, g, i0, i1); });
  return RTG_OK;
}

int rtg_gather(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
               unsigned lgtNum, const rtg_hit* hits, size_t n, const rtg_gather_params* params,
               const rtg_vec* dirs, const float* weights, unsigned nDirs, int stackSize,
               rtg_vec* outHost, unsigned short* skippedHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int rc = check_gather(hits, params, dirs, weights, nDirs, outHost, stackSize);
  if (!rc) rc = check_probe_points("gather", n);
  if (!rc) rc = check_scene_arrays("gather", spheres, sphNum, lights, lgtNum);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  const StageScene scene{spheres, sphNum, lights, lgtNum};
  return one_shot("gather", device, &scene,
                  {{n * sizeof(rtg_hit), hits, nullptr},
                   {(size_t)nDirs * sizeof(rtg_vec), dirs, nullptr},
                   {(size_t)nDirs * sizeof(float), weights, nullptr},
                   {n * sizeof(rtg_vec), nullptr, outHost},
                   {skippedHost ? n * sizeof(unsigned short) : 0, nullptr, skippedHost}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_gather_device(ctx, (const rtg_hit*)d[0], n, params,
                                             (const rtg_vec*)d[1], (const float*)d[2], nDirs,
                                             stackSize, (rtg_vec*)d[3], (unsigned short*)d[4],
                                             nullptr);
                  });
}

}  // extern "C"
