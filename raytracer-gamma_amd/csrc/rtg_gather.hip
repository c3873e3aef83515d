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
// gather_rays_kernel: one lane per ray, 24 B out; it needs no scene.
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

#include <vector>

#include "rtg.h"
#include "rtg_ao.h"
#include "rtg_entry.h"
#include "rtg_gather_kernels.h"
#include "rtg_host_scene.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"

static_assert(sizeof(rtg_gather_params) == 16, "rtg_gather_params is 16 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");
static_assert(sizeof(rtg_ray) == 24 && sizeof(rtg_vec) == 12, "24 B per ray, 12 B per colour");
static_assert(RTG_GATHER_MAX_SAMPLES <= 0xFFFF, "a skip count fits an unsigned short");

namespace rtg {

// Ray k of point i as six words; a record without a point: zeros.
RTG_HD void gather_ray(const rtg_hit* hits, size_t i, unsigned k, const rtg_gather_params& p,
                       const rtg_vec* dirs, unsigned nDirs, unsigned* w) {
  const AoPoint pt = ao_point(hits + i, p.bias);
  V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 0.f);
  if (pt.id >= 0) {
    o = pt.a;
    d = gather_dir(pt, ao_dir(dirs, ao_dir_index(ao_window(p.flags, p.seed, i, nDirs), k, nDirs)));
  }
  w[0] = nan_bits(o.x); w[1] = nan_bits(o.y); w[2] = nan_bits(o.z);
  w[3] = nan_bits(d.x); w[4] = nan_bits(d.y); w[5] = nan_bits(d.z);
}

// One lane per ray; total = n * K > 0.
__global__ __launch_bounds__(64) void gather_rays_kernel(const rtg_hit* __restrict__ hits,
                                                         size_t total, const rtg_gather_params p,
                                                         const rtg_vec* __restrict__ dirs,
                                                         unsigned nDirs,
                                                         rtg_ray* __restrict__ rays) {
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= total) return;
  unsigned w[6];
  gather_ray(hits, k / p.samples, (unsigned)(k % p.samples), p, dirs, nDirs, w);  // k / K < n
  unsigned* o = reinterpret_cast<unsigned*>(rays + k);  // k < total: 24 B of the batch
  for (int q = 0; q < 6; ++q) o[q] = w[q];
}

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

// The checks every form shares, in the order they are reported in; the
// generator has no weights and no stack (`fused` false).
static int check_gather(const char* what, const void* hits, const rtg_gather_params* p,
                        const void* dirs, bool fused, const void* weights, unsigned nDirs,
                        const void* out, int stackSize) {
  if (!hits || !p || !dirs || (fused && !weights) || !out) {
    rtg_set_error("%s: null %s", what,
                  !hits ? "hit buffer" : !p ? "params" : !dirs ? "direction table"
                  : (fused && !weights) ? "weight table" : "output buffer");
    return RTG_ERR_INVALID;
  }
  if (p->samples < 1 || p->samples > RTG_GATHER_MAX_SAMPLES) {
    rtg_set_error("%s: %u samples outside [1, %d]", what, p->samples, RTG_GATHER_MAX_SAMPLES);
    return RTG_ERR_INVALID;
  }
  if (nDirs < p->samples || nDirs > RTG_GATHER_MAX_DIRS) {
    rtg_set_error("%s: %u directions outside [samples = %u, %d]", what, nDirs, p->samples,
                  RTG_GATHER_MAX_DIRS);
    return RTG_ERR_INVALID;
  }
  const unsigned known = RTG_GATHER_JITTER | RTG_GATHER_SKIP_NONFINITE;
  if (p->flags & ~known) {
    rtg_set_error("%s: unknown flags 0x%x", what, p->flags & ~known);
    return RTG_ERR_INVALID;
  }
  return fused ? check_stack(what, stackSize) : RTG_OK;
}

// n as the window hash takes it.
static int check_gather_points(const char* what, size_t n) {
  if (n <= 0xFFFFFFFFull) return RTG_OK;
  rtg_set_error("%s: %zu points (at most 2^32 - 1)", what, n);
  return RTG_ERR_INVALID;
}

// The rays' n * K (reported before the point count: every n whose product
// overflows is above 2^32 - 1 too).
static int check_gather_product(const char* what, size_t n, unsigned K) {
  if (n <= SIZE_MAX / K) return check_gather_points(what, n);
  rtg_set_error("%s: %zu points x %u samples overflows size_t", what, n, K);
  return RTG_ERR_INVALID;
}

extern "C" {

int rtg_gather_rays_host(const rtg_hit* hits, size_t n, const rtg_gather_params* params,
                         const rtg_vec* dirs, unsigned nDirs, rtg_ray* raysHost, int nthreads) {
  rtg_clear_error();
  int rc = check_gather("gather_rays", hits, params, dirs, false, nullptr, nDirs, raysHost, 0);
  if (!rc) rc = check_gather_product("gather_rays", n, params->samples);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  const rtg_gather_params p = *params;
  host_bands(n, nthreads, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
      for (unsigned k = 0; k < p.samples; ++k) {
        unsigned w[6];
        gather_ray(hits, i, k, p, dirs, nDirs, w);
        memcpy(raysHost + i * p.samples + k, w, sizeof w);
      }
    }
  });
  return RTG_OK;
}

int rtg_gather_rays_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                           const rtg_gather_params* params, const rtg_vec* dirsDevice,
                           unsigned nDirs, rtg_ray* raysDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("gather_rays: no context");
    return RTG_ERR_INVALID;
  }
  int rc = check_gather("gather_rays", hitsDevice, params, dirsDevice, false, nullptr, nDirs,
                        raysDevice, 0);
  if (!rc) rc = check_gather_product("gather_rays", n, params->samples);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  const size_t total = n * params->samples;
  unsigned blocks;
  rc = ray_blocks("gather_rays", "batch", total, &blocks);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(gather_rays_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream,
                     hitsDevice, total, *params, dirsDevice, nDirs, raysDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
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
  int rc = check_gather("gather", hitsDevice, params, dirsDevice, true, weightsDevice, nDirs,
                        outDevice, stackSize);
  if (!rc) rc = check_gather_points("gather", n);
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
  int rc = check_gather("gather", hits, params, dirs, true, weights, nDirs, outHost, stackSize);
  if (!rc) rc = check_semantics("gather", semantics);
  if (!rc) rc = check_walk("gather", walk);
  if (!rc) rc = check_gather_points("gather", n);
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
  int rc = check_gather("gather", hits, params, dirs, true, weights, nDirs, outHost, stackSize);
  if (!rc) rc = check_gather_points("gather", n);
  if (!rc) rc = check_scene_arrays("gather", spheres, sphNum, lights, lgtNum);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  // one upload: the hit records, then the two tables; one download: the sums,
  // then the counts
  const size_t hitBytes = n * sizeof(rtg_hit), dirBytes = (size_t)nDirs * sizeof(rtg_vec),
               wBytes = (size_t)nDirs * sizeof(float), outBytes = n * sizeof(rtg_vec),
               skipBytes = skippedHost ? n * sizeof(unsigned short) : 0;
  std::vector<unsigned char> in(hitBytes + dirBytes + wBytes), back(outBytes + skipBytes);
  memcpy(in.data(), hits, hitBytes);
  memcpy(in.data() + hitBytes, dirs, dirBytes);
  memcpy(in.data() + hitBytes + dirBytes, weights, wBytes);
  rc = one_shot(device, spheres, sphNum, lights, lgtNum, in.data(), in.size(), back.data(),
                back.size(), [&](rtg_context* ctx, const void* dIn, void* out) {
                  const unsigned char* d = (const unsigned char*)dIn;
                  unsigned char* o = (unsigned char*)out;
                  return rtg_gather_device(
                      ctx, (const rtg_hit*)d, n, params, (const rtg_vec*)(d + hitBytes),
                      (const float*)(d + hitBytes + dirBytes), nDirs, stackSize, (rtg_vec*)o,
                      skippedHost ? (unsigned short*)(o + outBytes) : nullptr, nullptr);
                });
  if (rc) return rc;
  memcpy(outHost, back.data(), outBytes);
  if (skipBytes) memcpy(skippedHost, back.data() + outBytes, skipBytes);
  return RTG_OK;
}

}  // extern "C"
