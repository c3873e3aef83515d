// rtg_raytrace_kernels.h — the batch ray tracer's kernel (rtg_raytrace*,
// rtg.h) as a template over the stack capacity S, instantiated next to the
// render kernels in rtg_trace_s<S>.hip (raytrace_fn<S>); the launcher, the
// host forms and the exactness argument are in rtg_raytrace.hip.
#pragma once

#include "rtg_rays.h"
#include "rtg_trace_kernels.h"

namespace rtg {

// The kernel's LDS image, one wave: the lanes' frame colours as in the render
// kernels (frame_lds_levels), then the wave's 64-entry BVH traversal stack.
constexpr size_t raytrace_lds_bytes(int S, bool bvh) {
  return (size_t)frame_lds_levels(S, bvh) * 64 * 16 + (bvh ? 64 * sizeof(int) : 0);
}

// The scene of a ray-trace kernel (raytrace_kernel, camera_kernel): one wave,
// the LDS image above (`lds4`, the workgroup's dynamic LDS) and the context's
// tables.
template <int S, bool kBvh>
__device__ __forceinline__ void bind_raytrace_scene(RayScene<kBvh>& sc, const SceneTables& a,
                                                    float4* lds4) {
  constexpr int NFL = frame_lds_levels(S, kBvh);
  sc.lfr = reinterpret_cast<FrameC*>(lds4) + threadIdx.x;
  sc.nfl = NFL;
  bind_scene(sc, a, reinterpret_cast<int*>(lds4 + NFL * 64));  // the stack: kBvh only
}

// A colour into the caller's array, NaN as the frame's NaNs; `dst` is 12 B the
// lane owns.
__device__ __forceinline__ void store_colour_dev(rtg_vec* dst, V3 c) {
  float* w = reinterpret_cast<float*>(dst);
  w[0] = canon_nan(c.x);
  w[1] = canon_nan(c.y);
  w[2] = canon_nan(c.z);
}

// One lane per ray, one-wave workgroups; n > 0.  Lanes past n trace nothing
// and store nothing (the queries' wave-level tests are over the lanes in
// them).  dst[k] = rayTrace(ray k) before main.cpp:442-445 scales it.  With an
// index list (`order` not null, the _indexed launch: a kernel argument, so the
// select is wave-uniform) lane k works on ray order[k] instead; a lane whose
// entry is not an index of the batch (>= n, never dereferenced) leaves like a
// lane past n.
template <int S, bool kBvh, bool kCL>
__global__ __launch_bounds__(64) void raytrace_kernel(const SceneTables a, const RayBox box,
                                                      const rtg_ray* __restrict__ rays,
                                                      const unsigned* __restrict__ order,
                                                      size_t n, rtg_vec* __restrict__ dst) {
  extern __shared__ float4 lds4[];
  RayScene<kBvh> sc;
  bind_raytrace_scene<S>(sc, a, lds4);
  size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  if (order) {
    k = order[k];  // k < n: inside the index list
    if (k >= n) return;
  }
  const float* r = reinterpret_cast<const float*>(rays + k);  // k < n: 24 B of the batch
  const V3 o = v3(r[0], r[1], r[2]);
  const V3 d = v3(r[3], r[4], r[5]);
  store_colour_dev(dst + k, trace_ray<S, kCL, kBvh>(sc, box, o, d));  // k < n: 12 B of dst
}

// bvh: the scene has a BVH (SceneTables::bvhNodes); cl: RTG_SEMANTICS_OPENCL.
template <int S>
static RayTraceFn raytrace_fn(bool bvh, bool cl) {
  if (bvh) return cl ? raytrace_kernel<S, true, true> : raytrace_kernel<S, true, false>;
  return cl ? raytrace_kernel<S, false, true> : raytrace_kernel<S, false, false>;
}

}  // namespace rtg
