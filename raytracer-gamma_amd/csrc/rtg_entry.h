// rtg_entry.h — what the C ABI entry points of librtg.so share (rtg_kernel.hip,
// rtg_gbuffer.hip, rtg_rays.hip, rtg_raytrace.hip, rtg_order.hip, rtg_camera.hip): the HIP error
// return, the records' NaN form
// and 32-byte store, the host forms' plain scene and thread bands, and the
// one-shot body.  HIP translation units only.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <string.h>

#include <functional>
#include <thread>
#include <vector>

#include "rtg.h"
#include "rtg_internal.h"
#include "rtg_trace.h"

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      rtg_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                     \
      return RTG_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

namespace rtg {

// A record's float as its bits, NaN as the frame's NaNs (rtg.h).
RTG_HD unsigned nan_bits(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  return (v != v) ? 0xFFC00000u : u;
}

// A 32-byte record (rtg_gbuf_px, rtg_hit) as two 16-byte stores; `rec` is
// 16-byte aligned (the device entry points check their destination).
__device__ __forceinline__ void store_record(void* rec, const unsigned* w) {
  uint4* o = reinterpret_cast<uint4*>(rec);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// The caller's sphere array as a Scene of the plain loops (closest_hit /
// blocked): r*r as raySphere forms it (raytracer.h:100).
struct HostSpheres {
  const rtg_sphere* s;
  unsigned n;
  V3 sphere(unsigned i, float& r2) const {
    r2 = s[i].radius * s[i].radius;
    return v3(s[i].pos.x, s[i].pos.y, s[i].pos.z);
  }
};

// Contiguous bands of [0, n) on nthreads threads.
inline void host_bands(size_t n, int nthreads, const std::function<void(size_t, size_t)>& fn) {
  size_t nt = nthreads > 0 ? (size_t)nthreads : 1;
  if (nt > n) nt = n;
  if (nt <= 1) {
    fn(0, n);
    return;
  }
  std::vector<std::thread> pool;
  for (size_t k = 0; k < nt; ++k) pool.emplace_back(fn, n * k / nt, n * (k + 1) / nt);
  for (auto& th : pool) th.join();
}

// One-shot body (rtg_kernel.hip): a context on `device` with the scene,
// `inBytes` of input up (none: dIn is null), `launch` on the context,
// `outBytes` down, everything freed.  The caller has checked its arguments.
int one_shot(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
             unsigned lgtNum, const void* in, size_t inBytes, void* out, size_t outBytes,
             const std::function<int(rtg_context* ctx, const void* dIn, void* dOut)>& launch);

}  // namespace rtg

// rtg_kernel.hip: a context's device, with or without a scene (the posed
// camera's ray generator needs no scene); false when the context is null.
bool rtg_context_device(const rtg_context* ctx, int* device);
