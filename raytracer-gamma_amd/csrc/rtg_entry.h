// rtg_entry.h — what the C ABI entry points of librtg.so share (every .hip of
// this directory but the rtg_trace_s<S> instantiations): the HIP error
// return, the records' NaN form, the colour and 32-byte record stores, the
// host forms' plain scene and thread bands, the argument checks that differ
// between entry points only in their prefix, and the one-shot body.  HIP
// translation units only.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <string.h>

#include <functional>
#include <initializer_list>
#include <thread>
#include <vector>

#include "rtg.h"
#include "rtg_internal.h"
#include "rtg_stage.h"
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

// A colour of the host forms (rtg_raytrace_host, rtg_render_camera_host).
inline void store_colour(rtg_vec* dst, V3 c) {
  const unsigned w[3] = {nan_bits(c.x), nan_bits(c.y), nan_bits(c.z)};
  memcpy(dst, w, sizeof w);
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

// ---- argument checks ----
// Each sets the entry point's message, "<what>: ...", and returns
// RTG_ERR_INVALID, or returns RTG_OK.  An entry point calls them in the order
// it reports in: the first bad argument is the one named.

inline int check_stack(const char* what, int stackSize) {
  if (stackSize >= 1 && stackSize <= RTG_MAX_STACK) return RTG_OK;
  rtg_set_error("%s: stackSize %d outside [1, %d]", what, stackSize, RTG_MAX_STACK);
  return RTG_ERR_INVALID;
}

inline int check_semantics(const char* what, int semantics) {
  if (semantics == RTG_SEMANTICS_CPU || semantics == RTG_SEMANTICS_OPENCL) return RTG_OK;
  rtg_set_error("%s: semantics %d (0: CPU, 1: OpenCL)", what, semantics);
  return RTG_ERR_INVALID;
}

// The host forms' walk: 0 the plain loops, 1 the kernel's own path.
inline int check_walk(const char* what, int walk) {
  if (walk == 0 || walk == 1) return RTG_OK;
  rtg_set_error("%s: walk %d (0: plain loops, 1: the kernel's query path)", what, walk);
  return RTG_ERR_INVALID;
}

// What pack_scene takes (rtg_context_set_scene has its own message).
inline int check_sphere_count(const char* what, unsigned sphNum) {
  if (sphNum < RTG_MAX_SPHERES) return RTG_OK;
  rtg_set_error("%s: %u spheres (at most %u)", what, sphNum, RTG_MAX_SPHERES - 1);
  return RTG_ERR_INVALID;
}

// The caller's scene arrays; an entry point without lights passes none.
inline int check_scene_arrays(const char* what, const rtg_sphere* spheres, unsigned sphNum,
                              const rtg_light* lights = nullptr, unsigned lgtNum = 0) {
  if (!(sphNum && !spheres) && !(lgtNum && !lights)) return RTG_OK;
  rtg_set_error("%s: null scene array", what);
  return RTG_ERR_INVALID;
}

// The grid of n > 0 lanes in one-wave workgroups; `noun`: what the caller
// calls the n ("batch", "frame").
inline int ray_blocks(const char* what, const char* noun, size_t n, unsigned* blocks) {
  const size_t b = (n + 63) / 64;
  if (b > 0x7FFFFFFFu) {
    rtg_set_error("%s: %s too large (%zu workgroups)", what, noun, b);
    return RTG_ERR_INVALID;
  }
  *blocks = (unsigned)b;
  return RTG_OK;
}

// ---- one-shot body (rtg_kernel.hip) ----

// The scene of a one-shot call; the calls without one pass none.
struct StageScene {
  const rtg_sphere* spheres;
  unsigned sphNum;
  const rtg_light* lights;
  unsigned lgtNum;
};

// One array of a one-shot call on the device: uploaded from `from` before the
// launch, downloaded to `to` after it, device scratch with neither.  A part
// of 0 bytes has a null device pointer and no copy.
struct StagePart {
  size_t bytes;
  const void* from;
  void* to;
};

// A context on `device`, with the scene if there is one; the parts in one
// allocation (rtg_stage.h has the layout), the uploads, `launch` on the
// context with part i's device pointer in d[i], the downloads, everything
// freed.  The caller has checked its arguments; `what` prefixes the failures.
int one_shot(const char* what, int device, const StageScene* scene,
             std::initializer_list<StagePart> parts,
             const std::function<int(rtg_context* ctx, void* const* d)>& launch);

// One array up (none: dIn is null), one down.
inline int one_shot(
    const char* what, int device, const StageScene& scene, const void* in, size_t inBytes,
    void* out, size_t outBytes,
    const std::function<int(rtg_context* ctx, const void* dIn, void* dOut)>& launch) {
  return one_shot(what, device, &scene, {{inBytes, in, nullptr}, {outBytes, nullptr, out}},
                  [&](rtg_context* ctx, void* const* d) { return launch(ctx, d[0], d[1]); });
}

}  // namespace rtg

// rtg_kernel.hip: a context's device, with or without a scene (the posed
// camera's ray generator needs no scene); false when the context is null.
bool rtg_context_device(const rtg_context* ctx, int* device);
