// rtg_camera_kernels.h — the posed camera's fused render kernel
// (rtg_render_camera*, rtg.h) as a template over the stack capacity S,
// instantiated next to the render kernels and raytrace_kernel in
// rtg_trace_s<S>.hip (camera_fn<S>); the launcher, the generator kernel
// (camera_rays_kernel: not a template, so it is defined once, in the launcher's
// translation unit) and the host forms are in rtg_camera.hip.
#pragma once

#include "rtg_camera.h"
#include "rtg_raytrace_kernels.h"

namespace rtg {

// A wave's pixels: a kCamTileW x kCamTileH tile of the frame, lane l at
// (l % kCamTileW, l / kCamTileW) of it.  An 8 x 8 tile keeps a wave's rays
// closer together in the BVH walk than 64 pixels of a row: measured against
// the 64 x 1 mapping at 3840 x 2160, 0.485 against 0.543 ms on C3 and 61.8
// against 93.7 ms on C5 at aa = 1.
constexpr unsigned kCamTileW = 8, kCamTileH = 8;
static_assert(kCamTileW * kCamTileH == 64, "one lane per pixel of the tile");

// One lane per pixel, one-wave workgroups, workgroup b the tile (b % tilesX,
// b / tilesX); the LDS image and the scene binding are raytrace_kernel's.  A
// lane whose pixel lies outside the frame leaves before the trace (the
// queries' wave-level tests are over the lanes present).  The others trace
// the pixel's samples in the reference's order, each sample rayTrace of the
// pose's ray as raytrace_kernel runs it, and fold them as shade_pixel does:
// pix += (1/nS) * c.
template <int S, bool kBvh, bool kCL>
__global__ __launch_bounds__(64) void camera_kernel(const SceneTables a, const RayBox box,
                                                    const Camera cam, const CamPose pose,
                                                    unsigned W, unsigned H, unsigned tilesX,
                                                    rtg_vec* __restrict__ dst) {
  extern __shared__ float4 lds4[];
  RayScene<kBvh> sc;
  bind_raytrace_scene<S>(sc, a, lds4);
  const size_t px = (size_t)(blockIdx.x % tilesX) * kCamTileW + threadIdx.x % kCamTileW;
  const size_t py = (size_t)(blockIdx.x / tilesX) * kCamTileH + threadIdx.x / kCamTileW;
  if (px >= W || py >= H) return;
  const unsigned x = (unsigned)px, y = (unsigned)py;
  V3 pix = v3(0.f, 0.f, 0.f);
  for (int i = 0; i < cam.nAA; ++i) {
    for (int j = 0; j < cam.nAA; ++j) {
      const V3 d = camera_dir(cam, pose, x, y, i, j);
      V3 c = trace_ray<S, kCL, kBvh>(sc, box, pose.eye, d);
      c = vsmul(cam.inv, c);
      pix = vadd(pix, c);
    }
  }
  store_colour_dev(dst + (py * W + px), pix);  // px < W, py < H: 12 B of the frame
}

// bvh: the scene has a BVH (SceneTables::bvhNodes); cl: RTG_SEMANTICS_OPENCL.
template <int S>
static CameraFn camera_fn(bool bvh, bool cl) {
  if (bvh) return cl ? camera_kernel<S, true, true> : camera_kernel<S, true, false>;
  return cl ? camera_kernel<S, false, true> : camera_kernel<S, false, false>;
}

}  // namespace rtg
