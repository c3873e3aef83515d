// rtg_camera_kernels.h — the posed camera's fused render kernels
// (rtg_render_camera*: one pose; rtg_render_views*: a table of poses; rtg.h)
// as templates over the stack capacity S, instantiated next to the render
// kernels and raytrace_kernel in rtg_trace_s<S>.hip (camera_fn<S>,
// views_fn<S>); the launchers, the generator kernel
// (camera_rays_kernel: not a template, so it is defined once, in the launcher's
// translation unit) and the host forms are in rtg_camera.hip.
#pragma once

#include "rtg_camera.h"
#include "rtg_fold.h"
#include "rtg_raytrace_kernels.h"

namespace rtg {

// A wave's pixels: a kCamTileW x kCamTileH tile of the frame, lane l at
// (l % kCamTileW, l / kCamTileW) of it.  An 8 x 8 tile keeps a wave's rays
// closer together in the BVH walk than 64 pixels of a row: measured against
// the 64 x 1 mapping at 3840 x 2160, 0.485 against 0.543 ms on C3 and 61.8
// against 93.7 ms on C5 at aa = 1.
constexpr unsigned kCamTileW = 8, kCamTileH = 8;
static_assert(kCamTileW * kCamTileH == 64, "one lane per pixel of the tile");
static_assert(kCamTileW == kFoldTileW && kCamTileH == kFoldTileH, "rtg.h's fold is over these tiles");

// One wave's tile of one W x H frame: tile `tile` is (tile % tilesX,
// tile / tilesX), `dst` the frame's first pixel.  The LDS image and the scene
// binding are raytrace_kernel's.  A lane whose pixel lies outside the frame
// leaves before the trace (the queries' wave-level tests are over the lanes
// present), so a ragged tile never writes past its own frame's rows.  The
// others trace the pixel's samples in the
// reference's order, each sample rayTrace of the pose's ray as raytrace_kernel
// runs it, and fold them as shade_pixel does: pix += (1/nS) * c.
template <int S, bool kBvh, bool kCL>
__device__ __forceinline__ void camera_tile(const SceneTables& a, const RayBox& box,
                                            const Camera& cam, const CamPose& pose, unsigned W,
                                            unsigned H, unsigned tilesX, unsigned tile,
                                            rtg_vec* __restrict__ dst) {
  extern __shared__ float4 lds4[];
  RayScene<kBvh> sc;
  bind_raytrace_scene<S>(sc, a, lds4);
  const size_t px = (size_t)(tile % tilesX) * kCamTileW + threadIdx.x % kCamTileW;
  const size_t py = (size_t)(tile / tilesX) * kCamTileH + threadIdx.x / kCamTileW;
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

// One pose, one frame: one lane per pixel, one-wave workgroups, workgroup b
// the tile b, the pose by value in the kernel arguments.
template <int S, bool kBvh, bool kCL>
__global__ __launch_bounds__(64) void camera_kernel(const SceneTables a, const RayBox box,
                                                    const Camera cam, const CamPose pose,
                                                    unsigned W, unsigned H, unsigned tilesX,
                                                    rtg_vec* __restrict__ dst) {
  camera_tile<S, kBvh, kCL>(a, box, cam, pose, W, H, tilesX, blockIdx.x, dst);
}

// Many poses, one frame each (rtg_render_views*), view-major: workgroup b is
// tile b % tilesPerView of view b / tilesPerView, and the grid is exactly
// nViews * tilesPerView workgroups, so the view is one of the table's.  A
// view's tiles are neighbours in dispatch order: waves resident together walk
// the same part of the BVH.  The view index comes from blockIdx.x alone, so
// the pose's 48 B are read through a wave-uniform address: scalar loads into
// SGPRs, not 64 lanes' vector loads.  The table is only
// read, and it is complete before the launch (a kernel boundary), which is
// what the scalar cache needs.
template <int S, bool kBvh, bool kCL>
__global__ __launch_bounds__(64) void views_kernel(const SceneTables a, const RayBox box,
                                                   const Camera cam,
                                                   const CamPose* __restrict__ poses, unsigned W,
                                                   unsigned H, unsigned tilesX,
                                                   unsigned tilesPerView,
                                                   rtg_vec* __restrict__ dst) {
  const unsigned view = blockIdx.x / tilesPerView;
  const unsigned tile = blockIdx.x - view * tilesPerView;
  const CamPose pose = poses[view];  // view < nViews: 48 B of the table
  camera_tile<S, kBvh, kCL>(a, box, cam, pose, W, H, tilesX, tile,
                            dst + (size_t)view * W * H);
}

// Many poses folded into per-group coefficients (rtg_render_views_fold*): the
// grid, the pose read and the trace are views_kernel's, and no frame is
// written.  camera_tile lets a lane outside the frame LEAVE before the trace;
// here such a lane only steps round it (the queries' wave-level tests are
// still over the lanes present, so a traced pixel is camera_tile's bit for
// bit) and comes back holding +0.f, because the epilogue's tree sum
// (fold_tile, rtg_fold.h) reads all 64 lanes.  The pixel is folded as
// store_colour_dev would have stored it.
template <int S, bool kBvh, bool kCL>
__global__ __launch_bounds__(64) void views_fold_kernel(const SceneTables a, const RayBox box,
                                                        const Camera cam,
                                                        const CamPose* __restrict__ poses,
                                                        unsigned W, unsigned H, unsigned tilesX,
                                                        unsigned tilesPerView, const FoldArgs fa) {
  const unsigned view = blockIdx.x / tilesPerView;
  const unsigned tile = blockIdx.x - view * tilesPerView;
  const CamPose pose = poses[view];  // view < nViews: 48 B of the table
  extern __shared__ float4 lds4[];
  RayScene<kBvh> sc;
  bind_raytrace_scene<S>(sc, a, lds4);
  const size_t px = (size_t)(tile % tilesX) * kCamTileW + threadIdx.x % kCamTileW;
  const size_t py = (size_t)(tile / tilesX) * kCamTileH + threadIdx.x / kCamTileW;
  const bool live = px < W && py < H;
  V3 pix = v3(0.f, 0.f, 0.f);
  if (live) {
    const unsigned x = (unsigned)px, y = (unsigned)py;
    for (int i = 0; i < cam.nAA; ++i) {
      for (int j = 0; j < cam.nAA; ++j) {
        const V3 d = camera_dir(cam, pose, x, y, i, j);
        V3 c = trace_ray<S, kCL, kBvh>(sc, box, pose.eye, d);
        c = vsmul(cam.inv, c);
        pix = vadd(pix, c);
      }
    }
  }
  // the lane's texel in its group's table: K consecutive floats, read when live
  const float* w = fa.weights + (((size_t)(view % fa.G) * H + py) * W + px) * fa.K;
  fold_tile(live, canon_nan(pix.x), canon_nan(pix.y), canon_nan(pix.z), w, fa.K, fa.skip != 0,
            fa.partials + (size_t)blockIdx.x * fold_tile_words(fa.K));
}

// bvh: the scene has a BVH (SceneTables::bvhNodes); cl: RTG_SEMANTICS_OPENCL.
template <int S>
static CameraFn camera_fn(bool bvh, bool cl) {
  if (bvh) return cl ? camera_kernel<S, true, true> : camera_kernel<S, true, false>;
  return cl ? camera_kernel<S, false, true> : camera_kernel<S, false, false>;
}
template <int S>
static ViewsFn views_fn(bool bvh, bool cl) {
  if (bvh) return cl ? views_kernel<S, true, true> : views_kernel<S, true, false>;
  return cl ? views_kernel<S, false, true> : views_kernel<S, false, false>;
}
template <int S>
static ViewsFoldFn views_fold_fn(bool bvh, bool cl) {
  if (bvh) return cl ? views_fold_kernel<S, true, true> : views_fold_kernel<S, true, false>;
  return cl ? views_fold_kernel<S, false, true> : views_fold_kernel<S, false, false>;
}

}  // namespace rtg
