// rtg_camera.hip — the posed camera of librtg.so (rtg_camera*, rtg_render_camera*,
// rtg.h): a frame, or the sample rays of a frame, from any viewpoint.
//
// The reference keeps its camera at 0 looking down -z (main.cpp:384-436), and
// so do the renders.  A pose {eye, right, up, back} moves it: the sample's
// screen-plane point (rx, ry) is sample_dir's, and its ray is
//   origin = eye,  dir = vnorm((rx * right + ry * up) + zoom * back)
// per component in float with no contraction (camera_dir, rtg_camera.h: one
// function for every form below).  The identity pose gives the render's ray
// bit for bit.
//
// The fused render (camera_kernel, rtg_camera_kernels.h, per S in
// rtg_trace_s.hip) forms each sample ray in registers, runs rayTrace on it as
// rtg_raytrace_device does (trace_ray, rtg_rays.h: exact for any origin at
// every level of the tree; none of the renders' table paths, for the reasons
// there and at the head of rtg_raytrace.hip) and folds the pixel as
// shade_pixel does.  The posed frame is therefore, bit for
// bit, the host fold of rtg_raytrace_host(walk 0) over rtg_camera_rays_host's
// rays: no ray buffer, no colour buffer and no fold on the caller's side.
//
// Many views in one launch (rtg_render_views*, views_kernel next to
// camera_kernel): a table of poses in device memory, one frame each, the
// workgroups spanning the views; the per-tile body is camera_kernel's, so view
// v is bit for bit the single-view frame of pose v.  rtg_camera_cube writes
// the six poses of a cube map.
//
// Many views folded into per-group coefficients (rtg_render_views_fold*,
// views_fold_kernel): the same launch with rtg_fold.h's tile epilogue in place
// of the pixel store, then rtg_fold.hip's stage 2; no frame is written.
// rtg_cube_sh_weights builds the SH table for rtg_camera_cube's faces.
//
// The generator's inverse (rtg_camera_project*, camera_project of rtg_camera.h):
// a point's frame position {fx, fy} and k under a pose, one lane per point.
//
// This file holds the pose helpers, the generator (kernel and host form), the
// launchers of the fused kernels (picked from stack_kernels, rtg_trace_kernels.h),
// the pose's own argument checks (the rest are rtg_entry.h's) and the host
// forms of the render (walk 0: trace_ray_plain, the yardstick; walk 1:
// trace_ray, the kernel's own path over the packed tables, one pixel per
// "wave"; host_trace_fn, rtg_host_scene.h, picks the instantiation).
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "rtg.h"
#include "rtg_camera.h"
#include "rtg_camera_kernels.h"
#include "rtg_entry.h"
#include "rtg_fold.h"
#include "rtg_host_scene.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"

static_assert(sizeof(rtg_camera) == 48 && sizeof(rtg::CamPose) == 48, "the pose is 48 B");
static_assert(sizeof(rtg_ray) == 24 && sizeof(rtg_vec) == 12, "24 B per ray, 12 B per pixel");

namespace rtg {

// ---- the generator ----

// Ray k of the frame: pixel k / nS in row-major order, its sample k % nS in
// the reference's order (i outer, j inner).
RTG_HD void camera_ray(const Camera& cam, const CamPose& p, unsigned W, size_t k, float* r) {
  const size_t nS = (size_t)cam.nAA * cam.nAA;
  const size_t px = k / nS;
  const int s = (int)(k % nS);
  const V3 d = camera_dir(cam, p, (unsigned)(px % W), (unsigned)(px / W), s / cam.nAA, s % cam.nAA);
  r[0] = p.eye.x; r[1] = p.eye.y; r[2] = p.eye.z;
  r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

// One lane per sample ray, 24 B out; n > 0 (so cam.nAA > 0).
__global__ __launch_bounds__(64) void camera_rays_kernel(const Camera cam, const CamPose pose,
                                                         unsigned W, size_t n,
                                                         rtg_ray* __restrict__ rays) {
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  camera_ray(cam, pose, W, k, reinterpret_cast<float*>(rays + k));  // k < n: 24 B of the batch
}

// Point k of the batch under the pose: {fx, fy, k} as three words, NaN as the
// records' NaN.
RTG_HD void camera_project_words(const ProjFrame& f, const CamPose& p, const float* pt,
                                 unsigned* w) {
  const V3 r = camera_project(f, p, v3(pt[0], pt[1], pt[2]));
  w[0] = nan_bits(r.x); w[1] = nan_bits(r.y); w[2] = nan_bits(r.z);
}

// One lane per point, 12 B in and out; n > 0.
__global__ __launch_bounds__(64) void camera_project_kernel(const ProjFrame f, const CamPose pose,
                                                            size_t n,
                                                            const float* __restrict__ points,
                                                            unsigned* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  unsigned w[3];
  camera_project_words(f, pose, points + 3 * k, w);  // k < n: 12 B of each batch
  out[3 * k] = w[0]; out[3 * k + 1] = w[1]; out[3 * k + 2] = w[2];
}

// ---- host forms of the render ----

// Pixels [k0, k1) of the frame; kWalk 1: the kernel's path, else plain loops.
template <int S, bool kCL, bool kWalk, bool kBvh>
static void camera_host_range(const PackedScene& ps, const RayBox& box, const Camera& cam,
                              const CamPose& pose, unsigned W, size_t k0, size_t k1,
                              rtg_vec* dst) {
  const HostScene<kBvh> sc(ps, kWalk);  // walk 0: no masks, no BVH, no lists
  for (size_t k = k0; k < k1; ++k) {
    const unsigned x = (unsigned)(k % W), y = (unsigned)(k / W);
    V3 pix = v3(0.f, 0.f, 0.f);
    for (int i = 0; i < cam.nAA; ++i) {
      for (int j = 0; j < cam.nAA; ++j) {
        const V3 d = camera_dir(cam, pose, x, y, i, j);
        V3 c;
        if constexpr (kWalk) c = trace_ray<S, kCL, kBvh>(sc, box, pose.eye, d);
        else c = trace_ray_plain<S, kCL>(sc, pose.eye, d);
        c = vsmul(cam.inv, c);
        pix = vadd(pix, c);
      }
    }
    store_colour(dst + k, pix);
  }
}

typedef void (*CamHostFn)(const PackedScene&, const RayBox&, const Camera&, const CamPose&,
                          unsigned, size_t, size_t, rtg_vec*);

static V3 vcross(V3 a, V3 b) {
  return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

}  // namespace rtg

using namespace rtg;

// The frame's camera constants, or RTG_ERR_INVALID for a null pointer or with
// make_camera's message (an empty frame, an aliasFactor out of range).
static int check_frame(const char* what, const rtg_camera* cam, const void* dst, unsigned W,
                       unsigned H, float zoom, float aa, Camera* out) {
  if (!cam || !dst) {
    rtg_set_error("%s: null %s", what, cam ? "destination" : "camera");
    return RTG_ERR_INVALID;
  }
  return make_camera(W, H, zoom, aa, out);
}

// rtg_camera_project*'s arguments, in the order they are reported in.
static int check_project(const rtg_camera* cam, unsigned W, unsigned H, const void* points,
                         size_t n, const void* dst) {
  if (!cam || (n && (!points || !dst))) {
    rtg_set_error("camera_project: null %s", !cam ? "camera" : !points ? "points" : "destination");
    return RTG_ERR_INVALID;
  }
  if (W == 0 || H == 0) {
    rtg_set_error("camera_project: empty frame %ux%u", W, H);
    return RTG_ERR_INVALID;
  }
  if (W > (1u << 24) || H > (1u << 24)) {
    rtg_set_error("camera_project: frame %ux%u (at most 2^24 each way)", W, H);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// Workgroups of the fused kernel for a W x H frame; 0 when more than 2^31-1.
static size_t camera_blocks(unsigned W, unsigned H, unsigned* tilesX) {
  const size_t tx = ((size_t)W + kCamTileW - 1) / kCamTileW;
  const size_t ty = ((size_t)H + kCamTileH - 1) / kCamTileH;
  *tilesX = (unsigned)tx;
  return (ty && tx > 0x7FFFFFFFu / ty) ? 0 : tx * ty;
}

// The same for nViews frames of W x H (views_kernel: nViews * tilesPerView
// workgroups); 0 when more than 2^31-1.  nViews > 0.
static size_t views_blocks(size_t nViews, unsigned W, unsigned H, unsigned* tilesX,
                           unsigned* tilesPerView) {
  const size_t per = camera_blocks(W, H, tilesX);
  *tilesPerView = (unsigned)per;
  return (per && nViews > 0x7FFFFFFFu / per) ? 0 : nViews * per;
}

// What rtg_render_views* check first: the pointers (no views need no pose
// table), then the frame as check_frame does.
static int check_views_frame(const rtg_camera* poses, size_t nViews, const void* dst, unsigned W,
                             unsigned H, float zoom, float aa, Camera* out) {
  if (!dst || (nViews && !poses)) {
    rtg_set_error("render_views: null %s", dst ? "pose table" : "destination");
    return RTG_ERR_INVALID;
  }
  return make_camera(W, H, zoom, aa, out);
}

// The same for rtg_render_views_fold*, whose destination is the coefficients.
static int check_fold_views(const rtg_camera* poses, size_t nViews, const void* out, unsigned W,
                            unsigned H, float zoom, float aa, Camera* cam) {
  if (!out || (nViews && !poses)) {
    rtg_set_error("render_views_fold: null %s", out ? "pose table" : "output");
    return RTG_ERR_INVALID;
  }
  return make_camera(W, H, zoom, aa, cam);
}

// ... and after it (so W * H > 0): the stack size, then the batch's size, its
// workgroups (*blocks; 0 for no views) and its bytes.
static int check_views(size_t nViews, unsigned W, unsigned H, int stackSize, unsigned* tilesX,
                       unsigned* tilesPerView, size_t* blocks) {
  const int rc = check_stack("render_views", stackSize);
  if (rc || nViews == 0) return rc;
  *blocks = views_blocks(nViews, W, H, tilesX, tilesPerView);
  if (!*blocks) {
    rtg_set_error("render_views: batch too large (more than 2^31-1 workgroups)");
    return RTG_ERR_INVALID;
  }
  // W * H < 2^64 always; the views' pixels and their 12 B each may not be
  if (nViews > SIZE_MAX / sizeof(rtg_vec) / ((size_t)W * H)) {
    rtg_set_error("render_views: batch too large (%zu views of %u x %u pixels)", nViews, W, H);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// Face f of rtg_camera_cube: forward F, right R, up U (rtg.h's table; R =
// F x U, so (R, U, -F) is right-handed on all six).
static const signed char kCubeAxes[6][3][3] = {
    {{1, 0, 0}, {0, 0, 1}, {0, 1, 0}},    // +X
    {{-1, 0, 0}, {0, 0, -1}, {0, 1, 0}},  // -X
    {{0, 1, 0}, {-1, 0, 0}, {0, 0, -1}},  // +Y
    {{0, -1, 0}, {-1, 0, 0}, {0, 0, 1}},  // -Y
    {{0, 0, 1}, {-1, 0, 0}, {0, 1, 0}},   // +Z
    {{0, 0, -1}, {1, 0, 0}, {0, 1, 0}},   // -Z
};

extern "C" {

void rtg_camera_identity(rtg_camera* out) {
  if (!out) return;
  const rtg_camera c = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
  *out = c;
}

int rtg_camera_look_at(const rtg_vec* eye, const rtg_vec* target, const rtg_vec* up,
                       rtg_camera* out) {
  rtg_clear_error();
  if (!eye || !target || !up || !out) {
    rtg_set_error("camera_look_at: null pointer");
    return RTG_ERR_INVALID;
  }
  const V3 e = v3(eye->x, eye->y, eye->z);
  const V3 back = vnorm(vsub(e, v3(target->x, target->y, target->z)));
  const V3 right = vnorm(vcross(v3(up->x, up->y, up->z), back));
  const V3 u = vcross(back, right);
  const rtg_camera c = {{e.x, e.y, e.z},
                        {right.x, right.y, right.z},
                        {u.x, u.y, u.z},
                        {back.x, back.y, back.z}};
  *out = c;
  return RTG_OK;
}

int rtg_camera_sample_count(float aliasFactor, unsigned* nAA) {
  rtg_clear_error();
  if (!nAA) {
    rtg_set_error("camera_sample_count: null pointer");
    return RTG_ERR_INVALID;
  }
  Camera cam;
  const int rc = make_camera(1, 1, 0.f, aliasFactor, &cam);  // its range check and its loop
  if (rc) return rc;
  *nAA = (unsigned)cam.nAA;
  return RTG_OK;
}

int rtg_camera_rays_host(const rtg_camera* cam, unsigned width, unsigned height, float zoom,
                         float aliasFactor, rtg_ray* raysHost, int nthreads) {
  rtg_clear_error();
  Camera c;
  const int rc = check_frame("camera_rays", cam, raysHost, width, height, zoom, aliasFactor, &c);
  if (rc) return rc;
  const size_t n = (size_t)width * height * c.nAA * c.nAA;
  if (n == 0) return RTG_OK;
  const CamPose pose = cam_pose(*cam);
  host_bands(n, nthreads, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; ++k) {
      float r[6];
      camera_ray(c, pose, width, k, r);
      memcpy(raysHost + k, r, sizeof r);
    }
  });
  return RTG_OK;
}

int rtg_camera_rays_device(rtg_context* ctx, const rtg_camera* cam, unsigned width,
                           unsigned height, float zoom, float aliasFactor, rtg_ray* raysDevice,
                           void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("camera_rays: no context");
    return RTG_ERR_INVALID;
  }
  Camera c;
  int rc = check_frame("camera_rays", cam, raysDevice, width, height, zoom, aliasFactor, &c);
  if (rc) return rc;
  const size_t n = (size_t)width * height * c.nAA * c.nAA;
  if (n == 0) return RTG_OK;
  unsigned blocks;
  rc = ray_blocks("camera_rays", "frame", n, &blocks);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, c,
                     cam_pose(*cam), width, n, raysDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_camera_project_host(const rtg_camera* cam, unsigned width, unsigned height, float zoom,
                            const rtg_vec* points, size_t n, rtg_vec* outHost, int nthreads) {
  rtg_clear_error();
  const int rc = check_project(cam, width, height, points, n, outHost);
  if (rc || n == 0) return rc;
  const ProjFrame f = proj_frame(width, height, zoom);
  const CamPose pose = cam_pose(*cam);
  host_bands(n, nthreads, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; ++k) {
      unsigned w[3];
      camera_project_words(f, pose, &points[k].x, w);
      memcpy(outHost + k, w, sizeof w);
    }
  });
  return RTG_OK;
}

int rtg_camera_project_device(rtg_context* ctx, const rtg_camera* cam, unsigned width,
                              unsigned height, float zoom, const rtg_vec* pointsDevice, size_t n,
                              rtg_vec* outDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("camera_project: no context");
    return RTG_ERR_INVALID;
  }
  int rc = check_project(cam, width, height, pointsDevice, n, outDevice);
  if (rc || n == 0) return rc;
  unsigned blocks;
  rc = ray_blocks("camera_project", "batch", n, &blocks);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(camera_project_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream,
                     proj_frame(width, height, zoom), cam_pose(*cam), n,
                     reinterpret_cast<const float*>(pointsDevice),
                     reinterpret_cast<unsigned*>(outDevice));
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_camera_project(int device, const rtg_camera* cam, unsigned width, unsigned height,
                       float zoom, const rtg_vec* points, size_t n, rtg_vec* outHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int rc = check_project(cam, width, height, points, n, outHost);
  if (rc || n == 0) return rc;
  const size_t bytes = n * sizeof(rtg_vec);
  return one_shot("camera_project", device, nullptr,
                  {{bytes, points, nullptr}, {bytes, nullptr, outHost}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_camera_project_device(ctx, cam, width, height, zoom,
                                                     (const rtg_vec*)d[0], n, (rtg_vec*)d[1],
                                                     nullptr);
                  });
}

int rtg_render_camera_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                           unsigned lgtNum, const rtg_camera* cam, unsigned width,
                           unsigned height, float zoom, float aliasFactor, int stackSize,
                           int semantics, rtg_vec* dstHost, int walk, int nthreads) {
  rtg_clear_error();
  Camera c;
  int rc = check_frame("render_camera", cam, dstHost, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_stack("render_camera", stackSize);
  if (!rc) rc = check_scene_arrays("render_camera", spheres, sphNum, lights, lgtNum);
  if (!rc) rc = check_semantics("render_camera", semantics);
  if (!rc) rc = check_walk("render_camera", walk);
  if (!rc) rc = check_sphere_count("render_camera", sphNum);
  if (rc) return rc;
  PackedScene ps;
  pack_scene(spheres, sphNum, lights, lgtNum, &ps);  // as rtg_context_set_scene
  const bool bvh = walk == 1 && !ps.bvhNodes.empty();
  const RayBox box = bvh ? ray_box(ps.originBox) : RayBox{};
  const CamHostFn fn = host_trace_fn(
      stackSize, semantics == RTG_SEMANTICS_OPENCL, walk == 1, bvh,
      [](auto s, auto cl, auto wk, auto bv) -> CamHostFn {
        return camera_host_range<s.value, cl.value, wk.value, bv.value>;
      });
  const CamPose pose = cam_pose(*cam);
  host_bands((size_t)width * height, nthreads,
             [&](size_t k0, size_t k1) { fn(ps, box, c, pose, width, k0, k1, dstHost); });
  return RTG_OK;
}

int rtg_render_camera_device(rtg_context* ctx, const rtg_camera* cam, unsigned width,
                             unsigned height, float zoom, float aliasFactor, int stackSize,
                             rtg_vec* dstDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0, semantics = RTG_SEMANTICS_CPU;
  if (!rtg_context_scene(ctx, &a, &device, &box, &semantics)) {
    rtg_set_error("render_camera: no context/scene");
    return RTG_ERR_INVALID;
  }
  Camera c;
  int rc = check_frame("render_camera", cam, dstDevice, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_stack("render_camera", stackSize);
  if (rc) return rc;
  unsigned tilesX = 0;
  const size_t blocks = camera_blocks(width, height, &tilesX);
  if (!blocks) {
    rtg_set_error("render_camera: frame too large (more than 2^31-1 workgroups)");
    return RTG_ERR_INVALID;
  }
  const bool bvh = a.bvhNodes != nullptr;
  const StackKernels* sk = stack_kernels(stackSize);
  const CameraFn fn = sk ? sk->camera(bvh, semantics == RTG_SEMANTICS_OPENCL) : nullptr;
  if (!fn) {  // a missing kernel is an error, never another path
    rtg_set_error("render_camera: no kernel for stackSize %d", stackSize);
    return RTG_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64), raytrace_lds_bytes(stackSize, bvh),
                     (hipStream_t)stream, a, box, c, cam_pose(*cam), width, height, tilesX,
                     dstDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_render_camera(int device, const rtg_sphere* spheres, unsigned sphNum,
                      const rtg_light* lights, unsigned lgtNum, const rtg_camera* cam,
                      unsigned width, unsigned height, float zoom, float aliasFactor,
                      int stackSize, rtg_vec* dstHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  Camera c;
  int rc = check_frame("render_camera", cam, dstHost, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_stack("render_camera", stackSize);
  if (!rc) rc = check_scene_arrays("render_camera", spheres, sphNum, lights, lgtNum);
  if (rc) return rc;
  unsigned tilesX = 0;
  if (!camera_blocks(width, height, &tilesX)) {
    rtg_set_error("render_camera: frame too large (more than 2^31-1 workgroups)");
    return RTG_ERR_INVALID;
  }
  return one_shot("render_camera", device, {spheres, sphNum, lights, lgtNum}, nullptr, 0, dstHost,
                  (size_t)width * height * sizeof(rtg_vec),
                  [&](rtg_context* ctx, const void*, void* out) {
                    return rtg_render_camera_device(ctx, cam, width, height, zoom, aliasFactor,
                                                    stackSize, (rtg_vec*)out, nullptr);
                  });
}

// ---- many views in one launch ----

int rtg_camera_cube(const rtg_vec* eye, rtg_camera out[6]) {
  rtg_clear_error();
  if (!eye || !out) {
    rtg_set_error("camera_cube: null pointer");
    return RTG_ERR_INVALID;
  }
  const float rs = 3.f / 32.f, us = (float)(1.0 / 6.0);
  for (int f = 0; f < 6; ++f) {
    const signed char(*t)[3] = kCubeAxes[f];
    // a zero component is +0: the table's integers, converted
    const rtg_camera c = {*eye,
                          {(float)t[1][0] * rs, (float)t[1][1] * rs, (float)t[1][2] * rs},
                          {(float)t[2][0] * us, (float)t[2][1] * us, (float)t[2][2] * us},
                          {(float)-t[0][0], (float)-t[0][1], (float)-t[0][2]}};
    out[f] = c;
  }
  return RTG_OK;
}

int rtg_render_views_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                          unsigned lgtNum, const rtg_camera* poses, size_t nViews,
                          unsigned width, unsigned height, float zoom, float aliasFactor,
                          int stackSize, int semantics, rtg_vec* dstHost, int walk, int nthreads) {
  rtg_clear_error();
  Camera c;
  unsigned tilesX = 0, tilesPerView = 0;
  size_t blocks = 0;
  int rc = check_views_frame(poses, nViews, dstHost, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_views(nViews, width, height, stackSize, &tilesX, &tilesPerView, &blocks);
  if (!rc) rc = check_scene_arrays("render_views", spheres, sphNum, lights, lgtNum);
  if (!rc) rc = check_semantics("render_views", semantics);
  if (!rc) rc = check_walk("render_views", walk);
  if (!rc) rc = check_sphere_count("render_views", sphNum);
  if (rc) return rc;
  if (nViews == 0) return RTG_OK;
  PackedScene ps;
  pack_scene(spheres, sphNum, lights, lgtNum, &ps);  // as rtg_context_set_scene
  const bool bvh = walk == 1 && !ps.bvhNodes.empty();
  const RayBox box = bvh ? ray_box(ps.originBox) : RayBox{};
  const CamHostFn fn = host_trace_fn(
      stackSize, semantics == RTG_SEMANTICS_OPENCL, walk == 1, bvh,
      [](auto s, auto cl, auto wk, auto bv) -> CamHostFn {
        return camera_host_range<s.value, cl.value, wk.value, bv.value>;
      });
  const size_t per = (size_t)width * height;
  // bands of the batch's pixels; a band's part of view v is pixels [lo, hi) of it
  host_bands(nViews * per, nthreads, [&](size_t k0, size_t k1) {
    for (size_t v = k0 / per; v * per < k1; ++v) {
      const size_t lo = k0 > v * per ? k0 - v * per : 0;
      const size_t hi = k1 - v * per < per ? k1 - v * per : per;
      fn(ps, box, c, cam_pose(poses[v]), width, lo, hi, dstHost + v * per);
    }
  });
  return RTG_OK;
}

int rtg_render_views_device(rtg_context* ctx, const rtg_camera* posesDevice, size_t nViews,
                            unsigned width, unsigned height, float zoom, float aliasFactor,
                            int stackSize, rtg_vec* dstDevice, void* stream) {
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0, semantics = RTG_SEMANTICS_CPU;
  if (!rtg_context_scene(ctx, &a, &device, &box, &semantics)) {
    rtg_set_error("render_views: no context/scene");
    return RTG_ERR_INVALID;
  }
  Camera c;
  unsigned tilesX = 0, tilesPerView = 0;
  size_t blocks = 0;
  int rc = check_views_frame(posesDevice, nViews, dstDevice, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_views(nViews, width, height, stackSize, &tilesX, &tilesPerView, &blocks);
  if (rc) return rc;
  if ((uintptr_t)posesDevice % 4) {
    rtg_set_error("render_views: pose table not 4-byte aligned");
    return RTG_ERR_INVALID;
  }
  if (nViews == 0) return RTG_OK;
  DeviceGuard deviceGuard;  // (after the checks: no GPU call before them)
  const bool bvh = a.bvhNodes != nullptr;
  const StackKernels* sk = stack_kernels(stackSize);
  const ViewsFn fn = sk ? sk->views(bvh, semantics == RTG_SEMANTICS_OPENCL) : nullptr;
  if (!fn) {  // a missing kernel is an error, never another path
    rtg_set_error("render_views: no kernel for stackSize %d", stackSize);
    return RTG_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64), raytrace_lds_bytes(stackSize, bvh),
                     (hipStream_t)stream, a, box, c,
                     reinterpret_cast<const CamPose*>(posesDevice), width, height, tilesX,
                     tilesPerView, dstDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_render_views(int device, const rtg_sphere* spheres, unsigned sphNum,
                     const rtg_light* lights, unsigned lgtNum, const rtg_camera* poses,
                     size_t nViews, unsigned width, unsigned height, float zoom,
                     float aliasFactor, int stackSize, rtg_vec* dstHost) {
  rtg_clear_error();
  Camera c;
  unsigned tilesX = 0, tilesPerView = 0;
  size_t blocks = 0;
  int rc = check_views_frame(poses, nViews, dstHost, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_views(nViews, width, height, stackSize, &tilesX, &tilesPerView, &blocks);
  if (!rc) rc = check_scene_arrays("render_views", spheres, sphNum, lights, lgtNum);
  if (rc) return rc;
  if (nViews == 0) return RTG_OK;
  DeviceGuard deviceGuard;  // (after the checks: no GPU call before them)
  return one_shot("render_views", device, {spheres, sphNum, lights, lgtNum}, poses,
                  nViews * sizeof(rtg_camera), dstHost, nViews * width * height * sizeof(rtg_vec),
                  [&](rtg_context* ctx, const void* in, void* out) {
                    return rtg_render_views_device(ctx, (const rtg_camera*)in, nViews, width,
                                                   height, zoom, aliasFactor, stackSize,
                                                   (rtg_vec*)out, nullptr);
                  });
}

// ---- many views folded into per-group coefficients (rtg_fold.h) ----

int rtg_render_views_fold_host(const rtg_sphere* spheres, unsigned sphNum,
                               const rtg_light* lights, unsigned lgtNum, const rtg_camera* poses,
                               size_t nViews, unsigned width, unsigned height, float zoom,
                               float aliasFactor, int stackSize, int semantics,
                               const rtg_fold_params* params, const float* weights,
                               rtg_vec* outHost, unsigned* skippedHost, int walk, int nthreads) {
  rtg_clear_error();
  Camera c;
  unsigned tilesX = 0, tilesPerView = 0;
  size_t blocks = 0;
  int rc = check_fold_views(poses, nViews, outHost, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_views(nViews, width, height, stackSize, &tilesX, &tilesPerView, &blocks);
  if (!rc) rc = check_scene_arrays("render_views_fold", spheres, sphNum, lights, lgtNum);
  if (!rc) rc = check_semantics("render_views_fold", semantics);
  if (!rc) rc = check_walk("render_views_fold", walk);
  if (!rc) rc = check_sphere_count("render_views_fold", sphNum);
  if (!rc)
    rc = check_fold("render_views_fold", nViews, width, height, params, weights, outHost, false,
                    nullptr, 0, &tilesX, &tilesPerView);
  if (rc) return rc;
  if (nViews == 0) return RTG_OK;
  // the composition itself: the host's frames, then the host's fold
  std::vector<rtg_vec> frames(nViews * width * height);
  rc = rtg_render_views_host(spheres, sphNum, lights, lgtNum, poses, nViews, width, height, zoom,
                             aliasFactor, stackSize, semantics, frames.data(), walk, nthreads);
  if (rc) return rc;
  return rtg_views_fold_host(frames.data(), nViews, width, height, params, weights, outHost,
                             skippedHost, nthreads);
}

int rtg_render_views_fold_device(rtg_context* ctx, const rtg_camera* posesDevice, size_t nViews,
                                 unsigned width, unsigned height, float zoom, float aliasFactor,
                                 int stackSize, const rtg_fold_params* params,
                                 const float* weightsDevice, rtg_vec* outDevice,
                                 unsigned* skippedDevice, void* scratchDevice,
                                 size_t scratchBytes, void* stream) {
  rtg_clear_error();
  SceneTables a{};
  RayBox box{};
  int device = 0, semantics = RTG_SEMANTICS_CPU;
  if (!rtg_context_scene(ctx, &a, &device, &box, &semantics)) {
    rtg_set_error("render_views_fold: no context/scene");
    return RTG_ERR_INVALID;
  }
  Camera c;
  unsigned tilesX = 0, tilesPerView = 0;
  size_t blocks = 0;
  int rc = check_fold_views(posesDevice, nViews, outDevice, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_views(nViews, width, height, stackSize, &tilesX, &tilesPerView, &blocks);
  if (!rc && (uintptr_t)posesDevice % 4) {
    rtg_set_error("render_views_fold: pose table not 4-byte aligned");
    rc = RTG_ERR_INVALID;
  }
  if (!rc)
    rc = check_fold("render_views_fold", nViews, width, height, params, weightsDevice, outDevice,
                    true, scratchDevice, scratchBytes, &tilesX, &tilesPerView);
  if (rc) return rc;
  if (nViews == 0) return RTG_OK;
  DeviceGuard deviceGuard;  // (after the checks: no GPU call before them)
  const bool bvh = a.bvhNodes != nullptr;
  const StackKernels* sk = stack_kernels(stackSize);
  const ViewsFoldFn fn = sk ? sk->views_fold(bvh, semantics == RTG_SEMANTICS_OPENCL) : nullptr;
  if (!fn) {  // a missing kernel is an error, never another path
    rtg_set_error("render_views_fold: no kernel for stackSize %d", stackSize);
    return RTG_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  const FoldArgs fa = {weightsDevice, static_cast<unsigned*>(scratchDevice), params->weights,
                       params->viewsPerGroup, params->flags & RTG_FOLD_SKIP_NONFINITE};
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64), raytrace_lds_bytes(stackSize, bvh),
                     (hipStream_t)stream, a, box, c,
                     reinterpret_cast<const CamPose*>(posesDevice), width, height, tilesX,
                     tilesPerView, fa);
  HIP_TRY(hipGetLastError());
  return launch_fold_stage2(scratchDevice, nViews, tilesPerView, *params, outDevice,
                            skippedDevice, (hipStream_t)stream);
}

int rtg_render_views_fold(int device, const rtg_sphere* spheres, unsigned sphNum,
                          const rtg_light* lights, unsigned lgtNum, const rtg_camera* poses,
                          size_t nViews, unsigned width, unsigned height, float zoom,
                          float aliasFactor, int stackSize, const rtg_fold_params* params,
                          const float* weights, rtg_vec* outHost, unsigned* skippedHost) {
  rtg_clear_error();
  Camera c;
  unsigned tilesX = 0, tilesPerView = 0;
  size_t blocks = 0;
  int rc = check_fold_views(poses, nViews, outHost, width, height, zoom, aliasFactor, &c);
  if (!rc) rc = check_views(nViews, width, height, stackSize, &tilesX, &tilesPerView, &blocks);
  if (!rc) rc = check_scene_arrays("render_views_fold", spheres, sphNum, lights, lgtNum);
  if (!rc)
    rc = check_fold("render_views_fold", nViews, width, height, params, weights, outHost, false,
                    nullptr, 0, &tilesX, &tilesPerView);
  if (rc) return rc;
  if (nViews == 0) return RTG_OK;
  DeviceGuard deviceGuard;  // (after the checks: no GPU call before them)
  const size_t K = params->weights, nGroups = nViews / params->viewsPerGroup;
  const size_t tableBytes = (size_t)params->viewsPerGroup * width * height * K * sizeof(float);
  const size_t scratchBytes = nViews * tilesPerView * fold_tile_words(params->weights) * 4;
  const StageScene scene{spheres, sphNum, lights, lgtNum};
  return one_shot("render_views_fold", device, &scene,
                  {{nViews * sizeof(rtg_camera), poses, nullptr},
                   {tableBytes, weights, nullptr},
                   {scratchBytes, nullptr, nullptr},
                   {nGroups * K * sizeof(rtg_vec), nullptr, outHost},
                   {skippedHost ? nGroups * sizeof(unsigned) : 0, nullptr, skippedHost}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_render_views_fold_device(
                        ctx, (const rtg_camera*)d[0], nViews, width, height, zoom, aliasFactor,
                        stackSize, params, (const float*)d[1], (rtg_vec*)d[3], (unsigned*)d[4],
                        d[2], scratchBytes, nullptr);
                  });
}

// Real SH of bands l = 0 .. bands-1 at the unit vector (x, y, z), k = l(l+1)+m.
static void real_sh(unsigned bands, double x, double y, double z, double* Y) {
  Y[0] = 0.28209479177387814;
  if (bands < 2) return;
  Y[1] = 0.4886025119029199 * y;
  Y[2] = 0.4886025119029199 * z;
  Y[3] = 0.4886025119029199 * x;
  if (bands < 3) return;
  Y[4] = 1.0925484305920792 * (x * y);
  Y[5] = 1.0925484305920792 * (y * z);
  Y[6] = 0.31539156525252005 * (3.0 * (z * z) - 1.0);
  Y[7] = 1.0925484305920792 * (x * z);
  Y[8] = 0.5462742152960396 * (x * x - y * y);
  if (bands < 4) return;
  Y[9] = 0.5900435899266435 * (y * (3.0 * (x * x) - y * y));
  Y[10] = 2.890611442640554 * ((x * y) * z);
  Y[11] = 0.4570457994644658 * (y * (5.0 * (z * z) - 1.0));
  Y[12] = 0.3731763325901154 * (z * (5.0 * (z * z) - 3.0));
  Y[13] = 0.4570457994644658 * (x * (5.0 * (z * z) - 1.0));
  Y[14] = 1.445305721320277 * (z * (x * x - y * y));
  Y[15] = 0.5900435899266435 * (x * (x * x - 3.0 * (y * y)));
}

// The corner term of a rectangle's solid angle seen from distance 1.
static double corner_angle(double u, double v) { return atan2(u * v, sqrt((u * u + v * v) + 1.0)); }

int rtg_cube_sh_weights(unsigned res, unsigned bands, float aliasFactor, float* out) {
  rtg_clear_error();
  if (!out) {
    rtg_set_error("cube_sh_weights: null pointer");
    return RTG_ERR_INVALID;
  }
  if (bands < 1 || bands > 4) {
    rtg_set_error("cube_sh_weights: bands %u outside [1, 4]", bands);
    return RTG_ERR_INVALID;
  }
  Camera c;
  const int rc = make_camera(res, res, -1.f, aliasFactor, &c);  // res > 0, the range, nAA
  if (rc) return rc;
  const unsigned K = bands * bands;
  if (6 > SIZE_MAX / sizeof(float) / K / ((size_t)res * res)) {
    rtg_set_error("cube_sh_weights: table too large (res %u)", res);
    return RTG_ERR_INVALID;
  }
  const double cell = 2.0 / (double)res;
  // the mean of sample offsets 0 .. nAA-1, right of and above the corner
  const double mean = c.nAA > 0 ? 0.5 * (double)(c.nAA - 1) : 0.0;
  const double du = mean * (2.0 / ((double)res * (double)aliasFactor));
  const double dv = mean * ((8.0 / 3.0) / ((double)res * (double)aliasFactor));
  // the cells' solid angles: one face's, the same on all six
  std::vector<double> omega((size_t)res * res);
  double total = 0.0;
  for (unsigned y = 0; y < res; ++y) {
    for (unsigned x = 0; x < res; ++x) {
      const double u0 = -1.0 + cell * (double)x, v0 = 1.0 - cell * (double)y;
      const double u1 = u0 + cell, v1 = v0 + cell;
      const double o = ((corner_angle(u1, v1) - corner_angle(u0, v1)) - corner_angle(u1, v0)) +
                       corner_angle(u0, v0);
      omega[(size_t)y * res + x] = o;
      total += o;
    }
  }
  const double scale = (4.0 * 3.14159265358979323846) / (6.0 * total);
  for (unsigned f = 0; f < 6; ++f) {
    const signed char(*t)[3] = kCubeAxes[f];
    for (unsigned y = 0; y < res; ++y) {
      for (unsigned x = 0; x < res; ++x) {
        const double u = (-1.0 + cell * (double)x) + du, v = (1.0 - cell * (double)y) + dv;
        double d[3];
        for (int q = 0; q < 3; ++q) d[q] = ((double)t[0][q] + u * (double)t[1][q]) + v * (double)t[2][q];
        const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        double Y[16];
        real_sh(bands, d[0] / len, d[1] / len, d[2] / len, Y);
        const size_t e = ((size_t)f * res + y) * res + x;
        const double o = omega[(size_t)y * res + x] * scale;
        for (unsigned k = 0; k < K; ++k) out[e * K + k] = (float)(Y[k] * o);
      }
    }
  }
  return RTG_OK;
}

}  // extern "C"
