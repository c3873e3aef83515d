// rtg_camera.h — the posed camera's sample ray (rtg_camera, rtg.h), ONE
// function for the fused render kernel (rtg_camera_kernels.h), the generator
// kernel and both host forms (rtg_camera.hip), as sample_dir (rtg_trace.h) is
// shared by the renders.
#pragma once

#include "rtg.h"
#include "rtg_trace.h"

namespace rtg {

// rtg_camera as the kernels take it (48 B, by value).
struct CamPose {
  V3 eye, right, up, back;
};

inline CamPose cam_pose(const rtg_camera& c) {
  CamPose p;
  p.eye = v3(c.eye.x, c.eye.y, c.eye.z);
  p.right = v3(c.right.x, c.right.y, c.right.z);
  p.up = v3(c.up.x, c.up.y, c.up.z);
  p.back = v3(c.back.x, c.back.y, c.back.z);
  return p;
}

// Direction of sample (i, j) of pixel (x, y) from the pose: (rx, ry) are
// sample_dir's (main.cpp:419-426); per component q, with no contraction,
//   v.q = (rx * right.q + ry * up.q) + zoom * back.q,  dir = vnorm(v).
// The basis is used as given.  At the identity pose every added term is a
// zero that leaves the other operand's bits (zoom * 0 is -0 for the render's
// negative zoom, and rx, ry are never -0), so dir is sample_dir's.
RTG_HD V3 camera_dir(const Camera& cam, const CamPose& p, unsigned x, unsigned y, int i, int j) {
  const float pxX = (((float)x - cam.halfW)) * cam.xs;
  const float pxY = (cam.halfH - (float)y) * cam.ys;
  const float rx = (pxX + (float)(((float)j) * cam.st)) * cam.asp;
  const float ry = (pxY + (float)(((float)i) * cam.st));
  const V3 v = v3((rx * p.right.x + ry * p.up.x) + cam.zoom * p.back.x,
                  (rx * p.right.y + ry * p.up.y) + cam.zoom * p.back.y,
                  (rx * p.right.z + ry * p.up.z) + cam.zoom * p.back.z);
  return vnorm(v);
}

// The frame constants of rtg_camera_project* (rtg.h): W, H <= 2^24, so their
// floats are exact; halfW, halfH as make_camera computes them.
struct ProjFrame {
  float zoom, kx, ky, halfW, halfH;
};

RTG_HD ProjFrame proj_frame(unsigned W, unsigned H, float zoom) {
  ProjFrame f;
  f.zoom = zoom;
  f.kx = (float)W * 0.046875f;  // 1 / (xs * asp)
  f.ky = (float)H / 12.f;
  f.halfW = W * 0.5f;
  f.halfH = H * 0.5f;
  return f;
}

// camera_dir's inverse for an orthonormal basis (rtg.h has the arithmetic):
// {fx, fy, k} of point P; P lies in front of the camera exactly when k > 0.f.
// ONE function for rtg_camera_project*'s kernel and host loops and for the
// lookup of rtg_accumulate* (rtg_accumulate.h).
RTG_HD V3 camera_project(const ProjFrame& f, const CamPose& c, V3 P) {
  const V3 e = vsub(P, c.eye);
  const float a = vdot(e, c.right), b = vdot(e, c.up), d = vdot(e, c.back);
  const float k = f.zoom / d;
  const float rx = a * k, ry = b * k;
  return v3(rx * f.kx + f.halfW, f.halfH - ry * f.ky, k);
}

}  // namespace rtg
