// rtg_accumulate.h — temporal accumulation by reprojection (rtg_accumulate*,
// rtg.h): the per-pixel code, ONE definition for the kernel and the host loops
// (rtg_accumulate.hip), the way filter_tap is shared.
//
// A pixel projects its hit point into the previous pose (camera_project,
// rtg_camera.h), fetches the previous frame's state with four validated
// bilinear taps (the filter's id rule and weight terms, rtg_filter.h, on the
// bilinear weight) and blends its current value in by the history length.
// C is the channel count (3: RTG_FILTER_RGB, 1: GRAY and COUNT), kM2 whether
// the call carries second moments.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#pragma once

#include <math.h>

#include "rtg.h"
#include "rtg_camera.h"
#include "rtg_filter.h"

// (the terms are the filter's own code: one set of bits)
static_assert(RTG_ACCUM_SAME_ID == RTG_FILTER_SAME_ID && RTG_ACCUM_NORMAL == RTG_FILTER_NORMAL &&
                  RTG_ACCUM_PLANE == RTG_FILTER_PLANE &&
                  RTG_ACCUM_SKIP_NONFINITE == RTG_FILTER_SKIP_NONFINITE,
              "rtg_accumulate's flags are the filter's");

namespace rtg {

// The previous frame's state and how to find a point in it; hits == nullptr
// on a reset frame (then nothing else is read).
struct AccumPrev {
  const rtg_hit* hits;
  const float* acc;  // W H C
  const unsigned short* len;
  const float* m2;  // W H C, kM2 only
  ProjFrame frame;
  CamPose pose;
};

// What the pixels of a call share.
struct AccumTerms {
  FilterTerms t;        // RTG_ACCUM_* bits, normalLog2, planeScale
  unsigned maxHistory;  // 1..65535
  unsigned W, H;        // <= 2^24 each
};

// Pixel p: `c` its guide, `cur` its converted value; `guide(h)` reads a
// previous record (the kernel's two 16-byte loads, or plain loads).  Writes
// the C words of outAcc (and of outM2) and returns outLen.
template <int C, bool kM2, class Guide>
RTG_HD unsigned accum_pixel(const AccumTerms& a, const AccumPrev& pv, Guide guide,
                            const FilterGuide& c, const float* cur, float* outAcc, float* outM2) {
  float cur2[C];
  for (int q = 0; q < C; ++q) cur2[q] = cur[q] * cur[q];
  if (c.id < 0) {
    for (int q = 0; q < C; ++q) outAcc[q] = cur[q];
    if (kM2) for (int q = 0; q < C; ++q) outM2[q] = cur2[q];
    return 0;
  }
  float sum[C], s2[C], sw = 0.f;
  for (int q = 0; q < C; ++q) sum[q] = s2[q] = 0.f;
  unsigned nmin = 0xFFFFu;
  if (pv.hits) {
    const V3 r = camera_project(pv.frame, pv.pose, c.p);
    const float fx = r.x, fy = r.y, k = r.z;
    if (k > 0.f && fx > -1.f && fx < (float)a.W && fy > -1.f && fy < (float)a.H) {
      const float xf = floorf(fx), yf = floorf(fy);
      const float tx = fx - xf, ty = fy - yf;
      const int x0 = (int)xf, y0 = (int)yf;  // -1 .. 2^24 - 1
      for (int dy = 0; dy < 2; ++dy) {
        const int yq = y0 + dy;
        if (yq < 0 || yq >= (int)a.H) continue;
        const float wy = dy ? ty : 1.f - ty;
        for (int dx = 0; dx < 2; ++dx) {
          const int xq = x0 + dx;
          if (xq < 0 || xq >= (int)a.W) continue;
          const float wx = dx ? tx : 1.f - tx;
          const size_t j = (size_t)yq * a.W + (size_t)xq;  // inside the frame: < W H
          const unsigned len = pv.len[j];
          if (len == 0) continue;
          const FilterGuide g = guide(pv.hits + j);
          if (!filter_admits(a.t, c.id, g.id)) continue;
          float v[C];
          for (int q = 0; q < C; ++q) v[q] = pv.acc[j * C + q];
          if ((a.t.flags & RTG_ACCUM_SKIP_NONFINITE) && filter_nonfinite<C>(v)) continue;
          const float w = filter_weight(a.t, c, g, wy * wx);
          if (!(w > 0.f)) continue;
          for (int q = 0; q < C; ++q) sum[q] = sum[q] + w * v[q];
          if (kM2) for (int q = 0; q < C; ++q) s2[q] = s2[q] + w * pv.m2[j * C + q];
          sw = sw + w;
          nmin = len < nmin ? len : nmin;
        }
      }
    }
  }
  const bool found = sw > 0.f;
  const bool curOK = !((a.t.flags & RTG_ACCUM_SKIP_NONFINITE) && filter_nonfinite<C>(cur));
  if (!found) {
    for (int q = 0; q < C; ++q) outAcc[q] = cur[q];
    if (kM2) for (int q = 0; q < C; ++q) outM2[q] = cur2[q];
    return curOK ? 1u : 0u;
  }
  float hist[C], hist2[C];
  for (int q = 0; q < C; ++q) hist[q] = sum[q] / sw;
  for (int q = 0; q < C; ++q) hist2[q] = kM2 ? s2[q] / sw : 0.f;
  if (!curOK) {
    for (int q = 0; q < C; ++q) outAcc[q] = hist[q];
    if (kM2) for (int q = 0; q < C; ++q) outM2[q] = hist2[q];
    return nmin;
  }
  const unsigned n = nmin + 1 < a.maxHistory ? nmin + 1 : a.maxHistory;
  const float alpha = 1.f / (float)n;
  for (int q = 0; q < C; ++q) outAcc[q] = hist[q] + alpha * (cur[q] - hist[q]);
  if (kM2) for (int q = 0; q < C; ++q) outM2[q] = hist2[q] + alpha * (cur2[q] - hist2[q]);
  return n;
}

}  // namespace rtg
