// rtg_upsample.h — guided upsampling of a low-resolution signal
// (rtg_upsample*, rtg.h): the per-pixel code, ONE definition for the kernel and
// the host loops (rtg_upsample.hip), the way accum_pixel is shared.
//
// A full pixel lies between four pixels of the low frame of the same pose at
// dyadic fractions; each of the four is validated against the pixel's own
// record by the filter's id rule and weight terms (rtg_filter.h) on the
// bilinear weight.  A hit pixel none of whose taps is accepted is a hole.
// C is the channel count (3: RTG_FILTER_RGB, 1: GRAY and COUNT), kCount
// whether the low values are unsigned short.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#pragma once

#include "rtg.h"
#include "rtg_filter.h"

// (the terms are the filter's own code: one set of bits)
static_assert(RTG_UPSAMPLE_SAME_ID == RTG_FILTER_SAME_ID &&
                  RTG_UPSAMPLE_NORMAL == RTG_FILTER_NORMAL &&
                  RTG_UPSAMPLE_PLANE == RTG_FILTER_PLANE &&
                  RTG_UPSAMPLE_SKIP_NONFINITE == RTG_FILTER_SKIP_NONFINITE,
              "rtg_upsample's flags are the filter's");

namespace rtg {

// What the pixels of a call share.
struct UpTerms {
  FilterTerms t;    // RTG_UPSAMPLE_* bits, normalLog2, planeScale
  unsigned L;       // 1..3
  unsigned W;       // the full frame's width, <= 2^24
  unsigned Wl, Hl;  // the low frame
};

// The low frame.
struct UpLow {
  const rtg_hit* hits;
  const void* src;  // Wl Hl values of the kind
};

// Full pixel (x, y) with guide `c`, id >= 0; `guide(h)` reads a low record
// (the kernel's two 16-byte loads, or plain loads).  Writes the C words of
// `out` and returns whether the pixel is a hole.
template <int C, bool kCount, class Guide>
RTG_HD bool upsample_pixel(const UpTerms& u, const UpLow& lo, Guide guide, const FilterGuide& c,
                           unsigned x, unsigned y, float* out) {
  const unsigned f = 1u << u.L;
  const float inv = 1.f / (float)f;
  const unsigned x0 = x >> u.L, y0 = y >> u.L;  // inside the low frame
  const float tx = (float)(x & (f - 1)) * inv, ty = (float)(y & (f - 1)) * inv;
  float sum[C], sw = 0.f;
  for (int q = 0; q < C; ++q) sum[q] = 0.f;
  for (unsigned dy = 0; dy < 2; ++dy) {
    const unsigned yq = y0 + dy;
    if (yq >= u.Hl) continue;
    const float wy = dy ? ty : 1.f - ty;
    for (unsigned dx = 0; dx < 2; ++dx) {
      const unsigned xq = x0 + dx;
      if (xq >= u.Wl) continue;
      const float wx = dx ? tx : 1.f - tx;
      const size_t j = (size_t)yq * u.Wl + (size_t)xq;  // inside the low frame: < Wl Hl
      const FilterGuide g = guide(lo.hits + j);
      if (!filter_admits(u.t, c.id, g.id)) continue;
      float v[C];
      if (kCount) {
        v[0] = (float)static_cast<const unsigned short*>(lo.src)[j];
      } else {
        for (int q = 0; q < C; ++q) v[q] = static_cast<const float*>(lo.src)[j * C + q];
      }
      if ((u.t.flags & RTG_UPSAMPLE_SKIP_NONFINITE) && filter_nonfinite<C>(v)) continue;
      const float w = filter_weight(u.t, c, g, wy * wx);
      if (!(w > 0.f)) continue;
      for (int q = 0; q < C; ++q) sum[q] = sum[q] + w * v[q];
      sw = sw + w;
    }
  }
  const bool found = sw > 0.f;
  for (int q = 0; q < C; ++q) out[q] = found ? sum[q] / sw : 0.f;
  return !found;
}

}  // namespace rtg
