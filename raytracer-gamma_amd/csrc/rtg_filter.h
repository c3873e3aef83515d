// rtg_filter.h — the edge-stopping a-trous filter (rtg_filter*, rtg.h): the
// per-tap code, ONE definition for the pass kernels and the host loops
// (rtg_filter.hip), the way gather_add and ao_world are shared.
//
// A pass visits 25 taps per pixel.  filter_admits is the part of the tap rule
// that needs the ids alone (the forms read nothing else of a tap it rejects),
// filter_tap the weight and the accumulate step, filter_result the quotient.
// C is the channel count (3: RTG_FILTER_RGB, 1: GRAY and COUNT).
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#pragma once

#include "rtg.h"
#include "rtg_fold.h"
#include "rtg_trace.h"

namespace rtg {

// What the taps of a call share.
struct FilterTerms {
  unsigned flags;       // RTG_FILTER_* bits
  unsigned normalLog2;  // <= 8
  float planeScale;
};

// A pixel's guide words: rtg_hit without t.
struct FilterGuide {
  int id;
  V3 p, n;
};

template <int C>
struct FilterSum {
  float v[C];
  float sw;
};

RTG_HD FilterGuide filter_guide(const rtg_hit* h) {
  FilterGuide g;
  g.id = h->id;
  g.p = v3(h->point.x, h->point.y, h->point.z);
  g.n = v3(h->normal.x, h->normal.y, h->normal.z);
  return g;
}

// h[i + 2] of the definition, i = -2 .. 2.
RTG_HD float filter_h(int i) {
  return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f;
}

template <int C>
RTG_HD void filter_clear(FilterSum<C>& a) {
  for (int q = 0; q < C; ++q) a.v[q] = 0.f;
  a.sw = 0.f;
}

// The id part of the tap rule; the tap lies inside the frame.
RTG_HD bool filter_admits(const FilterTerms& t, int idP, int idQ) {
  return idQ >= 0 && (!(t.flags & RTG_FILTER_SAME_ID) || idQ == idP);
}

// Whether any of a value's C words is a NaN or an infinity.
template <int C>
RTG_HD bool filter_nonfinite(const float* v) {
  bool bad = false;
  for (int q = 0; q < C; ++q) bad = bad || fold_nonfinite(v[q]);
  return bad;
}

// A tap's weight: `hw` times the terms that are on, `c` the centre's guide and
// `g` the tap's (also the bilinear taps of rtg_accumulate.h).
RTG_HD float filter_weight(const FilterTerms& t, const FilterGuide& c, const FilterGuide& g,
                           float hw) {
  float w = hw;
  if (t.flags & RTG_FILTER_NORMAL) {
    float k = vdot(c.n, g.n);
    k = k > 0.f ? k : 0.f;
    for (unsigned i = 0; i < t.normalLog2; ++i) k = k * k;
    w = w * k;
  }
  if (t.flags & RTG_FILTER_PLANE) {
    const float d = fabsf(vdot(c.n, vsub(g.p, c.p)));
    float z = 1.f - d * t.planeScale;
    z = z > 0.f ? z : 0.f;
    w = w * z;
  }
  return w;
}

// An admitted tap: `hw` = h[dy + 2] * h[dx + 2], `c` the centre's guide, `g`
// and `v` the tap's guide and value.
template <int C>
RTG_HD void filter_tap(const FilterTerms& t, const FilterGuide& c, const FilterGuide& g,
                       const float* v, float hw, FilterSum<C>& a) {
  if ((t.flags & RTG_FILTER_SKIP_NONFINITE) && filter_nonfinite<C>(v)) return;
  const float w = filter_weight(t, c, g, hw);
  if (!(w > 0.f)) return;
  for (int q = 0; q < C; ++q) a.v[q] = a.v[q] + w * v[q];
  a.sw = a.sw + w;
}

// The pixel's result; `in` is its own value.
template <int C>
RTG_HD void filter_result(const FilterSum<C>& a, const float* in, float* out) {
  for (int q = 0; q < C; ++q) out[q] = a.sw > 0.f ? a.v[q] / a.sw : in[q];
}

}  // namespace rtg
