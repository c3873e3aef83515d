// rtg_svgf.h — the variance estimate and the variance-guided a-trous passes
// (rtg_variance*, rtg_svgf*, rtg.h): the per-pixel and per-tap code, ONE
// definition for the kernels and the host loops of rtg_svgf.hip.  The tap
// rule's id part, the geometric weight, the guides, the overlap test and the
// check of the terms are rtg_filter.h's.
//
// C is the channel count (3: RTG_FILTER_RGB, 1: RTG_FILTER_GRAY).
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#pragma once

#include <math.h>

#include "rtg_filter.h"

namespace rtg {

// lum(v) of the definition.
template <int C>
RTG_HD float svgf_lum(const float* v) {
  if (C == 1) return v[0];
  return (0.2126f * v[0] + 0.7152f * v[1]) + 0.0722f * v[2];
}

// ---- rtg_variance* ----

constexpr int kVarianceRadius = 3;  // the spatial estimate's 7 x 7 window

template <int C>
struct VarianceSum {
  float s1[C], s2[C];
  float sw;
};

template <int C>
RTG_HD void variance_clear(VarianceSum<C>& a) {
  for (int q = 0; q < C; ++q) a.s1[q] = a.s2[q] = 0.f;
  a.sw = 0.f;
}

// An admitted tap of the window: `c` the centre's guide, `g`, `acc` and `m2`
// the tap's guide and moments.
template <int C>
RTG_HD void variance_tap(const FilterTerms& t, const FilterGuide& c, const FilterGuide& g,
                         const float* acc, const float* m2, VarianceSum<C>& a) {
  if ((t.flags & RTG_FILTER_SKIP_NONFINITE) && (filter_nonfinite<C>(acc) || filter_nonfinite<C>(m2)))
    return;
  const float w = filter_weight(t, c, g, 1.f);
  if (!(w > 0.f)) return;
  for (int q = 0; q < C; ++q) {
    a.s1[q] = a.s1[q] + w * acc[q];
    a.s2[q] = a.s2[q] + w * m2[q];
  }
  a.sw = a.sw + w;
}

// The window's moments, or the pixel's own (`acc`, `m2`) when no tap was taken.
template <int C>
RTG_HD void variance_spatial(const VarianceSum<C>& a, const float* acc, const float* m2, float* m,
                             float* e) {
  for (int q = 0; q < C; ++q) {
    m[q] = a.sw > 0.f ? a.s1[q] / a.sw : acc[q];
    e[q] = a.sw > 0.f ? a.s2[q] / a.sw : m2[q];
  }
}

// var[p] of a hit pixel from its first and second moments.
template <int C>
RTG_HD float variance_value(const float* m, const float* e) {
  float d[C];
  for (int q = 0; q < C; ++q) {
    const float mm = m[q] * m[q];
    d[q] = e[q] - mm;
    d[q] = d[q] > 0.f ? d[q] : 0.f;
  }
  return svgf_lum<C>(d);
}

// ---- rtg_svgf* ----

// What the taps of a call share beside the filter's terms.
struct SvgfTerms {
  FilterTerms t;  // the filter's four bits only
  unsigned luma;  // RTG_SVGF_LUMA is set
  float sigmaL, epsL;
};

template <int C>
struct SvgfSum {
  float v[C];
  float sv, sw;
};

template <int C>
RTG_HD void svgf_clear(SvgfSum<C>& a) {
  for (int q = 0; q < C; ++q) a.v[q] = 0.f;
  a.sv = a.sw = 0.f;
}

// k[i + 1] of the 3 x 3 prefilter, i = -1 .. 1.
RTG_HD float svgf_k(int i) { return i == 0 ? 0.5f : 0.25f; }

// An admitted tap of the prefilter: `kw` = k[dy + 1] * k[dx + 1], `var` the
// tap's variance.
RTG_HD void svgf_prefilter_tap(const FilterTerms& t, float var, float kw, float& gs, float& gw) {
  if ((t.flags & RTG_FILTER_SKIP_NONFINITE) && fold_nonfinite(var)) return;
  gs = gs + kw * var;
  gw = gw + kw;
}

// ls of the definition: one over the centre's scaled standard deviation;
// `var` is the pixel's own variance.
RTG_HD float svgf_scale(const SvgfTerms& s, float gs, float gw, float var) {
  const float g = gw > 0.f ? gs / gw : var;
  const float den = s.sigmaL * sqrtf(g) + s.epsL;
  return 1.f / den;
}

// An admitted tap of a pass: `hw` = h[dy + 2] * h[dx + 2], `c` the centre's
// guide, `g`, `v` and `var` the tap's guide, value and variance, `lp` and `ls`
// the centre's luminance and scale (not read without LUMA).
template <int C>
RTG_HD void svgf_tap(const SvgfTerms& s, const FilterGuide& c, const FilterGuide& g, const float* v,
                     float var, float hw, float lp, float ls, SvgfSum<C>& a) {
  if ((s.t.flags & RTG_FILTER_SKIP_NONFINITE) && (filter_nonfinite<C>(v) || fold_nonfinite(var)))
    return;
  float w = filter_weight(s.t, c, g, hw);
  if (s.luma) {
    const float l = fabsf(svgf_lum<C>(v) - lp);
    float z = 1.f - l * ls;
    z = z > 0.f ? z : 0.f;
    w = w * z;
  }
  if (!(w > 0.f)) return;
  for (int q = 0; q < C; ++q) a.v[q] = a.v[q] + w * v[q];
  a.sv = a.sv + (w * w) * var;
  a.sw = a.sw + w;
}

// The pixel's result; `in` and `var` are its own value and variance.
template <int C>
RTG_HD void svgf_result(const SvgfSum<C>& a, const float* in, float var, float* out, float* vout) {
  for (int q = 0; q < C; ++q) out[q] = a.sw > 0.f ? a.v[q] / a.sw : in[q];
  *vout = a.sw > 0.f ? a.sv / (a.sw * a.sw) : var;
}

}  // namespace rtg
