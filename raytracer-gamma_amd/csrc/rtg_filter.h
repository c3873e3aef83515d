// rtg_filter.h — the edge-stopping a-trous filter (rtg_filter*, rtg.h): the
// per-tap code, ONE definition for the pass kernels and the host loops
// (rtg_filter.hip), the way gather_add and ao_world are shared, and what a
// frame of a kind is to the filter and to the accumulation alike
// (rtg_accumulate.hip): its sizes, the overlap test, the record loader and the
// check of the terms; and the tile geometry and the value store that the
// variance-guided passes (rtg_svgf.hip) share with the filter's kernels.
//
// A pass visits 25 taps per pixel.  filter_admits is the part of the tap rule
// that needs the ids alone (the forms read nothing else of a tap it rejects),
// filter_tap the weight and the accumulate step, filter_result the quotient.
// C is the channel count (3: RTG_FILTER_RGB, 1: GRAY and COUNT).
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rtg.h"
#include "rtg_fold.h"
#include "rtg_internal.h"
#include "rtg_trace.h"
#if defined(__HIPCC__)
#include "rtg_entry.h"  // nan_bits, for the kernels' stores
#endif

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

#if defined(__HIPCC__)
// The same words as two 16-byte loads; `h` is 16-byte aligned (the device
// entry points check).
__device__ __forceinline__ FilterGuide filter_load_guide(const rtg_hit* h) {
  const uint4* r = reinterpret_cast<const uint4*>(h);
  const uint4 a = r[0], b = r[1];
  FilterGuide g;
  g.id = (int)a.x;
  g.p = v3(__uint_as_float(a.z), __uint_as_float(a.w), __uint_as_float(b.x));
  g.n = v3(__uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w));
  return g;
}
#endif

// Channels and bytes per source value of a kind.
inline int filter_channels(unsigned kind) { return kind == RTG_FILTER_RGB ? 3 : 1; }
inline size_t filter_src_size(unsigned kind) {
  return kind == RTG_FILTER_RGB ? sizeof(rtg_vec)
                                : kind == RTG_FILTER_GRAY ? sizeof(float) : sizeof(unsigned short);
}

// Byte ranges [a, a + na) and [b, b + nb), addresses as numbers; a null or
// empty range overlaps nothing.
inline bool filter_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && na && nb && x < y + nb && y < x + na;
}

// normalLog2, the kind and the flags (RTG_ACCUM_* are the same bits,
// rtg_accumulate.h), in the order they are reported in.
inline int check_filter_terms(const char* what, unsigned normalLog2, unsigned kind,
                              unsigned flags) {
  if (normalLog2 > 8) {
    rtg_set_error("%s: normalLog2 %u outside [0, 8]", what, normalLog2);
    return RTG_ERR_INVALID;
  }
  if (kind > RTG_FILTER_COUNT) {
    rtg_set_error("%s: kind %u (0: RGB, 1: GRAY, 2: COUNT)", what, kind);
    return RTG_ERR_INVALID;
  }
  const unsigned known =
      RTG_FILTER_SAME_ID | RTG_FILTER_NORMAL | RTG_FILTER_PLANE | RTG_FILTER_SKIP_NONFINITE;
  if (flags & ~known) {
    rtg_set_error("%s: unknown flags 0x%x", what, flags & ~known);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
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

#if defined(__HIPCC__)
// ---- what the frame kernels share (rtg_filter.hip, rtg_svgf.hip) ----
// One lane per pixel, workgroups of 256 lanes on 32 x 8 tiles of the frame,
// tiles numbered row-major in a one-dimensional grid.
constexpr unsigned kFilterTileW = 32, kFilterTileH = 8, kFilterThreads = 256;
constexpr size_t kFilterLdsMax = 160 * 1024;  // a workgroup's LDS on gfx950

// The lane's pixel of a pass record (its W, H and tilesX); false outside the frame.
template <class Pass>
__device__ __forceinline__ bool filter_pixel(const Pass& a, long long& x, long long& y) {
  x = (long long)(blockIdx.x % a.tilesX) * kFilterTileW + threadIdx.x % kFilterTileW;
  y = (long long)(blockIdx.x / a.tilesX) * kFilterTileH + threadIdx.x / kFilterTileW;
  return x < (long long)a.W && y < (long long)a.H;
}

// A pixel's C words out; `last`: NaN words go out as 0xFFC00000.
template <int C>
__device__ __forceinline__ void filter_store_value(unsigned* out, size_t i, const float* v,
                                                   unsigned last) {
#pragma unroll
  for (int q = 0; q < C; ++q) out[i * C + q] = last ? nan_bits(v[q]) : __float_as_uint(v[q]);
}
#endif

}  // namespace rtg
