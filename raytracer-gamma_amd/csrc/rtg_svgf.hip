// rtg_svgf.hip — the variance-guided half of the denoising chain of librtg.so
// (rtg_variance*, rtg_svgf*, rtg.h): rtg_accumulate*'s moments in, one variance
// per pixel out; then the a-trous passes of rtg_filter* with one more
// edge-stopping term, on the signal itself and scaled by the local standard
// deviation, and the variance carried from pass to pass.
//
// The per-pixel and per-tap code is rtg_svgf.h's, one definition for the
// kernels and the host loops below; the tap rule, the geometric weight and the
// tile geometry are rtg_filter.h's.  All kernels: one lane per pixel,
// workgroups of 256 lanes on 32 x 8 tiles, tiles numbered row-major in a
// one-dimensional grid.
//
// variance_kernel: the workgroup votes whether any of its pixels is a hit with
// a history shorter than minHistory.  If none is (every tile of a converged
// sequence), the kernel is a stream: the record's id, acc, m2 and len in, one
// word out.  Otherwise the tile plus a halo of 3 cells, 38 x 14 cells, goes
// into LDS as planes of one word per cell (id, point, normal, acc's and m2's
// channels: 7 + 2C planes, 27 KB for RGB), cells outside the frame with id -1,
// and the 7 x 7 window runs from LDS with no bounds test.
//
// svgf_tiled_kernel: rtg_filter.hip's tiled form with one more plane, the
// variance (8 + C planes): (32 + 4s) x (8 + 4s) cells, 19 KB at s = 1 (RGB),
// 51 KB at s = 4, 110 KB at s = 8; s = 16 does not fit the 160 KiB.  The 3 x 3
// prefilter reads the staged variance plane: the halo is 2s >= 2 cells.  A
// tile without a point stages nothing.  Taps are ds_read_b32 of 32 consecutive
// words of one row of one plane per half-wave: no row padding is needed.
// svgf_direct_kernel: taps from global memory, for the steps whose halo does
// not fit or does not pay.  The choice per step is kSvgfTiledMaxStep
// (DESIGN.md §28); env RTG_SVGF_FORM=tiled|direct forces one form wherever it
// fits (a performance knob: the words are the same either way).
//
// A call of `passes` passes ping-pongs value and variance between (dst,
// dstVar) and the two parts of the caller's scratch so that the last pass
// lands in dst and dstVar.
//
// Bounds: a lane outside the frame leaves before any store (after the
// barriers, in the staged forms); a staged cell and a direct tap are read only
// after the frame test in 64-bit integers; a pixel index is < W H; a staged
// tap lies within the halo of its form (3 cells, 2s cells, 1 <= 2s cells).
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rtg.h"
#include "rtg_entry.h"
#include "rtg_svgf.h"

static_assert(sizeof(rtg_variance_params) == 20, "rtg_variance_params is 20 B");
static_assert(sizeof(rtg_svgf_params) == 28, "rtg_svgf_params is 28 B");
static_assert(RTG_SVGF_LUMA == 16, "next to the filter's four bits");

namespace rtg {

// The largest step the tiled form takes by default.
constexpr unsigned kSvgfTiledMaxStep = 4;

constexpr int kVarStageW = (int)kFilterTileW + 2 * kVarianceRadius;
constexpr int kVarStageH = (int)kFilterTileH + 2 * kVarianceRadius;
constexpr int kVarCells = kVarStageW * kVarStageH;

// What the variance kernel takes.
struct VariancePass {
  const rtg_hit* hits;
  const float *acc, *m2;  // W H C floats each
  const unsigned short* len;
  unsigned* out;  // W H words
  unsigned W, H, tilesX;
  FilterTerms t;
  unsigned minHistory;
};

// What a pass kernel takes.
struct SvgfPass {
  const rtg_hit* hits;
  const float *in, *vin;  // W H C floats, W H floats
  unsigned *out, *vout;   // W H C words, W H words
  unsigned W, H, tilesX, step;
  SvgfTerms s;
  unsigned last;  // the call's last pass: NaN words go out as 0xFFC00000
};

constexpr size_t svgf_stage_cells(unsigned s) {
  return (size_t)(kFilterTileW + 4 * s) * (kFilterTileH + 4 * s);
}
constexpr size_t svgf_stage_bytes(unsigned s, int C) {
  return svgf_stage_cells(s) * (8 + C) * sizeof(unsigned);
}

template <int C>
__device__ __forceinline__ void svgf_load_value(const float* in, size_t i, float* v) {
#pragma unroll
  for (int q = 0; q < C; ++q) v[q] = in[i * C + q];
}

// A staged cell's point and normal (planes 1 .. 6 of `cells` words each).
__device__ __forceinline__ V3 stage_v3(const unsigned* stage, int plane, int cells, int k) {
  return v3(__uint_as_float(stage[plane * cells + k]), __uint_as_float(stage[(plane + 1) * cells + k]),
            __uint_as_float(stage[(plane + 2) * cells + k]));
}

// A frame cell's guide into planes 0 .. 6 at cell k, id -1 outside the frame;
// true inside.
__device__ __forceinline__ bool stage_guide(unsigned* stage, int cells, int k, const rtg_hit* hits,
                                            long long gx, long long gy, unsigned W, unsigned H,
                                            size_t& j) {
  const bool in = gx >= 0 && gx < (long long)W && gy >= 0 && gy < (long long)H;
  int id = -1;
  if (in) {
    j = (size_t)gy * W + (size_t)gx;  // inside the frame: < W H
    const FilterGuide g = filter_load_guide(hits + j);
    id = g.id;
    stage[1 * cells + k] = __float_as_uint(g.p.x);
    stage[2 * cells + k] = __float_as_uint(g.p.y);
    stage[3 * cells + k] = __float_as_uint(g.p.z);
    stage[4 * cells + k] = __float_as_uint(g.n.x);
    stage[5 * cells + k] = __float_as_uint(g.n.y);
    stage[6 * cells + k] = __float_as_uint(g.n.z);
  }
  stage[k] = (unsigned)id;  // a cell outside the frame: only its id is ever read
  return in;
}

template <int C>
__global__ __launch_bounds__(kFilterThreads) void variance_kernel(const VariancePass a) {
  __shared__ unsigned stage[(7 + 2 * C) * kVarCells];
  constexpr int cells = kVarCells, RW = kVarStageW;
  long long x, y;
  const bool inside = filter_pixel(a, x, y);
  const size_t i = inside ? (size_t)y * a.W + (size_t)x : 0;  // < W H
  const int id = inside ? a.hits[i].id : -1;
  const bool isShort = id >= 0 && (unsigned)a.len[i] < a.minHistory;
  if (!__syncthreads_or(isShort)) {
    // the stream: every history of the tile is long enough
    if (!inside) return;
    float v = 0.f;
    if (id >= 0) {
      float m[C], e[C];
      svgf_load_value<C>(a.acc, i, m);
      svgf_load_value<C>(a.m2, i, e);
      v = variance_value<C>(m, e);
    }
    a.out[i] = nan_bits(v);
    return;
  }
  const long long ox = (long long)(blockIdx.x % a.tilesX) * kFilterTileW - kVarianceRadius;
  const long long oy = (long long)(blockIdx.x / a.tilesX) * kFilterTileH - kVarianceRadius;
  for (int k = (int)threadIdx.x; k < cells; k += (int)kFilterThreads) {  // k < cells: in the planes
    size_t j = 0;
    if (stage_guide(stage, cells, k, a.hits, ox + k % RW, oy + k / RW, a.W, a.H, j)) {
      float m[C], e[C];
      svgf_load_value<C>(a.acc, j, m);
      svgf_load_value<C>(a.m2, j, e);
#pragma unroll
      for (int q = 0; q < C; ++q) {
        stage[(7 + q) * cells + k] = __float_as_uint(m[q]);
        stage[(7 + C + q) * cells + k] = __float_as_uint(e[q]);
      }
    }
  }
  __syncthreads();
  if (!inside) return;
  if (id < 0) {
    a.out[i] = 0u;
    return;
  }
  // the lane's own cell: the tile starts 3 cells into the stage
  const int k0 = ((int)(threadIdx.x / kFilterTileW) + kVarianceRadius) * RW +
                 (int)(threadIdx.x % kFilterTileW) + kVarianceRadius;
  float m[C], e[C];
#pragma unroll
  for (int q = 0; q < C; ++q) {
    m[q] = __uint_as_float(stage[(7 + q) * cells + k0]);
    e[q] = __uint_as_float(stage[(7 + C + q) * cells + k0]);
  }
  if (isShort) {
    const bool wantN = (a.t.flags & RTG_FILTER_NORMAL) != 0, wantP = (a.t.flags & RTG_FILTER_PLANE) != 0;
    FilterGuide c;
    c.id = id;
    c.p = stage_v3(stage, 1, cells, k0);
    c.n = stage_v3(stage, 4, cells, k0);
    VarianceSum<C> sum;
    variance_clear(sum);
    for (int dy = -kVarianceRadius; dy <= kVarianceRadius; ++dy) {
#pragma unroll
      for (int dx = -kVarianceRadius; dx <= kVarianceRadius; ++dx) {
        const int k = k0 + dy * RW + dx;  // within 3 cells of the tile: in the stage
        FilterGuide g;
        g.id = (int)stage[k];
        if (!filter_admits(a.t, c.id, g.id)) continue;
        // (a term that is off reads none of its planes, and none of these zeros)
        g.p = g.n = v3(0.f, 0.f, 0.f);
        if (wantP) g.p = stage_v3(stage, 1, cells, k);
        if (wantN) g.n = stage_v3(stage, 4, cells, k);
        float mq[C], eq[C];
#pragma unroll
        for (int q = 0; q < C; ++q) {
          mq[q] = __uint_as_float(stage[(7 + q) * cells + k]);
          eq[q] = __uint_as_float(stage[(7 + C + q) * cells + k]);
        }
        variance_tap<C>(a.t, c, g, mq, eq, sum);
      }
    }
    float ms[C], es[C];
    variance_spatial<C>(sum, m, e, ms, es);
#pragma unroll
    for (int q = 0; q < C; ++q) {
      m[q] = ms[q];
      e[q] = es[q];
    }
  }
  a.out[i] = nan_bits(variance_value<C>(m, e));
}

template <int C>
__device__ __forceinline__ void svgf_store(const SvgfPass& a, size_t i, const float* v, float var) {
  filter_store_value<C>(a.out, i, v, a.last);
  filter_store_value<1>(a.vout, i, &var, a.last);
}

template <int C>
__global__ __launch_bounds__(kFilterThreads) void svgf_direct_kernel(const SvgfPass a) {
  long long x, y;
  if (!filter_pixel(a, x, y)) return;
  const size_t i = (size_t)y * a.W + (size_t)x;  // < W H
  const FilterGuide c = filter_load_guide(a.hits + i);
  float in[C], out[C];
  svgf_load_value<C>(a.in, i, in);
  const float var = a.vin[i];
  if (c.id < 0) {
    svgf_store<C>(a, i, in, var);
    return;
  }
  float lp = 0.f, ls = 0.f;
  if (a.s.luma) {
    float gs = 0.f, gw = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const long long yq = y + dy;
      if (yq < 0 || yq >= (long long)a.H) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const long long xq = x + dx;
        if (xq < 0 || xq >= (long long)a.W) continue;
        const size_t j = (size_t)yq * a.W + (size_t)xq;  // inside the frame: < W H
        if (!filter_admits(a.s.t, c.id, a.hits[j].id)) continue;
        svgf_prefilter_tap(a.s.t, a.vin[j], svgf_k(dy) * svgf_k(dx), gs, gw);
      }
    }
    ls = svgf_scale(a.s, gs, gw, var);
    lp = svgf_lum<C>(in);
  }
  SvgfSum<C> acc;
  svgf_clear(acc);
  const long long s = a.step;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const long long yq = y + dy * s;
    if (yq < 0 || yq >= (long long)a.H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const long long xq = x + dx * s;
      if (xq < 0 || xq >= (long long)a.W) continue;
      const size_t j = (size_t)yq * a.W + (size_t)xq;  // inside the frame: < W H
      const FilterGuide g = filter_load_guide(a.hits + j);
      if (!filter_admits(a.s.t, c.id, g.id)) continue;
      float v[C];
      svgf_load_value<C>(a.in, j, v);
      svgf_tap<C>(a.s, c, g, v, a.vin[j], filter_h(dy) * filter_h(dx), lp, ls, acc);
    }
  }
  float vout;
  svgf_result<C>(acc, in, var, out, &vout);
  svgf_store<C>(a, i, out, vout);
}

template <int C>
__global__ __launch_bounds__(kFilterThreads) void svgf_tiled_kernel(const SvgfPass a) {
  extern __shared__ unsigned stage[];  // 8 + C planes of RW * RH words
  const int s = (int)a.step;           // <= 8: the launcher's choice
  const int RW = (int)kFilterTileW + 4 * s, RH = (int)kFilterTileH + 4 * s, cells = RW * RH;
  long long x, y;
  const bool inside = filter_pixel(a, x, y);
  const size_t i = inside ? (size_t)y * a.W + (size_t)x : 0;  // < W H
  // a tile without a point has no taps: its pixels pass through, nothing is staged
  if (!__syncthreads_or(inside && a.hits[i].id >= 0)) {
    if (inside) {
      float v[C];
      svgf_load_value<C>(a.in, i, v);
      svgf_store<C>(a, i, v, a.vin[i]);
    }
    return;
  }
  const long long ox = (long long)(blockIdx.x % a.tilesX) * kFilterTileW - 2 * s;
  const long long oy = (long long)(blockIdx.x / a.tilesX) * kFilterTileH - 2 * s;
  for (int k = (int)threadIdx.x; k < cells; k += (int)kFilterThreads) {  // k < cells: in the planes
    size_t j = 0;
    if (stage_guide(stage, cells, k, a.hits, ox + k % RW, oy + k / RW, a.W, a.H, j)) {
      float v[C];
      svgf_load_value<C>(a.in, j, v);
#pragma unroll
      for (int q = 0; q < C; ++q) stage[(7 + q) * cells + k] = __float_as_uint(v[q]);
      stage[(7 + C) * cells + k] = __float_as_uint(a.vin[j]);
    }
  }
  __syncthreads();
  if (!inside) return;
  // the lane's own cell: the tile starts 2s cells into the stage
  const int k0 = ((int)(threadIdx.x / kFilterTileW) + 2 * s) * RW +
                 (int)(threadIdx.x % kFilterTileW) + 2 * s;
  const bool wantN = (a.s.t.flags & RTG_FILTER_NORMAL) != 0,
             wantP = (a.s.t.flags & RTG_FILTER_PLANE) != 0;
  FilterGuide c;
  c.id = (int)stage[k0];
  c.p = stage_v3(stage, 1, cells, k0);
  c.n = stage_v3(stage, 4, cells, k0);
  float in[C], out[C];
#pragma unroll
  for (int q = 0; q < C; ++q) in[q] = __uint_as_float(stage[(7 + q) * cells + k0]);
  const float var = __uint_as_float(stage[(7 + C) * cells + k0]);
  if (c.id < 0) {
    svgf_store<C>(a, i, in, var);
    return;
  }
  float lp = 0.f, ls = 0.f;
  if (a.s.luma) {
    float gs = 0.f, gw = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int k = k0 + dy * RW + dx;  // within 1 <= 2s cells of the tile: in the stage
        if (!filter_admits(a.s.t, c.id, (int)stage[k])) continue;
        svgf_prefilter_tap(a.s.t, __uint_as_float(stage[(7 + C) * cells + k]),
                           svgf_k(dy) * svgf_k(dx), gs, gw);
      }
    }
    ls = svgf_scale(a.s, gs, gw, var);
    lp = svgf_lum<C>(in);
  }
  SvgfSum<C> acc;
  svgf_clear(acc);
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = k0 + dy * s * RW + dx * s;  // within 2s cells of the tile: in the stage
      FilterGuide g;
      g.id = (int)stage[k];
      if (!filter_admits(a.s.t, c.id, g.id)) continue;
      // (a term that is off reads none of its planes, and none of these zeros)
      g.p = g.n = v3(0.f, 0.f, 0.f);
      if (wantP) g.p = stage_v3(stage, 1, cells, k);
      if (wantN) g.n = stage_v3(stage, 4, cells, k);
      float v[C];
#pragma unroll
      for (int q = 0; q < C; ++q) v[q] = __uint_as_float(stage[(7 + q) * cells + k]);
      svgf_tap<C>(a.s, c, g, v, __uint_as_float(stage[(7 + C) * cells + k]),
                  filter_h(dy) * filter_h(dx), lp, ls, acc);
    }
  }
  float vout;
  svgf_result<C>(acc, in, var, out, &vout);
  svgf_store<C>(a, i, out, vout);
}

// ---- host forms ----

static inline unsigned host_bits(float v, bool canon) {
  unsigned u;
  memcpy(&u, &v, 4);
  return canon ? nan_bits(v) : u;
}

// Rows [y0, y1) of the variance estimate.
template <int C>
static void variance_host_rows(const rtg_hit* hits, unsigned W, unsigned H, const FilterTerms& t,
                               unsigned minHistory, const float* acc, const float* m2,
                               const unsigned short* len, unsigned* out, size_t y0, size_t y1) {
  for (size_t y = y0; y < y1; ++y) {
    for (size_t x = 0; x < W; ++x) {
      const size_t i = y * W + x;
      const FilterGuide c = filter_guide(hits + i);
      float v = 0.f;
      if (c.id >= 0) {
        float m[C], e[C];
        for (int q = 0; q < C; ++q) {
          m[q] = acc[i * C + q];
          e[q] = m2[i * C + q];
        }
        if ((unsigned)len[i] < minHistory) {
          VarianceSum<C> sum;
          variance_clear(sum);
          for (int dy = -kVarianceRadius; dy <= kVarianceRadius; ++dy) {
            for (int dx = -kVarianceRadius; dx <= kVarianceRadius; ++dx) {
              const long long xq = (long long)x + dx, yq = (long long)y + dy;
              if (xq < 0 || xq >= (long long)W || yq < 0 || yq >= (long long)H) continue;
              const size_t j = (size_t)yq * W + (size_t)xq;
              const FilterGuide g = filter_guide(hits + j);
              if (!filter_admits(t, c.id, g.id)) continue;
              variance_tap<C>(t, c, g, acc + j * C, m2 + j * C, sum);
            }
          }
          variance_spatial<C>(sum, acc + i * C, m2 + i * C, m, e);
        }
        v = variance_value<C>(m, e);
      }
      out[i] = nan_bits(v);
    }
  }
}

// Rows [y0, y1) of one pass over (in, vin) into (out, vout).
template <int C>
static void svgf_host_rows(const rtg_hit* hits, unsigned W, unsigned H, unsigned step,
                           const SvgfTerms& s, const float* in, const float* vin, unsigned* out,
                           unsigned* vout, bool last, size_t y0, size_t y1) {
  const long long st = step;
  for (size_t y = y0; y < y1; ++y) {
    for (size_t x = 0; x < W; ++x) {
      const size_t i = y * W + x;
      const FilterGuide c = filter_guide(hits + i);
      float res[C], rv = vin[i];
      for (int q = 0; q < C; ++q) res[q] = in[i * C + q];
      if (c.id >= 0) {
        float lp = 0.f, ls = 0.f;
        if (s.luma) {
          float gs = 0.f, gw = 0.f;
          for (int dy = -1; dy <= 1; ++dy) {
            for (int dx = -1; dx <= 1; ++dx) {
              const long long xq = (long long)x + dx, yq = (long long)y + dy;
              if (xq < 0 || xq >= (long long)W || yq < 0 || yq >= (long long)H) continue;
              const size_t j = (size_t)yq * W + (size_t)xq;
              if (!filter_admits(s.t, c.id, hits[j].id)) continue;
              svgf_prefilter_tap(s.t, vin[j], svgf_k(dy) * svgf_k(dx), gs, gw);
            }
          }
          ls = svgf_scale(s, gs, gw, vin[i]);
          lp = svgf_lum<C>(in + i * C);
        }
        SvgfSum<C> acc;
        svgf_clear(acc);
        for (int dy = -2; dy <= 2; ++dy) {
          for (int dx = -2; dx <= 2; ++dx) {
            const long long xq = (long long)x + dx * st, yq = (long long)y + dy * st;
            if (xq < 0 || xq >= (long long)W || yq < 0 || yq >= (long long)H) continue;
            const size_t j = (size_t)yq * W + (size_t)xq;
            const FilterGuide g = filter_guide(hits + j);
            if (!filter_admits(s.t, c.id, g.id)) continue;
            svgf_tap<C>(s, c, g, in + j * C, vin[j], filter_h(dy) * filter_h(dx), lp, ls, acc);
          }
        }
        svgf_result<C>(acc, in + i * C, vin[i], res, &rv);
      }
      for (int q = 0; q < C; ++q) out[i * C + q] = host_bits(res[q], last);
      vout[i] = host_bits(rv, last);
    }
  }
}

}  // namespace rtg

using namespace rtg;

// W, H and the pixel count, in the order they are reported in; *n = W H.
static int check_frame_size(const char* what, unsigned W, unsigned H, size_t* n) {
  if (W == 0 || H == 0) {
    rtg_set_error("%s: empty frame %u x %u", what, W, H);
    return RTG_ERR_INVALID;
  }
  const unsigned long long px = (unsigned long long)W * H;
  if (px > 0xFFFFFFFFull) {
    rtg_set_error("%s: %llu pixels (at most 2^32 - 1)", what, px);
    return RTG_ERR_INVALID;
  }
  *n = (size_t)px;
  return RTG_OK;
}

// The terms of either call; the states are floats, so COUNT is no kind here.
static int check_float_terms(const char* what, unsigned normalLog2, unsigned kind, unsigned flags) {
  const int rc = check_filter_terms(what, normalLog2, kind, flags);
  if (rc) return rc;
  if (kind == RTG_FILTER_COUNT) {
    rtg_set_error("%s: kind COUNT (the values are floats: RGB or GRAY)", what);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// The grid of a frame; *tilesX and *tiles.
static int frame_tiles(const char* what, unsigned W, unsigned H, size_t* tilesX, size_t* tiles) {
  *tilesX = ((size_t)W + kFilterTileW - 1) / kFilterTileW;
  *tiles = *tilesX * (((size_t)H + kFilterTileH - 1) / kFilterTileH);
  if (*tiles > 0x7FFFFFFFu) {  // (with 32 x 8 tiles no frame of 2^32 - 1 pixels gets here)
    rtg_set_error("%s: frame too large (%zu workgroups)", what, *tiles);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// A named byte range of a call, for its overlap checks.
struct Range {
  const char* name;
  const void* p;
  size_t bytes;
  bool written;
};

// No written range may overlap another range.
static int check_ranges(const char* what, const Range* r, int count) {
  for (int a = 0; a < count; ++a) {
    for (int b = a + 1; b < count; ++b) {
      if ((r[a].written || r[b].written) && filter_overlap(r[a].p, r[a].bytes, r[b].p, r[b].bytes)) {
        rtg_set_error("%s: the %s overlaps the %s", what, r[b].name, r[a].name);
        return RTG_ERR_INVALID;
      }
    }
  }
  return RTG_OK;
}

// ---- rtg_variance* ----

// What the host and the device forms share.
static int check_variance(const char* what, const void* hits, unsigned W, unsigned H,
                          const rtg_variance_params* p, const void* acc, const void* m2,
                          const void* len, const void* var, size_t* n) {
  if (!hits || !acc || !m2 || !len || !var) {
    rtg_set_error("%s: null %s", what,
                  !hits ? "hit buffer" : !acc ? "acc" : !m2 ? "m2" : !len ? "len" : "destination");
    return RTG_ERR_INVALID;
  }
  if (!p) {
    rtg_set_error("%s: null params", what);
    return RTG_ERR_INVALID;
  }
  int rc = check_frame_size(what, W, H, n);
  if (rc) return rc;
  rc = check_float_terms(what, p->normalLog2, p->kind, p->flags);
  if (rc) return rc;
  if (p->minHistory > 65535) {
    rtg_set_error("%s: minHistory %u outside [0, 65535]", what, p->minHistory);
    return RTG_ERR_INVALID;
  }
  const size_t vb = *n * (size_t)filter_channels(p->kind) * sizeof(float);
  const Range r[] = {{"acc", acc, vb, false},
                     {"m2", m2, vb, false},
                     {"len", len, *n * sizeof(unsigned short), false},
                     {"destination", var, *n * sizeof(float), true}};
  return check_ranges(what, r, 4);
}

// ---- rtg_svgf* ----

static size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// The scratch's value part and the whole of it.
static size_t svgf_scratch_value_bytes(size_t n, const rtg_svgf_params& p) {
  return round16(n * (size_t)filter_channels(p.kind) * sizeof(float));
}
static size_t svgf_scratch_bytes(size_t n, const rtg_svgf_params& p) {
  if (p.passes < 2) return 0;
  return svgf_scratch_value_bytes(n, p) + round16(n * sizeof(float));
}

static int check_svgf_frame(const char* what, unsigned W, unsigned H, const rtg_svgf_params* p,
                            size_t* n) {
  if (!p) {
    rtg_set_error("%s: null params", what);
    return RTG_ERR_INVALID;
  }
  const int rc = check_frame_size(what, W, H, n);
  if (rc) return rc;
  if (p->passes < 1 || p->passes > RTG_FILTER_MAX_PASSES) {
    rtg_set_error("%s: %u passes outside [1, %d]", what, p->passes, RTG_FILTER_MAX_PASSES);
    return RTG_ERR_INVALID;
  }
  return check_float_terms(what, p->normalLog2, p->kind, p->flags & ~(unsigned)RTG_SVGF_LUMA);
}

// What the host and the device forms share; the scratch is null on the host.
static int check_svgf(const char* what, const void* hits, unsigned W, unsigned H,
                      const rtg_svgf_params* p, const void* src, const void* varSrc,
                      const void* dst, const void* dstVar, const void* scratch,
                      size_t scratchBytes, size_t* n) {
  if (!hits || !src || !varSrc || !dst || !dstVar) {
    rtg_set_error("%s: null %s", what,
                  !hits ? "hit buffer" : !src ? "source" : !varSrc ? "source variance"
                  : !dst ? "destination" : "destination variance");
    return RTG_ERR_INVALID;
  }
  const int rc = check_svgf_frame(what, W, H, p, n);
  if (rc) return rc;
  const size_t vb = *n * (size_t)filter_channels(p->kind) * sizeof(float);
  const Range r[] = {{"source", src, vb, false},
                     {"source variance", varSrc, *n * sizeof(float), false},
                     {"destination", dst, vb, true},
                     {"destination variance", dstVar, *n * sizeof(float), true},
                     {"scratch", scratch, scratchBytes, true}};
  return check_ranges(what, r, 5);
}

static SvgfTerms svgf_terms(const rtg_svgf_params& p) {
  SvgfTerms s;
  s.t = {p.flags & ~(unsigned)RTG_SVGF_LUMA, p.normalLog2, p.planeScale};
  s.luma = (p.flags & RTG_SVGF_LUMA) != 0;
  s.sigmaL = p.sigmaL;
  s.epsL = p.epsL;
  return s;
}

// One pass on `stream`; the device is set.
template <int C>
static int launch_svgf_pass(const SvgfPass& a, unsigned blocks, bool tiled, hipStream_t stream) {
  if (tiled) {
    const size_t lds = svgf_stage_bytes(a.step, C);
    if (lds > 48 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&svgf_tiled_kernel<C>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((svgf_tiled_kernel<C>), dim3(blocks), dim3(kFilterThreads), lds, stream, a);
  } else {
    hipLaunchKernelGGL((svgf_direct_kernel<C>), dim3(blocks), dim3(kFilterThreads), 0, stream, a);
  }
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

extern "C" {

int rtg_variance_host(const rtg_hit* hits, unsigned width, unsigned height,
                      const rtg_variance_params* params, const float* acc, const float* m2,
                      const unsigned short* len, float* varHost, int nthreads) {
  rtg_clear_error();
  size_t n = 0;
  const int rc = check_variance("variance", hits, width, height, params, acc, m2, len, varHost, &n);
  if (rc) return rc;
  const rtg_variance_params p = *params;
  const FilterTerms t = {p.flags, p.normalLog2, p.planeScale};
  unsigned* out = reinterpret_cast<unsigned*>(varHost);
  host_bands(height, nthreads, [&](size_t y0, size_t y1) {
    if (p.kind == RTG_FILTER_RGB)
      variance_host_rows<3>(hits, width, height, t, p.minHistory, acc, m2, len, out, y0, y1);
    else
      variance_host_rows<1>(hits, width, height, t, p.minHistory, acc, m2, len, out, y0, y1);
  });
  return RTG_OK;
}

int rtg_variance_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                        unsigned height, const rtg_variance_params* params, const float* accDevice,
                        const float* m2Device, const unsigned short* lenDevice, float* varDevice,
                        void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("variance: no context");
    return RTG_ERR_INVALID;
  }
  size_t n = 0;
  int rc = check_variance("variance", hitsDevice, width, height, params, accDevice, m2Device,
                          lenDevice, varDevice, &n);
  if (rc) return rc;
  if ((uintptr_t)hitsDevice & 15) {
    rtg_set_error("variance: hit buffer not 16-byte aligned");
    return RTG_ERR_INVALID;
  }
  size_t tilesX = 0, tiles = 0;
  rc = frame_tiles("variance", width, height, &tilesX, &tiles);
  if (rc) return rc;
  const rtg_variance_params p = *params;
  HIP_TRY(hipSetDevice(device));
  VariancePass a{};
  a.hits = hitsDevice;
  a.acc = accDevice;
  a.m2 = m2Device;
  a.len = lenDevice;
  a.out = reinterpret_cast<unsigned*>(varDevice);
  a.W = width;
  a.H = height;
  a.tilesX = (unsigned)tilesX;
  a.t = {p.flags, p.normalLog2, p.planeScale};
  a.minHistory = p.minHistory;
  const hipStream_t st = (hipStream_t)stream;
  if (p.kind == RTG_FILTER_RGB)
    hipLaunchKernelGGL((variance_kernel<3>), dim3((unsigned)tiles), dim3(kFilterThreads), 0, st, a);
  else
    hipLaunchKernelGGL((variance_kernel<1>), dim3((unsigned)tiles), dim3(kFilterThreads), 0, st, a);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_variance(int device, const rtg_hit* hits, unsigned width, unsigned height,
                 const rtg_variance_params* params, const float* acc, const float* m2,
                 const unsigned short* len, float* varHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  size_t n = 0;
  const int rc = check_variance("variance", hits, width, height, params, acc, m2, len, varHost, &n);
  if (rc) return rc;
  const size_t vb = n * (size_t)filter_channels(params->kind) * sizeof(float);
  return one_shot("variance", device, nullptr,
                  {{n * sizeof(rtg_hit), hits, nullptr},
                   {vb, acc, nullptr},
                   {vb, m2, nullptr},
                   {n * sizeof(unsigned short), len, nullptr},
                   {n * sizeof(float), nullptr, varHost}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_variance_device(ctx, (const rtg_hit*)d[0], width, height, params,
                                               (const float*)d[1], (const float*)d[2],
                                               (const unsigned short*)d[3], (float*)d[4], nullptr);
                  });
}

int rtg_svgf_scratch(unsigned width, unsigned height, const rtg_svgf_params* params,
                     size_t* bytes) {
  rtg_clear_error();
  if (!bytes) {
    rtg_set_error("svgf_scratch: null size");
    return RTG_ERR_INVALID;
  }
  size_t n = 0;
  const int rc = check_svgf_frame("svgf_scratch", width, height, params, &n);
  if (rc) return rc;
  *bytes = svgf_scratch_bytes(n, *params);
  return RTG_OK;
}

int rtg_svgf_host(const rtg_hit* hits, unsigned width, unsigned height,
                  const rtg_svgf_params* params, const float* src, const float* varSrc,
                  float* dstHost, float* dstVarHost, int nthreads) {
  rtg_clear_error();
  size_t n = 0;
  const int rc = check_svgf("svgf", hits, width, height, params, src, varSrc, dstHost, dstVarHost,
                            nullptr, 0, &n);
  if (rc) return rc;
  const rtg_svgf_params p = *params;
  const SvgfTerms s = svgf_terms(p);
  const size_t C = (size_t)filter_channels(p.kind);
  // the passes' images: two of each to ping-pong between
  std::vector<float> bufs[2], vbufs[2];
  const float *in = src, *vin = varSrc;
  for (unsigned i = 0; i < p.passes; ++i) {
    const bool last = i + 1 == p.passes;
    if (!last) {
      bufs[i & 1].resize(n * C);
      vbufs[i & 1].resize(n);
    }
    unsigned* out = reinterpret_cast<unsigned*>(last ? dstHost : bufs[i & 1].data());
    unsigned* vout = reinterpret_cast<unsigned*>(last ? dstVarHost : vbufs[i & 1].data());
    host_bands(height, nthreads, [&](size_t y0, size_t y1) {
      if (C == 3) svgf_host_rows<3>(hits, width, height, 1u << i, s, in, vin, out, vout, last, y0, y1);
      else svgf_host_rows<1>(hits, width, height, 1u << i, s, in, vin, out, vout, last, y0, y1);
    });
    in = reinterpret_cast<const float*>(out);
    vin = reinterpret_cast<const float*>(vout);
  }
  return RTG_OK;
}

int rtg_svgf_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width, unsigned height,
                    const rtg_svgf_params* params, const float* srcDevice,
                    const float* varSrcDevice, float* dstDevice, float* dstVarDevice,
                    void* scratchDevice, size_t scratchBytes, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("svgf: no context");
    return RTG_ERR_INVALID;
  }
  size_t n = 0;
  int rc = check_svgf("svgf", hitsDevice, width, height, params, srcDevice, varSrcDevice, dstDevice,
                      dstVarDevice, nullptr, 0, &n);
  if (rc) return rc;
  const rtg_svgf_params p = *params;
  if ((uintptr_t)hitsDevice & 15) {
    rtg_set_error("svgf: hit buffer not 16-byte aligned");
    return RTG_ERR_INVALID;
  }
  const size_t need = svgf_scratch_bytes(n, p);
  if (need) {
    if (!scratchDevice) {
      rtg_set_error("svgf: null scratch (%zu bytes needed)", need);
      return RTG_ERR_INVALID;
    }
    if (scratchBytes < need || ((uintptr_t)scratchDevice & 15)) {
      rtg_set_error("svgf: scratch of %zu bytes at %p (%zu needed, 16-byte aligned)", scratchBytes,
                    scratchDevice, need);
      return RTG_ERR_INVALID;
    }
    rc = check_svgf("svgf", hitsDevice, width, height, params, srcDevice, varSrcDevice, dstDevice,
                    dstVarDevice, scratchDevice, need, &n);
    if (rc) return rc;
  }
  size_t tilesX = 0, tiles = 0;
  rc = frame_tiles("svgf", width, height, &tilesX, &tiles);
  if (rc) return rc;
  int force = 0;  // 1: tiled wherever it fits, 2: direct
  if (const char* v = getenv("RTG_SVGF_FORM")) {  // A/B knob (performance only)
    force = !strcmp(v, "tiled") ? 1 : !strcmp(v, "direct") ? 2 : 0;
  }
  HIP_TRY(hipSetDevice(device));
  const int C = filter_channels(p.kind);
  unsigned* const scratchValue = static_cast<unsigned*>(scratchDevice);
  unsigned* const scratchVar = need ? reinterpret_cast<unsigned*>(static_cast<char*>(scratchDevice) +
                                                                  svgf_scratch_value_bytes(n, p))
                                    : nullptr;
  SvgfPass a{};
  a.hits = hitsDevice;
  a.W = width;
  a.H = height;
  a.tilesX = (unsigned)tilesX;
  a.s = svgf_terms(p);
  a.in = srcDevice;
  a.vin = varSrcDevice;
  for (unsigned i = 0; i < p.passes; ++i) {
    a.step = 1u << i;
    a.last = i + 1 == p.passes;
    const bool toDst = (p.passes - 1 - i) % 2 == 0;
    a.out = toDst ? reinterpret_cast<unsigned*>(dstDevice) : scratchValue;
    a.vout = toDst ? reinterpret_cast<unsigned*>(dstVarDevice) : scratchVar;
    const bool fits = svgf_stage_bytes(a.step, C) <= kFilterLdsMax;
    const bool tiled = fits && force != 2 && (force == 1 || a.step <= kSvgfTiledMaxStep);
    const hipStream_t st = (hipStream_t)stream;
    rc = C == 3 ? launch_svgf_pass<3>(a, (unsigned)tiles, tiled, st)
                : launch_svgf_pass<1>(a, (unsigned)tiles, tiled, st);
    if (rc) return rc;
    a.in = reinterpret_cast<const float*>(a.out);
    a.vin = reinterpret_cast<const float*>(a.vout);
  }
  return RTG_OK;
}

int rtg_svgf(int device, const rtg_hit* hits, unsigned width, unsigned height,
             const rtg_svgf_params* params, const float* src, const float* varSrc, float* dstHost,
             float* dstVarHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  size_t n = 0;
  const int rc = check_svgf("svgf", hits, width, height, params, src, varSrc, dstHost, dstVarHost,
                            nullptr, 0, &n);
  if (rc) return rc;
  const size_t scratchBytes = svgf_scratch_bytes(n, *params);
  const size_t vb = n * (size_t)filter_channels(params->kind) * sizeof(float);
  return one_shot("svgf", device, nullptr,
                  {{n * sizeof(rtg_hit), hits, nullptr},
                   {vb, src, nullptr},
                   {n * sizeof(float), varSrc, nullptr},
                   {vb, nullptr, dstHost},
                   {n * sizeof(float), nullptr, dstVarHost},
                   {scratchBytes, nullptr, nullptr}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_svgf_device(ctx, (const rtg_hit*)d[0], width, height, params,
                                           (const float*)d[1], (const float*)d[2], (float*)d[3],
                                           (float*)d[4], d[5], scratchBytes, nullptr);
                  });
}

}  // extern "C"
