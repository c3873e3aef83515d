// rtg_filter.hip — the edge-stopping a-trous filter of librtg.so (rtg_filter*,
// rtg.h): a frame's per-pixel signal and its rtg_hit records in, the signal
// smoothed along the frame's surfaces out.
//
// One pass of step s visits the 25 taps (x + dx s, y + dy s) of every pixel;
// the tap rule, the weight and the accumulate step are rtg_filter.h's, one
// definition for the two kernels and the host loops below.  A call is `passes`
// launches, pass i with step 1 << i, ping-ponging between dst and the
// caller's scratch so that the last pass lands in dst: pass i writes dst when
// passes - 1 - i is even.  src is only read.
//
// Both kernels: one lane per pixel, workgroups of 256 lanes on 32 x 8 tiles
// of the frame, tiles numbered row-major in a one-dimensional grid (a frame
// may be 1 x 2^32 - 1).  Unlike every other kernel here they are memory- and
// LDS-bound: a tap is 28 guide bytes and the value, a few multiplies and one
// add per channel.
//
// filter_tiled_kernel: the workgroup stages its tile plus the 2s halo, (32 +
// 4s) x (8 + 4s) cells, into LDS as structure-of-arrays planes of one word per
// cell: id, point, normal and the value's channels, 7 + C planes.  A cell
// outside the frame is staged with id -1, which the tap rule leaves out, so
// the tap loop has no bounds test.  A tile none of whose pixels has a point
// stages nothing: its pixels pass through.  Taps are ds_read_b32: its conflict
// groups are the wave's two halves of 32 lanes, and a half reads 32
// consecutive words of one row of one plane, so no row padding is needed for
// any stride.  17 KB per workgroup at s = 1 (RGB), 46 KB at s = 4, 102 KB at
// s = 8 (one workgroup per CU); s = 16 does not fit the 160 KiB.
//
// filter_direct_kernel: taps from global memory, a record as two 16-byte
// loads, for the steps whose halo does not fit or does not pay: the 25 taps
// of a wave are 5 rows s W records apart.
//
// The choice per step is kFilterTiledMaxStep (DESIGN.md §24 has the
// measurement); env RTG_FILTER_FORM=tiled|direct forces one form wherever it
// fits (a performance knob: the words are the same either way).
//
// Bounds: a lane outside the frame leaves before any store (after the
// barrier, in the tiled form); a staged cell and a direct tap are read only
// after the frame test in 64-bit integers; a pixel index is < W H.
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
#include "rtg_filter.h"

static_assert(sizeof(rtg_filter_params) == 20, "rtg_filter_params is 20 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, id) == 0 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");
static_assert(sizeof(rtg_vec) == 12, "three floats per colour");

namespace rtg {

// (the tile geometry, filter_pixel and filter_store_value are rtg_filter.h's)
// The largest step the tiled form takes by default.
constexpr unsigned kFilterTiledMaxStep = 4;

// What a pass kernel takes.
struct FilterPass {
  const rtg_hit* hits;
  const void* in;  // W H C floats; pass 0 of RTG_FILTER_COUNT: the counts
  unsigned* out;   // W H C words
  unsigned W, H, tilesX, step;
  FilterTerms t;
  unsigned last;  // the call's last pass: NaN words go out as 0xFFC00000
};

// Cells of the tiled form's stage at step s.
constexpr size_t filter_stage_cells(unsigned s) {
  return (size_t)(kFilterTileW + 4 * s) * (kFilterTileH + 4 * s);
}
constexpr size_t filter_stage_bytes(unsigned s, int C) {
  return filter_stage_cells(s) * (7 + C) * sizeof(unsigned);
}

template <int C, bool kCount>
__device__ __forceinline__ void filter_load_value(const void* in, size_t i, float* v) {
  if constexpr (kCount) {
    v[0] = (float)static_cast<const unsigned short*>(in)[i];
  } else {
#pragma unroll
    for (int q = 0; q < C; ++q) v[q] = static_cast<const float*>(in)[i * C + q];
  }
}

template <int C, bool kCount>
__global__ __launch_bounds__(kFilterThreads) void filter_direct_kernel(const FilterPass a) {
  long long x, y;
  if (!filter_pixel(a, x, y)) return;
  const size_t i = (size_t)y * a.W + (size_t)x;  // < W H
  const FilterGuide c = filter_load_guide(a.hits + i);
  float in[C], out[C];
  filter_load_value<C, kCount>(a.in, i, in);
  if (c.id < 0) {
    filter_store_value<C>(a.out, i, in, a.last);
    return;
  }
  FilterSum<C> acc;
  filter_clear(acc);
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
      if (!filter_admits(a.t, c.id, g.id)) continue;
      float v[C];
      filter_load_value<C, kCount>(a.in, j, v);
      filter_tap<C>(a.t, c, g, v, filter_h(dy) * filter_h(dx), acc);
    }
  }
  filter_result<C>(acc, in, out);
  filter_store_value<C>(a.out, i, out, a.last);
}

template <int C, bool kCount>
__global__ __launch_bounds__(kFilterThreads) void filter_tiled_kernel(const FilterPass a) {
  extern __shared__ unsigned stage[];  // 7 + C planes of RW * RH words
  const int s = (int)a.step;           // <= 8: the launcher's choice
  const int RW = (int)kFilterTileW + 4 * s, RH = (int)kFilterTileH + 4 * s, cells = RW * RH;
  long long x, y;
  const bool inside = filter_pixel(a, x, y);
  const size_t i = inside ? (size_t)y * a.W + (size_t)x : 0;  // < W H
  // a tile without a point has no taps: its pixels pass through and nothing is
  // staged (a frame's background costs what it costs the direct form)
  if (!__syncthreads_or(inside && a.hits[i].id >= 0)) {
    if (inside) {
      float v[C];
      filter_load_value<C, kCount>(a.in, i, v);
      filter_store_value<C>(a.out, i, v, a.last);
    }
    return;
  }
  const long long ox = (long long)(blockIdx.x % a.tilesX) * kFilterTileW - 2 * s;
  const long long oy = (long long)(blockIdx.x / a.tilesX) * kFilterTileH - 2 * s;
  for (int k = (int)threadIdx.x; k < cells; k += (int)kFilterThreads) {  // k < cells: in the planes
    const long long gx = ox + k % RW, gy = oy + k / RW;
    int id = -1;
    if (gx >= 0 && gx < (long long)a.W && gy >= 0 && gy < (long long)a.H) {
      const size_t j = (size_t)gy * a.W + (size_t)gx;  // inside the frame: < W H
      const FilterGuide g = filter_load_guide(a.hits + j);
      id = g.id;
      float v[C];
      filter_load_value<C, kCount>(a.in, j, v);
      stage[1 * cells + k] = __float_as_uint(g.p.x);
      stage[2 * cells + k] = __float_as_uint(g.p.y);
      stage[3 * cells + k] = __float_as_uint(g.p.z);
      stage[4 * cells + k] = __float_as_uint(g.n.x);
      stage[5 * cells + k] = __float_as_uint(g.n.y);
      stage[6 * cells + k] = __float_as_uint(g.n.z);
#pragma unroll
      for (int q = 0; q < C; ++q) stage[(7 + q) * cells + k] = __float_as_uint(v[q]);
    }
    stage[k] = (unsigned)id;  // a cell outside the frame: only its id is ever read
  }
  __syncthreads();
  if (!inside) return;
  // the lane's own cell: the tile starts 2s cells into the stage
  const int k0 = ((int)(threadIdx.x / kFilterTileW) + 2 * s) * RW +
                 (int)(threadIdx.x % kFilterTileW) + 2 * s;
  const bool wantN = (a.t.flags & RTG_FILTER_NORMAL) != 0, wantP = (a.t.flags & RTG_FILTER_PLANE) != 0;
  FilterGuide c;
  c.id = (int)stage[k0];
  c.p = v3(__uint_as_float(stage[1 * cells + k0]), __uint_as_float(stage[2 * cells + k0]),
           __uint_as_float(stage[3 * cells + k0]));
  c.n = v3(__uint_as_float(stage[4 * cells + k0]), __uint_as_float(stage[5 * cells + k0]),
           __uint_as_float(stage[6 * cells + k0]));
  float in[C], out[C];
#pragma unroll
  for (int q = 0; q < C; ++q) in[q] = __uint_as_float(stage[(7 + q) * cells + k0]);
  if (c.id < 0) {
    filter_store_value<C>(a.out, i, in, a.last);
    return;
  }
  FilterSum<C> acc;
  filter_clear(acc);
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = k0 + dy * s * RW + dx * s;  // within 2s cells of the tile: in the stage
      FilterGuide g;
      g.id = (int)stage[k];
      if (!filter_admits(a.t, c.id, g.id)) continue;
      // (a term that is off reads none of its planes; filter_tap reads none of these zeros)
      g.p = g.n = v3(0.f, 0.f, 0.f);
      if (wantP)
        g.p = v3(__uint_as_float(stage[1 * cells + k]), __uint_as_float(stage[2 * cells + k]),
                 __uint_as_float(stage[3 * cells + k]));
      if (wantN)
        g.n = v3(__uint_as_float(stage[4 * cells + k]), __uint_as_float(stage[5 * cells + k]),
                 __uint_as_float(stage[6 * cells + k]));
      float v[C];
#pragma unroll
      for (int q = 0; q < C; ++q) v[q] = __uint_as_float(stage[(7 + q) * cells + k]);
      filter_tap<C>(a.t, c, g, v, filter_h(dy) * filter_h(dx), acc);
    }
  }
  filter_result<C>(acc, in, out);
  filter_store_value<C>(a.out, i, out, a.last);
}

// ---- host form ----

// Rows [y0, y1) of one pass over `in` (W H C floats) into `out`.
template <int C>
static void filter_host_rows(const rtg_hit* hits, unsigned W, unsigned H, unsigned step,
                             const FilterTerms& t, const float* in, unsigned* out, bool last,
                             size_t y0, size_t y1) {
  const long long s = step;
  for (size_t y = y0; y < y1; ++y) {
    for (size_t x = 0; x < W; ++x) {
      const size_t i = y * W + x;
      const FilterGuide c = filter_guide(hits + i);
      float res[C];
      for (int q = 0; q < C; ++q) res[q] = in[i * C + q];
      if (c.id >= 0) {
        FilterSum<C> acc;
        filter_clear(acc);
        for (int dy = -2; dy <= 2; ++dy) {
          for (int dx = -2; dx <= 2; ++dx) {
            const long long xq = (long long)x + dx * s, yq = (long long)y + dy * s;
            if (xq < 0 || xq >= (long long)W || yq < 0 || yq >= (long long)H) continue;
            const size_t j = (size_t)yq * W + (size_t)xq;
            const FilterGuide g = filter_guide(hits + j);
            if (!filter_admits(t, c.id, g.id)) continue;
            filter_tap<C>(t, c, g, in + j * C, filter_h(dy) * filter_h(dx), acc);
          }
        }
        filter_result<C>(acc, in + i * C, res);
      }
      for (int q = 0; q < C; ++q) {
        unsigned u;
        memcpy(&u, &res[q], 4);
        out[i * C + q] = last ? nan_bits(res[q]) : u;
      }
    }
  }
}

}  // namespace rtg

using namespace rtg;

// The frame and the parameters, in the order they are reported in; *n = W H.
static int check_filter_frame(const char* what, unsigned W, unsigned H, const rtg_filter_params* p,
                              size_t* n) {
  if (!p) {
    rtg_set_error("%s: null params", what);
    return RTG_ERR_INVALID;
  }
  if (W == 0 || H == 0) {
    rtg_set_error("%s: empty frame %u x %u", what, W, H);
    return RTG_ERR_INVALID;
  }
  const unsigned long long px = (unsigned long long)W * H;
  if (px > 0xFFFFFFFFull) {
    rtg_set_error("%s: %llu pixels (at most 2^32 - 1)", what, px);
    return RTG_ERR_INVALID;
  }
  if (p->passes < 1 || p->passes > RTG_FILTER_MAX_PASSES) {
    rtg_set_error("%s: %u passes outside [1, %d]", what, p->passes, RTG_FILTER_MAX_PASSES);
    return RTG_ERR_INVALID;
  }
  const int rc = check_filter_terms(what, p->normalLog2, p->kind, p->flags);
  if (rc) return rc;
  *n = (size_t)px;
  return RTG_OK;
}

static size_t filter_scratch_bytes(size_t n, const rtg_filter_params& p) {
  if (p.passes < 2) return 0;
  return (n * (size_t)filter_channels(p.kind) * sizeof(float) + 15) & ~(size_t)15;
}

// What the host and the device forms share.
static int check_filter(const char* what, const void* hits, unsigned W, unsigned H,
                        const rtg_filter_params* p, const void* src, const void* dst, size_t* n) {
  if (!hits || !src || !dst) {
    rtg_set_error("%s: null %s", what, !hits ? "hit buffer" : !src ? "source" : "destination");
    return RTG_ERR_INVALID;
  }
  const int rc = check_filter_frame(what, W, H, p, n);
  if (rc) return rc;
  if (filter_overlap(dst, *n * filter_channels(p->kind) * sizeof(float), src,
                     *n * filter_src_size(p->kind))) {
    rtg_set_error("%s: the destination overlaps the source", what);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// One pass on `stream`; the device is set.
template <int C, bool kCount>
static int launch_filter_pass(const FilterPass& a, unsigned blocks, bool tiled, hipStream_t stream) {
  if (tiled) {
    const size_t lds = filter_stage_bytes(a.step, C);
    if (lds > 48 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&filter_tiled_kernel<C, kCount>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((filter_tiled_kernel<C, kCount>), dim3(blocks), dim3(kFilterThreads), lds,
                       stream, a);
  } else {
    hipLaunchKernelGGL((filter_direct_kernel<C, kCount>), dim3(blocks), dim3(kFilterThreads), 0,
                       stream, a);
  }
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

extern "C" {

int rtg_filter_scratch(unsigned width, unsigned height, const rtg_filter_params* params,
                       size_t* bytes) {
  rtg_clear_error();
  if (!bytes) {
    rtg_set_error("filter_scratch: null size");
    return RTG_ERR_INVALID;
  }
  size_t n = 0;
  const int rc = check_filter_frame("filter_scratch", width, height, params, &n);
  if (rc) return rc;
  *bytes = filter_scratch_bytes(n, *params);
  return RTG_OK;
}

int rtg_filter_host(const rtg_hit* hits, unsigned width, unsigned height,
                    const rtg_filter_params* params, const void* src, void* dstHost,
                    int nthreads) {
  rtg_clear_error();
  size_t n = 0;
  const int rc = check_filter("filter", hits, width, height, params, src, dstHost, &n);
  if (rc) return rc;
  const rtg_filter_params p = *params;
  const FilterTerms t = {p.flags, p.normalLog2, p.planeScale};
  const size_t C = (size_t)filter_channels(p.kind);
  // the passes' images: the converted counts, and two to ping-pong between
  std::vector<float> first, bufs[2];
  const float* in = static_cast<const float*>(src);
  if (p.kind == RTG_FILTER_COUNT) {
    first.resize(n);
    for (size_t i = 0; i < n; ++i) first[i] = (float)static_cast<const unsigned short*>(src)[i];
    in = first.data();
  }
  for (unsigned i = 0; i < p.passes; ++i) {
    const bool last = i + 1 == p.passes;
    if (!last) bufs[i & 1].resize(n * C);
    unsigned* out = last ? static_cast<unsigned*>(dstHost)
                         : reinterpret_cast<unsigned*>(bufs[i & 1].data());
    host_bands(height, nthreads, [&](size_t y0, size_t y1) {
      if (C == 3) filter_host_rows<3>(hits, width, height, 1u << i, t, in, out, last, y0, y1);
      else filter_host_rows<1>(hits, width, height, 1u << i, t, in, out, last, y0, y1);
    });
    in = reinterpret_cast<const float*>(out);
  }
  return RTG_OK;
}

int rtg_filter_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                      unsigned height, const rtg_filter_params* params, const void* srcDevice,
                      void* dstDevice, void* scratchDevice, size_t scratchBytes, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("filter: no context");
    return RTG_ERR_INVALID;
  }
  size_t n = 0;
  int rc = check_filter("filter", hitsDevice, width, height, params, srcDevice, dstDevice, &n);
  if (rc) return rc;
  const rtg_filter_params p = *params;
  if ((uintptr_t)hitsDevice & 15) {
    rtg_set_error("filter: hit buffer not 16-byte aligned");
    return RTG_ERR_INVALID;
  }
  const size_t need = filter_scratch_bytes(n, p);
  if (need) {
    if (!scratchDevice) {
      rtg_set_error("filter: null scratch (%zu bytes needed)", need);
      return RTG_ERR_INVALID;
    }
    if (scratchBytes < need || ((uintptr_t)scratchDevice & 15)) {
      rtg_set_error("filter: scratch of %zu bytes at %p (%zu needed, 16-byte aligned)",
                    scratchBytes, scratchDevice, need);
      return RTG_ERR_INVALID;
    }
    const size_t dstBytes = n * (size_t)filter_channels(p.kind) * sizeof(float);
    if (filter_overlap(dstDevice, dstBytes, scratchDevice, need)) {
      rtg_set_error("filter: the destination overlaps the scratch");
      return RTG_ERR_INVALID;
    }
    if (filter_overlap(srcDevice, n * filter_src_size(p.kind), scratchDevice, need)) {
      rtg_set_error("filter: the source overlaps the scratch");
      return RTG_ERR_INVALID;
    }
  }
  const size_t tilesX = ((size_t)width + kFilterTileW - 1) / kFilterTileW;
  const size_t tiles = tilesX * (((size_t)height + kFilterTileH - 1) / kFilterTileH);
  if (tiles > 0x7FFFFFFFu) {  // (with 32 x 8 tiles no frame of 2^32 - 1 pixels gets here)
    rtg_set_error("filter: frame too large (%zu workgroups)", tiles);
    return RTG_ERR_INVALID;
  }
  int force = 0;  // 1: tiled wherever it fits, 2: direct
  if (const char* v = getenv("RTG_FILTER_FORM")) {  // A/B knob (performance only)
    force = !strcmp(v, "tiled") ? 1 : !strcmp(v, "direct") ? 2 : 0;
  }
  HIP_TRY(hipSetDevice(device));
  const int C = filter_channels(p.kind);
  FilterPass a{};
  a.hits = hitsDevice;
  a.W = width;
  a.H = height;
  a.tilesX = (unsigned)tilesX;
  a.t = {p.flags, p.normalLog2, p.planeScale};
  a.in = srcDevice;
  for (unsigned i = 0; i < p.passes; ++i) {
    a.step = 1u << i;
    a.last = i + 1 == p.passes;
    a.out = static_cast<unsigned*>((p.passes - 1 - i) % 2 == 0 ? dstDevice : scratchDevice);
    const bool fits = filter_stage_bytes(a.step, C) <= kFilterLdsMax;
    const bool tiled = fits && force != 2 && (force == 1 || a.step <= kFilterTiledMaxStep);
    const hipStream_t st = (hipStream_t)stream;
    if (C == 3) rc = launch_filter_pass<3, false>(a, (unsigned)tiles, tiled, st);
    else if (i == 0 && p.kind == RTG_FILTER_COUNT) rc = launch_filter_pass<1, true>(a, (unsigned)tiles, tiled, st);
    else rc = launch_filter_pass<1, false>(a, (unsigned)tiles, tiled, st);
    if (rc) return rc;
    a.in = a.out;
  }
  return RTG_OK;
}

int rtg_filter(int device, const rtg_hit* hits, unsigned width, unsigned height,
               const rtg_filter_params* params, const void* src, void* dstHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  size_t n = 0;
  int rc = check_filter("filter", hits, width, height, params, src, dstHost, &n);
  if (rc) return rc;
  const size_t scratchBytes = filter_scratch_bytes(n, *params);
  return one_shot("filter", device, nullptr,
                  {{n * sizeof(rtg_hit), hits, nullptr},
                   {n * filter_src_size(params->kind), src, nullptr},
                   {n * (size_t)filter_channels(params->kind) * sizeof(float), nullptr, dstHost},
                   {scratchBytes, nullptr, nullptr}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_filter_device(ctx, (const rtg_hit*)d[0], width, height, params,
                                             d[1], d[2], d[3], scratchBytes, nullptr);
                  });
}

}  // extern "C"
