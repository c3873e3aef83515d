// rtg_fold.h — views folded into per-group coefficients (rtg_views_fold*,
// rtg_render_views_fold*, rtg.h): the tile epilogue, ONE device function for
// the stage-1 kernel over frames in memory (rtg_fold.hip) and the fused
// views kernel (views_fold_kernel, rtg_camera_kernels.h), and what the
// launchers of both share (rtg_fold.hip, rtg_camera.hip).
//
// Two stages.  Stage 1, one wave per 8 x 8 tile of one view (the views
// kernel's grid): the lanes' terms, the six-step tree sum, lane 0 stores the
// tile's 3K + 1 partial words.  Stage 2, one lane per (group, k, q): the
// group's tile partials added in tile order.  The partials are the caller's
// scratch; their layout (tile-major, word 3k + q of a tile, the skip count
// last) is not part of the contract.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"

namespace rtg {

// The tile of the definition; rtg_camera_kernels.h asserts it is the views
// kernel's.
constexpr unsigned kFoldTileW = 8, kFoldTileH = 8;

// What the stage-1 kernels take besides their frames or poses.
struct FoldArgs {
  const float* weights;  // G * W * H * K floats
  unsigned* partials;    // 3K + 1 words per workgroup
  unsigned K, G;
  unsigned skip;  // RTG_FOLD_SKIP_NONFINITE set
};

// Partial words of one tile.
constexpr unsigned fold_tile_words(unsigned K) { return 3 * K + 1; }

// A word whose exponent field is all ones: NaN or +-inf.
__host__ __device__ __forceinline__ bool fold_nonfinite(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  return (u & 0x7F800000u) == 0x7F800000u;
}

#if defined(__HIPCC__)
// Lane l's copy of lane l + n's value inside its row of 16 lanes (DPP
// row_shl:n, control word 0x100 + n), +0 past the row's end.
template <int kShift>
__device__ __forceinline__ float fold_row_shl(float v) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + kShift, 0xF, 0xF, true));
}

// The wave's sum in rtg.h's order, v[l] = v[l] + v[l + s] for every l that is
// a multiple of 2s, s = 1 .. 32; the same value in every lane.  Every lane of
// the wave is present.  Only the lanes the definition names need be right:
// steps 1 to 8 stay inside a row of 16, so each is one VALU add whose second
// operand comes through DPP, and lanes 0, 16, 32 and 48 then hold their rows'
// sums R0 .. R3; steps 16 and 32 are (R0 + R1) + (R2 + R3) over four
// v_readlane.  A __shfl_xor butterfly gives lane 0 the same bits, but each of
// its steps is a ds_bpermute through the LDS crossbar, 18 per k: with K = 9
// the fold of 1536 resident 32 x 32 frames took 0.086 ms that way and 0.063 ms
// this way.
__device__ __forceinline__ float fold_wave_sum(float v) {
  v = v + fold_row_shl<1>(v);
  v = v + fold_row_shl<2>(v);
  v = v + fold_row_shl<4>(v);
  v = v + fold_row_shl<8>(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (r0 + r1) + (r2 + r3);
}

// The tile epilogue.  EVERY lane of the wave calls it; a lane outside the
// frame (`live` false) holds +0.f and reads no weight.  `pix` is the lane's
// pixel, `w` its texel's K consecutive weights (live lanes only), `part` the
// tile's fold_tile_words(K) words, written by lane 0.  One k at a time: three
// sums in flight, not 3K.
__device__ __forceinline__ void fold_tile(bool live, float r, float g, float b,
                                          const float* __restrict__ w, unsigned K, bool skipFlag,
                                          unsigned* __restrict__ part) {
  const bool skipped =
      live && skipFlag && (fold_nonfinite(r) || fold_nonfinite(g) || fold_nonfinite(b));
  const bool on = live && !skipped;
  // the lane's K weights in one go, so that their latencies overlap (the sums
  // below wait for each other); a lane that holds +0.f reads none
  float wk[RTG_FOLD_MAX_WEIGHTS];
#pragma unroll
  for (unsigned k = 0; k < RTG_FOLD_MAX_WEIGHTS; ++k) wk[k] = 0.f;
  if (on) {
#pragma unroll
    for (unsigned k = 0; k < RTG_FOLD_MAX_WEIGHTS; ++k)
      if (k < K) wk[k] = w[k];  // live, k < K: inside the table
  }
#pragma unroll
  for (unsigned k = 0; k < RTG_FOLD_MAX_WEIGHTS; ++k) {
    if (k >= K) break;  // (wave-uniform)
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (on) {
      t0 = wk[k] * r;
      t1 = wk[k] * g;
      t2 = wk[k] * b;
    }
    t0 = fold_wave_sum(t0);
    t1 = fold_wave_sum(t1);
    t2 = fold_wave_sum(t2);
    if (threadIdx.x == 0) {  // words 3k .. 3k + 2 < 3K of the tile's
      part[3 * k + 0] = __float_as_uint(t0);
      part[3 * k + 1] = __float_as_uint(t1);
      part[3 * k + 2] = __float_as_uint(t2);
    }
  }
  const unsigned c = (unsigned)__popcll(__ballot(skipped));  // (a count: any order)
  if (threadIdx.x == 0) part[3 * K] = c;
}
#endif

// The fold's own argument checks, after the caller's checks of the frame (W,
// H > 0, the batch's size): `what: ...` and RTG_ERR_INVALID, or RTG_OK with
// the tiles of one view and the scratch bytes needed.  Host forms pass
// needScratch false.
int check_fold(const char* what, size_t nViews, unsigned W, unsigned H,
               const rtg_fold_params* params, const void* weights, const void* out,
               bool needScratch, const void* scratch, size_t scratchBytes, unsigned* tilesX,
               unsigned* tilesPerView);

// Stage 2 on `stream`: nGroups * (3K + 1) lanes over the partials stage 1 left
// in `scratch`.  The device is set.
int launch_fold_stage2(const void* scratch, size_t nViews, unsigned tilesPerView,
                       const rtg_fold_params& p, rtg_vec* out, unsigned* skipped,
                       hipStream_t stream);

}  // namespace rtg
