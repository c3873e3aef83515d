// rtg_fold.hip — views folded into per-group coefficients (rtg_views_fold*,
// rtg.h): a weighted sum of groups of frames in a DEFINED float order, so an
// SH probe is the same words on the host and on every GPU.
//
// The definition is rtg.h's: terms w * pix, a six-step tree over the 64 lanes
// of an 8 x 8 tile, then a sequential sum over the group's tiles.  Stage 1
// (fold_frames_kernel here, views_fold_kernel in rtg_camera_kernels.h for the
// fused call; both end in fold_tile, rtg_fold.h) leaves 3K + 1 words per tile
// in the caller's scratch; stage 2 (fold_groups_kernel) adds a group's tiles
// in order and writes the coefficients.  fold_host_group restates the whole
// in plain loops: the yardstick.
//
// The launcher of the fused call, the host render + fold and the one-shot form
// are in rtg_camera.hip, next to rtg_render_views*.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include "rtg_fold.h"

#include <vector>

#include "rtg_entry.h"

static_assert(sizeof(rtg_vec) == 12, "12 B per pixel");

namespace rtg {

// ---- stage 1 over frames in memory ----

// One wave per tile of one view, the views kernel's grid: workgroup b is tile
// b % tilesPerView of view b / tilesPerView, and the grid is exactly nViews *
// tilesPerView workgroups.  No lane leaves: the tree sum reads all 64.
__global__ __launch_bounds__(64) void fold_frames_kernel(const rtg_vec* __restrict__ frames,
                                                         unsigned W, unsigned H, unsigned tilesX,
                                                         unsigned tilesPerView,
                                                         const FoldArgs fa) {
  const unsigned view = blockIdx.x / tilesPerView;
  const unsigned tile = blockIdx.x - view * tilesPerView;
  const size_t px = (size_t)(tile % tilesX) * kFoldTileW + threadIdx.x % kFoldTileW;
  const size_t py = (size_t)(tile / tilesX) * kFoldTileH + threadIdx.x / kFoldTileW;
  const bool live = px < W && py < H;
  float r = 0.f, g = 0.f, b = 0.f;
  const size_t e = py * W + px;  // the texel inside its view (live lanes)
  if (live) {
    const float* p = reinterpret_cast<const float*>(frames + ((size_t)view * W * H + e));
    r = p[0];  // view < nViews, e < W * H: 12 B of the frames
    g = p[1];
    b = p[2];
  }
  const float* w = fa.weights + ((size_t)(view % fa.G) * W * H + e) * fa.K;  // read when live
  fold_tile(live, r, g, b, w, fa.K, fa.skip != 0,
            fa.partials + (size_t)blockIdx.x * fold_tile_words(fa.K));
}

// ---- stage 2 ----

// Lane i < n = nGroups * (3K + 1): group i / (3K + 1), word j = i % (3K + 1)
// of it.  j < 3K: coefficient word 3k + q, the group's G * tilesPerView
// partials added from +0.f in tile order; j == 3K: the skip count.
__global__ __launch_bounds__(256) void fold_groups_kernel(const unsigned* __restrict__ partials,
                                                          size_t n, unsigned tilesPerGroup,
                                                          unsigned K, float* __restrict__ out,
                                                          unsigned* __restrict__ skipped) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned words = fold_tile_words(K);
  const size_t g = i / words;
  const unsigned j = (unsigned)(i - g * words);
  const unsigned* p = partials + g * tilesPerGroup * words + j;  // g < nGroups: its tiles
  if (j < 3 * K) {
    // the adds wait for each other, the loads need not: kBatch partials are
    // read before they are added in tile order (one load per add in a plain
    // loop: 96 memory latencies in a row for a cube of 32 x 32 faces)
    constexpr unsigned kBatch = 16;
    float acc = 0.f;
    for (unsigned t0 = 0; t0 < tilesPerGroup; t0 += kBatch) {
      float v[kBatch];
#pragma unroll
      for (unsigned u = 0; u < kBatch; ++u)
        v[u] = t0 + u < tilesPerGroup ? __uint_as_float(p[(size_t)(t0 + u) * words]) : 0.f;
#pragma unroll
      for (unsigned u = 0; u < kBatch; ++u)
        if (t0 + u < tilesPerGroup) acc = acc + v[u];
    }
    out[g * 3 * K + j] = __uint_as_float(nan_bits(acc));  // word j of the group's K rtg_vec
  } else {
    unsigned c = 0;
    for (unsigned t = 0; t < tilesPerGroup; ++t) c += p[(size_t)t * words];
    if (skipped) skipped[g] = c;
  }
}

// ---- the host restatement ----

// Group g of the definition in plain loops.
static void fold_host_group(const rtg_vec* frames, size_t g, unsigned W, unsigned H, unsigned G,
                            unsigned K, bool skipFlag, const float* weights, rtg_vec* out,
                            unsigned* skipped) {
  const size_t tx = ((size_t)W + kFoldTileW - 1) / kFoldTileW;
  const size_t ty = ((size_t)H + kFoldTileH - 1) / kFoldTileH;
  float acc[3 * RTG_FOLD_MAX_WEIGHTS];
  for (unsigned j = 0; j < 3 * K; ++j) acc[j] = 0.f;
  unsigned count = 0;
  for (unsigned f = 0; f < G; ++f) {
    const float* view = reinterpret_cast<const float*>(frames + (g * G + f) * W * H);
    for (size_t tile = 0; tile < tx * ty; ++tile) {
      const float* pix[64];  // the lane's pixel; null: +0.f (outside the frame, or skipped)
      const float* w[64];
      for (unsigned l = 0; l < 64; ++l) {
        const size_t px = (tile % tx) * kFoldTileW + l % kFoldTileW;
        const size_t py = (tile / tx) * kFoldTileH + l / kFoldTileW;
        pix[l] = nullptr;
        w[l] = nullptr;
        if (px >= W || py >= H) continue;
        const size_t e = py * W + px;
        const float* p = view + e * 3;
        if (skipFlag && (fold_nonfinite(p[0]) || fold_nonfinite(p[1]) || fold_nonfinite(p[2]))) {
          ++count;
          continue;
        }
        pix[l] = p;
        w[l] = weights + ((size_t)f * W * H + e) * K;
      }
      for (unsigned k = 0; k < K; ++k) {
        for (unsigned q = 0; q < 3; ++q) {
          float v[64];
          for (unsigned l = 0; l < 64; ++l) v[l] = pix[l] ? w[l][k] * pix[l][q] : 0.f;
          for (unsigned s = 1; s < 64; s *= 2)
            for (unsigned l = 0; l < 64; l += 2 * s) v[l] = v[l] + v[l + s];
          acc[3 * k + q] = acc[3 * k + q] + v[0];
        }
      }
    }
  }
  unsigned words[3 * RTG_FOLD_MAX_WEIGHTS];
  for (unsigned j = 0; j < 3 * K; ++j) words[j] = nan_bits(acc[j]);
  memcpy(out + g * K, words, (size_t)3 * K * sizeof(unsigned));
  if (skipped) skipped[g] = count;
}

// Tiles of a W x H view (W, H > 0): never more than 2^58.
static size_t fold_tiles(unsigned W, unsigned H, unsigned* tilesX) {
  const size_t tx = ((size_t)W + kFoldTileW - 1) / kFoldTileW;
  const size_t ty = ((size_t)H + kFoldTileH - 1) / kFoldTileH;
  *tilesX = (unsigned)tx;
  return tx * ty;
}

int check_fold(const char* what, size_t nViews, unsigned W, unsigned H,
               const rtg_fold_params* params, const void* weights, const void* out,
               bool needScratch, const void* scratch, size_t scratchBytes, unsigned* tilesX,
               unsigned* tilesPerView) {
  if (!params || !weights || !out) {
    rtg_set_error("%s: null %s", what, !params ? "params" : !weights ? "weight table" : "output");
    return RTG_ERR_INVALID;
  }
  const unsigned G = params->viewsPerGroup, K = params->weights;
  if (G == 0 || nViews % G) {
    rtg_set_error("%s: %zu views are not a multiple of viewsPerGroup %u", what, nViews, G);
    return RTG_ERR_INVALID;
  }
  if (K < 1 || K > RTG_FOLD_MAX_WEIGHTS) {
    rtg_set_error("%s: weights %u outside [1, %d]", what, K, RTG_FOLD_MAX_WEIGHTS);
    return RTG_ERR_INVALID;
  }
  if (params->flags & ~(unsigned)RTG_FOLD_SKIP_NONFINITE) {
    rtg_set_error("%s: unknown flag 0x%x", what, params->flags);
    return RTG_ERR_INVALID;
  }
  // W * H < 2^64 always; the table's G * W * H * K floats may not be
  if (G > SIZE_MAX / sizeof(float) / K / ((size_t)W * H)) {
    rtg_set_error("%s: weight table too large (%u views of %u x %u texels, %u weights)", what, G,
                  W, H, K);
    return RTG_ERR_INVALID;
  }
  const size_t per = fold_tiles(W, H, tilesX);
  const size_t tileBytes = fold_tile_words(K) * sizeof(unsigned);
  if (nViews && (per > 0x7FFFFFFFu / nViews ||
                 nViews * per > SIZE_MAX / tileBytes)) {  // (the first holds on every caller's path)
    rtg_set_error("%s: scratch too large (%zu views of %zu tiles)", what, nViews, per);
    return RTG_ERR_INVALID;
  }
  *tilesPerView = (unsigned)per;
  if (!needScratch || nViews == 0) return RTG_OK;
  const size_t need = nViews * per * tileBytes;
  if (!scratch) {
    rtg_set_error("%s: null scratch", what);
    return RTG_ERR_INVALID;
  }
  if ((uintptr_t)scratch % 16) {
    rtg_set_error("%s: scratch not 16-byte aligned", what);
    return RTG_ERR_INVALID;
  }
  if (scratchBytes < need) {
    rtg_set_error("%s: scratch of %zu bytes, %zu needed", what, scratchBytes, need);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

int launch_fold_stage2(const void* scratch, size_t nViews, unsigned tilesPerView,
                       const rtg_fold_params& p, rtg_vec* out, unsigned* skipped,
                       hipStream_t stream) {
  // nViews * tilesPerView <= 2^31-1 (check_fold), so neither product overflows
  const size_t n = nViews / p.viewsPerGroup * fold_tile_words(p.weights);
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(fold_groups_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
                     static_cast<const unsigned*>(scratch), n, p.viewsPerGroup * tilesPerView,
                     p.weights, reinterpret_cast<float*>(out), skipped);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

}  // namespace rtg

using namespace rtg;

// What the fold-only forms check before check_fold: the frames and their size,
// as rtg_render_views* does (its messages).
static int check_fold_frames(const void* frames, size_t nViews, unsigned W, unsigned H) {
  if (nViews && !frames) {
    rtg_set_error("views_fold: null frames");
    return RTG_ERR_INVALID;
  }
  if (W == 0 || H == 0) {
    rtg_set_error("empty frame %ux%u", W, H);
    return RTG_ERR_INVALID;
  }
  unsigned tilesX;
  const size_t per = fold_tiles(W, H, &tilesX);
  if (nViews && per > 0x7FFFFFFFu / nViews) {
    rtg_set_error("views_fold: batch too large (more than 2^31-1 workgroups)");
    return RTG_ERR_INVALID;
  }
  if (nViews > SIZE_MAX / sizeof(rtg_vec) / ((size_t)W * H)) {
    rtg_set_error("views_fold: batch too large (%zu views of %u x %u pixels)", nViews, W, H);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

extern "C" {

int rtg_views_fold_scratch(size_t nViews, unsigned width, unsigned height, unsigned weights,
                           size_t* bytes) {
  rtg_clear_error();
  if (!bytes) {
    rtg_set_error("views_fold_scratch: null pointer");
    return RTG_ERR_INVALID;
  }
  int dummy = 0;  // any non-null table and output: only the sizes are looked at
  const rtg_fold_params p = {1, weights, 0};
  unsigned tilesX = 0, tilesPerView = 0;
  int rc = check_fold_frames(&dummy, nViews, width, height);
  if (!rc)
    rc = check_fold("views_fold_scratch", nViews, width, height, &p, &dummy, &dummy, false,
                    nullptr, 0, &tilesX, &tilesPerView);
  if (rc) return rc;
  *bytes = nViews * tilesPerView * fold_tile_words(weights) * sizeof(unsigned);
  return RTG_OK;
}

int rtg_views_fold_host(const rtg_vec* frames, size_t nViews, unsigned width, unsigned height,
                        const rtg_fold_params* params, const float* weights, rtg_vec* out,
                        unsigned* skipped, int nthreads) {
  rtg_clear_error();
  unsigned tilesX = 0, tilesPerView = 0;
  int rc = check_fold_frames(frames, nViews, width, height);
  if (!rc)
    rc = check_fold("views_fold", nViews, width, height, params, weights, out, false, nullptr, 0,
                    &tilesX, &tilesPerView);
  if (rc) return rc;
  if (nViews == 0) return RTG_OK;
  const bool skipFlag = (params->flags & RTG_FOLD_SKIP_NONFINITE) != 0;
  // whole groups per thread: the result does not depend on nthreads
  host_bands(nViews / params->viewsPerGroup, nthreads, [&](size_t g0, size_t g1) {
    for (size_t g = g0; g < g1; ++g)
      fold_host_group(frames, g, width, height, params->viewsPerGroup, params->weights, skipFlag,
                      weights, out, skipped);
  });
  return RTG_OK;
}

int rtg_views_fold_device(rtg_context* ctx, const rtg_vec* framesDevice, size_t nViews,
                          unsigned width, unsigned height, const rtg_fold_params* params,
                          const float* weightsDevice, rtg_vec* outDevice, unsigned* skippedDevice,
                          void* scratchDevice, size_t scratchBytes, void* stream) {
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("views_fold: no context");
    return RTG_ERR_INVALID;
  }
  unsigned tilesX = 0, tilesPerView = 0;
  int rc = check_fold_frames(framesDevice, nViews, width, height);
  if (!rc)
    rc = check_fold("views_fold", nViews, width, height, params, weightsDevice, outDevice, true,
                    scratchDevice, scratchBytes, &tilesX, &tilesPerView);
  if (rc) return rc;
  if (nViews == 0) return RTG_OK;
  DeviceGuard deviceGuard;  // (after the checks: no GPU call before them)
  HIP_TRY(hipSetDevice(device));
  const FoldArgs fa = {weightsDevice, static_cast<unsigned*>(scratchDevice), params->weights,
                       params->viewsPerGroup, params->flags & RTG_FOLD_SKIP_NONFINITE};
  hipLaunchKernelGGL(fold_frames_kernel, dim3((unsigned)(nViews * tilesPerView)), dim3(64), 0,
                     (hipStream_t)stream, framesDevice, width, height, tilesX, tilesPerView, fa);
  HIP_TRY(hipGetLastError());
  return launch_fold_stage2(scratchDevice, nViews, tilesPerView, *params, outDevice,
                            skippedDevice, (hipStream_t)stream);
}

}  // extern "C"
