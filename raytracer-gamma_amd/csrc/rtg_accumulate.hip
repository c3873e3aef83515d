// rtg_accumulate.hip — temporal accumulation by reprojection of librtg.so
// (rtg_accumulate*, rtg.h): the current frame's signal and records and the
// previous frame's state and pose in, the blended state out.
//
// accum_kernel: one lane per pixel, one launch per call.  A lane reads its own
// record as two 16-byte loads and its value, projects its point into the
// previous pose and gathers up to four taps of the previous state: a record
// (two 16-byte loads), a length and the value each.  The per-pixel code is
// rtg_accumulate.h's, one definition for the kernel and the host loops below.
// Pose and parameters are kernel arguments; channels, the COUNT conversion and
// the second moments are compiled in, the flags are read at run time as the
// filter's pass kernels read them.
//
// The own-pixel traffic streams; the taps are gathers whose addresses follow
// the camera move.  Under a coherent move a wave's taps fall into a window of
// the previous frame about the size of the wave's own footprint plus one
// pixel, so the wave's shape decides how many cache lines the gathers touch.
// A wave is 64 pixels of a row, a workgroup of 256 lanes 64 x 4 pixels, in a
// one-dimensional grid: its streams are whole cache lines.  (An 8 x 8 tile per
// wave, as in the camera kernels, was 7 to 16 % slower on every measured
// frame, DESIGN.md §25, and is gone.)
//
// Bounds: a lane outside the frame leaves before any load or store; a tap is
// read only after the frame test on its integer position; a pixel index is
// < W H.  Every store is a vector store of the lane's own pixel.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rtg.h"
#include "rtg_accumulate.h"
#include "rtg_entry.h"

static_assert(sizeof(rtg_accumulate_params) == 20, "rtg_accumulate_params is 20 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, id) == 0 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");

namespace rtg {

constexpr unsigned kAccumThreads = 256;
// A workgroup's footprint in pixels: a wave per row.
constexpr unsigned kAccumGroupW = 64, kAccumGroupH = kAccumThreads / 64;

// What the kernel takes.
struct AccumArgs {
  const rtg_hit* hits;
  const void* src;  // W H values of the kind
  AccumPrev prev;
  unsigned* outAcc;         // W H C words
  unsigned short* outLen;   // W H
  unsigned* outM2;          // W H C words, kM2 only
  AccumTerms a;
  unsigned groupsX;
};

// (the entry point checks the alignment)
struct AccumLoadGuide {
  __device__ __forceinline__ FilterGuide operator()(const rtg_hit* h) const {
    return filter_load_guide(h);
  }
};

struct AccumHostGuide {
  FilterGuide operator()(const rtg_hit* h) const { return filter_guide(h); }
};

template <int C, bool kCount, bool kM2>
__global__ __launch_bounds__(kAccumThreads) void accum_kernel(const AccumArgs k) {
  const unsigned wave = threadIdx.x / 64, l = threadIdx.x % 64;
  const size_t gx = blockIdx.x % k.groupsX, gy = blockIdx.x / k.groupsX;
  const size_t x = gx * kAccumGroupW + l;
  const size_t y = gy * kAccumGroupH + wave;
  if (x >= k.a.W || y >= k.a.H) return;
  const size_t i = y * k.a.W + x;  // < W H
  const FilterGuide c = AccumLoadGuide()(k.hits + i);
  float cur[C], acc[C], m2[C];
  if constexpr (kCount) {
    cur[0] = (float)static_cast<const unsigned short*>(k.src)[i];
  } else {
#pragma unroll
    for (int q = 0; q < C; ++q) cur[q] = static_cast<const float*>(k.src)[i * C + q];
  }
  const unsigned len = accum_pixel<C, kM2>(k.a, k.prev, AccumLoadGuide(), c, cur, acc, m2);
#pragma unroll
  for (int q = 0; q < C; ++q) k.outAcc[i * C + q] = nan_bits(acc[q]);
  if constexpr (kM2) {
#pragma unroll
    for (int q = 0; q < C; ++q) k.outM2[i * C + q] = nan_bits(m2[q]);
  }
  k.outLen[i] = (unsigned short)len;
}

// Rows [y0, y1) on the host.
template <int C, bool kM2>
static void accum_host_rows(const AccumArgs& k, unsigned kind, size_t y0, size_t y1) {
  for (size_t y = y0; y < y1; ++y) {
    for (size_t x = 0; x < k.a.W; ++x) {
      const size_t i = y * k.a.W + x;
      const FilterGuide c = filter_guide(k.hits + i);
      float cur[C], acc[C], m2[C];
      if (kind == RTG_FILTER_COUNT) cur[0] = (float)static_cast<const unsigned short*>(k.src)[i];
      else for (int q = 0; q < C; ++q) cur[q] = static_cast<const float*>(k.src)[i * C + q];
      const unsigned len = accum_pixel<C, kM2>(k.a, k.prev, AccumHostGuide(), c, cur, acc, m2);
      for (int q = 0; q < C; ++q) k.outAcc[i * C + q] = nan_bits(acc[q]);
      if (kM2) for (int q = 0; q < C; ++q) k.outM2[i * C + q] = nan_bits(m2[q]);
      k.outLen[i] = (unsigned short)len;
    }
  }
}

}  // namespace rtg

using namespace rtg;

// What the three forms share, in the order it is reported in; fills `k` but
// for its grid.
static int check_accumulate(const rtg_hit* hits, unsigned W, unsigned H,
                            const rtg_accumulate_params* p, const void* src,
                            const rtg_camera* prevCam, float zoom, const rtg_hit* prevHits,
                            const float* prevAcc, const unsigned short* prevLen,
                            const float* prevM2, float* outAcc, unsigned short* outLen,
                            float* outM2, AccumArgs* k) {
  if (!hits || !src || !p || !outAcc || !outLen) {
    rtg_set_error("accumulate: null %s", !hits ? "hit buffer" : !src ? "source" : !p ? "params"
                                         : !outAcc ? "outAcc" : "outLen");
    return RTG_ERR_INVALID;
  }
  const int nPrev = (prevHits != nullptr) + (prevAcc != nullptr) + (prevLen != nullptr);
  if (nPrev != 0 && nPrev != 3) {
    rtg_set_error("accumulate: prevHits, prevAcc and prevLen are all null or all non-null");
    return RTG_ERR_INVALID;
  }
  const bool reset = nPrev == 0;
  if (!reset && !prevCam) {
    rtg_set_error("accumulate: null previous pose");
    return RTG_ERR_INVALID;
  }
  if (!reset && outM2 && !prevM2) {
    rtg_set_error("accumulate: outM2 without prevM2");
    return RTG_ERR_INVALID;
  }
  if (!reset && prevM2 && !outM2) {
    rtg_set_error("accumulate: prevM2 without outM2");
    return RTG_ERR_INVALID;
  }
  if (W == 0 || H == 0) {
    rtg_set_error("accumulate: empty frame %u x %u", W, H);
    return RTG_ERR_INVALID;
  }
  if (W > (1u << 24) || H > (1u << 24)) {
    rtg_set_error("accumulate: frame %u x %u (at most 2^24 each way)", W, H);
    return RTG_ERR_INVALID;
  }
  const int rc = check_filter_terms("accumulate", p->normalLog2, p->kind, p->flags);
  if (rc) return rc;
  if (p->maxHistory < 1 || p->maxHistory > 65535) {
    rtg_set_error("accumulate: maxHistory %u outside [1, 65535]", p->maxHistory);
    return RTG_ERR_INVALID;
  }
  const size_t n = (size_t)W * H;  // <= 2^48
  const size_t vals = n * (size_t)filter_channels(p->kind) * sizeof(float);
  const struct { const char* name; const void* at; size_t bytes; bool out; } r[] = {
      {"outAcc", outAcc, vals, true},
      {"outLen", outLen, n * sizeof(unsigned short), true},
      {"outM2", outM2, vals, true},
      {"hits", hits, n * sizeof(rtg_hit), false},
      {"src", src, n * filter_src_size(p->kind), false},
      {"prevHits", prevHits, n * sizeof(rtg_hit), false},
      {"prevAcc", prevAcc, vals, false},
      {"prevLen", prevLen, n * sizeof(unsigned short), false},
      {"prevM2", reset ? nullptr : prevM2, vals, false},
  };
  for (size_t i = 0; i < 3; ++i)  // each output against every later range
    for (size_t j = i + 1; j < sizeof r / sizeof r[0]; ++j)
      if (filter_overlap(r[i].at, r[i].bytes, r[j].at, r[j].bytes)) {
        rtg_set_error("accumulate: %s overlaps %s", r[i].name, r[j].name);
        return RTG_ERR_INVALID;
      }
  *k = AccumArgs{};
  k->hits = hits;
  k->src = src;
  if (!reset) {
    k->prev.hits = prevHits;
    k->prev.acc = prevAcc;
    k->prev.len = prevLen;
    k->prev.m2 = prevM2;
    k->prev.frame = proj_frame(W, H, zoom);
    k->prev.pose = cam_pose(*prevCam);
  }
  k->outAcc = reinterpret_cast<unsigned*>(outAcc);
  k->outLen = outLen;
  k->outM2 = reinterpret_cast<unsigned*>(outM2);
  k->a.t = {p->flags, p->normalLog2, p->planeScale};
  k->a.maxHistory = p->maxHistory;
  k->a.W = W;
  k->a.H = H;
  return RTG_OK;
}

static void launch_accum(const AccumArgs& k, unsigned kind, unsigned blocks, hipStream_t st) {
  const dim3 g(blocks), b(kAccumThreads);
  const bool m2 = k.outM2 != nullptr;
  if (kind == RTG_FILTER_RGB) {
    if (m2) hipLaunchKernelGGL((accum_kernel<3, false, true>), g, b, 0, st, k);
    else hipLaunchKernelGGL((accum_kernel<3, false, false>), g, b, 0, st, k);
  } else if (kind == RTG_FILTER_COUNT) {
    if (m2) hipLaunchKernelGGL((accum_kernel<1, true, true>), g, b, 0, st, k);
    else hipLaunchKernelGGL((accum_kernel<1, true, false>), g, b, 0, st, k);
  } else {
    if (m2) hipLaunchKernelGGL((accum_kernel<1, false, true>), g, b, 0, st, k);
    else hipLaunchKernelGGL((accum_kernel<1, false, false>), g, b, 0, st, k);
  }
}

extern "C" {

int rtg_accumulate_host(const rtg_hit* hits, unsigned width, unsigned height,
                        const rtg_accumulate_params* params, const void* src,
                        const rtg_camera* prevCam, float zoom, const rtg_hit* prevHits,
                        const float* prevAcc, const unsigned short* prevLen, const float* prevM2,
                        float* outAcc, unsigned short* outLen, float* outM2, int nthreads) {
  rtg_clear_error();
  AccumArgs k;
  const int rc = check_accumulate(hits, width, height, params, src, prevCam, zoom, prevHits,
                                  prevAcc, prevLen, prevM2, outAcc, outLen, outM2, &k);
  if (rc) return rc;
  const unsigned kind = params->kind;
  host_bands(height, nthreads, [&](size_t y0, size_t y1) {
    if (kind == RTG_FILTER_RGB) {
      if (outM2) accum_host_rows<3, true>(k, kind, y0, y1);
      else accum_host_rows<3, false>(k, kind, y0, y1);
    } else {
      if (outM2) accum_host_rows<1, true>(k, kind, y0, y1);
      else accum_host_rows<1, false>(k, kind, y0, y1);
    }
  });
  return RTG_OK;
}

int rtg_accumulate_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                          unsigned height, const rtg_accumulate_params* params,
                          const void* srcDevice, const rtg_camera* prevCam, float zoom,
                          const rtg_hit* prevHitsDevice, const float* prevAccDevice,
                          const unsigned short* prevLenDevice, const float* prevM2Device,
                          float* outAccDevice, unsigned short* outLenDevice, float* outM2Device,
                          void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("accumulate: no context");
    return RTG_ERR_INVALID;
  }
  AccumArgs k;
  const int rc = check_accumulate(hitsDevice, width, height, params, srcDevice, prevCam, zoom,
                                  prevHitsDevice, prevAccDevice, prevLenDevice, prevM2Device,
                                  outAccDevice, outLenDevice, outM2Device, &k);
  if (rc) return rc;
  if (((uintptr_t)hitsDevice & 15) || ((uintptr_t)prevHitsDevice & 15)) {
    rtg_set_error("accumulate: %s not 16-byte aligned",
                  ((uintptr_t)hitsDevice & 15) ? "hit buffer" : "previous hit buffer");
    return RTG_ERR_INVALID;
  }
  const size_t groupsX = ((size_t)width + kAccumGroupW - 1) / kAccumGroupW;
  const size_t groups = groupsX * (((size_t)height + kAccumGroupH - 1) / kAccumGroupH);
  if (groups > 0x7FFFFFFFu) {
    rtg_set_error("accumulate: frame too large (%zu workgroups)", groups);
    return RTG_ERR_INVALID;
  }
  k.groupsX = (unsigned)groupsX;
  HIP_TRY(hipSetDevice(device));
  launch_accum(k, params->kind, (unsigned)groups, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_accumulate(int device, const rtg_hit* hits, unsigned width, unsigned height,
                   const rtg_accumulate_params* params, const void* src,
                   const rtg_camera* prevCam, float zoom, const rtg_hit* prevHits,
                   const float* prevAcc, const unsigned short* prevLen, const float* prevM2,
                   float* outAcc, unsigned short* outLen, float* outM2) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  AccumArgs k;
  int rc = check_accumulate(hits, width, height, params, src, prevCam, zoom, prevHits, prevAcc,
                            prevLen, prevM2, outAcc, outLen, outM2, &k);
  if (rc) return rc;
  const bool reset = !prevHits;
  const size_t n = (size_t)width * height;
  const size_t vals = n * (size_t)filter_channels(params->kind) * sizeof(float);
  const size_t recs = n * sizeof(rtg_hit), lens = n * sizeof(unsigned short);
  return one_shot(
      "accumulate", device, nullptr,
      {{recs, hits, nullptr},
       {n * filter_src_size(params->kind), src, nullptr},
       {reset ? 0 : recs, prevHits, nullptr},
       {reset ? 0 : vals, prevAcc, nullptr},
       {reset ? 0 : lens, prevLen, nullptr},
       {reset || !prevM2 ? 0 : vals, prevM2, nullptr},
       {vals, nullptr, outAcc},
       {lens, nullptr, outLen},
       {outM2 ? vals : 0, nullptr, outM2}},
      [&](rtg_context* ctx, void* const* d) {
        return rtg_accumulate_device(ctx, (const rtg_hit*)d[0], width, height, params, d[1],
                                     prevCam, zoom, (const rtg_hit*)d[2], (const float*)d[3],
                                     (const unsigned short*)d[4], (const float*)d[5],
                                     (float*)d[6], (unsigned short*)d[7], (float*)d[8], nullptr);
      });
}

}  // extern "C"
