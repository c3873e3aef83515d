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
// Two shapes, workgroups of 256 lanes in a one-dimensional grid either way:
//   row:  a wave is 64 pixels of a row, a workgroup 64 x 4;
//   tile: a wave is an 8 x 8 tile as in the camera kernels, a workgroup 32 x 8.
// The row shape is the default: it was 7 to 16 % faster on every measured frame
// (DESIGN.md §25), its streams being whole cache lines where the tile's are
// eight short runs.  env RTG_ACCUM_FORM=tile|row forces one (a performance
// knob: the words are the same either way).
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
#include <stdlib.h>
#include <string.h>

#include "rtg.h"
#include "rtg_accumulate.h"
#include "rtg_entry.h"

static_assert(sizeof(rtg_accumulate_params) == 20, "rtg_accumulate_params is 20 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, id) == 0 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");

namespace rtg {

constexpr unsigned kAccumThreads = 256;
// The wave shape taken by default.
constexpr bool kAccumDefaultTile = false;

// A workgroup's footprint in pixels for a wave shape.
constexpr unsigned accum_group_w(bool tile) { return tile ? 32 : 64; }
constexpr unsigned accum_group_h(bool tile) { return tile ? 8 : 4; }

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

// (filter_load_guide's loads; the entry point checks the alignment)
struct AccumLoadGuide {
  __device__ __forceinline__ FilterGuide operator()(const rtg_hit* h) const {
    const uint4* r = reinterpret_cast<const uint4*>(h);
    const uint4 a = r[0], b = r[1];
    FilterGuide g;
    g.id = (int)a.x;
    g.p = v3(__uint_as_float(a.z), __uint_as_float(a.w), __uint_as_float(b.x));
    g.n = v3(__uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w));
    return g;
  }
};

struct AccumHostGuide {
  FilterGuide operator()(const rtg_hit* h) const { return filter_guide(h); }
};

template <int C, bool kCount, bool kM2, bool kTile>
__global__ __launch_bounds__(kAccumThreads) void accum_kernel(const AccumArgs k) {
  const unsigned wave = threadIdx.x / 64, l = threadIdx.x % 64;
  const size_t gx = blockIdx.x % k.groupsX, gy = blockIdx.x / k.groupsX;
  const size_t x = gx * accum_group_w(kTile) + (kTile ? wave * 8 + l % 8 : l);
  const size_t y = gy * accum_group_h(kTile) + (kTile ? l / 8 : wave);
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

static int accum_channels(unsigned kind) { return kind == RTG_FILTER_RGB ? 3 : 1; }
static size_t accum_src_size(unsigned kind) {
  return kind == RTG_FILTER_RGB ? sizeof(rtg_vec)
                                : kind == RTG_FILTER_GRAY ? sizeof(float) : sizeof(unsigned short);
}

// Byte ranges [a, a + na) and [b, b + nb), addresses as numbers.
static bool accum_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && na && nb && x < y + nb && y < x + na;
}

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
  if (p->normalLog2 > 8) {
    rtg_set_error("accumulate: normalLog2 %u outside [0, 8]", p->normalLog2);
    return RTG_ERR_INVALID;
  }
  if (p->kind > RTG_FILTER_COUNT) {
    rtg_set_error("accumulate: kind %u (0: RGB, 1: GRAY, 2: COUNT)", p->kind);
    return RTG_ERR_INVALID;
  }
  const unsigned known =
      RTG_ACCUM_SAME_ID | RTG_ACCUM_NORMAL | RTG_ACCUM_PLANE | RTG_ACCUM_SKIP_NONFINITE;
  if (p->flags & ~known) {
    rtg_set_error("accumulate: unknown flags 0x%x", p->flags & ~known);
    return RTG_ERR_INVALID;
  }
  if (p->maxHistory < 1 || p->maxHistory > 65535) {
    rtg_set_error("accumulate: maxHistory %u outside [1, 65535]", p->maxHistory);
    return RTG_ERR_INVALID;
  }
  const size_t n = (size_t)W * H;  // <= 2^48
  const size_t vals = n * (size_t)accum_channels(p->kind) * sizeof(float);
  const struct { const char* name; const void* at; size_t bytes; bool out; } r[] = {
      {"outAcc", outAcc, vals, true},
      {"outLen", outLen, n * sizeof(unsigned short), true},
      {"outM2", outM2, vals, true},
      {"hits", hits, n * sizeof(rtg_hit), false},
      {"src", src, n * accum_src_size(p->kind), false},
      {"prevHits", prevHits, n * sizeof(rtg_hit), false},
      {"prevAcc", prevAcc, vals, false},
      {"prevLen", prevLen, n * sizeof(unsigned short), false},
      {"prevM2", reset ? nullptr : prevM2, vals, false},
  };
  for (size_t i = 0; i < 3; ++i)  // each output against every later range
    for (size_t j = i + 1; j < sizeof r / sizeof r[0]; ++j)
      if (accum_overlap(r[i].at, r[i].bytes, r[j].at, r[j].bytes)) {
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

template <bool kTile>
static void launch_accum(const AccumArgs& k, unsigned kind, unsigned blocks, hipStream_t st) {
  const dim3 g(blocks), b(kAccumThreads);
  const bool m2 = k.outM2 != nullptr;
  if (kind == RTG_FILTER_RGB) {
    if (m2) hipLaunchKernelGGL((accum_kernel<3, false, true, kTile>), g, b, 0, st, k);
    else hipLaunchKernelGGL((accum_kernel<3, false, false, kTile>), g, b, 0, st, k);
  } else if (kind == RTG_FILTER_COUNT) {
    if (m2) hipLaunchKernelGGL((accum_kernel<1, true, true, kTile>), g, b, 0, st, k);
    else hipLaunchKernelGGL((accum_kernel<1, true, false, kTile>), g, b, 0, st, k);
  } else {
    if (m2) hipLaunchKernelGGL((accum_kernel<1, false, true, kTile>), g, b, 0, st, k);
    else hipLaunchKernelGGL((accum_kernel<1, false, false, kTile>), g, b, 0, st, k);
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
  bool tile = kAccumDefaultTile;
  if (const char* v = getenv("RTG_ACCUM_FORM")) {  // A/B knob (performance only)
    tile = !strcmp(v, "tile") ? true : !strcmp(v, "row") ? false : tile;
  }
  const size_t groupsX = ((size_t)width + accum_group_w(tile) - 1) / accum_group_w(tile);
  const size_t groups = groupsX * (((size_t)height + accum_group_h(tile) - 1) / accum_group_h(tile));
  if (groups > 0x7FFFFFFFu) {
    rtg_set_error("accumulate: frame too large (%zu workgroups)", groups);
    return RTG_ERR_INVALID;
  }
  k.groupsX = (unsigned)groupsX;
  HIP_TRY(hipSetDevice(device));
  if (tile) launch_accum<true>(k, params->kind, (unsigned)groups, (hipStream_t)stream);
  else launch_accum<false>(k, params->kind, (unsigned)groups, (hipStream_t)stream);
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
  const size_t vals = n * (size_t)accum_channels(params->kind) * sizeof(float);
  // one allocation, each part 16-byte aligned: the inputs up, the outputs down
  struct Part { const void* from; void* to; size_t bytes, at; };
  Part parts[] = {
      {hits, nullptr, n * sizeof(rtg_hit), 0},
      {src, nullptr, n * accum_src_size(params->kind), 0},
      {prevHits, nullptr, reset ? 0 : n * sizeof(rtg_hit), 0},
      {prevAcc, nullptr, reset ? 0 : vals, 0},
      {prevLen, nullptr, reset ? 0 : n * sizeof(unsigned short), 0},
      {prevM2, nullptr, reset || !prevM2 ? 0 : vals, 0},
      {nullptr, outAcc, vals, 0},
      {nullptr, outLen, n * sizeof(unsigned short), 0},
      {nullptr, outM2, outM2 ? vals : 0, 0},
  };
  size_t total = 0;
  for (Part& p : parts) {
    p.at = total;
    total = (total + p.bytes + 15) & ~(size_t)15;
  }
  rtg_context* ctx = nullptr;
  rc = rtg_context_create(device, &ctx);
  if (rc) return rc;
  unsigned char* d = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&d, total) != hipSuccess) {
    rtg_set_error("accumulate: hipMalloc(%zu) failed", total);
    rc = RTG_ERR_NOMEM;
  }
  for (const Part& p : parts)
    if (!rc && p.from && p.bytes &&
        hipMemcpy(d + p.at, p.from, p.bytes, hipMemcpyHostToDevice) != hipSuccess) {
      rtg_set_error("accumulate: upload of %zu bytes failed", p.bytes);
      rc = RTG_ERR_HIP;
    }
  auto at = [&](int i) -> void* { return parts[i].bytes ? d + parts[i].at : nullptr; };
  if (!rc)
    rc = rtg_accumulate_device(ctx, (const rtg_hit*)at(0), width, height, params, at(1), prevCam,
                               zoom, (const rtg_hit*)at(2), (const float*)at(3),
                               (const unsigned short*)at(4), (const float*)at(5), (float*)at(6),
                               (unsigned short*)at(7), (float*)at(8), nullptr);
  for (const Part& p : parts)
    if (!rc && p.to && p.bytes) {
      const hipError_t e = hipMemcpy(p.to, d + p.at, p.bytes, hipMemcpyDeviceToHost);
      if (e != hipSuccess) {
        rtg_set_error("accumulate: kernel/readback failed: %s", hipGetErrorString(e));
        rc = RTG_ERR_HIP;
      }
    }
  (void)hipFree(d);
  rtg_context_destroy(ctx);
  return rc;
}

}  // extern "C"
