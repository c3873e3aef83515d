// rtg_upsample.hip — guided upsampling of a low-resolution signal of librtg.so
// (rtg_upsample*, rtg.h), its hole list, and the two index calls that act on
// such a list (rtg_hits_pick*, rtg_values_place*).
//
// upsample_kernel: one lane per full pixel.  A lane reads its own record as
// two 16-byte loads and gathers up to four taps of the low frame: a record
// (two 16-byte loads) and the value each.  The per-pixel code is
// rtg_upsample.h's, one definition for the kernel and the host loops below.
// Parameters are kernel arguments; channels, the COUNT conversion and whether
// there is a hole list are compiled in, the flags are read at run time as the
// filter's pass kernels read them.
//
// Pixels are numbered y W + x and a workgroup of 256 lanes takes 256
// consecutive numbers, a wave 64: for a width that is a multiple of 64 a wave
// is 64 pixels of a row, rtg_accumulate.hip's mapping, and otherwise a wave
// may end one row and begin the next.  The numbering is what the hole list is
// ordered by, so the workgroups' order is the list's order and the compaction
// needs no sort: the full records and dst stream in whole cache lines, and a
// wave's taps fall into 64 / f + 1 columns of two low rows.
//
// The list, three launches on the stream, none of which waits for another
// workgroup of its own launch:
//   1. upsample_kernel<.., true>: a wave's holes are a 64-bit ballot, stored to
//      the scratch; the workgroup's four counts meet in LDS and their sum goes
//      to the scratch.
//   2. upsample_scan_kernel: ONE workgroup turns the counts into exclusive
//      offsets in place, 1024 at a time with a running carry, and stores the
//      total to holeCount.
//   3. upsample_list_kernel: a lane whose ballot bit is set has the position
//      offset + (the bits before it in its workgroup) and stores its pixel
//      number there when that is below the capacity.  It reads 8 bytes per
//      wave, not the records again.
//
// Bounds: a lane outside the frame reads and stores nothing of the frame; a
// tap is read only after the frame test on its integer position; a pixel
// number is < W H; the scratch holds one count per workgroup and four masks;
// a list entry is stored only below holeCap.  Every store is a vector store.
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "rtg.h"
#include "rtg_entry.h"
#include "rtg_upsample.h"

static_assert(sizeof(rtg_upsample_params) == 20, "rtg_upsample_params is 20 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, id) == 0 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");

namespace rtg {

constexpr unsigned kUpThreads = 256, kUpWaves = kUpThreads / 64;
constexpr unsigned kUpScanThreads = 1024;

// What the kernels take.
struct UpArgs {
  const rtg_hit* hits;
  UpLow lo;
  unsigned* dst;  // W H C words
  UpTerms u;
  unsigned n;                 // W H <= 2^32 - 1
  unsigned* counts;           // one per workgroup (kHoles)
  unsigned long long* masks;  // kUpWaves per workgroup (kHoles)
};

// (the entry point checks the alignment)
struct UpLoadGuide {
  __device__ __forceinline__ FilterGuide operator()(const rtg_hit* h) const {
    return filter_load_guide(h);
  }
};

struct UpHostGuide {
  FilterGuide operator()(const rtg_hit* h) const { return filter_guide(h); }
};

template <int C, bool kCount, bool kHoles>
__global__ __launch_bounds__(kUpThreads) void upsample_kernel(const UpArgs k) {
  const size_t i = (size_t)blockIdx.x * kUpThreads + threadIdx.x;
  bool hole = false;
  if (i < k.n) {
    const unsigned p = (unsigned)i;
    const unsigned y = p / k.u.W, x = p - y * k.u.W;
    const FilterGuide c = UpLoadGuide()(k.hits + i);
    float out[C];
#pragma unroll
    for (int q = 0; q < C; ++q) out[q] = 0.f;
    if (c.id >= 0) hole = upsample_pixel<C, kCount>(k.u, k.lo, UpLoadGuide(), c, x, y, out);
#pragma unroll
    for (int q = 0; q < C; ++q) k.dst[i * C + q] = nan_bits(out[q]);
  }
  if constexpr (kHoles) {
    __shared__ unsigned cnt[kUpWaves];
    const unsigned wave = threadIdx.x / 64;
    const unsigned long long m = __ballot(hole);
    if (threadIdx.x % 64 == 0) {
      k.masks[(size_t)blockIdx.x * kUpWaves + wave] = m;
      cnt[wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) k.counts[blockIdx.x] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
  }
}

// One workgroup: counts[g] becomes the sum of the counts before g, *total the
// sum of all (<= W H, so no sum wraps).
__global__ __launch_bounds__(kUpScanThreads) void upsample_scan_kernel(unsigned* counts,
                                                                       unsigned groups,
                                                                       unsigned* total) {
  __shared__ unsigned waveSum[kUpScanThreads / 64];
  __shared__ unsigned carry;
  const unsigned lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (size_t base = 0; base < groups; base += kUpScanThreads) {  // (uniform trip count)
    const size_t g = base + threadIdx.x;
    const unsigned v = g < groups ? counts[g] : 0u;
    unsigned s = v;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(s, d);
      if (lane >= d) s += t;
    }
    if (lane == 63) waveSum[wave] = s;
    __syncthreads();
    unsigned pre = carry;
    for (unsigned w = 0; w < wave; ++w) pre += waveSum[w];
    if (g < groups) counts[g] = pre + (s - v);
    __syncthreads();
    if (threadIdx.x == kUpScanThreads - 1) carry = pre + s;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kUpThreads) void upsample_list_kernel(
    const unsigned* offsets, const unsigned long long* masks, unsigned* holes, unsigned cap) {
  const unsigned wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const unsigned long long* m = masks + (size_t)blockIdx.x * kUpWaves;
  const unsigned long long mine = m[wave];
  if (!((mine >> lane) & 1ull)) return;
  unsigned at = offsets[blockIdx.x];
  for (unsigned w = 0; w < wave; ++w) at += (unsigned)__popcll(m[w]);
  at += (unsigned)__popcll(mine & ((1ull << lane) - 1ull));  // < the frame's holes <= W H
  if (at < cap) holes[at] = blockIdx.x * kUpThreads + threadIdx.x;  // a pixel number: < W H
}

__global__ __launch_bounds__(kUpThreads) void hits_pick_kernel(const rtg_hit* hits, size_t n,
                                                               const unsigned* idx, size_t m,
                                                               rtg_hit* out) {
  const size_t i = (size_t)blockIdx.x * kUpThreads + threadIdx.x;
  if (i >= m) return;
  const unsigned j = idx[i];
  unsigned w[8] = {0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0};
  if (j < n) {
    const uint4* r = reinterpret_cast<const uint4*>(hits + j);
    const uint4 a = r[0], b = r[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
  }
  store_record(out + i, w);
}

template <int C, bool kCount>
__global__ __launch_bounds__(kUpThreads) void values_place_kernel(const void* vals,
                                                                  const unsigned* idx, size_t m,
                                                                  size_t n, unsigned* dst) {
  const size_t i = (size_t)blockIdx.x * kUpThreads + threadIdx.x;
  if (i >= m) return;
  const size_t j = idx[i];
  if (j >= n) return;
  if constexpr (kCount) {
    dst[j] = __float_as_uint((float)static_cast<const unsigned short*>(vals)[i]);
  } else {
#pragma unroll
    for (int q = 0; q < C; ++q) dst[j * C + q] = static_cast<const unsigned*>(vals)[i * C + q];
  }
}

// Rows [y0, y1) on the host; the rows' holes are appended to `found`.
template <int C, bool kCount>
static void upsample_host_rows(const UpArgs& k, size_t y0, size_t y1, std::vector<unsigned>* found) {
  for (size_t y = y0; y < y1; ++y) {
    for (size_t x = 0; x < k.u.W; ++x) {
      const size_t i = y * k.u.W + x;
      const FilterGuide c = filter_guide(k.hits + i);
      float out[C];
      for (int q = 0; q < C; ++q) out[q] = 0.f;
      if (c.id >= 0 &&
          upsample_pixel<C, kCount>(k.u, k.lo, UpHostGuide(), c, (unsigned)x, (unsigned)y, out))
        found->push_back((unsigned)i);
      for (int q = 0; q < C; ++q) k.dst[i * C + q] = nan_bits(out[q]);
    }
  }
}

inline size_t up_groups(size_t n) { return (n + kUpThreads - 1) / kUpThreads; }
inline size_t up_align16(size_t b) { return (b + 15) & ~(size_t)15; }
// The scratch of a frame with a hole list: the counts, then the masks.
inline size_t up_scratch_bytes(size_t n) {
  const size_t g = up_groups(n);
  return up_align16(g * sizeof(unsigned)) + g * kUpWaves * sizeof(unsigned long long);
}

}  // namespace rtg

using namespace rtg;

static int check_up_frame(unsigned W, unsigned H) {
  if (W == 0 || H == 0) {
    rtg_set_error("upsample: empty frame %u x %u", W, H);
    return RTG_ERR_INVALID;
  }
  if (W > (1u << 24) || H > (1u << 24)) {
    rtg_set_error("upsample: frame %u x %u (at most 2^24 each way)", W, H);
    return RTG_ERR_INVALID;
  }
  if ((unsigned long long)W * H > 0xFFFFFFFFull) {
    rtg_set_error("upsample: frame %u x %u (at most 2^32 - 1 pixels)", W, H);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// What the three forms share, in the order it is reported in; fills `k` but
// for its scratch pointers.
static int check_upsample(const rtg_hit* hits, unsigned W, unsigned H, const rtg_upsample_params* p,
                          const rtg_hit* lowHits, unsigned Wl, unsigned Hl, const void* lowSrc,
                          float* dst, unsigned* holes, unsigned holeCap, unsigned* holeCount,
                          const void* scratch, size_t scratchBytes, UpArgs* k) {
  if (!hits || !p || !lowHits || !lowSrc || !dst) {
    rtg_set_error("upsample: null %s", !hits ? "hit buffer" : !p ? "params"
                                       : !lowHits ? "low hit buffer" : !lowSrc ? "low source"
                                                                               : "destination");
    return RTG_ERR_INVALID;
  }
  if (Wl == 0 || Hl == 0) {
    rtg_set_error("upsample: empty low frame %u x %u", Wl, Hl);
    return RTG_ERR_INVALID;
  }
  int rc = check_up_frame(W, H);
  if (rc) return rc;
  const unsigned L = p->scaleLog2;
  if (L < 1 || L > RTG_UPSAMPLE_MAX_SCALE_LOG2) {
    rtg_set_error("upsample: scaleLog2 %u outside [1, %d]", L, RTG_UPSAMPLE_MAX_SCALE_LOG2);
    return RTG_ERR_INVALID;
  }
  if ((unsigned long long)Wl << L != W || (unsigned long long)Hl << L != H) {
    rtg_set_error("upsample: frame %u x %u is not %u times the low frame %u x %u", W, H, 1u << L,
                  Wl, Hl);
    return RTG_ERR_INVALID;
  }
  rc = check_filter_terms("upsample", p->normalLog2, p->kind, p->flags);
  if (rc) return rc;
  if ((holes != nullptr) != (holeCount != nullptr)) {
    rtg_set_error("upsample: %s", holes ? "holes without holeCount" : "holeCount without holes");
    return RTG_ERR_INVALID;
  }
  const size_t n = (size_t)W * H, nl = (size_t)Wl * Hl;
  const size_t C = (size_t)filter_channels(p->kind);
  const struct { const char* name; const void* at; size_t bytes; } r[] = {
      {"dst", dst, n * C * sizeof(float)},
      {"holes", holes, (size_t)holeCap * sizeof(unsigned)},
      {"holeCount", holeCount, sizeof(unsigned)},
      {"the scratch", scratch, scratchBytes},
      {"hits", hits, n * sizeof(rtg_hit)},
      {"lowHits", lowHits, nl * sizeof(rtg_hit)},
      {"lowSrc", lowSrc, nl * filter_src_size(p->kind)},
  };
  for (size_t i = 0; i < 4; ++i)  // each output against every later range
    for (size_t j = i + 1; j < sizeof r / sizeof r[0]; ++j)
      if (filter_overlap(r[i].at, r[i].bytes, r[j].at, r[j].bytes)) {
        rtg_set_error("upsample: %s overlaps %s", r[i].name, r[j].name);
        return RTG_ERR_INVALID;
      }
  *k = UpArgs{};
  k->hits = hits;
  k->lo = {lowHits, lowSrc};
  k->dst = reinterpret_cast<unsigned*>(dst);
  k->u.t = {p->flags, p->normalLog2, p->planeScale};
  k->u.L = L;
  k->u.W = W;
  k->u.Wl = Wl;
  k->u.Hl = Hl;
  k->n = (unsigned)n;
  return RTG_OK;
}

template <bool kHoles>
static void launch_upsample(const UpArgs& k, unsigned kind, unsigned blocks, hipStream_t st) {
  const dim3 g(blocks), b(kUpThreads);
  if (kind == RTG_FILTER_RGB) hipLaunchKernelGGL((upsample_kernel<3, false, kHoles>), g, b, 0, st, k);
  else if (kind == RTG_FILTER_COUNT)
    hipLaunchKernelGGL((upsample_kernel<1, true, kHoles>), g, b, 0, st, k);
  else hipLaunchKernelGGL((upsample_kernel<1, false, kHoles>), g, b, 0, st, k);
}

// The index calls' shared checks; `what` is "hits_pick" or "values_place".
static int check_index_call(const char* what, const void* in, const unsigned* idx, const void* out,
                            size_t n, size_t m, size_t inBytes, size_t outBytes) {
  if (!in || !idx || !out) {
    rtg_set_error("%s: null %s", what, !in ? "input" : !idx ? "index buffer" : "output");
    return RTG_ERR_INVALID;
  }
  if (n == 0) {
    rtg_set_error("%s: n is 0", what);
    return RTG_ERR_INVALID;
  }
  if (filter_overlap(out, outBytes, in, inBytes) ||
      filter_overlap(out, outBytes, idx, m * sizeof(unsigned))) {
    rtg_set_error("%s: the output overlaps an input", what);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

static int check_place(unsigned kind, const void* vals, const unsigned* idx, size_t m, size_t n,
                       float* dst) {
  if (kind > RTG_FILTER_COUNT) {
    rtg_set_error("values_place: kind %u (0: RGB, 1: GRAY, 2: COUNT)", kind);
    return RTG_ERR_INVALID;
  }
  return check_index_call("values_place", vals, idx, dst, n, m, m * filter_src_size(kind),
                          n * (size_t)filter_channels(kind) * sizeof(float));
}

extern "C" {

int rtg_upsample_scratch(unsigned width, unsigned height, int withHoles, size_t* bytes) {
  rtg_clear_error();
  if (!bytes) {
    rtg_set_error("upsample: null size");
    return RTG_ERR_INVALID;
  }
  const int rc = check_up_frame(width, height);
  if (rc) return rc;
  *bytes = withHoles ? up_scratch_bytes((size_t)width * height) : 0;
  return RTG_OK;
}

int rtg_upsample_host(const rtg_hit* hits, unsigned width, unsigned height,
                      const rtg_upsample_params* params, const rtg_hit* lowHits,
                      unsigned lowWidth, unsigned lowHeight, const void* lowSrc, float* dst,
                      unsigned* holes, unsigned holeCap, unsigned* holeCount, int nthreads) {
  rtg_clear_error();
  UpArgs k;
  const int rc = check_upsample(hits, width, height, params, lowHits, lowWidth, lowHeight, lowSrc,
                                dst, holes, holeCap, holeCount, nullptr, 0, &k);
  if (rc) return rc;
  const unsigned kind = params->kind;
  std::map<size_t, std::vector<unsigned>> bands;  // by first row: the list's order
  std::mutex lock;
  host_bands(height, nthreads, [&](size_t y0, size_t y1) {
    std::vector<unsigned> found;
    if (kind == RTG_FILTER_RGB) upsample_host_rows<3, false>(k, y0, y1, &found);
    else if (kind == RTG_FILTER_COUNT) upsample_host_rows<1, true>(k, y0, y1, &found);
    else upsample_host_rows<1, false>(k, y0, y1, &found);
    std::lock_guard<std::mutex> guard(lock);
    bands[y0].swap(found);
  });
  if (holeCount) {
    size_t count = 0;
    for (const auto& b : bands)
      for (const unsigned i : b.second) {
        if (count < holeCap) holes[count] = i;
        ++count;
      }
    *holeCount = (unsigned)count;  // <= W H
  }
  return RTG_OK;
}

int rtg_upsample_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                        unsigned height, const rtg_upsample_params* params,
                        const rtg_hit* lowHitsDevice, unsigned lowWidth, unsigned lowHeight,
                        const void* lowSrcDevice, float* dstDevice, unsigned* holesDevice,
                        unsigned holeCap, unsigned* holeCountDevice, void* scratchDevice,
                        size_t scratchBytes, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("upsample: no context");
    return RTG_ERR_INVALID;
  }
  UpArgs k;
  const int rc = check_upsample(hitsDevice, width, height, params, lowHitsDevice, lowWidth,
                                lowHeight, lowSrcDevice, dstDevice, holesDevice, holeCap,
                                holeCountDevice, scratchDevice, scratchDevice ? scratchBytes : 0,
                                &k);
  if (rc) return rc;
  if (((uintptr_t)hitsDevice & 15) || ((uintptr_t)lowHitsDevice & 15)) {
    rtg_set_error("upsample: %s not 16-byte aligned",
                  ((uintptr_t)hitsDevice & 15) ? "hit buffer" : "low hit buffer");
    return RTG_ERR_INVALID;
  }
  const bool list = holeCountDevice != nullptr;
  const size_t n = (size_t)width * height, groups = up_groups(n);  // groups <= 2^24
  const size_t need = list ? up_scratch_bytes(n) : 0;
  if (need && (!scratchDevice || scratchBytes < need || ((uintptr_t)scratchDevice & 15))) {
    rtg_set_error("upsample: scratch %s (%zu bytes needed, 16-byte aligned)",
                  !scratchDevice ? "is null" : scratchBytes < need ? "too small" : "misaligned",
                  need);
    return RTG_ERR_INVALID;
  }
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(device));
  if (!list) {
    launch_upsample<false>(k, params->kind, (unsigned)groups, st);
    HIP_TRY(hipGetLastError());
    return RTG_OK;
  }
  k.counts = static_cast<unsigned*>(scratchDevice);
  k.masks = reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(scratchDevice) +
                                                  up_align16(groups * sizeof(unsigned)));
  launch_upsample<true>(k, params->kind, (unsigned)groups, st);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(upsample_scan_kernel, dim3(1), dim3(kUpScanThreads), 0, st, k.counts,
                     (unsigned)groups, holeCountDevice);
  HIP_TRY(hipGetLastError());
  if (holeCap) {
    hipLaunchKernelGGL(upsample_list_kernel, dim3((unsigned)groups), dim3(kUpThreads), 0, st,
                       (const unsigned*)k.counts, (const unsigned long long*)k.masks, holesDevice,
                       holeCap);
    HIP_TRY(hipGetLastError());
  }
  return RTG_OK;
}

int rtg_upsample(int device, const rtg_hit* hits, unsigned width, unsigned height,
                 const rtg_upsample_params* params, const rtg_hit* lowHits, unsigned lowWidth,
                 unsigned lowHeight, const void* lowSrc, float* dstHost, unsigned* holesHost,
                 unsigned holeCap, unsigned* holeCountHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  UpArgs k;
  const int rc = check_upsample(hits, width, height, params, lowHits, lowWidth, lowHeight, lowSrc,
                                dstHost, holesHost, holeCap, holeCountHost, nullptr, 0, &k);
  if (rc) return rc;
  const bool list = holeCountHost != nullptr;
  const size_t n = (size_t)width * height, nl = (size_t)lowWidth * lowHeight;
  const size_t scratch = list ? up_scratch_bytes(n) : 0;
  const size_t cap = (size_t)holeCap * sizeof(unsigned);
  // (the list goes up as well as down: the entries past the count stay the
  // caller's; with no capacity the device form still wants a list pointer)
  return one_shot(
      "upsample", device, nullptr,
      {{n * sizeof(rtg_hit), hits, nullptr},
       {nl * sizeof(rtg_hit), lowHits, nullptr},
       {nl * filter_src_size(params->kind), lowSrc, nullptr},
       {n * (size_t)filter_channels(params->kind) * sizeof(float), nullptr, dstHost},
       {list ? (cap ? cap : sizeof(unsigned)) : 0, cap ? holesHost : nullptr,
        cap ? holesHost : nullptr},
       {list ? sizeof(unsigned) : 0, nullptr, holeCountHost},
       {scratch, nullptr, nullptr}},
      [&](rtg_context* ctx, void* const* d) {
        return rtg_upsample_device(ctx, (const rtg_hit*)d[0], width, height, params,
                                   (const rtg_hit*)d[1], lowWidth, lowHeight, d[2], (float*)d[3],
                                   (unsigned*)d[4], holeCap, (unsigned*)d[5], d[6], scratch,
                                   nullptr);
      });
}

int rtg_hits_pick_host(const rtg_hit* hits, size_t n, const unsigned* idx, size_t m,
                       rtg_hit* outHost, int nthreads) {
  rtg_clear_error();
  const int rc = check_index_call("hits_pick", hits, idx, outHost, n, m, n * sizeof(rtg_hit),
                                  m * sizeof(rtg_hit));
  if (rc) return rc;
  host_bands(m, nthreads, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
      if (idx[i] < n) {
        memcpy(outHost + i, hits + idx[i], sizeof(rtg_hit));
      } else {
        memset(outHost + i, 0, sizeof(rtg_hit));
        outHost[i].id = -1;
      }
    }
  });
  return RTG_OK;
}

int rtg_hits_pick_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                         const unsigned* idxDevice, size_t m, rtg_hit* outDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("hits_pick: no context");
    return RTG_ERR_INVALID;
  }
  int rc = check_index_call("hits_pick", hitsDevice, idxDevice, outDevice, n, m,
                            n * sizeof(rtg_hit), m * sizeof(rtg_hit));
  if (rc) return rc;
  if (((uintptr_t)hitsDevice & 15) || ((uintptr_t)outDevice & 15)) {
    rtg_set_error("hits_pick: %s not 16-byte aligned",
                  ((uintptr_t)hitsDevice & 15) ? "hit buffer" : "output");
    return RTG_ERR_INVALID;
  }
  if (m == 0) return RTG_OK;
  const size_t groups = up_groups(m);
  if (groups > 0x7FFFFFFFu) {
    rtg_set_error("hits_pick: list too large (%zu workgroups)", groups);
    return RTG_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(hits_pick_kernel, dim3((unsigned)groups), dim3(kUpThreads), 0,
                     (hipStream_t)stream, hitsDevice, n, idxDevice, m, outDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_values_place_host(unsigned kind, const void* vals, const unsigned* idx, size_t m, size_t n,
                          float* dstHost, int nthreads) {
  rtg_clear_error();
  const int rc = check_place(kind, vals, idx, m, n, dstHost);
  if (rc) return rc;
  const size_t C = (size_t)filter_channels(kind);
  host_bands(m, nthreads, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
      const size_t j = idx[i];
      if (j >= n) continue;
      if (kind == RTG_FILTER_COUNT) {
        dstHost[j] = (float)static_cast<const unsigned short*>(vals)[i];
      } else {  // the words as they are
        memcpy(dstHost + j * C, static_cast<const float*>(vals) + i * C, C * sizeof(float));
      }
    }
  });
  return RTG_OK;
}

int rtg_values_place_device(rtg_context* ctx, unsigned kind, const void* valsDevice,
                            const unsigned* idxDevice, size_t m, size_t n, float* dstDevice,
                            void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("values_place: no context");
    return RTG_ERR_INVALID;
  }
  const int rc = check_place(kind, valsDevice, idxDevice, m, n, dstDevice);
  if (rc) return rc;
  if (m == 0) return RTG_OK;
  const size_t groups = up_groups(m);
  if (groups > 0x7FFFFFFFu) {
    rtg_set_error("values_place: list too large (%zu workgroups)", groups);
    return RTG_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  const dim3 g((unsigned)groups), b(kUpThreads);
  const hipStream_t st = (hipStream_t)stream;
  unsigned* dst = reinterpret_cast<unsigned*>(dstDevice);
  if (kind == RTG_FILTER_RGB)
    hipLaunchKernelGGL((values_place_kernel<3, false>), g, b, 0, st, valsDevice, idxDevice, m, n, dst);
  else if (kind == RTG_FILTER_COUNT)
    hipLaunchKernelGGL((values_place_kernel<1, true>), g, b, 0, st, valsDevice, idxDevice, m, n, dst);
  else
    hipLaunchKernelGGL((values_place_kernel<1, false>), g, b, 0, st, valsDevice, idxDevice, m, n, dst);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

}  // extern "C"
