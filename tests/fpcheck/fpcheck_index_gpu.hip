// tests/fpcheck/fpcheck_index_gpu.hip — TEST-ONLY GPU checks of the index
// helpers with which the render and G-buffer kernels avoid integer division
// (rtg_trace_kernels.h), each against the plain 64-bit `/` and `%` of the
// device.  Loaded by tests/test_gpu_large.py through ctypes; not part of
// librtg.so.
//   * fpcheck_divmod_run: divmod_u64(a, d, RN(1.0 / d)) over seeded draws of
//     (q, d, r) with a = q d + r < 2^53, q < 2^32, 1 <= d < 2^32: d over the
//     whole range on the odd draws and over 1 .. 2^17 (a frame's width) on the
//     even ones, r one of 0, d - 1 and uniform.  Counted with the mismatches:
//     how often the f64 estimate was one too small (the upward correction)
//     and one too large (the downward one), so that a run in which a branch
//     never executed cannot pass for a check of it.
//   * fpcheck_divmod_edges_run: the same on a caller's list of (a, d, invd),
//     for the hand-made edges; the host's RN(1.0 / d) is compared with the
//     device's on the way.
//   * fpcheck_udiv_small_run: udiv_small(a, d) for every 0 <= a <= 64,
//     1 <= d <= 64.
//   * fpcheck_shard_row_run: shard_global_row_fast against shard_global_row
//     (rtg_internal.h) and against the same sum in 64 bits, over seeded
//     (localRow, B, g, G) whose global row stays below 2^32: B = 1, G = 1 and
//     the largest local row of a (B, g, G) each a fixed share of the draws.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtg_trace_kernels.h"

using namespace rtg;

__device__ __forceinline__ uint32_t mix32(uint64_t v) {
  v ^= v >> 33;
  v *= 0xff51afd7ed558ccdull;
  v ^= v >> 33;
  v *= 0xc4ceb9fe1a85ec53ull;
  v ^= v >> 33;
  return (uint32_t)v;
}
__device__ __forceinline__ uint64_t mix64(uint64_t key) {
  return ((uint64_t)mix32(key) << 32) | mix32(key ^ 0x9E3779B97F4A7C15ull);
}

// Adds the block's per-thread counters c[0 .. kSlots) to out.
template <int kSlots>
__device__ __forceinline__ void block_sum(const unsigned long long* c, unsigned long long* out) {
  __shared__ unsigned long long part[kSlots][256];
  for (int k = 0; k < kSlots; ++k) part[k][threadIdx.x] = c[k];
  __syncthreads();
  if (threadIdx.x < kSlots) {
    unsigned long long sum = 0;
    for (int t = 0; t < 256; ++t) sum += part[threadIdx.x][t];
    atomicAdd(&out[threadIdx.x], sum);
  }
}

template <int kSlots, class Launch>
static int run_counted(unsigned long long* out, Launch launch) {
  unsigned long long* d = nullptr;
  hipError_t e = hipMalloc(&d, kSlots * sizeof(unsigned long long));
  if (e != hipSuccess) return (int)e;
  e = hipMemset(d, 0, kSlots * sizeof(unsigned long long));
  if (e == hipSuccess) {
    launch(d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = hipMemcpy(out, d, kSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return (int)e;
}

enum { kDivN, kDivBad, kDivUp, kDivDown, kDivRZero, kDivRMax, kDivSmallD, kDivInvBad, kDivSlots };

// One (a, d, invd): divmod_u64 against / and %, and which correction its
// estimate needs (divmod_u64's own first two lines).
__device__ __forceinline__ void divmod_case(uint64_t a, unsigned d, double invd,
                                            unsigned long long* c) {
  unsigned q, r;
  divmod_u64(a, d, invd, q, r);
  const uint64_t wq = a / d, wr = a % d;
  ++c[kDivN];
  if ((uint64_t)q != wq || (uint64_t)r != wr) ++c[kDivBad];
  const uint64_t qq = (uint64_t)((double)a * invd);
  const int64_t rr = (int64_t)(a - qq * d);
  if (rr < 0) ++c[kDivDown];
  else if (rr >= (int64_t)d) ++c[kDivUp];
}

__global__ __launch_bounds__(256) void divmod_kernel(unsigned long long* out, uint64_t n) {
  unsigned long long c[kDivSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const bool small = (i & 1u) == 0u;
    const uint32_t hd = mix32(3 * i);
    // 1 .. 2^17, or 1 .. 2^32 - 1
    const unsigned d = small ? 1u + (hd & 0x1FFFFu) : 1u + hd % 0xFFFFFFFFu;
    // the largest q < 2^32 with q d + (d - 1) < 2^53
    uint64_t qmax = ((1ull << 53) - d) / d;
    if (qmax > 0xFFFFFFFFull) qmax = 0xFFFFFFFFull;
    const uint64_t q = mix64(3 * i + 1) % (qmax + 1);
    const uint64_t hr = mix64(3 * i + 2);
    const unsigned kind = (unsigned)(hr >> 60) % 3u;
    const uint64_t r = kind == 0u ? 0u : kind == 1u ? d - 1u : (hr & 0xFFFFFFFFull) % d;
    c[kDivRZero] += r == 0u ? 1 : 0;
    c[kDivRMax] += r == d - 1u ? 1 : 0;
    c[kDivSmallD] += small ? 1 : 0;
    divmod_case(q * d + r, d, 1.0 / (double)d, c);
  }
  block_sum<kDivSlots>(c, out);
}

extern "C" int fpcheck_divmod_run(unsigned long long count, unsigned long long* out8) {
  return run_counted<kDivSlots>(out8, [&](unsigned long long* d) {
    hipLaunchKernelGGL(divmod_kernel, dim3(16384), dim3(256), 0, nullptr, d, (uint64_t)count);
  });
}

__global__ __launch_bounds__(256) void divmod_edges_kernel(unsigned long long* out,
                                                           const uint64_t* a, const unsigned* d,
                                                           const double* invd, unsigned n) {
  unsigned long long c[kDivSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (__double_as_longlong(invd[i]) != __double_as_longlong(1.0 / (double)d[i])) ++c[kDivInvBad];
    divmod_case(a[i], d[i], invd[i], c);
  }
  block_sum<kDivSlots>(c, out);
}

// a, d, invd: host arrays of n entries, a[i] < 2^53, a[i] / d[i] < 2^32.
extern "C" int fpcheck_divmod_edges_run(const unsigned long long* a, const unsigned* d,
                                        const double* invd, unsigned n,
                                        unsigned long long* out8) {
  uint64_t* da = nullptr;
  unsigned* dd = nullptr;
  double* di = nullptr;
  hipError_t e = hipMalloc(&da, n * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&dd, n * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(&di, n * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(da, a, n * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dd, d, n * sizeof(unsigned), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(di, invd, n * sizeof(double), hipMemcpyHostToDevice);
  int rc = (int)e;
  if (e == hipSuccess)
    rc = run_counted<kDivSlots>(out8, [&](unsigned long long* o) {
      hipLaunchKernelGGL(divmod_edges_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, o, da,
                         dd, di, n);
    });
  (void)hipFree(da);
  (void)hipFree(dd);
  (void)hipFree(di);
  return rc;
}

enum { kSmallN, kSmallBad, kSmallSlots };

__global__ __launch_bounds__(256) void udiv_small_kernel(unsigned long long* out) {
  unsigned long long c[kSmallSlots] = {0, 0};
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 65u * 64u) {
    const unsigned a = i / 64u, d = 1u + i % 64u;
    ++c[kSmallN];
    if (udiv_small(a, d) != a / d) ++c[kSmallBad];
  }
  block_sum<kSmallSlots>(c, out);
}

extern "C" int fpcheck_udiv_small_run(unsigned long long* out2) {
  return run_counted<kSmallSlots>(out2, [&](unsigned long long* d) {
    hipLaunchKernelGGL(udiv_small_kernel, dim3((65 * 64 + 255) / 256), dim3(256), 0, nullptr, d);
  });
}

enum { kRowN, kRowBad, kRowB1, kRowG1, kRowTop, kRowHigh, kRowSlots };

__global__ __launch_bounds__(256) void shard_row_kernel(unsigned long long* out, uint64_t n) {
  unsigned long long c[kRowSlots] = {0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t hb = mix32(4 * i), hg = mix32(4 * i + 1), hs = mix32(4 * i + 2);
    const uint64_t hl = mix64(4 * i + 3);
    // B: 1, 1 .. 64, or 1 .. 2^20; G: 1, 1 .. 16, or 1 .. 2^16
    const unsigned kb = hs & 3u, kg = (hs >> 2) & 3u;
    const unsigned B = kb == 0u ? 1u : kb == 1u ? 1u + (hb & 63u) : 1u + (hb & 0xFFFFFu);
    const unsigned G = kg == 0u ? 1u : kg == 1u ? 1u + (hg & 15u) : 1u + (hg & 0xFFFFu);
    // 2^32 / B >= 4096 blocks below global row 2^32, so any g < G <= 2^16 ...
    const uint64_t blocks = (1ull << 32) / B;
    unsigned g = (hg >> 16) % G;
    if ((uint64_t)g + 1 > blocks) g = 0;  // ... but those past the last block
    // the shard's last local block whose rows all stay below 2^32, and its
    // last row
    const uint64_t lbmax = (blocks - g - 1) / G;
    const uint64_t top = lbmax * B + (B - 1);
    const unsigned kl = (hs >> 4) & 3u;
    const uint64_t row = kl == 0u   ? top
                         : kl == 1u ? top - (hl & 0xFFu) % (top + 1)
                                    : hl % (top + 1);
    const unsigned lr = (unsigned)row;
    const uint64_t want = ((uint64_t)(lr / B) * G + g) * B + lr % B;
    ++c[kRowN];
    c[kRowB1] += B == 1u ? 1 : 0;
    c[kRowG1] += G == 1u ? 1 : 0;
    c[kRowTop] += row == top ? 1 : 0;
    c[kRowHigh] += want >= (1ull << 31) ? 1 : 0;
    const unsigned fast = shard_global_row_fast(lr, B, 1.0 / (double)B, g, G);
    if (want >> 32 || (uint64_t)fast != want || (uint64_t)shard_global_row(lr, B, g, G) != want)
      ++c[kRowBad];
  }
  block_sum<kRowSlots>(c, out);
}

extern "C" int fpcheck_shard_row_run(unsigned long long count, unsigned long long* out6) {
  return run_counted<kRowSlots>(out6, [&](unsigned long long* d) {
    hipLaunchKernelGGL(shard_row_kernel, dim3(4096), dim3(256), 0, nullptr, d, (uint64_t)count);
  });
}
