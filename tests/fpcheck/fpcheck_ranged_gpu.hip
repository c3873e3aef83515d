// tests/fpcheck/fpcheck_ranged_gpu.hip — TEST-ONLY GPU checks of the value-
// range proofs under which the masked render kernel drops its rare-path
// guards (rtg_trace.h IsRangedScene).  Loaded by tests/test_gpu_ranged.py
// through ctypes; not part of librtg.so.
//   * fpcheck_sqrt_domain_run: the two call sites' square root in refraction,
//     sqrt_sel<true> (sqrt_fast_signed), against sqrtf(x) for EVERY float of
//     {0} and [2^-24, 1] (the operand 1 - sinA2^2), [0.001, +inf] (a radicand
//     past the |rad| < 0.001 test), every negative normal float and -inf, and
//     every NaN; and, counted apart, for -0 and the negative subnormals, which
//     neither site can produce (1 - y is 0 or at least 2^-24 in magnitude, a
//     radicand that is used at least 0.001) and where v_sqrt_f32 reads a zero:
//     sqrt_fast alone gives -0 there, sqrtf a NaN, which is what
//     sqrt_fast_signed's select is for.  Values bit for bit; a NaN wanted is a
//     NaN got (position, not payload).
//   * fpcheck_unit_dir_run: unit_dir_query's case analysis on pseudo-random
//     vectors over the whole exponent range, zeros, infinities and NaNs
//     included: den = 2 d.d of d = rcp_sqrt_rn(v.v) v is in [0.92, 5.24] or one
//     of NaN, 0, +inf, and for those three every short-sequence quotient is a
//     NaN where the division gives NaN, an infinity or a zero.
//   * fpcheck_fresnel_ranged_run: div_d_fresnel<true> (no `fast` test) against
//     a / b for the operands polarised_reflection forms from indices with
//     2^-96 <= |n| <= 2^96 and cosines in [-1, 1] or NaN, den^2 >= 1e-6 or NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtg_trace.h"

using namespace rtg;

__device__ __forceinline__ uint32_t mix32(uint64_t v) {
  v ^= v >> 33;
  v *= 0xff51afd7ed558ccdull;
  v ^= v >> 33;
  v *= 0xc4ceb9fe1a85ec53ull;
  v ^= v >> 33;
  return (uint32_t)v;
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

// NaN by position, everything else bit for bit.
__device__ __forceinline__ bool same_f(float got, float want) {
  if (want != want) return got != got;
  return __float_as_uint(got) == __float_as_uint(want);
}
__device__ __forceinline__ bool same_d(double got, double want) {
  if (want != want) return got != got;
  return __double_as_longlong(got) == __double_as_longlong(want);
}

enum { kDomUnit, kDomRad, kDomNeg, kDomNegSub, kDomNan, kDomBad, kDomBadNegSub, kDomSlots };

__global__ __launch_bounds__(256) void sqrt_domain_kernel(unsigned long long* out) {
  unsigned long long c[kDomSlots] = {0, 0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
    const uint32_t u = (uint32_t)i;
    const float x = __uint_as_float(u);
    const bool nan = x != x;
    const bool unit = u == 0u || (x >= 0x1p-24f && x <= 1.f);
    const bool rad = x >= 0.001f;  // +inf included
    const bool negSub = u >= 0x80000000u && u <= 0x807FFFFFu;  // -0 and the subnormals
    const bool neg = !nan && (u >> 31) != 0u && !negSub;
    if (!(nan || unit || rad || neg || negSub)) continue;
    c[kDomUnit] += unit ? 1 : 0;
    c[kDomRad] += rad ? 1 : 0;
    c[kDomNeg] += neg ? 1 : 0;
    c[kDomNegSub] += negSub ? 1 : 0;
    c[kDomNan] += nan ? 1 : 0;
    // the call sites' function: sqrt_sel<true> = sqrt_fast_signed
    if (!same_f(sqrt_sel<true>(x), sqrtf(x))) ++c[negSub ? kDomBadNegSub : kDomBad];
  }
  block_sum<kDomSlots>(c, out);
}

extern "C" int fpcheck_sqrt_domain_run(unsigned long long* out7) {
  unsigned long long* d = nullptr;
  hipError_t e = hipMalloc(&d, kDomSlots * sizeof(unsigned long long));
  if (e != hipSuccess) return (int)e;
  e = hipMemset(d, 0, kDomSlots * sizeof(unsigned long long));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(sqrt_domain_kernel, dim3(16384), dim3(256), 0, nullptr, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = hipMemcpy(out7, d, kDomSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return (int)e;
}

// A float for one component of v: mostly a random sign, mantissa and an
// exponent over the WHOLE range (subnormals and the top binade included);
// every 16th draw a special: +-0, +-inf, a NaN, the smallest subnormals.
__device__ __forceinline__ float rand_component(uint64_t key, int& scale) {
  const uint32_t h = mix32(key), h2 = mix32(key ^ 0x9E3779B97F4A7C15ull);
  if ((h2 & 15u) == 0u) {
    const uint32_t sp[8] = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u,
                            0x7FC00000u, 0x00000001u, 0x80000003u, 0x7F7FFFFFu};
    return __uint_as_float(sp[(h2 >> 4) & 7u]);
  }
  // the three components share `scale` three times in four, so that vectors
  // whose squares all underflow or all overflow are as common as mixed ones
  const int e = ((h2 >> 8) & 3u) ? scale + (int)((h2 >> 10) % 9u) - 4 : (int)((h2 >> 10) % 255u);
  const int ec = e < 0 ? 0 : (e > 254 ? 254 : e);
  return __uint_as_float((h & 0x807FFFFFu) | ((uint32_t)ec << 23));
}

enum { kDirRange, kDirNan, kDirZero, kDirInf, kDirOut, kDirQuotBad, kDirSlots };

__global__ __launch_bounds__(256) void unit_dir_kernel(unsigned long long* out, uint64_t n) {
  unsigned long long c[kDirSlots] = {0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int scale = (int)(mix32(i * 4 + 3) % 255u);
    V3 v;
    v.x = rand_component(i * 4 + 0, scale);
    v.y = rand_component(i * 4 + 1, scale);
    v.z = rand_component(i * 4 + 2, scale);
    const V3 d = vnorm(v);  // l = rcp_sqrt_rn(v.v); d = l v
    const RayQ q = make_query<true>(v3(0.f, 0.f, 0.f), d);
    const float den = q.den;
    if (den >= 0.92f && den <= 5.24f) {
      ++c[kDirRange];
      continue;
    }
    const bool nan = den != den, zero = den == 0.f, inf = den == __builtin_inff();
    if (!(nan || zero || inf)) {
      ++c[kDirOut];
      continue;
    }
    c[kDirNan] += nan ? 1 : 0;
    c[kDirZero] += zero ? 1 : 0;
    c[kDirInf] += inf ? 1 : 0;
    // numerators over the whole range: the division's quotient never passes
    // the root tests' u > 1e-5f && u < 10000.f, the short sequence's is a NaN
    for (int k = 0; k < 4; ++k) {
      const float x = __uint_as_float(mix32(i * 8 + (uint64_t)k + (1ull << 40)));
      const float slow = x / den;
      const float fast = quot_k<true>(x, q);
      if ((slow > 1.0e-5f && slow < 10000.f) || fast == fast) ++c[kDirQuotBad];
    }
  }
  block_sum<kDirSlots>(c, out);
}

extern "C" int fpcheck_unit_dir_run(unsigned long long count, unsigned long long* out6) {
  unsigned long long* d = nullptr;
  hipError_t e = hipMalloc(&d, kDirSlots * sizeof(unsigned long long));
  if (e != hipSuccess) return (int)e;
  e = hipMemset(d, 0, kDirSlots * sizeof(unsigned long long));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(unit_dir_kernel, dim3(16384), dim3(256), 0, nullptr, d, (uint64_t)count);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = hipMemcpy(out6, d, kDirSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return (int)e;
}

// A refractive index a ranged scene may hold: random sign and mantissa, the
// exponent near 1 three times in four, else anywhere in [2^-96, 2^96] (both
// ends included: the mantissa is cleared at the top).
__device__ __forceinline__ float rand_index(uint64_t key) {
  const uint32_t h = mix32(key), h2 = mix32(key ^ 0x9E3779B97F4A7C15ull);
  const int e = (h2 & 3u) ? (int)((h2 >> 4) % 5u) - 2 : (int)((h2 >> 4) % 193u) - 96;
  const uint32_t man = e == 96 ? 0u : (h & 0x007FFFFFu);
  return __uint_as_float((h & 0x80000000u) | man | ((uint32_t)(127 + e) << 23));
}
// A cosine as refraction hands it on: in [-1, 1] (the ends and zeros often),
// every 32nd a NaN.
__device__ __forceinline__ float rand_cos(uint64_t key) {
  const uint32_t h = mix32(key), h2 = mix32(key ^ 0x9E3779B97F4A7C15ull);
  if ((h2 & 31u) == 0u) return __uint_as_float(0x7FC00000u | (h & 0x803FFFFFu));
  if ((h2 & 31u) == 1u) return (h & 1u) ? 1.f : -1.f;
  if ((h2 & 31u) == 2u) return (h & 1u) ? 0.f : -0.f;
  // uniform exponent in [2^-40, 1), random mantissa: magnitude below 1
  const int e = -1 - (int)((h2 >> 8) % 40u);
  return __uint_as_float((h & 0x807FFFFFu) | ((uint32_t)(127 + e) << 23));
}

enum { kFrIn, kFrNan, kFrBad, kFrNotFast, kFrSlots };

__global__ __launch_bounds__(256) void fresnel_ranged_kernel(unsigned long long* out, uint64_t n) {
  unsigned long long c[kFrSlots] = {0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    // polarised_reflection's operations
    const float left = rand_index(4 * i) * rand_cos(4 * i + 1);
    const float right = rand_index(4 * i + 2) * rand_cos(4 * i + 3);
    const double num = (double)(left - right);
    double den = (double)(left + right);
    den *= den;
    if (den < (double)1.0e-6f) continue;  // tiny: the quotient is discarded
    const bool nan = den != den;
    ++c[kFrIn];
    c[kFrNan] += nan ? 1 : 0;
    // what the proof claims: every lane is `fast` or holds a NaN
    if (!nan && !(fabsf(left) <= 0x1p100f && fabsf(right) <= 0x1p100f)) ++c[kFrNotFast];
    const double a = num * num;
    if (!same_d(div_d_fresnel<true>(a, den, false), a / den)) ++c[kFrBad];
  }
  block_sum<kFrSlots>(c, out);
}

extern "C" int fpcheck_fresnel_ranged_run(unsigned long long count, unsigned long long* out4) {
  unsigned long long* d = nullptr;
  hipError_t e = hipMalloc(&d, kFrSlots * sizeof(unsigned long long));
  if (e != hipSuccess) return (int)e;
  e = hipMemset(d, 0, kFrSlots * sizeof(unsigned long long));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fresnel_ranged_kernel, dim3(16384), dim3(256), 0, nullptr, d,
                       (uint64_t)count);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = hipMemcpy(out4, d, kFrSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return (int)e;
}
