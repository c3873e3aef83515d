// tests/fpcheck/fpcheck_exact_gpu.hip — TEST-ONLY exhaustive GPU check of the
// float-only sinA1 of calculateRefraction (rtg_trace.h sin_from_cos2 /
// clamp_cos_sin) against the reference's own expression
//   (float)sqrt(1.0 - (double)(c * c))                       (raytracer.h:683)
// evaluated with the compiler's correctly rounded f64 square root:
//   * bit for bit for EVERY float c in [0, 1) (-c squares to the same float);
//   * the clamp (|c| >= 1: cosine +-1, sine 0) and NaN through clamp_cos_sin,
//     against the reference's three-way branch written out literally.
// And of the scene's material-pair table (rtg_scene_pack.h pair_consts, built
// on the host): for k refractive indices, the k^2 records against a kernel
// that forms nSrc / nTgt and 1.f - 1.f / (ratio * ratio) with the device's own
// operators (where host and device would part on denormals, it shows here).
// Loaded by tests/test_gpu_refraction_exact.py through ctypes; not part of librtg.so.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtg_scene_pack.h"
#include "rtg_trace.h"

using namespace rtg;

enum { kSinIn, kSinBad, kSinFirstBad, kSinSlots };

__global__ __launch_bounds__(256) void fpcheck_sin_kernel(unsigned long long* out, uint64_t n) {
  unsigned long long in = 0, bad = 0, first = ~0ull;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float c = __uint_as_float((uint32_t)i);
    const float cc = c * c;
    const float want = (float)sqrt(1.0 - (double)cc);
    ++in;
    if (__float_as_uint(sin_from_cos2(cc)) != __float_as_uint(want)) {
      ++bad;
      if (i < first) first = i;
    }
  }
  __shared__ unsigned long long part[3][256];
  part[0][threadIdx.x] = in;
  part[1][threadIdx.x] = bad;
  part[2][threadIdx.x] = first;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0, b = 0, f = ~0ull;
    for (int t = 0; t < 256; ++t) {
      a += part[0][t];
      b += part[1][t];
      f = part[2][t] < f ? part[2][t] : f;
    }
    atomicAdd(&out[kSinIn], a);
    atomicAdd(&out[kSinBad], b);
    atomicMin(&out[kSinFirstBad], f);
  }
}

// Every float c in [0, 1) (count = 0) or the first `count` bit patterns;
// out3 = {operands, mismatches, the first mismatching pattern or ~0}.
extern "C" int fpcheck_sin_run(unsigned long long count, unsigned long long* out3) {
  unsigned long long* d = nullptr;
  hipError_t e = hipMalloc(&d, kSinSlots * sizeof(unsigned long long));
  if (e != hipSuccess) return (int)e;
  const unsigned long long init[kSinSlots] = {0, 0, ~0ull};
  e = hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice);
  const uint64_t full = 0x3F800000ull;
  const uint64_t n = (count && count < full) ? count : full;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fpcheck_sin_kernel, dim3(8192), dim3(256), 0, nullptr, d, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = hipMemcpy(out3, d, kSinSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return (int)e;
}

// clamp_cos_sin on n caller-chosen cosines (bit patterns in, the clamped
// cosine's and the sine's bit patterns out), next to the reference's branch
// (raytracer.h:671-683) on the same values.
__global__ void fpcheck_clamp_kernel(const uint32_t* in, uint32_t* got, uint32_t* want, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float c = __uint_as_float(in[i]);
  float c1 = c;
  const float s1 = clamp_cos_sin(c1);
  got[2 * i] = __float_as_uint(c1);
  got[2 * i + 1] = __float_as_uint(s1);
  float s = 0.f;
  if (c <= -1.0f) { c = -1.f; s = 0.f; }
  else if (c >= 1.f) { c = 1.f; s = 0.f; }
  else s = (float)sqrt(1.0 - (double)(c * c));
  want[2 * i] = __float_as_uint(c);
  want[2 * i + 1] = __float_as_uint(s);
}

extern "C" int fpcheck_clamp_run(const uint32_t* in, unsigned n, uint32_t* got, uint32_t* want) {
  if (n == 0 || n > 65536) return -1;
  uint32_t *dIn = nullptr, *dGot = nullptr, *dWant = nullptr;
  hipError_t e = hipMalloc(&dIn, n * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&dGot, 2 * n * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&dWant, 2 * n * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(dIn, in, n * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fpcheck_clamp_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dIn, dGot,
                       dWant, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(got, dGot, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(want, dWant, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  (void)hipFree(dIn);
  (void)hipFree(dGot);
  (void)hipFree(dWant);
  return (int)e;
}

// The pair records of k indices: the host's (pair_consts) into host2, the
// device's own division and reciprocal into dev2 (k * k * 2 words each).
__global__ void fpcheck_pair_kernel(const float* idx, unsigned k, float* out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k * k) return;
  const float ratio = idx[i / k] / idx[i % k];
  out[2 * i] = ratio;
  out[2 * i + 1] = 1.f - 1.f / (ratio * ratio);
}

extern "C" int fpcheck_pair_run(const float* idx, unsigned k, float* host2, float* dev2) {
  if (k == 0 || k > 256) return -1;
  for (unsigned s = 0; s < k; ++s)
    for (unsigned t = 0; t < k; ++t) pair_consts(idx[s], idx[t], &host2[2 * ((size_t)s * k + t)]);
  const size_t n = (size_t)k * k;
  float *dIdx = nullptr, *dOut = nullptr;
  hipError_t e = hipMalloc(&dIdx, k * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&dOut, 2 * n * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(dIdx, idx, k * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fpcheck_pair_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                       dIdx, k, dOut);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(dev2, dOut, 2 * n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(dIdx);
  (void)hipFree(dOut);
  return (int)e;
}
