// rtg_probes.h — the probe generator of ambient occlusion and of the gather
// (rtg_ao_segments*, rtg_gather_rays*, rtg.h), written ONCE over "the last
// three words of probe k": the six-word record, the one-lane-per-probe kernel,
// the host loop, the device launcher, and the checks the generators share with
// the fused forms.  rtg_ao.hip supplies the far end ao_end(pt, l, radius) and
// rtg_gather.hip the direction gather_dir(pt, l); nothing here asks which.
// HIP translation units only.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_ao.h"
#include "rtg_entry.h"

namespace rtg {

// What rtg_ao_params and rtg_gather_params share.
struct ProbeParams {
  unsigned samples;
  float bias;
  unsigned seed, flags;
};
template <class P>
inline ProbeParams probe_params(const P& p) {
  return {p.samples, p.bias, p.seed, p.flags};
}

// Probe k of point i as six words: the start a, then tail(pt, l) for the
// local direction l of the probe; a record without a point: zeros.
template <class Tail>
RTG_HD void probe_words(const rtg_hit* hits, size_t i, unsigned k, const ProbeParams& p,
                        const Tail& tail, const rtg_vec* dirs, unsigned nDirs, unsigned* w) {
  const AoPoint pt = ao_point(hits + i, p.bias);
  V3 a = v3(0.f, 0.f, 0.f), b = v3(0.f, 0.f, 0.f);
  if (pt.id >= 0) {
    a = pt.a;
    b = tail(pt, ao_dir(dirs, ao_dir_index(ao_window(p.flags, p.seed, i, nDirs), k, nDirs)));
  }
  w[0] = nan_bits(a.x); w[1] = nan_bits(a.y); w[2] = nan_bits(a.z);
  w[3] = nan_bits(b.x); w[4] = nan_bits(b.y); w[5] = nan_bits(b.z);
}

// One lane per probe, 24 B out; total = n * K > 0.  It needs no scene.  (The
// tail comes last: an empty one then moves no other argument.)
template <class Tail>
__global__ __launch_bounds__(64) void probes_kernel(const rtg_hit* __restrict__ hits, size_t total,
                                                    const ProbeParams p,
                                                    const rtg_vec* __restrict__ dirs,
                                                    unsigned nDirs, unsigned* __restrict__ out,
                                                    const Tail tail) {
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= total) return;
  unsigned w[6];
  probe_words(hits, k / p.samples, (unsigned)(k % p.samples), p, tail, dirs, nDirs, w);  // k / K < n
  unsigned* o = out + 6 * k;  // k < total: 24 B of the batch
  for (int q = 0; q < 6; ++q) o[q] = w[q];
}

// ---- checks ----

// What every form of rtg_ao* and rtg_gather* shares, in the order it is
// reported in; `known`: the entry point's flag bits; the forms without a
// weight table pass wantWeights false.  (The limits are the gather's too:
// rtg_gather_kernels.h asserts it.)
template <class P>
inline int check_probes(const char* what, unsigned known, const void* hits, const P* p,
                        const void* dirs, bool wantWeights, const void* weights, unsigned nDirs,
                        const void* out) {
  if (!hits || !p || !dirs || (wantWeights && !weights) || !out) {
    rtg_set_error("%s: null %s", what,
                  !hits ? "hit buffer" : !p ? "params" : !dirs ? "direction table"
                  : (wantWeights && !weights) ? "weight table" : "output buffer");
    return RTG_ERR_INVALID;
  }
  if (p->samples < 1 || p->samples > RTG_AO_MAX_SAMPLES) {
    rtg_set_error("%s: %u samples outside [1, %d]", what, p->samples, RTG_AO_MAX_SAMPLES);
    return RTG_ERR_INVALID;
  }
  if (nDirs < p->samples || nDirs > RTG_AO_MAX_DIRS) {
    rtg_set_error("%s: %u directions outside [samples = %u, %d]", what, nDirs, p->samples,
                  RTG_AO_MAX_DIRS);
    return RTG_ERR_INVALID;
  }
  if (p->flags & ~known) {
    rtg_set_error("%s: unknown flags 0x%x", what, p->flags & ~known);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// n as the window hash takes it.
inline int check_probe_points(const char* what, size_t n) {
  if (n <= 0xFFFFFFFFull) return RTG_OK;
  rtg_set_error("%s: %zu points (at most 2^32 - 1)", what, n);
  return RTG_ERR_INVALID;
}

// The generators' n * K (reported before the point count: every n whose
// product overflows is above 2^32 - 1 too).
inline int check_probe_product(const char* what, size_t n, unsigned K) {
  if (n <= SIZE_MAX / K) return check_probe_points(what, n);
  rtg_set_error("%s: %zu points x %u samples overflows size_t", what, n, K);
  return RTG_ERR_INVALID;
}

// ---- the generators' two forms ----
// `tail_of(*params)` makes the Tail once the params are known not to be null.

template <class P, class TailOf>
int probes_host(const char* what, unsigned known, const rtg_hit* hits, size_t n, const P* params,
                TailOf tail_of, const rtg_vec* dirs, unsigned nDirs, void* outHost, int nthreads) {
  rtg_clear_error();
  int rc = check_probes(what, known, hits, params, dirs, false, nullptr, nDirs, outHost);
  if (!rc) rc = check_probe_product(what, n, params->samples);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  const ProbeParams p = probe_params(*params);
  const auto tail = tail_of(*params);
  host_bands(n, nthreads, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
      for (unsigned k = 0; k < p.samples; ++k) {
        unsigned w[6];
        probe_words(hits, i, k, p, tail, dirs, nDirs, w);
        memcpy(static_cast<unsigned char*>(outHost) + (i * p.samples + k) * sizeof w, w, sizeof w);
      }
    }
  });
  return RTG_OK;
}

template <class P, class TailOf>
int probes_device(const char* what, unsigned known, rtg_context* ctx, const rtg_hit* hitsDevice,
                  size_t n, const P* params, TailOf tail_of, const rtg_vec* dirsDevice,
                  unsigned nDirs, void* outDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("%s: no context", what);
    return RTG_ERR_INVALID;
  }
  int rc = check_probes(what, known, hitsDevice, params, dirsDevice, false, nullptr, nDirs,
                        outDevice);
  if (!rc) rc = check_probe_product(what, n, params->samples);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  const size_t total = n * params->samples;
  unsigned blocks;
  rc = ray_blocks(what, "batch", total, &blocks);
  if (rc) return rc;
  auto tail = tail_of(*params);
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(probes_kernel<decltype(tail)>, dim3(blocks), dim3(64), 0,
                     (hipStream_t)stream, hitsDevice, total, probe_params(*params), dirsDevice,
                     nDirs, static_cast<unsigned*>(outDevice), tail);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

}  // namespace rtg
