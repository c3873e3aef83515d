// rtg_gbuffer.hip — the primary-hit G-buffer of librtg.so (rtg_gbuf_px,
// rtg.h): per pixel the closest sphere of its primary rays, that hit's t and
// normal, and the coverage of its samples.  No shading, no recursion, no
// lights: the primary ray set-up (sample_dir), the primary cull (group_sel)
// and the closest-hit queries are the trace kernel's own (rtg_trace.h), so a
// sample's (id, t) here is what calcIntersection (raytracer.h:145-194) gives
// the render for its primary ray, bit for bit.
//
// Sample-parallel kernel (1 <= nAA <= 8, the trace kernel's mapping): a wave
// traces a pixel group, floor(64 / nAA^2) consecutive pixels of the shard,
// one (pixel, sample) per lane; each pixel's first lane reduces its samples
// from a 64-entry LDS array in sample order and writes the 32-byte record as
// two 16-byte stores.  A one-wave workgroup takes 64 groups: it culls them
// one per lane, writes the miss records of the empty ones at once and traces
// the others in turn.  Other nAA: one lane per pixel, samples in a loop.
// One translation unit, no instantiation per stack size: nothing here
// depends on it.  The launch takes none of rtg_context's render scratch.
//
// rtg_gbuffer_host computes the same records with plain loops (closest_hit
// over every sphere); it is the kernel's yardstick in the tests.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_entry.h"
#include "rtg_trace_kernels.h"
#include "rtg_scene_pack.h"

static_assert(sizeof(rtg_gbuf_px) == 32, "rtg_gbuf_px is 32 B");
static_assert(offsetof(rtg_gbuf_px, t) == 4 && offsetof(rtg_gbuf_px, hits) == 8 &&
                  offsetof(rtg_gbuf_px, sample) == 12 && offsetof(rtg_gbuf_px, normal) == 16 &&
                  offsetof(rtg_gbuf_px, idSum) == 28,
              "rtg_gbuf_px layout (two 16-byte halves)");

namespace rtg {

// A pixel's record while its samples are taken in the reference's loop order.
struct GbufAcc {
  int id = -1;
  float t = 1000.f;
  unsigned hits = 0, sample = 0, idSum = 0;
};
// Sample s with closest hit (id, t); id < 0: a miss.  A hit's t is below
// 1000 (calcIntersection's minT), so the strict < keeps the smallest t and,
// on a tie, the earlier sample.
RTG_HD void gbuf_take(GbufAcc& r, int id, float t, unsigned s) {
  if (id >= 0) {
    ++r.hits;
    r.idSum += (unsigned)id + 1u;
    if (t < r.t) {
      r.t = t;
      r.id = id;
      r.sample = s;
    }
  }
}
// The finished record of pixel (x, gy) as its eight words; the normal is
// the shading normal of the winning hit only (raytracer.h:464-468: P = o +
// t d with o = (0,0,0), N = vnorm(P - c)).
template <class Scene>
RTG_HD void gbuf_record(const Scene& sc, const Camera& cam, unsigned x, unsigned gy,
                        const GbufAcc& r, unsigned* w) {
  V3 N = v3(0.f, 0.f, 0.f);
  if (r.id >= 0) {
    const unsigned nAA = (unsigned)cam.nAA;
    const unsigned i = r.sample / nAA, j = r.sample - i * nAA;
    float rx, ry, r2;
    const V3 d = sample_dir(cam, x, gy, (int)i, (int)j, rx, ry);
    const V3 c = sc.sphere((unsigned)r.id, r2);
    const V3 P = vadd(v3(0.f, 0.f, 0.f), vsmul(r.t, d));
    N = vnorm(vsub(P, c));
  }
  w[0] = (unsigned)r.id;
  w[1] = nan_bits(r.t);
  w[2] = r.hits;
  w[3] = r.sample;
  w[4] = nan_bits(N.x);
  w[5] = nan_bits(N.y);
  w[6] = nan_bits(N.z);
  w[7] = r.idSum;
}

static void gbuffer_host_rows(const HostSpheres& sc, const Camera& cam, unsigned W, size_t y0,
                              size_t y1, rtg_gbuf_px* dst) {
  for (unsigned y = (unsigned)y0; y < y1; ++y)
    for (unsigned x = 0; x < W; ++x) {
      GbufAcc r;
      for (int i = 0; i < cam.nAA; ++i)
        for (int j = 0; j < cam.nAA; ++j) {
          float rx, ry, t;
          const V3 d = sample_dir(cam, x, y, i, j, rx, ry);
          const int id = closest_hit(sc, v3(0.f, 0.f, 0.f), d, t);
          gbuf_take(r, id, t, (unsigned)(i * cam.nAA + j));
        }
      unsigned w[8];
      gbuf_record(sc, cam, x, y, r, w);
      memcpy(&dst[(size_t)y * W + x], w, sizeof w);
    }
}

// The trace kernels' scene over the context's tables (bind_scene: global
// memory, scalar loads for wave-uniform indices), without frames.
template <bool kBvh>
using GbufScene = DevScene<false, 64, kBvh, kFusePrim>;

// The closest hit of a primary ray of a scene without a usable sphere mask:
// the BVH when the scene has one (kBvh), else every sphere, four per step.
template <bool kBvh>
__device__ __forceinline__ int gbuf_closest(const GbufScene<kBvh>& sc, V3 d, float& t) {
  const V3 o = v3(0.f, 0.f, 0.f);
  if constexpr (kBvh) return closest_bvh(sc, make_query(o, d), t);
  else return closest_hit4(sc, o, d, t);
}

// Order the wave's LDS accesses before and after this point.
__device__ __forceinline__ void gbuf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Pixel group gw (1 <= nAA <= 8) on the whole wave, entered converged: lane =
// (pixel pl, sample s) as in trace_group.  masked: `sel` is the group's
// sphere mask (not empty), for the fused masked query.
template <bool kBvh>
__device__ __forceinline__ void gbuf_group(const KernelArgs& a, const GbufScene<kBvh>& sc,
                                           size_t gw, bool masked, uint64_t sel, float* sT,
                                           int* sId, rtg_gbuf_px* __restrict__ dst) {
  const unsigned lane = threadIdx.x;
  const unsigned nAA = (unsigned)a.cam.nAA;
  const unsigned SP = nAA * nAA;
  const unsigned PPW = 64u / SP;
  const unsigned pl = udiv_small(lane, SP), s = lane - pl * SP;
  const size_t p0 = gw * PPW;  // the group's first pixel (wave-uniform)
  const size_t total = (size_t)a.W * a.rowsLocal;
  const size_t p = p0 + pl;
  const bool valid = pl < PPW && p < total;
  unsigned col0, r0;
  divmod_u64(p0, a.W, a.invW, r0, col0);
  unsigned x = col0 + pl, lr = r0, gy = 0;
  while (x >= a.W) {
    x -= a.W;
    ++lr;
  }
  if (valid) gy = shard_global_row_fast(lr, a.rowBlock, a.invRowBlock, a.shard, a.nShards);
  const int si = (int)udiv_small(s, nAA), sj = (int)(s - (unsigned)si * nAA);

  int id = -1;
  float t = 1000.f;
  if (valid) {
    float rx, ry;
    const V3 dir = sample_dir(a.cam, x, gy, si, sj, rx, ry);
    if (masked) id = closest_hit_sel(sc, v3(0.f, 0.f, 0.f), dir, t, sel);
    else id = gbuf_closest<kBvh>(sc, dir, t);
  }
  // whole wave converged again: every lane parks its sample, each pixel's
  // first lane takes its nAA^2 samples in order
  sT[lane] = t;
  sId[lane] = id;
  gbuf_wave_sync();
  if (valid && s == 0) {
    const unsigned base = pl * SP;  // base + SP <= 64: pl < PPW
    GbufAcc r;
    for (unsigned k = 0; k < SP; ++k) gbuf_take(r, sId[base + k], sT[base + k], k);
    unsigned w[8];
    gbuf_record(sc, a.cam, x, gy, r, w);
    store_record(dst + p, w);  // p < total: inside the shard's records
  }
  gbuf_wave_sync();  // the next group parks its samples in the same slots
}

// Sample-parallel kernel (1 <= nAA <= 8).  A one-wave workgroup takes 64
// consecutive pixel groups (`groups` in all).  Scenes of at most 64 spheres:
// each lane culls one group (group_sel, as the render's cull pass: the
// sphere loop is wave-uniform, so the records are scalar loads); the groups
// no sphere can be reached from get their miss records from the whole wave,
// in coalesced 16-byte stores and with no query; the others are traced in
// turn.  Larger scenes trace every group (BVH, or every sphere).  One wave
// per group, the trace kernel's direct launch, measured 1.14 ms on the C3
// frame against 0.1 ms of record writes: 1.2 M one-wave workgroups, seven of
// eight of them over empty groups.
template <bool kBvh>
__global__ __launch_bounds__(64) void gbuffer_samples_kernel(const KernelArgs a, size_t groups,
                                                             rtg_gbuf_px* __restrict__ dst) {
  __shared__ float sT[64];
  __shared__ int sId[64];
  __shared__ int stk[kBvh ? 64 : 1];
  GbufScene<kBvh> sc;
  bind_scene_no_frames(sc, a.scene, stk);  // stk: the wave's BVH traversal stack
  const unsigned lane = threadIdx.x;
  const unsigned nAA = (unsigned)a.cam.nAA;
  const unsigned PPW = 64u / (nAA * nAA);
  const size_t total = (size_t)a.W * a.rowsLocal;
  const size_t g0 = (size_t)blockIdx.x * 64;  // the wave's first group
  const size_t g = g0 + lane;
  const bool masked = !kBvh && a.scene.n <= 64;
  uint64_t sel = 0;
  if (masked && g < groups) sel = group_sel(a, g, PPW, total);
  const uint64_t live = __ballot(g < groups && (!masked || sel != 0ull));
  // Miss records of the other groups: the wave's pixels are contiguous, two
  // 16-byte halves each.  Pixel px of the wave is in its group px / PPW,
  // taken as a float product: px < 4096, so (px + 0.5) / PPW is at least
  // 1/128 from an integer, far beyond the product's error (udiv_small).
  const size_t px0 = g0 * PPW;
  const size_t left = total - px0;  // > 0: g0 < groups
  const unsigned npx = left < (size_t)64 * PPW ? (unsigned)left : 64u * PPW;
  const float invP = 1.0f / (float)PPW;
  uint4* half = reinterpret_cast<uint4*>(dst + px0);
  for (unsigned q = lane; q < 2u * npx; q += 64u) {
    const unsigned grp = (unsigned)(((float)(q >> 1) + 0.5f) * invP);
    if (!((live >> grp) & 1ull))
      half[q] = (q & 1u) ? make_uint4(0u, 0u, 0u, 0u)
                         : make_uint4(0xFFFFFFFFu, 0x447A0000u /* 1000.f */, 0u, 0u);
  }
  for (uint64_t m = live; m;) {  // wave-uniform
    const int k = __builtin_ctzll(m);
    m &= m - 1;
    const uint64_t selk =
        (uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)sel, k) |
        ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sel >> 32), k) << 32);
    gbuf_group<kBvh>(a, sc, g0 + (unsigned)k, masked, selk, sT, sId, dst);
  }
}

// Any other nAA (0, or more than 8: a pixel's samples do not fit a wave):
// one lane per pixel, its samples in the reference's loop order.
template <bool kBvh>
__global__ __launch_bounds__(64) void gbuffer_pixels_kernel(const KernelArgs a, size_t,
                                                            rtg_gbuf_px* __restrict__ dst) {
  __shared__ int stk[kBvh ? 64 : 1];
  GbufScene<kBvh> sc;
  bind_scene_no_frames(sc, a.scene, stk);  // stk: the wave's BVH traversal stack
  const size_t total = (size_t)a.W * a.rowsLocal;
  const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= total) return;
  unsigned x, lr;
  divmod_u64(p, a.W, a.invW, lr, x);
  const unsigned gy = shard_global_row_fast(lr, a.rowBlock, a.invRowBlock, a.shard, a.nShards);
  GbufAcc r;
  const int nAA = a.cam.nAA;  // wave-uniform trip counts
  for (int i = 0; i < nAA; ++i)
    for (int j = 0; j < nAA; ++j) {
      float rx, ry, t;
      const V3 dir = sample_dir(a.cam, x, gy, i, j, rx, ry);
      const int id = gbuf_closest<kBvh>(sc, dir, t);
      gbuf_take(r, id, t, (unsigned)(i * nAA + j));
    }
  unsigned w[8];
  gbuf_record(sc, a.cam, x, gy, r, w);
  store_record(dst + p, w);
}

}  // namespace rtg

using namespace rtg;

// Argument checks shared by the host and one-shot entry points (no HIP call).
static int check_gbuffer_args(const rtg_sphere* spheres, unsigned sphNum, unsigned width,
                              unsigned height, float zoom, float aliasFactor, const void* dst,
                              Camera* cam) {
  if (!dst) {
    rtg_set_error("gbuffer: null destination");
    return RTG_ERR_INVALID;
  }
  const int rc = check_scene_arrays("gbuffer", spheres, sphNum);
  return rc ? rc : make_camera(width, height, zoom, aliasFactor, cam);
}

extern "C" {

int rtg_gbuffer_host(const rtg_sphere* spheres, unsigned sphNum, unsigned width,
                     unsigned height, float zoom, float aliasFactor, rtg_gbuf_px* dstHost,
                     int nthreads) {
  rtg_clear_error();
  Camera cam;
  const int rc = check_gbuffer_args(spheres, sphNum, width, height, zoom, aliasFactor, dstHost,
                                    &cam);
  if (rc) return rc;
  const HostSpheres sc{spheres, sphNum};
  host_bands(height, nthreads, [&](size_t y0, size_t y1) {  // contiguous row bands
    gbuffer_host_rows(sc, cam, width, y0, y1, dstHost);
  });
  return RTG_OK;
}

int rtg_gbuffer_device(rtg_context* ctx, unsigned width, unsigned height, float zoom,
                       float aliasFactor, unsigned rowBlock, unsigned shard, unsigned nShards,
                       rtg_gbuf_px* dstDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  KernelArgs a{};
  int device = 0;
  if (!rtg_context_scene(ctx, &a.scene, &device)) {
    rtg_set_error("gbuffer: no context/scene");
    return RTG_ERR_INVALID;
  }
  if (!dstDevice || ((uintptr_t)dstDevice & 15u) != 0) {
    rtg_set_error(dstDevice ? "gbuffer: destination not 16-byte aligned"
                            : "gbuffer: null destination");
    return RTG_ERR_INVALID;
  }
  int rc = make_camera(width, height, zoom, aliasFactor, &a.cam);
  if (rc) return rc;
  if (rowBlock == 0 || nShards == 0 || shard >= nShards) {
    rtg_set_error("gbuffer: bad sharding %u/%u block %u", shard, nShards, rowBlock);
    return RTG_ERR_INVALID;
  }
  const unsigned rows = shard_row_count(height, rowBlock, shard, nShards);
  if (rows == 0) return RTG_OK;
  if ((double)width * rows >= 0x1p53) {  // divmod_u64's range (rtg_trace_kernels.h)
    rtg_set_error("gbuffer: frame too large (%u x %u)", width, rows);
    return RTG_ERR_INVALID;
  }
  a.W = width;
  a.rowsLocal = rows;
  a.rowBlock = rowBlock;
  a.invW = 1.0 / (double)width;
  a.invRowBlock = 1.0 / (double)rowBlock;
  a.shard = shard;
  a.nShards = nShards;
  const size_t total = (size_t)width * rows;
  const bool sampleKernel = a.cam.nAA >= 1 && a.cam.nAA <= 8;
  // one-wave workgroups: 64 pixel groups each (sample kernel), or 64 pixels
  const unsigned ppw = sampleKernel ? 64u / (unsigned)(a.cam.nAA * a.cam.nAA) : 1u;
  const size_t groups = (total + ppw - 1) / ppw;
  unsigned blocks;
  rc = ray_blocks("gbuffer", "frame", groups, &blocks);
  if (rc) return rc;
  const bool bvh = a.scene.bvhNodes != nullptr;
  void (*fn)(const KernelArgs, size_t, rtg_gbuf_px*) =
      sampleKernel ? (bvh ? gbuffer_samples_kernel<true> : gbuffer_samples_kernel<false>)
                   : (bvh ? gbuffer_pixels_kernel<true> : gbuffer_pixels_kernel<false>);
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, groups, dstDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_gbuffer(int device, const rtg_sphere* spheres, unsigned sphNum, unsigned width,
                unsigned height, float zoom, float aliasFactor, rtg_gbuf_px* dstHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  Camera cam;
  const int rc0 = check_gbuffer_args(spheres, sphNum, width, height, zoom, aliasFactor, dstHost,
                                     &cam);
  if (rc0) return rc0;
  return one_shot("gbuffer", device, {spheres, sphNum, nullptr, 0}, nullptr, 0, dstHost,
                  (size_t)width * height * sizeof(rtg_gbuf_px),
                  [&](rtg_context* ctx, const void*, void* d) {
                    return rtg_gbuffer_device(ctx, width, height, zoom, aliasFactor, 16, 0, 1,
                                              (rtg_gbuf_px*)d, nullptr);
                  });
}

}  // extern "C"
