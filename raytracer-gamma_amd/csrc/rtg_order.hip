// rtg_order.hip — the coherence order of a ray batch (rtg_ray_order*, rtg.h):
// the sort key of every ray (rtg_order.h) and a stable sort of the batch's
// indices by it.  The 64 rays of a wave walk the scene together, so a batch
// in no particular order pays several times over (DESIGN); order[k] names the
// ray that belongs at position k, and the _indexed launches (rtg_rays.hip,
// rtg_raytrace.hip) take it.  Reordering changes no output bit: rays are
// independent.
//
// The device sort is an LSD radix sort of (key, index) pairs with 8-bit digits
// over the key's kKeyBits used bits (kPasses digit positions), one-wave
// workgroups, a tile of kTile = 64 x kRounds keys per workgroup:
//
//   keys     one read of the batch: key(ray i) to keysA[i] (and to the caller's
//            keys buffer), order[i] = i, and the histograms of ALL digit
//            positions at once (per workgroup in LDS, then one vector atomic
//            add per occupied bin: integer sums, the same whatever the order)
//   plan     one wave: per digit position, the exclusive scan of its 256 bin
//            totals, and whether it has a single occupied bin.  Such a
//            position is SKIPPED (sorting by a constant digit is the identity);
//            with the origin-major key every origin position of a batch with
//            one origin goes that way.  The call is asynchronous, so the host
//            cannot know: every pass's kernels are launched and a skipped
//            pass's workgroups return at their first instruction; the plan
//            also tells each executed pass which buffer pair it reads (the
//            parity of the executed passes before it) and whether it is the
//            last (which writes indices only, straight into `order`).
//   per executed pass p
//     hist     per tile, the digit histogram into the bin-major table
//              T[bin][tile]
//     scan     one wave per bin: T[bin][..] to its exclusive prefix over the
//              tiles plus the bin's base, kScanTiles = 256 tiles a step with a
//              running carry
//     scatter  per tile: the running per-digit counters start at T[..][tile]
//              in LDS; 64 keys a round, each lane finds the lanes of its round
//              with the same digit by one __ballot per digit bit, ranks itself
//              among them with mbcnt, takes counter + rank, and the group's
//              last lane advances the counter.  Rounds, lanes and tiles are in
//              batch order, so the sort is stable and the result is the one
//              std::stable_sort gives (the host form), word for word.
//
// Nothing here depends on timing: the only atomics are integer adds into
// histograms (LDS and global vector atomics), every store is a plain vector
// store to an address fixed by the data.  No allocation, no host
// synchronisation, none of the context's render scratch.
//
// Bounds: every access of the batch, the key and index buffers is guarded by
// i < n; a scatter position is a histogram prefix of the same keys, below n by
// construction (and guarded).  T has 256 rows of rowStride = tiles rounded up
// to 4 words, so the scan's 16-byte accesses stay inside a row.
//
// RTG_ORDER_LAYOUT=5d (environment, read per call by the device and the host
// form): the 5-D Morton key of rtg_order.h instead of rtg.h's origin-major one;
// a measurement knob (tools/bench_rays.py, DESIGN), not part of the contract.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rtg.h"
#include "rtg_entry.h"
#include "rtg_trace_kernels.h"
#include "rtg_order.h"
#include "rtg_scene_pack.h"

namespace rtg {

typedef unsigned long long u64;

constexpr int kBins = 256;                      // 8-bit digits
constexpr int kPasses = (kKeyBits + 7) / 8;     // digit positions of the used bits
constexpr int kRounds = RTG_ORDER_TILE_RAYS / 64;
constexpr unsigned kTile = RTG_ORDER_TILE_RAYS;  // keys per workgroup
constexpr unsigned kScanTiles = RTG_ORDER_SCAN_TILES;  // tiles per scan step: 64 lanes x 4
constexpr unsigned kKeyGrid = RTG_ORDER_KEY_GRID;  // workgroups of the keys kernel (tile-strided)
static_assert(kTile == 64u * kRounds && kScanTiles == 256u, "one wave: 64 lanes");
// plan words per pass: {skipped, executed passes before it, is the last executed}
constexpr int kPlanWords = 4;

struct OrderScratch {
  size_t keysA, keysB, idxA, idxB, table, ghist, plan, base, bytes;
  size_t tiles, rowStride;
};

static size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

static OrderScratch order_scratch(size_t n) {
  OrderScratch s;
  s.tiles = (n + kTile - 1) / kTile;
  s.rowStride = (s.tiles + 3u) & ~(size_t)3u;
  size_t at = 0;
  s.keysA = at; at = align16(at + n * sizeof(u64));
  s.keysB = at; at = align16(at + n * sizeof(u64));
  s.idxA = at; at = align16(at + n * sizeof(unsigned));
  s.idxB = at; at = align16(at + n * sizeof(unsigned));
  s.table = at; at = align16(at + (size_t)kBins * s.rowStride * sizeof(unsigned));
  s.ghist = at; at = align16(at + (size_t)kPasses * kBins * sizeof(unsigned));
  s.plan = at; at = align16(at + (size_t)(kPasses * kPlanWords + 4) * sizeof(unsigned));
  s.base = at; at = align16(at + (size_t)kPasses * kBins * sizeof(unsigned));
  s.bytes = at;
  return s;
}

// ---- device side ----

__device__ __forceinline__ unsigned lane_rank(u64 m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Inclusive sum over the wave's lanes.
__device__ __forceinline__ unsigned wave_inclusive(unsigned x) {
  const unsigned lane = threadIdx.x;
  for (unsigned d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(x, d);
    if (lane >= d) x += o;
  }
  return x;
}

// keys: tile-strided over the batch; n > 0, tiles = ceil(n / kTile).
template <bool kSegments, bool kLayout5D>
__global__ __launch_bounds__(64) void order_keys_kernel(const KeyBox box,
                                                        const float* __restrict__ rays, size_t n,
                                                        size_t tiles, u64* __restrict__ keys,
                                                        u64* __restrict__ keysOut,
                                                        unsigned* __restrict__ order,
                                                        unsigned* __restrict__ ghist) {
  __shared__ unsigned h[kPasses * kBins];
  const unsigned lane = threadIdx.x;
  for (unsigned i = lane; i < kPasses * kBins; i += 64) h[i] = 0u;
  __syncthreads();
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    for (int r = 0; r < kRounds; ++r) {
      const size_t i = t * kTile + (size_t)r * 64 + lane;
      const bool valid = i < n;
      u64 key = 0;
      if (valid) {  // i < n: 24 B of the batch, 8 B and 4 B of the buffers
        V3 o, d;
        key_ray_of(rays + 6 * i, kSegments, o, d);
        key = ray_key<kLayout5D>(box, o, d);
        keys[i] = key;
        if (keysOut) keysOut[i] = key;
        order[i] = (unsigned)i;
      }
      const u64 live = __ballot(valid);
      for (int p = 0; p < kPasses; ++p) {
        const unsigned dg = (unsigned)(key >> (8 * p)) & 0xFFu;
        // one digit for the whole round (a constant digit position: the usual
        // case of the origin's): one add instead of 64 on one LDS word
        const unsigned first = __builtin_amdgcn_readfirstlane(dg);
        if (__all(!valid || dg == first)) {
          if (valid && lane_rank(live) == 0u) h[p * kBins + dg] += (unsigned)__popcll(live);
        } else if (valid) {
          atomicAdd(&h[p * kBins + dg], 1u);
        }
      }
      __syncthreads();  // the plain add above against the next round's atomics
    }
  }
  __syncthreads();
  for (unsigned i = lane; i < kPasses * kBins; i += 64) {
    const unsigned c = h[i];
    if (c) atomicAdd(&ghist[i], c);
  }
}

// plan: one wave.  plan[p] = {skipped, executed before p, last executed, -},
// plan[kPasses * kPlanWords] = executed passes; base[p][bin] = keys of the
// batch with a smaller digit at position p.
__global__ __launch_bounds__(64) void order_plan_kernel(const unsigned* __restrict__ ghist,
                                                        size_t n, unsigned* __restrict__ plan,
                                                        unsigned* __restrict__ base) {
  const unsigned lane = threadIdx.x;
  unsigned executed = 0, lastPass = 0;
  for (int p = 0; p < kPasses; ++p) {
    unsigned c[4], s = 0;
    bool single = false;
    for (int j = 0; j < 4; ++j) {
      c[j] = ghist[p * kBins + 4 * lane + j];
      single = single || c[j] == (unsigned)n;  // n <= 2^32 - 1: every key in one bin
      s += c[j];
    }
    const bool skip = __any(single);
    unsigned run = wave_inclusive(s) - s;
    for (int j = 0; j < 4; ++j) {
      base[p * kBins + 4 * lane + j] = run;
      run += c[j];
    }
    if (lane == 0) {
      plan[p * kPlanWords + 0] = skip ? 1u : 0u;
      plan[p * kPlanWords + 1] = executed;
      plan[p * kPlanWords + 2] = 0u;
      plan[p * kPlanWords + 3] = 0u;
    }
    if (!skip) {
      ++executed;
      lastPass = (unsigned)p;
    }
  }
  if (lane == 0) {
    if (executed) plan[lastPass * kPlanWords + 2] = 1u;
    plan[kPasses * kPlanWords] = executed;
  }
}

// hist: one tile per workgroup; T[bin * rowStride + tile] = the tile's keys
// with digit `bin` at position p.
__global__ __launch_bounds__(64) void order_hist_kernel(const unsigned* __restrict__ plan, int p,
                                                        const u64* __restrict__ keysA,
                                                        const u64* __restrict__ keysB, size_t n,
                                                        size_t rowStride,
                                                        unsigned* __restrict__ table) {
  if (plan[p * kPlanWords]) return;  // a constant digit: the pass is skipped
  __shared__ unsigned h[kBins];
  const unsigned lane = threadIdx.x;
  const size_t tile = blockIdx.x;
  const u64* src = (plan[p * kPlanWords + 1] & 1u) ? keysB : keysA;
  for (int j = 0; j < 4; ++j) h[lane + 64 * j] = 0u;
  __syncthreads();
  for (int r = 0; r < kRounds; ++r) {
    const size_t i = tile * kTile + (size_t)r * 64 + lane;
    if (i < n) atomicAdd(&h[(unsigned)(src[i] >> (8 * p)) & 0xFFu], 1u);
  }
  __syncthreads();
  for (int j = 0; j < 4; ++j) {  // tile < tiles <= rowStride
    const unsigned b = lane + 64 * j;
    table[(size_t)b * rowStride + tile] = h[b];
  }
}

// scan: one wave per bin; its row of T becomes base + the exclusive prefix
// over the tiles, kScanTiles tiles a step.
__global__ __launch_bounds__(64) void order_scan_kernel(const unsigned* __restrict__ plan, int p,
                                                        const unsigned* __restrict__ base,
                                                        size_t tiles, size_t rowStride,
                                                        unsigned* __restrict__ table) {
  if (plan[p * kPlanWords]) return;
  const unsigned lane = threadIdx.x;
  const unsigned bin = blockIdx.x;
  unsigned carry = base[p * kBins + bin];
  unsigned* row = table + (size_t)bin * rowStride;  // 16-byte aligned: rowStride % 4 == 0
  for (size_t t0 = 0; t0 < tiles; t0 += kScanTiles) {
    const size_t t = t0 + 4 * (size_t)lane;
    const bool in = t < rowStride;  // then t + 3 < rowStride: inside the row
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (in) v = *reinterpret_cast<const uint4*>(row + t);
    if (t + 0 >= tiles) v.x = 0u;  // the row's padding words hold nothing
    if (t + 1 >= tiles) v.y = 0u;
    if (t + 2 >= tiles) v.z = 0u;
    if (t + 3 >= tiles) v.w = 0u;
    const unsigned s = v.x + v.y + v.z + v.w;
    const unsigned incl = wave_inclusive(s);
    uint4 o;
    o.x = carry + (incl - s);
    o.y = o.x + v.x;
    o.z = o.y + v.y;
    o.w = o.z + v.z;
    if (in) *reinterpret_cast<uint4*>(row + t) = o;
    carry += __shfl(incl, 63);
  }
}

// scatter: one tile per workgroup, stable.
__global__ __launch_bounds__(64) void order_scatter_kernel(
    const unsigned* __restrict__ plan, int p, u64* __restrict__ keysA, u64* __restrict__ keysB,
    unsigned* __restrict__ idxA, unsigned* __restrict__ idxB, unsigned* __restrict__ order,
    size_t n, size_t rowStride, const unsigned* __restrict__ table) {
  if (plan[p * kPlanWords]) return;
  __shared__ unsigned cnt[kBins];
  const unsigned lane = threadIdx.x;
  const size_t tile = blockIdx.x;
  const unsigned before = plan[p * kPlanWords + 1];
  const bool last = plan[p * kPlanWords + 2] != 0u;
  const bool odd = (before & 1u) != 0u;
  const u64* srcK = odd ? keysB : keysA;
  const unsigned* srcI = before == 0u ? nullptr : (odd ? idxB : idxA);  // none yet: i itself
  u64* dstK = odd ? keysA : keysB;
  unsigned* dstI = last ? order : (odd ? idxA : idxB);
  for (int j = 0; j < 4; ++j) {
    const unsigned b = lane + 64 * j;
    cnt[b] = table[(size_t)b * rowStride + tile];
  }
  u64 key[kRounds];
  unsigned idx[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const size_t i = tile * kTile + (size_t)r * 64 + lane;
    key[r] = 0;
    idx[r] = 0;
    if (i < n) {
      key[r] = srcK[i];
      idx[r] = srcI ? srcI[i] : (unsigned)i;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const size_t i = tile * kTile + (size_t)r * 64 + lane;
    const bool valid = i < n;
    const unsigned dg = (unsigned)(key[r] >> (8 * p)) & 0xFFu;
    u64 peers = __ballot(valid);  // the lanes of this round with my digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = ((dg >> b) & 1u) != 0u;
      const u64 set = __ballot(valid && bit);
      peers &= bit ? set : ~set;
    }
    const unsigned rank = lane_rank(peers);
    const unsigned group = (unsigned)__popcll(peers);
    unsigned pos = 0;
    if (valid) pos = cnt[dg] + rank;
    __syncthreads();
    if (valid && rank + 1u == group) cnt[dg] += group;  // one lane per digit
    __syncthreads();
    if (valid && pos < n) {  // a prefix of the same keys' histogram: below n
      dstI[pos] = idx[r];
      if (!last) dstK[pos] = key[r];
    }
  }
}

// ---- host form ----

static bool layout_5d() {
  const char* e = getenv("RTG_ORDER_LAYOUT");
  return e && (strcmp(e, "5d") == 0 || strcmp(e, "5D") == 0);
}

template <bool kLayout5D>
static void keys_host_range(const KeyBox& box, const float* rays, bool segments, size_t k0,
                            size_t k1, u64* keys) {
  for (size_t i = k0; i < k1; ++i) {
    V3 o, d;
    key_ray_of(rays + 6 * i, segments, o, d);
    keys[i] = ray_key<kLayout5D>(box, o, d);
  }
}

}  // namespace rtg

using namespace rtg;

static int check_kind(int kind) {
  if (kind != RTG_ORDER_RAYS && kind != RTG_ORDER_SEGMENTS) {
    rtg_set_error("ray_order: kind %d (0: rays, 1: segments)", kind);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

static int check_count(size_t n) {
  if (n > 0xFFFFFFFFull) {
    rtg_set_error("ray_order: %zu rays (at most 2^32 - 1: indices are 32 bits)", n);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

extern "C" {

int rtg_ray_order_scratch(size_t n, size_t* bytes) {
  rtg_clear_error();
  if (!bytes) {
    rtg_set_error("ray_order_scratch: null result");
    return RTG_ERR_INVALID;
  }
  const int rc = check_count(n);
  if (rc) return rc;
  *bytes = order_scratch(n).bytes;
  return RTG_OK;
}

int rtg_ray_order_host(const rtg_sphere* spheres, unsigned sphNum, const void* rays, size_t n,
                       int kind, unsigned* orderHost, unsigned long long* keysHost, int nthreads) {
  rtg_clear_error();
  if (!rays || !orderHost) {
    rtg_set_error("ray_order: null %s buffer", rays ? "order" : "ray");
    return RTG_ERR_INVALID;
  }
  int rc = check_scene_arrays("ray_order", spheres, sphNum);
  if (!rc) rc = check_kind(kind);
  if (!rc) rc = check_count(n);
  if (rc) return rc;
  if (n == 0) return RTG_OK;
  float lo[3], hi[3];
  key_bounds(spheres, sphNum, lo, hi);  // as rtg_context_set_scene
  const KeyBox box = key_box(lo, hi);
  std::vector<u64> own;
  u64* keys = keysHost;
  if (!keys) {
    own.resize(n);
    keys = own.data();
  }
  const float* r = static_cast<const float*>(rays);
  const bool seg = kind == RTG_ORDER_SEGMENTS;
  const bool l5 = layout_5d();
  host_bands(n, nthreads, [&](size_t k0, size_t k1) {
    if (l5) keys_host_range<true>(box, r, seg, k0, k1, keys);
    else keys_host_range<false>(box, r, seg, k0, k1, keys);
  });
  for (size_t i = 0; i < n; ++i) orderHost[i] = (unsigned)i;
  std::stable_sort(orderHost, orderHost + n,
                   [keys](unsigned a, unsigned b) { return keys[a] < keys[b]; });
  return RTG_OK;
}

int rtg_ray_order_device(rtg_context* ctx, const void* raysDevice, size_t n, int kind,
                         unsigned* orderDevice, unsigned long long* keysDevice,
                         void* scratchDevice, size_t scratchBytes, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  SceneTables a{};
  KeyBox box{};
  int device = 0;
  if (!rtg_context_scene(ctx, &a, &device, nullptr, nullptr, &box)) {
    rtg_set_error("ray_order: no context/scene");
    return RTG_ERR_INVALID;
  }
  if (!raysDevice || !orderDevice || !scratchDevice) {
    rtg_set_error("ray_order: null %s buffer",
                  !raysDevice ? "ray" : (!orderDevice ? "order" : "scratch"));
    return RTG_ERR_INVALID;
  }
  int rc = check_kind(kind);
  if (!rc) rc = check_count(n);
  if (rc) return rc;
  const OrderScratch s = order_scratch(n);
  if (scratchBytes < s.bytes) {
    rtg_set_error("ray_order: scratch of %zu bytes, %zu needed (rtg_ray_order_scratch)",
                  scratchBytes, s.bytes);
    return RTG_ERR_INVALID;
  }
  if (((uintptr_t)scratchDevice & 15u) != 0) {
    rtg_set_error("ray_order: scratch not 16-byte aligned");
    return RTG_ERR_INVALID;
  }
  if (n == 0) return RTG_OK;
  char* sc = static_cast<char*>(scratchDevice);
  u64* keysA = reinterpret_cast<u64*>(sc + s.keysA);
  u64* keysB = reinterpret_cast<u64*>(sc + s.keysB);
  unsigned* idxA = reinterpret_cast<unsigned*>(sc + s.idxA);
  unsigned* idxB = reinterpret_cast<unsigned*>(sc + s.idxB);
  unsigned* table = reinterpret_cast<unsigned*>(sc + s.table);
  unsigned* ghist = reinterpret_cast<unsigned*>(sc + s.ghist);
  unsigned* plan = reinterpret_cast<unsigned*>(sc + s.plan);
  unsigned* base = reinterpret_cast<unsigned*>(sc + s.base);
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)s.tiles;  // <= 2^22
  const bool seg = kind == RTG_ORDER_SEGMENTS;
  const bool l5 = layout_5d();
  void (*keysFn)(const KeyBox, const float*, size_t, size_t, u64*, u64*, unsigned*, unsigned*) =
      seg ? (l5 ? order_keys_kernel<true, true> : order_keys_kernel<true, false>)
          : (l5 ? order_keys_kernel<false, true> : order_keys_kernel<false, false>);
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemsetAsync(ghist, 0, (size_t)kPasses * kBins * sizeof(unsigned), st));
  hipLaunchKernelGGL(keysFn, dim3(tiles < kKeyGrid ? tiles : kKeyGrid), dim3(64), 0, st, box,
                     static_cast<const float*>(raysDevice), n, s.tiles, keysA,
                     reinterpret_cast<u64*>(keysDevice), orderDevice, ghist);
  hipLaunchKernelGGL(order_plan_kernel, dim3(1), dim3(64), 0, st, ghist, n, plan, base);
  for (int p = 0; p < kPasses; ++p) {
    hipLaunchKernelGGL(order_hist_kernel, dim3(tiles), dim3(64), 0, st, plan, p, keysA, keysB, n,
                       s.rowStride, table);
    hipLaunchKernelGGL(order_scan_kernel, dim3(kBins), dim3(64), 0, st, plan, p, base, s.tiles,
                       s.rowStride, table);
    hipLaunchKernelGGL(order_scatter_kernel, dim3(tiles), dim3(64), 0, st, plan, p, keysA, keysB,
                       idxA, idxB, orderDevice, n, s.rowStride, table);
  }
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

}  // extern "C"
