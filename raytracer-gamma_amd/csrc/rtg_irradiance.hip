// rtg_irradiance.hip — the probe grid's consumer of librtg.so (rtg_irradiance*,
// rtg_probe_grid_points, rtg_probe_grid_poses, rtg.h): hit points in, the light
// of a lattice of SH probes at each point out, with the weight that was left.
//
// Point i starts at A = P + bias N (ao_point, rtg_ao.h: rtg_ao*'s start
// point), finds its cell of the lattice (irr_axis per axis), evaluates the SH
// basis along N once (irr_basis) and goes through the cell's eight corners in
// order (irr_point: ONE definition for the kernel and both host walks).  A
// corner is left out when its trilinear weight is not > 0, when its validity
// byte is 0 (RTG_IRR_VALID), when it is not in front of the point's tangent
// plane (RTG_IRR_FACING) or when the point does not see it (RTG_IRR_VISIBLE):
// hasClearLineOfSight(A, X_p), the line of sight of rtg_visible (segment_ray
// and ray_blocked, rtg_rays.h).  The fused result is therefore a function of
// rtg_visible_host(walk 0) over the n x 8 segments (A, X_p), with no segment
// buffer, no gather and no fold on the caller's side.
//
// irradiance_kernel: one lane per point in one-wave workgroups, the wave's BVH
// stack in LDS (matte_kernel's mapping, rtg_matte.hip).  The loop over the
// corners is wave-uniform.  The eight segments of a point share their origin,
// so ray_delta of A is taken once (MattePath's argument) and ray_blocked's
// overload takes it.  The query has no side effect, so it runs after the other
// tests: a lane whose corner is already left out (and lanes past n, and
// records with id < 0) enters the walk as an inactive query (never blocked),
// and a corner no lane of the wave still needs makes no walk at all
// (sc.any).  kScene: 0 no query (no RTG_IRR_VISIBLE: the kernel reads no scene
// table and the context needs no scene), 1 the flat scene, 2 the BVH.  kBands
// is a template parameter: K = kBands^2 is then a constant, the basis b_0 ..
// b_{K-1} stays in registers (a runtime K indexes it, which puts it in
// scratch) and the loop over a probe's coefficients unrolls.  The three flags
// are wave-uniform branches on a kernel argument.
//
// A probe's coefficients are 12 K contiguous bytes at a per-lane address, read
// as words (no alignment beyond a float's is asked of the caller's table).
// Lanes of a coherent frame share cells, so the table lives in cache.
//
// Bounds.  Per axis q: g is clamped to [0, n_q - 1] before it is converted (NaN
// goes to 0, n_q <= 2^20 is exact in float), so i0 <= n_q - 1 and i1 = min(i0 +
// 1, n_q - 1): both < n_q for every lane, active or not, whatever the record
// holds.  So p = (iz ny + iy) nx + ix < nx ny nz, the validity byte valid[p] is
// inside its nx ny nz bytes, and p K + k <= nx ny nz K - 1 <= 2^31 - 2 is
// inside the table (the entry points check the product; the index is formed in
// size_t).  A record index is < n (lanes past n read record n - 1 and store
// nothing), an output and a weight index < n.
//
// Host forms: walk 0 = the plain loops, the yardstick (blocked over every
// sphere of the caller's array); walk 1 = the kernel's own path over the
// packed tables, one point per "wave".
//
// FP contract: the Makefile's FPFLAGS, as every kernel.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rtg.h"
#include "rtg_ao.h"
#include "rtg_entry.h"
#include "rtg_host_scene.h"
#include "rtg_rays.h"
#include "rtg_scene_pack.h"
#include "rtg_trace_kernels.h"

static_assert(sizeof(rtg_probe_grid) == 40 && offsetof(rtg_probe_grid, step) == 12 &&
                  offsetof(rtg_probe_grid, nx) == 24 && offsetof(rtg_probe_grid, bands) == 36,
              "rtg_probe_grid is 40 B");
static_assert(sizeof(rtg_irradiance_params) == 20 && offsetof(rtg_irradiance_params, lobe) == 4 &&
                  offsetof(rtg_irradiance_params, flags) == 16,
              "rtg_irradiance_params is 20 B");
static_assert(sizeof(rtg_hit) == 32 && offsetof(rtg_hit, point) == 8 &&
                  offsetof(rtg_hit, normal) == 20,
              "rtg_hit layout");
static_assert(sizeof(rtg_vec) == 12 && sizeof(rtg_camera) == 48, "12 B per colour, 48 per pose");

namespace rtg {

constexpr unsigned kIrrFlags = RTG_IRR_VALID | RTG_IRR_FACING | RTG_IRR_VISIBLE;
constexpr unsigned kIrrMaxDim = 1u << 20;

// real_sh's constants (rtg_camera.hip) rounded to float.
constexpr float kShC0 = (float)0.28209479177387814;
constexpr float kShC1 = (float)0.4886025119029199;
constexpr float kShC2 = (float)1.0925484305920792;
constexpr float kShC3 = (float)0.31539156525252005;
constexpr float kShC4 = (float)0.5462742152960396;

// One axis of the point's cell: the two lattice indices and the fraction.
struct IrrAxis {
  unsigned i0, i1;
  float f;
};

// rtg.h's `cell` for one axis; n in [1, 2^20].  i0, i1 < n for any a.
RTG_HD IrrAxis irr_axis(float a, float origin, float step, unsigned n) {
  float g = (a - origin) / step;
  if (!(g >= 0.f)) g = 0.f;  // NaN too
  const float top = (float)(n - 1);
  if (g > top) g = top;
  IrrAxis x;
  x.i0 = (unsigned)g;  // 0 <= g <= n - 1 < 2^20
  if (n >= 2 && x.i0 > n - 2) x.i0 = n - 2;
  x.f = g - (float)x.i0;
  x.i1 = x.i0 + 1 < n ? x.i0 + 1 : x.i0;
  return x;
}

// rtg.h's `basis`: b_k = lobe[l] * Y_k(N), the bands above kBands not formed.
template <int kBands>
RTG_HD void irr_basis(const float* lobe, V3 N, float* b) {
  b[0] = lobe[0] * kShC0;
  if constexpr (kBands >= 2) {
    b[1] = lobe[1] * (kShC1 * N.y);
    b[2] = lobe[1] * (kShC1 * N.z);
    b[3] = lobe[1] * (kShC1 * N.x);
  }
  if constexpr (kBands >= 3) {
    b[4] = lobe[2] * (kShC2 * (N.x * N.y));
    b[5] = lobe[2] * (kShC2 * (N.y * N.z));
    b[6] = lobe[2] * (kShC3 * (3.f * (N.z * N.z) - 1.f));
    b[7] = lobe[2] * (kShC2 * (N.x * N.z));
    b[8] = lobe[2] * (kShC4 * (N.x * N.x - N.y * N.y));
  }
}

// Probe index i of an axis in the world.
RTG_HD float irr_coord(float origin, float step, unsigned i) { return origin + (float)i * step; }

// The looked-up light of one point and its weight W.  `live`: the lane has a
// point (i < n and id >= 0); a lane without one keeps every corner out, loads
// nothing and enters every query as inactive.  path.blocked(A, d, gap, need) is
// the line of sight of the lanes that still `need` it; every lane of a wave
// calls it for every corner.
template <int kBands, class Path>
RTG_HD V3 irr_point(const Path& path, const rtg_probe_grid& g, const rtg_irradiance_params& pr,
                    const rtg_vec* __restrict__ coeffs, const unsigned char* __restrict__ valid,
                    V3 A, V3 N, bool live, float& W) {
  constexpr unsigned K = kBands * kBands;
  const IrrAxis ax = irr_axis(A.x, g.origin.x, g.step.x, g.nx);
  const IrrAxis ay = irr_axis(A.y, g.origin.y, g.step.y, g.ny);
  const IrrAxis az = irr_axis(A.z, g.origin.z, g.step.z, g.nz);
  float b[K];
  irr_basis<kBands>(pr.lobe, N, b);
  V3 acc = v3(0.f, 0.f, 0.f);
  W = 0.f;
#pragma unroll 1
  for (unsigned c = 0; c < 8; ++c) {
    const bool cx = (c & 1u) != 0, cy = ((c >> 1) & 1u) != 0, cz = (c >> 2) != 0;
    const unsigned ix = cx ? ax.i1 : ax.i0, iy = cy ? ay.i1 : ay.i0, iz = cz ? az.i1 : az.i0;
    const float tx = cx ? ax.f : 1.f - ax.f;
    const float ty = cy ? ay.f : 1.f - ay.f;
    const float tz = cz ? az.f : 1.f - az.f;
    const float w = (tx * ty) * tz;
    const size_t p = ((size_t)iz * g.ny + iy) * g.nx + ix;  // < nx ny nz (header)
    bool keep = live && w > 0.f;
    if (pr.flags & RTG_IRR_VALID) {
      if (keep) keep = valid[p] != 0;  // p < nx ny nz
    }
    const V3 X = v3(irr_coord(g.origin.x, g.step.x, ix), irr_coord(g.origin.y, g.step.y, iy),
                    irr_coord(g.origin.z, g.step.z, iz));
    if (pr.flags & RTG_IRR_FACING) {
      const V3 d = vsub(X, A);
      const float s = (N.x * d.x + N.y * d.y) + N.z * d.z;
      keep = keep && s > 0.f;
    }
    if constexpr (Path::kOn) {
      if (pr.flags & RTG_IRR_VISIBLE) {  // wave-uniform
        float gap;
        const V3 d = segment_ray(A, X, gap);
        const bool blk = path.blocked(A, d, gap, keep);
        keep = keep && !blk;
      }
    }
    if (keep) {
      const float* t = reinterpret_cast<const float*>(coeffs + p * K);  // p K + k < nx ny nz K
      V3 e = v3(0.f, 0.f, 0.f);
#pragma unroll
      for (unsigned k = 0; k < K; ++k) {
        e.x = e.x + b[k] * t[3 * k];
        e.y = e.y + b[k] * t[3 * k + 1];
        e.z = e.z + b[k] * t[3 * k + 2];
      }
      W = W + w;
      acc.x = acc.x + w * e.x;
      acc.y = acc.y + w * e.y;
      acc.z = acc.z + w * e.z;
    }
  }
  if (W > 0.f) return v3(acc.x / W, acc.y / W, acc.z / W);
  return v3(0.f, 0.f, 0.f);
}

// No query: RTG_IRR_VISIBLE is not set.
struct IrrNoPath {
  static constexpr bool kOn = false;
};

// The kernel's and walk 1's line of sight: ray_blocked with the delta of A,
// taken once; a corner nobody needs makes no walk.
template <bool kBvh, class Scene>
struct IrrPath {
  static constexpr bool kOn = true;
  const Scene& sc;
  float delta = 0.f;
  bool oddOrigin = false;
  RTG_HD bool blocked(V3 o, V3 d, float gap, bool need) const {
    bool blk = false;
    if (sc.any(need)) blk = ray_blocked<kBvh>(sc, o, d, gap, need, delta, oddOrigin);
    return blk;
  }
};

// The plain loops': every sphere of the caller's array.
struct IrrPlainPath {
  static constexpr bool kOn = true;
  HostSpheres sc;
  bool blocked(V3 o, V3 d, float gap, bool need) const {
    return need && rtg::blocked(sc, o, d, gap);
  }
};

// One lane per point; n > 0.  kScene 0: no scene table is read.
template <int kScene, int kBands>
__global__ __launch_bounds__(64) void irradiance_kernel(
    const SceneTables a, const RayBox box, const rtg_hit* __restrict__ hits, size_t n,
    const rtg_probe_grid g, const rtg_irradiance_params pr, const rtg_vec* __restrict__ coeffs,
    const unsigned char* __restrict__ valid, rtg_vec* __restrict__ out,
    float* __restrict__ weight) {
  constexpr bool kBvh = kScene == 2;
  __shared__ int stk[kBvh ? 64 : 1];
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool inside = i < n;
  const AoPoint pt = ao_point(hits + (inside ? i : n - 1), pr.bias);  // < n: a batch record
  const bool live = inside && pt.id >= 0;
  float W;
  V3 v;
  if constexpr (kScene == 0) {
    v = irr_point<kBands>(IrrNoPath{}, g, pr, coeffs, valid, pt.a, pt.N, live, W);
  } else {
    RayScene<kBvh> sc;
    bind_scene_no_frames(sc, a, stk);  // stk: the wave's BVH traversal stack
    IrrPath<kBvh, RayScene<kBvh>> path{sc};
    if constexpr (kBvh) path.delta = ray_delta(box, pt.a, path.oddOrigin);
    v = irr_point<kBands>(path, g, pr, coeffs, valid, pt.a, pt.N, live, W);
  }
  if (inside) {  // i < n; a record without a point: zeros (irr_point kept no corner)
    unsigned* o = reinterpret_cast<unsigned*>(out + i);
    o[0] = nan_bits(v.x);
    o[1] = nan_bits(v.y);
    o[2] = nan_bits(v.z);
  }
  if (weight) {  // wave-uniform: a kernel argument
    if (inside) weight[i] = W;
  }
}

// ---- host forms ----

// Points [i0, i1) over `make_path(A)`'s line of sight.
template <int kBands, class MakePath>
static void irr_host_range(const MakePath& make_path, const rtg_hit* hits, size_t i0, size_t i1,
                           const rtg_probe_grid& g, const rtg_irradiance_params& pr,
                           const rtg_vec* coeffs, const unsigned char* valid, rtg_vec* out,
                           float* weight) {
  for (size_t i = i0; i < i1; ++i) {
    const AoPoint pt = ao_point(hits + i, pr.bias);
    float W = 0.f;
    V3 v = v3(0.f, 0.f, 0.f);
    if (pt.id >= 0)
      v = irr_point<kBands>(make_path(pt.a), g, pr, coeffs, valid, pt.a, pt.N, true, W);
    store_colour(out + i, v);
    if (weight) weight[i] = W;
  }
}

template <class MakePath>
static void irr_host_bands(const MakePath& make_path, const rtg_hit* hits, size_t n,
                           const rtg_probe_grid& g, const rtg_irradiance_params& pr,
                           const rtg_vec* coeffs, const unsigned char* valid, rtg_vec* out,
                           float* weight, int nthreads) {
  host_bands(n, nthreads, [&](size_t i0, size_t i1) {
    if (g.bands == 1) irr_host_range<1>(make_path, hits, i0, i1, g, pr, coeffs, valid, out, weight);
    else if (g.bands == 2)
      irr_host_range<2>(make_path, hits, i0, i1, g, pr, coeffs, valid, out, weight);
    else irr_host_range<3>(make_path, hits, i0, i1, g, pr, coeffs, valid, out, weight);
  });
}

}  // namespace rtg

using namespace rtg;

static bool finite3(const rtg_vec& v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// The grid alone (the two conveniences check no more).
static int check_grid(const char* what, const rtg_probe_grid* g) {
  if (!g) {
    rtg_set_error("%s: null grid", what);
    return RTG_ERR_INVALID;
  }
  if (!finite3(g->origin)) {
    rtg_set_error("%s: grid origin is not finite", what);
    return RTG_ERR_INVALID;
  }
  if (!(finite3(g->step) && g->step.x > 0.f && g->step.y > 0.f && g->step.z > 0.f)) {
    rtg_set_error("%s: grid step (%g, %g, %g) is not finite and > 0", what, (double)g->step.x,
                  (double)g->step.y, (double)g->step.z);
    return RTG_ERR_INVALID;
  }
  if (g->nx < 1 || g->ny < 1 || g->nz < 1 || g->nx > kIrrMaxDim || g->ny > kIrrMaxDim ||
      g->nz > kIrrMaxDim) {
    rtg_set_error("%s: grid dims %u x %u x %u outside [1, 2^20]", what, g->nx, g->ny, g->nz);
    return RTG_ERR_INVALID;
  }
  if (g->bands < 1 || g->bands > 3) {
    rtg_set_error("%s: %u bands outside [1, 3]", what, g->bands);
    return RTG_ERR_INVALID;
  }
  // nx ny <= 2^40 and nz K <= 9 2^20: no overflow in 128 bits, checked in two steps
  const unsigned long long K = (unsigned long long)g->bands * g->bands;
  const unsigned long long plane = (unsigned long long)g->nx * g->ny;
  if (plane > 0x7FFFFFFFull || plane * g->nz > 0x7FFFFFFFull || plane * g->nz * K > 0x7FFFFFFFull) {
    rtg_set_error("%s: grid of %u x %u x %u probes of %llu coefficients (at most 2^31 - 1 in all)",
                  what, g->nx, g->ny, g->nz, K);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

// The checks every form shares, in the order they are reported in.
static int check_irradiance(const rtg_hit* hits, size_t n, const rtg_probe_grid* g,
                            const rtg_vec* coeffs, const unsigned char* valid,
                            const rtg_irradiance_params* p, const rtg_vec* out) {
  const char* what = "irradiance";
  if (!hits || !coeffs || !p || !out) {
    rtg_set_error("%s: null %s", what,
                  !hits ? "hit buffer" : !coeffs ? "coefficient table" : !p ? "params"
                                                                           : "output buffer");
    return RTG_ERR_INVALID;
  }
  const int rc = check_grid(what, g);
  if (rc) return rc;
  if (p->flags & ~kIrrFlags) {
    rtg_set_error("%s: unknown flag bits 0x%x", what, p->flags & ~kIrrFlags);
    return RTG_ERR_INVALID;
  }
  if ((p->flags & RTG_IRR_VALID) && !valid) {
    rtg_set_error("%s: RTG_IRR_VALID with a null validity table", what);
    return RTG_ERR_INVALID;
  }
  if (n > 0xFFFFFFFFull) {
    rtg_set_error("%s: %zu points (at most 2^32 - 1)", what, n);
    return RTG_ERR_INVALID;
  }
  return RTG_OK;
}

typedef void (*IrrKernel)(const SceneTables, const RayBox, const rtg_hit*, size_t,
                          const rtg_probe_grid, const rtg_irradiance_params, const rtg_vec*,
                          const unsigned char*, rtg_vec*, float*);

template <int kScene>
static IrrKernel irr_kernel_of(unsigned bands) {
  return bands == 1 ? irradiance_kernel<kScene, 1>
                    : bands == 2 ? irradiance_kernel<kScene, 2> : irradiance_kernel<kScene, 3>;
}

extern "C" {

int rtg_probe_grid_points(const rtg_probe_grid* grid, rtg_vec* out) {
  rtg_clear_error();
  int rc = check_grid("probe_grid_points", grid);
  if (!rc && !out) {
    rtg_set_error("probe_grid_points: null output");
    rc = RTG_ERR_INVALID;
  }
  if (rc) return rc;
  const rtg_probe_grid g = *grid;
  size_t p = 0;
  for (unsigned iz = 0; iz < g.nz; ++iz)
    for (unsigned iy = 0; iy < g.ny; ++iy)
      for (unsigned ix = 0; ix < g.nx; ++ix, ++p) {
        out[p].x = irr_coord(g.origin.x, g.step.x, ix);
        out[p].y = irr_coord(g.origin.y, g.step.y, iy);
        out[p].z = irr_coord(g.origin.z, g.step.z, iz);
      }
  return RTG_OK;
}

int rtg_probe_grid_poses(const rtg_probe_grid* grid, rtg_camera* out) {
  rtg_clear_error();
  int rc = check_grid("probe_grid_poses", grid);
  if (!rc && !out) {
    rtg_set_error("probe_grid_poses: null output");
    rc = RTG_ERR_INVALID;
  }
  if (rc) return rc;
  const rtg_probe_grid g = *grid;
  size_t p = 0;
  for (unsigned iz = 0; iz < g.nz; ++iz)
    for (unsigned iy = 0; iy < g.ny; ++iy)
      for (unsigned ix = 0; ix < g.nx; ++ix, ++p) {
        const rtg_vec eye = {irr_coord(g.origin.x, g.step.x, ix),
                             irr_coord(g.origin.y, g.step.y, iy),
                             irr_coord(g.origin.z, g.step.z, iz)};
        rc = rtg_camera_cube(&eye, out + 6 * p);
        if (rc) return rc;
      }
  return RTG_OK;
}

int rtg_irradiance_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                          const rtg_probe_grid* grid, const rtg_vec* coeffsDevice,
                          const unsigned char* validDevice, const rtg_irradiance_params* params,
                          rtg_vec* outDevice, float* weightDevice, void* stream) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int device = 0;
  if (!rtg_context_device(ctx, &device)) {
    rtg_set_error("irradiance: no context");
    return RTG_ERR_INVALID;
  }
  int rc = check_irradiance(hitsDevice, n, grid, coeffsDevice, validDevice, params, outDevice);
  if (rc) return rc;
  SceneTables a{};
  RayBox box{};
  const bool query = (params->flags & RTG_IRR_VISIBLE) != 0;
  if (query && !rtg_context_scene(ctx, &a, &device, &box)) {
    rtg_set_error("irradiance: RTG_IRR_VISIBLE on a context without a scene");
    return RTG_ERR_INVALID;
  }
  if (n == 0) return RTG_OK;
  unsigned blocks;
  rc = ray_blocks("irradiance", "batch", n, &blocks);
  if (rc) return rc;
  const IrrKernel fn = !query ? irr_kernel_of<0>(grid->bands)
                              : a.bvhNodes ? irr_kernel_of<2>(grid->bands)
                                           : irr_kernel_of<1>(grid->bands);
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a, box, hitsDevice, n,
                     *grid, *params, coeffsDevice, validDevice, outDevice, weightDevice);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_irradiance_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits, size_t n,
                        const rtg_probe_grid* grid, const rtg_vec* coeffs,
                        const unsigned char* valid, const rtg_irradiance_params* params,
                        rtg_vec* outHost, float* weightHost, int walk, int nthreads) {
  rtg_clear_error();
  int rc = check_irradiance(hits, n, grid, coeffs, valid, params, outHost);
  if (!rc) rc = check_scene_arrays("irradiance", spheres, sphNum);
  if (!rc) rc = check_walk("irradiance", walk);
  if (!rc && walk == 1) rc = check_sphere_count("irradiance", sphNum);
  if (rc || n == 0) return rc;
  const rtg_probe_grid g = *grid;
  const rtg_irradiance_params p = *params;
  auto run = [&](const auto& make_path) {
    irr_host_bands(make_path, hits, n, g, p, coeffs, valid, outHost, weightHost, nthreads);
  };
  if (!(p.flags & RTG_IRR_VISIBLE)) {
    run([](V3) { return IrrNoPath{}; });
  } else if (walk == 0) {
    const HostSpheres sc{spheres, sphNum};
    run([&](V3) { return IrrPlainPath{sc}; });
  } else {
    PackedScene ps;
    pack_scene(spheres, sphNum, nullptr, 0, &ps);  // as rtg_context_set_scene
    if (!ps.bvhNodes.empty()) {
      const RayBox box = ray_box(ps.originBox);
      const HostScene<true> sc(ps, true);
      run([&](V3 A) {
        IrrPath<true, HostScene<true>> path{sc};
        path.delta = ray_delta(box, A, path.oddOrigin);
        return path;
      });
    } else {
      const HostScene<false> sc(ps, true);
      run([&](V3) { return IrrPath<false, HostScene<false>>{sc}; });
    }
  }
  return RTG_OK;
}

int rtg_irradiance(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits,
                   size_t n, const rtg_probe_grid* grid, const rtg_vec* coeffs,
                   const unsigned char* valid, const rtg_irradiance_params* params,
                   rtg_vec* outHost, float* weightHost) {
  DeviceGuard deviceGuard;  // the caller's current device is restored on return
  rtg_clear_error();
  int rc = check_irradiance(hits, n, grid, coeffs, valid, params, outHost);
  if (!rc) rc = check_scene_arrays("irradiance", spheres, sphNum);
  if (rc || n == 0) return rc;
  const size_t probes = (size_t)grid->nx * grid->ny * grid->nz;
  const StageScene scene{spheres, sphNum, nullptr, 0};
  return one_shot("irradiance", device, &scene,
                  {{n * sizeof(rtg_hit), hits, nullptr},
                   {probes * grid->bands * grid->bands * sizeof(rtg_vec), coeffs, nullptr},
                   {valid ? probes : 0, valid, nullptr},
                   {n * sizeof(rtg_vec), nullptr, outHost},
                   {weightHost ? n * sizeof(float) : 0, nullptr, weightHost}},
                  [&](rtg_context* ctx, void* const* d) {
                    return rtg_irradiance_device(ctx, (const rtg_hit*)d[0], n, grid,
                                                 (const rtg_vec*)d[1],
                                                 (const unsigned char*)d[2], params,
                                                 (rtg_vec*)d[3], (float*)d[4], nullptr);
                  });
}

}  // extern "C"
