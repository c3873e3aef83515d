// rtg_gather_kernels.h — the gather (rtg_gather*, rtg.h): what its generator,
// its fused kernel and both host walks share (the probe ray and one step of
// the sum, each written ONCE), and the fused kernel as a template over the
// stack capacity S, instantiated next to raytrace_kernel in rtg_trace_s<S>.hip
// (gather_fn<S>).  The launcher, the generator kernel, the host forms and the
// one-shot are in rtg_gather.hip.
#pragma once

#include "rtg_ao.h"
#include "rtg_fold.h"
#include "rtg_raytrace_kernels.h"

static_assert(RTG_GATHER_JITTER == RTG_AO_JITTER, "ao_window reads the jitter bit");
static_assert(RTG_GATHER_MAX_SAMPLES == RTG_AO_MAX_SAMPLES &&
                  RTG_GATHER_MAX_DIRS == RTG_AO_MAX_DIRS,
              "check_probes (rtg_probes.h) states one pair of limits");

namespace rtg {

// Probe k's direction for the local direction l: rtg_ao's world vector through
// the posed camera's vnorm (camera_dir, rtg_camera.h).  The origin is pt.a.
RTG_HD V3 gather_dir(const AoPoint& pt, V3 l) { return vnorm(ao_world(pt, l)); }

// One step of the sum, acc.q = acc.q + w * c.q; with `skip`
// (RTG_GATHER_SKIP_NONFINITE) a colour with a NaN or infinite word adds +0.f
// to every channel and is counted.  The weight is never tested.
RTG_HD void gather_add(V3& acc, unsigned& skipped, float w, V3 c, bool skip) {
  V3 t = v3(w * c.x, w * c.y, w * c.z);
  if (skip && (fold_nonfinite(c.x) || fold_nonfinite(c.y) || fold_nonfinite(c.z))) {
    t = v3(0.f, 0.f, 0.f);
    ++skipped;
  }
  acc = v3(acc.x + t.x, acc.y + t.y, acc.z + t.z);
}

// The kernel's arguments besides the scene: the batch, the two tables and the
// two results (`skipped` may be null).
struct GatherArgs {
  const rtg_hit* hits;
  size_t n;
  rtg_gather_params p;
  const rtg_vec* dirs;
  const float* weights;
  unsigned nDirs;
  rtg_vec* out;
  unsigned short* skipped;
};

// One lane per point, one-wave workgroups; n > 0.  The LDS image and the scene
// binding are raytrace_kernel's.  The frame and a are taken once per point,
// and the loop over k is wave-uniform: a wave's 64 lanes sit on neighbouring
// points and all ask for local direction k, which for a coherent batch of hits
// are similar rays, the case the tracer is fast at.  Lanes past n and records
// with id < 0 step round the loop, as raytrace_kernel lets lanes past n leave
// before the trace: the queries' wave-level tests (all / any, the wave-uniform
// BVH walk and its LDS stack) are over the lanes present, so a traced probe is
// raytrace_kernel's bit for bit.
//
// The tables: k < K <= nDirs indexes both for the whole wave, so entry k is
// read through a wave-uniform address (scalar loads, as ao_kernel's).  With
// RTG_GATHER_JITTER (a kernel argument: the branch is wave-uniform, and the
// trace is compiled once, not once per flag) each lane then reads its own
// entry j < nDirs of its window instead.  Both tables are only read and are
// complete before the launch.  Bounds: a record index is < n (lanes past n
// read record n - 1 and store nothing), a table index < nDirs (ao_dir_index),
// an output index < n.
template <int S, bool kBvh, bool kCL>
__global__ __launch_bounds__(64) void gather_kernel(const SceneTables a, const RayBox box,
                                                    const GatherArgs g) {
  extern __shared__ float4 lds4[];
  RayScene<kBvh> sc;
  bind_raytrace_scene<S>(sc, a, lds4);
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool inside = i < g.n;
  const AoPoint pt = ao_point(g.hits + (inside ? i : g.n - 1), g.p.bias);  // < n: a batch record
  const bool jitter = (g.p.flags & RTG_GATHER_JITTER) != 0;
  const bool skip = (g.p.flags & RTG_GATHER_SKIP_NONFINITE) != 0;
  V3 acc = v3(0.f, 0.f, 0.f);
  unsigned skipped = 0;
  if (inside && pt.id >= 0) {
    const unsigned s = ao_window(g.p.flags, g.p.seed, i, g.nDirs);
    for (unsigned k = 0; k < g.p.samples; ++k) {
      V3 l = ao_dir(g.dirs, k);  // k for the whole wave, a scalar load; k < K <= nDirs
      float w = g.weights[k];
      if (jitter) {
        const unsigned j = ao_dir_index(s, k, g.nDirs);  // < nDirs
        l = ao_dir(g.dirs, j);
        w = g.weights[j];
      }
      const V3 c = trace_ray<S, kCL, kBvh>(sc, box, pt.a, gather_dir(pt, l));
      gather_add(acc, skipped, w, c, skip);
    }
  }
  if (!inside) return;
  store_colour_dev(g.out + i, acc);  // i < n: 12 B of out
  if (g.skipped) g.skipped[i] = (unsigned short)skipped;  // <= K <= 1024
}

// bvh: the scene has a BVH (SceneTables::bvhNodes); cl: RTG_SEMANTICS_OPENCL.
template <int S>
static GatherFn gather_fn(bool bvh, bool cl) {
  if (bvh) return cl ? gather_kernel<S, true, true> : gather_kernel<S, true, false>;
  return cl ? gather_kernel<S, false, true> : gather_kernel<S, false, false>;
}

}  // namespace rtg
