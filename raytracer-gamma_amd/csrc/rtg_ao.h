// rtg_ao.h — the ambient-occlusion probe (rtg_ao*, rtg.h), written ONCE for the
// segment generator, the fused kernel and both host walks (rtg_ao.hip), and
// for the gather's probe rays (rtg_gather*, rtg_gather.h), as
// camera_dir (rtg_camera.h) is for the posed camera: the window hash, the
// tangent frame of a normal, the window index and the probe's end points, in
// the operand order rtg.h states.  No libm call: copysignf is a bit operation
// and the one division is the correctly rounded one on both sides.
#pragma once

#include <math.h>
#include <stddef.h>
#include <string.h>

#include "rtg.h"
#include "rtg_trace.h"

namespace rtg {

RTG_HD unsigned ao_mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// What depends on the point alone: the probes' common start a = P + bias N and
// the frame (T1, T2, N) of its normal.  id < 0: no point.
struct AoPoint {
  int id;
  V3 a, T1, T2, N;
};

RTG_HD AoPoint ao_point(int id, V3 P, V3 N, float bias) {
  AoPoint p;
  p.id = id;
  p.N = N;
  const float s = copysignf(1.f, N.z);
  const float a = -1.f / (s + N.z);
  const float b = (N.x * N.y) * a;
  p.T1 = v3(1.f + s * ((N.x * N.x) * a), s * b, -(s * N.x));
  p.T2 = v3(b, s + (N.y * N.y) * a, -N.y);
  p.a = v3(P.x + bias * N.x, P.y + bias * N.y, P.z + bias * N.z);
  return p;
}

// The point of a hit record as rtg_intersect* writes it (32 B, read as words:
// no alignment beyond a float's is asked of the caller's buffer).
RTG_HD AoPoint ao_point(const rtg_hit* hit, float bias) {
  const float* w = reinterpret_cast<const float*>(hit);
  int id;
  memcpy(&id, w, 4);
  return ao_point(id, v3(w[2], w[3], w[4]), v3(w[5], w[6], w[7]), bias);
}

// s_i of point i, and the table index of its probe k (s < nDirs, k < K <=
// nDirs: j < 2 nDirs, one subtraction wraps it).
RTG_HD unsigned ao_window(unsigned flags, unsigned seed, size_t i, unsigned nDirs) {
  return (flags & RTG_AO_JITTER) ? ao_mix32(seed + (unsigned)i) % nDirs : 0u;
}
RTG_HD unsigned ao_window(const rtg_ao_params& p, size_t i, unsigned nDirs) {
  return ao_window(p.flags, p.seed, i, nDirs);
}
RTG_HD unsigned ao_dir_index(unsigned s, unsigned k, unsigned nDirs) {
  const unsigned j = s + k;
  return j >= nDirs ? j - nDirs : j;
}

// Entry j < nDirs of the caller's table of local directions.
RTG_HD V3 ao_dir(const rtg_vec* dirs, unsigned j) {
  const float* t = reinterpret_cast<const float*>(dirs + j);
  return v3(t[0], t[1], t[2]);
}

// The local direction l in the world: rtg.h's `world` (rtg_gather's too).
RTG_HD V3 ao_world(const AoPoint& p, V3 l) {
  return v3((l.x * p.T1.x + l.y * p.T2.x) + l.z * p.N.x,
            (l.x * p.T1.y + l.y * p.T2.y) + l.z * p.N.y,
            (l.x * p.T1.z + l.y * p.T2.z) + l.z * p.N.z);
}

// The probe's far end for the local direction l.
RTG_HD V3 ao_end(const AoPoint& p, V3 l, float radius) {
  const V3 w = ao_world(p, l);
  return v3(p.a.x + radius * w.x, p.a.y + radius * w.y, p.a.z + radius * w.z);
}

}  // namespace rtg
