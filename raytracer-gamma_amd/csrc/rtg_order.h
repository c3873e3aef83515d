// rtg_order.h — the coherence sort key of a ray batch (rtg_ray_order*, rtg.h):
// one function of a ray (origin, dir) and the scene's key box, the same bits on
// host and device (the Makefile's FPFLAGS: no contraction; every operation is
// an IEEE add, subtract, multiply or correctly rounded divide).  The sort, the
// entry points and the host form are in rtg_order.hip; the key box comes from
// key_bounds (rtg_scene_pack.h) through key_box below, for the context
// (rtg_context_set_scene) and the host form alike.
//
// Key, kKeyBits = 3 kOriginBits + 2 kDirBits = 50 used bits (rtg.h states it
// as part of the contract):
//   bits 49..20  Morton code of the origin's cell (x bit i at 3 i, y at 3 i +
//                1, z at 3 i + 2 of the code), kOriginBits per axis
//   bits 19..0   Morton code of the direction's octahedral bin (u bit i at
//                2 i, v at 2 i + 1), kDirBits per axis
// Origin-major: rays that start together sort together and, among those, rays
// that point the same way; a batch with one origin (a camera's, a probe's)
// has constant high bits, and the sort skips their digit positions.  The
// layout that interleaves all five coordinates into one Morton code (kLayout5D,
// the measured alternative, DESIGN) is kept behind the same function.
#pragma once

#include <math.h>

#include "rtg_trace.h"

namespace rtg {

// (the macros: measurement builds of other bit counts, tools/bench_rays.py
// --order-label; rtg.h fixes 10 and 10)
#ifndef RTG_ORDER_ORIGIN_BITS
#define RTG_ORDER_ORIGIN_BITS 10
#endif
#ifndef RTG_ORDER_DIR_BITS
#define RTG_ORDER_DIR_BITS 10
#endif
constexpr int kOriginBits = RTG_ORDER_ORIGIN_BITS;  // b: cells per axis = 2^b
constexpr int kDirBits = RTG_ORDER_DIR_BITS;        // c: octahedral bins per axis = 2^c
constexpr int kKeyBits = 3 * kOriginBits + 2 * kDirBits;
static_assert(kKeyBits <= 64 && kOriginBits <= 10 && kDirBits <= 16, "the spreads below");

// The key box as the key function takes it: per axis the low plane and the
// cells per unit length, 2^b / (hi - lo); 0 for a degenerate axis (hi <= lo,
// or a width whose quotient is not finite), whose cell is then always 0.
struct KeyBox {
  float lo[3], scale[3];
};

inline KeyBox key_box(const float lo[3], const float hi[3]) {
  KeyBox b;
  for (int a = 0; a < 3; ++a) {
    const float w = hi[a] - lo[a];
    float s = 0.f;
    if (w > 0.f && w < __builtin_inff()) {
      s = (float)(1 << kOriginBits) / w;
      if (!(s < __builtin_inff())) s = 0.f;
    }
    b.lo[a] = lo[a];
    b.scale[a] = s;
  }
  return b;
}

// (int)v of a float clamped to [0, top] IN FLOAT first: NaN and negatives give
// 0, +inf and anything above gives top; the conversion never sees a value
// outside [0, top], so it is defined (and the same) everywhere.
RTG_HD unsigned key_quantise(float v, float top) {
  float c = (v >= 0.f) ? v : 0.f;  // NaN: 0
  c = (c <= top) ? c : top;
  return (unsigned)(int)c;
}

// Bits of a 10-bit value two apart (bit i -> bit 3 i).
RTG_HD unsigned key_spread3(unsigned v) {
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// Bits of a 16-bit value one apart (bit i -> bit 2 i).
RTG_HD unsigned key_spread2(unsigned v) {
  v &= 0xFFFFu;
  v = (v | (v << 8)) & 0x00FF00FFu;
  v = (v | (v << 4)) & 0x0F0F0F0Fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

// The origin's cell per axis: clamp((int)((o - lo) * scale), 0, 2^b - 1).  An
// infinite or NaN coordinate, and inf * 0 of a degenerate axis, go through the
// float clamp: NaN and -inf to cell 0, +inf to the last cell.
RTG_HD void key_cells(const KeyBox& B, V3 o, unsigned cell[3]) {
  const float top = (float)((1 << kOriginBits) - 1);
  cell[0] = key_quantise((o.x - B.lo[0]) * B.scale[0], top);
  cell[1] = key_quantise((o.y - B.lo[1]) * B.scale[1], top);
  cell[2] = key_quantise((o.z - B.lo[2]) * B.scale[2], top);
}

// The direction's octahedral bin (u, v), kDirBits each: p = d / (|x| + |y| +
// |z|) lies on the octahedron |x| + |y| + |z| = 1; its upper half (z >= 0)
// projects to the diamond |x| + |y| <= 1, the lower half folds into the
// corners; (u, v) = (p + 1) / 2 in [0, 1] scaled to 2^c bins.  A direction
// whose |x| + |y| + |z| is zero, NaN or infinite gets bin (0, 0).
RTG_HD void key_dir_bins(V3 d, unsigned bin[2]) {
  bin[0] = bin[1] = 0u;
  const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z);
  if (!(s > 0.f && s < __builtin_inff())) return;
  float px = d.x / s, py = d.y / s;
  if (d.z < 0.f) {
    const float qx = 1.f - fabsf(py), qy = 1.f - fabsf(px);
    px = (d.x < 0.f) ? -qx : qx;
    py = (d.y < 0.f) ? -qy : qy;
  }
  const float half = (float)(1 << (kDirBits - 1));  // (p + 1) / 2 * 2^c = (p + 1) * 2^(c-1)
  const float top = (float)((1 << kDirBits) - 1);
  bin[0] = key_quantise((px + 1.f) * half, top);
  bin[1] = key_quantise((py + 1.f) * half, top);
}

// The sort key of ray (o, d).  kLayout5D false: origin-major, the layout of
// rtg.h.  true: one 5-D Morton code, the alternative measured in DESIGN: from
// the top, rounds of (z, y, x, v, u) bits while both have bits left, then the
// remaining rounds of the longer of the two alone.
template <bool kLayout5D = false>
RTG_HD unsigned long long ray_key(const KeyBox& B, V3 o, V3 d) {
  unsigned cell[3], bin[2];
  key_cells(B, o, cell);
  key_dir_bins(d, bin);
  if constexpr (!kLayout5D) {
    const unsigned long long om = (unsigned long long)key_spread3(cell[0]) |
                                  ((unsigned long long)key_spread3(cell[1]) << 1) |
                                  ((unsigned long long)key_spread3(cell[2]) << 2);
    const unsigned dm = key_spread2(bin[0]) | (key_spread2(bin[1]) << 1);
    return (om << (2 * kDirBits)) | dm;
  } else {
    unsigned long long key = 0;
    for (int r = 0; r < (kOriginBits > kDirBits ? kOriginBits : kDirBits); ++r) {  // from the top
      const int ob = kOriginBits - 1 - r, db = kDirBits - 1 - r;
      if (ob >= 0)
        key = (key << 3) | (((cell[2] >> ob) & 1u) << 2) | (((cell[1] >> ob) & 1u) << 1) |
              ((cell[0] >> ob) & 1u);
      if (db >= 0) key = (key << 2) | (((bin[1] >> db) & 1u) << 1) | ((bin[0] >> db) & 1u);
    }
    return key;
  }
}

// A batch record (24 bytes: rtg_ray, or rtg_segment when `segments`) as the
// ray the key is taken of; a segment (a, b) is the ray (a, b - a).
RTG_HD void key_ray_of(const float* r, bool segments, V3& o, V3& d) {
  o = v3(r[0], r[1], r[2]);
  d = v3(r[3], r[4], r[5]);
  if (segments) d = vsub(d, o);
}

}  // namespace rtg
