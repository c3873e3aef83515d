// rtg_host_scene.h — the packed scene tables (pack_scene, rtg_scene_pack.h) as
// a one-lane Scene of rtg_trace.h's functions on the host: every accessor the
// device scene (DevScene, rtg_trace_kernels.h) has, a "wave" of one ray, the
// frame colours in a member array.  The host forms of the batch ray tracer
// and the posed camera run trace_sample over it (rtg_raytrace_host,
// rtg_render_camera_host: with_stack and host_trace_fn below pick their
// instantiation), the walk-1 host queries ray_closest / ray_blocked
// (rtg_intersect_host, rtg_visible_host).  kBvh: as DevScene's.
#pragma once

#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "rtg.h"
#include "rtg_scene_pack.h"
#include "rtg_trace.h"
#include "rtg_trace_kernels.h"

namespace rtg {

template <bool kBvh>
struct HostScene {
  static constexpr bool kIsBvh = kBvh;
  int fuse = 0;  // fused query forms (kFuse*): none
  const float* geom = nullptr;
  const float* crad2 = nullptr;
  const float* mats = nullptr;
  const float* lights = nullptr;
  const unsigned* smask = nullptr;
  const unsigned* cone = nullptr;
  const float* prim = nullptr;
  const float* bvhNodes = nullptr;
  const float* capRec = nullptr;
  const unsigned* capOff = nullptr;
  const float* ovRec = nullptr;
  const unsigned* ovOff = nullptr;
  unsigned n = 0, m = 0, n4 = 0;
  mutable FrameC fr[RTG_MAX_STACK];

  // The basic tables (records, materials, lights); `tables`: the masks, the
  // BVH and the sphere lists too, as bind_scene binds them.
  HostScene(const PackedScene& ps, bool tables) {
    geom = ps.geom.data();
    crad2 = ps.crad2.data();
    mats = ps.mats.data();
    lights = ps.lights.data();
    prim = ps.prim.data();
    n = ps.n;
    m = ps.m;
    n4 = ps.n4;
    if (!tables) return;
    if (!ps.smask.empty()) smask = ps.smask.data();
    if (!ps.cone.empty()) cone = ps.cone.data();
    if (!ps.bvhNodes.empty()) bvhNodes = ps.bvhNodes.data();
    if (!ps.capOff.empty()) {
      capRec = ps.capRec.data();
      capOff = ps.capOff.data();
      ovRec = ps.ovRec.data();
      ovOff = ps.ovOff.data();
    }
  }

  void count(int, long) const {}
  void probe_begin(int) const {}
  void probe_end(int) const {}
  bool all(bool b) const { return b; }
  bool any(bool b) const { return b; }
  V3 first_lane(V3 v) const { return v; }
  float first_lane(float v) const { return v; }
  int first_lane_i(int v) const { return v; }
  int lane_with(int v, bool) const { return v; }

  struct Frames {
    FrameC* f;
    FrameC get(int lv) const { return f[lv]; }
    void set(int lv, const FrameC& v) const { f[lv] = v; }
  };
  Frames frames() const { return Frames{fr}; }

  bool has_bvh() const { return kBvh; }
  bool has_lists() const { return kBvh && capOff != nullptr; }
  bool has_cone() const { return cone != nullptr; }
  bool has_smask() const { return smask != nullptr; }
  int* bvh_stack() const { return nullptr; }
  void bvh_rec(unsigned nd, BvhRec& r) const {
    const float* g = bvhNodes + (size_t)kBvhWords * nd;
    memcpy(r.s, g, 24 * 4);
    memcpy(r.ch, g + 24, 4 * 4);
    memcpy(r.cr, g + 28, 4 * 4);
  }

  V3 sphere(unsigned i, float& r2) const {
    const float* g = geom + 4 * (size_t)i;
    r2 = g[3];
    return v3(g[0], g[1], g[2]);
  }
  V3 sphere_lane(unsigned i, float& r2) const { return sphere(i, r2); }
  float sphere_r2(unsigned i) const { return geom[4 * (size_t)i + 3]; }
  void sphere4(unsigned i, V3* c, float* r2) const {
    for (int k = 0; k < 4; ++k) c[k] = sphere(i + k, r2[k]);
  }
  void sphere4_screen(unsigned i, V3* c, float* rs) const { sphere4(n4 + 4 + i, c, rs); }
  V3 sphere_screen(unsigned i, float& rs) const { return sphere(n4 + 4 + i, rs); }
  void sphere4_contain(unsigned i, V3* c, float* cr) const { sphere4(2 * (n4 + 4) + i, c, cr); }
  V3 sphere_contain(unsigned i, float& cr) const { return sphere(2 * (n4 + 4) + i, cr); }
  V3 sphere_fused(unsigned i, float& rs, float& r2, float& oc) const {
    const float* g = geom + 12 * (size_t)(n4 + 4) + 8 * (size_t)i;
    rs = g[3];
    r2 = g[4];
    oc = g[5];
    return v3(g[0], g[1], g[2]);
  }
  float contain_r2(unsigned i) const { return crad2[i]; }
  float origin_c(unsigned i) const { return crad2[n + i]; }
  float guard_r2(unsigned i) const { return crad2[2 * (size_t)n + i]; }
  bool prim_possible(const PrimBundle& b, unsigned i, V3 c) const {
    const float* k = prim + 4 * (size_t)i;
    return primary_possible(b, c, k[0], k[1], k[2]);
  }

  // sphere lists (BVH scenes)
  void cap_range(unsigned l, unsigned h, unsigned cell, unsigned& k0, unsigned& k1) const {
    const size_t slot = ((size_t)l * n + h) * kCapCells + cell;
    k0 = capOff[2 * slot];
    k1 = capOff[2 * slot + 1];
  }
  void ov_range(unsigned h, unsigned& k0, unsigned& k1) const {
    k0 = ovOff[h];
    k1 = ovOff[h + 1];
  }
  static V3 list_rec(const float* b, unsigned k, float& rs, float& r2, float& cr, int& idx,
                     float& rf) {
    const float* g = b + 8 * (size_t)k;
    rs = g[3];
    r2 = g[4];
    cr = g[5];
    memcpy(&idx, &g[6], 4);
    rf = g[7];
    return v3(g[0], g[1], g[2]);
  }
  static void list_rec2(const float* b, unsigned k, ListRec& r0, ListRec& r1) {
    r0.c = list_rec(b, k, r0.rs, r0.r2, r0.cr, r0.idx, r0.rf);
    r1.c = list_rec(b, k + 1, r1.rs, r1.r2, r1.cr, r1.idx, r1.rf);
  }
  void cap_rec4(unsigned k, CapRec* r) const {
    for (int j = 0; j < 4; ++j) {
      const float* g = capRec + 4 * ((size_t)k + j);
      r[j].c = v3(g[0], g[1], g[2]);
      r[j].r2 = g[3];
    }
  }
  void ov_rec2(unsigned k, ListRec& r0, ListRec& r1) const { list_rec2(ovRec, k, r0, r1); }
  V3 ov_rec(unsigned k, float& rs, float& r2, float& cr, int& idx, float& rf) const {
    return list_rec(ovRec, k, rs, r2, cr, idx, rf);
  }

  // masks (n <= 64): a single lane, so a union is that lane's mask
  uint64_t mask_at(size_t w) const {
    return (uint64_t)smask[2 * w] | ((uint64_t)smask[2 * w + 1] << 32);
  }
  uint64_t every() const { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }
  uint64_t overlap_mask(unsigned h) const { return mask_at((size_t)m * n + h); }
  uint64_t overlap_union(int h, uint64_t& own) const {
    own = overlap_mask((unsigned)h);
    return own;
  }
  uint64_t contain_union(int hit, bool ok) const {
    return ok ? overlap_mask((unsigned)hit) : every();
  }
  uint64_t shadow_union(unsigned l, int hit, bool guardOK) const {
    return guardOK ? mask_at((size_t)l * n + (unsigned)hit) : every();
  }
  uint64_t cone_union(int h, unsigned tier, unsigned cell) const {
    const unsigned* w = cone + 2u * (((unsigned)h * kConeTiers + tier) * kConeCells + cell);
    return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  }

  Mat mat(int i) const {
    const float* p = mats + 8 * (size_t)i;
    Mat r;
    r.matte = v3(p[0], p[1], p[2]);
    r.gloss = v3(p[3], p[4], p[5]);
    r.opacity = p[6];
    r.refr = p[7];
    return r;
  }
  float refr(int i) const { return mats[8 * (size_t)i + 7]; }
  // refraction's constants of the material pair (scenes with masks: pack_scene)
  void pair(int src, int tgt, float& ratio, float& qc) const {
    const float* p = mats + 8 * (size_t)(n + 1) + 2 * ((size_t)src * (n + 1) + (size_t)tgt);
    ratio = p[0];
    qc = p[1];
  }
  void hit_data(int i, V3& c, float& g2, float& r2, Mat& mt) const {
    c = sphere((unsigned)i, r2);
    g2 = guard_r2((unsigned)i);
    mt = mat(i);
  }
  V3 sphere_guard(int h, float& r2, float& g2) const {
    g2 = guard_r2((unsigned)h);
    return sphere((unsigned)h, r2);
  }
  void light(unsigned l, V3& pos, V3& col) const {
    const float* p = lights + 6 * (size_t)l;
    pos = v3(p[0], p[1], p[2]);
    col = v3(p[3], p[4], p[5]);
  }
};

// A run-time stack capacity as a compile-time one: f(integral_constant<int, S>)
// for S in 1..RTG_MAX_STACK, a value-initialised result (a null function
// pointer) outside it.
template <class F>
auto with_stack(int S, F&& f) -> decltype(f(std::integral_constant<int, 1>{})) {
  switch (S) {
#define RTG_X(k) case k: return f(std::integral_constant<int, k>{});
    RTG_FOR_EACH_S(RTG_X)
#undef RTG_X
    default: return {};
  }
}

// The instantiations a host form has per S, THE ladder: {cl} x {walk 0, walk 1
// flat, walk 1 BVH} (walk 0 has no BVH).  f(S, cl, walk, bvh) gets them as
// integral constants and returns the host form's range function.
template <class F>
auto host_trace_fn(int S, bool cl, bool walk, bool bvh, F&& f) {
  using std::false_type;
  using std::true_type;
  return with_stack(S, [&](auto s) {
    if (!walk) return cl ? f(s, true_type{}, false_type{}, false_type{})
                         : f(s, false_type{}, false_type{}, false_type{});
    if (bvh) return cl ? f(s, true_type{}, true_type{}, true_type{})
                       : f(s, false_type{}, true_type{}, true_type{});
    return cl ? f(s, true_type{}, true_type{}, false_type{})
              : f(s, false_type{}, true_type{}, false_type{});
  });
}

}  // namespace rtg
