// tests/hostsim/query_forms.cpp — TEST-ONLY stand-alone program (its own main):
// the masked scenes' query forms of rtg_trace.h, compiled for the host, against
// the plain loops (closest_hit, blocked, primary_container) bit for bit, on
// small hand-placed scenes whose selections sit at chosen bit positions.
//
//   closest_sel / closest_sel_fused / closest_sel_lazy   (cone queries)
//   closest_hit_sel / closest_hit_sel_fused              (primary rays)
//   closest_enter / closest_enter_fused                  (entering rays)
//   blocked_sel / blocked_sel_fused                      (shadow rays)
//   primary_container_sel                                (refraction target)
//
// A scene has 64 slots; the slots outside the selection hold NaN spheres, which
// accept no root and contain no point, so the plain loops over all 64 slots
// answer for the selection alone.  tests/test_query_forms_host.py builds this
// file with -fsanitize=address,undefined and runs it; it prints one summary
// line and returns 0 when every comparison held and none of them was vacuous.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rtg.h"
#include "rtg_internal.h"
#include "rtg_scene_pack.h"
#include "rtg_trace.h"

void rtg_set_error(const char*, ...) {}
void rtg_clear_error() {}

namespace {
using rtg::V3;
using rtg::v3;

long g_counts[rtg::kCntSlots];

// A single-lane scene over PackedScene's tables: what the query forms above
// and the plain loops read (hostsim.cpp's HostScene, without the traversal).
struct HostScene {
  void count(int slot, long v) const { g_counts[slot] += v; }
  const float* geom;
  const float* crad2;
  const float* mats;
  unsigned n, m, n4;
  int fuse = 0;
  bool all(bool b) const { return b; }
  bool any(bool b) const { return b; }
  int first_lane_i(int v) const { return v; }
  bool has_bvh() const { return false; }  // (container_bvh is compiled, never run)
  int* bvh_stack() const { return nullptr; }
  void bvh_rec(unsigned, rtg::BvhRec& r) const { memset(&r, 0, sizeof r); }
  V3 sphere(unsigned i, float& r2) const {
    const float* g = geom + 4 * i;
    r2 = g[3];
    return v3(g[0], g[1], g[2]);
  }
  V3 sphere_lane(unsigned i, float& r2) const { return sphere(i, r2); }
  V3 sphere_fused(unsigned i, float& rs, float& r2, float& oc) const {
    const float* g = geom + 12 * (n4 + 4) + 8 * i;
    rs = g[3];
    r2 = g[4];
    oc = g[5];
    return v3(g[0], g[1], g[2]);
  }
  void sphere4(unsigned i, V3* c, float* r2) const {
    for (int k = 0; k < 4; ++k) c[k] = sphere(i + k, r2[k]);
  }
  V3 sphere_screen(unsigned i, float& rs) const { return sphere(n4 + 4 + i, rs); }
  void sphere4_contain(unsigned i, V3* c, float* cr) const { sphere4(2 * (n4 + 4) + i, c, cr); }
  V3 sphere_contain(unsigned i, float& cr) const { return sphere(2 * (n4 + 4) + i, cr); }
  float guard_r2(unsigned i) const { return crad2[2 * n + i]; }
  float origin_c(unsigned i) const { return crad2[n + i]; }
  float refr(int i) const { return mats[8 * i + 7]; }
  V3 sphere_guard(int h, float& r2, float& g2) const {
    g2 = guard_r2((unsigned)h);
    return sphere((unsigned)h, r2);
  }
};

constexpr unsigned kN = 64;
constexpr int kFuseAll = rtg::kFusePrim | rtg::kFuseCone | rtg::kFuseShadow | rtg::kFuseEnter;

long g_checks = 0, g_fail = 0;
long g_hits = 0, g_blocks = 0, g_enterOK = 0, g_slowRays = 0, g_ties = 0, g_contained = 0,
     g_ownSubset = 0;

unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

void expect(bool ok, const char* fmt, ...) {
  ++g_checks;
  if (ok) return;
  if (++g_fail > 20) return;
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "FAIL: ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
}

struct Lcg {
  unsigned long long s;
  double u01() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  }
  V3 unit() {
    for (;;) {
      const double x = 2 * u01() - 1, y = 2 * u01() - 1, z = 2 * u01() - 1;
      const double l = sqrt(x * x + y * y + z * z);
      if (l > 1e-3 && l <= 1.0) return v3((float)(x / l), (float)(y / l), (float)(z / l));
    }
  }
};

// The overlap query's masks: the union the wave loops over and the lane's own.
struct EnterScene : HostScene {
  uint64_t uni = 0, mine = 0;
  uint64_t overlap_union(int, uint64_t& own) const {
    own = mine;
    return uni;
  }
  uint64_t overlap_mask(unsigned) const { return mine; }  // (the two-pass form's)
};

struct Built {
  std::vector<rtg_sphere> sph;
  rtg::PackedScene ps;
  EnterScene sc;
};

// 64 slots, NaN everywhere but `slots[k]` (increasing), which take the k-th
// sphere of arrangement `arr`; `without` (a slot or -1) stays NaN as well.
void build(Built& b, const std::vector<unsigned>& slots, int arr, int without = -1) {
  const float nan = __builtin_nanf("");
  b.sph.assign(kN, rtg_sphere{});
  for (unsigned i = 0; i < kN; ++i) {
    b.sph[i].pos = rtg_vec{nan, nan, nan};
    b.sph[i].radius = nan;
    b.sph[i].material.opacity = 0.5f;
    b.sph[i].material.refractiveIndex = 1.1f + 0.01f * (float)i;
  }
  for (size_t k = 0; k < slots.size(); ++k) {
    if ((int)slots[k] == without) continue;
    rtg_sphere& s = b.sph[slots[k]];
    const float fk = (float)k;
    switch (arr) {
      case 0:  // a row along the view axis: the first one blocks
        s.pos = rtg_vec{0.3f * fk, 0.f, -10.f - 4.f * fk};
        s.radius = 1.5f;
        break;
      case 1:  // the first two coincide (equal t: the lower index wins), the third behind
        s.pos = rtg_vec{0.f, 0.25f, k < 2 ? -10.f : -16.f};
        s.radius = 1.5f;
        break;
      default:  // nested: every overlap mask is full
        s.pos = rtg_vec{0.1f * fk, 0.f, -12.f};
        s.radius = 2.f + 1.25f * fk;
        break;
    }
  }
  rtg_light lg[2] = {{{5.f, 20.f, 0.f}, {1.f, 1.f, 1.f}}, {{-30.f, 2.f, -12.f}, {1.f, 1.f, 1.f}}};
  rtg::pack_scene(b.sph.data(), kN, lg, 2, &b.ps);
  EnterScene& sc = b.sc;
  sc.geom = b.ps.geom.data();
  sc.crad2 = b.ps.crad2.data();
  sc.mats = b.ps.mats.data();
  sc.n = kN;
  sc.m = 2;
  sc.n4 = b.ps.n4;
  sc.fuse = kFuseAll;
}

struct Ray {
  V3 o, d;
};

void add_scaled(std::vector<Ray>& out, const Ray& r) {
  // raygen.scaled's set (tests/raygen.py): direction lengths 1e-3, 7, 2^-40 and
  // 2^40 (the last two put 2a outside [2^-60, 2^60]), a zero direction, and NaN
  // and both infinities in each component of the origin and of the direction
  const float sc[4] = {1e-3f, 7.f, 0x1p-40f, 0x1p40f};
  for (float s : sc) out.push_back(Ray{r.o, rtg::vsmul(s, r.d)});
  out.push_back(Ray{r.o, v3(0.f, 0.f, 0.f)});
  const float bad[3] = {__builtin_nanf(""), __builtin_inff(), -__builtin_inff()};
  for (int comp = 0; comp < 6; ++comp)
    for (float v : bad) {
      Ray x = r;
      float* p = comp < 3 ? &x.o.x : &x.d.x;
      p[comp % 3] = v;
      out.push_back(x);
    }
}

std::vector<Ray> make_rays(const Built& b, const std::vector<unsigned>& slots, Lcg& rng,
                           bool primaryOnly) {
  std::vector<Ray> rays;
  const V3 zero = v3(0.f, 0.f, 0.f);
  for (int k = 0; k < 24; ++k) {  // a cone around the view axis
    const V3 u = rng.unit();
    rays.push_back(Ray{zero, rtg::vnorm(v3(0.35f * u.x, 0.35f * u.y, -1.f))});
  }
  for (unsigned s : slots) {
    const rtg_sphere& sp = b.sph[s];
    const V3 c = v3(sp.pos.x, sp.pos.y, sp.pos.z);
    rays.push_back(Ray{zero, rtg::vnorm(c)});
    rays.push_back(Ray{zero, c});  // unnormalised: the hit near t = 1
    for (float e : {-1e-3f, 1e-6f, 1e-3f}) {  // grazing, in and out of the silhouette
      const V3 aim = v3(c.x, c.y + sp.radius * (1.f + e), c.z);
      rays.push_back(Ray{zero, rtg::vnorm(aim)});
    }
  }
  if (!primaryOnly) {
    for (unsigned s : slots) {
      const rtg_sphere& sp = b.sph[s];
      const V3 c = v3(sp.pos.x, sp.pos.y, sp.pos.z);
      V3 nrm[5] = {rtg::vnorm(v3(-c.x, -c.y, -c.z)), v3(0.f, 1.f, 0.f), v3(0.f, 0.f, -1.f),
                   rng.unit(), rng.unit()};
      for (const V3& nn : nrm) {
        const V3 P = rtg::vadd(c, rtg::vsmul(sp.radius, nn));  // the renderer's kind of origin
        V3 dirs[6] = {nn, rtg::vsmul(-1.f, nn), rng.unit(), v3(0.f, 0.f, -1.f), v3(0.f, 0.f, 1.f),
                      rtg::vnorm(rtg::vsub(v3(5.f, 20.f, 0.f), P))};
        for (const V3& dd : dirs) {
          rays.push_back(Ray{P, dd});
          rays.push_back(Ray{rtg::vadd(P, rtg::vsmul(0.01f, dd)), dd});
        }
      }
      for (int k = 0; k < 4; ++k)  // from inside
        rays.push_back(Ray{rtg::vadd(c, rtg::vsmul(0.4f * sp.radius, rng.unit())), rng.unit()});
    }
  }
  const size_t base = rays.size();
  for (size_t k = 0; k < base; k += 7) {
    std::vector<Ray> sc;
    add_scaled(sc, rays[k]);
    for (const Ray& r : sc)
      if (!primaryOnly || (r.o.x == 0.f && r.o.y == 0.f && r.o.z == 0.f)) rays.push_back(r);
  }
  return rays;
}

void same_hit(const char* form, int fuse, size_t ray, int got, float tg, int want, float tw) {
  expect(got == want && bits(tg) == bits(tw), "%s (fuse %d) ray %zu: hit %d t %08x, plain loop %d %08x",
         form, fuse, ray, got, bits(tg), want, bits(tw));
}

uint64_t mask_of(const std::vector<unsigned>& slots) {
  uint64_t m = 0;
  for (unsigned s : slots) m |= 1ull << s;
  return m;
}

void run_scene(const std::vector<unsigned>& slots, int arr, Lcg& rng) {
  Built b;
  build(b, slots, arr);
  const uint64_t sel = mask_of(slots);
  EnterScene& sc = b.sc;
  sc.uni = sc.mine = sel;
  const std::vector<Ray> rays = make_rays(b, slots, rng, false);
  // the plain loops of the scenes with one selected sphere left out (the enter
  // loop's own-mask test: a lane must not test a sphere of another lane's mask)
  std::vector<Built> less(slots.size());
  for (size_t k = 0; k < slots.size(); ++k) build(less[k], slots, arr, (int)slots[k]);

  for (int fuse : {kFuseAll, 0}) {
    sc.fuse = fuse;
    for (size_t r = 0; r < rays.size(); ++r) {
      const V3 o = rays[r].o, d = rays[r].d;
      const rtg::RayQ q = rtg::make_query(o, d);
      if (!q.fast) ++g_slowRays;
      float tw;
      const int want = rtg::closest_hit(sc, o, d, tw);
      if (want >= 0) ++g_hits;
      // --- cone queries
      float t;
      int got = rtg::closest_sel(sc, q, sel, t, -1);
      same_hit("closest_sel", fuse, r, got, t, want, tw);
      got = rtg::closest_sel_fused<false>(sc, q, sel, t, -1);
      same_hit("closest_sel_fused<false>", fuse, r, got, t, want, tw);
      if (q.fast) {
        got = rtg::closest_sel_fused<true>(sc, q, sel, t, -1);
        same_hit("closest_sel_fused<true>", fuse, r, got, t, want, tw);
      }
      for (unsigned h : slots) {  // the cone-query site of trace_sample, origin sphere h
        float qa;
        rtg::RayQ ql = rtg::query_head(o, d, qa);
        uint64_t cm = sel;
        int skip = -1;
        float r2o, g2o;
        const V3 co = sc.sphere_guard((int)h, r2o, g2o);
        const V3 e = rtg::vsub(ql.o, co);
        if (rtg::no_root(ql, 2.0f * rtg::vdot(ql.d, e), rtg::vdot(e, e) - r2o)) skip = (int)h;
        if (skip == (int)h) cm &= ~(1ull << h);
        got = rtg::closest_sel_lazy(sc, ql, qa, cm, t, skip);
        same_hit("closest_sel_lazy", fuse, r, got, t, want, tw);
        // ... and a wave that could not drop it: the lane skips it in the loop
        ql = rtg::query_head(o, d, qa);
        got = rtg::closest_sel_lazy(sc, ql, qa, sel, t, skip);
        same_hit("closest_sel_lazy (skip in the loop)", fuse, r, got, t, want, tw);
      }
      // --- entering rays
      for (size_t k = 0; k < slots.size(); ++k) {
        const int h = (int)slots[k];
        bool ok;
        sc.uni = sc.mine = sel;
        got = rtg::closest_enter(sc, q, h, t, ok);
        if (ok) {
          ++g_enterOK;
          same_hit("closest_enter", fuse, r, got, t, want, tw);
          if (want >= 0 && want != h) ++g_ties;
        }
        if (fuse) {
          bool ok2;
          got = rtg::closest_enter_fused<false>(sc, q, h, t, ok2);
          expect(ok2 == ok, "closest_enter_fused<false> ray %zu h %d: ok %d vs %d", r, h, ok2, ok);
          if (ok2) same_hit("closest_enter_fused<false>", fuse, r, got, t, want, tw);
          // the lane's own mask lacks sphere x (another lane's): the answer is
          // the plain loop's of the scene without x
          for (size_t kx = 0; kx < slots.size(); ++kx) {
            if (kx == k) continue;
            sc.uni = sel;
            sc.mine = sel & ~(1ull << slots[kx]);
            float tl;
            const int wl = rtg::closest_hit(less[kx].sc, o, d, tl);
            got = rtg::closest_enter(sc, q, h, t, ok2);
            expect(ok2 == ok, "closest_enter (own subset) ray %zu: ok %d vs %d", r, ok2, ok);
            if (ok2) {
              ++g_ownSubset;
              same_hit("closest_enter (own subset)", fuse, r, got, t, wl, tl);
            }
          }
          sc.uni = sc.mine = sel;
        }
      }
      // --- shadow rays
      for (float gap : {0.25f, 30.f, 150.f, 400.f, 1.0e6f, __builtin_inff(), __builtin_nanf("")}) {
        const bool wb = rtg::blocked(sc, o, d, gap);
        if (wb) ++g_blocks;
        bool gb = rtg::blocked_sel(sc, o, d, gap, sel);
        expect(gb == wb, "blocked_sel (fuse %d) ray %zu gap %g: %d, plain loop %d", fuse, r, gap, gb, wb);
        gb = rtg::blocked_sel_fused<false>(sc, q, gap, sel, -1);
        expect(gb == wb, "blocked_sel_fused<false> ray %zu gap %g: %d, plain loop %d", r, gap, gb, wb);
        if (q.fast) {
          gb = rtg::blocked_sel_fused<true>(sc, q, gap, sel, -1);
          expect(gb == wb, "blocked_sel_fused<true> ray %zu gap %g: %d, plain loop %d", r, gap, gb, wb);
        }
        for (unsigned h : slots) {  // the ray leaves hit sphere h (matte_light's call)
          float hr2;
          const V3 hc = sc.sphere(h, hr2);
          gb = rtg::blocked_sel(sc, o, d, gap, sel, (int)h, hc, hr2);
          expect(gb == wb, "blocked_sel hit %u (fuse %d) ray %zu gap %g: %d, plain loop %d", h, fuse, r,
                 gap, gb, wb);
        }
      }
      // --- refraction target: the test point 0.01 along the ray
      {
        const V3 pt = rtg::vadd(rtg::vsmul(0.01f, d), o);
        const int wc = rtg::primary_container(sc, pt);
        if (wc >= 0) ++g_contained;
        float nT;
        const int gc = rtg::primary_container_sel(sc, pt, sel, nT);
        expect(gc == wc && bits(nT) == bits(sc.refr(wc < 0 ? (int)kN : wc)),
               "primary_container_sel ray %zu: %d n %08x, plain loop %d", r, gc, bits(nT), wc);
      }
    }
  }
  // --- primary rays (origin 0)
  const std::vector<Ray> prays = make_rays(b, slots, rng, true);
  for (int fuse : {kFuseAll, 0}) {
    sc.fuse = fuse;
    for (size_t r = 0; r < prays.size(); ++r) {
      const V3 o = prays[r].o, d = prays[r].d;
      float tw, t;
      const int want = rtg::closest_hit(sc, o, d, tw);
      int got = rtg::closest_hit_sel(sc, o, d, t, sel);
      same_hit("closest_hit_sel", fuse, r, got, t, want, tw);
      const rtg::RayQ q = rtg::make_query(o, d);
      got = rtg::closest_hit_sel_fused<false>(sc, q, sel, t);
      same_hit("closest_hit_sel_fused<false>", fuse, r, got, t, want, tw);
    }
  }
}
}  // namespace

int main() {
  // selections of 0, 1, 2 and 3 bits, at positions 0, 31, 32 and 63
  const std::vector<std::vector<unsigned>> patterns = {
      {}, {0}, {31}, {32}, {63}, {0, 31}, {31, 32}, {32, 63}, {0, 63},
      {0, 31, 32}, {31, 32, 63}, {0, 32, 63}};
  Lcg rng{20240611ull};
  for (int k = 0; k < rtg::kCntSlots; ++k) g_counts[k] = 0;
  for (int arr = 0; arr < 3; ++arr)
    for (const auto& p : patterns) run_scene(p, arr, rng);
  // none of it vacuous: the plain loops hit, block and contain; entering rays
  // pass their guard tests; selections ran empty after the own-sphere and the
  // origin-sphere drop; rays took the division fallback; exact tests ran in
  // every loop
  const long shdEmpty = g_counts[rtg::kUDiagShdEmpty], coneEmpty = g_counts[rtg::kUDiagConeEmpty];
  const bool live = g_hits > 1000 && g_blocks > 1000 && g_enterOK > 100 && g_ownSubset > 100 &&
                    g_ties > 10 && g_contained > 100 && g_slowRays > 100 && shdEmpty > 100 &&
                    coneEmpty > 100 && g_counts[rtg::kUEnterExact] > 100 &&
                    g_counts[rtg::kUSelExact] > 100 && g_counts[rtg::kUShdExact] > 100 &&
                    g_counts[rtg::kUPrimExact] > 100;
  printf("query_forms: %ld comparisons, %ld failed; hits %ld, blocks %ld, enter ok %ld (own subset %ld, "
         "other sphere first %ld), contained %ld, slow rays %ld, empty shadow selections %ld, empty cone "
         "selections %ld%s\n",
         g_checks, g_fail, g_hits, g_blocks, g_enterOK, g_ownSubset, g_ties, g_contained, g_slowRays,
         shdEmpty, coneEmpty, live ? "" : " -- VACUOUS");
  return (g_fail == 0 && live) ? 0 : 1;
}
