// rtg_main.cpp — the reference's host program (main.cpp) on librtg.so.
//
// Same flow as main.cpp:94-508: build the scene (main.cpp:104-168, or the
// seeded generator for larger scenes), render on the GPU through the C ABI
// (replacing the OpenCL setup/enqueue/readback of main.cpp:182-468), compute
// the colour max (algebra.h:68) and write the P6 PPM (main.cpp:43-91).  Errors
// print a message and exit(EXIT_FAILURE), like checkError (err_code.h:143-155).
// Device selection follows device_picker.h:70-119 (--list, --device N, -h).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "rtg.h"

static void check(int rc, const char* what) {
  if (rc != RTG_OK) {
    fprintf(stderr, "Error: %s failed (%d): %s\n", what, rc, rtg_last_error());
    exit(EXIT_FAILURE);
  }
}

static void usage() {
  printf("\nUsage: ./rtg_main [OPTIONS]\n\n");
  printf("Options:\n");
  printf("  -h  --help               Print the message\n");
  printf("      --list               List available devices\n");
  printf("      --device     INDEX   Select device at INDEX (default 0)\n");
  printf("      --width      W       Frame width  (default 800, main.cpp:105)\n");
  printf("      --height     H       Frame height (default 600, main.cpp:106)\n");
  printf("      --spheres    N       Spheres (default 3 = main.cpp scene)\n");
  printf("      --lights     M       Lights  (default 2 = main.cpp scene)\n");
  printf("      --depth      D       Recursion depth = RTSTACK_MAXSIZE - 1 (default 5)\n");
  printf("      --aa         F       Alias factor (default 3 -> 3x3 samples)\n");
  printf("      --zoom       Z       Zoom factor (default -4)\n");
  printf("      --seed       S       Scene generator seed (default 42)\n");
  printf("      --out        FILE    Output PPM (default testPPM.ppm)\n");
  printf("      --gbuffer    FILE    Also write the primary-hit G-buffer: W*H raw little-endian\n");
  printf("                           rtg_gbuf_px records (id, t, hits, sample, normal, idSum)\n");
  printf("      --rays       FILE    Also intersect the rays of FILE with the scene: raw little-endian\n");
  printf("                           24-byte rtg_ray records (origin, dir); needs --hits and/or\n");
  printf("                           --radiance\n");
  printf("      --sort-rays          With --rays: order the batch for coherence on the device\n");
  printf("                           (rtg_ray_order_device) and run it through the indexed\n");
  printf("                           launches; the files written are the same bytes\n");
  printf("      --hits       FILE    Write their closest hits: 32-byte rtg_hit records\n");
  printf("                           (id, t, point, normal)\n");
  printf("      --radiance   FILE    Write their colours (rayTrace's return at --depth and\n");
  printf("                           --semantics): 12-byte rtg_vec records\n");
  printf("      --camera     POSE    Render from a posed camera: ex,ey,ez,tx,ty,tz[,ux,uy,uz] (eye,\n");
  printf("                           target, up; up defaults to 0,1,0), rtg_camera_look_at\n");
  printf("      --views      FILE    Render one frame per line of FILE, each a pose in --camera's\n");
  printf("                           syntax, in one launch (rtg_render_views_device); frame k goes\n");
  printf("                           to <out stem>.<k>.ppm\n");
  printf("      --cube       EYE     Render the six cube-map faces at ex,ey,ez (rtg_camera_cube: +X,\n");
  printf("                           -X, +Y, -Y, +Z, -Z) the same way; square frames at zoom -1\n");
  printf("                           (--width defaults to --height and the reverse, both to 64)\n");
  printf("      --sh         BANDS   With --cube: fold the faces into the probe's BANDS^2 real-SH RGB\n");
  printf("                           coefficients (1..4 bands; rtg_cube_sh_weights, the fused\n");
  printf("                           rtg_render_views_fold_device) instead of writing them; needs\n");
  printf("      --sh-out     FILE    The coefficients as text, one line \"r g b\" per k = l(l+1)+m,\n");
  printf("                           %%.9g: the floats read back exactly\n");
  printf("      --ao         SPEC    Also write the frame's ambient occlusion: K,radius[,bias[,seed]]\n");
  printf("                           (K probes of rtg_ao_directions(K) per primary hit at aa 1, from\n");
  printf("                           --camera or the identity pose; bias defaults to 0.001; a seed\n");
  printf("                           turns RTG_AO_JITTER on); needs --ao-out\n");
  printf("      --ao-out     FILE    The 8-bit binary PGM of (255 * count) / K per pixel\n");
  printf("      --ao-filter  SPEC    Smooth the counts before they are written: PASSES[,planeScale\n");
  printf("                           [,normalLog2]] (rtg_filter_device guided by the primary hits,\n");
  printf("                           RTG_FILTER_SAME_ID | NORMAL | PLANE; planeScale defaults to 1,\n");
  printf("                           normalLog2 to 3); the PGM is then 255 * value / K, clamped to\n");
  printf("                           0..255; needs --ao\n");
  printf("      --ao-scale   L[,planeScale[,normalLog2]]\n");
  printf("                           Trace the probes on the frame of width >> L and height >> L of\n");
  printf("                           the same pose (L in 1..3; both must divide by 1 << L), bring\n");
  printf("                           the counts up with rtg_upsample_device (RTG_UPSAMPLE_SAME_ID |\n");
  printf("                           NORMAL | PLANE; planeScale 1, normalLog2 3 unless given) and\n");
  printf("                           trace at full resolution only the pixels no low tap agrees with\n");
  printf("                           (rtg_hits_pick_device, rtg_values_place_device); the frame is\n");
  printf("                           then floats for --ao-history and --ao-filter; needs --ao\n");
  printf("      --ao-history FILE[,MAXHISTORY]\n");
  printf("                           Accumulate the counts over a camera path before they are written:\n");
  printf("                           one frame per line of FILE (poses in --camera's syntax, oldest\n");
  printf("                           first) and then the --camera frame, frame k with seed + k, each\n");
  printf("                           blended onto the last by rtg_accumulate_device (reprojection,\n");
  printf("                           RTG_ACCUM_SAME_ID | NORMAL | PLANE, planeScale 1, normalLog2 3,\n");
  printf("                           maxHistory 65535 unless given); the PGM is 255 * value / K as\n");
  printf("                           with --ao-filter, which then smooths the accumulated frame;\n");
  printf("                           needs --ao\n");
  printf("      --ao-variance SIGMA[,MINHISTORY]\n");
  printf("                           Guide --ao-filter's passes by the variance of the counts: the\n");
  printf("                           history carries the second moment (without --ao-history one\n");
  printf("                           reset frame is accumulated), rtg_variance_device estimates a\n");
  printf("                           variance per pixel with the filter's terms (spatially where the\n");
  printf("                           history is shorter than MINHISTORY, 4 unless given) and the\n");
  printf("                           passes run as rtg_svgf_device with RTG_SVGF_LUMA, sigmaL SIGMA and\n");
  printf("                           epsL 1e-6; needs --ao-filter\n");
  printf("      --matte      FILE   Also write the frame's direct light (rtg_matte_device of every\n");
  printf("                           primary hit at aa 1, from --camera or the identity pose) as a\n");
  printf("                           P6 PPM, scaled by its own largest component like the render\n");
  printf("      --probe-grid SPEC    Bake a grid of SH light probes over the scene's bounds:\n");
  printf("                           nx,ny,nz[,res[,bands]] (probe (0,0,0) at the bounds' low corner,\n");
  printf("                           the last at the high one; res x res cube faces per probe, 16\n");
  printf("                           unless given, at aa 1; 1..3 SH bands, 3 unless given; the fused\n");
  printf("                           rtg_render_views_fold_device with RTG_FOLD_SKIP_NONFINITE over\n");
  printf("                           rtg_probe_grid_poses, validity from rtg_contains_device); needs\n");
  printf("                           --irradiance\n");
  printf("      --irradiance FILE    Also write the grid's light at every primary hit at aa 1, from\n");
  printf("                           --camera or the identity pose (rtg_irradiance_device with\n");
  printf("                           RTG_IRR_LOBE_COSINE) as a P6 PPM, scaled by its own largest\n");
  printf("                           component like the render\n");
  printf("      --irr-flags  LIST    Which probes a point leaves out: a comma list of valid, facing,\n");
  printf("                           visible, or none (default valid,facing,visible)\n");
  printf("      --irr-bias   B       The lookup's start offset along the normal (default 0.001)\n");
  printf("      --gather     SPEC    Also write the frame's one-bounce indirect light: K[,bias[,seed]]\n");
  printf("                           (rtg_gather_device of every primary hit at aa 1, from --camera\n");
  printf("                           or the identity pose: K probes of rtg_ao_directions(K), weights\n");
  printf("                           1/K, --depth's stack; bias defaults to 0.001; a seed turns\n");
  printf("                           RTG_GATHER_JITTER on); needs --gather-out\n");
  printf("      --gather-out FILE    The P6 PPM, scaled by its own largest component like the render\n");
  printf("      --gather-skip        Leave NaN and infinite probe colours out (RTG_GATHER_SKIP_NONFINITE)\n");
  printf("      --gather-filter SPEC Smooth the gathered light before it is scaled and written: the\n");
  printf("                           spec and the filter of --ao-filter, with\n");
  printf("                           RTG_FILTER_SKIP_NONFINITE under --gather-skip; needs --gather\n");
  printf("      --gather-scale L[,planeScale[,normalLog2]]\n");
  printf("                           Gather on the low frame and upsample, as --ao-scale does (with\n");
  printf("                           RTG_UPSAMPLE_SKIP_NONFINITE under --gather-skip); needs --gather\n");
  printf("      --gather-history FILE[,MAXHISTORY]\n");
  printf("                           Accumulate the gathered light the same way (with\n");
  printf("                           RTG_ACCUM_SKIP_NONFINITE under --gather-skip) before it is\n");
  printf("                           filtered, scaled and written; needs --gather\n");
  printf("      --gather-variance SIGMA[,MINHISTORY]\n");
  printf("                           Guide --gather-filter's passes by the variance of the gathered\n");
  printf("                           light, as --ao-variance does; needs --gather-filter\n");
  printf("      --repeat     K       Render K times, report the best time\n");
  printf("      --scene      FILE    Load the scene from FILE (format: include/rtg.h)\n");
  printf("      --save-scene FILE    Write the scene used to FILE\n");
  printf("      --gpus       N       Render on devices 0..N-1 (row-cyclic shards, RCCL gather)\n");
  printf("      --semantics  MODE    cpu (default: raytracer.h, bit-exact) or opencl\n");
  printf("                           (raytrace_kernel.cl; use with --depth 4 = its stack of 5)\n");
  printf("\n");
}

// "ex,ey,ez,tx,ty,tz[,ux,uy,uz]" as rtg_camera_look_at's pose; false when it is not that.
static bool parse_pose(const char* s, rtg_camera* out) {
  float v[9] = {0, 0, 0, 0, 0, 0, 0.f, 1.f, 0.f};
  char tail = 0;
  const int k = sscanf(s, "%f,%f,%f,%f,%f,%f,%f,%f,%f%c", v, v + 1, v + 2, v + 3, v + 4, v + 5,
                       v + 6, v + 7, v + 8, &tail);
  if (k != 6 && k != 9) return false;
  const rtg_vec eye = {v[0], v[1], v[2]}, target = {v[3], v[4], v[5]}, up = {v[6], v[7], v[8]};
  check(rtg_camera_look_at(&eye, &target, &up, out), "rtg_camera_look_at");
  return true;
}

// "valid,facing,visible" (any subset, or "none") as RTG_IRR_* bits; false when it is not that.
static bool parse_irr_flags(const char* s, unsigned* flags) {
  *flags = 0;
  if (!strcmp(s, "none")) return true;
  while (*s) {
    const size_t k = strcspn(s, ",");
    if (k == 5 && !strncmp(s, "valid", k)) *flags |= RTG_IRR_VALID;
    else if (k == 6 && !strncmp(s, "facing", k)) *flags |= RTG_IRR_FACING;
    else if (k == 7 && !strncmp(s, "visible", k)) *flags |= RTG_IRR_VISIBLE;
    else return false;
    s += k;
    if (*s == ',' && !*++s) return false;
  }
  return *flags != 0;
}

// The grid of --probe-grid over the scene's bounds, in float: per axis lo = the
// least pos - |radius| and hi = the greatest pos + |radius| (comparisons as
// written: a NaN never wins), origin = lo and step = (hi - lo) / (float)(n - 1)
// for n >= 2; 1.f for n == 1 or a step that is not > 0.  No sphere: [-1, 1]^3.
static rtg_probe_grid grid_over(const std::vector<rtg_sphere>& spheres, const unsigned dims[3],
                                unsigned bands) {
  float lo[3] = {-1.f, -1.f, -1.f}, hi[3] = {1.f, 1.f, 1.f};
  for (size_t i = 0; i < spheres.size(); ++i) {
    const float c[3] = {spheres[i].pos.x, spheres[i].pos.y, spheres[i].pos.z};
    const float r = fabsf(spheres[i].radius);
    for (int q = 0; q < 3; ++q) {
      const float a = c[q] - r, b = c[q] + r;
      if (i == 0 || a < lo[q]) lo[q] = a;
      if (i == 0 || b > hi[q]) hi[q] = b;
    }
  }
  float st[3];
  for (int q = 0; q < 3; ++q) {
    st[q] = dims[q] >= 2 ? (hi[q] - lo[q]) / (float)(dims[q] - 1) : 1.f;
    if (!(st[q] > 0.f)) st[q] = 1.f;
  }
  return rtg_probe_grid{{lo[0], lo[1], lo[2]}, {st[0], st[1], st[2]}, dims[0], dims[1], dims[2],
                        bands};
}

// "PASSES[,planeScale[,normalLog2]]" of --ao-filter and --gather-filter; false when it is not that.
static bool parse_filter(const char* s, rtg_filter_params* p) {
  char tail = 0;
  p->planeScale = 1.f;
  p->normalLog2 = 3;
  const int k = sscanf(s, "%u,%f,%u%c", &p->passes, &p->planeScale, &p->normalLog2, &tail);
  p->flags = RTG_FILTER_SAME_ID | RTG_FILTER_NORMAL | RTG_FILTER_PLANE;
  return k >= 1 && k <= 3 && p->passes >= 1 && p->passes <= RTG_FILTER_MAX_PASSES &&
         p->normalLog2 <= 8;
}

// rtg_filter_device of the frame at `src` into a new device buffer, on the default stream.
static void* filter_frame(rtg_context* ctx, const rtg_hit* hits, unsigned W, unsigned H,
                          const rtg_filter_params& p, const void* src) {
  const size_t n = (size_t)W * H, out = n * (p.kind == RTG_FILTER_RGB ? 3 : 1) * sizeof(float);
  size_t bytes = 0;
  check(rtg_filter_scratch(W, H, &p, &bytes), "rtg_filter_scratch");
  void *dst = nullptr, *scratch = nullptr;
  if (hipMalloc(&dst, out) != hipSuccess || (bytes && hipMalloc(&scratch, bytes) != hipSuccess))
    check(RTG_ERR_NOMEM, "hipMalloc");
  check(rtg_filter_device(ctx, hits, W, H, &p, src, dst, scratch, bytes, nullptr),
        "rtg_filter_device");
  if (hipDeviceSynchronize() != hipSuccess) check(RTG_ERR_HIP, "rtg_filter_device");
  (void)hipFree(scratch);
  return dst;
}

// The poses of a file, one per line in --camera's syntax (blank lines are
// skipped); exits on a file that cannot be read or a line that is no pose.
static std::vector<rtg_camera> read_poses(const std::string& path) {
  std::vector<rtg_camera> poses;
  FILE* f = fopen(path.c_str(), "r");
  if (!f) {
    fprintf(stderr, "Error: can't read %s\n", path.c_str());
    exit(EXIT_FAILURE);
  }
  char line[512];
  while (fgets(line, sizeof line, f)) {
    size_t len = strlen(line);
    while (len && strchr(" \t\r\n", line[len - 1])) line[--len] = 0;
    if (line[strspn(line, " \t")] == 0) continue;  // a blank line
    rtg_camera c;
    if (!parse_pose(line, &c)) {
      printf("Invalid pose on line %zu of %s (ex,ey,ez,tx,ty,tz[,ux,uy,uz])\n", poses.size() + 1,
             path.c_str());
      exit(1);
    }
    poses.push_back(c);
  }
  fclose(f);
  return poses;
}

// "FILE[,maxHistory]" of --ao-history and --gather-history: a camera path to
// accumulate over; false when maxHistory is not in 1..65535.
struct History {
  bool on = false;
  std::string file;
  std::vector<rtg_camera> poses;  // oldest first; the --camera frame follows them
  rtg_accumulate_params params = {0, RTG_ACCUM_SAME_ID | RTG_ACCUM_NORMAL | RTG_ACCUM_PLANE, 3, 1.f,
                                  65535};
};
static bool parse_history(const char* s, History* h) {
  h->file = s;
  h->on = true;
  const size_t comma = h->file.rfind(',');
  if (comma == std::string::npos) return true;
  const std::string tail = h->file.substr(comma + 1);
  if (tail.empty() || tail.find_first_not_of("0123456789") != std::string::npos) return true;
  h->file.resize(comma);
  h->params.maxHistory = (unsigned)strtoul(tail.c_str(), nullptr, 10);
  return tail.size() <= 5 && h->params.maxHistory >= 1 && h->params.maxHistory <= 65535;
}

// One frame of a history on the default stream: the state `to` from the
// frame's records and signal and the state `from` (null: a reset frame).
struct HistoryState {
  rtg_camera pose;
  rtg_hit* hits;
  float* acc;
  unsigned short* len;
  float* m2;  // the second moment, carried under --ao-variance / --gather-variance only
};
static void accumulate_frame(rtg_context* ctx, const History& h, unsigned W, unsigned H, float zoom,
                             const void* src, const HistoryState* from, const HistoryState& to) {
  check(rtg_accumulate_device(ctx, to.hits, W, H, &h.params, src, from ? &from->pose : nullptr,
                              zoom, from ? from->hits : nullptr, from ? from->acc : nullptr,
                              from ? from->len : nullptr, from ? from->m2 : nullptr, to.acc, to.len,
                              to.m2, nullptr),
        "rtg_accumulate_device");
}

// "SIGMA[,minHistory]" of --ao-variance and --gather-variance; false when it is not that.
struct Variance {
  bool on = false;
  float sigma = 0.f;
  unsigned minHistory = 4;
};
static bool parse_variance(const char* s, Variance* v) {
  char tail = 0;
  const int k = sscanf(s, "%f,%u%c", &v->sigma, &v->minHistory, &tail);
  v->on = true;
  return k >= 1 && k <= 2 && v->minHistory <= 65535;
}

// rtg_variance_device of the accumulated state `s` with the filter's terms, then the filter's
// passes as rtg_svgf_device with RTG_SVGF_LUMA, into a new device buffer, on the default stream.
static void* svgf_frame(rtg_context* ctx, const HistoryState& s, unsigned W, unsigned H,
                        const rtg_filter_params& fp, const Variance& v) {
  const unsigned kind = fp.kind == RTG_FILTER_RGB ? RTG_FILTER_RGB : RTG_FILTER_GRAY;
  const size_t n = (size_t)W * H, out = n * (kind == RTG_FILTER_RGB ? 3 : 1) * sizeof(float);
  const rtg_variance_params vp = {kind, fp.flags, fp.normalLog2, fp.planeScale, v.minHistory};
  const rtg_svgf_params sp = {fp.passes, fp.normalLog2, fp.planeScale, kind,
                              fp.flags | RTG_SVGF_LUMA, v.sigma, 1e-6f};
  size_t bytes = 0;
  check(rtg_svgf_scratch(W, H, &sp, &bytes), "rtg_svgf_scratch");
  void *dst = nullptr, *scratch = nullptr;
  float *var = nullptr, *dstVar = nullptr;
  if (hipMalloc(&dst, out) != hipSuccess || hipMalloc(&var, n * sizeof(float)) != hipSuccess ||
      hipMalloc(&dstVar, n * sizeof(float)) != hipSuccess ||
      (bytes && hipMalloc(&scratch, bytes) != hipSuccess))
    check(RTG_ERR_NOMEM, "hipMalloc");
  check(rtg_variance_device(ctx, s.hits, W, H, &vp, s.acc, s.m2, s.len, var, nullptr),
        "rtg_variance_device");
  check(rtg_svgf_device(ctx, s.hits, W, H, &sp, s.acc, var, (float*)dst, dstVar, scratch, bytes,
                        nullptr),
        "rtg_svgf_device");
  if (hipDeviceSynchronize() != hipSuccess) check(RTG_ERR_HIP, "rtg_svgf_device");
  (void)hipFree(scratch);
  (void)hipFree(var);
  (void)hipFree(dstVar);
  return dst;
}

// "L[,planeScale[,normalLog2]]" of --ao-scale and --gather-scale; false when it is not that.
struct Scale {
  unsigned L = 0;  // 0: the signal is traced at full resolution
  float planeScale = 1.f;
  unsigned normalLog2 = 3;
};
static bool parse_scale(const char* s, Scale* sc) {
  char tail = 0;
  const int k = sscanf(s, "%u,%f,%u%c", &sc->L, &sc->planeScale, &sc->normalLog2, &tail);
  return k >= 1 && k <= 3 && sc->L >= 1 && sc->L <= RTG_UPSAMPLE_MAX_SCALE_LOG2 &&
         sc->normalLog2 <= 8;
}

// The device buffers of a mixed-resolution frame: the low frame's rays, records
// and values, the hole list with its scratch, and the holes' records and values.
struct Mixed {
  unsigned Wl, Hl;
  rtg_ray* lowRays;
  rtg_hit* lowHits;
  void* lowSig;
  rtg_hit* picked;
  void* pickedSig;
  unsigned* holes;
  unsigned* count;
  void* scratch;
  size_t scratchBytes;
};
static Mixed mixed_alloc(const Scale& sc, unsigned W, unsigned H, size_t valueBytes) {
  Mixed m = {};
  m.Wl = W >> sc.L;
  m.Hl = H >> sc.L;
  const size_t n = (size_t)W * H, nl = (size_t)m.Wl * m.Hl;
  check(rtg_upsample_scratch(W, H, 1, &m.scratchBytes), "rtg_upsample_scratch");
  if (hipMalloc(&m.lowRays, nl * sizeof(rtg_ray)) != hipSuccess ||
      hipMalloc(&m.lowHits, nl * sizeof(rtg_hit)) != hipSuccess ||
      hipMalloc(&m.lowSig, nl * valueBytes) != hipSuccess ||
      hipMalloc(&m.picked, n * sizeof(rtg_hit)) != hipSuccess ||
      hipMalloc(&m.pickedSig, n * valueBytes) != hipSuccess ||
      hipMalloc(&m.holes, n * sizeof(unsigned)) != hipSuccess ||
      hipMalloc(&m.count, sizeof(unsigned)) != hipSuccess ||
      hipMalloc(&m.scratch, m.scratchBytes) != hipSuccess)
    check(RTG_ERR_NOMEM, "hipMalloc");
  return m;
}
static void mixed_free(Mixed& m) {
  (void)hipFree(m.lowRays);
  (void)hipFree(m.lowHits);
  (void)hipFree(m.lowSig);
  (void)hipFree(m.picked);
  (void)hipFree(m.pickedSig);
  (void)hipFree(m.holes);
  (void)hipFree(m.count);
  (void)hipFree(m.scratch);
  m = Mixed{};
}
// The low frame's records of a pose, on the default stream.
static void mixed_low_hits(rtg_context* ctx, const Mixed& m, const rtg_camera& pose, float zoom) {
  check(rtg_camera_rays_device(ctx, &pose, m.Wl, m.Hl, zoom, 1.f, m.lowRays, nullptr),
        "rtg_camera_rays_device");
  check(rtg_intersect_device(ctx, m.lowRays, (size_t)m.Wl * m.Hl, m.lowHits, nullptr),
        "rtg_intersect_device");
}
// m.lowSig brought up to `dst` by the full records `hits`; the holes' records
// go to m.picked.  Returns the number of holes (one 4-byte copy back).
static size_t mixed_upsample(rtg_context* ctx, const Mixed& m, const Scale& sc, unsigned kind,
                             unsigned moreFlags, unsigned W, unsigned H, const rtg_hit* hits,
                             float* dst) {
  const size_t n = (size_t)W * H;
  const rtg_upsample_params up = {
      kind, RTG_UPSAMPLE_SAME_ID | RTG_UPSAMPLE_NORMAL | RTG_UPSAMPLE_PLANE | moreFlags,
      sc.normalLog2, sc.planeScale, sc.L};
  check(rtg_upsample_device(ctx, hits, W, H, &up, m.lowHits, m.Wl, m.Hl, m.lowSig, dst, m.holes,
                            (unsigned)n, m.count, m.scratch, m.scratchBytes, nullptr),
        "rtg_upsample_device");
  unsigned count = 0;
  if (hipMemcpy(&count, m.count, sizeof count, hipMemcpyDeviceToHost) != hipSuccess)
    check(RTG_ERR_HIP, "readback");
  check(rtg_hits_pick_device(ctx, hits, n, m.holes, count, m.picked, nullptr),
        "rtg_hits_pick_device");
  return count;
}

static bool parse_uint(const char* s, unsigned* out) {
  char* end;
  unsigned long v = strtoul(s, &end, 10);
  if (*end) return false;
  *out = (unsigned)v;
  return true;
}

int main(int argc, char** argv) {
  unsigned device = 0, W = 800, H = 600, nSph = 3, nLgt = 2, depth = 5, repeat = 1;
  unsigned long long seed = 42;
  float aa = 3.f, zoom = -4.f;
  std::string out = "testPPM.ppm", sceneIn, sceneOut, gbufOut, raysIn, hitsOut, radianceOut, aoOut;
  std::string matteOut, gatherOut, irrOut;
  bool probeGrid = false;
  unsigned gridDims[3] = {0, 0, 0}, gridRes = 16, gridBands = 3;
  rtg_irradiance_params irrParams = {1.0e-3f, RTG_IRR_LOBE_COSINE,
                                     RTG_IRR_VALID | RTG_IRR_FACING | RTG_IRR_VISIBLE};
  bool ao = false, matte = false, gather = false, gatherSkip = false;
  rtg_gather_params gatherParams = {0, 1.0e-3f, 0, 0};
  rtg_ao_params aoParams = {0, 0.f, 1.0e-3f, 0, 0};
  bool aoFilter = false, gatherFilter = false;
  rtg_filter_params aoFilterParams = {}, gatherFilterParams = {};
  History aoHistory, gatherHistory;
  Variance aoVariance, gatherVariance;
  Scale aoScale, gatherScale;
  unsigned gpus = 0;
  int semantics = RTG_SEMANTICS_CPU;
  bool posed = false;
  bool sortRays = false;
  rtg_camera camera;
  std::string viewsIn;  // --views
  bool cube = false, haveW = false, haveH = false, haveZoom = false;
  rtg_vec cubeEye = {0.f, 0.f, 0.f};
  unsigned shBands = 0;  // --sh
  std::string shOut;     // --sh-out
  for (int i = 1; i < argc; ++i) {
    auto need = [&](const char* opt) -> const char* {
      if (++i >= argc) {
        printf("Missing value for %s\n", opt);
        exit(1);
      }
      return argv[i];
    };
    const char* a = argv[i];
    if (!strcmp(a, "-h") || !strcmp(a, "--help")) {
      usage();
      return 0;
    } else if (!strcmp(a, "--list")) {
      int n = 0;
      check(rtg_device_count(&n), "rtg_device_count");
      if (n == 0) printf("No devices found.\n");
      printf("\nDevices:\n");
      for (int d = 0; d < n; ++d) {
        char buf[256];
        check(rtg_device_info(d, buf, sizeof buf), "rtg_device_info");
        printf("%2d: %s\n", d, buf);
      }
      printf("\n");
      return 0;
    } else if (!strcmp(a, "--device")) {
      if (!parse_uint(need(a), &device)) { printf("Invalid device index\n"); return 1; }
    } else if (!strcmp(a, "--width")) {
      if (!parse_uint(need(a), &W)) { printf("Invalid width\n"); return 1; }
      haveW = true;
    } else if (!strcmp(a, "--height")) {
      if (!parse_uint(need(a), &H)) { printf("Invalid height\n"); return 1; }
      haveH = true;
    } else if (!strcmp(a, "--spheres")) {
      if (!parse_uint(need(a), &nSph)) { printf("Invalid sphere count\n"); return 1; }
    } else if (!strcmp(a, "--lights")) {
      if (!parse_uint(need(a), &nLgt)) { printf("Invalid light count\n"); return 1; }
    } else if (!strcmp(a, "--depth")) {
      if (!parse_uint(need(a), &depth)) { printf("Invalid depth\n"); return 1; }
    } else if (!strcmp(a, "--repeat")) {
      if (!parse_uint(need(a), &repeat) || repeat == 0) { printf("Invalid repeat\n"); return 1; }
    } else if (!strcmp(a, "--aa")) {
      aa = strtof(need(a), nullptr);
    } else if (!strcmp(a, "--zoom")) {
      zoom = strtof(need(a), nullptr);
      haveZoom = true;
    } else if (!strcmp(a, "--seed")) {
      seed = strtoull(need(a), nullptr, 10);
    } else if (!strcmp(a, "--out")) {
      out = need(a);
    } else if (!strcmp(a, "--gbuffer")) {
      gbufOut = need(a);
    } else if (!strcmp(a, "--rays")) {
      raysIn = need(a);
    } else if (!strcmp(a, "--sort-rays")) {
      sortRays = true;
    } else if (!strcmp(a, "--hits")) {
      hitsOut = need(a);
    } else if (!strcmp(a, "--radiance")) {
      radianceOut = need(a);
    } else if (!strcmp(a, "--camera")) {
      if (!parse_pose(need(a), &camera)) {
        printf("Invalid camera (ex,ey,ez,tx,ty,tz[,ux,uy,uz])\n");
        return 1;
      }
      posed = true;
    } else if (!strcmp(a, "--views")) {
      viewsIn = need(a);
    } else if (!strcmp(a, "--cube")) {
      char tail = 0;
      if (sscanf(need(a), "%f,%f,%f%c", &cubeEye.x, &cubeEye.y, &cubeEye.z, &tail) != 3) {
        printf("Invalid cube (ex,ey,ez)\n");
        return 1;
      }
      cube = true;
    } else if (!strcmp(a, "--sh")) {
      if (!parse_uint(need(a), &shBands) || shBands < 1 || shBands > 4) {
        printf("Invalid SH band count (1..4)\n");
        return 1;
      }
    } else if (!strcmp(a, "--sh-out")) {
      shOut = need(a);
    } else if (!strcmp(a, "--ao")) {
      char tail = 0;
      const int k = sscanf(need(a), "%u,%f,%f,%u%c", &aoParams.samples, &aoParams.radius,
                           &aoParams.bias, &aoParams.seed, &tail);
      if (k < 2 || k > 4 || aoParams.samples < 1 || aoParams.samples > RTG_AO_MAX_SAMPLES) {
        printf("Invalid ao (K,radius[,bias[,seed]], K in 1..%d)\n", RTG_AO_MAX_SAMPLES);
        return 1;
      }
      if (k == 4) aoParams.flags = RTG_AO_JITTER;
      ao = true;
    } else if (!strcmp(a, "--ao-out")) {
      aoOut = need(a);
    } else if (!strcmp(a, "--gather")) {
      char tail = 0;
      const int k = sscanf(need(a), "%u,%f,%u%c", &gatherParams.samples, &gatherParams.bias,
                           &gatherParams.seed, &tail);
      if (k < 1 || k > 3 || gatherParams.samples < 1 ||
          gatherParams.samples > RTG_GATHER_MAX_SAMPLES) {
        printf("Invalid gather (K[,bias[,seed]], K in 1..%d)\n", RTG_GATHER_MAX_SAMPLES);
        return 1;
      }
      if (k == 3) gatherParams.flags |= RTG_GATHER_JITTER;
      gather = true;
    } else if (!strcmp(a, "--gather-out")) {
      gatherOut = need(a);
    } else if (!strcmp(a, "--gather-skip")) {
      gatherSkip = true;
    } else if (!strcmp(a, "--ao-filter") || !strcmp(a, "--gather-filter")) {
      const bool forAo = a[2] == 'a';
      if (!parse_filter(need(a), forAo ? &aoFilterParams : &gatherFilterParams)) {
        printf("Invalid filter (PASSES[,planeScale[,normalLog2]], PASSES in 1..%d, normalLog2 in "
               "0..8)\n", RTG_FILTER_MAX_PASSES);
        return 1;
      }
      (forAo ? aoFilter : gatherFilter) = true;
    } else if (!strcmp(a, "--ao-history") || !strcmp(a, "--gather-history")) {
      if (!parse_history(need(a), a[2] == 'a' ? &aoHistory : &gatherHistory)) {
        printf("Invalid history (FILE[,maxHistory], maxHistory in 1..65535)\n");
        return 1;
      }
    } else if (!strcmp(a, "--ao-variance") || !strcmp(a, "--gather-variance")) {
      if (!parse_variance(need(a), a[2] == 'a' ? &aoVariance : &gatherVariance)) {
        printf("Invalid variance (SIGMA[,minHistory], minHistory in 0..65535)\n");
        return 1;
      }
    } else if (!strcmp(a, "--ao-scale") || !strcmp(a, "--gather-scale")) {
      if (!parse_scale(need(a), a[2] == 'a' ? &aoScale : &gatherScale)) {
        printf("Invalid scale (L[,planeScale[,normalLog2]], L in 1..%d, normalLog2 in 0..8)\n",
               RTG_UPSAMPLE_MAX_SCALE_LOG2);
        return 1;
      }
    } else if (!strcmp(a, "--matte")) {
      matteOut = need(a);
      matte = true;
    } else if (!strcmp(a, "--probe-grid")) {
      char tail = 0;
      const int k = sscanf(need(a), "%u,%u,%u,%u,%u%c", gridDims, gridDims + 1, gridDims + 2,
                           &gridRes, &gridBands, &tail);
      if (k < 3 || k > 5 || !gridDims[0] || !gridDims[1] || !gridDims[2] || !gridRes ||
          gridBands < 1 || gridBands > 3) {
        printf("Invalid probe grid (nx,ny,nz[,res[,bands]], each >= 1, bands in 1..3)\n");
        return 1;
      }
      probeGrid = true;
    } else if (!strcmp(a, "--irradiance")) {
      irrOut = need(a);
    } else if (!strcmp(a, "--irr-flags")) {
      if (!parse_irr_flags(need(a), &irrParams.flags)) {
        printf("Invalid irradiance flags (a comma list of valid, facing, visible, or none)\n");
        return 1;
      }
    } else if (!strcmp(a, "--irr-bias")) {
      irrParams.bias = strtof(need(a), nullptr);
    } else if (!strcmp(a, "--scene")) {
      sceneIn = need(a);
    } else if (!strcmp(a, "--save-scene")) {
      sceneOut = need(a);
    } else if (!strcmp(a, "--semantics")) {
      const char* v = need(a);
      if (!strcmp(v, "cpu")) semantics = RTG_SEMANTICS_CPU;
      else if (!strcmp(v, "opencl")) semantics = RTG_SEMANTICS_OPENCL;
      else { printf("Invalid semantics %s (cpu|opencl)\n", v); return 1; }
    } else if (!strcmp(a, "--gpus")) {
      if (!parse_uint(need(a), &gpus) || gpus == 0) { printf("Invalid GPU count\n"); return 1; }
    } else {
      printf("Unknown option %s\n", a);
      usage();
      return 1;
    }
  }

  if (raysIn.empty() ? !hitsOut.empty() : (hitsOut.empty() && radianceOut.empty())) {
    printf("--rays and --hits go together\n");
    return 1;
  }
  if (raysIn.empty() && sortRays) {
    printf("--sort-rays needs --rays\n");
    return 1;
  }
  if (raysIn.empty() && !radianceOut.empty()) {
    printf("--radiance needs --rays\n");
    return 1;
  }

  if (ao == aoOut.empty()) {
    printf("--ao and --ao-out go together\n");
    return 1;
  }

  if (matte && (matteOut.empty() || matteOut == out || W == 0 || H == 0)) {
    printf("Invalid matte (a file other than --out, for a frame with pixels)\n");
    return 1;
  }

  if (probeGrid == irrOut.empty() || (probeGrid && (irrOut == out || W == 0 || H == 0))) {
    printf("--probe-grid and --irradiance go together (a file other than --out, for a frame with "
           "pixels)\n");
    return 1;
  }

  if (gather == gatherOut.empty() || (gatherSkip && !gather) ||
      (gather && (gatherOut == out || W == 0 || H == 0))) {
    printf("--gather and --gather-out go together (a file other than --out, for a frame with "
           "pixels; --gather-skip needs both)\n");
    return 1;
  }
  if (gatherSkip) gatherParams.flags |= RTG_GATHER_SKIP_NONFINITE;
  if ((aoFilter && !ao) || (gatherFilter && !gather)) {
    printf("--ao-filter needs --ao, --gather-filter needs --gather\n");
    return 1;
  }
  if ((aoHistory.on && !ao) || (gatherHistory.on && !gather)) {
    printf("--ao-history needs --ao, --gather-history needs --gather\n");
    return 1;
  }
  if ((aoVariance.on && !aoFilter) || (gatherVariance.on && !gatherFilter)) {
    printf("--ao-variance needs --ao-filter, --gather-variance needs --gather-filter\n");
    return 1;
  }
  if ((aoScale.L && !ao) || (gatherScale.L && !gather)) {
    printf("--ao-scale needs --ao, --gather-scale needs --gather\n");
    return 1;
  }
  for (const Scale* sc : {&aoScale, &gatherScale})
    if (sc->L && (W == 0 || H == 0 || W % (1u << sc->L) || H % (1u << sc->L))) {
      printf("A frame of %ux%u does not divide by the scale's factor %u\n", W, H, 1u << sc->L);
      return 1;
    }
  // the variance needs the accumulated moments: without a history, of one reset frame
  const bool aoAccum = aoHistory.on || aoVariance.on;
  const bool gatherAccum = gatherHistory.on || gatherVariance.on;
  // (an accumulated frame is floats, and so is an upsampled one: the filter then takes it as GRAY)
  aoFilterParams.kind = aoAccum || aoScale.L ? RTG_FILTER_GRAY : RTG_FILTER_COUNT;
  gatherFilterParams.kind = RTG_FILTER_RGB;
  if (gatherSkip) gatherFilterParams.flags |= RTG_FILTER_SKIP_NONFINITE;
  aoHistory.params.kind = aoScale.L ? RTG_FILTER_GRAY : RTG_FILTER_COUNT;
  gatherHistory.params.kind = RTG_FILTER_RGB;
  if (gatherSkip) gatherHistory.params.flags |= RTG_ACCUM_SKIP_NONFINITE;
  if (aoHistory.on) aoHistory.poses = read_poses(aoHistory.file);
  if (gatherHistory.on) gatherHistory.poses = read_poses(gatherHistory.file);

  if (posed && gpus) {
    printf("--camera renders on one device\n");
    return 1;
  }

  const bool manyViews = cube || !viewsIn.empty();
  if (manyViews && (cube == !viewsIn.empty() || posed || gpus || ao || matte || gather ||
                    probeGrid || !gbufOut.empty() || !raysIn.empty())) {
    printf("--views or --cube renders alone: one of them, on one device, without --camera,\n"
           "--gbuffer, --rays, --ao, --matte, --gather or --probe-grid\n");
    return 1;
  }
  if ((shBands != 0) != !shOut.empty() || (shBands && !cube)) {
    printf("--sh BANDS and --sh-out FILE go together, with --cube\n");
    return 1;
  }
  if (cube) {  // rtg_camera_cube's poses are for a square frame at zoom -1
    if (!haveW) W = haveH ? H : 64;
    if (!haveH) H = W;
    if (W != H || (haveZoom && zoom != -1.f)) {
      printf("--cube renders square frames at --zoom -1 (got %ux%u, zoom %g)\n", W, H,
             haveZoom ? (double)zoom : -1.0);
      return 1;
    }
    zoom = -1.f;
  }
  std::vector<rtg_camera> views;
  if (cube) {
    views.resize(6);
    check(rtg_camera_cube(&cubeEye, views.data()), "rtg_camera_cube");
  } else if (manyViews) {
    views = read_poses(viewsIn);
  }

  std::vector<rtg_sphere> spheres;
  std::vector<rtg_light> lights;
  if (!sceneIn.empty()) {
    check(rtg_scene_load(sceneIn.c_str(), nullptr, 0, &nSph, nullptr, 0, &nLgt),
          "rtg_scene_load");
    spheres.resize(nSph);
    lights.resize(nLgt);
    check(rtg_scene_load(sceneIn.c_str(), spheres.data(), nSph, &nSph, lights.data(), nLgt,
                         &nLgt),
          "rtg_scene_load");
  } else {
    spheres.resize(nSph);
    lights.resize(nLgt);
    check(rtg_scene_generate(seed, nSph, nLgt, spheres.data(), lights.data()),
          "rtg_scene_generate");
  }
  if (!sceneOut.empty())
    check(rtg_scene_save(sceneOut.c_str(), spheres.data(), nSph, lights.data(), nLgt),
          "rtg_scene_save");

  char info[256];
  check(rtg_device_info((int)device, info, sizeof info), "rtg_device_info");
  printf("Device %u: %s\n", device, info);

  if (manyViews) {  // one context, the poses up, one launch, every frame down
    const size_t nV = views.size(), per = (size_t)W * H;
    std::vector<rtg_vec> frames(nV * per);
    rtg_context* ctx = nullptr;
    check(rtg_context_create((int)device, &ctx), "rtg_context_create");
    check(rtg_context_set_semantics(ctx, semantics), "rtg_context_set_semantics");
    check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
          "rtg_context_set_scene");
    if (shBands) {  // the probe: poses in, coefficients out, no face anywhere
      const unsigned K = shBands * shBands;
      const rtg_fold_params fp = {6, K, 0};
      std::vector<float> wts(6 * per * K);
      check(rtg_cube_sh_weights(W, shBands, aa, wts.data()), "rtg_cube_sh_weights");
      size_t scratchBytes = 0;
      check(rtg_views_fold_scratch(nV, W, H, K, &scratchBytes), "rtg_views_fold_scratch");
      rtg_camera* dPoses = nullptr;
      float* dW = nullptr;
      rtg_vec* dOut = nullptr;
      void* dScratch = nullptr;
      if (hipMalloc(&dPoses, nV * sizeof(rtg_camera)) != hipSuccess ||
          hipMalloc(&dW, wts.size() * sizeof(float)) != hipSuccess ||
          hipMalloc(&dOut, K * sizeof(rtg_vec)) != hipSuccess ||
          hipMalloc(&dScratch, scratchBytes) != hipSuccess)
        check(RTG_ERR_NOMEM, "hipMalloc");
      if (hipMemcpy(dPoses, views.data(), nV * sizeof(rtg_camera), hipMemcpyHostToDevice) !=
              hipSuccess ||
          hipMemcpy(dW, wts.data(), wts.size() * sizeof(float), hipMemcpyHostToDevice) !=
              hipSuccess)
        check(RTG_ERR_HIP, "upload");
      check(rtg_render_views_fold_device(ctx, dPoses, nV, W, H, zoom, aa, (int)depth + 1, &fp, dW,
                                         dOut, nullptr, dScratch, scratchBytes, nullptr),
            "rtg_render_views_fold_device");
      std::vector<rtg_vec> coef(K);
      if (hipMemcpy(coef.data(), dOut, K * sizeof(rtg_vec), hipMemcpyDeviceToHost) != hipSuccess)
        check(RTG_ERR_HIP, "readback");
      (void)hipFree(dPoses);
      (void)hipFree(dW);
      (void)hipFree(dOut);
      (void)hipFree(dScratch);
      rtg_context_destroy(ctx);
      FILE* f = fopen(shOut.c_str(), "w");
      if (!f) {
        fprintf(stderr, "Error: can't write %s\n", shOut.c_str());
        exit(EXIT_FAILURE);
      }
      for (unsigned k = 0; k < K; ++k)
        fprintf(f, "%.9g %.9g %.9g\n", (double)coef[k].x, (double)coef[k].y, (double)coef[k].z);
      fclose(f);
      printf("Wrote %s (%u SH coefficients of the probe at %g,%g,%g, %ux%u faces)\n",
             shOut.c_str(), K, (double)cubeEye.x, (double)cubeEye.y, (double)cubeEye.z, W, H);
      return 0;
    }
    rtg_camera* dv = nullptr;
    rtg_vec* d = nullptr;
    if (nV && per) {
      if (hipMalloc(&dv, nV * sizeof(rtg_camera)) != hipSuccess ||
          hipMalloc(&d, frames.size() * sizeof(rtg_vec)) != hipSuccess)
        check(RTG_ERR_NOMEM, "hipMalloc");
      if (hipMemcpy(dv, views.data(), nV * sizeof(rtg_camera), hipMemcpyHostToDevice) !=
          hipSuccess)
        check(RTG_ERR_HIP, "upload");
    }
    if (nV)
      check(rtg_render_views_device(ctx, dv, nV, W, H, zoom, aa, (int)depth + 1, d, nullptr),
            "rtg_render_views_device");
    if (nV && per &&
        hipMemcpy(frames.data(), d, frames.size() * sizeof(rtg_vec), hipMemcpyDeviceToHost) !=
            hipSuccess)
      check(RTG_ERR_HIP, "readback");
    (void)hipFree(dv);
    (void)hipFree(d);
    rtg_context_destroy(ctx);
    const size_t dot = out.rfind('.'), slash = out.find_last_of('/');
    const bool ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
    const std::string stem = ext ? out.substr(0, dot) : out, suffix = ext ? out.substr(dot) : "";
    for (size_t k = 0; k < nV; ++k) {  // each frame scaled by its own largest colour, as --camera's
      const std::string name = stem + "." + std::to_string(k) + suffix;
      const float mx = rtg_max_colour(frames.data() + k * per, per);
      check(rtg_save_ppm(frames.data() + k * per, name.c_str(), (int)W, (int)H, mx),
            "rtg_save_ppm");
      printf("Wrote %s (%ux%u, view %zu of %zu, max colour %.8g)\n", name.c_str(), W, H, k, nV,
             (double)mx);
    }
    return 0;
  }

  std::vector<rtg_vec> pixels((size_t)W * H);
  rtg_multi* mg = nullptr;  // --gpus: one communicator for every repeat
  if (gpus) {
    std::vector<int> devs(gpus);
    for (unsigned g = 0; g < gpus; ++g) devs[g] = (int)g;
    check(rtg_multi_create(devs.data(), (int)gpus, &mg), "rtg_multi_create");
    check(rtg_multi_set_scene(mg, spheres.data(), nSph, lights.data(), nLgt),
          "rtg_multi_set_scene");
  }
  double best = 1e30;
  for (unsigned r = 0; r < repeat; ++r) {
    auto t0 = std::chrono::steady_clock::now();
    if (semantics != RTG_SEMANTICS_CPU) {  // persistent context: semantics is per context
      if (gpus) { printf("--semantics opencl renders on one device\n"); return 1; }
      rtg_context* ctx = nullptr;
      check(rtg_context_create((int)device, &ctx), "rtg_context_create");
      check(rtg_context_set_semantics(ctx, semantics), "rtg_context_set_semantics");
      check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
            "rtg_context_set_scene");
      rtg_vec* d = nullptr;
      if (hipMalloc(&d, pixels.size() * sizeof(rtg_vec)) != hipSuccess)
        check(RTG_ERR_NOMEM, "hipMalloc");
      if (posed)
        check(rtg_render_camera_device(ctx, &camera, W, H, zoom, aa, (int)depth + 1, d, nullptr),
              "rtg_render_camera_device");
      else
        check(rtg_render_device(ctx, W, H, zoom, aa, (int)depth + 1, 16, 0, 1, d, nullptr),
              "rtg_render_device");
      if (hipMemcpy(pixels.data(), d, pixels.size() * sizeof(rtg_vec),
                    hipMemcpyDeviceToHost) != hipSuccess)
        check(RTG_ERR_HIP, "readback");
      (void)hipFree(d);
      rtg_context_destroy(ctx);
    } else if (gpus) {
      float tm[3];
      check(rtg_multi_render(mg, W, H, zoom, aa, (int)depth + 1, 16, pixels.data(), tm),
            "rtg_multi_render");
      printf("  %u GPUs: render %.3f ms (slowest device), gather+assemble %.3f ms\n", gpus,
             (double)tm[0], (double)tm[1]);
    } else if (posed) {
      check(rtg_render_camera((int)device, spheres.data(), nSph, lights.data(), nLgt, &camera, W, H,
                              zoom, aa, (int)depth + 1, pixels.data()),
            "rtg_render_camera");
    } else {
      check(rtg_render((int)device, spheres.data(), nSph, lights.data(), nLgt, W, H, zoom, aa,
                       (int)depth + 1, pixels.data()),
            "rtg_render");
    }
    auto t1 = std::chrono::steady_clock::now();
    double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (ms < best) best = ms;
  }
  if (mg) rtg_multi_destroy(mg);
  // main.cpp:374 prints integer milliseconds; report the measured value.
  printf("Exec time: %.5f ms (end to end: upload, render, readback)\n", best);

  const float mx = rtg_max_colour(pixels.data(), pixels.size());
  check(rtg_save_ppm(pixels.data(), out.c_str(), (int)W, (int)H, mx), "rtg_save_ppm");
  printf("Wrote %s (%ux%u, %u spheres, %u lights, depth %u, max colour %.8g)\n", out.c_str(), W,
         H, nSph, nLgt, depth, (double)mx);

  if (!gbufOut.empty()) {  // the records as they lie in memory (the GPU hosts are little-endian)
    std::vector<rtg_gbuf_px> gbuf((size_t)W * H);
    check(rtg_gbuffer((int)device, spheres.data(), nSph, W, H, zoom, aa, gbuf.data()),
          "rtg_gbuffer");
    FILE* f = fopen(gbufOut.c_str(), "wb");
    if (!f || fwrite(gbuf.data(), sizeof(rtg_gbuf_px), gbuf.size(), f) != gbuf.size() ||
        fclose(f) != 0) {
      fprintf(stderr, "Error: can't write %s\n", gbufOut.c_str());
      exit(EXIT_FAILURE);
    }
    printf("Wrote %s (%zu G-buffer records of %zu bytes)\n", gbufOut.c_str(), gbuf.size(),
           sizeof(rtg_gbuf_px));
  }

  if (ao) {  // pose -> primary rays -> hits -> counts, all on the device; only the counts come back
    const size_t n = (size_t)W * H;
    const unsigned K = aoParams.samples;
    if (!posed) rtg_camera_identity(&camera);
    std::vector<rtg_vec> table(K);
    check(rtg_ao_directions(K, table.data()), "rtg_ao_directions");
    rtg_context* ctx = nullptr;
    check(rtg_context_create((int)device, &ctx), "rtg_context_create");
    check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
          "rtg_context_set_scene");
    rtg_ray* dr = nullptr;
    rtg_vec* dd = nullptr;
    unsigned short* dc = nullptr;
    float* dsig = nullptr;  // --ao-scale: the upsampled counts with the holes' own placed in
    Mixed mixed = {};
    if (aoScale.L) {
      mixed = mixed_alloc(aoScale, W, H, sizeof(unsigned short));
      if (hipMalloc(&dsig, n * sizeof(float)) != hipSuccess) check(RTG_ERR_NOMEM, "hipMalloc");
    }
    // the frames of --ao-history ping-pong between two states; without it
    // there is one frame and only its records
    const size_t frames = aoHistory.on ? aoHistory.poses.size() + 1 : 1;
    HistoryState st[2] = {};
    if (hipMalloc(&dr, n * sizeof(rtg_ray)) != hipSuccess ||
        hipMalloc(&dd, K * sizeof(rtg_vec)) != hipSuccess ||
        hipMalloc(&dc, n * sizeof(unsigned short)) != hipSuccess)
      check(RTG_ERR_NOMEM, "hipMalloc");
    for (size_t k = 0; k < (frames > 1 ? 2u : 1u); ++k)
      if (hipMalloc(&st[k].hits, n * sizeof(rtg_hit)) != hipSuccess ||
          (aoAccum && (hipMalloc(&st[k].acc, n * sizeof(float)) != hipSuccess ||
                       hipMalloc(&st[k].len, n * sizeof(unsigned short)) != hipSuccess)) ||
          (aoVariance.on && hipMalloc(&st[k].m2, n * sizeof(float)) != hipSuccess))
        check(RTG_ERR_NOMEM, "hipMalloc");
    if (hipMemcpy(dd, table.data(), K * sizeof(rtg_vec), hipMemcpyHostToDevice) != hipSuccess)
      check(RTG_ERR_HIP, "upload");
    size_t holesSeen = 0;
    for (size_t k = 0; k < frames; ++k) {
      HistoryState& cur = st[k & 1];
      cur.pose = k + 1 < frames ? aoHistory.poses[k] : camera;
      rtg_ao_params ap = aoParams;
      ap.seed += (unsigned)k;
      check(rtg_camera_rays_device(ctx, &cur.pose, W, H, zoom, 1.f, dr, nullptr),
            "rtg_camera_rays_device");
      check(rtg_intersect_device(ctx, dr, n, cur.hits, nullptr), "rtg_intersect_device");
      if (aoScale.L) {  // the probes on the low frame, then on the holes alone
        mixed_low_hits(ctx, mixed, cur.pose, zoom);
        check(rtg_ao_device(ctx, mixed.lowHits, (size_t)mixed.Wl * mixed.Hl, &ap, dd, K,
                            (unsigned short*)mixed.lowSig, nullptr),
              "rtg_ao_device");
        const size_t m =
            mixed_upsample(ctx, mixed, aoScale, RTG_FILTER_COUNT, 0, W, H, cur.hits, dsig);
        if (m) {
          check(rtg_ao_device(ctx, mixed.picked, m, &ap, dd, K, (unsigned short*)mixed.pickedSig,
                              nullptr),
                "rtg_ao_device");
          check(rtg_values_place_device(ctx, RTG_FILTER_COUNT, mixed.pickedSig, mixed.holes, m, n,
                                        dsig, nullptr),
                "rtg_values_place_device");
        }
        holesSeen += m;
      } else {
        check(rtg_ao_device(ctx, cur.hits, n, &ap, dd, K, dc, nullptr), "rtg_ao_device");
      }
      if (aoAccum)
        accumulate_frame(ctx, aoHistory, W, H, zoom, aoScale.L ? (const void*)dsig : dc,
                         k ? &st[(k - 1) & 1] : nullptr, cur);
    }
    const HistoryState& last = st[(frames - 1) & 1];
    std::vector<unsigned short> counts(n);
    std::vector<float> smooth;
    if (!aoScale.L &&
        hipMemcpy(counts.data(), dc, n * sizeof(unsigned short), hipMemcpyDeviceToHost) !=
            hipSuccess)
      check(RTG_ERR_HIP, "readback");
    if (aoFilter || aoHistory.on || aoScale.L) {  // the frame never leaves the device on its way to the filter
      const void* sig = aoScale.L ? (const void*)dsig : dc;
      void* df = aoVariance.on ? svgf_frame(ctx, last, W, H, aoFilterParams, aoVariance)
                 : aoFilter    ? filter_frame(ctx, last.hits, W, H, aoFilterParams,
                                              aoHistory.on ? (const void*)last.acc : sig)
                 : aoHistory.on ? (void*)last.acc
                                : (void*)dsig;
      smooth.resize(n);
      if (hipMemcpy(smooth.data(), df, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        check(RTG_ERR_HIP, "readback");
      if (aoFilter) (void)hipFree(df);
    }
    (void)hipFree(dr);
    (void)hipFree(dd);
    (void)hipFree(dc);
    (void)hipFree(dsig);
    mixed_free(mixed);
    for (HistoryState& s : st) {
      (void)hipFree(s.hits);
      (void)hipFree(s.acc);
      (void)hipFree(s.len);
      (void)hipFree(s.m2);
    }
    rtg_context_destroy(ctx);
    std::vector<unsigned char> grey(n);
    for (size_t k = 0; k < n; ++k) grey[k] = (unsigned char)((255u * counts[k]) / K);
    for (size_t k = 0; k < smooth.size(); ++k) {
      const float v = 255.f * smooth[k] / (float)K;
      grey[k] = (unsigned char)(v > 0.f ? (v < 255.f ? v : 255.f) : 0.f);  // (a NaN: 0)
    }
    FILE* f = fopen(aoOut.c_str(), "wb");
    if (!f || fprintf(f, "P5\n%u %u\n255\n", W, H) < 0 ||
        fwrite(grey.data(), 1, n, f) != n || fclose(f) != 0) {
      fprintf(stderr, "Error: can't write %s\n", aoOut.c_str());
      exit(EXIT_FAILURE);
    }
    printf("Wrote %s (%ux%u, %u probes of length %.8g per primary hit", aoOut.c_str(), W, H, K,
           (double)aoParams.radius);
    if (aoHistory.on) printf(", accumulated over %zu frames", frames);
    if (aoScale.L)
      printf(", traced at %ux%u and on %zu holes", W >> aoScale.L, H >> aoScale.L, holesSeen);
    printf(")\n");
  }

  if (matte) {  // pose -> primary rays -> hits -> direct light -> bytes, all on the device
    const size_t n = (size_t)W * H;
    if (!posed) rtg_camera_identity(&camera);
    rtg_context* ctx = nullptr;
    check(rtg_context_create((int)device, &ctx), "rtg_context_create");
    check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
          "rtg_context_set_scene");
    rtg_ray* dr = nullptr;
    rtg_hit* dh = nullptr;
    rtg_vec* dl = nullptr;
    float* dmax = nullptr;
    unsigned char* db = nullptr;
    if (hipMalloc(&dr, n * sizeof(rtg_ray)) != hipSuccess ||
        hipMalloc(&dh, n * sizeof(rtg_hit)) != hipSuccess ||
        hipMalloc(&dl, n * sizeof(rtg_vec)) != hipSuccess ||
        hipMalloc(&dmax, sizeof(float)) != hipSuccess || hipMalloc(&db, n * 3) != hipSuccess)
      check(RTG_ERR_NOMEM, "hipMalloc");
    check(rtg_camera_rays_device(ctx, &camera, W, H, zoom, 1.f, dr, nullptr),
          "rtg_camera_rays_device");
    check(rtg_intersect_device(ctx, dr, n, dh, nullptr), "rtg_intersect_device");
    check(rtg_matte_device(ctx, dh, n, dl, nullptr, nullptr), "rtg_matte_device");
    check(rtg_max_colour_device(ctx, dl, n, dmax, nullptr), "rtg_max_colour_device");
    check(rtg_ppm_bytes_device(ctx, dl, n, dmax, db, nullptr), "rtg_ppm_bytes_device");
    std::vector<unsigned char> bytes(n * 3);
    float lightMax = 0.f;
    if (hipMemcpy(bytes.data(), db, n * 3, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&lightMax, dmax, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      check(RTG_ERR_HIP, "readback");
    (void)hipFree(dr);
    (void)hipFree(dh);
    (void)hipFree(dl);
    (void)hipFree(dmax);
    (void)hipFree(db);
    rtg_context_destroy(ctx);
    FILE* f = fopen(matteOut.c_str(), "wb");
    if (!f || fprintf(f, "P6\n%u %u\n255\n", W, H) < 0 ||
        fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) {
      fprintf(stderr, "Error: can't write %s\n", matteOut.c_str());
      exit(EXIT_FAILURE);
    }
    printf("Wrote %s (%ux%u, direct light of %u lights per primary hit, max %.8g)\n",
           matteOut.c_str(), W, H, nLgt, (double)lightMax);
  }

  if (probeGrid) {  // the bake, then pose -> primary rays -> hits -> the grid's light -> bytes
    const size_t n = (size_t)W * H;
    if (!posed) rtg_camera_identity(&camera);
    const rtg_probe_grid grid = grid_over(spheres, gridDims, gridBands);
    const size_t probes = (size_t)grid.nx * grid.ny * grid.nz, nV = 6 * probes;
    const unsigned K = gridBands * gridBands;
    std::vector<rtg_vec> pts(probes);
    check(rtg_probe_grid_points(&grid, pts.data()), "rtg_probe_grid_points");
    std::vector<rtg_camera> poses(nV);
    check(rtg_probe_grid_poses(&grid, poses.data()), "rtg_probe_grid_poses");
    std::vector<float> wts((size_t)6 * gridRes * gridRes * K);
    check(rtg_cube_sh_weights(gridRes, gridBands, 1.f, wts.data()), "rtg_cube_sh_weights");
    const rtg_fold_params fp = {6, K, RTG_FOLD_SKIP_NONFINITE};
    size_t scratchBytes = 0;
    check(rtg_views_fold_scratch(nV, gridRes, gridRes, K, &scratchBytes), "rtg_views_fold_scratch");
    rtg_context* ctx = nullptr;
    check(rtg_context_create((int)device, &ctx), "rtg_context_create");
    check(rtg_context_set_semantics(ctx, semantics), "rtg_context_set_semantics");
    check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
          "rtg_context_set_scene");
    rtg_camera* dPoses = nullptr;
    float* dW = nullptr;
    rtg_vec *dCoef = nullptr, *dPts = nullptr, *dl = nullptr;
    void* dScratch = nullptr;
    int* dIn = nullptr;
    unsigned char *dValid = nullptr, *db = nullptr;
    rtg_ray* dr = nullptr;
    rtg_hit* dh = nullptr;
    float* dmax = nullptr;
    if (hipMalloc(&dPoses, nV * sizeof(rtg_camera)) != hipSuccess ||
        hipMalloc(&dW, wts.size() * sizeof(float)) != hipSuccess ||
        hipMalloc(&dCoef, probes * K * sizeof(rtg_vec)) != hipSuccess ||
        hipMalloc(&dScratch, scratchBytes) != hipSuccess ||
        hipMalloc(&dPts, probes * sizeof(rtg_vec)) != hipSuccess ||
        hipMalloc(&dIn, probes * sizeof(int)) != hipSuccess ||
        hipMalloc(&dValid, probes) != hipSuccess ||
        hipMalloc(&dr, n * sizeof(rtg_ray)) != hipSuccess ||
        hipMalloc(&dh, n * sizeof(rtg_hit)) != hipSuccess ||
        hipMalloc(&dl, n * sizeof(rtg_vec)) != hipSuccess ||
        hipMalloc(&dmax, sizeof(float)) != hipSuccess || hipMalloc(&db, n * 3) != hipSuccess)
      check(RTG_ERR_NOMEM, "hipMalloc");
    if (hipMemcpy(dPoses, poses.data(), nV * sizeof(rtg_camera), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(dW, wts.data(), wts.size() * sizeof(float), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(dPts, pts.data(), probes * sizeof(rtg_vec), hipMemcpyHostToDevice) != hipSuccess)
      check(RTG_ERR_HIP, "upload");
    check(rtg_render_views_fold_device(ctx, dPoses, nV, gridRes, gridRes, -1.f, 1.f,
                                       (int)depth + 1, &fp, dW, dCoef, nullptr, dScratch,
                                       scratchBytes, nullptr),
          "rtg_render_views_fold_device");
    // validity: a probe inside a sphere is left out (rtg_contains* < 0 is valid)
    check(rtg_contains_device(ctx, dPts, probes, dIn, nullptr), "rtg_contains_device");
    std::vector<int> in(probes);
    if (hipMemcpy(in.data(), dIn, probes * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
      check(RTG_ERR_HIP, "readback");
    std::vector<unsigned char> valid(probes);
    size_t nValid = 0;
    for (size_t p = 0; p < probes; ++p) nValid += valid[p] = in[p] < 0;
    if (hipMemcpy(dValid, valid.data(), probes, hipMemcpyHostToDevice) != hipSuccess)
      check(RTG_ERR_HIP, "upload");
    check(rtg_camera_rays_device(ctx, &camera, W, H, zoom, 1.f, dr, nullptr),
          "rtg_camera_rays_device");
    check(rtg_intersect_device(ctx, dr, n, dh, nullptr), "rtg_intersect_device");
    check(rtg_irradiance_device(ctx, dh, n, &grid, dCoef, dValid, &irrParams, dl, nullptr,
                                nullptr),
          "rtg_irradiance_device");
    check(rtg_max_colour_device(ctx, dl, n, dmax, nullptr), "rtg_max_colour_device");
    check(rtg_ppm_bytes_device(ctx, dl, n, dmax, db, nullptr), "rtg_ppm_bytes_device");
    std::vector<unsigned char> bytes(n * 3);
    float lightMax = 0.f;
    if (hipMemcpy(bytes.data(), db, n * 3, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&lightMax, dmax, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      check(RTG_ERR_HIP, "readback");
    for (void* d : {(void*)dPoses, (void*)dW, (void*)dCoef, dScratch, (void*)dPts, (void*)dIn,
                    (void*)dValid, (void*)dr, (void*)dh, (void*)dl, (void*)dmax, (void*)db})
      (void)hipFree(d);
    rtg_context_destroy(ctx);
    FILE* f = fopen(irrOut.c_str(), "wb");
    if (!f || fprintf(f, "P6\n%u %u\n255\n", W, H) < 0 ||
        fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) {
      fprintf(stderr, "Error: can't write %s\n", irrOut.c_str());
      exit(EXIT_FAILURE);
    }
    printf("Wrote %s (%ux%u, light of a %ux%ux%u grid of SH%u probes from %.9g,%.9g,%.9g by "
           "%.9g,%.9g,%.9g, %zu valid, %ux%u faces, flags %u, max %.8g)\n",
           irrOut.c_str(), W, H, grid.nx, grid.ny, grid.nz, K, (double)grid.origin.x,
           (double)grid.origin.y, (double)grid.origin.z, (double)grid.step.x, (double)grid.step.y,
           (double)grid.step.z, nValid, gridRes, gridRes, irrParams.flags, (double)lightMax);
  }

  if (gather) {  // pose -> primary rays -> hits -> gathered light -> bytes, all on the device
    const size_t n = (size_t)W * H;
    const unsigned K = gatherParams.samples;
    if (!posed) rtg_camera_identity(&camera);
    std::vector<rtg_vec> table(K);
    check(rtg_ao_directions(K, table.data()), "rtg_ao_directions");
    const std::vector<float> weights(K, 1.f / (float)K);
    rtg_context* ctx = nullptr;
    check(rtg_context_create((int)device, &ctx), "rtg_context_create");
    check(rtg_context_set_semantics(ctx, semantics), "rtg_context_set_semantics");
    check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
          "rtg_context_set_scene");
    rtg_ray* dr = nullptr;
    rtg_vec* dd = nullptr;
    float* dw = nullptr;
    rtg_vec* dl = nullptr;
    float* dmax = nullptr;
    unsigned char* db = nullptr;
    const size_t frames = gatherHistory.on ? gatherHistory.poses.size() + 1 : 1;  // as for --ao
    HistoryState st[2] = {};
    Mixed mixed = {};
    if (gatherScale.L) mixed = mixed_alloc(gatherScale, W, H, sizeof(rtg_vec));
    size_t holesSeen = 0;
    for (size_t k = 0; k < (frames > 1 ? 2u : 1u); ++k)
      if (hipMalloc(&st[k].hits, n * sizeof(rtg_hit)) != hipSuccess ||
          (gatherAccum && (hipMalloc(&st[k].acc, n * sizeof(rtg_vec)) != hipSuccess ||
                           hipMalloc(&st[k].len, n * sizeof(unsigned short)) != hipSuccess)) ||
          (gatherVariance.on && hipMalloc(&st[k].m2, n * sizeof(rtg_vec)) != hipSuccess))
        check(RTG_ERR_NOMEM, "hipMalloc");
    if (hipMalloc(&dr, n * sizeof(rtg_ray)) != hipSuccess ||
        hipMalloc(&dd, K * sizeof(rtg_vec)) != hipSuccess ||
        hipMalloc(&dw, K * sizeof(float)) != hipSuccess ||
        hipMalloc(&dl, n * sizeof(rtg_vec)) != hipSuccess ||
        hipMalloc(&dmax, sizeof(float)) != hipSuccess || hipMalloc(&db, n * 3) != hipSuccess)
      check(RTG_ERR_NOMEM, "hipMalloc");
    if (hipMemcpy(dd, table.data(), K * sizeof(rtg_vec), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dw, weights.data(), K * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      check(RTG_ERR_HIP, "upload");
    for (size_t k = 0; k < frames; ++k) {
      HistoryState& cur = st[k & 1];
      cur.pose = k + 1 < frames ? gatherHistory.poses[k] : camera;
      rtg_gather_params gp = gatherParams;
      gp.seed += (unsigned)k;
      check(rtg_camera_rays_device(ctx, &cur.pose, W, H, zoom, 1.f, dr, nullptr),
            "rtg_camera_rays_device");
      check(rtg_intersect_device(ctx, dr, n, cur.hits, nullptr), "rtg_intersect_device");
      if (gatherScale.L) {  // the gather on the low frame, then on the holes alone
        mixed_low_hits(ctx, mixed, cur.pose, zoom);
        check(rtg_gather_device(ctx, mixed.lowHits, (size_t)mixed.Wl * mixed.Hl, &gp, dd, dw, K,
                                (int)depth + 1, (rtg_vec*)mixed.lowSig, nullptr, nullptr),
              "rtg_gather_device");
        const size_t m = mixed_upsample(ctx, mixed, gatherScale, RTG_FILTER_RGB,
                                        gatherSkip ? RTG_UPSAMPLE_SKIP_NONFINITE : 0, W, H,
                                        cur.hits, (float*)dl);
        if (m) {
          check(rtg_gather_device(ctx, mixed.picked, m, &gp, dd, dw, K, (int)depth + 1,
                                  (rtg_vec*)mixed.pickedSig, nullptr, nullptr),
                "rtg_gather_device");
          check(rtg_values_place_device(ctx, RTG_FILTER_RGB, mixed.pickedSig, mixed.holes, m, n,
                                        (float*)dl, nullptr),
                "rtg_values_place_device");
        }
        holesSeen += m;
      } else {
        check(rtg_gather_device(ctx, cur.hits, n, &gp, dd, dw, K, (int)depth + 1, dl, nullptr,
                                nullptr),
              "rtg_gather_device");
      }
      if (gatherAccum)
        accumulate_frame(ctx, gatherHistory, W, H, zoom, dl, k ? &st[(k - 1) & 1] : nullptr, cur);
    }
    const HistoryState& last = st[(frames - 1) & 1];
    if (gatherAccum &&  // the accumulated frame takes the gathered one's place
        hipMemcpy(dl, last.acc, n * sizeof(rtg_vec), hipMemcpyDeviceToDevice) != hipSuccess)
      check(RTG_ERR_HIP, "copy");
    if (gatherFilter) {
      rtg_vec* smooth =
          (rtg_vec*)(gatherVariance.on
                         ? svgf_frame(ctx, last, W, H, gatherFilterParams, gatherVariance)
                         : filter_frame(ctx, last.hits, W, H, gatherFilterParams, dl));
      (void)hipFree(dl);
      dl = smooth;
    }
    check(rtg_max_colour_device(ctx, dl, n, dmax, nullptr), "rtg_max_colour_device");
    check(rtg_ppm_bytes_device(ctx, dl, n, dmax, db, nullptr), "rtg_ppm_bytes_device");
    std::vector<unsigned char> bytes(n * 3);
    float lightMax = 0.f;
    if (hipMemcpy(bytes.data(), db, n * 3, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&lightMax, dmax, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      check(RTG_ERR_HIP, "readback");
    (void)hipFree(dr);
    mixed_free(mixed);
    for (HistoryState& s : st) {
      (void)hipFree(s.hits);
      (void)hipFree(s.acc);
      (void)hipFree(s.len);
      (void)hipFree(s.m2);
    }
    (void)hipFree(dd);
    (void)hipFree(dw);
    (void)hipFree(dl);
    (void)hipFree(dmax);
    (void)hipFree(db);
    rtg_context_destroy(ctx);
    FILE* f = fopen(gatherOut.c_str(), "wb");
    if (!f || fprintf(f, "P6\n%u %u\n255\n", W, H) < 0 ||
        fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) {
      fprintf(stderr, "Error: can't write %s\n", gatherOut.c_str());
      exit(EXIT_FAILURE);
    }
    printf("Wrote %s (%ux%u, %u probes per primary hit, depth %u, max %.8g",
           gatherOut.c_str(), W, H, K, depth, (double)lightMax);
    if (gatherHistory.on) printf(", accumulated over %zu frames", frames);
    if (gatherScale.L)
      printf(", gathered at %ux%u and on %zu holes", W >> gatherScale.L, H >> gatherScale.L,
             holesSeen);
    printf(")\n");
  }

  if (!raysIn.empty()) {  // records as they lie in memory, like the G-buffer's
    std::vector<rtg_ray> rays;
    FILE* f = fopen(raysIn.c_str(), "rb");
    bool ok = f != nullptr;
    if (ok) {
      ok = fseek(f, 0, SEEK_END) == 0;
      const long bytes = ok ? ftell(f) : -1;
      ok = ok && bytes >= 0 && bytes % (long)sizeof(rtg_ray) == 0 && fseek(f, 0, SEEK_SET) == 0;
      if (ok) {
        rays.resize((size_t)bytes / sizeof(rtg_ray));
        ok = fread(rays.data(), sizeof(rtg_ray), rays.size(), f) == rays.size();
      }
      fclose(f);
    }
    if (!ok) {
      fprintf(stderr, "Error: can't read %s as %zu-byte ray records\n", raysIn.c_str(),
              sizeof(rtg_ray));
      exit(EXIT_FAILURE);
    }
    // --sort-rays: one context, the batch's order on the device, both outputs
    // through the indexed launches (results land at each ray's own place)
    std::vector<rtg_hit> sortedHits;
    std::vector<rtg_vec> sortedCols;
    const bool sorted = sortRays && !rays.empty();
    if (sorted) {
      const size_t n = rays.size();
      rtg_context* ctx = nullptr;
      check(rtg_context_create((int)device, &ctx), "rtg_context_create");
      check(rtg_context_set_semantics(ctx, semantics), "rtg_context_set_semantics");
      check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
            "rtg_context_set_scene");
      size_t scratchBytes = 0;
      check(rtg_ray_order_scratch(n, &scratchBytes), "rtg_ray_order_scratch");
      rtg_ray* dr = nullptr;
      unsigned* dOrder = nullptr;
      void* dScratch = nullptr;
      rtg_hit* dh = nullptr;
      rtg_vec* dc = nullptr;
      if (hipMalloc(&dr, n * sizeof(rtg_ray)) != hipSuccess ||
          hipMalloc(&dOrder, n * sizeof(unsigned)) != hipSuccess ||
          hipMalloc(&dScratch, scratchBytes) != hipSuccess ||
          hipMalloc(&dh, n * sizeof(rtg_hit)) != hipSuccess ||
          hipMalloc(&dc, n * sizeof(rtg_vec)) != hipSuccess)
        check(RTG_ERR_NOMEM, "hipMalloc");
      if (hipMemcpy(dr, rays.data(), n * sizeof(rtg_ray), hipMemcpyHostToDevice) != hipSuccess)
        check(RTG_ERR_HIP, "upload");
      check(rtg_ray_order_device(ctx, dr, n, RTG_ORDER_RAYS, dOrder, nullptr, dScratch,
                                 scratchBytes, nullptr),
            "rtg_ray_order_device");
      if (!hitsOut.empty()) {
        sortedHits.resize(n);
        check(rtg_intersect_indexed_device(ctx, dr, dOrder, n, dh, nullptr),
              "rtg_intersect_indexed_device");
        if (hipMemcpy(sortedHits.data(), dh, n * sizeof(rtg_hit), hipMemcpyDeviceToHost) !=
            hipSuccess)
          check(RTG_ERR_HIP, "readback");
      }
      if (!radianceOut.empty()) {
        sortedCols.resize(n);
        check(rtg_raytrace_indexed_device(ctx, dr, dOrder, n, (int)depth + 1, dc, nullptr),
              "rtg_raytrace_indexed_device");
        if (hipMemcpy(sortedCols.data(), dc, n * sizeof(rtg_vec), hipMemcpyDeviceToHost) !=
            hipSuccess)
          check(RTG_ERR_HIP, "readback");
      }
      (void)hipFree(dr);
      (void)hipFree(dOrder);
      (void)hipFree(dScratch);
      (void)hipFree(dh);
      (void)hipFree(dc);
      rtg_context_destroy(ctx);
      printf("Ordered %zu rays on the device (--sort-rays)\n", n);
    }
    if (!hitsOut.empty()) {
      std::vector<rtg_hit> hits(rays.size());
      if (sorted) hits.swap(sortedHits);
      else if (!rays.empty())
        check(rtg_intersect((int)device, spheres.data(), nSph, rays.data(), rays.size(),
                            hits.data()),
              "rtg_intersect");
      f = fopen(hitsOut.c_str(), "wb");
      if (!f || fwrite(hits.data(), sizeof(rtg_hit), hits.size(), f) != hits.size() ||
          fclose(f) != 0) {
        fprintf(stderr, "Error: can't write %s\n", hitsOut.c_str());
        exit(EXIT_FAILURE);
      }
      printf("Wrote %s (%zu hit records of %zu bytes)\n", hitsOut.c_str(), hits.size(),
             sizeof(rtg_hit));
    }
    if (!radianceOut.empty()) {
      std::vector<rtg_vec> cols(rays.size());
      if (sorted) {
        cols.swap(sortedCols);
      } else if (!rays.empty() && semantics == RTG_SEMANTICS_CPU) {
        check(rtg_raytrace((int)device, spheres.data(), nSph, lights.data(), nLgt, rays.data(),
                           rays.size(), (int)depth + 1, cols.data()),
              "rtg_raytrace");
      } else if (!rays.empty()) {  // semantics is per context, as for the render above
        rtg_context* ctx = nullptr;
        check(rtg_context_create((int)device, &ctx), "rtg_context_create");
        check(rtg_context_set_semantics(ctx, semantics), "rtg_context_set_semantics");
        check(rtg_context_set_scene(ctx, spheres.data(), nSph, lights.data(), nLgt),
              "rtg_context_set_scene");
        rtg_ray* dr = nullptr;
        rtg_vec* dc = nullptr;
        if (hipMalloc(&dr, rays.size() * sizeof(rtg_ray)) != hipSuccess ||
            hipMalloc(&dc, cols.size() * sizeof(rtg_vec)) != hipSuccess)
          check(RTG_ERR_NOMEM, "hipMalloc");
        if (hipMemcpy(dr, rays.data(), rays.size() * sizeof(rtg_ray), hipMemcpyHostToDevice) !=
            hipSuccess)
          check(RTG_ERR_HIP, "upload");
        check(rtg_raytrace_device(ctx, dr, rays.size(), (int)depth + 1, dc, nullptr),
              "rtg_raytrace_device");
        if (hipMemcpy(cols.data(), dc, cols.size() * sizeof(rtg_vec), hipMemcpyDeviceToHost) !=
            hipSuccess)
          check(RTG_ERR_HIP, "readback");
        (void)hipFree(dr);
        (void)hipFree(dc);
        rtg_context_destroy(ctx);
      }
      f = fopen(radianceOut.c_str(), "wb");
      if (!f || fwrite(cols.data(), sizeof(rtg_vec), cols.size(), f) != cols.size() ||
          fclose(f) != 0) {
        fprintf(stderr, "Error: can't write %s\n", radianceOut.c_str());
        exit(EXIT_FAILURE);
      }
      printf("Wrote %s (%zu colours of %zu bytes)\n", radianceOut.c_str(), cols.size(),
             sizeof(rtg_vec));
    }
  }
  return 0;
}
