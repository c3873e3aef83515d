/*
 * rtg.h — C ABI of the MI355X-native raytracer-gamma hot path (librtg.so).
 *
 * This header is the drop-in boundary that replaces the reference's OpenCL
 * enqueue of the per-pixel kernel:
 *
 *   reference (snowzurfer/raytracer-gamma)            replaced by
 *   ------------------------------------------------  ------------------------------
 *   clCreateBuffer/clEnqueueWriteBuffer scene          rtg_render (one-shot) or
 *     main.cpp:277-294                                 rtg_context_set_scene
 *   clSetKernelArg x11, clEnqueueNDRangeKernel,        rtg_render / rtg_render_device /
 *     clFinish  main.cpp:339-363                       rtg_render_rows[_device]
 *     (kernel raytrace_kernel.cl:870-881)
 *   clEnqueueReadBuffer  main.cpp:460                  rtg_render (dstHost) or the
 *                                                      caller's copy of dstDevice
 *   maxColourValuePixelBuffer  algebra.h:68-91         rtg_max_colour (host) /
 *                                                      rtg_max_colour_device
 *   savePPM  main.cpp:43-91                            rtg_save_ppm / rtg_ppm_bytes
 *   rayTrace(...)  raytracer.h:410-636 (CPU entry)     (inside the HIP kernel)
 *   (8-GPU node, SURVEY.md §8e: none in the reference) rtg_render_multi (RCCL gather)
 *   (primary visibility per pixel: none in the reference) rtg_gbuffer / rtg_gbuffer_device /
 *                                                      rtg_gbuffer_host
 *   calcIntersection / hasClearLineOfSight for a       rtg_intersect[_device|_host] /
 *     caller's own rays  raytracer.h:145-194, 272-309  rtg_visible[_device|_host]
 *   rayTrace for a caller's own rays                   rtg_raytrace[_device|_host]
 *     raytracer.h:410-636
 *   the camera of main.cpp:384-436, moved to a pose   rtg_camera_look_at, rtg_camera_rays[_device|_host],
 *     (fixed at 0 looking down -z in the reference)    rtg_render_camera[_device|_host]
 *   (many poses, one frame each: probes, cube maps)    rtg_render_views[_device|_host], rtg_camera_cube
 *   (groups of views folded by a weight table: SH       rtg_views_fold[_device|_host],
 *     probes, ambient cubes)                              rtg_render_views_fold[_device|_host],
 *                                                         rtg_cube_sh_weights
 *   (hemisphere visibility of a hit point: the caller's  rtg_ao[_device|_host],
 *     loop over hasClearLineOfSight in the reference)    rtg_ao_segments[_device|_host]
 *   calculateMatte for a caller's own hit points       rtg_matte[_device|_host]
 *     raytracer.h:313-367
 *   (the light of a grid of baked SH probes at a hit    rtg_irradiance[_device|_host],
 *     point: the consumer of the folded views)            rtg_probe_grid_points, rtg_probe_grid_poses
 *   (one-bounce indirect light of a hit point: the      rtg_gather[_device|_host],
 *     caller's loop over rayTrace in the reference)       rtg_gather_rays[_device|_host]
 *   (a frame of those per-pixel signals smoothed along   rtg_filter[_device|_host],
 *     its surfaces, guided by the frame's hit records)    rtg_filter_scratch
 *   (such a signal carried from frame to frame while     rtg_accumulate[_device|_host],
 *     the camera moves: reprojection by the hit points)   rtg_camera_project[_device|_host]
 *   (a variance per pixel from the carried moments, and  rtg_variance[_device|_host],
 *     the filter guided by it: edges inside a surface)    rtg_svgf[_device|_host], rtg_svgf_scratch
 *   (such a signal traced on a coarser frame, brought up  rtg_upsample[_device|_host], rtg_upsample_scratch,
 *     by the full frame's records; the pixels it cannot    rtg_hits_pick[_device|_host],
 *     reach listed, traced alone and placed)               rtg_values_place[_device|_host]
 *   primaryContainer for a caller's own points         rtg_contains[_device|_host]
 *     raytracer.h:245-270
 *   checkError -> exit(EXIT_FAILURE)  err_code.h:143   negative return + rtg_last_error
 *   output_device_info  device_info.cpp:30             rtg_device_info
 *   parseArguments --list/--device  device_picker.h:70 rtg_device_count / device index args
 *
 * Scene records are byte-identical to the reference structs (static_asserts in
 * the implementation): a `struct Sphere*` / `struct Light*` / `Vec*` from the
 * reference host can be passed by a plain pointer cast.
 *
 * Semantics: the output is the framebuffer the reference CPU path
 * (raytracer.h, main.cpp:404-453) produces, bit for bit (NaNs are written as
 * the x86 default NaN 0xFFC00000 that path produces).  `stackSize` is the
 * reference's RTSTACK_MAXSIZE (raytraceStack.h:10; 6 as shipped) = depth + 1.
 *
 * All calls are blocking unless they take a `stream`; no call exits the
 * process.  Not re-entrant per context.
 */
#ifndef RTG_H
#define RTG_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTG_ABI_VERSION 1
#define RTG_MAX_STACK 16 /* largest supported RTSTACK_MAXSIZE */
/* Scenes hold fewer than RTG_MAX_SPHERES spheres (rtg_context_set_scene
 * rejects larger ones with RTG_ERR_INVALID): the kernel keeps material
 * indices in 22-bit fields and 32-bit table offsets. */
#define RTG_MAX_SPHERES (1u << 22)

/* vec.h:27-29 */
typedef struct rtg_vec { float x, y, z; } rtg_vec;
/* material.h:8-14 */
typedef struct rtg_material {
  rtg_vec matteColour;
  rtg_vec glossColour;
  float opacity;
  float refractiveIndex;
} rtg_material;
/* sphere.h:9-14 */
typedef struct rtg_sphere {
  rtg_vec pos;
  float radius;
  rtg_material material;
} rtg_sphere;
/* raytracer.h:20-25 */
typedef struct rtg_light { rtg_vec pos; rtg_vec col; } rtg_light;

/* Error codes (err_code.h:143-155 printed-and-exited; here they are returned). */
#define RTG_OK 0
#define RTG_ERR_INVALID (-1)   /* bad argument */
#define RTG_ERR_HIP (-2)       /* HIP runtime error; see rtg_last_error() */
#define RTG_ERR_NOMEM (-3)
#define RTG_ERR_NODEVICE (-4)
#define RTG_ERR_IO (-5)

/* Thread-local message for the last failing call ("" if none). */
const char* rtg_last_error(void);
int rtg_abi_version(void);

/* ---- device selection (device_picker.h:70-119, device_info.cpp:30-125) ---- */
int rtg_device_count(int* count);
/* Writes a one-line description ("name, CUs, clock, memory") into buf. */
int rtg_device_info(int device, char* buf, size_t buflen);

/* ---- one-shot drop-in for main.cpp:277-468 ----
 * Uploads the scene, renders the whole W x H frame on `device`, downloads
 * W*H rtg_vec into dstHost.  aliasFactor: the reference's kAliasFactor (3.f =
 * 3x3 supersampling); zoom: kZoom (-4.f). */
int rtg_render(int device, const rtg_sphere* spheres, unsigned sphNum,
               const rtg_light* lights, unsigned lgtNum, unsigned width,
               unsigned height, float zoom, float aliasFactor, int stackSize,
               rtg_vec* dstHost);

/* ---- multi-GPU one-shot: one process, nDevices GPUs ----
 * `devices` lists distinct device ids; devices[0] is the root.  Rows are dealt
 * row-cyclically in blocks of rowBlock (16 is a good default); every device
 * renders its shard on its own stream, ONE grouped RCCL gather (ncclGather)
 * brings the shards to the root over xGMI, the root restores row order
 * (rtg_assemble_shards_device) and W*H rtg_vec are copied to dstHost.
 * Bit-identical to rtg_render.  timingsMs (optional, 3 floats): slowest
 * device's render, gather + assemble on the root, wall time of the call. */
int rtg_render_multi(const int* devices, int nDevices, const rtg_sphere* spheres,
                     unsigned sphNum, const rtg_light* lights, unsigned lgtNum,
                     unsigned width, unsigned height, float zoom, float aliasFactor,
                     int stackSize, unsigned rowBlock, rtg_vec* dstHost, float* timingsMs);
/* The same with a persistent multi-device handle: the RCCL communicator
 * (ncclCommInitAll, ~0.5 s), the per-device contexts, streams and buffers
 * are kept across frames.  Not re-entrant per handle. */
typedef struct rtg_multi rtg_multi;
int rtg_multi_create(const int* devices, int nDevices, rtg_multi** out);
int rtg_multi_set_scene(rtg_multi* mg, const rtg_sphere* spheres, unsigned sphNum,
                        const rtg_light* lights, unsigned lgtNum);
int rtg_multi_render(rtg_multi* mg, unsigned width, unsigned height, float zoom,
                     float aliasFactor, int stackSize, unsigned rowBlock, rtg_vec* dstHost,
                     float* timingsMs);
int rtg_multi_destroy(rtg_multi* mg);
/* How rtg_multi_render brings the shards to the root:
 * RTG_GATHER_RCCL (default): one grouped ncclGather of the padded shards, then
 * the assemble kernel; RTG_GATHER_PEER_COPY (ablation): no collective, no
 * assemble — every device writes its shard's row blocks straight into the
 * root's frame with one strided peer copy (rtg_place_shard_device); needs
 * peer access to the root (enabled here, or RTG_ERR_HIP). */
#define RTG_GATHER_RCCL 0
#define RTG_GATHER_PEER_COPY 1
int rtg_multi_set_gather(rtg_multi* mg, int mode);

/* ---- persistent context: scene resident in HBM, caller-owned streams ----
 * A context may render on several streams; it orders its own scratch between
 * them with events (a launch on a stream other than the one its scratch slot
 * last ran on waits for that launch; hipStreamPerThread always waits).  A
 * stream handle that is destroyed and recreated while renders of the context
 * are still pending on it may come back with the same value: synchronise
 * such a stream (or the device) before destroying it. */
typedef struct rtg_context rtg_context;
int rtg_context_create(int device, rtg_context** out);
/* Waits for the context's pending work on every stream before it frees
 * anything: a caller may destroy a context right behind its launches. */
int rtg_context_destroy(rtg_context* ctx);
/* Copies the scene into device memory (kept until the next call / destroy).
 * Waits for the context's pending work on every stream before it frees the
 * old scene: launches already enqueued finish on the scene they were given. */
int rtg_context_set_scene(rtg_context* ctx, const rtg_sphere* spheres, unsigned sphNum,
                          const rtg_light* lights, unsigned lgtNum);

/* Cost of the last rtg_context_set_scene (end-to-end reporting, SURVEY.md
 * §8d): out4 = {host preparation ms (packed records, shadow / overlap / cone
 * masks, BVH build), upload ms (device allocation + H2D copies), device bytes
 * of the scene, BVH nodes}.  Zeros before the first scene. */
int rtg_context_scene_stats(rtg_context* ctx, double* out4);

/* Row sharding.  Rows are grouped in blocks of `rowBlock` rows; block b belongs
 * to shard (b % nShards) (row-cyclic).  A shard's rows are
 * packed in increasing row order.  nShards == 1 gives the whole frame in
 * row-major order.  Returns the number of rows of `shard` in *rows. */
int rtg_shard_rows(unsigned height, unsigned rowBlock, unsigned shard, unsigned nShards,
                   unsigned* rows);
/* Global row index of local row `localRow` of `shard`. */
unsigned rtg_shard_global_row(unsigned localRow, unsigned rowBlock, unsigned shard,
                              unsigned nShards);

/* Asynchronous render of shard `shard` of a W x H frame into device memory
 * dstDevice (rtg_shard_rows(...) * W rtg_vec) on `stream` (a hipStream_t, or
 * NULL for the null stream).  The camera uses global row indices, so the
 * shard's pixels are bit-identical to the same pixels of a 1-shard render.
 * Exercised, with rtg_render_rows_device, up to a frame of 32771 x 21845 (8.59
 * GB, past byte offset 2^32 and float index 2^31), whole and in 3 shards (tests/test_gpu_large.py). */
int rtg_render_device(rtg_context* ctx, unsigned width, unsigned height, float zoom,
                      float aliasFactor, int stackSize, unsigned rowBlock, unsigned shard,
                      unsigned nShards, rtg_vec* dstDevice, void* stream);

/* Restore row order after a gather of row-cyclic shards:
 * `gathered` holds nShards shard buffers of paddedRows x width rtg_vec each
 * (shard g's rows as rtg_render_device(..., rowBlock, g, nShards) packs them,
 * padded to paddedRows = ceil(ceil(H / rowBlock) / nShards) * rowBlock);
 * writes the height x width frame to `frame` on `stream`.  Device memory. */
int rtg_assemble_shards_device(rtg_context* ctx, const rtg_vec* gathered, unsigned nShards,
                               unsigned paddedRows, unsigned width, unsigned height,
                               unsigned rowBlock, rtg_vec* frame, void* stream);

/* The inverse placement without a gather buffer: copy shard `shardIdx`'s
 * packed rows (as rtg_render_device packs them) into their rows of the
 * height x width `frame` with one strided copy (hipMemcpy2DAsync; `frame` may
 * be another device's memory with peer access) plus one copy for a ragged
 * last block, on `stream`. */
int rtg_place_shard_device(rtg_context* ctx, const rtg_vec* shard, unsigned shardIdx,
                           unsigned nShards, unsigned width, unsigned height, unsigned rowBlock,
                           rtg_vec* frame, void* stream);

/* Render an explicit list of global rows (each < height) into dstDevice
 * (nRows * width rtg_vec, in list order); rowsDevice is device memory. */
int rtg_render_rows_device(rtg_context* ctx, unsigned width, unsigned height, float zoom,
                           float aliasFactor, int stackSize, const unsigned* rowsDevice,
                           unsigned nRows, rtg_vec* dstDevice, void* stream);
/* One-shot host version of the above (rows and dstHost in host memory). */
int rtg_render_rows(int device, const rtg_sphere* spheres, unsigned sphNum,
                    const rtg_light* lights, unsigned lgtNum, unsigned width, unsigned height,
                    float zoom, float aliasFactor, int stackSize, const unsigned* rows,
                    unsigned nRows, rtg_vec* dstHost);

/* ---- primary-hit G-buffer: id, depth, normal and coverage per pixel ----
 * What the primary rays of a pixel see, before any shading (picking, object
 * masks and alpha, denoiser guides, edge detection, "why is this pixel
 * black?").  Per sample (i, j) of the pixel, in the reference's loop order
 * (main.cpp:411-452), the ray starts at o = (0,0,0) with the direction the
 * render uses, and its hit is calcIntersection's (raytracer.h:145-194) in the
 * same float operations: the raySphere root test with the 1e-5 / 10000
 * window, minT starting at 1000, strict <, the first index winning ties.
 * The pixel's winning sample is the one with the smallest t among those that
 * hit, the lowest sample index on a tie.
 *   hits * (id + 1) != idSum marks a mixed pixel: its samples hit more than
 *   one sphere (an edge between spheres); 0 < hits < nAA*nAA is a silhouette
 *   against the background (hits / nAA^2 is its coverage).  hits == 0 is a
 *   pixel the render leaves +0 in every channel.
 * NaN or degenerate inputs follow the comparisons as written (a comparison
 * with NaN is false: a miss); a NaN normal component is written as
 * 0xFFC00000, like the frame's NaNs.  The G-buffer does not depend on
 * stackSize, lights or rtg_context_set_semantics. */
typedef struct rtg_gbuf_px { /* 32 bytes */
  int id;          /* sphere index of the winning sample's closest hit; -1: no sample hit */
  float t;         /* that hit's t (calcIntersection's minT); 1000.f when id == -1 */
  unsigned hits;   /* samples of the pixel whose primary ray hit a sphere, 0..nAA*nAA */
  unsigned sample; /* winning sample's index i*nAA + j (reference loop order); 0 when none */
  rtg_vec normal;  /* vnorm(P - c) at the winning hit, P = o + t*d; (0,0,0) when none */
  unsigned idSum;  /* sum over the pixel's samples of (id_sample + 1), mod 2^32; a miss adds 0 */
} rtg_gbuf_px;
/* Asynchronous G-buffer of shard `shard` of a W x H frame of the context's
 * scene into device memory dstDevice (rtg_shard_rows(...) * W records, 16-byte
 * aligned) on `stream`; shard rows packed as rtg_render_device packs them.
 * Uses none of the context's render scratch: it may be mixed freely with
 * rtg_render_device calls on the same context.  Exercised up to 32771 x 4097
 * records (4.30 GB), whole and in 3 shards (tests/test_gpu_large.py). */
int rtg_gbuffer_device(rtg_context* ctx, unsigned width, unsigned height, float zoom,
                       float aliasFactor, unsigned rowBlock, unsigned shard, unsigned nShards,
                       rtg_gbuf_px* dstDevice, void* stream);
/* One-shot: uploads the scene, runs on `device`, downloads W*H records. */
int rtg_gbuffer(int device, const rtg_sphere* spheres, unsigned sphNum, unsigned width,
                unsigned height, float zoom, float aliasFactor, rtg_gbuf_px* dstHost);
/* The same records computed on the host with plain loops over every pixel,
 * sample and sphere (no GPU call; the device kernel's yardstick, and usable
 * on a machine without a GPU).  nthreads <= 0: 1. */
int rtg_gbuffer_host(const rtg_sphere* spheres, unsigned sphNum, unsigned width,
                     unsigned height, float zoom, float aliasFactor, rtg_gbuf_px* dstHost,
                     int nthreads);

/* ---- batch ray queries: closest hit and line of sight for arbitrary rays ----
 * The two scene queries of the reference, calcIntersection (raytracer.h:
 * 145-194) and hasClearLineOfSight (raytracer.h:272-309), for a buffer of the
 * caller's own rays against the resident scene: picking from another camera,
 * ambient occlusion, light baking, collision and visibility tests, or one
 * secondary ray of a bad pixel.  A buffer of rays goes in, a buffer of
 * results comes out, bit for bit what the reference's functions return.
 *
 * rtg_intersect: ray k gets calcIntersection(spheres, n, &ray) in the same
 * float operations: the raySphere root test with the 1e-5 / 10000 window,
 * minT starting at 1000, strict <, the first index winning ties.  `dir` is
 * used as given: it is not normalised, and any length is legal.  `point` and
 * `normal` are computed for the final winner only (the reference recomputes
 * them at each improvement, so its last values are these).
 *
 * rtg_visible: out[k] = hasClearLineOfSight(a, b) ? 1 : 0, with dir =
 * vnorm(b - a), gap = dot(b - a, b - a) taken before normalising, blocked iff
 * the closest hit's |t dir|^2 < gap.
 *
 * NaN, infinite and degenerate inputs (a zero dir, a == b, NaN or infinite
 * components) follow the comparisons as written: a comparison with NaN is
 * false, so no hit and visible.  NaN words of point and normal are written
 * as 0xFFC00000, as the frame and the G-buffer do.
 *
 * The results do not depend on lights, stackSize or
 * rtg_context_set_semantics.  Rays are independent; the order of a batch
 * affects speed only: the 64 rays of a wave walk the scene's BVH together,
 * so coherent neighbours (a pixel grid, a sorted batch) are faster than a
 * shuffled one.  Origins may lie anywhere: far outside the scene the BVH's
 * boxes are widened per ray (by 2^-8 of the distance to the scene), so very
 * distant origins are exact but slower.
 *
 * The device calls are asynchronous on `stream`, use none of the context's
 * render scratch and may be mixed freely with rtg_render_device and
 * rtg_gbuffer_device on one context.  n == 0 is RTG_OK with no launch.
 * RTG_ERR_INVALID with a message, before any GPU call, for a null buffer,
 * hits not 16-byte aligned, a context without a scene, or a batch of more
 * than 2^31-1 workgroups (64 rays each).  Exercised up to n = 357 924 864 (8.6
 * GB of rays, 11.5 GB of hits), the _indexed forms too (tests/test_gpu_large.py). */
typedef struct rtg_ray     { rtg_vec origin, dir; } rtg_ray;      /* 24 B */
typedef struct rtg_segment { rtg_vec a, b; }        rtg_segment;  /* 24 B */
typedef struct rtg_hit {                                           /* 32 B */
  int id;          /* calcIntersection's sphere index; -1: no hit */
  float t;         /* its minT; 1000.f when id == -1 */
  rtg_vec point;   /* origin + t*dir, as raytracer.h:172-173; (0,0,0) when none */
  rtg_vec normal;  /* vnorm(point - c), :176-177; (0,0,0) when none */
} rtg_hit;

int rtg_intersect_device(rtg_context* ctx, const rtg_ray* raysDevice, size_t n,
                         rtg_hit* hitsDevice /* 16-byte aligned */, void* stream);
/* One-shot: uploads the scene and the rays, runs on `device`, downloads n hits. */
int rtg_intersect(int device, const rtg_sphere* spheres, unsigned sphNum,
                  const rtg_ray* rays, size_t n, rtg_hit* hitsHost);
/* The same on the host, no GPU call.  walk 0: plain loops over every ray and
 * sphere (the yardstick).  walk 1: the device kernel's own query path compiled
 * for the host, one ray per "wave": the scene tables built as
 * rtg_context_set_scene builds them, then the branch the kernel takes (the
 * BVH with the outside-origin treatment, the 64-sphere two-pass query, or
 * the flat loop), so the culls can be checked without a GPU.  Any other walk
 * is RTG_ERR_INVALID.  nthreads <= 0: 1. */
int rtg_intersect_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_ray* rays,
                       size_t n, rtg_hit* hitsHost, int walk, int nthreads);

int rtg_visible_device(rtg_context* ctx, const rtg_segment* segsDevice, size_t n,
                       unsigned char* outDevice, void* stream);
int rtg_visible(int device, const rtg_sphere* spheres, unsigned sphNum,
                const rtg_segment* segs, size_t n, unsigned char* outHost);
int rtg_visible_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_segment* segs,
                     size_t n, unsigned char* outHost, int walk, int nthreads);

/* ---- batch ray tracing: rayTrace's colour for arbitrary rays ----
 * The third scene function of the reference, rayTrace itself (raytracer.h:
 * 410-636), for a buffer of the caller's own rays: a frame from a moved
 * camera, a reflection probe, a cube map, or the colour along one suspicious
 * ray.  A buffer of rays goes in, a buffer of colours comes out:
 *
 *   dst[k] = rayTrace(spheres, n, lights, m, ray, bgMaterial, 0) with
 *   ray = {rays[k].origin, rays[k].dir, intensity (1,1,1)} and the background
 *   material of main.cpp:423-426 (the one every render uses), for stack
 *   capacity stackSize (RTSTACK_MAXSIZE), bit for bit.
 *
 * `dir` is used as given: it is not normalised, and any length is legal.
 * The value is rayTrace's return before main.cpp:442-445 scales and sums it:
 * NaN words are written as 0xFFC00000, as the frame's, and a -0 stays -0.
 * To rebuild a pixel from its nS sample rays, fold them as the reference
 * does, in float and in sample order:
 *   pix = 0; for each sample s in order: pix += col[s] * (1 / nS);
 * (1 / nS is the float quotient 1.f / (aliasFactor * aliasFactor)); with the
 * sample directions of main.cpp:411-436 that is the render's pixel, bit for
 * bit.  NaN, infinite and degenerate rays follow the comparisons as written,
 * as in rtg_intersect.
 *
 * The device call follows rtg_context_set_semantics (CPU or OpenCL), as the
 * renders do; the host call takes the mode as an argument.
 * rtg_set_launch_opts does not apply.  The device call is asynchronous on
 * `stream`, takes none of the context's render scratch (group lists, cost
 * tables, slots) and may be mixed freely with rtg_render_device,
 * rtg_gbuffer_device and the ray queries on one context; its frames live in
 * LDS and private memory as in the render kernels.  Rays are independent; the
 * order of a batch affects speed only (the 64 rays of a wave walk the scene
 * together).  The call is exact for origins anywhere, at every level of a
 * ray's tree, because it uses none of the tables the renders keep for their
 * own camera; a render of the same rays is therefore faster (README).
 *
 * n == 0 is RTG_OK with no launch.  RTG_ERR_INVALID with a message, before
 * any GPU call, for a null buffer, a context without a scene, stackSize
 * outside 1..RTG_MAX_STACK, an unknown walk or semantics, or a batch of more
 * than 2^31-1 workgroups (64 rays each).  Exercised up to n = 357 924 864 (4.3
 * GB of colours), the _indexed form too (tests/test_gpu_large.py).
 *
 * Out of scope: a per-ray intensity, a caller-chosen refractive material for
 * the ray's medium, and multi-GPU batches.  (Ordering a batch for coherence:
 * the ray order, below.  A frame's rays and its fold: the posed camera.) */
int rtg_raytrace_device(rtg_context* ctx, const rtg_ray* raysDevice, size_t n,
                        int stackSize, rtg_vec* dstDevice, void* stream);
/* One-shot: uploads the scene and the rays, runs on `device`, downloads n colours. */
int rtg_raytrace(int device, const rtg_sphere* spheres, unsigned sphNum,
                 const rtg_light* lights, unsigned lgtNum, const rtg_ray* rays,
                 size_t n, int stackSize, rtg_vec* dstHost);
/* The same on the host, no GPU call.  walk 0: plain loops over every sphere
 * for every query of every ray's tree (the yardstick).  walk 1: the device
 * kernel's own path compiled for the host, one ray per "wave", over the scene
 * tables built as rtg_context_set_scene builds them (as rtg_intersect_host).
 * semantics: RTG_SEMANTICS_CPU or RTG_SEMANTICS_OPENCL.  nthreads <= 0: 1. */
int rtg_raytrace_host(const rtg_sphere* spheres, unsigned sphNum,
                      const rtg_light* lights, unsigned lgtNum, const rtg_ray* rays,
                      size_t n, int stackSize, int semantics, rtg_vec* dstHost,
                      int walk, int nthreads);

/* ---- ray order: coherence ordering of a batch, and indexed launches ----
 * The 64 rays of a wave walk the scene together, so a batch in no particular
 * order (ambient occlusion, light baking, probes, secondary rays) costs several
 * times what the same rays cost in a coherent order (README).  Rays are
 * independent, so launching them in another order changes no output bit.
 * rtg_ray_order* computes such an order; the _indexed launches take it (or
 * any other index list) and still write every result at its ray's own place.
 *
 * THE KEY of ray (origin o, direction d), 50 used bits of 64, bit 0 lowest:
 *   bits 49..20  the origin's cell, 10 bits per axis, Morton-interleaved: bit
 *                i of the x, y, z cell index at bit 20 + 3 i, + 3 i + 1, + 3 i + 2
 *   bits 19..0   the direction's octahedral bin, 10 bits per axis, Morton-
 *                interleaved: bit i of u, v at bit 2 i, 2 i + 1
 * all in float arithmetic without contraction (the same bits on host and
 * device):
 *   key box   per axis lo = min(c - |r|), hi = max(c + |r|) over the scene's
 *             spheres (a sphere with a non-finite centre component or radius
 *             is skipped; no sphere left: [-1, 1]^3), computed when the scene
 *             is set; scale = 1024 / (hi - lo), or 0 when hi <= lo or either
 *             the width or the quotient is not finite.
 *   cell      per axis (int)clamp((o - lo) * scale, 0, 1023), the clamp done
 *             in float with NaN going to 0 (so a NaN or -inf coordinate is in
 *             cell 0, +inf in cell 1023; origins outside the box clamp to its
 *             faces).
 *   bin       s = (|dx| + |dy|) + |dz|; s zero, NaN or infinite: (0, 0).
 *             Otherwise p = (dx / s, dy / s), and for dz < 0 the fold p =
 *             ((1 - |py|) sign(dx), (1 - |px|) sign(dy)) (sign(0) = +1);
 *             u = (int)clamp((px + 1) * 512, 0, 1023), v likewise of py.
 * A segment (a, b) of rtg_visible has the key of the ray (a, b - a), the
 * difference taken in float.
 *
 * order[k] is the index of the ray at position k of the batch sorted by key;
 * the sort is stable (equal keys keep index order), so the device and the host
 * form give the same words.  keys, when not NULL, receives key(ray i) at
 * keys[i], in batch order.
 *
 * rtg_ray_order_device: asynchronous on `stream`; allocates nothing, takes
 * none of the context's render scratch, may be mixed with every other call on
 * the context; needs the context's scene (the key box).  scratchDevice: at
 * least rtg_ray_order_scratch(n) bytes of device memory, 16-byte aligned,
 * owned by the call until it has finished on the stream.  The sort is a radix
 * sort by 8-bit digits in tiles of RTG_ORDER_TILE_RAYS rays, with a scan over
 * RTG_ORDER_SCAN_TILES tiles a step; a digit position on which every key
 * agrees costs nothing.  The keys are made by at most RTG_ORDER_KEY_GRID
 * workgroups: a batch of more tiles gives each several, tile-strided.  n == 0
 * is RTG_OK with no launch.  RTG_ERR_INVALID
 * with a message, before any GPU call, for a null ray, order or scratch
 * buffer, an unknown kind, n > 2^32 - 1, a scratch that is too small or not
 * 16-byte aligned, or a context without a scene.  Exercised up to n =
 * 178 957 056 rays (4.29 GB) (tests/test_gpu_large.py).
 *
 * The _indexed launches: lane k of the launch takes ray order[k] and writes
 * its result at order[k], so the outputs are in the caller's order and, for
 * any permutation, bit for bit those of the un-indexed call.  `order` is any
 * list of n indices; an entry >= n is skipped and never dereferenced, a
 * repeated entry writes the same record twice, a record no entry names is not
 * written.  Arguments are checked as in the un-indexed calls; a null order is
 * RTG_ERR_INVALID.
 *
 * Out of scope: reordering inside the un-indexed calls, re-sorting secondary
 * rays between bounces, multi-GPU batches. */
#define RTG_ORDER_RAYS 0      /* the batch holds rtg_ray records */
#define RTG_ORDER_SEGMENTS 1  /* the batch holds rtg_segment records */
#define RTG_ORDER_TILE_RAYS 1024
#define RTG_ORDER_SCAN_TILES 256
#define RTG_ORDER_KEY_GRID 2048
int rtg_ray_order_scratch(size_t n, size_t* bytes);
int rtg_ray_order_device(rtg_context* ctx, const void* raysDevice, size_t n, int kind,
                         unsigned* orderDevice, unsigned long long* keysDevice /* may be NULL */,
                         void* scratchDevice, size_t scratchBytes, void* stream);
/* The same on the host, no GPU call: the same key function and
 * std::stable_sort.  nthreads <= 0: 1 (the keys; the result does not depend
 * on it). */
int rtg_ray_order_host(const rtg_sphere* spheres, unsigned sphNum, const void* rays, size_t n,
                       int kind, unsigned* orderHost, unsigned long long* keysHost /* may be NULL */,
                       int nthreads);
int rtg_intersect_indexed_device(rtg_context* ctx, const rtg_ray* raysDevice,
                                 const unsigned* orderDevice, size_t n, rtg_hit* hitsDevice,
                                 void* stream);
int rtg_visible_indexed_device(rtg_context* ctx, const rtg_segment* segsDevice,
                               const unsigned* orderDevice, size_t n, unsigned char* outDevice,
                               void* stream);
int rtg_raytrace_indexed_device(rtg_context* ctx, const rtg_ray* raysDevice,
                                const unsigned* orderDevice, size_t n, int stackSize,
                                rtg_vec* dstDevice, void* stream);

/* ---- posed camera: rays and frames from any viewpoint ----
 * The reference keeps its camera at the origin looking down -z (main.cpp:
 * 384-436), and so do rtg_render* and rtg_gbuffer*.  A pose moves it.  The
 * camera vector of sample (i, j) of pixel (x, y) is (rx, ry, zoom) with rx,
 * ry exactly those of main.cpp:411-436; the posed ray is, per component q in
 * float with no contraction and in this operand order,
 *
 *   v.q    = (rx * right.q + ry * up.q) + zoom * back.q
 *   dir    = vnorm(v)            (vec.h:41: l = 1/sqrt(dot), l * v)
 *   origin = eye
 *
 * The basis is used as given: it is not normalised or orthogonalised, so a
 * scaled, sheared or mirrored basis is legal.  NaN, infinite or zero
 * components follow the arithmetic and the comparisons as written, as in
 * rtg_intersect.  The identity pose (eye 0, right (1,0,0), up (0,1,0), back
 * (0,0,1)) gives, for a nonzero zoom, the render's ray bit for bit.
 *
 * The frame of a pose is, per pixel,
 *   pix = 0; for each sample s in the reference's order (i outer, j inner):
 *       pix += (1/nS) * rayTrace(ray_s)
 * in main.cpp:442-445's operations, rayTrace as rtg_raytrace* defines it
 * (background material, intensity (1,1,1), stack capacity stackSize, the
 * context's semantics), NaN words stored as 0xFFC00000: bit for bit the fold
 * of rtg_raytrace_host(walk 0) over rtg_camera_rays_host's rays, and at the
 * identity pose rtg_render's frame.  Like rtg_raytrace it uses none of the
 * tables the renders keep for their own camera, so it is exact for any pose
 * and slower than rtg_render_device at the identity pose (README).
 *
 * RTG_ERR_INVALID with a message, before any GPU call, for a null pointer, an
 * empty frame, an aliasFactor above 256 or NaN, stackSize outside
 * 1..RTG_MAX_STACK, an unknown walk or semantics, a context without a scene
 * (the render only) or a frame of more than 2^31-1 workgroups.  Exercised up
 * to 32771 x 10923 pixels (the render, 4.30 GB) and 16384 x 21846 rays (8.6 GB)
 * (tests/test_gpu_large.py).
 *
 * Out of scope: row shards and multi-GPU for posed frames, a posed G-buffer
 * call (rtg_camera_rays_device plus rtg_intersect_device gives it), a camera
 * record in scene files, lens models. */
typedef struct rtg_camera { rtg_vec eye, right, up, back; } rtg_camera;   /* 48 B */
void rtg_camera_identity(rtg_camera* out);
/* All in float, in this order: back = vnorm(eye - target), right =
 * vnorm(cross(up, back)), up' = cross(back, right), with cross(a, b) =
 * (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).  look_at(0,
 * (0,0,-1), (0,1,0)) is the identity pose.  A degenerate input (eye ==
 * target, up parallel to the view) yields the NaN basis the arithmetic
 * yields and RTG_OK; the only error is a null pointer. */
int rtg_camera_look_at(const rtg_vec* eye, const rtg_vec* target, const rtg_vec* up,
                       rtg_camera* out);
/* *nAA = iterations of `for (int i = 0; i < aliasFactor; ++i)`: a pixel has
 * nAA * nAA samples.  aliasFactor above 256 or NaN is RTG_ERR_INVALID. */
int rtg_camera_sample_count(float aliasFactor, unsigned* nAA);
/* The pose's sample rays: W * H * nAA * nAA records in pixel order (row
 * major), a pixel's samples in the reference's order.  nAA == 0 writes
 * nothing and is RTG_OK.  nthreads <= 0: 1. */
int rtg_camera_rays_host(const rtg_camera* cam, unsigned width, unsigned height, float zoom,
                         float aliasFactor, rtg_ray* raysHost, int nthreads);
/* The same into device memory, asynchronously on `stream`.  The context names
 * the device; it needs no scene. */
int rtg_camera_rays_device(rtg_context* ctx, const rtg_camera* cam, unsigned width,
                           unsigned height, float zoom, float aliasFactor, rtg_ray* raysDevice,
                           void* stream);
/* The generator's inverse: where in the pose's W x H frame a point P lies.
 * All in float with no contraction and in this operand order, dot(a, b) =
 * (a.x * b.x + a.y * b.y) + a.z * b.z:
 *
 *   e.q = P.q - eye.q
 *   a = dot(e, right);  b = dot(e, up);  d = dot(e, back)
 *   k = zoom / d                       (the correctly rounded quotient)
 *   rx = a * k;  ry = b * k
 *   fx = rx * kx + halfW               kx = (float)W * 0.046875f  (= 1 / (xs * asp))
 *   fy = halfH - ry * ky               ky = (float)H / 12.f
 *                                      halfW = W * 0.5f, halfH = H * 0.5f
 *
 * out[i] = {fx, fy, k} as computed, NaN words stored as 0xFFC00000.  P lies in
 * front of the camera exactly when k > 0.f; the caller tests it.  Integer fx,
 * fy are the positions of the aa-1 sample rays of rtg_camera_rays*: the point
 * rtg_intersect* finds on the ray of pixel (x, y) projects to (x, y) up to
 * rounding.  This is the generator's inverse only for an orthonormal basis,
 * which is what rtg_camera_look_at builds; any other basis gives what the
 * arithmetic gives.  NaN and infinite inputs and d == 0 follow the arithmetic.
 *
 * n == 0 writes nothing and is RTG_OK.  RTG_ERR_INVALID with a message, before
 * any GPU call, for a null pointer, an empty frame, W or H above 2^24 (their
 * floats are then exact) or a batch of more than 2^31-1 workgroups (device).
 * Exercised up to n = 357 924 864 points (4.3 GB) (tests/test_gpu_large.py).
 * The device form is asynchronous on `stream`, takes points in device memory
 * and needs no scene; the pose is host memory, read before return. */
int rtg_camera_project_host(const rtg_camera* cam, unsigned width, unsigned height, float zoom,
                            const rtg_vec* points, size_t n, rtg_vec* outHost, int nthreads);
int rtg_camera_project_device(rtg_context* ctx, const rtg_camera* cam, unsigned width,
                              unsigned height, float zoom, const rtg_vec* pointsDevice, size_t n,
                              rtg_vec* outDevice, void* stream);
/* One-shot: uploads the points, runs on `device`, downloads n records. */
int rtg_camera_project(int device, const rtg_camera* cam, unsigned width, unsigned height,
                       float zoom, const rtg_vec* points, size_t n, rtg_vec* outHost);
/* Fused render of the pose's whole W x H frame (row major) into device memory
 * on `stream`, asynchronously: no ray buffer, no colour buffer, no fold on the
 * caller's side.  Follows rtg_context_set_semantics; rtg_set_launch_opts does
 * not apply.  Takes none of the context's render scratch: it may be mixed
 * freely with rtg_render_device, rtg_gbuffer_device, the ray queries and
 * rtg_raytrace_device on one context. */
int rtg_render_camera_device(rtg_context* ctx, const rtg_camera* cam, unsigned width,
                             unsigned height, float zoom, float aliasFactor, int stackSize,
                             rtg_vec* dstDevice, void* stream);
/* One-shot: uploads the scene, renders on `device`, downloads W*H rtg_vec. */
int rtg_render_camera(int device, const rtg_sphere* spheres, unsigned sphNum,
                      const rtg_light* lights, unsigned lgtNum, const rtg_camera* cam,
                      unsigned width, unsigned height, float zoom, float aliasFactor,
                      int stackSize, rtg_vec* dstHost);
/* The same on the host, no GPU call; walk, semantics and nthreads as in
 * rtg_raytrace_host (walk 0: plain loops, the yardstick; walk 1: the kernel's
 * own path over the packed tables). */
int rtg_render_camera_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                           unsigned lgtNum, const rtg_camera* cam, unsigned width,
                           unsigned height, float zoom, float aliasFactor, int stackSize,
                           int semantics, rtg_vec* dstHost, int walk, int nthreads);

/* ---- many posed views in one launch: cube maps, light probes ----
 * A probe bake renders many small frames (six faces per probe, hundreds of
 * probes, 16 x 16 to 64 x 64 pixels a face); one rtg_render_camera_device per
 * frame fills a fraction of the GPU and ends in its own tail.  These calls
 * take a table of nViews poses and write nViews frames of one size, view-major:
 * pixel (x, y) of view v at dst[(v * height + y) * width + x].
 *
 * VIEW v of the output is, bit for bit, the frame rtg_render_camera_host(...,
 * &poses[v], ..., walk 0) writes: the posed camera's arithmetic above, NaN
 * words as 0xFFC00000, the context's semantics (the `semantics` argument of
 * the host form), the stack capacity stackSize.  Width, height, zoom,
 * aliasFactor and stackSize are shared by all views; a view's pixels never
 * depend on another view's pose (a NaN pose spoils its own frame only).
 *
 * The device form reads the poses from DEVICE memory: nViews 48-byte
 * rtg_camera records, 4-byte aligned, complete before the call's work starts
 * on `stream`.  A caller may write them on the GPU (from rtg_intersect_device's
 * hit points, say) with no trip to the host.  It is asynchronous on `stream`,
 * follows rtg_context_set_semantics, takes none of the context's render
 * scratch (so it mixes with every other call on a context, as
 * rtg_render_camera_device does), and rtg_set_launch_opts does not apply.
 *
 * nViews == 0 is RTG_OK: nothing is launched, nothing is written, and the pose
 * table may be null.  RTG_ERR_INVALID with a message, before any GPU call, for
 * everything rtg_render_camera* rejects, a null pose table with nViews > 0, a
 * pose table off 4-byte alignment (device form), nViews * tilesX * tilesY
 * above 2^31-1 workgroups (tiles of 8 x 8 pixels, rounded up per view) and
 * nViews * width * height * 12 not representable in size_t.  Exercised up to
 * 7 views of 8192 x 8192 (5.6 GB of frames) (tests/test_gpu_large.py).
 *
 * Out of scope: per-view sizes or zooms, a G-buffer or ray generator over
 * views, row shards and multi-GPU for views, filtering or SH projection of
 * the faces. */
int rtg_render_views_device(rtg_context* ctx, const rtg_camera* posesDevice, size_t nViews,
                            unsigned width, unsigned height, float zoom, float aliasFactor,
                            int stackSize, rtg_vec* dstDevice, void* stream);
/* One-shot: uploads the scene and the poses, renders on `device`, downloads
 * nViews * W * H rtg_vec. */
int rtg_render_views(int device, const rtg_sphere* spheres, unsigned sphNum,
                     const rtg_light* lights, unsigned lgtNum, const rtg_camera* poses,
                     size_t nViews, unsigned width, unsigned height, float zoom,
                     float aliasFactor, int stackSize, rtg_vec* dstHost);
/* The same on the host, no GPU call; walk, semantics and nthreads as in
 * rtg_render_camera_host (threads take contiguous bands of the nViews * W * H
 * pixels). */
int rtg_render_views_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                          unsigned lgtNum, const rtg_camera* poses, size_t nViews,
                          unsigned width, unsigned height, float zoom, float aliasFactor,
                          int stackSize, int semantics, rtg_vec* dstHost, int walk, int nthreads);
/* The six 90-degree poses of a cube map at `eye`, in the order +X, -X, +Y, -Y,
 * +Z, -Z, for a SQUARE frame rendered at zoom = -1.  Face f has forward axis
 * F, right axis R = F x U and up axis U:
 *
 *    f   face   F           R           U
 *    0   +X    ( 1, 0, 0)  ( 0, 0, 1)  ( 0, 1, 0)
 *    1   -X    (-1, 0, 0)  ( 0, 0,-1)  ( 0, 1, 0)
 *    2   +Y    ( 0, 1, 0)  (-1, 0, 0)  ( 0, 0,-1)
 *    3   -Y    ( 0,-1, 0)  (-1, 0, 0)  ( 0, 0, 1)
 *    4   +Z    ( 0, 0, 1)  (-1, 0, 0)  ( 0, 1, 0)
 *    5   -Z    ( 0, 0,-1)  ( 1, 0, 0)  ( 0, 1, 0)
 *
 * and out[f] = {eye, right = R * (3.f/32.f), up = U * (float)(1.0/6.0), back =
 * -F}, a zero component being +0.  The frame's edge is at rx = -+8 * (16/12)
 * and ry = +-6 (main.cpp:384-402), so 8 * (16/12) * (3/32) = 1 and 6 * (1/6)
 * = 1 in float: the face spans -1..1 along R and U at distance 1 along F.  The
 * four side faces have U = +Y (the image's top row is up); +Y takes U = -Z
 * and -Y takes U = +Z, which is the +Z face pitched up and down, and (R, U,
 * -F) is right-handed on all six; face 5 is the identity pose's basis, scaled.
 * The reference's sample grid starts at a pixel's CORNER, not its centre
 * (main.cpp:411-436, camera_dir), and the faces inherit that: sample (0, 0) of
 * pixel (0, 0) is the face's top left corner exactly, a face holds its top and
 * left edges and not its bottom and right ones, and with aliasFactor > 1 the
 * samples of a pixel lie right of and ABOVE its corner.  (So +Y's top row and
 * left column are, at aliasFactor 1, directions the side faces' top rows have
 * too.)  The only error is a null pointer. */
int rtg_camera_cube(const rtg_vec* eye, rtg_camera out[6]);

/* ---- views folded into per-group coefficients: SH light probes ----
 * A probe is not its faces but a handful of numbers: nine SH coefficients,
 * six ambient-cube colours, a mean.  These calls reduce GROUPS of views with
 * a caller-owned weight table, in a float summation order that is defined
 * here, so the result is the same words on the host and on every GPU.
 *
 * INPUTS.  nViews frames of W x H pixels (rtg_vec), view-major, as
 * rtg_render_views* writes them.  A group is G = viewsPerGroup >= 1
 * consecutive views; nViews is a multiple of G and nGroups = nViews / G.
 * K = weights, 1 <= K <= RTG_FOLD_MAX_WEIGHTS.  ONE weight table of G * W * H
 * * K floats is shared by all groups: w[e * K + k] is weight k of texel e =
 * (f * H + y) * W + x, f the view's index inside its group.  The caller owns
 * the table (a device pointer in the device calls), so no transcendental
 * function is evaluated inside the defined arithmetic, as with rtg_ao*'s
 * direction table.
 *
 * ARITHMETIC, all in float with no contraction and in this order:
 *   term     for texel e of group g, weight k, channel q:
 *              term = w[e * K + k] * pix.q,  pix the pixel of view g * G + f.
 *            With RTG_FOLD_SKIP_NONFINITE a pixel with any word whose exponent
 *            field is all ones (NaN, +-inf) gives +0.f for every k and q and
 *            counts one towards the group's `skipped`.  The weight is never
 *            tested.
 *   tile     a view is cut into the views kernel's 8 x 8 tiles, row-major;
 *            lane l is pixel (l % 8, l / 8) of the tile, a lane outside the
 *            frame holds +0.f.  For s = 1, 2, 4, 8, 16, 32 in that order:
 *              v[l] = v[l] + v[l + s]  for every l that is a multiple of 2s.
 *            The tile's sum is v[0] (what lane 0 of a wave holds after an xor
 *            butterfly in that order).
 *   group    acc = +0.f; for f = 0 .. G-1, for each tile of view g * G + f in
 *            tile order: acc = acc + tilesum.   out[g * K + k].q = acc, NaN
 *            words stored as 0xFFC00000, as every record's.
 *   skipped  skipped[g] (may be null) is the group's count of skipped texels,
 *            0 without the flag.
 * NaN, infinite and -0 inputs follow the arithmetic as written.
 *
 * rtg_views_fold_host restates this in plain loops: the yardstick.
 * rtg_views_fold_device folds frames already in device memory (its context
 * names the device; it needs no scene).  rtg_render_views_fold_device is the
 * FUSED call: poses in, coefficients out, no frame written anywhere; word for
 * word rtg_views_fold_host over rtg_render_views_host(walk 0)'s frames.  It
 * follows rtg_context_set_semantics, takes none of the context's render
 * scratch and allocates nothing.  Both device calls are asynchronous on
 * `stream` and need a caller-owned scratch for their tile partials, 3K + 1
 * words per tile of every view (rtg_views_fold_scratch gives the bytes):
 * 16-byte aligned, and the call's until the call has finished on the stream.
 * `params` is host memory in every call, read before the call returns.
 *
 * nViews == 0 is RTG_OK: nothing is launched, nothing is written, and the
 * pose table, the frames and the scratch may be null.  RTG_ERR_INVALID with a
 * message, before any GPU call, for everything rtg_render_views* rejects, a
 * null params, weight table, output or (nViews > 0) scratch, G == 0, nViews
 * not a multiple of G, K outside 1..RTG_FOLD_MAX_WEIGHTS, an unknown flag, a
 * scratch that is too small or off 16-byte alignment, and G * W * H * K floats
 * or the scratch size not representable in size_t.  rtg_views_fold_device is
 * exercised up to 7 frames of 8192 x 8192 (5.6 GB) and a weight table as large
 * (tests/test_gpu_large.py).
 *
 * Out of scope: per-group weight tables, per-view sizes, a tree-shaped group
 * sum (the sequential one is the definition; it is slow only for very large
 * faces), irradiance convolution or windowing, folds over G-buffers or ray
 * batches, row shards and multi-GPU. */
#define RTG_FOLD_MAX_WEIGHTS 16
#define RTG_FOLD_SKIP_NONFINITE 1  /* flags: a NaN or infinite pixel adds +0.f and is counted */
typedef struct rtg_fold_params {
  unsigned viewsPerGroup; /* G >= 1; nViews is a multiple of it */
  unsigned weights;       /* K, 1..RTG_FOLD_MAX_WEIGHTS */
  unsigned flags;         /* RTG_FOLD_* bits; an unknown bit is RTG_ERR_INVALID */
} rtg_fold_params;
/* Bytes of tile partials the device calls need: nViews * tiles * (3K + 1) * 4,
 * tiles = ceil(W / 8) * ceil(H / 8). */
int rtg_views_fold_scratch(size_t nViews, unsigned width, unsigned height, unsigned weights,
                           size_t* bytes);
/* Plain loops; the result does not depend on nthreads (threads take whole
 * groups).  nthreads <= 0: 1. */
int rtg_views_fold_host(const rtg_vec* frames, size_t nViews, unsigned width, unsigned height,
                        const rtg_fold_params* params, const float* weights, rtg_vec* out,
                        unsigned* skipped, int nthreads);
int rtg_views_fold_device(rtg_context* ctx, const rtg_vec* framesDevice, size_t nViews,
                          unsigned width, unsigned height, const rtg_fold_params* params,
                          const float* weightsDevice, rtg_vec* outDevice, unsigned* skippedDevice,
                          void* scratchDevice, size_t scratchBytes, void* stream);
int rtg_render_views_fold_device(rtg_context* ctx, const rtg_camera* posesDevice, size_t nViews,
                                 unsigned width, unsigned height, float zoom, float aliasFactor,
                                 int stackSize, const rtg_fold_params* params,
                                 const float* weightsDevice, rtg_vec* outDevice,
                                 unsigned* skippedDevice, void* scratchDevice,
                                 size_t scratchBytes, void* stream);
/* One-shot: uploads the scene, the poses and the weights, allocates its own
 * scratch, runs the fused call on `device`, downloads nGroups * K rtg_vec and
 * (skipped not null) nGroups counts. */
int rtg_render_views_fold(int device, const rtg_sphere* spheres, unsigned sphNum,
                          const rtg_light* lights, unsigned lgtNum, const rtg_camera* poses,
                          size_t nViews, unsigned width, unsigned height, float zoom,
                          float aliasFactor, int stackSize, const rtg_fold_params* params,
                          const float* weights, rtg_vec* outHost, unsigned* skippedHost);
/* Renders on the host (rtg_render_views_host: walk, semantics, nthreads), then
 * folds on the host; no GPU call. */
int rtg_render_views_fold_host(const rtg_sphere* spheres, unsigned sphNum,
                               const rtg_light* lights, unsigned lgtNum, const rtg_camera* poses,
                               size_t nViews, unsigned width, unsigned height, float zoom,
                               float aliasFactor, int stackSize, int semantics,
                               const rtg_fold_params* params, const float* weights,
                               rtg_vec* outHost, unsigned* skippedHost, int walk, int nthreads);
/* A convenience, host only: real-SH projection weights for rtg_camera_cube's
 * six faces of res x res at zoom -1, G = 6, K = bands * bands (bands 1..4),
 * k = l * (l + 1) + m:  out[e * K + k] = Y_k(d_e) * O_e, 6 * res * res * K
 * floats.  d_e is the normalised MEAN sample position of pixel e under its
 * face's basis: the pixel's corner is u = -1 + 2x / res along R, v = 1 - 2y /
 * res along U, and sample (i, j) lies 2j / (res * aliasFactor) right of it and
 * (8/3) i / (res * aliasFactor) above it (the reference's sample step is not
 * scaled by the aspect vertically).  O_e is the solid angle of the pixel's
 * cell [u, u + 2 / res] x [v, v + 2 / res] seen from the eye, scaled so that
 * the 6 * res * res values sum to 4 pi.  Y_k is the orthonormal real basis
 * (Y_0 = 1 / (2 sqrt(pi)), m < 0 the sine terms), so folding an all-ones cube
 * gives c_0 = 2 sqrt(pi).  Computed in double and rounded to float; its bits
 * are NOT part of the contract, as rtg_ao_directions' are not.
 * RTG_ERR_INVALID for a null pointer, res == 0, bands outside 1..4, an
 * aliasFactor rtg_render_views* rejects or a table size that overflows. */
int rtg_cube_sh_weights(unsigned res, unsigned bands, float aliasFactor, float* out);

/* ---- ambient occlusion: hemisphere visibility per hit point ----
 * Hit points go in, one count of unoccluded probes per point comes out: no
 * segment buffer, no sort and no fold on the caller's side.  The call takes n
 * rtg_hit records exactly as rtg_intersect* writes them, and a table of nDirs
 * local directions `dirs`, samples <= nDirs <= RTG_AO_MAX_DIRS, in the frame
 * whose z axis is the normal.  The directions are used as given: they are not
 * normalised, and any length or sign is legal.  The caller owns the table (a
 * device pointer in the device calls), so no sin or cos is evaluated inside
 * the defined arithmetic.
 *
 * PROBE k of point i (P = point, N = normal), all in float with no contraction
 * and in this operand order:
 *   frame    s = copysignf(1, N.z);  a = -1.f / (s + N.z);  b = (N.x * N.y) * a
 *            T1 = (1.f + s * ((N.x * N.x) * a), s * b, -(s * N.x))
 *            T2 = (b, s + (N.y * N.y) * a, -N.y)
 *   window   s_i = (flags & RTG_AO_JITTER) ? mix32(seed + (unsigned)i) % nDirs : 0
 *            mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 *                      x *= 0x846ca68b; x ^= x >> 16   (32-bit, wrapping)
 *            j = s_i + k, minus nDirs if j >= nDirs;  l = dirs[j]
 *   world    per component q: w.q = (l.x * T1.q + l.y * T2.q) + l.z * N.q
 *            (the posed camera's form)
 *   segment  a.q = P.q + bias * N.q;  b.q = a.q + radius * w.q
 * A record with id < 0 (no point) has K all-zero segments.
 *
 * out[i] (an unsigned short) is the number of k in 0..K-1 for which
 * hasClearLineOfSight(a, b) holds, exactly as rtg_visible defines it (a
 * segment with a == b is visible by its rule): the count of UNOCCLUDED
 * probes, out[i] / (float)K the usual AO term.  A record with id < 0 gets K
 * and makes no query.  NaN, infinite and degenerate inputs follow the
 * arithmetic and the comparisons as written.  The result does not depend on
 * lights, stackSize or rtg_context_set_semantics.
 *
 * rtg_ao_segments* write the n * K segments, point-major (segment k of point
 * i at i * K + k): the generator that pins the definition.  NaN words are
 * written as 0xFFC00000, as every record's.  rtg_ao* is, word for word, the
 * per-point sum of rtg_visible_host(walk 0) over them.
 *
 * n == 0 is RTG_OK with no launch.  RTG_ERR_INVALID with a message, before
 * any GPU call, for a null pointer, samples outside 1..RTG_AO_MAX_SAMPLES,
 * nDirs outside samples..RTG_AO_MAX_DIRS, an unknown flag, n > 2^32 - 1, an
 * n * K that overflows size_t (the segments), more than 2^31-1 workgroups (64
 * lanes each) or, for the fused call only, a context without a scene.
 * Exercised up to n = 134 217 792 records (4.29 GB) and, the segments, n * K =
 * 268 439 552 (6.4 GB) (tests/test_gpu_large.py).
 *
 * Out of scope: an _indexed form, bent normals, distance falloff, a
 * G-buffer-record input, multi-GPU batches. */
#define RTG_AO_MAX_SAMPLES 1024
#define RTG_AO_MAX_DIRS    65536
#define RTG_AO_JITTER 1            /* flags: per-point window into the direction table */
typedef struct rtg_ao_params {
  unsigned samples;  /* K probes per point, 1..RTG_AO_MAX_SAMPLES */
  float radius;      /* probe length factor, used as given */
  float bias;        /* start offset along the normal, used as given */
  unsigned seed;     /* RTG_AO_JITTER only */
  unsigned flags;    /* RTG_AO_* bits; an unknown bit is RTG_ERR_INVALID */
} rtg_ao_params;
/* A convenience, host only: the cosine-weighted golden-angle set, u = (k +
 * 0.5) / nDirs, phi = 2 pi frac(k * 0.6180339887498949), direction k =
 * (sqrt(u) cos phi, sqrt(u) sin phi, sqrt(1 - u)), computed in double and
 * rounded to float.  Its bits are NOT part of the contract (libm's sin and
 * cos are involved): a caller who needs the same counts everywhere keeps the
 * table it used.  nDirs outside 1..RTG_AO_MAX_DIRS is RTG_ERR_INVALID. */
int rtg_ao_directions(unsigned nDirs, rtg_vec* out);
/* The n * K probe segments on the host.  nthreads <= 0: 1. */
int rtg_ao_segments_host(const rtg_hit* hits, size_t n, const rtg_ao_params* params,
                         const rtg_vec* dirs, unsigned nDirs, rtg_segment* segsHost,
                         int nthreads);
/* The same into device memory, asynchronously on `stream`.  The context names
 * the device; it needs no scene.  `params` is host memory in every call, read
 * before the call returns. */
int rtg_ao_segments_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                           const rtg_ao_params* params, const rtg_vec* dirsDevice,
                           unsigned nDirs, rtg_segment* segsDevice, void* stream);
/* The fused kernel: n counts into outDevice, asynchronously on `stream`.
 * Allocates nothing, takes none of the context's render scratch and may be
 * mixed with every other call on the context. */
int rtg_ao_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                  const rtg_ao_params* params, const rtg_vec* dirsDevice, unsigned nDirs,
                  unsigned short* outDevice, void* stream);
/* One-shot: uploads the scene, the hits and the table, runs on `device`,
 * downloads n counts. */
int rtg_ao(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits,
           size_t n, const rtg_ao_params* params, const rtg_vec* dirs, unsigned nDirs,
           unsigned short* outHost);
/* The same on the host, no GPU call.  walk 0: plain loops over every probe
 * and sphere (the yardstick).  walk 1: the kernel's own path over the packed
 * tables, as rtg_visible_host.  nthreads <= 0: 1. */
int rtg_ao_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits, size_t n,
                const rtg_ao_params* params, const rtg_vec* dirs, unsigned nDirs,
                unsigned short* outHost, int walk, int nthreads);

/* ---- direct light: calculateMatte per hit point ----
 * Hit points go in, the direct (Lambert) light of the scene's lights at each
 * point comes out, with a mask of the lights that reach it: lightmaps,
 * irradiance probes and shadow masks for a caller's own shading in one launch,
 * with no n x m segment buffer.  The call takes n rtg_hit records exactly as
 * rtg_intersect* writes them; the lights are the context's (the one-shot and
 * host forms take them as arguments).  It pairs with rtg_ao* on the same
 * records.
 *
 * For a record with id >= 0, P = point and N = normal, all in float with no
 * contraction and in this operand order (calculateMatte, raytracer.h:313-367):
 *   sum = (0, 0, 0)
 *   for l = 0 .. m-1, in order:
 *     dist = L_l.pos - P                                   (per component)
 *     gap  = (dist.x * dist.x + dist.y * dist.y) + dist.z * dist.z
 *     dir  = (1.f / sqrt(gap)) * dist                      (vec.h:41)
 *     incidence = (N.x * dir.x + N.y * dir.y) + N.z * dir.z
 *     if hasClearLineOfSight(P, L_l.pos), rtg_visible's rule for the segment
 *        (P, L_l.pos) word for word, and incidence > 0.f:
 *          intensity = incidence / gap
 *          sum.q = sum.q + intensity * L_l.col.q           (per component q)
 *          bit l of the mask is set                        (l < 64 only)
 *   out[i] = sum, NaN words written as 0xFFC00000;  lit[i] = the mask
 * A record with id < 0 gets (0, 0, 0) and mask 0 and makes no query.  `id` is
 * read for its sign only (an id >= sphNum is legal and is never used as an
 * index) and `t` is not read.  The normal is used as given: it is not
 * normalised, and a flipped or scaled normal is legal.  There is no bias: the
 * reference starts its shadow ray at P and relies on raySphere's 1e-5 window,
 * and so does this call.  NaN, infinite and degenerate inputs (P == L, a NaN
 * or infinite light) follow the arithmetic and the comparisons as written.
 * Lights from index 64 on add to the sum and set no bit.  The result does not
 * depend on stackSize or rtg_context_set_semantics.  On a scene whose spheres
 * are opaque, white and matte, rtg_raytrace* of a ray is rtg_matte* of its
 * rtg_intersect* record.
 *
 * `lit` may be NULL: it exists for callers with their own BRDF, who need the
 * per-light visibility and not the Lambert sum.
 *
 * n == 0 is RTG_OK with no launch.  RTG_ERR_INVALID with a message, before
 * any GPU call, for a null hit or output buffer, a context without a scene,
 * n > 2^32 - 1, more than 2^31-1 workgroups (64 lanes each) or an unknown
 * walk.  Exercised up to n = 134 217 792 records (4.29 GB) (tests/test_gpu_large.py).
 *
 * Out of scope: lights other than the context's, an _indexed form, a
 * per-light colour breakdown beyond the mask, gloss or specular terms, a
 * generator of surface sample points (a caller's rays through rtg_intersect*
 * give the records), multi-GPU batches. */
/* The fused kernel: n sums into outDevice (12 B each) and, when litDevice is
 * not NULL, n masks (8-byte aligned), asynchronously on `stream`.  Allocates
 * nothing, takes none of the context's render scratch and may be mixed with
 * every other call on the context. */
int rtg_matte_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n, rtg_vec* outDevice,
                     unsigned long long* litDevice, void* stream);
/* One-shot: uploads the scene and the hits, runs on `device`, downloads the
 * sums and (litHost not NULL) the masks. */
int rtg_matte(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
              unsigned lgtNum, const rtg_hit* hits, size_t n, rtg_vec* outHost,
              unsigned long long* litHost);
/* The same on the host, no GPU call.  walk 0: plain loops over every light
 * and sphere (the yardstick).  walk 1: the kernel's own path over the packed
 * tables, as rtg_visible_host.  nthreads <= 0: 1. */
int rtg_matte_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                   unsigned lgtNum, const rtg_hit* hits, size_t n, rtg_vec* outHost,
                   unsigned long long* litHost, int walk, int nthreads);

/* ---- irradiance: a grid of SH probes per hit point ----
 * Hit points go in, the light that a lattice of baked probes holds for each
 * point comes out, with the interpolation weight that was left: the consumer
 * of rtg_render_views_fold*'s coefficients, and the table-driven alternative
 * to rtg_gather* for indirect light.  A plain trilinear fetch is not usable:
 * probes inside a sphere and probes behind a wall leak their light, so the
 * lookup leaves out invalid probes, probes behind the point's tangent plane
 * and probes the point cannot see, which makes it a scene query (rtg_visible's
 * rule for eight segments per point that share their origin), fused: no n x 8
 * segment buffer on the caller's side.  The call takes n rtg_hit records
 * exactly as rtg_intersect* writes them and pairs with rtg_ao*, rtg_matte* and
 * rtg_gather* on the same records.
 *
 * THE GRID.  Probe (ix, iy, iz) of an nx x ny x nz lattice has index
 * p = (iz * ny + iy) * nx + ix and position X_p.q = origin.q + (float)i_q *
 * step.q.  Its K = bands * bands coefficients (rtg_vec) are coeffs[p * K + k],
 * k = l * (l + 1) + m: exactly what rtg_render_views_fold* writes with G = 6,
 * one group per probe in index order, and rtg_cube_sh_weights' table, so a
 * bake feeds the lookup with no reshuffle.  valid[p] (RTG_IRR_VALID only) is
 * one byte per probe, 0: leave the probe out.  The validity bytes are the
 * caller's: rtg_contains*(rtg_probe_grid_points) < 0 gives them (a probe
 * inside a sphere sees only that sphere's inside).
 *
 * ARITHMETIC, all in float with no contraction and in this order.  A record
 * with id < 0 gets (0, 0, 0) and weight +0.f and makes no query.  For a record
 * with id >= 0 (`id` is read for its sign only, `t` is not read, N = normal is
 * used as given: not normalised, a flipped or scaled normal is legal):
 *   start    A.q = P.q + bias * N.q                        (rtg_ao*'s start point)
 *   cell     per axis q:  g = (A.q - origin.q) / step.q
 *              if !(g >= 0.f) g = 0.f                       (NaN goes to 0)
 *              if g > (float)(n_q - 1) g = (float)(n_q - 1)
 *              i0 = (unsigned)g, lowered to n_q - 2 when above it and n_q >= 2
 *              f = g - (float)i0
 *              i1 = i0 + 1 if that is < n_q, else i0
 *   basis    once per point, c0 .. c4 the constants of the orthonormal real
 *            basis (rtg_cube_sh_weights' Y_k) rounded from double to float,
 *            c0 = 0.28209479177387814, c1 = 0.4886025119029199, c2 =
 *            1.0925484305920792, c3 = 0.31539156525252005, c4 =
 *            0.5462742152960396:
 *              b0 = lobe[0] * c0
 *              b1 = lobe[1] * (c1 * N.y)    b2 = lobe[1] * (c1 * N.z)
 *              b3 = lobe[1] * (c1 * N.x)
 *              b4 = lobe[2] * (c2 * (N.x * N.y))
 *              b5 = lobe[2] * (c2 * (N.y * N.z))
 *              b6 = lobe[2] * (c3 * (3.f * (N.z * N.z) - 1.f))
 *              b7 = lobe[2] * (c2 * (N.x * N.z))
 *              b8 = lobe[2] * (c4 * (N.x * N.x - N.y * N.y))
 *   corners  W = +0.f, acc = (0, 0, 0); for c = 0 .. 7 in order: bits cx = c &
 *            1, cy = (c >> 1) & 1, cz = c >> 2 pick i1 (set) or i0 per axis,
 *            and t_q = f_q (set) or 1.f - f_q;  w = (t_x * t_y) * t_z.  The
 *            corner's probe p is LEFT OUT if any of these holds:
 *              !(w > 0.f)                                   (zero or NaN)
 *              RTG_IRR_VALID and valid[p] == 0
 *              RTG_IRR_FACING and !(s > 0.f), with d = X_p - A and
 *                s = (N.x * d.x + N.y * d.y) + N.z * d.z
 *              RTG_IRR_VISIBLE and the segment (A, X_p) is blocked under
 *                rtg_visible's rule, word for word
 *            (the query has no side effect: it is made only for corners that
 *            passed the other tests).  A kept corner does
 *              e = (+0.f, +0.f, +0.f)
 *              for k = 0 .. K-1:  e.q = e.q + b_k * coeffs[p * K + k].q
 *              W = W + w;  acc.q = acc.q + w * e.q
 *   result   out[i].q = acc.q / W if W > 0.f, else (0, 0, 0); NaN words are
 *            stored as 0xFFC00000, as every record's.  weight[i] = W (`weight`
 *            may be NULL): where it is 0 no probe reached the point and the
 *            caller falls back to its ambient term.
 * So an axis with n_q == 1 has f = 0: its second corner has weight 0 and is
 * never fetched (a flat floor-plan grid), and a point outside the lattice
 * takes the boundary cell's edge.  Coefficients are used as given, so a NaN
 * or infinite coefficient follows the arithmetic: bake with
 * RTG_FOLD_SKIP_NONFINITE.  The result does not depend on lights, stackSize
 * or rtg_context_set_semantics.
 *
 * lobe[l] scales band l: RTG_IRR_LOBE_RADIANCE reconstructs the baked radiance
 * along N, RTG_IRR_LOBE_COSINE is the clamped-cosine convolution (irradiance /
 * pi, the radiance a white matte surface leaves with).
 *
 * rtg_irradiance_device is the FUSED call, asynchronous on `stream`: it
 * allocates nothing, takes none of the context's render scratch and may be
 * mixed with every other call on the context.  `grid` and `params` are host
 * memory in every call, read before the call returns.  The context needs a
 * scene only with RTG_IRR_VISIBLE; without that flag a context with no scene
 * is legal, as with rtg_views_fold_device.
 *
 * n == 0 is RTG_OK with no launch.  RTG_ERR_INVALID with a message, before
 * any GPU call, for a null hit, coefficient, params, grid or output pointer,
 * a null `valid` with RTG_IRR_VALID, a step that is not finite or not > 0, a
 * non-finite origin, a dimension outside 1..2^20, nx * ny * nz * K > 2^31 - 1,
 * bands outside 1..3, an unknown flag, an unknown walk, n > 2^32 - 1, more
 * than 2^31-1 workgroups (64 lanes each), or RTG_IRR_VISIBLE on a context
 * without a scene.
 *
 * Out of scope: smooth backface wraps, Chebyshev or depth-moment visibility
 * (DDGI), bands above 3, per-probe offsets, probes off a lattice, an _indexed
 * form, a device-side pose generator, multi-GPU batches. */
typedef struct rtg_probe_grid {
  rtg_vec origin;        /* position of probe (0,0,0) */
  rtg_vec step;          /* spacing per axis; finite and > 0 */
  unsigned nx, ny, nz;   /* >= 1 each, <= 2^20 each; nx*ny*nz*K <= 2^31 - 1 */
  unsigned bands;        /* 1..3; K = bands*bands coefficients (rtg_vec) per probe */
} rtg_probe_grid;

#define RTG_IRR_VALID    1  /* a corner whose valid[] byte is 0 is left out */
#define RTG_IRR_FACING   2  /* a corner not in front of the point's tangent plane is left out */
#define RTG_IRR_VISIBLE  4  /* a corner the point does not see is left out */
typedef struct rtg_irradiance_params {
  float bias;      /* start offset along the normal, used as given (rtg_ao's) */
  float lobe[3];   /* per-band factor l = 0, 1, 2; used as given */
  unsigned flags;  /* an unknown bit is RTG_ERR_INVALID */
} rtg_irradiance_params;
#define RTG_IRR_LOBE_RADIANCE {1.f, 1.f, 1.f}          /* reconstructs the baked radiance along N */
#define RTG_IRR_LOBE_COSINE   {1.f, 2.f / 3.f, 0.25f}  /* clamped-cosine irradiance / pi */
/* Host conveniences whose bits ARE part of the contract (one multiplication
 * and one addition per word, and a copy): the nx * ny * nz probe positions in
 * index order, and rtg_camera_cube of each, 6 per probe, probe-major: the pose
 * table of a bake with G = 6.  RTG_ERR_INVALID for a null pointer or a grid
 * the lookup rejects. */
int rtg_probe_grid_points(const rtg_probe_grid* grid, rtg_vec* out);
int rtg_probe_grid_poses(const rtg_probe_grid* grid, rtg_camera* out);
/* The fused kernel: n colours into outDevice (12 B each) and, when
 * weightDevice is not NULL, n weights.  validDevice may be NULL without
 * RTG_IRR_VALID. */
int rtg_irradiance_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                          const rtg_probe_grid* grid, const rtg_vec* coeffsDevice,
                          const unsigned char* validDevice, const rtg_irradiance_params* params,
                          rtg_vec* outDevice, float* weightDevice, void* stream);
/* One-shot: uploads the scene, the hits and the tables, runs on `device`,
 * downloads the colours and (weightHost not NULL) the weights. */
int rtg_irradiance(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits,
                   size_t n, const rtg_probe_grid* grid, const rtg_vec* coeffs,
                   const unsigned char* valid, const rtg_irradiance_params* params,
                   rtg_vec* outHost, float* weightHost);
/* The same on the host, no GPU call.  walk 0: plain loops over every corner
 * and sphere (the yardstick).  walk 1: the kernel's own path over the packed
 * tables, as rtg_visible_host.  nthreads <= 0: 1. */
int rtg_irradiance_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_hit* hits, size_t n,
                        const rtg_probe_grid* grid, const rtg_vec* coeffs,
                        const unsigned char* valid, const rtg_irradiance_params* params,
                        rtg_vec* outHost, float* weightHost, int walk, int nthreads);

/* ---- gather: a hemisphere of rayTrace colours per hit point ----
 * Hit points go in, one colour per point comes out: the weighted sum of
 * rayTrace's colour along K directions of the point's hemisphere, the one-bounce
 * indirect light ("final gather") of a lightmap or irradiance bake, with no
 * n x K ray buffer, no colour buffer, no sort and no fold on the caller's side.
 * The call takes n rtg_hit records exactly as rtg_intersect* writes them, a
 * table of nDirs local directions `dirs` in the frame whose z axis is the
 * normal, and a table of nDirs floats `weights`, one per direction, samples <=
 * nDirs <= RTG_GATHER_MAX_DIRS.  Both tables are the caller's (device pointers
 * in the device calls), as with rtg_ao*: rtg_ao_directions(K) with weights 1 / K
 * is the cosine-weighted estimate of the irradiance over pi.  It pairs with
 * rtg_ao* and rtg_matte* on the same records.
 *
 * For a record with id >= 0 (P = point, N = normal), all in float with no
 * contraction and in this operand order:
 *   point, frame, window   rtg_ao's, word for word: a.q = P.q + bias * N.q, the
 *            frame T1, T2, N, the window s_i (RTG_GATHER_JITTER, seed) and the
 *            table index j of probe k
 *   world    per component q: w.q = (l.x * T1.q + l.y * T2.q) + l.z * N.q with
 *            l = dirs[j] (rtg_ao's `world`)
 *   ray k    origin = a;  dir = (1.f / sqrt((w.x * w.x + w.y * w.y) + w.z * w.z)) * w
 *            (vec.h:41, the posed camera's normalisation: the reference's rays
 *            are unit rays, and a scaled normal or table entry must not change
 *            what rayTrace shades with)
 *   colour   c_k = rayTrace(ray k) exactly as rtg_raytrace* defines it:
 *            background material, intensity (1, 1, 1), stack capacity
 *            stackSize, the context's semantics (the host form takes them)
 *   sum      acc = (+0, +0, +0);  for k = 0 .. K-1 in order, per component q:
 *              acc.q = acc.q + weights[j] * c_k.q
 *            With RTG_GATHER_SKIP_NONFINITE a colour with any word whose
 *            exponent field is all ones (NaN or +-inf) adds +0.f to every
 *            channel instead and counts one towards skipped[i]; the weight is
 *            never tested.
 *   out[i] = acc, NaN words written as 0xFFC00000;  skipped[i] (an unsigned
 *            short; 0 without the flag)
 * A record with id < 0 (no point) gets (0, 0, 0) and skipped 0 and makes no
 * trace.  The directions, the weights and the normal are used as given: any
 * length or sign is legal, a zero or NaN direction gives a NaN ray, and NaN,
 * infinite and degenerate inputs follow the arithmetic and the comparisons as
 * written.  `skipped` may be NULL.
 *
 * rtg_gather_rays* write the n * K rays, point-major (ray k of point i at i * K
 * + k), all-zero rays for a record with id < 0: the generator that pins the
 * definition.  NaN words are written as 0xFFC00000, as every record's.
 *
 * THE CONTRACT: rtg_gather_host(walk 0) is, word for word, the sum above over
 * rtg_raytrace_host(walk 0) of rtg_gather_rays_host's rays; walk 1, the fused
 * device call and the one-shot give the same words.
 *
 * n == 0 is RTG_OK with no launch.  RTG_ERR_INVALID with a message, before
 * any GPU call, for a null pointer (`skipped` excepted), samples outside
 * 1..RTG_GATHER_MAX_SAMPLES, nDirs outside samples..RTG_GATHER_MAX_DIRS, an
 * unknown flag, a stackSize outside 1..RTG_MAX_STACK, an unknown walk or
 * semantics, n > 2^32 - 1, an n * K that overflows size_t (the rays), more than
 * 2^31-1 workgroups (64 lanes each) or, for the fused call only, a context
 * without a scene.  Exercised up to n = 134 217 792 records (4.29 GB) and, the
 * rays, n * K = 268 439 552 (6.4 GB) (tests/test_gpu_large.py).
 *
 * Out of scope: per-point direction tables, hit distances or bent normals as
 * outputs, an _indexed form, re-sorting the rays between bounces, multi-GPU
 * batches. */
#define RTG_GATHER_MAX_SAMPLES 1024
#define RTG_GATHER_MAX_DIRS    65536
#define RTG_GATHER_JITTER          1  /* per-point window into the tables, as RTG_AO_JITTER */
#define RTG_GATHER_SKIP_NONFINITE  2  /* a NaN or infinite colour adds +0.f and is counted */
typedef struct rtg_gather_params {    /* 16 B */
  unsigned samples;  /* K probes per point, 1..RTG_GATHER_MAX_SAMPLES */
  float bias;        /* start offset along the normal, used as given */
  unsigned seed;     /* RTG_GATHER_JITTER only */
  unsigned flags;    /* RTG_GATHER_* bits; an unknown bit is RTG_ERR_INVALID */
} rtg_gather_params;
/* The n * K probe rays on the host.  nthreads <= 0: 1. */
int rtg_gather_rays_host(const rtg_hit* hits, size_t n, const rtg_gather_params* params,
                         const rtg_vec* dirs, unsigned nDirs, rtg_ray* raysHost, int nthreads);
/* The same into device memory, asynchronously on `stream`.  The context names
 * the device; it needs no scene.  `params` is host memory in every call, read
 * before the call returns. */
int rtg_gather_rays_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                           const rtg_gather_params* params, const rtg_vec* dirsDevice,
                           unsigned nDirs, rtg_ray* raysDevice, void* stream);
/* The fused kernel: n sums into outDevice (12 B each) and, when skippedDevice
 * is not NULL, n counts, asynchronously on `stream`.  Allocates nothing, takes
 * none of the context's render scratch and may be mixed with every other call
 * on the context. */
int rtg_gather_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                      const rtg_gather_params* params, const rtg_vec* dirsDevice,
                      const float* weightsDevice, unsigned nDirs, int stackSize,
                      rtg_vec* outDevice, unsigned short* skippedDevice, void* stream);
/* One-shot: uploads the scene, the hits and the tables, runs on `device`
 * (CPU semantics), downloads the sums and (skippedHost not NULL) the counts. */
int rtg_gather(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
               unsigned lgtNum, const rtg_hit* hits, size_t n, const rtg_gather_params* params,
               const rtg_vec* dirs, const float* weights, unsigned nDirs, int stackSize,
               rtg_vec* outHost, unsigned short* skippedHost);
/* The same on the host, no GPU call.  walk 0: plain loops over every sphere
 * for every query of every probe (the yardstick).  walk 1: the kernel's own
 * path over the packed tables, as rtg_raytrace_host.  nthreads <= 0: 1. */
int rtg_gather_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_light* lights,
                    unsigned lgtNum, const rtg_hit* hits, size_t n,
                    const rtg_gather_params* params, const rtg_vec* dirs, const float* weights,
                    unsigned nDirs, int stackSize, int semantics, rtg_vec* outHost,
                    unsigned short* skippedHost, int walk, int nthreads);

/* ---- filter: edge-stopping a-trous filter guided by hit records ----
 * rtg_ao*'s counts, rtg_matte*'s and rtg_gather*'s colours at a few probes per
 * pixel are Monte-Carlo noise.  These calls smooth such a frame along its
 * surfaces with the edge-avoiding a-trous wavelet filter, guided by the
 * frame's own rtg_hit records (the "denoiser guides" of the G-buffer), in
 * float arithmetic that is defined here: the same words on the host and on
 * every GPU.
 *
 * INPUTS.  A W x H frame, row-major, n = W * H pixels.  `hits`: n rtg_hit
 * records exactly as rtg_intersect* writes them for the aa-1 rays of
 * rtg_camera_rays*.  Of a record, id is read for its sign and for equality
 * only (an id >= sphNum is legal), point and normal are used as given, t is
 * not read.  `src`: n values of one `kind`: RTG_FILTER_RGB rtg_vec (3
 * channels), RTG_FILTER_GRAY float, RTG_FILTER_COUNT unsigned short with value
 * (float)c, which is exact (rtg_ao*'s counts go in as they are).  `dst`:
 * rtg_vec for RGB, float for GRAY and COUNT.  The call needs no scene: the
 * context only names the device, as for rtg_views_fold_device.
 *
 * ONE PASS of step s reads image `in` (floats) and writes `out`, all in float
 * with no contraction and in this operand order; dot(a, b) = (a.x * b.x +
 * a.y * b.y) + a.z * b.z:
 *   centre p = (x, y) with id_p < 0:  out[p] = in[p]; there are no taps.
 *   otherwise  sum.q = +0.f per channel q, sw = +0.f; then for dy = -2 .. 2
 *            (outer) and dx = -2 .. 2 (inner), q = (x + dx * s, y + dy * s) in
 *            integer arithmetic that cannot wrap.  The tap is left out
 *            (nothing is added) when q is outside the frame, or id_q < 0, or
 *            RTG_FILTER_SAME_ID is set and id_q != id_p, or
 *            RTG_FILTER_SKIP_NONFINITE is set and any channel word of in[q]
 *            has an all-ones exponent field (NaN, +-inf).  Otherwise
 *              w = h[dy + 2] * h[dx + 2],  h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *                                          (every product is exact)
 *              RTG_FILTER_NORMAL:  c = dot(N_p, N_q);  c = c > 0.f ? c : 0.f
 *                                  (a NaN goes to 0); normalLog2 times c = c * c;
 *                                  w = w * c
 *              RTG_FILTER_PLANE:   e = P_q - P_p per component;
 *                                  d = fabsf(dot(N_p, e));
 *                                  z = 1.f - d * planeScale;
 *                                  z = z > 0.f ? z : 0.f;  w = w * z
 *              (a term whose flag is off is not multiplied in)
 *              if (!(w > 0.f)) the tap is left out (zero, negative, NaN)
 *              sum.q = sum.q + w * in[q].q per channel;  sw = sw + w
 *            The centre tap is a tap like any other.
 *   result   out[p].q = sw > 0.f ? sum.q / sw : in[p].q, the division the
 *            correctly rounded float quotient.
 * PASSES.  Pass i = 0 .. passes - 1 has step 1 << i.  Pass 0 reads src (COUNT
 * converted), pass i the output of pass i - 1; the guides never change.  dst
 * receives the last pass, NaN words stored as 0xFFC00000 as in every record.
 * NaN, infinite and degenerate inputs follow the arithmetic and the
 * comparisons as written.  The result depends on no scene, light, stack size
 * or semantics.
 *
 * rtg_filter_host restates this in plain loops: the yardstick.
 * rtg_filter_device is asynchronous on `stream`, allocates nothing, takes none
 * of the context's render scratch and may be mixed with every other call on
 * the context; `params` is host memory, read before the call returns.  It
 * needs a caller-owned scratch of rtg_filter_scratch's bytes (the ping-pong
 * image of passes >= 2; 0 for one pass, and then the scratch may be null):
 * at least that many bytes, 16-byte aligned, the call's until it has finished
 * on the stream.  dst holds intermediate passes before the last one lands.
 *
 * RTG_ERR_INVALID with a message, before any GPU call, for a null pointer (a
 * null scratch is legal only when 0 bytes are needed), W or H equal to 0,
 * W * H above 2^32 - 1 or (device) a grid above 2^31 - 1 workgroups, passes,
 * normalLog2 or kind out of range, an unknown flag, hits off 16-byte alignment
 * (device), a scratch that is too small or misaligned, and dst's byte range
 * overlapping src's or the scratch's (addresses compared as numbers, on the
 * host and on the device alike).  Exercised up to 16387 x 21846 pixels (11.5
 * GB of records, 4.30 GB of colours) (tests/test_gpu_large.py).
 *
 * A value- and variance-driven term is rtg_svgf*'s, below, with parameter
 * records of its own.  Out of scope: rtg_gbuf_px records as guides, per-pass
 * parameters, filtering ray batches that are not a frame, views and
 * multi-GPU. */
#define RTG_FILTER_MAX_PASSES 8
#define RTG_FILTER_RGB   0           /* kind: src and dst are rtg_vec */
#define RTG_FILTER_GRAY  1           /* kind: src and dst are float */
#define RTG_FILTER_COUNT 2           /* kind: src is unsigned short, dst is float */
#define RTG_FILTER_SAME_ID 1         /* a tap of another id is left out */
#define RTG_FILTER_NORMAL 2          /* the normal term */
#define RTG_FILTER_PLANE 4           /* the plane-distance term */
#define RTG_FILTER_SKIP_NONFINITE 8  /* a tap whose value has a NaN or infinite word is left out */
typedef struct rtg_filter_params {   /* 20 B */
  unsigned passes;      /* 1..RTG_FILTER_MAX_PASSES; pass i has step 1 << i */
  unsigned normalLog2;  /* 0..8: the clamped cosine is squared this many times */
  float planeScale;     /* used as given */
  unsigned kind;        /* RTG_FILTER_RGB / GRAY / COUNT */
  unsigned flags;       /* RTG_FILTER_* bits; an unknown bit is RTG_ERR_INVALID */
} rtg_filter_params;
/* Bytes of scratch rtg_filter_device needs for such a frame. */
int rtg_filter_scratch(unsigned width, unsigned height, const rtg_filter_params* params,
                       size_t* bytes);
/* Plain loops; the result does not depend on nthreads (threads take bands of
 * rows of one pass).  nthreads <= 0: 1. */
int rtg_filter_host(const rtg_hit* hits, unsigned width, unsigned height,
                    const rtg_filter_params* params, const void* src, void* dstHost,
                    int nthreads);
int rtg_filter_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                      unsigned height, const rtg_filter_params* params, const void* srcDevice,
                      void* dstDevice, void* scratchDevice, size_t scratchBytes, void* stream);
/* One-shot: uploads the hits and src, allocates its own scratch, runs on
 * `device`, downloads n values. */
int rtg_filter(int device, const rtg_hit* hits, unsigned width, unsigned height,
               const rtg_filter_params* params, const void* src, void* dstHost);

/* ---- accumulate: temporal accumulation by reprojection ----
 * rtg_ao* and rtg_gather* give a different probe set per frame under their
 * JITTER flags and a seed; rtg_filter* smooths one frame in space.  These calls
 * are the time half: they carry a per-pixel running mean from frame to frame
 * while the camera moves.  Scenes are static, so the world-space hit point of
 * a pixel is the exact key into the previous frame: it is projected into the
 * previous pose (rtg_camera_project*'s arithmetic) and the previous state is
 * fetched there with four validated bilinear taps.  Float arithmetic that is
 * defined here: the same words on the host and on every GPU.
 *
 * INPUTS.  A W x H frame, row-major, n = W * H pixels.  `hits`: the current
 * pose's aa-1 rtg_hit records, read as rtg_filter* reads them (id for its sign
 * and for equality, point and normal as given, t not read).  `src`: the current
 * signal, one of rtg_filter*'s kinds (RTG_FILTER_RGB rtg_vec, RTG_FILTER_GRAY
 * float, RTG_FILTER_COUNT unsigned short with value (float)c); C = 3 channels
 * for RGB, else 1.  The previous frame's state: `prevHits` (its records),
 * `prevAcc` (n * C floats, its outAcc), `prevLen` (n unsigned short, its
 * outLen, the history length), optionally `prevM2` (n * C floats, its outM2),
 * and the previous pose `prevCam` with the frame's `zoom`.  Outputs: outAcc
 * (n * C floats), outLen (n unsigned short) and optionally outM2 (n * C
 * floats), a running mean of the squared signal.
 * prevHits, prevAcc and prevLen are all null or all non-null.  All null is a
 * RESET FRAME: no pixel finds history, prevCam and prevM2 are not read and
 * may be null.  Otherwise prevM2 follows outM2: both null or both non-null.
 *
 * PER PIXEL p = (x, y), all in float with no contraction and in this operand
 * order, dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z, q over the channels:
 *   cur.q = src[p].q (converted);  cur2.q = cur.q * cur.q
 *   id_p < 0:  outAcc[p] = cur, outM2[p] = cur2, outLen[p] = 0; nothing else.
 *   LOOKUP.  {fx, fy, k} = rtg_camera_project's of P_p under prevCam, W, H,
 *     zoom.  There is no history on a reset frame, or when !(k > 0.f), or when
 *     !(fx > -1.f && fx < (float)W && fy > -1.f && fy < (float)H).  Otherwise
 *     x0 = floorf(fx), tx = fx - x0, y0 = floorf(fy), ty = fy - y0 (x0, y0
 *     then convert to int exactly); sum.q = s2.q = sw = +0.f, nmin = 65535;
 *     taps dy = 0, 1 (outer), dx = 0, 1 (inner): q = (x0 + dx, y0 + dy),
 *     wx = dx ? tx : 1.f - tx, wy = dy ? ty : 1.f - ty, w = wy * wx.  The tap
 *     is left out when q is outside the frame, or prevId_q < 0, or
 *     prevLen_q == 0, or RTG_ACCUM_SAME_ID is set and prevId_q != id_p, or
 *     RTG_ACCUM_SKIP_NONFINITE is set and any word of prevAcc[q] has an
 *     all-ones exponent field.  Then rtg_filter*'s two terms, verbatim:
 *       RTG_ACCUM_NORMAL:  c = dot(N_p, prevN_q);  c = c > 0.f ? c : 0.f;
 *                          normalLog2 times c = c * c;  w = w * c
 *       RTG_ACCUM_PLANE:   e = prevP_q - P_p per component;
 *                          d = fabsf(dot(N_p, e));  z = 1.f - d * planeScale;
 *                          z = z > 0.f ? z : 0.f;  w = w * z
 *     and the tap is left out when !(w > 0.f).  An accepted tap gives
 *       sum.q = sum.q + w * prevAcc[q].q;  s2.q = s2.q + w * prevM2[q].q;
 *       sw = sw + w;  nmin = min(nmin, prevLen_q)
 *     The lookup is FOUND when sw > 0.f; then hist.q = sum.q / sw and
 *     hist2.q = s2.q / sw, the correctly rounded quotients.
 *   BLEND.  curOK is false only when RTG_ACCUM_SKIP_NONFINITE is set and a
 *     word of cur has an all-ones exponent field.
 *       found,  curOK:  n = min(nmin + 1, maxHistory), alpha = 1.f / (float)n,
 *                       outAcc.q = hist.q + alpha * (cur.q - hist.q), outLen = n
 *       found, !curOK:  outAcc.q = hist.q, outLen = nmin
 *       !found, curOK:  outAcc.q = cur.q,  outLen = 1
 *       !found, !curOK: outAcc.q = cur.q,  outLen = 0
 *     outM2 follows outAcc's pattern with cur2 and hist2.
 * NaN words are stored as 0xFFC00000.  NaN poses, points and normals follow
 * the comparisons as written.  With maxHistory = 65535 outAcc is the running
 * mean of the pixel's surface point over the frames it was seen in; a smaller
 * maxHistory is an exponential average with alpha >= 1 / maxHistory.
 *
 * rtg_accumulate_host restates this in plain loops: the yardstick.
 * rtg_accumulate_device is one kernel launch, asynchronous on `stream`; it
 * allocates nothing, needs no scratch and no scene, takes none of the
 * context's render scratch and may be mixed with every other call on the
 * context.  `params` and `prevCam` are host memory, read before return.
 *
 * RTG_ERR_INVALID with a message, before any GPU call, for a null hits, src,
 * params, outAcc or outLen, a partly null prev set, a null prevCam with a prev
 * set, outM2 without prevM2 with a prev set or prevM2 without outM2, W or H
 * equal to 0 or above 2^24, normalLog2 above 8, an unknown kind or flag,
 * maxHistory 0 or above 65535, hits or prevHits off 16-byte alignment
 * (device), a grid above 2^31 - 1 workgroups (device), and any output's byte
 * range overlapping any input's or another output's: the kernel gathers from
 * the previous state, so in-place use is a race (addresses compared as
 * numbers, on the host and on the device alike).
 *
 * outM2 is what rtg_variance* reads, below.  Out of scope: moving spheres and
 * motion vectors, per-pixel alpha clamps, views and multi-GPU. */
#define RTG_ACCUM_SAME_ID 1         /* a tap of another id is left out */
#define RTG_ACCUM_NORMAL 2          /* the normal term */
#define RTG_ACCUM_PLANE 4           /* the plane-distance term */
#define RTG_ACCUM_SKIP_NONFINITE 8  /* non-finite history taps and current values are left out */
typedef struct rtg_accumulate_params { /* 20 B */
  unsigned kind;        /* RTG_FILTER_RGB / GRAY / COUNT */
  unsigned flags;       /* RTG_ACCUM_* bits; an unknown bit is RTG_ERR_INVALID */
  unsigned normalLog2;  /* 0..8 */
  float planeScale;     /* used as given */
  unsigned maxHistory;  /* 1..65535: outLen's cap */
} rtg_accumulate_params;
/* Plain loops; the result does not depend on nthreads (threads take bands of
 * rows).  nthreads <= 0: 1. */
int rtg_accumulate_host(const rtg_hit* hits, unsigned width, unsigned height,
                        const rtg_accumulate_params* params, const void* src,
                        const rtg_camera* prevCam, float zoom, const rtg_hit* prevHits,
                        const float* prevAcc, const unsigned short* prevLen, const float* prevM2,
                        float* outAcc, unsigned short* outLen, float* outM2, int nthreads);
int rtg_accumulate_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                          unsigned height, const rtg_accumulate_params* params,
                          const void* srcDevice, const rtg_camera* prevCam, float zoom,
                          const rtg_hit* prevHitsDevice, const float* prevAccDevice,
                          const unsigned short* prevLenDevice, const float* prevM2Device,
                          float* outAccDevice, unsigned short* outLenDevice, float* outM2Device,
                          void* stream);
/* One-shot: uploads the inputs (host memory), runs on `device`, downloads the
 * outputs. */
int rtg_accumulate(int device, const rtg_hit* hits, unsigned width, unsigned height,
                   const rtg_accumulate_params* params, const void* src,
                   const rtg_camera* prevCam, float zoom, const rtg_hit* prevHits,
                   const float* prevAcc, const unsigned short* prevLen, const float* prevM2,
                   float* outAcc, unsigned short* outLen, float* outM2);

/* ---- variance and svgf: the variance-guided a-trous filter ----
 * rtg_filter* stops at geometric edges: id, normal and plane.  The signals it
 * is meant for have their edges inside one sphere: contact shadows, shadow
 * boundaries, indirect light.  These calls are the stage SVGF adds:
 * rtg_variance* turns rtg_accumulate*'s moments into one variance per pixel,
 * and rtg_svgf* runs the filter's passes with one more edge-stopping term, on
 * the signal itself and scaled by the local standard deviation, carrying the
 * variance from pass to pass so that the term tightens as the noise goes down.
 * The chain is rtg_ao* / rtg_gather* -> rtg_accumulate* (with outM2) ->
 * rtg_variance* -> rtg_svgf*.  Float arithmetic that is defined here: the same
 * words on the host and on every GPU.  Frames, records, kinds, the tap rule's
 * bits and dot(a, b) are rtg_filter*'s; C = 3 channels for RTG_FILTER_RGB, 1
 * for RTG_FILTER_GRAY; RTG_FILTER_COUNT is RTG_ERR_INVALID here (the states
 * are floats).  lum(v) = v for GRAY and (0.2126f * v.r + 0.7152f * v.g) +
 * 0.0722f * v.b for RGB.
 *
 * VARIANCE.  `hits`: n records; `acc`, `m2`: n * C floats each,
 * rtg_accumulate*'s outAcc and outM2; `len`: n unsigned short, its outLen.
 * Output `var`: n floats.  Per pixel p:
 *   id_p < 0:  var[p] = +0.f.
 *   len_p >= minHistory:  m = acc[p], e = m2[p] (the temporal estimate).
 *   otherwise the spatial estimate: s1.q = s2.q = sw = +0.f; for dy = -3 .. 3
 *     (outer), dx = -3 .. 3 (inner), q = (x + dx, y + dy).  The tap is left out
 *     when q is outside the frame, or id_q < 0, or SAME_ID is set and id_q !=
 *     id_p, or SKIP_NONFINITE is set and any word of acc[q] or m2[q] has an
 *     all-ones exponent field.  w = 1.f times rtg_filter*'s NORMAL and PLANE
 *     terms, verbatim; the tap is left out when !(w > 0.f).  Otherwise
 *       s1.q = s1.q + w * acc[q].q;  s2.q = s2.q + w * m2[q].q;  sw = sw + w
 *     and then m.q = s1.q / sw, e.q = s2.q / sw if sw > 0.f, else m = acc[p],
 *     e = m2[p].
 *   d.q = e.q - m.q * m.q;  d.q = d.q > 0.f ? d.q : 0.f (a NaN goes to 0);
 *   var[p] = lum(d): for RGB a luminance-weighted mean of the channel
 *   variances (the second moment is per channel, so the variance of the
 *   luminance cannot be had).  NaN words are stored as 0xFFC00000.
 *
 * SVGF, ONE PASS of step s reads `in` (n * C floats) and `vin` (n floats) and
 * writes `out` and `vout`:
 *   id_p < 0:  out[p] = in[p], vout[p] = vin[p]; there are no taps.
 *   RTG_SVGF_LUMA only, the prefiltered variance at the centre: gs = gw =
 *     +0.f; for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = (x + dx,
 *     y + dy), always at step 1, kw = k[dy + 1] * k[dx + 1], k = {1/4, 1/2,
 *     1/4}.  The tap is left out when q is outside the frame, or id_q < 0, or
 *     SAME_ID is set and id_q != id_p, or SKIP_NONFINITE is set and vin[q] has
 *     an all-ones exponent field.  Otherwise gs = gs + kw * vin[q], gw = gw +
 *     kw.  Then g = gw > 0.f ? gs / gw : vin[p];  den = sigmaL * sqrtf(g) +
 *     epsL;  ls = 1.f / den, sqrtf and the quotient correctly rounded;
 *     lp = lum(in[p]).
 *   The 25 taps in rtg_filter*'s order and under its rule; SKIP_NONFINITE also
 *     leaves a tap out when vin[q] has an all-ones exponent field.  w is
 *     rtg_filter*'s weight; with LUMA then
 *       l = fabsf(lum(in[q]) - lp);  z = 1.f - l * ls;  z = z > 0.f ? z : 0.f;
 *       w = w * z
 *     and the tap is left out when !(w > 0.f).  Otherwise
 *       sum.q = sum.q + w * in[q].q;  sv = sv + (w * w) * vin[q];  sw = sw + w
 *   result   sw > 0.f:  out[p].q = sum.q / sw, vout[p] = sv / (sw * sw);
 *            otherwise  out[p] = in[p], vout[p] = vin[p].
 * The luminance falloff is the plane term's clamped line, not SVGF's exp:
 * there is no expf whose float words the host, numpy and the GPU share, and the
 * same words everywhere is the contract.  Pass i = 0 .. passes - 1 has step
 * 1 << i; pass 0 reads src and varSrc; dst and dstVar (required) receive the
 * last pass, NaN words stored as 0xFFC00000.  NaN and infinite inputs follow
 * the arithmetic and the comparisons as written.  With LUMA off and every
 * vin finite the values are rtg_filter*'s.
 *
 * The _host forms restate this in plain loops: the yardstick.  The _device
 * forms are asynchronous on `stream`, allocate nothing, need no scene and
 * may be mixed with every other call on the context; `params` is host memory,
 * read before return.  rtg_svgf_device needs a caller-owned scratch of
 * rtg_svgf_scratch's bytes (a ping-pong value image and variance image, each
 * rounded up to 16 bytes; 0 for one pass, and then the scratch may be null),
 * 16-byte aligned, the call's until it has finished on the stream.
 *
 * RTG_ERR_INVALID with a message, before any GPU call, for a null pointer
 * (varSrc and dstVar included), W or H equal to 0, W * H above 2^32 - 1 or
 * (device) a grid above 2^31 - 1 workgroups, passes, normalLog2, minHistory or
 * kind out of range, COUNT as the kind, an unknown flag, hits off 16-byte
 * alignment (device), a scratch that is too small or misaligned, and any
 * written byte range (var; dst, dstVar, the scratch) overlapping another of
 * the call's value buffers (addresses compared as numbers).  Both exercised
 * up to 16387 x 8192 pixels (4.30 GB of records) (tests/test_gpu_large.py).
 *
 * Out of scope: fusing the variance estimate into pass 0, feeding the first
 * pass back as history, per-pass parameters, moving spheres, views and
 * multi-GPU. */
typedef struct rtg_variance_params { /* 20 B */
  unsigned kind;        /* RTG_FILTER_RGB or RTG_FILTER_GRAY; COUNT is RTG_ERR_INVALID (states are floats) */
  unsigned flags;       /* RTG_FILTER_SAME_ID | NORMAL | PLANE | SKIP_NONFINITE: the window's tap rule */
  unsigned normalLog2;  /* 0..8 */
  float planeScale;     /* used as given */
  unsigned minHistory;  /* 0..65535: a hit pixel with len < minHistory takes the spatial estimate; 0: none does */
} rtg_variance_params;
/* Plain loops; the result does not depend on nthreads.  nthreads <= 0: 1. */
int rtg_variance_host(const rtg_hit* hits, unsigned width, unsigned height,
                      const rtg_variance_params* params, const float* acc, const float* m2,
                      const unsigned short* len, float* varHost, int nthreads);
int rtg_variance_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                        unsigned height, const rtg_variance_params* params, const float* accDevice,
                        const float* m2Device, const unsigned short* lenDevice, float* varDevice,
                        void* stream);
/* One-shot: uploads the inputs, runs on `device`, downloads n floats. */
int rtg_variance(int device, const rtg_hit* hits, unsigned width, unsigned height,
                 const rtg_variance_params* params, const float* acc, const float* m2,
                 const unsigned short* len, float* varHost);

#define RTG_SVGF_LUMA 16   /* next to the filter's four bits, which keep their meaning */
typedef struct rtg_svgf_params { /* 28 B */
  unsigned passes;      /* 1..RTG_FILTER_MAX_PASSES; pass i has step 1 << i */
  unsigned normalLog2;  /* 0..8 */
  float planeScale;     /* used as given */
  unsigned kind;        /* RTG_FILTER_RGB or RTG_FILTER_GRAY; COUNT is RTG_ERR_INVALID */
  unsigned flags;       /* the filter's bits | RTG_SVGF_LUMA */
  float sigmaL;         /* used as given */
  float epsL;           /* used as given */
} rtg_svgf_params;
/* Bytes of scratch rtg_svgf_device needs for such a frame. */
int rtg_svgf_scratch(unsigned width, unsigned height, const rtg_svgf_params* params,
                     size_t* bytes);
/* Plain loops; the result does not depend on nthreads.  nthreads <= 0: 1. */
int rtg_svgf_host(const rtg_hit* hits, unsigned width, unsigned height,
                  const rtg_svgf_params* params, const float* src, const float* varSrc,
                  float* dstHost, float* dstVarHost, int nthreads);
int rtg_svgf_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width, unsigned height,
                    const rtg_svgf_params* params, const float* srcDevice,
                    const float* varSrcDevice, float* dstDevice, float* dstVarDevice,
                    void* scratchDevice, size_t scratchBytes, void* stream);
/* One-shot: uploads the hits, src and varSrc, allocates its own scratch, runs
 * on `device`, downloads dst and dstVar. */
int rtg_svgf(int device, const rtg_hit* hits, unsigned width, unsigned height,
             const rtg_svgf_params* params, const float* src, const float* varSrc, float* dstHost,
             float* dstVarHost);

/* ---- upsample: a low-resolution signal brought up by full-resolution guides ----
 * The per-pixel signals above cost what their probes cost; everything after
 * them is cheap.  These calls let a caller trace the signal on a coarser frame
 * of the same pose and zoom, bring it up to the full frame with the full
 * frame's own records as guides, and learn which pixels no coarse tap agrees
 * with: the HOLE LIST, on which the signal is then run at full resolution
 * (rtg_hits_pick*, the signal's own call, rtg_values_place*, below).  Float
 * arithmetic that is defined here: the same words on the host and on every GPU.
 *
 * THE TWO FRAMES.  scaleLog2 = L in 1..3, f = 1 << L.  The full frame is W x H,
 * the low frame Wl x Hl with W == Wl << L and H == Hl << L.  The aa-1 sample of
 * pixel x of a W-wide frame leaves the eye at (x - W/2) * (16/W) (main.cpp:
 * 411-413 with sample (0, 0) of :432-433, camera_dir): no half-pixel offset.
 * (X - Wl/2) is (f X - W/2) / f and 16/Wl is f * (16/W), both exactly, so low
 * pixel (X, Y) is the ray of full pixel (f X, f Y), bit for bit, and its record
 * is that pixel's record.  A full pixel x lies between low columns x >> L and
 * (x >> L) + 1 at the fraction (x mod f) / f, which is exact in float, as is
 * every product of two such fractions.
 *
 * INPUTS.  `hits`: W * H full-resolution rtg_hit records, `lowHits`: Wl * Hl
 * records of the low frame, both read as rtg_filter* reads them (id for its
 * sign and for equality, point and normal as given, t not read).  `lowSrc`:
 * Wl * Hl values of one of rtg_filter*'s kinds (RTG_FILTER_RGB rtg_vec,
 * RTG_FILTER_GRAY float, RTG_FILTER_COUNT unsigned short with value (float)c);
 * C = 3 channels for RGB, else 1.  `dst`: W * H * C floats.  The call needs no
 * scene.
 *
 * PER FULL PIXEL p = (x, y), all in float with no contraction and in this
 * operand order, dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z, q over the
 * channels:
 *   id_p < 0:  dst[p].q = +0.f; the pixel is no hole and nothing else is read.
 *   otherwise  x0 = x >> L, tx = (float)(x & (f - 1)) * (1.f / f); y0 = y >> L,
 *     ty = (float)(y & (f - 1)) * (1.f / f); sum.q = sw = +0.f;
 *     taps dy = 0, 1 (outer), dx = 0, 1 (inner): q = (x0 + dx, y0 + dy),
 *     wx = dx ? tx : 1.f - tx, wy = dy ? ty : 1.f - ty, w = wy * wx.  The tap
 *     is left out when q is outside the low frame, or lowId_q < 0, or
 *     RTG_UPSAMPLE_SAME_ID is set and lowId_q != id_p, or
 *     RTG_UPSAMPLE_SKIP_NONFINITE is set and any word of lowSrc[q] has an
 *     all-ones exponent field.  Then rtg_filter*'s two terms, verbatim:
 *       RTG_UPSAMPLE_NORMAL:  c = dot(N_p, lowN_q);  c = c > 0.f ? c : 0.f;
 *                             normalLog2 times c = c * c;  w = w * c
 *       RTG_UPSAMPLE_PLANE:   e = lowP_q - P_p per component;
 *                             d = fabsf(dot(N_p, e));  z = 1.f - d * planeScale;
 *                             z = z > 0.f ? z : 0.f;  w = w * z
 *     and the tap is left out when !(w > 0.f), which also drops the taps whose
 *     bilinear weight is zero (tx == 0.f or ty == 0.f).  An accepted tap gives
 *       sum.q = sum.q + w * lowSrc[q].q;  sw = sw + w
 *   sw > 0.f:  dst[p].q = sum.q / sw, the correctly rounded quotient.
 *   otherwise  the pixel is a HOLE: dst[p].q = +0.f, and the pixel is listed.
 * NaN words are stored as 0xFFC00000.  NaN points, normals and values follow
 * the comparisons as written.
 *
 * THE HOLE LIST is optional: `holes` (unsigned, capacity holeCap) and
 * `holeCount` (one unsigned) are both null or both non-null.  holeCount
 * receives the number of holes of the frame, also when it exceeds holeCap;
 * holes[0 .. min(count, holeCap)) receive the holes' pixel indices y * W + x in
 * ascending order, and no entry past that is written.  The order is part of
 * the contract: two runs and the host form give the same words.
 *
 * rtg_upsample_host restates this in plain loops: the yardstick.
 * rtg_upsample_device is asynchronous on `stream`, allocates nothing, needs no
 * scene, takes none of the context's render scratch and may be mixed with
 * every other call on the context; `params` is host memory, read before
 * return.  Without a hole list it is one launch and needs no scratch
 * (rtg_upsample_scratch gives 0, and the scratch may be null).  With one it
 * is three launches (the pixels, a scan over the workgroups' hole counts, the
 * list's entries) and needs a caller-owned scratch of rtg_upsample_scratch's
 * bytes, 16-byte aligned, the call's until it has finished on the stream.  No
 * kernel waits for another workgroup of its own launch.
 *
 * RTG_ERR_INVALID with a message, before any GPU call, for a null pointer (a
 * null scratch is legal only when 0 bytes are needed), W, H, Wl or Hl equal to
 * 0, W != Wl << L or H != Hl << L, L outside 1..3, W or H above 2^24, W * H
 * above 2^32 - 1 (which also keeps the grid below 2^31 workgroups),
 * normalLog2 above 8, an unknown kind or flag, holes without holeCount or the
 * reverse, hits or lowHits off 16-byte alignment (device), a scratch that is
 * too small or misaligned, and any output's byte range (dst, holes, holeCount,
 * the scratch) overlapping an input's or another output's (addresses compared
 * as numbers, on the host and on the device alike).
 *
 * rtg_hits_pick*: out[i] = hits[idx[i]] for i < m, the 32 bytes as they are;
 * an index >= n gives a miss record (id -1, every other word 0) and reads
 * nothing.  rtg_values_place*: dst[idx[i]] = vals[i] for i < m, `vals` m values
 * of `kind` and `dst` n * C floats, converted as rtg_filter* converts (COUNT to
 * float, float words as they are); an index >= n is skipped.  The indices are
 * taken as DISTINCT, as a hole list's are: with a repeated index any one of
 * its values lands.  `m` is a host value: the caller reads holeCount back, one
 * 4-byte copy.  m == 0 is legal and does nothing.  RTG_ERR_INVALID for a null
 * pointer, n == 0, an unknown kind, hits or out off 16-byte alignment
 * (device), more than 2^31 - 1 workgroups (device), and an output's byte range
 * overlapping an input's.
 *
 * Out of scope: factors that are no power of two and frames not divisible by
 * f, upsampling moments or history lengths (accumulate at full resolution
 * after the upsample), checkerboard or adaptive sample placement, rtg_gbuf_px
 * guides, views and multi-GPU. */
#define RTG_UPSAMPLE_MAX_SCALE_LOG2 3
#define RTG_UPSAMPLE_SAME_ID 1         /* a tap of another id is left out */
#define RTG_UPSAMPLE_NORMAL 2          /* the normal term */
#define RTG_UPSAMPLE_PLANE 4           /* the plane-distance term */
#define RTG_UPSAMPLE_SKIP_NONFINITE 8  /* a tap whose value has a NaN or infinite word is left out */
typedef struct rtg_upsample_params { /* 20 B */
  unsigned kind;        /* RTG_FILTER_RGB / GRAY / COUNT */
  unsigned flags;       /* RTG_UPSAMPLE_* bits; an unknown bit is RTG_ERR_INVALID */
  unsigned normalLog2;  /* 0..8 */
  float planeScale;     /* used as given */
  unsigned scaleLog2;   /* 1..RTG_UPSAMPLE_MAX_SCALE_LOG2 */
} rtg_upsample_params;
/* Bytes of scratch rtg_upsample_device needs for such a full frame: 0 when
 * withHoles is 0. */
int rtg_upsample_scratch(unsigned width, unsigned height, int withHoles, size_t* bytes);
/* Plain loops; the result does not depend on nthreads (threads take bands of
 * rows; the list is written in order afterwards).  nthreads <= 0: 1. */
int rtg_upsample_host(const rtg_hit* hits, unsigned width, unsigned height,
                      const rtg_upsample_params* params, const rtg_hit* lowHits,
                      unsigned lowWidth, unsigned lowHeight, const void* lowSrc, float* dst,
                      unsigned* holes, unsigned holeCap, unsigned* holeCount, int nthreads);
int rtg_upsample_device(rtg_context* ctx, const rtg_hit* hitsDevice, unsigned width,
                        unsigned height, const rtg_upsample_params* params,
                        const rtg_hit* lowHitsDevice, unsigned lowWidth, unsigned lowHeight,
                        const void* lowSrcDevice, float* dstDevice, unsigned* holesDevice,
                        unsigned holeCap, unsigned* holeCountDevice, void* scratchDevice,
                        size_t scratchBytes, void* stream);
/* One-shot: uploads the inputs (host memory), allocates its own scratch, runs
 * on `device`, downloads dst and, with a list, holeCount and holeCap entries
 * (the entries past min(count, holeCap) are the caller's own words). */
int rtg_upsample(int device, const rtg_hit* hits, unsigned width, unsigned height,
                 const rtg_upsample_params* params, const rtg_hit* lowHits, unsigned lowWidth,
                 unsigned lowHeight, const void* lowSrc, float* dstHost, unsigned* holesHost,
                 unsigned holeCap, unsigned* holeCountHost);
int rtg_hits_pick_host(const rtg_hit* hits, size_t n, const unsigned* idx, size_t m,
                       rtg_hit* outHost, int nthreads);
int rtg_hits_pick_device(rtg_context* ctx, const rtg_hit* hitsDevice, size_t n,
                         const unsigned* idxDevice, size_t m, rtg_hit* outDevice, void* stream);
int rtg_values_place_host(unsigned kind, const void* vals, const unsigned* idx, size_t m, size_t n,
                          float* dstHost, int nthreads);
int rtg_values_place_device(rtg_context* ctx, unsigned kind, const void* valsDevice,
                            const unsigned* idxDevice, size_t m, size_t n, float* dstDevice,
                            void* stream);

/* ---- containment: primaryContainer per point ----
 * "Which medium is this point in": out[i] is the lowest sphere index s for
 * which, all in float (primaryContainer, raytracer.h:245-270),
 *   r = radius_s + 1e-6f;  d = p - c_s;  (d.x * d.x + d.y * d.y) + d.z * d.z <= r * r
 * holds for point p = points[i], or -1.  A NaN coordinate gives -1.  It is the
 * refraction target rayTrace looks up for its test point P + 0.01 d.
 * The checks are rtg_matte's, with a null point buffer in place of the hits. */
int rtg_contains_device(rtg_context* ctx, const rtg_vec* pointsDevice, size_t n, int* outDevice,
                        void* stream);
int rtg_contains(int device, const rtg_sphere* spheres, unsigned sphNum, const rtg_vec* points,
                 size_t n, int* outHost);
/* walk 0: the literal loop over the caller's array.  walk 1: the kernel's
 * path (four containment records per step, or the BVH). */
int rtg_contains_host(const rtg_sphere* spheres, unsigned sphNum, const rtg_vec* points, size_t n,
                      int* outHost, int walk, int nthreads);

/* Semantics of a context's renders.  RTG_SEMANTICS_CPU (default) is the
 * reference CPU path (raytracer.h), bit for bit.  RTG_SEMANTICS_OPENCL is the
 * reference's OpenCL kernel (raytrace_kernel.cl:641-867) under IEEE binary32:
 * f32 Fresnel (:399-432) and sinA1 (:507), the return register zeroed by the
 * reflection push (:835-845); pass stackSize 5 for the .cl's RTSTACK_MAXSIZE
 * (:58).  That kernel ran under OpenCL's relaxed division/sqrt, so its own
 * output (testPPM.ppm) is only approached, not reproduced bit for bit. */
#define RTG_SEMANTICS_CPU 0
#define RTG_SEMANTICS_OPENCL 1
int rtg_context_set_semantics(rtg_context* ctx, int semantics);

/* Launch-configuration knobs (performance only; results never change). */
typedef struct rtg_launch_opts {
  int variant;        /* 0 = default kernel; 9 tile kernel; 100, 110, 120 diagnostic builds */
  int flags;          /* RTG_LAUNCH_* bits */
  int reserved[6];
} rtg_launch_opts;
int rtg_set_launch_opts(rtg_context* ctx, const rtg_launch_opts* opts);
/* Diagnostic variants (variant >= 100) sum per-wave s_memtime cycles spent in
 * {closest-hit queries, shadow queries, refraction, whole pixel} into 8
 * counters; read (and optionally zero) them.  Zeros for normal variants. */
int rtg_diag_read(rtg_context* ctx, unsigned long long* out8, int reset);
/* Executed-work counters of the counting build (variant 120: the default
 * kernel's control flow with per-unit counters): out[0 .. n/2)
 * wave-level executions of each unit (rtg_trace.h kCnt* / kU* slots), out[n/2
 * .. n) lane-level sums.  Copies min(cap, n) values, optionally zeroes them,
 * and returns n (cap <= 0: just returns n); negative on error. */
int rtg_diag_counts(rtg_context* ctx, unsigned long long* out, int cap, int reset);
/* Diagnostic, no GPU: *ranged = 1 when the scene passes the value-range proof
 * under which renders of scenes with sphere masks run the kernel compiled
 * without its rare-path guards (every refractive index finite, with
 * 2^-96 <= |n| <= 2^96), else 0 (such a scene renders through the guarded
 * kernel; the frame is the same either way). */
int rtg_scene_ranged(const rtg_sphere* spheres, unsigned sphNum, int* ranged);
#define RTG_LAUNCH_TIMELINE 1 /* record a per-wave timeline (rtg_diag_timeline) */
/* Compacted launches list pixel groups heaviest first, by the trace times the
 * previous launch of the same frame geometry measured (launch-order feedback:
 * a scheduling hint, the frame is the same either way).  This flag lists them
 * by primary-ray sphere count only (also env RTG_LAUNCH_ORDER=popcount). */
#define RTG_LAUNCH_NO_ORDER_FEEDBACK 2
/* Wave timeline of the last launch made with RTG_LAUNCH_TIMELINE: one record
 * per wave {start, end (s_memrealtime, 100 MHz, low 32 bits), HW_ID, XCC_ID | tag << 4}
 * (tag: the popcount of the wave's first group's sphere mask, 7 bits, then the
 * group's index, 21 bits; compacted launches only),
 * in launch order.  Copies min(cap, waves) records; *count = waves recorded.
 * Diagnostic only (occupancy analysis, tools/timeline.py). */
int rtg_diag_timeline(rtg_context* ctx, unsigned* out4, size_t cap, size_t* count);
/* The last compacted launch's pixel-group list (diagnostic; launch-order
 * studies, tools/cost_study.py): *groups = its pixel groups; cost[g] (cap
 * entries at most) the trace time of group g in s_memrealtime ticks (100 MHz)
 * as its cost table holds it (0 when the launch had none; a group not listed
 * keeps a stale value), list / sel (min(cap, groups) entries each) the listed
 * group indices and sphere masks in the order the trace kernel's waves take
 * them (runs[0] + ... + runs[3] entries), runs[4] the four run lengths summed
 * over the list's partitions.  Any output pointer may be null.
 * RTG_ERR_INVALID when the context has made no compacted launch. */
int rtg_diag_group_list(rtg_context* ctx, unsigned* cost, unsigned* list,
                        unsigned long long* sel, unsigned* runs, size_t cap, size_t* groups);

/* ---- output side ---- */
/* algebra.h:68-91 on the host. */
float rtg_max_colour(const rtg_vec* pixels, size_t n);
/* Same reduction on the device into *maxDevice (one float), on `stream`. */
int rtg_max_colour_device(rtg_context* ctx, const rtg_vec* pixelsDevice, size_t n,
                          float* maxDevice, void* stream);
/* main.cpp:66-81: 3 bytes per pixel, (unsigned char)(min(1,c)*255/max) with the
 * x86 truncating conversion (low byte of a 32-bit cvttss2si). */
void rtg_ppm_bytes(const rtg_vec* pixels, size_t n, float maxColourVal,
                   unsigned char* out);
/* Device version: reads *maxDevice, writes n*3 bytes to outDevice. */
int rtg_ppm_bytes_device(rtg_context* ctx, const rtg_vec* pixelsDevice, size_t n,
                         const float* maxDevice, unsigned char* outDevice, void* stream);
/* main.cpp:43-91: binary P6 writer. */
int rtg_save_ppm(const rtg_vec* pixels, const char* filename, int width, int height,
                 float maxColourVal);

/* ---- scene construction helpers (main.cpp:53-74, 113-168) ---- */
/* setMatOpacity + setMatteGlossBalance + setMatRefractivityIndex. */
void rtg_make_material(float opacity, float glossFactor, const rtg_vec* matte,
                       const rtg_vec* gloss, float refractiveIndex, rtg_material* out);
/* The reference's hard-coded 3-sphere / 2-light scene (main.cpp:104-168) when
 * sphNum<=3 && lgtNum<=2, extended by the seeded generator of SURVEY.md §8d.
 * seed 42 is the benchmark scene. */
int rtg_scene_generate(unsigned long long seed, unsigned sphNum, unsigned lgtNum,
                       rtg_sphere* spheres, rtg_light* lights);

/* ---- scene files (the reference hard-codes main.cpp:104-168) ----
 * Text format, one record per line ('#' starts a comment):
 *   material NAME opacity glossFactor mr mg mb gr gg gb refractiveIndex
 *   sphere x y z radius NAME
 *   sphere_raw x y z radius mr mg mb gr gg gb opacity refractiveIndex
 *   light x y z r g b
 * `material` builds the record with rtg_make_material (the reference's
 * setters).  Loads up to sphCap / lgtCap records and sets *sphNum / *lgtNum
 * to the file's totals (call with capacity 0 to size the arrays).  Errors
 * name the file and line.  rtg_scene_save writes sphere_raw / light records
 * that load back bit for bit. */
int rtg_scene_load(const char* path, rtg_sphere* spheres, unsigned sphCap, unsigned* sphNum,
                   rtg_light* lights, unsigned lgtCap, unsigned* lgtNum);
int rtg_scene_save(const char* path, const rtg_sphere* spheres, unsigned sphNum,
                   const rtg_light* lights, unsigned lgtNum);

#ifdef __cplusplus
}
#endif
#endif /* RTG_H */
