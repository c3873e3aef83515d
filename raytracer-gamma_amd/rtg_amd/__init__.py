"""rtg_amd — ctypes binding of librtg.so, the MI355X raytracer-gamma hot path.

This is the binding a Python maintainer would add over the C ABI in
include/rtg.h (INTEGRATION.md shows the C/C++ and ctypes forms).  It mirrors
the reference's host interface for the path:

  reference                                   here
  ------------------------------------------  ------------------------------------
  struct Sphere / Light / Material (C)        SPHERE_DTYPE / LIGHT_DTYPE / MATERIAL_DTYPE
  setMatOpacity+setMatteGlossBalance+...      make_material()   (raytracer.h:53-74)
  scene of main.cpp:104-168                   generate_scene()  (+ SURVEY §8d generator)
  OpenCL raytrace kernel + enqueue/readback   render() / Context.render_device()
    (raytrace_kernel.cl:870, main.cpp:277-468)
  maxColourValuePixelBuffer (algebra.h:68)    max_colour_value()
  savePPM (main.cpp:43-91)                    save_ppm() / ppm_bytes()

There is no CPU fallback: every render call goes to the HIP kernel and raises
RtgError when the library or a GPU is missing.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

# torch (when present) must own the HIP runtime of this process: librtg.so's
# libamdhip64.so.7 dependency then resolves to the runtime torch already
# loaded, so torch streams / pointers and ours are the same runtime's.
try:  # pragma: no cover - import side effect only
    import torch  # noqa: F401
except Exception:  # torch absent: librtg loads /opt/rocm's runtime itself
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTG_LIB: an alternative build of the same library (compiler-flag A/B runs).
LIB_PATH = os.environ.get("RTG_LIB") or os.path.join(os.path.dirname(_HERE), "librtg.so")

VEC_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
MATERIAL_DTYPE = np.dtype([("matteColour", "<f4", 3), ("glossColour", "<f4", 3),
                           ("opacity", "<f4"), ("refractiveIndex", "<f4")])
SPHERE_DTYPE = np.dtype([("pos", "<f4", 3), ("radius", "<f4"), ("material", MATERIAL_DTYPE)])
LIGHT_DTYPE = np.dtype([("pos", "<f4", 3), ("col", "<f4", 3)])
assert VEC_DTYPE.itemsize == 12 and MATERIAL_DTYPE.itemsize == 32
assert SPHERE_DTYPE.itemsize == 48 and LIGHT_DTYPE.itemsize == 24
# rtg_gbuf_px (include/rtg.h): the primary-hit G-buffer's record
GBUF_DTYPE = np.dtype([("id", "<i4"), ("t", "<f4"), ("hits", "<u4"), ("sample", "<u4"),
                       ("normal", "<f4", 3), ("idSum", "<u4")])
assert GBUF_DTYPE.itemsize == 32
# rtg_ray, rtg_segment and rtg_hit (include/rtg.h): the batch ray queries' records
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("dir", "<f4", 3)])
SEGMENT_DTYPE = np.dtype([("a", "<f4", 3), ("b", "<f4", 3)])
HIT_DTYPE = np.dtype([("id", "<i4"), ("t", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3)])
assert RAY_DTYPE.itemsize == 24 and SEGMENT_DTYPE.itemsize == 24 and HIT_DTYPE.itemsize == 32
# rtg_camera (include/rtg.h): the posed camera
CAMERA_DTYPE = np.dtype([("eye", "<f4", 3), ("right", "<f4", 3), ("up", "<f4", 3),
                         ("back", "<f4", 3)])
assert CAMERA_DTYPE.itemsize == 48
# rtg_ao_params (include/rtg.h): ambient occlusion
AO_PARAMS_DTYPE = np.dtype([("samples", "<u4"), ("radius", "<f4"), ("bias", "<f4"),
                            ("seed", "<u4"), ("flags", "<u4")])
assert AO_PARAMS_DTYPE.itemsize == 20
AO_MAX_SAMPLES, AO_MAX_DIRS, AO_JITTER = 1024, 65536, 1  # RTG_AO_*
# rtg_gather_params (include/rtg.h): the gather
GATHER_PARAMS_DTYPE = np.dtype([("samples", "<u4"), ("bias", "<f4"), ("seed", "<u4"),
                                ("flags", "<u4")])
assert GATHER_PARAMS_DTYPE.itemsize == 16
GATHER_MAX_SAMPLES, GATHER_MAX_DIRS = 1024, 65536  # RTG_GATHER_*
GATHER_JITTER, GATHER_SKIP_NONFINITE = 1, 2
# rtg_fold_params (include/rtg.h): views folded into per-group coefficients
FOLD_PARAMS_DTYPE = np.dtype([("viewsPerGroup", "<u4"), ("weights", "<u4"), ("flags", "<u4")])
assert FOLD_PARAMS_DTYPE.itemsize == 12
FOLD_MAX_WEIGHTS, FOLD_SKIP_NONFINITE = 16, 1  # RTG_FOLD_*
# rtg_filter_params (include/rtg.h): the edge-stopping a-trous filter
FILTER_PARAMS_DTYPE = np.dtype([("passes", "<u4"), ("normalLog2", "<u4"), ("planeScale", "<f4"),
                                ("kind", "<u4"), ("flags", "<u4")])
assert FILTER_PARAMS_DTYPE.itemsize == 20
FILTER_MAX_PASSES = 8  # RTG_FILTER_*
FILTER_RGB, FILTER_GRAY, FILTER_COUNT = 0, 1, 2
FILTER_SAME_ID, FILTER_NORMAL, FILTER_PLANE, FILTER_SKIP_NONFINITE = 1, 2, 4, 8
# rtg_accumulate_params (include/rtg.h): temporal accumulation by reprojection
ACCUM_PARAMS_DTYPE = np.dtype([("kind", "<u4"), ("flags", "<u4"), ("normalLog2", "<u4"),
                               ("planeScale", "<f4"), ("maxHistory", "<u4")])
assert ACCUM_PARAMS_DTYPE.itemsize == 20
ACCUM_SAME_ID, ACCUM_NORMAL, ACCUM_PLANE, ACCUM_SKIP_NONFINITE = 1, 2, 4, 8  # RTG_ACCUM_*
# rtg_upsample_params (include/rtg.h): guided upsampling of a low-resolution signal
UPSAMPLE_PARAMS_DTYPE = np.dtype([("kind", "<u4"), ("flags", "<u4"), ("normalLog2", "<u4"),
                                  ("planeScale", "<f4"), ("scaleLog2", "<u4")])
assert UPSAMPLE_PARAMS_DTYPE.itemsize == 20
UPSAMPLE_MAX_SCALE_LOG2 = 3  # RTG_UPSAMPLE_*
UPSAMPLE_SAME_ID, UPSAMPLE_NORMAL, UPSAMPLE_PLANE, UPSAMPLE_SKIP_NONFINITE = 1, 2, 4, 8
# rtg_variance_params and rtg_svgf_params (include/rtg.h): the variance-guided filter
VARIANCE_PARAMS_DTYPE = np.dtype([("kind", "<u4"), ("flags", "<u4"), ("normalLog2", "<u4"),
                                  ("planeScale", "<f4"), ("minHistory", "<u4")])
assert VARIANCE_PARAMS_DTYPE.itemsize == 20
SVGF_PARAMS_DTYPE = np.dtype([("passes", "<u4"), ("normalLog2", "<u4"), ("planeScale", "<f4"),
                              ("kind", "<u4"), ("flags", "<u4"), ("sigmaL", "<f4"),
                              ("epsL", "<f4")])
assert SVGF_PARAMS_DTYPE.itemsize == 28
SVGF_LUMA = 16  # RTG_SVGF_LUMA, next to the FILTER_* bits
# rtg_probe_grid and rtg_irradiance_params (include/rtg.h): the SH probe grid's lookup
PROBE_GRID_DTYPE = np.dtype([("origin", "<f4", 3), ("step", "<f4", 3), ("nx", "<u4"),
                             ("ny", "<u4"), ("nz", "<u4"), ("bands", "<u4")])
assert PROBE_GRID_DTYPE.itemsize == 40
IRR_PARAMS_DTYPE = np.dtype([("bias", "<f4"), ("lobe", "<f4", 3), ("flags", "<u4")])
assert IRR_PARAMS_DTYPE.itemsize == 20
IRR_VALID, IRR_FACING, IRR_VISIBLE = 1, 2, 4  # RTG_IRR_*
IRR_LOBE_RADIANCE = (1.0, 1.0, 1.0)
IRR_LOBE_COSINE = (1.0, float(np.float32(2.0) / np.float32(3.0)), 0.25)

RTG_OK = 0
ERRORS = {-1: "invalid argument", -2: "HIP error", -3: "out of memory",
          -4: "no such device", -5: "I/O error"}

# Every symbol include/rtg.h declares (checked by tests/test_host.py).
EXPORTED = [
    "rtg_last_error", "rtg_abi_version", "rtg_device_count", "rtg_device_info",
    "rtg_render", "rtg_context_create", "rtg_context_destroy", "rtg_context_set_scene",
    "rtg_shard_rows", "rtg_shard_global_row", "rtg_render_device", "rtg_render_rows_device",
    "rtg_render_rows", "rtg_set_launch_opts", "rtg_diag_read", "rtg_diag_timeline", "rtg_diag_counts",
    "rtg_diag_group_list",
    "rtg_context_scene_stats", "rtg_scene_ranged",
    "rtg_max_colour", "rtg_max_colour_device", "rtg_ppm_bytes", "rtg_ppm_bytes_device",
    "rtg_save_ppm", "rtg_make_material", "rtg_scene_generate", "rtg_assemble_shards_device",
    "rtg_render_multi", "rtg_scene_load", "rtg_scene_save", "rtg_context_set_semantics",
    "rtg_multi_create", "rtg_multi_set_scene", "rtg_multi_render", "rtg_multi_destroy",
    "rtg_multi_set_gather", "rtg_place_shard_device",
    "rtg_gbuffer_device", "rtg_gbuffer", "rtg_gbuffer_host",
    "rtg_intersect_device", "rtg_intersect", "rtg_intersect_host",
    "rtg_visible_device", "rtg_visible", "rtg_visible_host",
    "rtg_raytrace_device", "rtg_raytrace", "rtg_raytrace_host",
    "rtg_ray_order_scratch", "rtg_ray_order_device", "rtg_ray_order_host",
    "rtg_intersect_indexed_device", "rtg_visible_indexed_device", "rtg_raytrace_indexed_device",
    "rtg_camera_identity", "rtg_camera_look_at", "rtg_camera_sample_count",
    "rtg_camera_rays_host", "rtg_camera_rays_device",
    "rtg_camera_project_host", "rtg_camera_project_device", "rtg_camera_project",
    "rtg_render_camera_device", "rtg_render_camera", "rtg_render_camera_host",
    "rtg_render_views_device", "rtg_render_views", "rtg_render_views_host", "rtg_camera_cube",
    "rtg_views_fold_scratch", "rtg_views_fold_host", "rtg_views_fold_device",
    "rtg_render_views_fold_device", "rtg_render_views_fold", "rtg_render_views_fold_host",
    "rtg_cube_sh_weights",
    "rtg_ao_directions", "rtg_ao_segments_host", "rtg_ao_segments_device", "rtg_ao_device",
    "rtg_ao", "rtg_ao_host",
    "rtg_matte_device", "rtg_matte", "rtg_matte_host",
    "rtg_probe_grid_points", "rtg_probe_grid_poses",
    "rtg_irradiance_device", "rtg_irradiance", "rtg_irradiance_host",
    "rtg_gather_rays_host", "rtg_gather_rays_device", "rtg_gather_device", "rtg_gather",
    "rtg_gather_host",
    "rtg_filter_scratch", "rtg_filter_host", "rtg_filter_device", "rtg_filter",
    "rtg_accumulate_host", "rtg_accumulate_device", "rtg_accumulate",
    "rtg_variance_host", "rtg_variance_device", "rtg_variance",
    "rtg_svgf_scratch", "rtg_svgf_host", "rtg_svgf_device", "rtg_svgf",
    "rtg_upsample_scratch", "rtg_upsample_host", "rtg_upsample_device", "rtg_upsample",
    "rtg_hits_pick_host", "rtg_hits_pick_device",
    "rtg_values_place_host", "rtg_values_place_device",
    "rtg_contains_device", "rtg_contains", "rtg_contains_host",
]


# Counter slots of the traversal (rtg_trace.h kCnt* then the kU* executed-work
# units), the order of rtg_diag_counts / hostsim_counts.
UNIT_NAMES = [
    "samples", "primQ", "primSel", "primCand", "enterQ", "enterOK", "fullQ", "fullCand",
    "shadowQ", "shadowSel", "shadowCand", "containMasked", "containSel", "containFull",
    "refraction", "reflPush", "bvhNodeTests", "bvhSphereTests", "coneQ", "coneSel",
    "bvhShadowQ", "bvhShadowNodeTests", "bvhShadowSphereTests",
    "U.query", "U.primIter", "U.primExact", "U.selIter", "U.selExact", "U.shdIter",
    "U.shdExact", "U.enterHead", "U.enterIter", "U.enterExact", "U.fullGroup", "U.fullExact",
    "U.bvhNode", "U.bvhSlot", "U.bvhExact", "U.contIter", "U.cont4", "U.contBvhNode", "U.cone",
    "U.maskIter", "U.node", "U.shade", "U.light", "U.shadow", "U.lit", "U.refr", "U.refrLeaf",
    "U.push", "U.descend", "U.unwind", "U.sample", "U.bvhPass",
    "U.capIter", "U.ovIter", "D.shdSame", "D.enterAll", "D.enterSame", "D.contSame",
    "U.lightDir", "D.insig", "D.insigAll", "U.wave",
    "U.queryHead", "D.shdEmpty", "D.coneEmpty",
]


class RtgError(RuntimeError):
    pass


_lib = None


def lib() -> ctypes.CDLL:
    """Load librtg.so (built in-tree by `make -C raytracer-gamma_amd`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RtgError(f"librtg.so not built at {LIB_PATH}; run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        vp, u, i, f, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
        L.rtg_last_error.restype = ctypes.c_char_p
        L.rtg_abi_version.restype = i
        L.rtg_device_count.argtypes = [ctypes.POINTER(i)]
        L.rtg_device_info.argtypes = [i, ctypes.c_char_p, sz]
        L.rtg_render.argtypes = [i, vp, u, vp, u, u, u, f, f, i, vp]
        L.rtg_context_create.argtypes = [i, ctypes.POINTER(vp)]
        L.rtg_context_destroy.argtypes = [vp]
        L.rtg_context_set_scene.argtypes = [vp, vp, u, vp, u]
        L.rtg_shard_rows.argtypes = [u, u, u, u, ctypes.POINTER(u)]
        L.rtg_shard_global_row.argtypes = [u, u, u, u]
        L.rtg_shard_global_row.restype = u
        L.rtg_render_device.argtypes = [vp, u, u, f, f, i, u, u, u, vp, vp]
        L.rtg_render_rows_device.argtypes = [vp, u, u, f, f, i, vp, u, vp, vp]
        L.rtg_render_rows.argtypes = [i, vp, u, vp, u, u, u, f, f, i, vp, u, vp]
        L.rtg_set_launch_opts.argtypes = [vp, vp]
        L.rtg_context_set_semantics.argtypes = [vp, i]
        L.rtg_diag_read.argtypes = [vp, vp, i]
        L.rtg_diag_timeline.argtypes = [vp, vp, sz, vp]
        if hasattr(L, "rtg_diag_group_list"):  # (A/B libraries of older revisions lack it)
            L.rtg_diag_group_list.argtypes = [vp, vp, vp, vp, vp, sz, vp]
        # round-3 entry points; an RTG_LIB build from before them (same-box A/B
        # of older kernels, tools/ab_bench.sh) loads without them
        for name, at in (("rtg_diag_counts", [vp, vp, i, i]),
                         ("rtg_context_scene_stats", [vp, vp]),
                         ("rtg_multi_set_gather", [vp, i]),
                         ("rtg_scene_ranged", [vp, u, ctypes.POINTER(i)]),
                         ("rtg_place_shard_device", [vp, vp, u, u, u, u, u, vp, vp])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        L.rtg_max_colour.argtypes = [vp, sz]
        L.rtg_max_colour.restype = f
        L.rtg_max_colour_device.argtypes = [vp, vp, sz, vp, vp]
        L.rtg_ppm_bytes.argtypes = [vp, sz, f, vp]
        L.rtg_ppm_bytes.restype = None
        L.rtg_ppm_bytes_device.argtypes = [vp, vp, sz, vp, vp, vp]
        L.rtg_assemble_shards_device.argtypes = [vp, vp, u, u, u, u, u, vp, vp]
        L.rtg_render_multi.argtypes = [vp, i, vp, u, vp, u, u, u, f, f, i, u, vp, vp]
        L.rtg_multi_create.argtypes = [vp, i, ctypes.POINTER(vp)]
        L.rtg_multi_set_scene.argtypes = [vp, vp, u, vp, u]
        L.rtg_multi_render.argtypes = [vp, u, u, f, f, i, u, vp, vp]
        L.rtg_multi_destroy.argtypes = [vp]
        L.rtg_gbuffer_device.argtypes = [vp, u, u, f, f, u, u, u, vp, vp]
        L.rtg_gbuffer.argtypes = [i, vp, u, u, u, f, f, vp]
        L.rtg_gbuffer_host.argtypes = [vp, u, u, u, f, f, vp, i]
        for q in ("intersect", "visible"):
            getattr(L, f"rtg_{q}_device").argtypes = [vp, vp, sz, vp, vp]
            getattr(L, f"rtg_{q}").argtypes = [i, vp, u, vp, sz, vp]
            getattr(L, f"rtg_{q}_host").argtypes = [vp, u, vp, sz, vp, i, i]
        L.rtg_raytrace_device.argtypes = [vp, vp, sz, i, vp, vp]
        L.rtg_raytrace.argtypes = [i, vp, u, vp, u, vp, sz, i, vp]
        L.rtg_raytrace_host.argtypes = [vp, u, vp, u, vp, sz, i, i, vp, i, i]
        L.rtg_ray_order_scratch.argtypes = [sz, ctypes.POINTER(sz)]
        L.rtg_ray_order_device.argtypes = [vp, vp, sz, i, vp, vp, vp, sz, vp]
        L.rtg_ray_order_host.argtypes = [vp, u, vp, sz, i, vp, vp, i]
        L.rtg_intersect_indexed_device.argtypes = [vp, vp, vp, sz, vp, vp]
        L.rtg_visible_indexed_device.argtypes = [vp, vp, vp, sz, vp, vp]
        L.rtg_raytrace_indexed_device.argtypes = [vp, vp, vp, sz, i, vp, vp]
        L.rtg_camera_identity.argtypes = [vp]
        L.rtg_camera_identity.restype = None
        L.rtg_camera_look_at.argtypes = [vp, vp, vp, vp]
        L.rtg_camera_sample_count.argtypes = [f, ctypes.POINTER(u)]
        L.rtg_camera_rays_host.argtypes = [vp, u, u, f, f, vp, i]
        L.rtg_camera_rays_device.argtypes = [vp, vp, u, u, f, f, vp, vp]
        L.rtg_render_camera_device.argtypes = [vp, vp, u, u, f, f, i, vp, vp]
        L.rtg_render_camera.argtypes = [i, vp, u, vp, u, vp, u, u, f, f, i, vp]
        L.rtg_render_camera_host.argtypes = [vp, u, vp, u, vp, u, u, f, f, i, i, vp, i, i]
        L.rtg_render_views_device.argtypes = [vp, vp, sz, u, u, f, f, i, vp, vp]
        L.rtg_render_views.argtypes = [i, vp, u, vp, u, vp, sz, u, u, f, f, i, vp]
        L.rtg_render_views_host.argtypes = [vp, u, vp, u, vp, sz, u, u, f, f, i, i, vp, i, i]
        L.rtg_camera_cube.argtypes = [vp, vp]
        # the views folded into coefficients; an RTG_LIB build of the commit before
        # them (tools/ab_bench.sh against the parent) loads without them
        for name, at in (
                ("rtg_views_fold_scratch", [sz, u, u, u, vp]),
                ("rtg_views_fold_host", [vp, sz, u, u, vp, vp, vp, vp, i]),
                ("rtg_views_fold_device", [vp, vp, sz, u, u, vp, vp, vp, vp, vp, sz, vp]),
                ("rtg_render_views_fold_device",
                 [vp, vp, sz, u, u, f, f, i, vp, vp, vp, vp, vp, sz, vp]),
                ("rtg_render_views_fold",
                 [i, vp, u, vp, u, vp, sz, u, u, f, f, i, vp, vp, vp, vp]),
                ("rtg_render_views_fold_host",
                 [vp, u, vp, u, vp, sz, u, u, f, f, i, i, vp, vp, vp, vp, i, i]),
                ("rtg_cube_sh_weights", [u, u, f, vp])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        L.rtg_ao_directions.argtypes = [u, vp]
        L.rtg_ao_segments_host.argtypes = [vp, sz, vp, vp, u, vp, i]
        L.rtg_ao_segments_device.argtypes = [vp, vp, sz, vp, vp, u, vp, vp]
        L.rtg_ao_device.argtypes = [vp, vp, sz, vp, vp, u, vp, vp]
        L.rtg_ao.argtypes = [i, vp, u, vp, sz, vp, vp, u, vp]
        L.rtg_ao_host.argtypes = [vp, u, vp, sz, vp, vp, u, vp, i, i]
        L.rtg_matte_device.argtypes = [vp, vp, sz, vp, vp, vp]
        L.rtg_matte.argtypes = [i, vp, u, vp, u, vp, sz, vp, vp]
        L.rtg_matte_host.argtypes = [vp, u, vp, u, vp, sz, vp, vp, i, i]
        # the probe grid's lookup; an RTG_LIB build of the commit before it
        # (tools/ab_bench.sh against the parent) loads without it
        for name, at in (
                ("rtg_probe_grid_points", [vp, vp]),
                ("rtg_probe_grid_poses", [vp, vp]),
                ("rtg_irradiance_device", [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
                ("rtg_irradiance", [i, vp, u, vp, sz, vp, vp, vp, vp, vp, vp]),
                ("rtg_irradiance_host", [vp, u, vp, sz, vp, vp, vp, vp, vp, vp, i, i])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        # the gather; an RTG_LIB build of the commit before it (tools/ab_bench.sh
        # against the parent) loads without it
        for name, at in (
                ("rtg_gather_rays_host", [vp, sz, vp, vp, u, vp, i]),
                ("rtg_gather_rays_device", [vp, vp, sz, vp, vp, u, vp, vp]),
                ("rtg_gather_device", [vp, vp, sz, vp, vp, vp, u, i, vp, vp, vp]),
                ("rtg_gather", [i, vp, u, vp, u, vp, sz, vp, vp, vp, u, i, vp, vp]),
                ("rtg_gather_host", [vp, u, vp, u, vp, sz, vp, vp, vp, u, i, i, vp, vp, i, i])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        # the filter; an RTG_LIB build of the commit before it (tools/ab_bench.sh
        # against the parent) loads without it
        for name, at in (
                ("rtg_filter_scratch", [u, u, vp, vp]),
                ("rtg_filter_host", [vp, u, u, vp, vp, vp, i]),
                ("rtg_filter_device", [vp, vp, u, u, vp, vp, vp, vp, sz, vp]),
                ("rtg_filter", [i, vp, u, u, vp, vp, vp])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        # the accumulation and the projection; an RTG_LIB build of the commit before
        # them (tools/ab_bench.sh against the parent) loads without them
        for name, at in (
                ("rtg_camera_project_host", [vp, u, u, f, vp, sz, vp, i]),
                ("rtg_camera_project_device", [vp, vp, u, u, f, vp, sz, vp, vp]),
                ("rtg_camera_project", [i, vp, u, u, f, vp, sz, vp]),
                ("rtg_accumulate_host", [vp, u, u, vp, vp, vp, f, vp, vp, vp, vp, vp, vp, vp, i]),
                ("rtg_accumulate_device",
                 [vp, vp, u, u, vp, vp, vp, f, vp, vp, vp, vp, vp, vp, vp, vp]),
                ("rtg_accumulate", [i, vp, u, u, vp, vp, vp, f, vp, vp, vp, vp, vp, vp, vp])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        # the variance-guided filter; an RTG_LIB build of the commit before it
        # (tools/ab_bench.sh against the parent) loads without it
        for name, at in (
                ("rtg_variance_host", [vp, u, u, vp, vp, vp, vp, vp, i]),
                ("rtg_variance_device", [vp, vp, u, u, vp, vp, vp, vp, vp, vp]),
                ("rtg_variance", [i, vp, u, u, vp, vp, vp, vp, vp]),
                ("rtg_svgf_scratch", [u, u, vp, vp]),
                ("rtg_svgf_host", [vp, u, u, vp, vp, vp, vp, vp, i]),
                ("rtg_svgf_device", [vp, vp, u, u, vp, vp, vp, vp, vp, vp, sz, vp]),
                ("rtg_svgf", [i, vp, u, u, vp, vp, vp, vp, vp])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        # the guided upsampling and the index calls; an RTG_LIB build of the commit
        # before them (tools/ab_bench.sh against the parent) loads without them
        for name, at in (
                ("rtg_upsample_scratch", [u, u, i, vp]),
                ("rtg_upsample_host", [vp, u, u, vp, vp, u, u, vp, vp, vp, u, vp, i]),
                ("rtg_upsample_device",
                 [vp, vp, u, u, vp, vp, u, u, vp, vp, vp, u, vp, vp, sz, vp]),
                ("rtg_upsample", [i, vp, u, u, vp, vp, u, u, vp, vp, vp, u, vp]),
                ("rtg_hits_pick_host", [vp, sz, vp, sz, vp, i]),
                ("rtg_hits_pick_device", [vp, vp, sz, vp, sz, vp, vp]),
                ("rtg_values_place_host", [u, vp, vp, sz, sz, vp, i]),
                ("rtg_values_place_device", [vp, u, vp, vp, sz, sz, vp, vp])):
            try:
                getattr(L, name).argtypes = at
            except AttributeError:
                if not os.environ.get("RTG_LIB"):
                    raise
        L.rtg_contains_device.argtypes = [vp, vp, sz, vp, vp]
        L.rtg_contains.argtypes = [i, vp, u, vp, sz, vp]
        L.rtg_contains_host.argtypes = [vp, u, vp, sz, vp, i, i]

        pu = ctypes.POINTER(u)
        L.rtg_scene_load.argtypes = [ctypes.c_char_p, vp, u, pu, vp, u, pu]
        L.rtg_scene_save.argtypes = [ctypes.c_char_p, vp, u, vp, u]
        L.rtg_save_ppm.argtypes = [vp, ctypes.c_char_p, i, i, f]
        L.rtg_make_material.argtypes = [f, f, vp, vp, f, vp]
        L.rtg_make_material.restype = None
        L.rtg_scene_generate.argtypes = [ctypes.c_ulonglong, u, u, vp, vp]
        _lib = L
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != RTG_OK:
        msg = lib().rtg_last_error().decode(errors="replace")
        raise RtgError(f"{what}: {ERRORS.get(rc, rc)}: {msg}")


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


# ---------------------------------------------------------------- scene helpers
def make_material(opacity, gloss_factor, matte, gloss, refractive_index):
    """setMatOpacity + setMatteGlossBalance + setMatRefractivityIndex (raytracer.h:53-74)."""
    out = np.zeros(1, MATERIAL_DTYPE)
    m = np.asarray(matte, np.float32)
    g = np.asarray(gloss, np.float32)
    lib().rtg_make_material(float(opacity), float(gloss_factor), _ptr(m), _ptr(g),
                            float(refractive_index), _ptr(out))
    return out[0]


def generate_scene(n_spheres: int, n_lights: int, seed: int = 42):
    """main.cpp:104-168 scene, extended by the seeded generator of SURVEY.md §8d."""
    sph = np.zeros(n_spheres, SPHERE_DTYPE)
    lgt = np.zeros(n_lights, LIGHT_DTYPE)
    _check(lib().rtg_scene_generate(seed, n_spheres, n_lights, _ptr(sph), _ptr(lgt)),
           "rtg_scene_generate")
    return sph, lgt


def load_scene_file(path: str):
    """Spheres and lights of a scene file (rtg_scene_load; format in include/rtg.h)."""
    n, m = ctypes.c_uint(0), ctypes.c_uint(0)
    _check(lib().rtg_scene_load(path.encode(), None, 0, ctypes.byref(n), None, 0,
                                ctypes.byref(m)), "rtg_scene_load")
    sph = np.zeros(n.value, SPHERE_DTYPE)
    lgt = np.zeros(m.value, LIGHT_DTYPE)
    _check(lib().rtg_scene_load(path.encode(), _ptr(sph), n.value, ctypes.byref(n), _ptr(lgt),
                                m.value, ctypes.byref(m)), "rtg_scene_load")
    return sph, lgt


def save_scene_file(path: str, spheres, lights) -> None:
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    _check(lib().rtg_scene_save(path.encode(), _ptr(spheres), len(spheres), _ptr(lights),
                                len(lights)), "rtg_scene_save")


def reference_scene():
    """The scene hard-coded in main.cpp:104-168 (3 spheres, 2 lights)."""
    return generate_scene(3, 2)


# ---------------------------------------------------------------- output helpers
def max_colour_value(fb: np.ndarray) -> float:
    """maxColourValuePixelBuffer, algebra.h:68-91."""
    fb = np.ascontiguousarray(fb, np.float32)
    return float(lib().rtg_max_colour(_ptr(fb), fb.size // 3))


def ppm_bytes(fb: np.ndarray, max_colour: float) -> np.ndarray:
    fb = np.ascontiguousarray(fb, np.float32)
    out = np.empty(fb.size, np.uint8)
    lib().rtg_ppm_bytes(_ptr(fb), fb.size // 3, float(max_colour), _ptr(out))
    return out


def ppm_file_bytes(fb: np.ndarray, max_colour: float | None = None) -> bytes:
    """Exact bytes savePPM (main.cpp:43-91) writes for an (H, W, 3) framebuffer."""
    h, w = fb.shape[0], fb.shape[1]
    mx = max_colour_value(fb) if max_colour is None else max_colour
    return b"P6\n%d %d\n255\n" % (w, h) + ppm_bytes(fb, mx).tobytes()


def save_ppm(fb: np.ndarray, filename: str, max_colour: float | None = None) -> None:
    fb = np.ascontiguousarray(fb, np.float32)
    mx = max_colour_value(fb) if max_colour is None else max_colour
    _check(lib().rtg_save_ppm(_ptr(fb), filename.encode(), fb.shape[1], fb.shape[0], mx),
           "rtg_save_ppm")


def shard_rows(height: int, row_block: int, shard: int, n_shards: int) -> int:
    r = ctypes.c_uint(0)
    _check(lib().rtg_shard_rows(height, row_block, shard, n_shards, ctypes.byref(r)),
           "rtg_shard_rows")
    return r.value


def shard_row_indices(height: int, row_block: int, shard: int, n_shards: int) -> np.ndarray:
    n = shard_rows(height, row_block, shard, n_shards)
    f = lib().rtg_shard_global_row
    return np.array([f(k, row_block, shard, n_shards) for k in range(n)], np.int64)


# ---------------------------------------------------------------- device
def device_count() -> int:
    c = ctypes.c_int(0)
    _check(lib().rtg_device_count(ctypes.byref(c)), "rtg_device_count")
    return c.value


def device_info(device: int = 0) -> str:
    buf = ctypes.create_string_buffer(256)
    _check(lib().rtg_device_info(device, buf, 256), "rtg_device_info")
    return buf.value.decode()


def render(spheres, lights, width: int, height: int, zoom: float = -4.0,
           alias_factor: float = 3.0, stack_size: int = 6, device: int = 0) -> np.ndarray:
    """One-shot drop-in for the reference's GPU launch (main.cpp:277-468):
    returns the (H, W, 3) float32 framebuffer of the reference CPU path."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    out = np.empty((height, width, 3), np.float32)
    _check(lib().rtg_render(device, _ptr(spheres), len(spheres), _ptr(lights), len(lights),
                            width, height, float(zoom), float(alias_factor), stack_size,
                            _ptr(out)), "rtg_render")
    return out


def render_multi(spheres, lights, width: int, height: int, devices=(0,), zoom: float = -4.0,
                 alias_factor: float = 3.0, stack_size: int = 6, row_block: int = 16):
    """Multi-GPU one-shot in ONE process (rtg_render_multi): row-cyclic shards on
    `devices`, one RCCL gather to devices[0].  Returns (frame, timings_ms) with
    timings = [slowest render, gather + assemble, wall]."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    devs = np.ascontiguousarray(devices, np.int32)
    out = np.empty((height, width, 3), np.float32)
    tm = np.zeros(3, np.float32)
    _check(lib().rtg_render_multi(_ptr(devs), len(devs), _ptr(spheres), len(spheres),
                                  _ptr(lights), len(lights), width, height, float(zoom),
                                  float(alias_factor), stack_size, row_block, _ptr(out),
                                  _ptr(tm)), "rtg_render_multi")
    return out, [float(v) for v in tm]


def scene_ranged(spheres) -> bool:
    """Whether the scene passes the value-range proof of the masked render
    kernel's guard-free build (rtg_scene_ranged; host only, no GPU needed)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    out = ctypes.c_int(-1)
    _check(lib().rtg_scene_ranged(_ptr(spheres), len(spheres), ctypes.byref(out)),
           "rtg_scene_ranged")
    return bool(out.value)


def gbuffer(spheres, width: int, height: int, zoom: float = -4.0, alias_factor: float = 3.0,
            device: int = 0) -> np.ndarray:
    """Primary-hit G-buffer of a scene on the GPU (rtg_gbuffer): an (H, W) array
    of GBUF_DTYPE records (closest sphere id, t, normal, sample coverage)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    out = np.empty((height, width), GBUF_DTYPE)
    _check(lib().rtg_gbuffer(device, _ptr(spheres), len(spheres), width, height, float(zoom),
                             float(alias_factor), _ptr(out)), "rtg_gbuffer")
    return out


def gbuffer_host(spheres, width: int, height: int, zoom: float = -4.0,
                 alias_factor: float = 3.0, threads: int = 1) -> np.ndarray:
    """The same records computed on the host with plain loops (rtg_gbuffer_host;
    no GPU needed)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    out = np.empty((height, width), GBUF_DTYPE)
    _check(lib().rtg_gbuffer_host(_ptr(spheres), len(spheres), width, height, float(zoom),
                                  float(alias_factor), _ptr(out), threads), "rtg_gbuffer_host")
    return out


def _batch(records, dtype, out_dtype):
    """A batch as a contiguous 1-D record array (an (N, 6) float32 array is
    taken as N records), its length, and the result array with pointers that
    are never null (an empty batch is legal: RTG_OK, nothing written)."""
    a = np.asarray(records)
    if a.dtype != dtype:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 6).view(dtype).reshape(-1)
    a = np.ascontiguousarray(a).reshape(-1)
    n = len(a)
    out = np.empty(n, out_dtype)
    src = a if n else np.zeros(1, dtype)
    dst = out if n else np.zeros(1, out_dtype)
    return src, n, out, dst


def intersect(spheres, rays, device: int = 0) -> np.ndarray:
    """Closest hit of every ray of a batch on the GPU (rtg_intersect): RAY_DTYPE
    records (or an (N, 6) float32 array: origin, dir) in, HIT_DTYPE records out,
    calcIntersection's answer bit for bit.  Directions are used as given."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    src, n, out, dst = _batch(rays, RAY_DTYPE, HIT_DTYPE)
    _check(lib().rtg_intersect(device, _ptr(spheres), len(spheres), _ptr(src), n, _ptr(dst)),
           "rtg_intersect")
    return out


def intersect_host(spheres, rays, walk: int = 0, threads: int = 1) -> np.ndarray:
    """The same on the host (rtg_intersect_host; no GPU needed).  walk 0: plain
    loops over every ray and sphere; walk 1: the device kernel's own query path
    (BVH, 64-sphere query or flat loop) compiled for the host."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    src, n, out, dst = _batch(rays, RAY_DTYPE, HIT_DTYPE)
    _check(lib().rtg_intersect_host(_ptr(spheres), len(spheres), _ptr(src), n, _ptr(dst), walk,
                                    threads), "rtg_intersect_host")
    return out


def visible(spheres, segments, device: int = 0) -> np.ndarray:
    """Line of sight of every segment of a batch on the GPU (rtg_visible):
    SEGMENT_DTYPE records (or (N, 6) float32: a, b) in, uint8 out, 1 where
    hasClearLineOfSight(a, b) holds."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    src, n, out, dst = _batch(segments, SEGMENT_DTYPE, np.uint8)
    _check(lib().rtg_visible(device, _ptr(spheres), len(spheres), _ptr(src), n, _ptr(dst)),
           "rtg_visible")
    return out


def visible_host(spheres, segments, walk: int = 0, threads: int = 1) -> np.ndarray:
    """The same on the host (rtg_visible_host; walk as intersect_host)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    src, n, out, dst = _batch(segments, SEGMENT_DTYPE, np.uint8)
    _check(lib().rtg_visible_host(_ptr(spheres), len(spheres), _ptr(src), n, _ptr(dst), walk,
                                  threads), "rtg_visible_host")
    return out


def _colours(rays):
    """A ray batch and its (N, 3) float32 result, as _batch."""
    src, n, out, dst = _batch(rays, RAY_DTYPE, np.dtype(("<f4", 3)))
    return src, n, out.reshape(n, 3), dst


def raytrace(spheres, lights, rays, stack_size: int = 6, device: int = 0) -> np.ndarray:
    """rayTrace's colour of every ray of a batch on the GPU (rtg_raytrace):
    RAY_DTYPE records (or (N, 6) float32: origin, dir) in, (N, 3) float32 out,
    the reference's return value bit for bit (before the 1/nS scale of a
    pixel's sum).  Directions are used as given."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    src, n, out, dst = _colours(rays)
    _check(lib().rtg_raytrace(device, _ptr(spheres), len(spheres), _ptr(lights), len(lights),
                              _ptr(src), n, stack_size, _ptr(dst)), "rtg_raytrace")
    return out


def raytrace_host(spheres, lights, rays, stack_size: int = 6, semantics: int = 0,
                  walk: int = 0, threads: int = 1) -> np.ndarray:
    """The same on the host (rtg_raytrace_host; no GPU needed).  walk 0: plain
    loops over every sphere for every query; walk 1: the device kernel's own
    path compiled for the host.  semantics: 0 the CPU path, 1 the OpenCL kernel's."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    src, n, out, dst = _colours(rays)
    _check(lib().rtg_raytrace_host(_ptr(spheres), len(spheres), _ptr(lights), len(lights),
                                   _ptr(src), n, stack_size, semantics, _ptr(dst), walk, threads),
           "rtg_raytrace_host")
    return out


# The ray order (include/rtg.h): RTG_ORDER_RAYS / RTG_ORDER_SEGMENTS, and the
# device sort's geometry: rays per tile (RTG_ORDER_TILE_RAYS) and tiles per
# scan step (RTG_ORDER_SCAN_TILES), and the keys kernel's largest grid
# (RTG_ORDER_KEY_GRID workgroups: a batch of more tiles strides over them).
ORDER_RAYS, ORDER_SEGMENTS = 0, 1
ORDER_TILE_RAYS = 1024
ORDER_SCAN_TILES = 256
ORDER_KEY_GRID = 2048
ORDER_ORIGIN_BITS, ORDER_DIR_BITS = 10, 10  # key bits per origin axis / direction axis
ORDER_KEY_BITS = 3 * ORDER_ORIGIN_BITS + 2 * ORDER_DIR_BITS  # the key's used bits


def ray_order_scratch(n: int) -> int:
    """Bytes of device scratch Context.ray_order needs for n rays (rtg_ray_order_scratch)."""
    b = ctypes.c_size_t(0)
    _check(lib().rtg_ray_order_scratch(n, ctypes.byref(b)), "rtg_ray_order_scratch")
    return b.value


def ray_order_host(spheres, rays, kind: int = 0, threads: int = 1, keys: bool = False):
    """The coherence order of a batch on the host (rtg_ray_order_host; no GPU
    needed): uint32 order with order[k] = the index of the ray at position k of
    the batch stably sorted by key.  rays: RAY_DTYPE records, SEGMENT_DTYPE
    records with kind = ORDER_SEGMENTS, or (N, 6) float32.  keys=True: returns
    (order, keys), keys[i] the uint64 key of ray i."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    dtype = SEGMENT_DTYPE if kind == ORDER_SEGMENTS else RAY_DTYPE
    src, n, order, dst = _batch(rays, dtype, np.uint32)
    k = np.zeros(n, np.uint64)
    kp = _ptr(k) if keys and n else None
    _check(lib().rtg_ray_order_host(_ptr(spheres), len(spheres), _ptr(src), n, kind, _ptr(dst),
                                    kp, threads), "rtg_ray_order_host")
    return (order, k) if keys else order


def _camera(cam) -> np.ndarray:
    """A pose as one CAMERA_DTYPE record (a record, or 12 floats: eye, right, up, back)."""
    a = np.asarray(cam)
    if a.dtype != CAMERA_DTYPE:
        a = np.ascontiguousarray(a, np.float32).reshape(12).view(CAMERA_DTYPE)
    return np.ascontiguousarray(a).reshape(1)


def camera_identity() -> np.ndarray:
    """The reference's own camera as a pose (rtg_camera_identity): eye 0, right
    +x, up +y, back +z."""
    out = np.zeros(1, CAMERA_DTYPE)
    lib().rtg_camera_identity(_ptr(out))
    return out[0]


def camera_look_at(eye, target, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """The pose at `eye` looking at `target` (rtg_camera_look_at), in float32."""
    e, t, u = (np.ascontiguousarray(v, np.float32).reshape(3) for v in (eye, target, up))
    out = np.zeros(1, CAMERA_DTYPE)
    _check(lib().rtg_camera_look_at(_ptr(e), _ptr(t), _ptr(u), _ptr(out)), "rtg_camera_look_at")
    return out[0]


def camera_sample_count(alias_factor: float) -> int:
    """nAA of rtg_camera_sample_count: a pixel has nAA * nAA samples."""
    n = ctypes.c_uint(0)
    _check(lib().rtg_camera_sample_count(float(alias_factor), ctypes.byref(n)),
           "rtg_camera_sample_count")
    return n.value


def camera_rays_host(cam, width: int, height: int, zoom: float = -4.0,
                     alias_factor: float = 3.0, threads: int = 1) -> np.ndarray:
    """The pose's sample rays on the host (rtg_camera_rays_host): (W*H*nAA*nAA, 6)
    float32 (origin, dir), pixel order, a pixel's samples in the reference's order."""
    c = _camera(cam)
    n = width * height * camera_sample_count(alias_factor) ** 2
    out = np.empty((n, 6), np.float32)
    dst = out if n else np.zeros((1, 6), np.float32)
    _check(lib().rtg_camera_rays_host(_ptr(c), width, height, float(zoom), float(alias_factor),
                                      _ptr(dst), threads), "rtg_camera_rays_host")
    return out


def camera_rays(cam, width: int, height: int, zoom: float = -4.0, alias_factor: float = 3.0,
                device: int = 0) -> np.ndarray:
    """The same rays formed on the GPU (rtg_camera_rays_device) into a torch
    tensor and downloaded; to keep them on the device use Context.camera_rays."""
    if torch is None:
        raise RtgError("camera_rays: needs torch for the device buffer")
    n = width * height * camera_sample_count(alias_factor) ** 2
    with torch.cuda.device(device):
        buf = torch.empty((max(n, 1), 6), dtype=torch.float32, device="cuda")
        ctx = Context(device)
        try:
            ctx.camera_rays(cam, width, height, buf.data_ptr(), zoom, alias_factor,
                            stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            ctx.close()
    return buf[:n].cpu().numpy()


def render_camera(spheres, lights, cam, width: int, height: int, zoom: float = -4.0,
                  alias_factor: float = 3.0, stack_size: int = 6, device: int = 0) -> np.ndarray:
    """One-shot frame of a posed camera on the GPU (rtg_render_camera): the
    (H, W, 3) float32 framebuffer, per pixel the reference's fold of rayTrace
    over the pose's sample rays, bit for bit."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    c = _camera(cam)
    out = np.empty((height, width, 3), np.float32)
    _check(lib().rtg_render_camera(device, _ptr(spheres), len(spheres), _ptr(lights), len(lights),
                                   _ptr(c), width, height, float(zoom), float(alias_factor),
                                   stack_size, _ptr(out)), "rtg_render_camera")
    return out


def render_camera_host(spheres, lights, cam, width: int, height: int, zoom: float = -4.0,
                       alias_factor: float = 3.0, stack_size: int = 6, semantics: int = 0,
                       walk: int = 0, threads: int = 1) -> np.ndarray:
    """The same on the host (rtg_render_camera_host; no GPU needed); walk and
    semantics as raytrace_host."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    c = _camera(cam)
    out = np.empty((height, width, 3), np.float32)
    _check(lib().rtg_render_camera_host(_ptr(spheres), len(spheres), _ptr(lights), len(lights),
                                        _ptr(c), width, height, float(zoom), float(alias_factor),
                                        stack_size, semantics, _ptr(out), walk, threads),
           "rtg_render_camera_host")
    return out


def _cameras(cams) -> np.ndarray:
    """A pose table as CAMERA_DTYPE records (records, or (n, 12) floats)."""
    a = np.asarray(cams)
    if a.dtype != CAMERA_DTYPE:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 12).view(CAMERA_DTYPE)
    return np.ascontiguousarray(a).reshape(-1)


def camera_cube(eye) -> np.ndarray:
    """The six cube-map poses at `eye` (rtg_camera_cube): +X, -X, +Y, -Y, +Z, -Z,
    for a square frame at zoom = -1."""
    e = np.ascontiguousarray(eye, np.float32).reshape(3)
    out = np.zeros(6, CAMERA_DTYPE)
    _check(lib().rtg_camera_cube(_ptr(e), _ptr(out)), "rtg_camera_cube")
    return out


def render_views(spheres, lights, cams, width: int, height: int, zoom: float = -4.0,
                 alias_factor: float = 3.0, stack_size: int = 6, device: int = 0) -> np.ndarray:
    """One-shot frames of a table of poses on the GPU in one launch
    (rtg_render_views): (n, H, W, 3) float32, view v bit for bit
    render_camera_host of cams[v]."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    c = _cameras(cams)
    out = np.empty((len(c), height, width, 3), np.float32)
    dst = out if len(c) else np.zeros((1, 3), np.float32)
    _check(lib().rtg_render_views(device, _ptr(spheres), len(spheres), _ptr(lights), len(lights),
                                  _ptr(c) if len(c) else None, len(c), width, height,
                                  float(zoom), float(alias_factor), stack_size, _ptr(dst)),
           "rtg_render_views")
    return out


def render_views_host(spheres, lights, cams, width: int, height: int, zoom: float = -4.0,
                      alias_factor: float = 3.0, stack_size: int = 6, semantics: int = 0,
                      walk: int = 0, threads: int = 1) -> np.ndarray:
    """The same on the host (rtg_render_views_host; no GPU needed); walk and
    semantics as raytrace_host."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    c = _cameras(cams)
    out = np.empty((len(c), height, width, 3), np.float32)
    dst = out if len(c) else np.zeros((1, 3), np.float32)
    _check(lib().rtg_render_views_host(_ptr(spheres), len(spheres), _ptr(lights), len(lights),
                                       _ptr(c) if len(c) else None, len(c), width, height,
                                       float(zoom), float(alias_factor), stack_size, semantics,
                                       _ptr(dst), walk, threads), "rtg_render_views_host")
    return out


def fold_params(views_per_group: int, weights: int, flags: int = 0) -> np.ndarray:
    """One rtg_fold_params record (flags: FOLD_SKIP_NONFINITE)."""
    p = np.zeros(1, FOLD_PARAMS_DTYPE)
    p[0] = (views_per_group, weights, flags)
    return p


def _fold_table(weights, params):
    """The weight table as contiguous float32 (never a null pointer) and the
    params record."""
    w = np.ascontiguousarray(weights, np.float32)
    p = np.ascontiguousarray(params, FOLD_PARAMS_DTYPE).reshape(1)
    return (w if w.size else np.zeros(1, np.float32)), p


def views_fold_scratch(n_views: int, width: int, height: int, weights: int) -> int:
    """Bytes of tile partials Context.views_fold / render_views_fold need
    (rtg_views_fold_scratch): caller-owned, 16-byte aligned."""
    out = ctypes.c_size_t(0)
    _check(lib().rtg_views_fold_scratch(n_views, width, height, weights, ctypes.byref(out)),
           "rtg_views_fold_scratch")
    return int(out.value)


def views_fold_host(frames, weights, params, threads: int = 1, skipped: bool = False):
    """Groups of frames folded by a weight table on the host (rtg_views_fold_host,
    the plain-loop statement of rtg.h's summation order): frames (n, H, W, 3)
    float32, weights G * H * W * K float32 (any shape), params from fold_params();
    (nGroups, K, 3) float32, with skipped=True also the uint32 counts."""
    fr = np.ascontiguousarray(frames, np.float32)
    assert fr.ndim == 4 and fr.shape[3] == 3, "frames are (n, H, W, 3)"
    n, H, W = fr.shape[:3]
    w, p = _fold_table(weights, params)
    G, K = max(int(p["viewsPerGroup"][0]), 1), int(p["weights"][0])
    out = np.empty((n // G, K, 3), np.float32)
    cnt = np.zeros(max(n // G, 1), np.uint32)
    dst = out if out.size else np.zeros((1, 3), np.float32)
    _check(lib().rtg_views_fold_host(_ptr(fr) if fr.size else None, n, W, H, _ptr(p), _ptr(w),
                                     _ptr(dst), _ptr(cnt) if skipped else None, threads),
           "rtg_views_fold_host")
    return (out, cnt[:n // G]) if skipped else out


def render_views_fold_host(spheres, lights, cams, width: int, height: int, weights, params,
                           zoom: float = -4.0, alias_factor: float = 3.0, stack_size: int = 6,
                           semantics: int = 0, walk: int = 0, threads: int = 1,
                           skipped: bool = False):
    """render_views_host, then views_fold_host, in one call with no frames on the
    caller's side (rtg_render_views_fold_host; no GPU needed)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    c = _cameras(cams)
    w, p = _fold_table(weights, params)
    G, K = max(int(p["viewsPerGroup"][0]), 1), int(p["weights"][0])
    out = np.empty((len(c) // G, K, 3), np.float32)
    cnt = np.zeros(max(len(c) // G, 1), np.uint32)
    dst = out if out.size else np.zeros((1, 3), np.float32)
    _check(lib().rtg_render_views_fold_host(
        _ptr(spheres), len(spheres), _ptr(lights), len(lights), _ptr(c) if len(c) else None,
        len(c), width, height, float(zoom), float(alias_factor), stack_size, semantics, _ptr(p),
        _ptr(w), _ptr(dst), _ptr(cnt) if skipped else None, walk, threads),
        "rtg_render_views_fold_host")
    return (out, cnt[:len(c) // G]) if skipped else out


def render_views_fold(spheres, lights, cams, width: int, height: int, weights, params,
                      zoom: float = -4.0, alias_factor: float = 3.0, stack_size: int = 6,
                      device: int = 0, skipped: bool = False):
    """One-shot fused render + fold on the GPU (rtg_render_views_fold): poses in,
    (nGroups, K, 3) coefficients out, no frame anywhere; word for word
    render_views_fold_host(walk 0)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    c = _cameras(cams)
    w, p = _fold_table(weights, params)
    G, K = max(int(p["viewsPerGroup"][0]), 1), int(p["weights"][0])
    out = np.empty((len(c) // G, K, 3), np.float32)
    cnt = np.zeros(max(len(c) // G, 1), np.uint32)
    dst = out if out.size else np.zeros((1, 3), np.float32)
    _check(lib().rtg_render_views_fold(
        device, _ptr(spheres), len(spheres), _ptr(lights), len(lights),
        _ptr(c) if len(c) else None, len(c), width, height, float(zoom), float(alias_factor),
        stack_size, _ptr(p), _ptr(w), _ptr(dst), _ptr(cnt) if skipped else None),
        "rtg_render_views_fold")
    return (out, cnt[:len(c) // G]) if skipped else out


def cube_sh_weights(res: int, bands: int = 3, alias_factor: float = 1.0) -> np.ndarray:
    """Real-SH projection weights for camera_cube's six res x res faces at zoom -1
    (rtg_cube_sh_weights): (6, res, res, bands * bands) float32, for fold_params(6,
    bands * bands).  A convenience; its bits are not part of the contract."""
    out = np.zeros((6, max(res, 1), max(res, 1), max(bands * bands, 1)), np.float32)
    _check(lib().rtg_cube_sh_weights(res, bands, float(alias_factor), _ptr(out)),
           "rtg_cube_sh_weights")
    return out


def ao_params(samples: int, radius: float, bias: float = 1e-3, seed: int = 0,
              flags: int = 0) -> np.ndarray:
    """One rtg_ao_params record (flags: AO_JITTER for a per-point window into the table)."""
    p = np.zeros(1, AO_PARAMS_DTYPE)
    p[0] = (samples, radius, bias, seed & 0xFFFFFFFF, flags)
    return p


def ao_directions(n_dirs: int) -> np.ndarray:
    """The cosine-weighted golden-angle direction set (rtg_ao_directions): (n_dirs, 3)
    float32 in the frame whose z axis is the normal.  A convenience; its bits
    are not part of the contract."""
    out = np.zeros((max(n_dirs, 1), 3), np.float32)
    _check(lib().rtg_ao_directions(n_dirs, _ptr(out)), "rtg_ao_directions")
    return out[:n_dirs]


def _ao_args(hits, dirs, params):
    """Hit records, direction table and params as contiguous arrays whose
    pointers are never null (an empty batch is legal), and the two counts."""
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(params, AO_PARAMS_DTYPE).reshape(1)
    return (h if len(h) else np.zeros(1, HIT_DTYPE)), len(h), \
        (d if len(d) else np.zeros((1, 3), np.float32)), len(d), p


def ao_segments_host(hits, dirs, params, threads: int = 1) -> np.ndarray:
    """The probe segments of every hit point on the host (rtg_ao_segments_host):
    (n * K, 6) float32 (a, b), point-major; params from ao_params()."""
    h, n, d, nd, p = _ao_args(hits, dirs, params)
    k = int(p["samples"][0])
    out = np.empty((n * k, 6), np.float32)
    dst = out if out.size else np.zeros((1, 6), np.float32)
    _check(lib().rtg_ao_segments_host(_ptr(h), n, _ptr(p), _ptr(d), nd, _ptr(dst), threads),
           "rtg_ao_segments_host")
    return out


def ao_host(spheres, hits, dirs, params, walk: int = 0, threads: int = 1) -> np.ndarray:
    """Ambient occlusion on the host (rtg_ao_host; no GPU needed): per hit point
    the uint16 count of its K probes with a clear line of sight.  walk 0: plain
    loops; walk 1: the kernel's own path over the packed tables."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    h, n, d, nd, p = _ao_args(hits, dirs, params)
    out = np.empty(n, np.uint16)
    dst = out if n else np.zeros(1, np.uint16)
    _check(lib().rtg_ao_host(_ptr(spheres), len(spheres), _ptr(h), n, _ptr(p), _ptr(d), nd,
                             _ptr(dst), walk, threads), "rtg_ao_host")
    return out


def ao(spheres, hits, dirs, params, device: int = 0) -> np.ndarray:
    """The same on the GPU, one-shot (rtg_ao): HIT_DTYPE records as intersect()
    returns them in, uint16 counts out; count / K is the usual AO term."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    h, n, d, nd, p = _ao_args(hits, dirs, params)
    out = np.empty(n, np.uint16)
    dst = out if n else np.zeros(1, np.uint16)
    _check(lib().rtg_ao(device, _ptr(spheres), len(spheres), _ptr(h), n, _ptr(p), _ptr(d), nd,
                        _ptr(dst)), "rtg_ao")
    return out


def _matte_args(spheres, lights, hits, mask: bool):
    """Scene arrays, hit records and the two results, with pointers that are
    never null for an empty batch (legal: RTG_OK, nothing written)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    n = len(h)
    out = np.empty((n, 3), np.float32)
    lit = np.empty(n, np.uint64) if mask else None
    src = h if n else np.zeros(1, HIT_DTYPE)
    dst = out if n else np.zeros((1, 3), np.float32)
    lp = None if lit is None else ctypes.c_void_p((lit if n else np.zeros(1, np.uint64)).ctypes.data)
    return spheres, lights, src, n, out, dst, lit, lp


def matte_host(spheres, lights, hits, walk: int = 0, threads: int = 1, mask: bool = False):
    """Direct light on the host (rtg_matte_host; no GPU needed): per HIT_DTYPE
    record calculateMatte's sum over the lights, (n, 3) float32, the reference's
    bits.  mask=True: returns (sums, lit), lit the uint64 mask of the first 64
    lights that reach the point.  walk 0: plain loops; walk 1: the kernel's own
    path over the packed tables."""
    sph, lgt, src, n, out, dst, lit, lp = _matte_args(spheres, lights, hits, mask)
    _check(lib().rtg_matte_host(_ptr(sph), len(sph), _ptr(lgt), len(lgt), _ptr(src), n, _ptr(dst),
                                lp, walk, threads), "rtg_matte_host")
    return (out, lit) if mask else out


def matte(spheres, lights, hits, device: int = 0, mask: bool = False):
    """The same on the GPU, one-shot (rtg_matte): HIT_DTYPE records as
    intersect() returns them in."""
    sph, lgt, src, n, out, dst, lit, lp = _matte_args(spheres, lights, hits, mask)
    _check(lib().rtg_matte(device, _ptr(sph), len(sph), _ptr(lgt), len(lgt), _ptr(src), n,
                           _ptr(dst), lp), "rtg_matte")
    return (out, lit) if mask else out


def probe_grid(origin, step, dims, bands: int = 3) -> np.ndarray:
    """One rtg_probe_grid record: probe (ix, iy, iz) of the dims = (nx, ny, nz)
    lattice sits at origin + (ix, iy, iz) * step and holds bands * bands
    coefficients."""
    g = np.zeros(1, PROBE_GRID_DTYPE)
    g[0] = (tuple(origin), tuple(step), dims[0], dims[1], dims[2], bands)
    return g


def irradiance_params(bias: float = 1e-3, lobe=IRR_LOBE_RADIANCE, flags: int = 0) -> np.ndarray:
    """One rtg_irradiance_params record (flags: IRR_VALID | IRR_FACING |
    IRR_VISIBLE; lobe: IRR_LOBE_RADIANCE, IRR_LOBE_COSINE or three factors)."""
    p = np.zeros(1, IRR_PARAMS_DTYPE)
    p[0] = (bias, tuple(lobe), flags)
    return p


def _grid(grid) -> np.ndarray:
    return np.ascontiguousarray(grid, PROBE_GRID_DTYPE).reshape(1)


def _grid_probes(g) -> int:
    return int(g["nx"][0]) * int(g["ny"][0]) * int(g["nz"][0])


def _grid_rows(g) -> int:
    """Rows to allocate for a per-probe result: the probes of a grid the library
    accepts, one for a grid it rejects before it writes."""
    n = _grid_probes(g)
    return n if 1 <= n * int(g["bands"][0]) ** 2 < 1 << 31 else 1


def probe_grid_points(grid) -> np.ndarray:
    """The probe positions in index order (rtg_probe_grid_points): (nx * ny * nz, 3)
    float32.  contains*(...) < 0 of them gives the lookup's validity bytes."""
    g = _grid(grid)
    out = np.zeros((_grid_rows(g), 3), np.float32)
    _check(lib().rtg_probe_grid_points(_ptr(g), _ptr(out)), "rtg_probe_grid_points")
    return out


def probe_grid_poses(grid) -> np.ndarray:
    """camera_cube of every probe position, 6 per probe, probe-major
    (rtg_probe_grid_poses): the pose table of a bake with fold_params(6, K)."""
    g = _grid(grid)
    out = np.zeros(6 * _grid_rows(g), CAMERA_DTYPE)
    _check(lib().rtg_probe_grid_poses(_ptr(g), _ptr(out)), "rtg_probe_grid_poses")
    return out


def _irradiance_args(spheres, hits, grid, coeffs, valid, params, weight: bool):
    """Scene, records, tables and the two results, with pointers that are never
    null for an empty batch (legal: RTG_OK, nothing written); the validity
    table's pointer is null when there is none."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    n = len(h)
    g = _grid(grid)
    p = np.ascontiguousarray(params, IRR_PARAMS_DTYPE).reshape(1)
    c = np.ascontiguousarray(coeffs, np.float32).reshape(-1, 3)
    k = int(g["bands"][0]) ** 2
    assert len(c) == _grid_probes(g) * k, "coeffs are (nx * ny * nz * bands^2, 3)"
    v = None
    if valid is not None:
        v = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        assert len(v) == _grid_probes(g), "valid is one byte per probe"
    out = np.empty((n, 3), np.float32)
    w = np.empty(n, np.float32) if weight else None
    src = h if n else np.zeros(1, HIT_DTYPE)
    dst = out if n else np.zeros((1, 3), np.float32)
    wp = None if w is None else ctypes.c_void_p((w if n else np.zeros(1, np.float32)).ctypes.data)
    return spheres, src, n, g, p, c, v, out, dst, w, wp


def irradiance_host(spheres, hits, grid, coeffs, params, valid=None, walk: int = 0,
                    threads: int = 1, weight: bool = False):
    """The light of a grid of SH probes at every hit point on the host
    (rtg_irradiance_host; no GPU needed): (n, 3) float32; weight=True: returns
    (colours, weights), a weight of 0 where no probe was left.  grid from
    probe_grid(), coeffs as render_views_fold* returns them for
    probe_grid_poses(grid), params from irradiance_params().  walk 0: plain
    loops; walk 1: the kernel's own path over the packed tables."""
    sph, src, n, g, p, c, v, out, dst, w, wp = _irradiance_args(spheres, hits, grid, coeffs, valid,
                                                                params, weight)
    _check(lib().rtg_irradiance_host(_ptr(sph), len(sph), _ptr(src), n, _ptr(g), _ptr(c), _ptr(v),
                                     _ptr(p), _ptr(dst), wp, walk, threads), "rtg_irradiance_host")
    return (out, w) if weight else out


def irradiance(spheres, hits, grid, coeffs, params, valid=None, device: int = 0,
               weight: bool = False):
    """The same on the GPU, one-shot (rtg_irradiance): HIT_DTYPE records as
    intersect() returns them in."""
    sph, src, n, g, p, c, v, out, dst, w, wp = _irradiance_args(spheres, hits, grid, coeffs, valid,
                                                                params, weight)
    _check(lib().rtg_irradiance(device, _ptr(sph), len(sph), _ptr(src), n, _ptr(g), _ptr(c),
                                _ptr(v), _ptr(p), _ptr(dst), wp), "rtg_irradiance")
    return (out, w) if weight else out


def gather_params(samples: int, bias: float = 1e-3, seed: int = 0, flags: int = 0) -> np.ndarray:
    """One rtg_gather_params record (flags: GATHER_JITTER for a per-point window
    into the tables, GATHER_SKIP_NONFINITE to leave NaN and infinite colours out)."""
    p = np.zeros(1, GATHER_PARAMS_DTYPE)
    p[0] = (samples, bias, seed & 0xFFFFFFFF, flags)
    return p


def _gather_args(hits, dirs, weights, params):
    """Hit records, the two tables and params as contiguous arrays whose
    pointers are never null (an empty batch is legal), and the two counts; the
    weights are checked against the directions when given."""
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(params, GATHER_PARAMS_DTYPE).reshape(1)
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        if len(w) != len(d):
            raise RtgError(f"gather: {len(w)} weights for {len(d)} directions")
        w = w if len(w) else np.zeros(1, np.float32)
    return (h if len(h) else np.zeros(1, HIT_DTYPE)), len(h), \
        (d if len(d) else np.zeros((1, 3), np.float32)), len(d), w, p


def gather_rays_host(hits, dirs, params, threads: int = 1) -> np.ndarray:
    """The probe rays of every hit point on the host (rtg_gather_rays_host):
    (n * K, 6) float32 (origin, dir), point-major; params from gather_params()."""
    h, n, d, nd, _, p = _gather_args(hits, dirs, None, params)
    k = int(p["samples"][0])
    out = np.empty((n * k, 6), np.float32)
    dst = out if out.size else np.zeros((1, 6), np.float32)
    _check(lib().rtg_gather_rays_host(_ptr(h), n, _ptr(p), _ptr(d), nd, _ptr(dst), threads),
           "rtg_gather_rays_host")
    return out


def _gather_out(n: int, skipped: bool):
    out = np.empty((n, 3), np.float32)
    skp = np.empty(n, np.uint16) if skipped else None
    dst = out if n else np.zeros((1, 3), np.float32)
    sp = None if skp is None else ctypes.c_void_p((skp if n else np.zeros(1, np.uint16)).ctypes.data)
    return out, skp, dst, sp


def gather_host(spheres, lights, hits, dirs, weights, params, stack_size: int = 6,
                semantics: int = 0, walk: int = 0, threads: int = 1, skipped: bool = False):
    """The gather on the host (rtg_gather_host; no GPU needed): per HIT_DTYPE
    record the weighted sum of rayTrace's colour along its K probes, (n, 3)
    float32.  skipped=True: returns (sums, counts), counts the uint16 number of
    probes GATHER_SKIP_NONFINITE left out.  walk 0: plain loops; walk 1: the
    kernel's own path over the packed tables."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    h, n, d, nd, w, p = _gather_args(hits, dirs, weights, params)
    out, skp, dst, sp = _gather_out(n, skipped)
    _check(lib().rtg_gather_host(_ptr(spheres), len(spheres), _ptr(lights), len(lights), _ptr(h),
                                 n, _ptr(p), _ptr(d), _ptr(w), nd, stack_size, semantics,
                                 _ptr(dst), sp, walk, threads), "rtg_gather_host")
    return (out, skp) if skipped else out


def gather(spheres, lights, hits, dirs, weights, params, stack_size: int = 6, device: int = 0,
           skipped: bool = False):
    """The same on the GPU, one-shot (rtg_gather): HIT_DTYPE records as
    intersect() returns them in."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    h, n, d, nd, w, p = _gather_args(hits, dirs, weights, params)
    out, skp, dst, sp = _gather_out(n, skipped)
    _check(lib().rtg_gather(device, _ptr(spheres), len(spheres), _ptr(lights), len(lights),
                            _ptr(h), n, _ptr(p), _ptr(d), _ptr(w), nd, stack_size, _ptr(dst), sp),
           "rtg_gather")
    return (out, skp) if skipped else out


def filter_params(passes: int, kind: int = FILTER_RGB, flags: int = 0, plane_scale: float = 0.0,
                  normal_log2: int = 0) -> np.ndarray:
    """One rtg_filter_params record (kind: FILTER_RGB / GRAY / COUNT; flags:
    FILTER_SAME_ID | NORMAL | PLANE | SKIP_NONFINITE)."""
    p = np.zeros(1, FILTER_PARAMS_DTYPE)
    p[0] = (passes, normal_log2, plane_scale, kind, flags)
    return p


def filter_scratch(width: int, height: int, params) -> int:
    """Bytes of device scratch Context.filter_device needs for such a frame
    (rtg_filter_scratch): caller-owned, 16-byte aligned; 0 for one pass."""
    p = np.ascontiguousarray(params, FILTER_PARAMS_DTYPE).reshape(1)
    out = ctypes.c_size_t(0)
    _check(lib().rtg_filter_scratch(width, height, _ptr(p), ctypes.byref(out)),
           "rtg_filter_scratch")
    return out.value


def _filter_args(hits, width: int, height: int, params, src):
    """Hit records, params and the source as contiguous arrays of the kind's
    type, and the destination: (H, W, 3) float32 for RGB, (H, W) otherwise."""
    p = np.ascontiguousarray(params, FILTER_PARAMS_DTYPE).reshape(1)
    kind = int(p["kind"][0])
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    s = np.ascontiguousarray(src, np.uint16 if kind == FILTER_COUNT else np.float32).reshape(-1)
    n = width * height
    if len(h) != n or len(s) != n * (3 if kind == FILTER_RGB else 1):
        raise ValueError(f"filter: {len(h)} hit records and {len(s)} source words for a "
                         f"{width} x {height} frame of kind {kind}")
    out = np.empty((height, width, 3) if kind == FILTER_RGB else (height, width), np.float32)
    return h, p, s, out


def filter_host(hits, width: int, height: int, params, src, threads: int = 1) -> np.ndarray:
    """The edge-stopping a-trous filter on the host (rtg_filter_host; no GPU
    needed): HIT_DTYPE records of the frame's aa-1 primary rays as guides, src
    the frame's signal (float32 (H, W, 3) or (H, W), or uint16 counts), params
    from filter_params(); float32 out."""
    h, p, s, out = _filter_args(hits, width, height, params, src)
    _check(lib().rtg_filter_host(_ptr(h), width, height, _ptr(p), _ptr(s), _ptr(out), threads),
           "rtg_filter_host")
    return out


def filter(hits, width: int, height: int, params, src, device: int = 0) -> np.ndarray:  # noqa: A001
    """The same on the GPU, one-shot (rtg_filter)."""
    h, p, s, out = _filter_args(hits, width, height, params, src)
    _check(lib().rtg_filter(device, _ptr(h), width, height, _ptr(p), _ptr(s), _ptr(out)),
           "rtg_filter")
    return out


def accumulate_params(kind: int = FILTER_RGB, flags: int = 0, plane_scale: float = 0.0,
                      normal_log2: int = 0, max_history: int = 65535) -> np.ndarray:
    """One rtg_accumulate_params record (kind: FILTER_RGB / GRAY / COUNT; flags:
    ACCUM_SAME_ID | NORMAL | PLANE | SKIP_NONFINITE)."""
    p = np.zeros(1, ACCUM_PARAMS_DTYPE)
    p[0] = (kind, flags, normal_log2, plane_scale, max_history)
    return p


def _accumulate_args(hits, width: int, height: int, params, src, prev, m2: bool):
    """The current records, params and source as contiguous arrays, the previous
    state (None on a reset frame, else (camera, hits, acc, len[, m2])) likewise,
    and the outputs: acc (H, W, 3) or (H, W) float32, len (H, W) uint16, m2 as
    acc or None."""
    p = np.ascontiguousarray(params, ACCUM_PARAMS_DTYPE).reshape(1)
    kind = int(p["kind"][0])
    C = 3 if kind == FILTER_RGB else 1
    n = width * height
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    s = np.ascontiguousarray(src, np.uint16 if kind == FILTER_COUNT else np.float32).reshape(-1)
    if len(h) != n or len(s) != n * C:
        raise ValueError(f"accumulate: {len(h)} hit records and {len(s)} source words for a "
                         f"{width} x {height} frame of kind {kind}")
    pv = [None] * 5
    if prev is not None:
        pv[0] = np.ascontiguousarray(prev[0], CAMERA_DTYPE).reshape(1)
        pv[1] = np.ascontiguousarray(prev[1], HIT_DTYPE).reshape(-1)
        pv[2] = np.ascontiguousarray(prev[2], np.float32).reshape(-1)
        pv[3] = np.ascontiguousarray(prev[3], np.uint16).reshape(-1)
        if len(prev) > 4 and prev[4] is not None:
            pv[4] = np.ascontiguousarray(prev[4], np.float32).reshape(-1)
        if len(pv[1]) != n or len(pv[3]) != n or len(pv[2]) != n * C or \
                (pv[4] is not None and len(pv[4]) != n * C):
            raise ValueError(f"accumulate: previous state of another size than the "
                             f"{width} x {height} frame of kind {kind}")
    shape = (height, width, 3) if C == 3 else (height, width)
    acc = np.empty(shape, np.float32)
    ln = np.empty((height, width), np.uint16)
    return h, p, s, pv, acc, ln, (np.empty(shape, np.float32) if m2 else None)


def accumulate_host(hits, width: int, height: int, params, src, prev=None, zoom: float = -4.0,
                    m2: bool = False, threads: int = 1):
    """Temporal accumulation by reprojection on the host (rtg_accumulate_host; no
    GPU needed): HIT_DTYPE records of the current pose's aa-1 primary rays, src
    the current signal (float32 (H, W, 3) or (H, W), or uint16 counts), params
    from accumulate_params(), `prev` the previous frame's (camera, hits, acc,
    len[, m2]) or None for a reset frame.  Returns (acc, len) or, with m2, (acc,
    len, m2)."""
    h, p, s, pv, acc, ln, o2 = _accumulate_args(hits, width, height, params, src, prev, m2)
    _check(lib().rtg_accumulate_host(_ptr(h), width, height, _ptr(p), _ptr(s), _ptr(pv[0]),
                                     float(zoom), _ptr(pv[1]), _ptr(pv[2]), _ptr(pv[3]),
                                     _ptr(pv[4]), _ptr(acc), _ptr(ln), _ptr(o2), threads),
           "rtg_accumulate_host")
    return (acc, ln, o2) if m2 else (acc, ln)


def accumulate(hits, width: int, height: int, params, src, prev=None, zoom: float = -4.0,
               m2: bool = False, device: int = 0):
    """The same on the GPU, one-shot (rtg_accumulate)."""
    h, p, s, pv, acc, ln, o2 = _accumulate_args(hits, width, height, params, src, prev, m2)
    _check(lib().rtg_accumulate(device, _ptr(h), width, height, _ptr(p), _ptr(s), _ptr(pv[0]),
                                float(zoom), _ptr(pv[1]), _ptr(pv[2]), _ptr(pv[3]), _ptr(pv[4]),
                                _ptr(acc), _ptr(ln), _ptr(o2)),
           "rtg_accumulate")
    return (acc, ln, o2) if m2 else (acc, ln)


def upsample_params(scale_log2: int, kind: int = FILTER_RGB, flags: int = 0,
                    plane_scale: float = 0.0, normal_log2: int = 0) -> np.ndarray:
    """One rtg_upsample_params record (scale_log2 1..3; kind: FILTER_RGB / GRAY /
    COUNT; flags: UPSAMPLE_SAME_ID | NORMAL | PLANE | SKIP_NONFINITE)."""
    p = np.zeros(1, UPSAMPLE_PARAMS_DTYPE)
    p[0] = (kind, flags, normal_log2, plane_scale, scale_log2)
    return p


def upsample_scratch(width: int, height: int, with_holes: bool = True) -> int:
    """Bytes of device scratch Context.upsample_device needs for such a full
    frame (rtg_upsample_scratch): caller-owned, 16-byte aligned; 0 without a
    hole list."""
    out = ctypes.c_size_t(0)
    _check(lib().rtg_upsample_scratch(width, height, int(with_holes), ctypes.byref(out)),
           "rtg_upsample_scratch")
    return out.value


def _upsample_args(hits, width: int, height: int, params, low_hits, low_width: int,
                   low_height: int, low_src, holes):
    """The records, params and the low signal as contiguous arrays of the kind's
    type, the destination ((H, W, 3) float32 for RGB, (H, W) otherwise), and
    the list: `holes` None (no list), a capacity (a new array) or the caller's
    own uint32 array, written in place."""
    p = np.ascontiguousarray(params, UPSAMPLE_PARAMS_DTYPE).reshape(1)
    kind = int(p["kind"][0])
    C = 3 if kind == FILTER_RGB else 1
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    lh = np.ascontiguousarray(low_hits, HIT_DTYPE).reshape(-1)
    s = np.ascontiguousarray(low_src, np.uint16 if kind == FILTER_COUNT else np.float32).reshape(-1)
    nl = low_width * low_height
    if len(h) != width * height or len(lh) != nl or len(s) != nl * C:
        raise ValueError(f"upsample: {len(h)} records, {len(lh)} low records and {len(s)} low "
                         f"source words for a {width} x {height} frame over a "
                         f"{low_width} x {low_height} one of kind {kind}")
    out = np.empty((height, width, 3) if C == 3 else (height, width), np.float32)
    if holes is None:
        return h, p, lh, s, out, None, 0, None
    if isinstance(holes, np.ndarray):
        if holes.dtype != np.uint32 or not holes.flags.c_contiguous or not holes.flags.writeable:
            raise ValueError("upsample: holes is a writable contiguous uint32 array or a capacity")
        lst = holes.reshape(-1)
    else:
        lst = np.zeros(int(holes), np.uint32)
    return h, p, lh, s, out, lst, len(lst), np.zeros(1, np.uint32)


def _list_ptr(lst):
    """The list's address; a list of capacity 0 still has one."""
    if lst is None:
        return None, None
    keep = lst if lst.size else np.zeros(1, np.uint32)
    return keep, ctypes.c_void_p(keep.ctypes.data)


def upsample_host(hits, width: int, height: int, params, low_hits, low_width: int,
                  low_height: int, low_src, holes=None, threads: int = 1):
    """Guided upsampling on the host (rtg_upsample_host; no GPU needed): the full
    frame's HIT_DTYPE records, the low frame's records and signal (float32
    (Hl, Wl, 3) or (Hl, Wl), or uint16 counts), params from upsample_params().
    Returns the full frame, float32; with `holes` (a capacity, or a uint32
    array that is written in place) returns (frame, list, count): the list
    holds min(count, capacity) pixel indices in ascending order."""
    h, p, lh, s, out, lst, cap, cnt = _upsample_args(hits, width, height, params, low_hits,
                                                     low_width, low_height, low_src, holes)
    keep, lp = _list_ptr(lst)
    _check(lib().rtg_upsample_host(_ptr(h), width, height, _ptr(p), _ptr(lh), low_width,
                                   low_height, _ptr(s), _ptr(out), lp, cap,
                                   _ptr(cnt) if cnt is not None else None, threads),
           "rtg_upsample_host")
    return out if lst is None else (out, lst, int(cnt[0]))


def upsample(hits, width: int, height: int, params, low_hits, low_width: int, low_height: int,
             low_src, holes=None, device: int = 0):
    """The same on the GPU, one-shot (rtg_upsample)."""
    h, p, lh, s, out, lst, cap, cnt = _upsample_args(hits, width, height, params, low_hits,
                                                     low_width, low_height, low_src, holes)
    keep, lp = _list_ptr(lst)
    _check(lib().rtg_upsample(device, _ptr(h), width, height, _ptr(p), _ptr(lh), low_width,
                              low_height, _ptr(s), _ptr(out), lp, cap,
                              _ptr(cnt) if cnt is not None else None),
           "rtg_upsample")
    return out if lst is None else (out, lst, int(cnt[0]))


def hits_pick_host(hits, idx, threads: int = 1) -> np.ndarray:
    """out[i] = hits[idx[i]] on the host (rtg_hits_pick_host): HIT_DTYPE records
    and uint32 indices; an index >= len(hits) gives a miss record."""
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    ix = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    out = np.zeros(max(len(ix), 1), HIT_DTYPE)
    keep = ix if ix.size else np.zeros(1, np.uint32)
    _check(lib().rtg_hits_pick_host(_ptr(h), len(h), ctypes.c_void_p(keep.ctypes.data), len(ix),
                                    ctypes.c_void_p(out.ctypes.data), threads),
           "rtg_hits_pick_host")
    return out[:len(ix)]


def values_place_host(kind: int, vals, idx, dst, threads: int = 1) -> None:
    """dst[idx[i]] = vals[i] on the host, in place (rtg_values_place_host): vals of
    `kind` (float32 x 3, float32 or uint16 counts), dst a contiguous float32
    array of n values; an index >= n is skipped; the indices are distinct."""
    C = 3 if kind == FILTER_RGB else 1
    v = np.ascontiguousarray(vals, np.uint16 if kind == FILTER_COUNT else np.float32).reshape(-1)
    ix = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.float32 and dst.flags.c_contiguous
            and dst.flags.writeable) or dst.size % C or len(v) != len(ix) * C:
        raise ValueError("values_place: dst is a writable contiguous float32 array of n values "
                         "and vals holds one value per index")
    keep = ix if ix.size else np.zeros(1, np.uint32)
    kv = v if v.size else np.zeros(C, v.dtype)
    _check(lib().rtg_values_place_host(kind, ctypes.c_void_p(kv.ctypes.data),
                                       ctypes.c_void_p(keep.ctypes.data), len(ix), dst.size // C,
                                       ctypes.c_void_p(dst.ctypes.data), threads),
           "rtg_values_place_host")


def variance_params(kind: int = FILTER_RGB, flags: int = 0, plane_scale: float = 0.0,
                    normal_log2: int = 0, min_history: int = 4) -> np.ndarray:
    """One rtg_variance_params record (kind: FILTER_RGB / GRAY; flags:
    FILTER_SAME_ID | NORMAL | PLANE | SKIP_NONFINITE, the spatial window's tap
    rule; a hit pixel with len < min_history takes the spatial estimate)."""
    p = np.zeros(1, VARIANCE_PARAMS_DTYPE)
    p[0] = (kind, flags, normal_log2, plane_scale, min_history)
    return p


def _variance_args(hits, width: int, height: int, params, acc, m2, length):
    """The records, params and the accumulated state as contiguous arrays, and
    the destination: (H, W) float32."""
    p = np.ascontiguousarray(params, VARIANCE_PARAMS_DTYPE).reshape(1)
    C = 3 if int(p["kind"][0]) == FILTER_RGB else 1
    n = width * height
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    a = np.ascontiguousarray(acc, np.float32).reshape(-1)
    m = np.ascontiguousarray(m2, np.float32).reshape(-1)
    ln = np.ascontiguousarray(length, np.uint16).reshape(-1)
    if len(h) != n or len(a) != n * C or len(m) != n * C or len(ln) != n:
        raise ValueError(f"variance: {len(h)} hit records, {len(a)} and {len(m)} moment words and "
                         f"{len(ln)} lengths for a {width} x {height} frame of {C} channels")
    return h, p, a, m, ln, np.empty((height, width), np.float32)


def variance_host(hits, width: int, height: int, params, acc, m2, length,
                  threads: int = 1) -> np.ndarray:
    """One variance per pixel from accumulate's moments on the host
    (rtg_variance_host; no GPU needed): acc, m2 and length are accumulate's
    (acc, len, m2) of the frame, params from variance_params(); (H, W) float32
    out."""
    h, p, a, m, ln, out = _variance_args(hits, width, height, params, acc, m2, length)
    _check(lib().rtg_variance_host(_ptr(h), width, height, _ptr(p), _ptr(a), _ptr(m), _ptr(ln),
                                   _ptr(out), threads), "rtg_variance_host")
    return out


def variance(hits, width: int, height: int, params, acc, m2, length, device: int = 0) -> np.ndarray:
    """The same on the GPU, one-shot (rtg_variance)."""
    h, p, a, m, ln, out = _variance_args(hits, width, height, params, acc, m2, length)
    _check(lib().rtg_variance(device, _ptr(h), width, height, _ptr(p), _ptr(a), _ptr(m), _ptr(ln),
                              _ptr(out)), "rtg_variance")
    return out


def svgf_params(passes: int, kind: int = FILTER_RGB, flags: int = 0, plane_scale: float = 0.0,
                normal_log2: int = 0, sigma_l: float = 4.0, eps_l: float = 1e-6) -> np.ndarray:
    """One rtg_svgf_params record (kind: FILTER_RGB / GRAY; flags: the FILTER_*
    bits | SVGF_LUMA, the luminance term scaled by sigma_l and eps_l)."""
    p = np.zeros(1, SVGF_PARAMS_DTYPE)
    p[0] = (passes, normal_log2, plane_scale, kind, flags, sigma_l, eps_l)
    return p


def svgf_scratch(width: int, height: int, params) -> int:
    """Bytes of device scratch Context.svgf_device needs for such a frame
    (rtg_svgf_scratch): caller-owned, 16-byte aligned; 0 for one pass."""
    p = np.ascontiguousarray(params, SVGF_PARAMS_DTYPE).reshape(1)
    out = ctypes.c_size_t(0)
    _check(lib().rtg_svgf_scratch(width, height, _ptr(p), ctypes.byref(out)), "rtg_svgf_scratch")
    return out.value


def _svgf_args(hits, width: int, height: int, params, src, var):
    """The records, params, source and its variance as contiguous arrays, and
    the destinations: (H, W, 3) or (H, W) float32, and (H, W) float32."""
    p = np.ascontiguousarray(params, SVGF_PARAMS_DTYPE).reshape(1)
    C = 3 if int(p["kind"][0]) == FILTER_RGB else 1
    n = width * height
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    s = np.ascontiguousarray(src, np.float32).reshape(-1)
    v = np.ascontiguousarray(var, np.float32).reshape(-1)
    if len(h) != n or len(s) != n * C or len(v) != n:
        raise ValueError(f"svgf: {len(h)} hit records, {len(s)} source words and {len(v)} "
                         f"variances for a {width} x {height} frame of {C} channels")
    out = np.empty((height, width, 3) if C == 3 else (height, width), np.float32)
    return h, p, s, v, out, np.empty((height, width), np.float32)


def svgf_host(hits, width: int, height: int, params, src, var, threads: int = 1):
    """The variance-guided a-trous passes on the host (rtg_svgf_host; no GPU
    needed): src the frame's float32 signal, var its per-pixel variance
    (variance_host's), params from svgf_params().  Returns (dst, dst_var)."""
    h, p, s, v, out, vout = _svgf_args(hits, width, height, params, src, var)
    _check(lib().rtg_svgf_host(_ptr(h), width, height, _ptr(p), _ptr(s), _ptr(v), _ptr(out),
                               _ptr(vout), threads), "rtg_svgf_host")
    return out, vout


def svgf(hits, width: int, height: int, params, src, var, device: int = 0):
    """The same on the GPU, one-shot (rtg_svgf)."""
    h, p, s, v, out, vout = _svgf_args(hits, width, height, params, src, var)
    _check(lib().rtg_svgf(device, _ptr(h), width, height, _ptr(p), _ptr(s), _ptr(v), _ptr(out),
                          _ptr(vout)), "rtg_svgf")
    return out, vout


def _project_args(camera, points):
    c = np.ascontiguousarray(camera, CAMERA_DTYPE).reshape(1)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    return c, p, np.empty((len(p), 3), np.float32)


def camera_project_host(camera, width: int, height: int, points, zoom: float = -4.0,
                        threads: int = 1) -> np.ndarray:
    """Where the points lie in the pose's width x height frame
    (rtg_camera_project_host; no GPU needed): (n, 3) float32 rows {fx, fy, k};
    a point is in front of the camera exactly when k > 0."""
    c, p, out = _project_args(camera, points)
    _check(lib().rtg_camera_project_host(_ptr(c), width, height, float(zoom), _ptr(p), len(p),
                                         _ptr(out), threads), "rtg_camera_project_host")
    return out


def camera_project(camera, width: int, height: int, points, zoom: float = -4.0,
                   device: int = 0) -> np.ndarray:
    """The same on the GPU, one-shot (rtg_camera_project)."""
    c, p, out = _project_args(camera, points)
    _check(lib().rtg_camera_project(device, _ptr(c), width, height, float(zoom), _ptr(p), len(p),
                                    _ptr(out)), "rtg_camera_project")
    return out


def _points(points):
    """Points as a contiguous (n, 3) float32 array, n, the int32 result and
    pointers that are never null for an empty batch."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    out = np.empty(n, np.int32)
    return (p if n else np.zeros((1, 3), np.float32)), n, out, (out if n else np.zeros(1, np.int32))


def contains_host(spheres, points, walk: int = 0, threads: int = 1) -> np.ndarray:
    """The containing sphere of every point on the host (rtg_contains_host; no
    GPU needed): int32, primaryContainer's lowest index or -1.  walk 0: the
    literal loop; walk 1: the kernel's own path."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    src, n, out, dst = _points(points)
    _check(lib().rtg_contains_host(_ptr(spheres), len(spheres), _ptr(src), n, _ptr(dst), walk,
                                   threads), "rtg_contains_host")
    return out


def contains(spheres, points, device: int = 0) -> np.ndarray:
    """The same on the GPU, one-shot (rtg_contains)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    src, n, out, dst = _points(points)
    _check(lib().rtg_contains(device, _ptr(spheres), len(spheres), _ptr(src), n, _ptr(dst)),
           "rtg_contains")
    return out


class MultiContext:
    """Persistent multi-device handle (rtg_multi_*): RCCL communicator, contexts,
    streams and buffers kept across frames."""

    def __init__(self, devices=(0,)):
        self._h = ctypes.c_void_p()
        self._devs = np.ascontiguousarray(devices, np.int32)
        _check(lib().rtg_multi_create(_ptr(self._devs), len(self._devs), ctypes.byref(self._h)),
               "rtg_multi_create")

    def set_scene(self, spheres, lights):
        self._sph = np.ascontiguousarray(spheres, SPHERE_DTYPE)
        self._lgt = np.ascontiguousarray(lights, LIGHT_DTYPE)
        _check(lib().rtg_multi_set_scene(self._h, _ptr(self._sph), len(self._sph),
                                         _ptr(self._lgt), len(self._lgt)), "rtg_multi_set_scene")

    GATHER_RCCL, GATHER_PEER_COPY = 0, 1  # RTG_GATHER_*

    def set_gather(self, mode: int):
        """RCCL gather + assemble (default) or the peer-copy ablation."""
        _check(lib().rtg_multi_set_gather(self._h, int(mode)), "rtg_multi_set_gather")

    def render(self, width, height, zoom=-4.0, alias_factor=3.0, stack_size=6, row_block=16):
        out = np.empty((height, width, 3), np.float32)
        tm = np.zeros(3, np.float32)
        _check(lib().rtg_multi_render(self._h, width, height, float(zoom), float(alias_factor),
                                      stack_size, row_block, _ptr(out), _ptr(tm)),
               "rtg_multi_render")
        return out, [float(v) for v in tm]

    def close(self):
        if self._h:
            lib().rtg_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def render_rows(spheres, lights, width: int, height: int, rows, zoom: float = -4.0,
                alias_factor: float = 3.0, stack_size: int = 6, device: int = 0) -> np.ndarray:
    """Render only the listed global rows; returns (len(rows), W, 3)."""
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    lights = np.ascontiguousarray(lights, LIGHT_DTYPE)
    rows = np.ascontiguousarray(rows, np.uint32)
    out = np.empty((len(rows), width, 3), np.float32)
    _check(lib().rtg_render_rows(device, _ptr(spheres), len(spheres), _ptr(lights),
                                 len(lights), width, height, float(zoom), float(alias_factor),
                                 stack_size, _ptr(rows), len(rows), _ptr(out)),
           "rtg_render_rows")
    return out


class Context:
    """Persistent device context: scene resident in HBM, renders into caller
    device memory (e.g. a torch tensor's data_ptr()) on a caller stream."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        _check(lib().rtg_context_create(device, ctypes.byref(self._h)), "rtg_context_create")
        self.device = device

    def close(self):
        if self._h:
            lib().rtg_context_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, spheres, lights):
        self._sph = np.ascontiguousarray(spheres, SPHERE_DTYPE)
        self._lgt = np.ascontiguousarray(lights, LIGHT_DTYPE)
        _check(lib().rtg_context_set_scene(self._h, _ptr(self._sph), len(self._sph),
                                           _ptr(self._lgt), len(self._lgt)),
               "rtg_context_set_scene")

    def scene_stats(self):
        """{prep_ms, upload_ms, device_bytes, bvh_nodes} of the last set_scene."""
        if not hasattr(lib(), "rtg_context_scene_stats"):  # an older RTG_LIB build
            return {"prep_ms": 0.0, "upload_ms": 0.0, "device_bytes": 0, "bvh_nodes": 0}
        out = (ctypes.c_double * 4)()
        _check(lib().rtg_context_scene_stats(self._h, ctypes.cast(out, ctypes.c_void_p)),
               "rtg_context_scene_stats")
        return {"prep_ms": out[0], "upload_ms": out[1], "device_bytes": int(out[2]),
                "bvh_nodes": int(out[3])}

    LAUNCH_TIMELINE = 1  # RTG_LAUNCH_TIMELINE
    LAUNCH_NO_ORDER_FEEDBACK = 2  # RTG_LAUNCH_NO_ORDER_FEEDBACK
    SEMANTICS_CPU, SEMANTICS_OPENCL = 0, 1  # RTG_SEMANTICS_*

    def set_semantics(self, semantics: int):
        """CPU path (default, bit-exact) or the reference OpenCL kernel's semantics."""
        _check(lib().rtg_context_set_semantics(self._h, int(semantics)),
               "rtg_context_set_semantics")

    def set_variant(self, variant: int, flags: int = 0):
        opts = (ctypes.c_int * 8)(variant, flags, 0, 0, 0, 0, 0, 0)
        _check(lib().rtg_set_launch_opts(self._h, ctypes.cast(opts, ctypes.c_void_p)),
               "rtg_set_launch_opts")

    def diag_read(self, reset: bool = True):
        out = (ctypes.c_ulonglong * 8)()
        _check(lib().rtg_diag_read(self._h, ctypes.cast(out, ctypes.c_void_p), int(reset)),
               "rtg_diag_read")
        return [int(v) for v in out]

    def diag_counts(self, reset: bool = True):
        """Executed-work unit counters of the counting build (variant 120):
        (wave-level, lane-level) arrays indexed by UNIT_NAMES."""
        n = lib().rtg_diag_counts(self._h, None, 0, 0)
        if n < 0:
            _check(n, "rtg_diag_counts")
        out = (ctypes.c_ulonglong * n)()
        rc = lib().rtg_diag_counts(self._h, ctypes.cast(out, ctypes.c_void_p), n, int(reset))
        if rc < 0:
            _check(rc, "rtg_diag_counts")
        v = np.array(out[:], np.int64)
        return v[:n // 2], v[n // 2:]

    def diag_timeline(self, cap: int = 1 << 20) -> np.ndarray:
        """Per-wave records {start, end, HW_ID, XCC_ID} of the last timeline-variant launch."""
        out = np.zeros((cap, 4), np.uint32)
        cnt = ctypes.c_size_t(0)
        _check(lib().rtg_diag_timeline(self._h, ctypes.c_void_p(out.ctypes.data), cap,
                                       ctypes.byref(cnt)), "rtg_diag_timeline")
        return out[:min(cap, cnt.value)]

    def diag_group_list(self, cap: int = 1 << 26):
        """The last compacted launch: {cost[groups], list[listed], sel[listed],
        runs[4]}, list and sel in the trace kernel's order (rtg_diag_group_list;
        costs in 100 MHz ticks)."""
        n = ctypes.c_size_t(0)
        _check(lib().rtg_diag_group_list(self._h, None, None, None, None, 0, ctypes.byref(n)),
               "rtg_diag_group_list")
        g = min(cap, n.value)
        cost = np.zeros(g, np.uint32)
        lst = np.zeros(g, np.uint32)
        sel = np.zeros(g, np.uint64)
        runs = np.zeros(4, np.uint32)
        _check(lib().rtg_diag_group_list(self._h, ctypes.c_void_p(cost.ctypes.data),
                                         ctypes.c_void_p(lst.ctypes.data),
                                         ctypes.c_void_p(sel.ctypes.data),
                                         ctypes.c_void_p(runs.ctypes.data), g, ctypes.byref(n)),
               "rtg_diag_group_list")
        k = int(runs.sum())
        return {"cost": cost, "list": lst[:k], "sel": sel[:k], "runs": runs}

    def render_device(self, width, height, dst_ptr: int, zoom=-4.0, alias_factor=3.0,
                      stack_size=6, row_block=16, shard=0, n_shards=1, stream: int = 0):
        _check(lib().rtg_render_device(self._h, width, height, float(zoom),
                                       float(alias_factor), stack_size, row_block, shard,
                                       n_shards, ctypes.c_void_p(dst_ptr),
                                       ctypes.c_void_p(stream) if stream else None),
               "rtg_render_device")

    def gbuffer_device(self, width, height, dst_ptr: int, zoom=-4.0, alias_factor=3.0,
                       row_block=16, shard=0, n_shards=1, stream: int = 0):
        """Primary-hit G-buffer of the resident scene into device memory
        (GBUF_DTYPE records, the shard's rows packed as render_device packs them)."""
        _check(lib().rtg_gbuffer_device(self._h, width, height, float(zoom),
                                        float(alias_factor), row_block, shard, n_shards,
                                        ctypes.c_void_p(dst_ptr),
                                        ctypes.c_void_p(stream) if stream else None),
               "rtg_gbuffer_device")

    def ray_order(self, rays_ptr: int, n: int, order_ptr: int, scratch_ptr: int,
                  scratch_bytes: int, kind: int = 0, keys_ptr: int = 0, stream: int = 0):
        """The coherence order of n rays (kind ORDER_RAYS) or segments
        (ORDER_SEGMENTS) at rays_ptr (device, 24-byte records) into order_ptr
        (device, n uint32) and, when keys_ptr is given, their keys (device, n
        uint64, batch order), asynchronously on `stream` (rtg_ray_order_device).
        scratch_ptr: ray_order_scratch(n) bytes of device memory, 16-byte
        aligned.  Pass the order as order= to intersect_device, visible_device
        or raytrace_device."""
        _check(lib().rtg_ray_order_device(self._h, ctypes.c_void_p(rays_ptr), n, kind,
                                          ctypes.c_void_p(order_ptr),
                                          ctypes.c_void_p(keys_ptr) if keys_ptr else None,
                                          ctypes.c_void_p(scratch_ptr), scratch_bytes,
                                          ctypes.c_void_p(stream) if stream else None),
               "rtg_ray_order_device")

    def intersect_device(self, rays_ptr: int, n: int, dst_ptr: int, stream: int = 0,
                         order: int = 0):
        """Closest hits of n rays at rays_ptr (device, 24-byte RAY_DTYPE records:
        an (N, 6) float32 tensor) into dst_ptr (device, 32-byte HIT_DTYPE records,
        16-byte aligned: an (N, 8) int32 tensor), asynchronously on `stream`.
        order: a device pointer to n uint32 indices (rtg_intersect_indexed_device:
        lane k takes ray order[k]; the results stay in the caller's order)."""
        if order:
            _check(lib().rtg_intersect_indexed_device(self._h, ctypes.c_void_p(rays_ptr),
                                                      ctypes.c_void_p(order), n,
                                                      ctypes.c_void_p(dst_ptr),
                                                      ctypes.c_void_p(stream) if stream else None),
                   "rtg_intersect_indexed_device")
            return
        _check(lib().rtg_intersect_device(self._h, ctypes.c_void_p(rays_ptr), n,
                                          ctypes.c_void_p(dst_ptr),
                                          ctypes.c_void_p(stream) if stream else None),
               "rtg_intersect_device")

    def visible_device(self, segs_ptr: int, n: int, dst_ptr: int, stream: int = 0,
                       order: int = 0):
        """Line of sight of n segments at segs_ptr (device, 24-byte SEGMENT_DTYPE
        records) into dst_ptr (device, one uint8 per segment: 1 visible).
        order: as intersect_device (rtg_visible_indexed_device)."""
        if order:
            _check(lib().rtg_visible_indexed_device(self._h, ctypes.c_void_p(segs_ptr),
                                                    ctypes.c_void_p(order), n,
                                                    ctypes.c_void_p(dst_ptr),
                                                    ctypes.c_void_p(stream) if stream else None),
                   "rtg_visible_indexed_device")
            return
        _check(lib().rtg_visible_device(self._h, ctypes.c_void_p(segs_ptr), n,
                                        ctypes.c_void_p(dst_ptr),
                                        ctypes.c_void_p(stream) if stream else None),
               "rtg_visible_device")

    def raytrace_device(self, rays_ptr: int, n: int, dst_ptr: int, stack_size: int = 6,
                        stream: int = 0, order: int = 0):
        """rayTrace's colours of n rays at rays_ptr (device, 24-byte RAY_DTYPE
        records) into dst_ptr (device, an (N, 3) float32 tensor), asynchronously
        on `stream`, under the context's semantics.  order: as intersect_device
        (rtg_raytrace_indexed_device)."""
        if order:
            _check(lib().rtg_raytrace_indexed_device(self._h, ctypes.c_void_p(rays_ptr),
                                                     ctypes.c_void_p(order), n, stack_size,
                                                     ctypes.c_void_p(dst_ptr),
                                                     ctypes.c_void_p(stream) if stream else None),
                   "rtg_raytrace_indexed_device")
            return
        _check(lib().rtg_raytrace_device(self._h, ctypes.c_void_p(rays_ptr), n, stack_size,
                                         ctypes.c_void_p(dst_ptr),
                                         ctypes.c_void_p(stream) if stream else None),
               "rtg_raytrace_device")

    def render_camera(self, cam, width, height, dst_ptr: int, zoom=-4.0, alias_factor=3.0,
                      stack_size=6, stream: int = 0):
        """The posed camera's whole frame of the resident scene into dst_ptr
        (device, an (H, W, 3) float32 tensor), asynchronously on `stream`, under
        the context's semantics (rtg_render_camera_device)."""
        c = _camera(cam)
        _check(lib().rtg_render_camera_device(self._h, _ptr(c), width, height, float(zoom),
                                              float(alias_factor), stack_size,
                                              ctypes.c_void_p(dst_ptr),
                                              ctypes.c_void_p(stream) if stream else None),
               "rtg_render_camera_device")

    def render_views(self, cams_ptr: int, n_views: int, width, height, dst_ptr: int, zoom=-4.0,
                     alias_factor=3.0, stack_size=6, stream: int = 0):
        """n_views posed frames of the resident scene in one launch: the poses at
        cams_ptr (DEVICE, n_views 48-byte CAMERA_DTYPE records: an (n, 12) float32
        tensor), the frames into dst_ptr (device, an (n, H, W, 3) float32 tensor),
        asynchronously on `stream` (rtg_render_views_device)."""
        _check(lib().rtg_render_views_device(self._h, ctypes.c_void_p(cams_ptr), n_views, width,
                                             height, float(zoom), float(alias_factor), stack_size,
                                             ctypes.c_void_p(dst_ptr),
                                             ctypes.c_void_p(stream) if stream else None),
               "rtg_render_views_device")

    def views_fold(self, frames_ptr: int, n_views: int, width, height, params, weights_ptr: int,
                   dst_ptr: int, scratch_ptr: int, scratch_bytes: int, skipped_ptr: int = 0,
                   stream: int = 0):
        """Groups of n_views frames at frames_ptr (device, (n, H, W, 3) float32,
        render_views' or the caller's own) folded by the weight table at
        weights_ptr (device, G * H * W * K float32) into dst_ptr (device, (nGroups,
        K, 3) float32) and, if given, skipped_ptr (nGroups uint32), asynchronously
        on `stream` (rtg_views_fold_device; params from fold_params(), the scratch
        views_fold_scratch() bytes, 16-byte aligned; the context needs no scene)."""
        p = np.ascontiguousarray(params, FOLD_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_views_fold_device(self._h, ctypes.c_void_p(frames_ptr), n_views, width,
                                           height, _ptr(p), ctypes.c_void_p(weights_ptr),
                                           ctypes.c_void_p(dst_ptr), ctypes.c_void_p(skipped_ptr),
                                           ctypes.c_void_p(scratch_ptr), scratch_bytes,
                                           ctypes.c_void_p(stream) if stream else None),
               "rtg_views_fold_device")

    def render_views_fold(self, cams_ptr: int, n_views: int, width, height, params,
                          weights_ptr: int, dst_ptr: int, scratch_ptr: int, scratch_bytes: int,
                          skipped_ptr: int = 0, zoom=-4.0, alias_factor=3.0, stack_size=6,
                          stream: int = 0):
        """The fused call: n_views poses at cams_ptr (device, as render_views takes
        them) rendered and folded in one launch plus a small second kernel, no
        frame written anywhere (rtg_render_views_fold_device); the other
        arguments as views_fold."""
        p = np.ascontiguousarray(params, FOLD_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_render_views_fold_device(
            self._h, ctypes.c_void_p(cams_ptr), n_views, width, height, float(zoom),
            float(alias_factor), stack_size, _ptr(p), ctypes.c_void_p(weights_ptr),
            ctypes.c_void_p(dst_ptr), ctypes.c_void_p(skipped_ptr), ctypes.c_void_p(scratch_ptr),
            scratch_bytes, ctypes.c_void_p(stream) if stream else None),
            "rtg_render_views_fold_device")

    def camera_rays(self, cam, width, height, dst_ptr: int, zoom=-4.0, alias_factor=3.0,
                    stream: int = 0):
        """The posed camera's sample rays into dst_ptr (device, W*H*nAA*nAA 24-byte
        RAY_DTYPE records: an (N, 6) float32 tensor), asynchronously on `stream`
        (rtg_camera_rays_device; the context needs no scene)."""
        c = _camera(cam)
        _check(lib().rtg_camera_rays_device(self._h, _ptr(c), width, height, float(zoom),
                                            float(alias_factor), ctypes.c_void_p(dst_ptr),
                                            ctypes.c_void_p(stream) if stream else None),
               "rtg_camera_rays_device")

    def ao_device(self, hits_ptr: int, n: int, params, dirs_ptr: int, n_dirs: int, dst_ptr: int,
                  stream: int = 0):
        """Ambient occlusion of n hit points at hits_ptr (device, 32-byte HIT_DTYPE
        records as intersect_device writes them) with the direction table at
        dirs_ptr (device, an (n_dirs, 3) float32 tensor) into dst_ptr (device, n
        uint16 counts of unoccluded probes), asynchronously on `stream`
        (rtg_ao_device; params from ao_params())."""
        p = np.ascontiguousarray(params, AO_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_ao_device(self._h, ctypes.c_void_p(hits_ptr), n, _ptr(p),
                                   ctypes.c_void_p(dirs_ptr), n_dirs, ctypes.c_void_p(dst_ptr),
                                   ctypes.c_void_p(stream) if stream else None),
               "rtg_ao_device")

    def ao_segments_device(self, hits_ptr: int, n: int, params, dirs_ptr: int, n_dirs: int,
                           dst_ptr: int, stream: int = 0):
        """The n * K probe segments of those points into dst_ptr (device, 24-byte
        SEGMENT_DTYPE records, point-major), asynchronously on `stream`
        (rtg_ao_segments_device; the context needs no scene)."""
        p = np.ascontiguousarray(params, AO_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_ao_segments_device(self._h, ctypes.c_void_p(hits_ptr), n, _ptr(p),
                                            ctypes.c_void_p(dirs_ptr), n_dirs,
                                            ctypes.c_void_p(dst_ptr),
                                            ctypes.c_void_p(stream) if stream else None),
               "rtg_ao_segments_device")

    def filter_device(self, hits_ptr: int, width: int, height: int, params, src_ptr: int,
                      dst_ptr: int, scratch_ptr: int = 0, scratch_bytes: int = 0,
                      stream: int = 0):
        """The edge-stopping a-trous filter of a width x height frame: guides at
        hits_ptr (device, 32-byte HIT_DTYPE records as intersect_device writes
        them), the signal at src_ptr (device; float32 x 3, float32 or uint16 per
        pixel by params' kind) into dst_ptr (device, float32 per channel),
        asynchronously on `stream` (rtg_filter_device; params from
        filter_params(), the scratch filter_scratch() bytes, 16-byte aligned; the
        context needs no scene)."""
        p = np.ascontiguousarray(params, FILTER_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_filter_device(self._h, ctypes.c_void_p(hits_ptr), width, height, _ptr(p),
                                       ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr),
                                       ctypes.c_void_p(scratch_ptr), scratch_bytes,
                                       ctypes.c_void_p(stream) if stream else None),
               "rtg_filter_device")

    def accumulate_device(self, hits_ptr: int, width: int, height: int, params, src_ptr: int,
                          out_acc_ptr: int, out_len_ptr: int, prev=None, zoom: float = -4.0,
                          out_m2_ptr: int = 0, stream: int = 0):
        """Temporal accumulation by reprojection of a width x height frame: the
        current records at hits_ptr and signal at src_ptr (device, as
        filter_device takes them), `prev` the previous frame's (camera,
        hits_ptr, acc_ptr, len_ptr[, m2_ptr]) or None for a reset frame, into
        out_acc_ptr (float32 per channel), out_len_ptr (uint16) and, when given,
        out_m2_ptr, asynchronously on `stream` (rtg_accumulate_device; params
        from accumulate_params(); the context needs no scene)."""
        p = np.ascontiguousarray(params, ACCUM_PARAMS_DTYPE).reshape(1)
        cam = None if prev is None or prev[0] is None else \
            np.ascontiguousarray(prev[0], CAMERA_DTYPE).reshape(1)
        pv = [0, 0, 0, 0] if prev is None else (list(prev[1:]) + [0])[:4]
        v = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
        _check(lib().rtg_accumulate_device(self._h, v(hits_ptr), width, height, _ptr(p),
                                           v(src_ptr), _ptr(cam), float(zoom), v(pv[0]), v(pv[1]),
                                           v(pv[2]), v(pv[3]), v(out_acc_ptr), v(out_len_ptr),
                                           v(out_m2_ptr), v(stream)),
               "rtg_accumulate_device")

    def upsample_device(self, hits_ptr: int, width: int, height: int, params, low_hits_ptr: int,
                        low_width: int, low_height: int, low_src_ptr: int, dst_ptr: int,
                        holes_ptr: int = 0, hole_cap: int = 0, hole_count_ptr: int = 0,
                        scratch_ptr: int = 0, scratch_bytes: int = 0, stream: int = 0):
        """Guided upsampling of a low_width x low_height signal at low_src_ptr to
        the width x height frame at dst_ptr (float32 per channel): the full
        records at hits_ptr and the low ones at low_hits_ptr (device, as
        filter_device takes them); with holes_ptr (uint32 x hole_cap) and
        hole_count_ptr (one uint32) also the hole list, which needs the scratch
        of upsample_scratch() bytes, 16-byte aligned; asynchronously on `stream`
        (rtg_upsample_device; params from upsample_params(); the context needs
        no scene)."""
        p = np.ascontiguousarray(params, UPSAMPLE_PARAMS_DTYPE).reshape(1)
        v = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
        _check(lib().rtg_upsample_device(self._h, v(hits_ptr), width, height, _ptr(p),
                                         v(low_hits_ptr), low_width, low_height, v(low_src_ptr),
                                         v(dst_ptr), v(holes_ptr), hole_cap, v(hole_count_ptr),
                                         v(scratch_ptr), scratch_bytes, v(stream)),
               "rtg_upsample_device")

    def hits_pick_device(self, hits_ptr: int, n: int, idx_ptr: int, m: int, out_ptr: int,
                         stream: int = 0):
        """out[i] = hits[idx[i]] for i < m: n HIT_DTYPE records at hits_ptr, m
        uint32 indices at idx_ptr, m records into out_ptr (device, 16-byte
        aligned), asynchronously on `stream` (rtg_hits_pick_device; an index >= n
        gives a miss record)."""
        v = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
        _check(lib().rtg_hits_pick_device(self._h, v(hits_ptr), n, v(idx_ptr), m, v(out_ptr),
                                          v(stream)),
               "rtg_hits_pick_device")

    def values_place_device(self, kind: int, vals_ptr: int, idx_ptr: int, m: int, n: int,
                            dst_ptr: int, stream: int = 0):
        """dst[idx[i]] = vals[i] for i < m: m values of `kind` at vals_ptr into the
        n float32 values (x 3 for RGB) at dst_ptr, asynchronously on `stream`
        (rtg_values_place_device; an index >= n is skipped, the indices are
        distinct)."""
        v = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
        _check(lib().rtg_values_place_device(self._h, kind, v(vals_ptr), v(idx_ptr), m, n,
                                             v(dst_ptr), v(stream)),
               "rtg_values_place_device")

    def variance_device(self, hits_ptr: int, width: int, height: int, params, acc_ptr: int,
                        m2_ptr: int, len_ptr: int, var_ptr: int, stream: int = 0):
        """One variance per pixel of a width x height frame from the accumulated
        state at acc_ptr, m2_ptr (float32 per channel) and len_ptr (uint16),
        accumulate_device's outputs, into var_ptr (device, float32 per pixel),
        asynchronously on `stream` (rtg_variance_device; params from
        variance_params(); the context needs no scene)."""
        p = np.ascontiguousarray(params, VARIANCE_PARAMS_DTYPE).reshape(1)
        v = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
        _check(lib().rtg_variance_device(self._h, v(hits_ptr), width, height, _ptr(p), v(acc_ptr),
                                         v(m2_ptr), v(len_ptr), v(var_ptr), v(stream)),
               "rtg_variance_device")

    def svgf_device(self, hits_ptr: int, width: int, height: int, params, src_ptr: int,
                    var_ptr: int, dst_ptr: int, dst_var_ptr: int, scratch_ptr: int = 0,
                    scratch_bytes: int = 0, stream: int = 0):
        """The variance-guided a-trous passes of a width x height frame: the signal
        at src_ptr (float32 per channel) and its variance at var_ptr (float32 per
        pixel) into dst_ptr and dst_var_ptr, asynchronously on `stream`
        (rtg_svgf_device; params from svgf_params(), the scratch svgf_scratch()
        bytes, 16-byte aligned; the context needs no scene)."""
        p = np.ascontiguousarray(params, SVGF_PARAMS_DTYPE).reshape(1)
        v = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
        _check(lib().rtg_svgf_device(self._h, v(hits_ptr), width, height, _ptr(p), v(src_ptr),
                                     v(var_ptr), v(dst_ptr), v(dst_var_ptr), v(scratch_ptr),
                                     scratch_bytes, v(stream)),
               "rtg_svgf_device")

    def camera_project_device(self, camera, width: int, height: int, points_ptr: int, n: int,
                              dst_ptr: int, zoom: float = -4.0, stream: int = 0):
        """Where n points at points_ptr (device, an (n, 3) float32 tensor) lie in
        the pose's frame, into dst_ptr (device, (n, 3) float32 rows {fx, fy, k}),
        asynchronously on `stream` (rtg_camera_project_device; the context needs
        no scene)."""
        c = np.ascontiguousarray(camera, CAMERA_DTYPE).reshape(1)
        _check(lib().rtg_camera_project_device(self._h, _ptr(c), width, height, float(zoom),
                                               ctypes.c_void_p(points_ptr), n,
                                               ctypes.c_void_p(dst_ptr),
                                               ctypes.c_void_p(stream) if stream else None),
               "rtg_camera_project_device")

    def matte_device(self, hits_ptr: int, n: int, dst_ptr: int, lit_ptr: int = 0,
                     stream: int = 0):
        """Direct light of n hit points at hits_ptr (device, 32-byte HIT_DTYPE
        records as intersect_device writes them) under the resident scene's
        lights into dst_ptr (device, an (N, 3) float32 tensor) and, when lit_ptr
        is given, the masks of the lights that reach each point (device, n
        uint64), asynchronously on `stream` (rtg_matte_device)."""
        _check(lib().rtg_matte_device(self._h, ctypes.c_void_p(hits_ptr), n,
                                      ctypes.c_void_p(dst_ptr),
                                      ctypes.c_void_p(lit_ptr) if lit_ptr else None,
                                      ctypes.c_void_p(stream) if stream else None),
               "rtg_matte_device")

    def irradiance_device(self, hits_ptr: int, n: int, grid, coeffs_ptr: int, params,
                          dst_ptr: int, valid_ptr: int = 0, weight_ptr: int = 0, stream: int = 0):
        """The light of the probe grid `grid` (probe_grid()) at n hit points at
        hits_ptr (device, 32-byte HIT_DTYPE records as intersect_device writes
        them), with the coefficients at coeffs_ptr (device, (nx * ny * nz * K, 3)
        float32 as render_views_fold writes them) and, with IRR_VALID, the
        validity bytes at valid_ptr (device, one uint8 per probe), into dst_ptr
        (device, an (N, 3) float32 tensor) and, when weight_ptr is given, the
        weights (device, n float32), asynchronously on `stream`
        (rtg_irradiance_device; params from irradiance_params()).  The context
        needs a scene only with IRR_VISIBLE."""
        g = _grid(grid)
        p = np.ascontiguousarray(params, IRR_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_irradiance_device(self._h, ctypes.c_void_p(hits_ptr), n, _ptr(g),
                                           ctypes.c_void_p(coeffs_ptr),
                                           ctypes.c_void_p(valid_ptr) if valid_ptr else None,
                                           _ptr(p), ctypes.c_void_p(dst_ptr),
                                           ctypes.c_void_p(weight_ptr) if weight_ptr else None,
                                           ctypes.c_void_p(stream) if stream else None),
               "rtg_irradiance_device")

    def gather_device(self, hits_ptr: int, n: int, params, dirs_ptr: int, weights_ptr: int,
                      n_dirs: int, dst_ptr: int, skipped_ptr: int = 0, stack_size: int = 6,
                      stream: int = 0):
        """The gather of n hit points at hits_ptr (device, 32-byte HIT_DTYPE records
        as intersect_device writes them) with the direction table at dirs_ptr
        (device, (n_dirs, 3) float32) and the weights at weights_ptr (device,
        n_dirs float32) into dst_ptr (device, an (N, 3) float32 tensor) and, when
        skipped_ptr is given, the counts of skipped probes (device, n uint16),
        asynchronously on `stream`, under the context's semantics
        (rtg_gather_device; params from gather_params())."""
        p = np.ascontiguousarray(params, GATHER_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_gather_device(self._h, ctypes.c_void_p(hits_ptr), n, _ptr(p),
                                       ctypes.c_void_p(dirs_ptr), ctypes.c_void_p(weights_ptr),
                                       n_dirs, stack_size, ctypes.c_void_p(dst_ptr),
                                       ctypes.c_void_p(skipped_ptr) if skipped_ptr else None,
                                       ctypes.c_void_p(stream) if stream else None),
               "rtg_gather_device")

    def gather_rays_device(self, hits_ptr: int, n: int, params, dirs_ptr: int, n_dirs: int,
                           dst_ptr: int, stream: int = 0):
        """The n * K probe rays of those points into dst_ptr (device, 24-byte
        RAY_DTYPE records, point-major), asynchronously on `stream`
        (rtg_gather_rays_device; the context needs no scene)."""
        p = np.ascontiguousarray(params, GATHER_PARAMS_DTYPE).reshape(1)
        _check(lib().rtg_gather_rays_device(self._h, ctypes.c_void_p(hits_ptr), n, _ptr(p),
                                            ctypes.c_void_p(dirs_ptr), n_dirs,
                                            ctypes.c_void_p(dst_ptr),
                                            ctypes.c_void_p(stream) if stream else None),
               "rtg_gather_rays_device")

    def contains_device(self, points_ptr: int, n: int, dst_ptr: int, stream: int = 0):
        """The containing sphere of n points at points_ptr (device, an (N, 3)
        float32 tensor) into dst_ptr (device, n int32: the lowest index or -1),
        asynchronously on `stream` (rtg_contains_device)."""
        _check(lib().rtg_contains_device(self._h, ctypes.c_void_p(points_ptr), n,
                                         ctypes.c_void_p(dst_ptr),
                                         ctypes.c_void_p(stream) if stream else None),
               "rtg_contains_device")

    def render_rows_device(self, width, height, rows_ptr: int, n_rows: int, dst_ptr: int,
                           zoom=-4.0, alias_factor=3.0, stack_size=6, stream: int = 0):
        """Render the global rows listed at rows_ptr (device uint32[n_rows])."""
        _check(lib().rtg_render_rows_device(self._h, width, height, float(zoom),
                                            float(alias_factor), stack_size,
                                            ctypes.c_void_p(rows_ptr), n_rows,
                                            ctypes.c_void_p(dst_ptr),
                                            ctypes.c_void_p(stream) if stream else None),
               "rtg_render_rows_device")

    def max_colour_device(self, src_ptr: int, n_pixels: int, dst_ptr: int, stream: int = 0):
        _check(lib().rtg_max_colour_device(self._h, ctypes.c_void_p(src_ptr), n_pixels,
                                           ctypes.c_void_p(dst_ptr),
                                           ctypes.c_void_p(stream) if stream else None),
               "rtg_max_colour_device")

    def assemble_shards_device(self, gathered_ptr: int, n_shards: int, padded_rows: int,
                               width: int, height: int, row_block: int, frame_ptr: int,
                               stream: int = 0):
        """Row order back from gathered row-cyclic shards (rtg_assemble_shards_device)."""
        _check(lib().rtg_assemble_shards_device(self._h, ctypes.c_void_p(gathered_ptr), n_shards,
                                                padded_rows, width, height, row_block,
                                                ctypes.c_void_p(frame_ptr),
                                                ctypes.c_void_p(stream) if stream else None),
               "rtg_assemble_shards_device")

    def place_shard_device(self, shard_ptr: int, shard: int, n_shards: int, width: int,
                           height: int, row_block: int, frame_ptr: int, stream: int = 0):
        """Copy one shard's packed rows into their rows of a frame (rtg_place_shard_device)."""
        _check(lib().rtg_place_shard_device(self._h, ctypes.c_void_p(shard_ptr), shard, n_shards,
                                            width, height, row_block, ctypes.c_void_p(frame_ptr),
                                            ctypes.c_void_p(stream) if stream else None),
               "rtg_place_shard_device")

    def ppm_bytes_device(self, src_ptr: int, n_pixels: int, max_ptr: int, dst_ptr: int,
                         stream: int = 0):
        _check(lib().rtg_ppm_bytes_device(self._h, ctypes.c_void_p(src_ptr), n_pixels,
                                          ctypes.c_void_p(max_ptr), ctypes.c_void_p(dst_ptr),
                                          ctypes.c_void_p(stream) if stream else None),
               "rtg_ppm_bytes_device")


def canonical_bits(fb: np.ndarray) -> np.ndarray:
    """uint32 view with every NaN mapped to the x86 default NaN 0xFFC00000."""
    b = np.ascontiguousarray(fb, np.float32).view(np.uint32).copy()
    b[np.isnan(np.ascontiguousarray(fb, np.float32))] = 0xFFC00000
    return b
