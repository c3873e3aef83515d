#!/usr/bin/env python3
"""tools/bench_rays.py [--rounds N] [--out FILE] [--parent-json FILE] [--only-camera]
                       [--only-order] [--only-ao] [--only-matte] [--only-views]
                       [--only-fold] [--only-gather] [--only-filter] [--only-accumulate]
                       [--only-svgf] [--only-irradiance] [--only-upsample]
                       [--order-alt-json FILE ...]

Times rtg_intersect_device (the batch closest-hit query, csrc/rtg_rays.hip)
with the scene and the rays resident, on three batches of bench.py's frames:

  c3_ordered    the C3 scene (16 spheres), the 3840 x 2160 aa = 1 primary rays
                in pixel order
  c5_ordered    the C5 scene (1024 spheres, the BVH), the same rays
  c5_shuffled   the C5 scene, those rays in a seeded random permutation

Device events around back-to-back launches on one stream (a window of about
0.3 s), after a warm-up; medians over the rounds.  Writes FILE (default
profiles/rays/bench.json) with ms and Mrays/s of the three, the ordered /
shuffled ratio on C5 (the coherence sensitivity rtg.h mentions) and one
sanity relation, reported and not gated: rtg_gbuffer_device of the C3 frame
at aa = 1, timed in the same process round by round.  The ray query has no
primary cull (group_sel), so it is expected to be the slower of the two.
--parent-json FILE stores that file's object under "parent_commit" (the same
measurements taken on the parent commit's build, for the side-by-side).
The tool also checks that the ordered C3 hits are the G-buffer's (id, t,
normal) and that the shuffled hits are the ordered ones permuted.

rtg_raytrace_device (the batch ray tracer, csrc/rtg_raytrace.hip) gets rows of
its own under "raytrace": for C3 and C5 at their golden stack sizes (6 and 8),
the same 8.3 M one-sample primary rays in pixel order and shuffled, and next
to each, round by round in the same process, rtg_render_device of that frame
at alias_factor = 1, which traces exactly those rays.  The render has the
camera's cull, the compacted launch and the launch-order feedback, and every
table keyed to its own rays; the batch call has none of them.  The ratio
raytrace / render is therefore the price of generality; it is reported, not
gated.  The ordered colours must be the render's frame and the shuffled ones
the ordered ones permuted.

The posed camera (csrc/rtg_camera.hip) gets rows under "camera" (camera_rows
below): the fused render at the identity pose next to the batch call and the
render, at aa = 1 and aa = 3, the orbit pose, and the generator.
--only-camera runs these alone; --mapping NAME records the build's lane-to-pixel
mapping and --mapping-json FILE puts such a run of a build with another
mapping next to this one's (how the 8 x 8 tile was chosen over 64 x 1).

The ray order (csrc/rtg_order.hip) gets rows under "order" (order_rows below)
for the shuffled batches above: C5 intersect, C3 and C5 raytrace.  Each times,
round by round in one process, rtg_ray_order_device of the shuffled batch, the
indexed launch with that order, the plain launch of the same shuffled batch
and the plain launch of the pixel-ordered batch; it records the sum order +
indexed per round, the digit passes the sort executed and skipped, whether
the indexed outputs are the plain ones word for word, and, as a yardstick
outside the library, torch.sort of the same keys (a library radix sort of all
64 bits with indices).  The speed claim is gated on the two raytrace rows: the
sum must be below the plain shuffled launch by more than either's min-max
spread.  --only-order runs these rows alone (--order-label NAME is recorded:
the key layout or bit counts of the library under RTG_LIB / RTG_ORDER_LAYOUT);
--order-alt-json FILE puts such runs of other layouts next to this one's.

Ambient occlusion (csrc/rtg_ao.hip) gets rows under "ao" (ao_rows below): the
fused call on the frame's primary hits next to the unfused path (segments,
visible, a torch sum), with and without the ray order.  --only-ao runs these
alone and keeps FILE's other sections.

Direct light and containment (csrc/rtg_matte.hip) get rows under "matte" and
"contains" (matte_rows, contains_rows below): the fused call on the frame's
primary hits, with and without the mask, next to the unfused path (torch
segments, visible, a torch fold); the containment of the refraction test points
of the same hits.  --only-matte runs these alone and keeps FILE's other
sections.

The gather (csrc/rtg_gather.hip) gets rows under "gather" (gather_rows below):
the fused call on the frame's primary hits next to the unfused chain (the ray
generator, the batch ray tracer, a torch fold), with and without jitter and,
with it, the ray order.  --only-gather runs these alone and keeps FILE's other
sections.

Many views in one launch (rtg_render_views_device, csrc/rtg_camera.hip) get
rows under "views" (views_rows below): a bake of 256 probes x 6 cube faces of
32 x 32 pixels, as one launch, as 1536 single-view launches and through the ray
generator plus the batch ray tracer, next to one frame of the same pixel count.
--only-views runs these alone and keeps FILE's other sections.

The views folded into per-probe SH coefficients (rtg_render_views_fold_device,
csrc/rtg_fold.hip) get rows under "fold" (fold_rows below): the same bake
through the fused call, through rtg_render_views_device + rtg_views_fold_device
and through rtg_render_views_device + a torch einsum, with the bytes each route
allocates.  --only-fold runs these alone and keeps FILE's other sections.

The edge-stopping a-trous filter (rtg_filter_device, csrc/rtg_filter.hip) gets
rows under "filter" (filter_rows below): five passes over the frame's AO counts
and gathered light, the total and each pass, the tiled and the direct form of
the pass kernel side by side per step, and a torch chain of the same
arithmetic.  --only-filter runs these alone and keeps FILE's other sections.

Temporal accumulation (rtg_accumulate_device, csrc/rtg_accumulate.hip) gets
rows under "accumulate" (accumulate_rows below): one frame blended onto the
previous one under a small pan and under a roll, both wave shapes of the kernel
side by side, a torch chain of the same arithmetic and the streaming floor.
--only-accumulate runs these alone and keeps FILE's other sections.

The variance estimate and the variance-guided passes (rtg_variance_device,
rtg_svgf_device, csrc/rtg_svgf.hip) get rows under "svgf" (svgf_rows below): the
filter's four frames fed through one accumulation with M2, the variance with
every history long and short against its streaming floor, five passes against
rtg_filter_device in the same rounds, per pass and form, and a torch chain.
--only-svgf runs these alone and keeps FILE's other sections.

The probe grid's lookup (rtg_irradiance_device, csrc/rtg_irradiance.hip) gets
rows under "irradiance" (irradiance_rows below): an 8 x 8 x 4 grid of SH9 probes
baked as fold_rows bakes, looked up at the primary hits of a frame with no flag,
with VALID | FACING and with all three, next to the unfused chain (torch cells
and segments, rtg_visible_device, a torch gather and fold of the same
arithmetic) and the streaming floor.  --only-irradiance runs these alone and
keeps FILE's other sections.

The guided upsampling (rtg_upsample_device, rtg_hits_pick_device,
rtg_values_place_device, csrc/rtg_upsample.hip) gets rows under "upsample"
(upsample_rows below): the call alone on C3 and C5 frames at L = 1 and 2 with
and without the hole list, against its streaming floor and a torch chain of
the same arithmetic plus nonzero (gated: equal words and list), and the
mixed-resolution route of the gather and of the AO against the full-resolution
call in the same rounds.  --only-upsample runs these alone and keeps FILE's
other sections.
GPU only.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-gamma_amd"))
sys.path.insert(0, ROOT)
import rtg_amd as R  # noqa: E402
from bench import CONFIGS  # noqa: E402

F = np.float32


def primary_rays(W, H, zoom=-4.0):
    """The aa = 1 primary rays of a W x H frame (main.cpp:384-436) in float32,
    pixel order: origin 0, direction vnorm((x, y, zoom))."""
    xs, ys, asp = F(16) / F(W), F(12) / F(H), F(16) / F(12)
    halfW, halfH = F(W) * F(0.5), F(H) * F(0.5)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    vx = ((x.astype(F) - halfW) * xs) * asp
    vy = (halfH - y.astype(F)) * ys
    vz = np.full(x.shape, F(zoom))
    l = F(1) / np.sqrt((vx * vx + vy * vy) + vz * vz)
    out = np.zeros((H * W, 6), F)
    out[:, 3], out[:, 4], out[:, 5] = (l * vx).ravel(), (l * vy).ravel(), (l * vz).ravel()
    return out


def timed(fn, stream, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(fns, rounds, window_ms=300.0, raw=None, min_reps=3, names=None):
    """Median, min and max ms per launch of each fn, interleaved round by round
    (raw: a list that receives each fn's per-round times; min_reps: launches per
    round of an fn slower than the window; names: report each fn's first timing
    on stderr as it is taken)."""
    s = torch.cuda.current_stream()
    reps = []
    for k, fn in enumerate(fns):
        for _ in range(min_reps):
            fn()
        torch.cuda.synchronize()
        first = timed(fn, s, min(2, min_reps))
        reps.append(max(min_reps, min(2000, int(window_ms / max(first, 1e-3)))))
        if names:
            print(f"  {names[k]}: {first:.4f} ms, {reps[-1]} per round", file=sys.stderr, flush=True)
    t = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            t[k].append(timed(fn, s, reps[k]))
    if raw is not None:
        raw.extend(t)
    return [{"ms_median": round(float(np.median(v)), 5), "ms_min": round(min(v), 5),
             "ms_max": round(max(v), 5), "launches_per_round": r} for v, r in zip(t, reps)]


def orbit_pose(sph):
    """The `orbit` pose of tests/test_camera_host.py for a scene: from 1.2
    extents off the scene's centre, looking at it; zoom -12."""
    c = sph["pos"].astype(np.float64)
    r = np.abs(sph["radius"].astype(np.float64))[:, None]
    lo, hi = (c - r).min(0), (c + r).max(0)
    mid, s = (lo + hi) * 0.5, float((hi - lo).max())
    return R.camera_look_at(mid + 1.2 * s * np.array([0.6, 0.35, 0.72]), mid), -12.0


def camera_rows(args, W, H, rays, col, fb, stream):
    """The posed camera (csrc/rtg_camera.hip), C3 and C5 at their stack sizes,
    round by round in one process: (a) the fused render at the identity pose
    and aa = 1 next to rtg_raytrace_device of the same pixel-ordered rays and
    rtg_render_device at alias_factor = 1: the same trees, the fused kernel
    moving 24 B per ray less than the batch call; (b) the identity pose at
    aa = 3 next to rtg_render_device at aa = 3: the price of a frame that is
    exact for any viewpoint; (c) the orbit pose at aa = 3, recorded only; and
    the generator's time for the aa = 3 frame next to the bytes it writes.
    The identity frames must be the render's."""
    n = W * H
    fc = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gen = torch.empty((n * 9, 6), dtype=torch.float32, device="cuda")
    ident = R.camera_identity()
    out, ok = {"mapping": args.mapping}, True

    def same(a, b):
        return bool((a.view(torch.int32) == b.view(torch.int32)).all())

    for name in ("c3", "c5"):
        S = CONFIGS[name][4] + 1
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        orbit, ozoom = orbit_pose(sph)
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        c1, b1, r1 = measure(
            [lambda: ctx.render_camera(ident, W, H, fc.data_ptr(), -4.0, 1.0, S, stream),
             lambda: ctx.raytrace_device(rays.data_ptr(), n, col.data_ptr(), S, stream),
             lambda: ctx.render_device(W, H, fb.data_ptr(), alias_factor=1.0, stack_size=S,
                                       stream=stream)], args.rounds)
        eq1 = same(fc, fb) and same(col, fb.view(-1, 3))
        c3, r3, o3, g3 = measure(
            [lambda: ctx.render_camera(ident, W, H, fc.data_ptr(), -4.0, 3.0, S, stream),
             lambda: ctx.render_device(W, H, fb.data_ptr(), alias_factor=3.0, stack_size=S,
                                       stream=stream),
             lambda: ctx.render_camera(orbit, W, H, col.data_ptr(), ozoom, 3.0, S, stream),
             lambda: ctx.camera_rays(orbit, W, H, gen.data_ptr(), ozoom, 3.0, stream)],
            args.rounds)
        ctx.close()
        eq3 = same(fc, fb)
        ok = ok and eq1 and eq3
        g3["bytes"] = n * 9 * 24
        g3["GB_per_s"] = round(g3["bytes"] / (g3["ms_median"] * 1e-3) / 1e9, 1)
        out[name] = {
            "stack_size": S, "camera_aa1": c1, "raytrace_aa1": b1, "render_aa1": r1,
            "camera_over_raytrace_aa1": round(c1["ms_median"] / b1["ms_median"], 3),
            "camera_over_render_aa1": round(c1["ms_median"] / r1["ms_median"], 3),
            "camera_aa3": c3, "render_aa3": r3, "orbit_aa3": o3,
            "camera_over_render_aa3": round(c3["ms_median"] / r3["ms_median"], 3),
            "generator_aa3": g3,
            "identity_aa1_equals_render_and_raytrace": eq1, "identity_aa3_equals_render": eq3}
    return out, ok


def order_rows(args, n, rays, shuffled, stream):
    """The ray order (csrc/rtg_order.hip) on the shuffled 8.3 M primary rays:
    order, indexed launch, plain shuffled launch and pixel-ordered launch, round
    by round; see the module text.  Returns (rows, ok): ok is the gate of the
    two raytrace rows and the word-for-word equality of all three."""
    nbytes = R.ray_order_scratch(n)
    scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
    order = torch.empty((n,), dtype=torch.int32, device="cuda")
    keys = torch.empty((n,), dtype=torch.int64, device="cuda")
    out, ok = {"label": args.order_label, "scratch_bytes": nbytes}, True
    for row, name, call in (("c5_intersect", "c5", "intersect"), ("c3_raytrace", "c3", "raytrace"),
                            ("c5_raytrace", "c5", "raytrace")):
        S = CONFIGS[name][4] + 1
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        if call == "intersect":
            shape, dt = (n, 8), torch.int32
            run = lambda src, dst, o: ctx.intersect_device(src.data_ptr(), n, dst.data_ptr(),  # noqa: E731
                                                           stream, order=o)
        else:
            shape, dt = (n, 3), torch.float32
            run = lambda src, dst, o: ctx.raytrace_device(src.data_ptr(), n, dst.data_ptr(), S,  # noqa: E731
                                                          stream, order=o)
        d_idx = torch.empty(shape, dtype=dt, device="cuda")
        d_plain = torch.empty(shape, dtype=dt, device="cuda")
        d_pix = torch.empty(shape, dtype=dt, device="cuda")
        ctx.ray_order(shuffled.data_ptr(), n, order.data_ptr(), scratch.data_ptr(), nbytes,
                      keys_ptr=keys.data_ptr(), stream=stream)  # once with the keys, for the counts
        sort = lambda: ctx.ray_order(shuffled.data_ptr(), n, order.data_ptr(), scratch.data_ptr(),  # noqa: E731
                                     nbytes, stream=stream)
        raw = []
        so, ix, pl, px, ts = measure(
            [sort, lambda: run(shuffled, d_idx, order.data_ptr()),
             lambda: run(shuffled, d_plain, 0), lambda: run(rays, d_pix, 0),
             lambda: torch.sort(keys, stable=True)], args.rounds, raw=raw)
        ctx.close()
        equal = bool((d_idx.view(torch.int32) == d_plain.view(torch.int32)).all())
        k = keys.cpu().numpy().view(np.uint64)
        ran = [bool(np.ptp((k >> np.uint64(8 * p)) & np.uint64(0xFF)) > 0)
               for p in range(-(-R.ORDER_KEY_BITS // 8))]
        is_sorted = bool((np.diff(k[order.cpu().numpy().view(np.uint32)].astype(np.int64)) >= 0).all())
        both = [a + b for a, b in zip(raw[0], raw[1])]
        spread = max(max(both) - min(both), pl["ms_max"] - pl["ms_min"])
        gain = pl["ms_median"] - float(np.median(both))
        faster = bool(gain > spread)
        out[row] = {
            "stack_size": S if call == "raytrace" else None,
            "order": so, "indexed": ix, "plain_shuffled": pl, "pixel_order": px,
            "order_plus_indexed": {"ms_median": round(float(np.median(both)), 5),
                                   "ms_min": round(min(both), 5), "ms_max": round(max(both), 5)},
            "plain_shuffled_over_order_plus_indexed":
                round(pl["ms_median"] / float(np.median(both)), 3),
            "indexed_over_pixel_order": round(ix["ms_median"] / px["ms_median"], 3),
            "faster_by_more_than_the_spread": faster,
            "gated": call == "raytrace",
            "digit_passes_executed": int(sum(ran)), "digit_passes_skipped": int(len(ran) - sum(ran)),
            "distinct_keys": int(len(np.unique(k))),
            "indexed_equals_plain_shuffled": equal, "keys_sorted_by_order": is_sorted,
            "torch_sort_64bit_pairs": ts}
        ok = ok and equal and is_sorted and (faster or call != "raytrace")
        del d_idx, d_plain, d_pix
    return out, ok


def ao_rows(args, W, H, rays, stream):
    """Ambient occlusion (csrc/rtg_ao.hip) of the frame's 8.3 M aa = 1 primary
    hits on C3 and C5: K = 16 probes of rtg_ao_directions(16), radius 2.5 x the
    scene's largest |radius|, bias 1e-3, jitter off and on.  Round by round in
    one process: the fused call, and the pieces of the unfused path on the same
    hits: rtg_ao_segments_device (24 K bytes per point), rtg_visible_device over
    the n K segments, a torch sum of K bytes per point, and for the sorted form
    rtg_ray_order_device of the segments plus the indexed launch.  The unfused
    rows are the per-round sums of their pieces.  Reported, not gated: whether
    the fused call is slower than the best unfused row by more than that row's
    own min-max spread.  Gated: the fused counts are the folded ones."""
    n, K = W * H, 16
    table = torch.from_numpy(R.ao_directions(K)).cuda()
    hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    segs = torch.empty((n * K, 6), dtype=torch.float32, device="cuda")
    vis = torch.empty((n * K,), dtype=torch.uint8, device="cuda")
    vis_idx = torch.empty((n * K,), dtype=torch.uint8, device="cuda")
    cnt = torch.empty((n,), dtype=torch.int16, device="cuda")
    nbytes = R.ray_order_scratch(n * K)
    scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
    order = torch.empty((n * K,), dtype=torch.int32, device="cuda")
    out, ok = {"samples": K, "directions": K, "bias": 1e-3, "segment_bytes": n * K * 24,
               "order_scratch_bytes": nbytes}, True
    for name in ("c3", "c5"):
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        radius = float(F(2.5) * np.abs(sph["radius"]).max())
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream)
        out[name] = {"radius": radius, "hit_points": int((hits[:, 0] >= 0).sum())}
        for label, flags in (("plain", 0), ("jitter", R.AO_JITTER)):
            p = R.ao_params(K, radius, 1e-3, 42, flags)
            raw = []
            fu, sg, vs, fo, so, vi = measure(
                [lambda: ctx.ao_device(hits.data_ptr(), n, p, table.data_ptr(), K, cnt.data_ptr(),
                                       stream),
                 lambda: ctx.ao_segments_device(hits.data_ptr(), n, p, table.data_ptr(), K,
                                                segs.data_ptr(), stream),
                 lambda: ctx.visible_device(segs.data_ptr(), n * K, vis.data_ptr(), stream),
                 lambda: vis.view(n, K).sum(1, dtype=torch.int32),
                 lambda: ctx.ray_order(segs.data_ptr(), n * K, order.data_ptr(), scratch.data_ptr(),
                                       nbytes, kind=R.ORDER_SEGMENTS, stream=stream),
                 lambda: ctx.visible_device(segs.data_ptr(), n * K, vis_idx.data_ptr(), stream,
                                            order=order.data_ptr())], args.rounds, raw=raw)
            folded = vis.view(n, K).sum(1, dtype=torch.int32)
            equal = bool((cnt.to(torch.int32) == folded).all()) and bool((vis == vis_idx).all())
            ok = ok and equal
            sums = {"unfused": [a + b + c for a, b, c in zip(raw[1], raw[2], raw[3])],
                    "unfused_sorted": [a + b + c + d for a, b, c, d in
                                       zip(raw[1], raw[4], raw[5], raw[3])]}
            rows = {k: {"ms_median": round(float(np.median(v)), 5), "ms_min": round(min(v), 5),
                        "ms_max": round(max(v), 5)} for k, v in sums.items()}
            best = min(rows, key=lambda k: rows[k]["ms_median"])
            spread = rows[best]["ms_max"] - rows[best]["ms_min"]
            out[name][label] = {
                "fused": fu, "segments": sg, "visible": vs, "fold": fo, "order": so,
                "visible_indexed": vi, **rows, "best_unfused": best,
                "best_unfused_over_fused": round(rows[best]["ms_median"] / fu["ms_median"], 3),
                "fused_slower_than_best_unfused_by_more_than_its_spread":
                    bool(fu["ms_median"] - rows[best]["ms_median"] > spread),
                "Mprobes_per_s": round(n * K / (fu["ms_median"] * 1e-3) / 1e6, 1),
                "blocked_share_of_hit_points": round(
                    1.0 - float(cnt[hits[:, 0] >= 0].to(torch.float64).sum()) /
                    (K * max(1, out[name]["hit_points"])), 4),
                "fused_equals_folded_visible": equal}
            print(f"ao {name} {label}: fused {fu['ms_median']} ms, {best} "
                  f"{rows[best]['ms_median']} ms", file=sys.stderr, flush=True)
        ctx.close()
    return out, ok


def _spread_rows(sums):
    return {k: {"ms_median": round(float(np.median(v)), 5), "ms_min": round(min(v), 5),
                "ms_max": round(max(v), 5)} for k, v in sums.items()}


def gather_rows(args, stream):
    """The gather (csrc/rtg_gather.hip) of a frame's aa = 1 primary hits: C3 at
    stack size 6 on the 3840 x 2160 frame, C5 at stack size 8 on a 640 x 360
    frame (a jittered round of the full frame would take seconds) and, because
    that frame gives the fused call's one lane per point only 3600 waves, on a
    1920 x 1080 frame too; K = 16 probes
    of rtg_ao_directions(16), weights 1 / K, bias 1e-3, jitter off and on.  Round
    by round in one process: the fused call, and the pieces of the unfused chain
    on the same hits: rtg_gather_rays_device (24 K bytes per point),
    rtg_raytrace_device over the n K rays (12 K bytes per point), a torch fold
    and, for the sorted form, rtg_ray_order_device of the rays plus the indexed
    launch.  The unfused rows are the per-round sums of their pieces.  Reported,
    not gated: whether the fused call is slower than the unfused chain by more
    than the chain's own min-max spread.  Gated: the fused sums are, word for
    word, the chain's colours folded on the host in the defined order."""
    K = 16
    table = torch.from_numpy(R.ao_directions(K)).cuda()
    wt_np = np.full(K, F(1) / F(K), F)
    wt = torch.from_numpy(wt_np).cuda()
    out, ok = {"samples": K, "directions": K, "bias": 1e-3, "weights": "1 / K"}, True
    for name, cfg, (W, H) in (("c3", "c3", CONFIGS["c3"][:2]), ("c5", "c5", (640, 360)),
                              ("c5_1080p", "c5", (1920, 1080))):
        n, S = W * H, CONFIGS[cfg][4] + 1
        rays0 = torch.from_numpy(primary_rays(W, H)).cuda()
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        rays = torch.empty((n * K, 6), dtype=torch.float32, device="cuda")
        cols = torch.empty((n * K, 3), dtype=torch.float32, device="cuda")
        cols_idx = torch.empty((n * K, 3), dtype=torch.float32, device="cuda")
        acc = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        nbytes = R.ray_order_scratch(n * K)
        scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
        order = torch.empty((n * K,), dtype=torch.int32, device="cuda")
        sph, lg = R.generate_scene(CONFIGS[cfg][2], CONFIGS[cfg][3], 42)
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        ctx.intersect_device(rays0.data_ptr(), n, hits.data_ptr(), stream)
        real = (hits[:, 0] >= 0).cpu().numpy()
        out[name] = {"W": W, "H": H, "points": n, "stack_size": S, "hit_points": int(real.sum()),
                     "ray_bytes": n * K * 24, "colour_bytes": n * K * 12,
                     "order_scratch_bytes": nbytes}
        for label, flags in (("plain", 0), ("jitter", R.GATHER_JITTER)):
            p = R.gather_params(K, 1e-3, 42, flags)
            fns = [lambda: ctx.gather_device(hits.data_ptr(), n, p, table.data_ptr(), wt.data_ptr(),
                                             K, acc.data_ptr(), stack_size=S, stream=stream),
                   lambda: ctx.gather_rays_device(hits.data_ptr(), n, p, table.data_ptr(), K,
                                                  rays.data_ptr(), stream),
                   lambda: ctx.raytrace_device(rays.data_ptr(), n * K, cols.data_ptr(), S, stream),
                   # (the weights are all 1 / K, so the jittered window folds the same way)
                   lambda: (cols.view(n, K, 3) * wt.view(1, K, 1)).sum(1)]
            if flags:
                fns += [lambda: ctx.ray_order(rays.data_ptr(), n * K, order.data_ptr(),
                                              scratch.data_ptr(), nbytes, stream=stream),
                        lambda: ctx.raytrace_device(rays.data_ptr(), n * K, cols_idx.data_ptr(), S,
                                                    stream, order=order.data_ptr())]
            raw = []
            m = measure(fns, args.rounds, raw=raw, min_reps=2,
                        names=[f"gather {name} {label} {k}" for k in
                               ("fused", "rays", "raytrace", "fold", "order", "indexed")][:len(fns)])
            # the chain's colours folded on the host in the defined order
            c = cols.cpu().numpy().reshape(n, K, 3)
            want = np.zeros((n, 3), F)
            with np.errstate(all="ignore"):
                for k in range(K):
                    want = want + wt_np[k] * c[:, k, :]
            want[~real] = 0
            del c
            got = acc.cpu().numpy()

            def words(a):
                b = a.view(np.uint32).copy()
                b[np.isnan(a)] = 0xFFC00000
                return b
            equal = bool((words(got) == words(want)).all())
            if flags:
                equal = equal and bool((cols.view(torch.int32) == cols_idx.view(torch.int32)).all())
            ok = ok and equal
            sums = {"unfused": [a + b + c for a, b, c in zip(raw[1], raw[2], raw[3])]}
            if flags:
                sums["unfused_sorted"] = [a + b + c + d for a, b, c, d in
                                          zip(raw[1], raw[4], raw[5], raw[3])]
            rows = _spread_rows(sums)
            fu = m[0]
            spread = rows["unfused"]["ms_max"] - rows["unfused"]["ms_min"]
            out[name][label] = {
                "fused": fu, "rays": m[1], "raytrace": m[2], "fold": m[3],
                **({"order": m[4], "raytrace_indexed": m[5]} if flags else {}), **rows,
                "unfused_over_fused": round(rows["unfused"]["ms_median"] / fu["ms_median"], 3),
                "fused_slower_than_unfused_by_more_than_its_spread":
                    bool(fu["ms_median"] - rows["unfused"]["ms_median"] > spread),
                "Mprobes_per_s": round(n * K / (fu["ms_median"] * 1e-3) / 1e6, 1),
                "nonfinite_share_of_sums": round(float((~np.isfinite(got[real]).all(1)).mean()), 4),
                "fused_equals_chain_folded_on_host": equal}
            print(f"gather {name} {label}: fused {fu['ms_median']} ms, unfused "
                  f"{rows['unfused']['ms_median']} ms, equal {equal}", file=sys.stderr, flush=True)
        ctx.close()
        del rays0, hits, rays, cols, cols_idx, acc, scratch, order
    return out, ok


def torch_filter(ids, P, N, img, passes, flags, normal_log2, scale):
    """rtg_filter*'s arithmetic as a torch chain: shifted slices over the padded
    planes, `where` for the left-out taps.  ids (H, W) int32, P and N three
    (H, W) planes each, img a list of C (H, W) planes; the filtered planes."""
    import torch.nn.functional as TF
    H, W = ids.shape
    hw = (0.0625, 0.25, 0.375, 0.25, 0.0625)
    zero = torch.zeros((), dtype=torch.float32, device=ids.device)
    for i in range(passes):
        s = 1 << i
        b = 2 * s
        pad = lambda a, v: TF.pad(a, (b, b, b, b), value=v)  # noqa: E731
        idp = pad(ids, -1)
        Pp, Np, vp = [pad(a, 0.0) for a in P], [pad(a, 0.0) for a in N], [pad(a, 0.0) for a in img]
        acc = [torch.zeros_like(a) for a in img]
        sw = torch.zeros_like(img[0])
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = slice(b + dy * s, b + dy * s + H), slice(b + dx * s, b + dx * s + W)
                idq = idp[ys, xs]
                keep = idq >= 0
                if flags & R.FILTER_SAME_ID:
                    keep &= idq == ids
                if flags & R.FILTER_SKIP_NONFINITE:
                    for a in vp:
                        keep &= torch.isfinite(a[ys, xs])
                w = torch.full_like(sw, hw[dy + 2] * hw[dx + 2])
                if flags & R.FILTER_NORMAL:
                    c = (N[0] * Np[0][ys, xs] + N[1] * Np[1][ys, xs]) + N[2] * Np[2][ys, xs]
                    c = torch.where(c > 0, c, zero)
                    for _ in range(normal_log2):
                        c = c * c
                    w = w * c
                if flags & R.FILTER_PLANE:
                    e = [Pp[q][ys, xs] - P[q] for q in range(3)]
                    d = ((N[0] * e[0] + N[1] * e[1]) + N[2] * e[2]).abs()
                    z = 1.0 - d * scale
                    w = w * torch.where(z > 0, z, zero)
                keep &= w > 0
                w = torch.where(keep, w, zero)
                for q in range(len(img)):
                    acc[q] += torch.where(keep, w * vp[q][ys, xs], zero)
                sw += w
        done = (sw > 0) & (ids >= 0)
        img = [torch.where(done, acc[q] / sw, img[q]) for q in range(len(img))]
    return img


def filter_rows(args, stream):
    """The edge-stopping a-trous filter (csrc/rtg_filter.hip) at passes 5 with
    SAME_ID | NORMAL | PLANE, planeScale 1 / (the scene's largest |radius|),
    normalLog2 3, on the aa = 1 primary hits of C3 and C5: the counts of
    rtg_ao_device (K = 16, jittered) at 3840 x 2160, the light of
    rtg_gather_device (K = 16, jittered, the skip flag) at 3840 x 2160 on C3 and
    1920 x 1080 on C5.  Round by round in one process: the call as it chooses
    its forms, the call with each form forced (RTG_FILTER_FORM) at passes 1 to 5,
    whose differences are the passes on their own (step 16 does not fit the
    tiled form's LDS and runs direct under either name), and a torch chain of
    the same arithmetic.  Reported, not gated: every time, and each pass's
    distance from the streaming floor (32 guide bytes, the value in and out per
    pixel at 6 TB/s).  Gated: the call and the torch chain agree to 1e-4
    relative on finite pixels (torch's sum order is its own: a sanity bound)."""
    K, passes, nlog = 16, 5, 3
    FORMS = ("tiled", "direct")
    flags = R.FILTER_SAME_ID | R.FILTER_NORMAL | R.FILTER_PLANE
    table = torch.from_numpy(R.ao_directions(K)).cuda()
    wt = torch.full((K,), 1.0 / K, dtype=torch.float32, device="cuda")
    out, ok = {"passes": passes, "flags": flags, "normalLog2": nlog, "samples": K,
               "floor_bandwidth_TBps": 6.0}, True
    for name, cfg, (W, H), kind in (("c3_count", "c3", CONFIGS["c3"][:2], R.FILTER_COUNT),
                                    ("c5_count", "c5", CONFIGS["c5"][:2], R.FILTER_COUNT),
                                    ("c3_rgb", "c3", CONFIGS["c3"][:2], R.FILTER_RGB),
                                    ("c5_rgb_1080p", "c5", (1920, 1080), R.FILTER_RGB)):
        n, S, C = W * H, CONFIGS[cfg][4] + 1, 3 if kind == R.FILTER_RGB else 1
        sph, lg = R.generate_scene(CONFIGS[cfg][2], CONFIGS[cfg][3], 42)
        scale = float(F(1) / np.abs(sph["radius"]).max())
        rays0 = torch.from_numpy(primary_rays(W, H)).cuda()
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        ctx.intersect_device(rays0.data_ptr(), n, hits.data_ptr(), stream)
        if kind == R.FILTER_COUNT:
            src = torch.empty((n,), dtype=torch.int16, device="cuda")
            radius = float(F(2.5) * np.abs(sph["radius"]).max())
            ctx.ao_device(hits.data_ptr(), n, R.ao_params(K, radius, 1e-3, 42, R.AO_JITTER),
                          table.data_ptr(), K, src.data_ptr(), stream)
        else:
            src = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            gp = R.gather_params(K, 1e-3, 42, R.GATHER_JITTER | R.GATHER_SKIP_NONFINITE)
            ctx.gather_device(hits.data_ptr(), n, gp, table.data_ptr(), wt.data_ptr(), K,
                              src.data_ptr(), stack_size=S, stream=stream)
        torch.cuda.synchronize()
        del rays0
        dst = torch.empty((n, C), dtype=torch.float32, device="cuda")
        ps = [R.filter_params(k, kind, flags, scale, nlog) for k in range(1, passes + 1)]
        nbytes = R.filter_scratch(W, H, ps[-1])
        scratch = torch.empty((max(nbytes, 16) // 4,), dtype=torch.int32, device="cuda")

        def call(form, p):
            if form:
                os.environ["RTG_FILTER_FORM"] = form
            else:
                os.environ.pop("RTG_FILTER_FORM", None)
            ctx.filter_device(hits.data_ptr(), W, H, p, src.data_ptr(), dst.data_ptr(),
                              scratch.data_ptr(), nbytes, stream)

        fns = [lambda: call("", ps[-1])]
        fns += [(lambda f=f, p=p: call(f, p)) for f in FORMS for p in ps]
        raw = []
        m = measure(fns, args.rounds, window_ms=100.0, raw=raw,
                    names=[f"filter {name} default"] + [f"filter {name} {f} passes {k}" for f in FORMS
                                                         for k in range(1, passes + 1)])
        os.environ.pop("RTG_FILTER_FORM", None)
        floor = n * (32 + 8 * C) / 6.0e12 * 1e3
        forms = {}
        for fi, f in enumerate(FORMS):
            cum = raw[1 + fi * passes:1 + (fi + 1) * passes]
            per = [cum[0]] + [[b - a for a, b in zip(cum[k - 1], cum[k])] for k in range(1, passes)]
            forms[f] = {"cumulative": m[1 + fi * passes:1 + (fi + 1) * passes],
                        "pass_ms_median": [round(float(np.median(v)), 5) for v in per],
                        "pass_ms_min": [round(min(v), 5) for v in per],
                        "pass_ms_max": [round(max(v), 5) for v in per],
                        "pass_over_floor": [round(float(np.median(v)) / floor, 2) for v in per]}
        # the call's own answer, then the torch chain of the same arithmetic
        call("", ps[-1])
        torch.cuda.synchronize()
        got = dst.clone()
        h = hits.view(torch.float32)
        ids = hits[:, 0].reshape(H, W).contiguous()
        P = [h[:, 2 + q].reshape(H, W).contiguous() for q in range(3)]
        N = [h[:, 5 + q].reshape(H, W).contiguous() for q in range(3)]
        if kind == R.FILTER_COUNT:
            img = [(src.to(torch.int32) & 0xFFFF).to(torch.float32).reshape(H, W)]
        else:
            img = [src[:, q].reshape(H, W).contiguous() for q in range(3)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        chain = lambda: torch_filter(ids, P, N, img, passes, flags, nlog, scale)  # noqa: E731
        ref = torch.stack(chain(), -1).reshape(n, C)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - ref.numel() * 4
        tm = measure([chain], args.rounds, window_ms=100.0, min_reps=1,
                     names=[f"filter {name} torch chain"])[0]
        fin = torch.isfinite(got) & torch.isfinite(ref)
        same_nonfinite = bool((torch.isfinite(got) == torch.isfinite(ref)).all())
        rel = ((got - ref).abs() / ref.abs().clamp_min(1e-30))[fin]
        worst = float(rel.max()) if rel.numel() else 0.0
        agree = same_nonfinite and worst <= 1e-4
        ok = ok and agree
        real = hits[:, 0] >= 0
        out[name] = {
            "W": W, "H": H, "kind": int(kind), "hit_points": int(real.sum()),
            "plane_scale": scale, "floor_ms_per_pass": round(floor, 5), "default": m[0],
            "default_forms": "tiled up to step 4, direct beyond", "forms": forms,
            "filter_scratch_bytes": nbytes, "torch_chain": tm, "torch_extra_bytes": int(extra),
            "torch_over_filter": round(tm["ms_median"] / m[0]["ms_median"], 2),
            "changed_share_of_hit_pixels": round(float(
                ((got != torch.stack(img, -1).reshape(n, C)).any(1) & real).sum() / real.sum()), 4),
            "largest_relative_difference": worst, "bit_equal": bool(
                (got.view(torch.int32)[fin] == ref.view(torch.int32)[fin]).all()),
            "agree_to_1e-4": agree}
        print(f"filter {name}: {m[0]['ms_median']} ms, torch {tm['ms_median']} ms, "
              f"largest relative difference {worst:.3g}", file=sys.stderr, flush=True)
        ctx.close()
        del hits, src, dst, scratch, got, ref, ids, P, N, img, h, fin, rel, real
        torch.cuda.empty_cache()
    return out, ok


def torch_svgf(ids, P, N, img, var, passes, flags, normal_log2, scale, sigma, eps):
    """rtg_svgf*'s arithmetic with RTG_SVGF_LUMA as a torch chain, in the manner
    of torch_filter: img a list of C (H, W) planes, var an (H, W) plane; the
    filtered planes and the carried variance."""
    import torch.nn.functional as TF
    H, W = ids.shape
    hw, kw = (0.0625, 0.25, 0.375, 0.25, 0.0625), (0.25, 0.5, 0.25)
    zero = torch.zeros((), dtype=torch.float32, device=ids.device)

    def lum(v):
        return v[0] if len(v) == 1 else (0.2126 * v[0] + 0.7152 * v[1]) + 0.0722 * v[2]

    def admits(idq, vals):
        keep = idq >= 0
        if flags & R.FILTER_SAME_ID:
            keep &= idq == ids
        if flags & R.FILTER_SKIP_NONFINITE:
            for a in vals:
                keep &= torch.isfinite(a)
        return keep

    for i in range(passes):
        s = 1 << i
        b = 2 * s
        pad = lambda a, v: TF.pad(a, (b, b, b, b), value=v)  # noqa: E731
        idp, varp = pad(ids, -1), pad(var, 0.0)
        Pp, Np, vp = [pad(a, 0.0) for a in P], [pad(a, 0.0) for a in N], [pad(a, 0.0) for a in img]
        gs, gw = torch.zeros_like(var), torch.zeros_like(var)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                ys, xs = slice(b + dy, b + dy + H), slice(b + dx, b + dx + W)
                keep = admits(idp[ys, xs], [varp[ys, xs]])
                k = kw[dy + 1] * kw[dx + 1]
                gs += torch.where(keep, k * varp[ys, xs], zero)
                gw += torch.where(keep, torch.full_like(gw, k), zero)
        g = torch.where(gw > 0, gs / gw, var)
        ls = 1.0 / (sigma * torch.sqrt(g) + eps)
        lp = lum(img)
        acc = [torch.zeros_like(a) for a in img]
        sv, sw = torch.zeros_like(var), torch.zeros_like(var)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = slice(b + dy * s, b + dy * s + H), slice(b + dx * s, b + dx * s + W)
                vq = [a[ys, xs] for a in vp]
                keep = admits(idp[ys, xs], vq + [varp[ys, xs]])
                w = torch.full_like(sw, hw[dy + 2] * hw[dx + 2])
                if flags & R.FILTER_NORMAL:
                    c = (N[0] * Np[0][ys, xs] + N[1] * Np[1][ys, xs]) + N[2] * Np[2][ys, xs]
                    c = torch.where(c > 0, c, zero)
                    for _ in range(normal_log2):
                        c = c * c
                    w = w * c
                if flags & R.FILTER_PLANE:
                    e = [Pp[q][ys, xs] - P[q] for q in range(3)]
                    d = ((N[0] * e[0] + N[1] * e[1]) + N[2] * e[2]).abs()
                    z = 1.0 - d * scale
                    w = w * torch.where(z > 0, z, zero)
                z = 1.0 - (lum(vq) - lp).abs() * ls
                w = w * torch.where(z > 0, z, zero)
                keep &= w > 0
                w = torch.where(keep, w, zero)
                for q in range(len(img)):
                    acc[q] += torch.where(keep, w * vq[q], zero)
                sv += torch.where(keep, (w * w) * varp[ys, xs], zero)
                sw += w
        done = (sw > 0) & (ids >= 0)
        img = [torch.where(done, acc[q] / sw, img[q]) for q in range(len(img))]
        var = torch.where(done, sv / (sw * sw), var)
    return img, var


def svgf_rows(args, stream):
    """The variance estimate and the variance-guided passes (csrc/rtg_svgf.hip)
    on filter_rows' four frames, each fed through one rtg_accumulate_device
    (a reset frame, with M2), floats from there on.  Round by round in one
    process: rtg_variance_device with every history long (minHistory 0: the
    stream) and with every history short (minHistory 65535: every tile with a
    hit stages its window), against the streaming floor (the id, acc, m2 and len
    in, one word out per pixel at 6 TB/s); rtg_filter_device at five passes on
    the accumulated frame, the yardstick; rtg_svgf_device at five passes with
    SAME_ID | NORMAL | PLANE | RTG_SVGF_LUMA, sigmaL 4, epsL 1e-6, as it chooses
    its forms and with each form forced (RTG_SVGF_FORM) at passes 1 to 5, whose
    differences are the passes on their own (floor per pass: 32 guide bytes,
    value and variance in and out); and a torch chain of the same arithmetic.
    Reported, not gated: every time.  Gated: the call and the torch chain agree
    to 1e-4 relative on finite pixels, value and variance."""
    K, passes, nlog, sigma, eps = 16, 5, 3, 4.0, 1e-6
    FORMS = ("tiled", "direct")
    flags = R.FILTER_SAME_ID | R.FILTER_NORMAL | R.FILTER_PLANE
    table = torch.from_numpy(R.ao_directions(K)).cuda()
    wt = torch.full((K,), 1.0 / K, dtype=torch.float32, device="cuda")
    out, ok = {"passes": passes, "flags": flags | R.SVGF_LUMA, "normalLog2": nlog, "samples": K,
               "sigmaL": sigma, "epsL": eps, "floor_bandwidth_TBps": 6.0}, True
    for name, cfg, (W, H), kind in (("c3_count", "c3", CONFIGS["c3"][:2], R.FILTER_COUNT),
                                    ("c5_count", "c5", CONFIGS["c5"][:2], R.FILTER_COUNT),
                                    ("c3_rgb", "c3", CONFIGS["c3"][:2], R.FILTER_RGB),
                                    ("c5_rgb_1080p", "c5", (1920, 1080), R.FILTER_RGB)):
        n, S, C = W * H, CONFIGS[cfg][4] + 1, 3 if kind == R.FILTER_RGB else 1
        fkind = R.FILTER_RGB if C == 3 else R.FILTER_GRAY
        sph, lg = R.generate_scene(CONFIGS[cfg][2], CONFIGS[cfg][3], 42)
        scale = float(F(1) / np.abs(sph["radius"]).max())
        rays0 = torch.from_numpy(primary_rays(W, H)).cuda()
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        ctx.intersect_device(rays0.data_ptr(), n, hits.data_ptr(), stream)
        if kind == R.FILTER_COUNT:
            src = torch.empty((n,), dtype=torch.int16, device="cuda")
            radius = float(F(2.5) * np.abs(sph["radius"]).max())
            ctx.ao_device(hits.data_ptr(), n, R.ao_params(K, radius, 1e-3, 42, R.AO_JITTER),
                          table.data_ptr(), K, src.data_ptr(), stream)
        else:
            src = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            gp = R.gather_params(K, 1e-3, 42, R.GATHER_JITTER | R.GATHER_SKIP_NONFINITE)
            ctx.gather_device(hits.data_ptr(), n, gp, table.data_ptr(), wt.data_ptr(), K,
                              src.data_ptr(), stack_size=S, stream=stream)
        acc = torch.empty((n, C), dtype=torch.float32, device="cuda")
        m2 = torch.empty((n, C), dtype=torch.float32, device="cuda")
        ln = torch.empty((n,), dtype=torch.int16, device="cuda")
        ctx.accumulate_device(hits.data_ptr(), W, H,
                              R.accumulate_params(kind, flags | R.ACCUM_SKIP_NONFINITE, scale, nlog),
                              src.data_ptr(), acc.data_ptr(), ln.data_ptr(), None,
                              out_m2_ptr=m2.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        del rays0, src
        var, dvar = (torch.empty((n,), dtype=torch.float32, device="cuda") for _ in range(2))
        dst = torch.empty((n, C), dtype=torch.float32, device="cuda")
        fdst = torch.empty((n, C), dtype=torch.float32, device="cuda")
        ps = [R.svgf_params(k, fkind, flags | R.SVGF_LUMA, scale, nlog, sigma, eps)
              for k in range(1, passes + 1)]
        fp = R.filter_params(passes, fkind, flags, scale, nlog)
        nbytes, fbytes = R.svgf_scratch(W, H, ps[-1]), R.filter_scratch(W, H, fp)
        scratch = torch.empty((max(nbytes, 16) // 4,), dtype=torch.int32, device="cuda")

        def variance(min_history):
            ctx.variance_device(hits.data_ptr(), W, H,
                                R.variance_params(fkind, flags, scale, nlog, min_history),
                                acc.data_ptr(), m2.data_ptr(), ln.data_ptr(), var.data_ptr(), stream)

        def plain():
            ctx.filter_device(hits.data_ptr(), W, H, fp, acc.data_ptr(), fdst.data_ptr(),
                              scratch.data_ptr(), fbytes, stream)

        def call(form, p):
            if form:
                os.environ["RTG_SVGF_FORM"] = form
            else:
                os.environ.pop("RTG_SVGF_FORM", None)
            ctx.svgf_device(hits.data_ptr(), W, H, p, acc.data_ptr(), var.data_ptr(), dst.data_ptr(),
                            dvar.data_ptr(), scratch.data_ptr(), nbytes, stream)

        variance(65535)  # what the passes are timed on: the spatial estimate of the one frame
        fns = [lambda: variance(0), lambda: variance(65535), plain, lambda: call("", ps[-1])]
        fns += [(lambda f=f, p=p: call(f, p)) for f in FORMS for p in ps]
        head = 4
        raw = []
        m = measure(fns, args.rounds, window_ms=100.0, raw=raw,
                    names=[f"svgf {name} variance long", f"svgf {name} variance short",
                           f"svgf {name} filter", f"svgf {name} default"] +
                          [f"svgf {name} {f} passes {k}" for f in FORMS for k in range(1, passes + 1)])
        os.environ.pop("RTG_SVGF_FORM", None)
        vfloor = n * (4 + 8 * C + 2 + 4) / 6.0e12 * 1e3
        floor = n * (40 + 8 * C) / 6.0e12 * 1e3
        forms = {}
        for fi, f in enumerate(FORMS):
            cum = raw[head + fi * passes:head + (fi + 1) * passes]
            per = [cum[0]] + [[b - a for a, b in zip(cum[k - 1], cum[k])] for k in range(1, passes)]
            forms[f] = {"cumulative": m[head + fi * passes:head + (fi + 1) * passes],
                        "pass_ms_median": [round(float(np.median(v)), 5) for v in per],
                        "pass_ms_min": [round(min(v), 5) for v in per],
                        "pass_ms_max": [round(max(v), 5) for v in per],
                        "pass_over_floor": [round(float(np.median(v)) / floor, 2) for v in per]}
        # the call's own answer, then the torch chain of the same arithmetic
        variance(65535)
        call("", ps[-1])
        torch.cuda.synchronize()
        got, gvar = dst.clone(), dvar.clone()
        h = hits.view(torch.float32)
        ids = hits[:, 0].reshape(H, W).contiguous()
        P = [h[:, 2 + q].reshape(H, W).contiguous() for q in range(3)]
        N = [h[:, 5 + q].reshape(H, W).contiguous() for q in range(3)]
        img = [acc[:, q].reshape(H, W).contiguous() for q in range(C)]
        v0 = var.reshape(H, W)
        torch.cuda.synchronize()
        chain = lambda: torch_svgf(ids, P, N, img, v0, passes, flags, nlog, scale, sigma, eps)  # noqa: E731
        rimg, rvar = chain()
        ref, rvar = torch.stack(rimg, -1).reshape(n, C), rvar.reshape(n)
        torch.cuda.synchronize()
        tm = measure([chain], args.rounds, window_ms=100.0, min_reps=1,
                     names=[f"svgf {name} torch chain"])[0]

        def compare(a, b):
            fin = torch.isfinite(a) & torch.isfinite(b)
            rel = ((a - b).abs() / b.abs().clamp_min(1e-30))[fin]
            worst = float(rel.max()) if rel.numel() else 0.0
            words = int((a.view(torch.int32)[fin] != b.view(torch.int32)[fin]).sum())
            return bool((torch.isfinite(a) == torch.isfinite(b)).all()) and worst <= 1e-4, worst, words

        agree_v, worst_v, words_v = compare(got, ref)
        agree_s, worst_s, words_s = compare(gvar, rvar)
        ok = ok and agree_v and agree_s
        real = hits[:, 0] >= 0
        out[name] = {
            "W": W, "H": H, "kind": int(fkind), "hit_points": int(real.sum()), "plane_scale": scale,
            "variance_long": m[0], "variance_short": m[1],
            "variance_floor_ms": round(vfloor, 5),
            "variance_long_over_floor": round(m[0]["ms_median"] / vfloor, 2),
            "variance_short_over_floor": round(m[1]["ms_median"] / vfloor, 2),
            "filter": m[2], "default": m[3],
            "svgf_over_filter": round(m[3]["ms_median"] / m[2]["ms_median"], 2),
            "floor_ms_per_pass": round(floor, 5),
            "default_forms": "tiled up to step 4, direct beyond", "forms": forms,
            "svgf_scratch_bytes": nbytes, "torch_chain": tm,
            "torch_over_svgf": round(tm["ms_median"] / m[3]["ms_median"], 2),
            "changed_share_of_hit_pixels_against_filter": round(float(
                ((got != fdst).any(1) & real).sum() / real.sum()), 4),
            "largest_relative_difference": worst_v, "words_that_differ": words_v,
            "variance_largest_relative_difference": worst_s, "variance_words_that_differ": words_s,
            "agree_to_1e-4": agree_v and agree_s}
        print(f"svgf {name}: {m[3]['ms_median']} ms against the filter's {m[2]['ms_median']} ms, "
              f"variance {m[0]['ms_median']} / {m[1]['ms_median']} ms (floor {vfloor:.4f}), torch "
              f"{tm['ms_median']} ms, largest relative difference {worst_v:.3g} / {worst_s:.3g}",
              file=sys.stderr, flush=True)
        ctx.close()
        del hits, acc, m2, ln, var, dvar, dst, fdst, scratch, got, gvar, ref, rvar, rimg, ids, P, N
        del img, h, v0, real
        torch.cuda.empty_cache()
    return out, ok


def torch_accumulate(cur, prev, pose, W, H, zoom, flags, nlog, scale, max_history):
    """rtg_accumulate* (include/rtg.h) as a chain of torch operations in the
    definition's operand order: the projection, index gathers for the four taps,
    `where` for the rules and a lerp.  cur = (ids, P, N, value planes), prev =
    (ids, P, N, acc planes, len), planes of (H, W); returns (planes, len)."""
    ids, P, N, val = cur
    pid, pP, pN, pacc, plen = prev
    eye, right, up, back = (tuple(float(v) for v in pose[k].reshape(-1)) for k in
                            ("eye", "right", "up", "back"))
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    zero = torch.zeros((), dtype=torch.float32, device="cuda")
    e = [P[q] - eye[q] for q in range(3)]
    k = float(zoom) / dot(e, back)
    fx = (dot(e, right) * k) * float(F(W) * F(0.046875)) + float(F(W) * F(0.5))
    fy = float(F(H) * F(0.5)) - (dot(e, up) * k) * float(F(H) / F(12))
    ok = (k > 0) & (fx > -1) & (fx < W) & (fy > -1) & (fy < H) & (ids >= 0)
    xf, yf = torch.floor(fx), torch.floor(fy)
    tx, ty = fx - xf, fy - yf
    x0 = torch.where(ok, xf, zero).to(torch.int64)
    y0 = torch.where(ok, yf, zero).to(torch.int64)
    acc = [torch.zeros_like(v) for v in val]
    sw = torch.zeros_like(fx)
    nmin = torch.full_like(x0, 65535)
    for dy in (0, 1):
        for dx in (0, 1):
            xq, yq = x0 + dx, y0 + dy
            keep = ok & (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
            xs, ys = xq.clamp(0, W - 1), yq.clamp(0, H - 1)
            w = (ty if dy else 1.0 - ty) * (tx if dx else 1.0 - tx)
            idq, lq = pid[ys, xs], plen[ys, xs]
            keep &= (idq >= 0) & (lq != 0)
            if flags & R.ACCUM_SAME_ID:
                keep &= idq == ids
            if flags & R.ACCUM_NORMAL:
                c = dot(N, [pN[q][ys, xs] for q in range(3)])
                c = torch.where(c > 0, c, zero)
                for _ in range(nlog):
                    c = c * c
                w = w * c
            if flags & R.ACCUM_PLANE:
                d = dot(N, [pP[q][ys, xs] - P[q] for q in range(3)]).abs()
                z = 1.0 - d * scale
                w = w * torch.where(z > 0, z, zero)
            keep &= w > 0
            for q in range(len(val)):
                acc[q] = torch.where(keep, acc[q] + w * pacc[q][ys, xs], acc[q])
            sw = torch.where(keep, sw + w, sw)
            nmin = torch.where(keep, torch.minimum(nmin, lq), nmin)
    found = sw > 0
    n = torch.minimum(nmin + 1, torch.full_like(nmin, max_history))
    alpha = 1.0 / n.to(torch.float32)
    out = []
    for q in range(len(val)):
        hist = acc[q] / sw
        out.append(torch.where(found, hist + alpha * (val[q] - hist), val[q]))
    ln = torch.where(ids >= 0, torch.where(found, n, torch.ones_like(n)), torch.zeros_like(n))
    return out, ln


def accumulate_rows(args, stream):
    """Temporal accumulation (csrc/rtg_accumulate.hip) with SAME_ID | NORMAL |
    PLANE, planeScale 1 / (the scene's largest |radius|), normalLog2 3 and
    maxHistory 64: the K = 16 jittered AO counts and the K = 16 gathered light
    of the aa = 1 primary hits, 3840 x 2160 on C3 and 1920 x 1080 on C5, blended
    onto the state of a previous pose a small pan away and of one a roll away
    (that pose's own records and signal, every length 3).  Round by round in one
    process: the call, and a torch chain of the same arithmetic.
    Reported, not gated: every time, and the distance from the streaming floor
    (the current and the previous records, src, prevAcc, prevLen, outAcc and
    outLen once each at 6 TB/s; next to it the same with the previous state
    counted for the pixels that have a point only, which is what a frame with
    background moves).  Gated: the call's lengths are the chain's and
    its values agree to 1e-4 relative on finite pixels."""
    K, nlog, max_history = 16, 3, 64
    flags = R.ACCUM_SAME_ID | R.ACCUM_NORMAL | R.ACCUM_PLANE
    table = torch.from_numpy(R.ao_directions(K)).cuda()
    wt = torch.full((K,), 1.0 / K, dtype=torch.float32, device="cuda")
    eye, target = np.array((0.0, 0.0, 0.0)), np.array((0.0, 0.0, -10.0))
    moves = {"pan": R.camera_look_at(eye + (0.05, 0.02, 0.0), target + (0.03, 0.01, 0.0)),
             "roll": R.camera_look_at(eye, target, (0.03, 1.0, 0.0))}
    now = R.camera_look_at(eye, target)
    out, ok = {"flags": flags, "normalLog2": nlog, "maxHistory": max_history, "samples": K,
               "floor_bandwidth_TBps": 6.0, "moves": {
                   "pan": "eye +(0.05, 0.02, 0), target +(0.03, 0.01, 0)", "roll": "up (0.03, 1, 0)"}}, True
    for name, cfg, (W, H), kind in (("c3_count", "c3", CONFIGS["c3"][:2], R.FILTER_COUNT),
                                    ("c3_rgb", "c3", CONFIGS["c3"][:2], R.FILTER_RGB),
                                    ("c5_count_1080p", "c5", (1920, 1080), R.FILTER_COUNT),
                                    ("c5_rgb_1080p", "c5", (1920, 1080), R.FILTER_RGB)):
        n, S, C = W * H, CONFIGS[cfg][4] + 1, 3 if kind == R.FILTER_RGB else 1
        sph, lg = R.generate_scene(CONFIGS[cfg][2], CONFIGS[cfg][3], 42)
        scale = float(F(1) / np.abs(sph["radius"]).max())
        radius = float(F(2.5) * np.abs(sph["radius"]).max())
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")

        def frame(cam, seed):
            """(records, signal) of a pose."""
            hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
            ctx.camera_rays(cam, W, H, rays.data_ptr(), alias_factor=1.0, stream=stream)
            ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream)
            if kind == R.FILTER_COUNT:
                src = torch.empty((n,), dtype=torch.int16, device="cuda")
                ctx.ao_device(hits.data_ptr(), n, R.ao_params(K, radius, 1e-3, seed, R.AO_JITTER),
                              table.data_ptr(), K, src.data_ptr(), stream)
            else:
                src = torch.empty((n, 3), dtype=torch.float32, device="cuda")
                gp = R.gather_params(K, 1e-3, seed, R.GATHER_JITTER | R.GATHER_SKIP_NONFINITE)
                ctx.gather_device(hits.data_ptr(), n, gp, table.data_ptr(), wt.data_ptr(), K,
                                  src.data_ptr(), stack_size=S, stream=stream)
            torch.cuda.synchronize()
            return hits, src

        def planes(hits, src):
            h = hits.view(torch.float32)
            val = [(src.to(torch.int32) & 0xFFFF).to(torch.float32).reshape(H, W)] \
                if kind == R.FILTER_COUNT else [src[:, q].reshape(H, W).contiguous() for q in range(3)]
            return (hits[:, 0].reshape(H, W).contiguous(),
                    [h[:, 2 + q].reshape(H, W).contiguous() for q in range(3)],
                    [h[:, 5 + q].reshape(H, W).contiguous() for q in range(3)], val)

        hits, src = frame(now, 43)
        cur = planes(hits, src)
        p = R.accumulate_params(kind, flags, scale, nlog, max_history)
        o_acc = torch.empty((n, C), dtype=torch.float32, device="cuda")
        o_len = torch.empty((n,), dtype=torch.int16, device="cuda")
        bytes_px = 32 + (2 if kind == R.FILTER_COUNT else 12) + 32 + 4 * C + 2 + 4 * C + 2
        floor = n * bytes_px / 6.0e12 * 1e3
        # (a pixel without a point reads no previous state: the floor of this frame's traffic)
        n_hit = int((hits[:, 0] >= 0).sum())
        prev_px = 32 + 4 * C + 2
        floor_hit = (n * (bytes_px - prev_px) + n_hit * prev_px) / 6.0e12 * 1e3
        row = {"W": W, "H": H, "kind": int(kind), "hit_points": n_hit,
               "plane_scale": scale, "bytes_per_pixel": bytes_px, "floor_ms": round(floor, 5),
               "floor_ms_previous_state_of_hits_only": round(floor_hit, 5)}
        for move, cam in moves.items():
            p_hits, p_src = frame(cam, 42)
            pv = planes(p_hits, p_src)
            p_acc = torch.stack(pv[3], -1).reshape(n, C).contiguous()
            p_len = torch.full((n,), 3, dtype=torch.int16, device="cuda")
            prev = (cam, p_hits.data_ptr(), p_acc.data_ptr(), p_len.data_ptr())

            def call():
                ctx.accumulate_device(hits.data_ptr(), W, H, p, src.data_ptr(), o_acc.data_ptr(),
                                      o_len.data_ptr(), prev, stream=stream)

            m = measure([call], args.rounds, window_ms=100.0,
                        names=[f"accumulate {name} {move} default"])
            call()
            torch.cuda.synchronize()
            got, got_len = o_acc.clone(), o_len.to(torch.int64) & 0xFFFF
            tp = (pv[0], pv[1], pv[2], pv[3], p_len.to(torch.int64).reshape(H, W))
            chain = lambda: torch_accumulate(cur, tp, cam, W, H, -4.0, flags, nlog, scale,  # noqa: E731
                                             max_history)
            ref, ref_len = chain()
            ref = torch.stack(ref, -1).reshape(n, C)
            tm = measure([chain], args.rounds, window_ms=100.0, min_reps=1,
                         names=[f"accumulate {name} {move} torch chain"])[0]
            fin = torch.isfinite(got) & torch.isfinite(ref)
            same_len = bool((got_len == ref_len.reshape(-1)).all())
            rel = ((got - ref).abs() / ref.abs().clamp_min(1e-30))[fin]
            worst = float(rel.max()) if rel.numel() else 0.0
            agree = same_len and worst <= 1e-4 and \
                bool((torch.isfinite(got) == torch.isfinite(ref)).all())
            ok = ok and agree
            real = hits[:, 0] >= 0
            row[move] = {
                "default": m[0],
                "default_over_floor": round(m[0]["ms_median"] / floor, 2),
                "torch_chain": tm, "torch_over_accumulate": round(tm["ms_median"] / m[0]["ms_median"], 2),
                "found_share_of_hit_pixels": round(float(((got_len == 4) & real).sum() / real.sum()), 4),
                "lengths_equal": same_len, "largest_relative_difference": worst,
                "bit_equal": bool((got.view(torch.int32) == ref.view(torch.int32))[fin].all()),
                "agree_to_1e-4": agree}
            print(f"accumulate {name} {move}: {m[0]['ms_median']} ms (floor {floor:.4f}), torch "
                  f"{tm['ms_median']} ms, largest relative difference {worst:.3g}",
                  file=sys.stderr, flush=True)
            del p_hits, p_src, pv, p_acc, p_len, tp, ref, ref_len, got, got_len, fin, rel
        out[name] = row
        ctx.close()
        del hits, src, cur, rays, o_acc, o_len
        torch.cuda.empty_cache()
    return out, ok


def torch_upsample(full, low, L, W, H, flags, nlog, scale):
    """rtg_upsample* (include/rtg.h) as a chain of torch operations in the
    definition's operand order: index gathers for the four taps, `where` for the
    rules, the quotient, and `nonzero` for the list.  full = (ids, P, N), low =
    (ids, P, N, value planes), planes of (H, W) and (Hl, Wl); returns (planes,
    the holes' pixel indices)."""
    ids, P, N = full
    lid, lP, lN, val = low
    f, Wl, Hl = 1 << L, W >> L, H >> L
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    zero = torch.zeros((), dtype=torch.float32, device="cuda")
    y, x = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    x0, y0 = x >> L, y >> L
    tx = (x & (f - 1)).to(torch.float32) * (1.0 / f)
    ty = (y & (f - 1)).to(torch.float32) * (1.0 / f)
    acc = [torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in val]
    sw = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    for dy in (0, 1):
        for dx in (0, 1):
            xq, yq = x0 + dx, y0 + dy
            keep = (xq < Wl) & (yq < Hl) & (ids >= 0)
            xs, ys = xq.clamp(max=Wl - 1), yq.clamp(max=Hl - 1)
            w = (ty if dy else 1.0 - ty) * (tx if dx else 1.0 - tx)
            idq = lid[ys, xs]
            keep &= idq >= 0
            if flags & R.UPSAMPLE_SAME_ID:
                keep &= idq == ids
            if flags & R.UPSAMPLE_NORMAL:
                c = dot(N, [lN[q][ys, xs] for q in range(3)])
                c = torch.where(c > 0, c, zero)
                for _ in range(nlog):
                    c = c * c
                w = w * c
            if flags & R.UPSAMPLE_PLANE:
                d = dot(N, [lP[q][ys, xs] - P[q] for q in range(3)]).abs()
                z = 1.0 - d * scale
                w = w * torch.where(z > 0, z, zero)
            keep &= w > 0
            for q in range(len(val)):
                acc[q] = torch.where(keep, acc[q] + w * val[q][ys, xs], acc[q])
            sw = torch.where(keep, sw + w, sw)
    found = sw > 0
    out = [torch.where(found, a / sw, zero) for a in acc]
    holes = torch.nonzero(((ids >= 0) & ~found).reshape(-1)).reshape(-1)
    return out, holes


def upsample_rows(args, stream):
    """The guided upsampling (csrc/rtg_upsample.hip) with SAME_ID | NORMAL |
    PLANE, planeScale 4 / (the scene's largest |radius|) and normalLog2 3, from
    the identity pose.  THE CALL ALONE: the K = 16 AO counts (COUNT) and the
    direct light (RGB) of the low frame's aa = 1 primary hits brought up to
    3840 x 2160 on C3 and to 1920 x 1080 on C5, L = 1 and 2, with and without the
    hole list, against the streaming floor (32 B of record in and 4 C B out per
    full pixel, the low records and values once, at 6 TB/s) and against a torch
    chain of the same arithmetic plus `nonzero`.  Gated: the call's words and
    list are the chain's.  THE ROUTE: the gather at K = 16 on C5 at 1920 x 1080
    and the AO at K = 16 on C5 at 3840 x 2160, jitter off, at full resolution
    against the sum of low records + low signal + upsample with the list + pick
    + the signal on the holes + place, L = 1 and 2; the gather's low frame and
    its holes both through the fused call and through gather_rays + raytrace +
    a torch fold (mixed: both fused; mixed_low_unfused; mixed_unfused: both).
    Reported, not gated: every time, the hole share, and the mean and largest
    absolute difference of the mixed-resolution frame from the full one."""
    K, nlog = 16, 3
    flags = R.UPSAMPLE_SAME_ID | R.UPSAMPLE_NORMAL | R.UPSAMPLE_PLANE
    table = torch.from_numpy(R.ao_directions(K)).cuda()
    wt = torch.full((K,), 1.0 / K, dtype=torch.float32, device="cuda")
    cam = R.camera_identity()
    out, ok = {"flags": flags, "normalLog2": nlog, "plane_scale": "4 / largest |radius|",
               "samples": K, "floor_bandwidth_TBps": 6.0, "call": {}, "route": {}}, True

    def records(ctx, W, H):
        n = W * H
        rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        ctx.camera_rays(cam, W, H, rays.data_ptr(), alias_factor=1.0, stream=stream)
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream)
        torch.cuda.synchronize()
        return rays, hits

    def planes(hits, W, H):
        h = hits.view(torch.float32)
        return (hits[:, 0].reshape(H, W).contiguous(),
                [h[:, 2 + q].reshape(H, W).contiguous() for q in range(3)],
                [h[:, 5 + q].reshape(H, W).contiguous() for q in range(3)])

    # ---- the call alone ----
    for cfg, (W, H) in (("c3", CONFIGS["c3"][:2]), ("c5", (1920, 1080))):
        n = W * H
        sph, lg = R.generate_scene(CONFIGS[cfg][2], CONFIGS[cfg][3], 42)
        scale = float(F(4) / np.abs(sph["radius"]).max())
        radius = float(F(2.5) * np.abs(sph["radius"]).max())
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        _, hits = records(ctx, W, H)
        full = planes(hits, W, H)
        n_hit = int((hits[:, 0] >= 0).sum())
        nbytes = R.upsample_scratch(W, H, True)
        scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
        lst = torch.empty((n,), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
        for L in (1, 2):
            Wl, Hl = W >> L, H >> L
            nl = Wl * Hl
            _, low = records(ctx, Wl, Hl)
            lowp = planes(low, Wl, Hl)
            for kname, kind, C in (("count", R.FILTER_COUNT, 1), ("rgb", R.FILTER_RGB, 3)):
                if kind == R.FILTER_COUNT:
                    src = torch.empty((nl,), dtype=torch.int16, device="cuda")
                    ctx.ao_device(low.data_ptr(), nl, R.ao_params(K, radius, 1e-3, 42, 0),
                                  table.data_ptr(), K, src.data_ptr(), stream)
                    val = [(src.to(torch.int32) & 0xFFFF).to(torch.float32).reshape(Hl, Wl)]
                else:
                    src = torch.empty((nl, 3), dtype=torch.float32, device="cuda")
                    ctx.matte_device(low.data_ptr(), nl, src.data_ptr(), stream=stream)
                    torch.cuda.synchronize()
                    val = [src[:, q].reshape(Hl, Wl).contiguous() for q in range(3)]
                p = R.upsample_params(L, kind, flags, scale, nlog)
                dst = torch.empty((n, C), dtype=torch.float32, device="cuda")
                args_ = (hits.data_ptr(), W, H, p, low.data_ptr(), Wl, Hl, src.data_ptr(), dst.data_ptr())
                plain = lambda: ctx.upsample_device(*args_, stream=stream)  # noqa: E731
                listed = lambda: ctx.upsample_device(*args_, lst.data_ptr(), n, cnt.data_ptr(),  # noqa: E731
                                                     scratch.data_ptr(), nbytes, stream=stream)
                chain = lambda: torch_upsample(full, lowp + (val,), L, W, H, flags, nlog, scale)  # noqa: E731
                row_name = f"{cfg}_{kname}_L{L}"
                m = measure([plain, listed], args.rounds, window_ms=100.0,
                            names=[f"upsample {row_name} {k}" for k in ("no list", "list")])
                tm = measure([chain], args.rounds, window_ms=100.0, min_reps=1,
                             names=[f"upsample {row_name} torch chain"])[0]
                listed()
                torch.cuda.synchronize()
                holes = int(cnt.cpu().numpy().view(np.uint32)[0])
                ref, ref_holes = chain()
                ref = torch.stack(ref, -1).reshape(n, C)
                nan = torch.isnan(ref)
                same = bool(((dst.view(torch.int32) == ref.view(torch.int32)) | nan).all()) and \
                    bool((torch.isnan(dst) == nan).all())
                same_list = holes == ref_holes.numel() and \
                    bool((lst[:holes].to(torch.int64) == ref_holes).all())
                ok = ok and same and same_list
                floor = (n * (32 + 4 * C) + nl * (32 + (2 if kind == R.FILTER_COUNT else 12))) / 6.0e12 * 1e3
                out["call"][row_name] = {
                    "W": W, "H": H, "scaleLog2": L, "kind": int(kind), "hit_points": n_hit,
                    "holes": holes, "hole_share_of_hit_pixels": round(holes / max(n_hit, 1), 5),
                    "scratch_bytes": nbytes, "floor_ms": round(floor, 5),
                    "no_list": m[0], "list": m[1],
                    "no_list_over_floor": round(m[0]["ms_median"] / floor, 2),
                    "list_over_floor": round(m[1]["ms_median"] / floor, 2),
                    "torch_chain": tm, "torch_over_list": round(tm["ms_median"] / m[1]["ms_median"], 2),
                    "words_equal": same, "list_equal": same_list}
                print(f"upsample {row_name}: {m[0]['ms_median']} / {m[1]['ms_median']} ms (floor "
                      f"{floor:.4f}), torch {tm['ms_median']} ms, holes {holes}, equal "
                      f"{same and same_list}", file=sys.stderr, flush=True)
                del src, val, dst, ref, ref_holes, nan
            del low, lowp
        ctx.close()
        del hits, full, scratch, lst, cnt
        torch.cuda.empty_cache()

    # ---- the route it exists for ----
    sph, lg = R.generate_scene(CONFIGS["c5"][2], CONFIGS["c5"][3], 42)
    scale = float(F(4) / np.abs(sph["radius"]).max())
    radius = float(F(2.5) * np.abs(sph["radius"]).max())
    S = CONFIGS["c5"][4] + 1
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    gp = R.gather_params(K, 1e-3, 42, R.GATHER_SKIP_NONFINITE)
    ap = R.ao_params(K, radius, 1e-3, 42, 0)
    for rname, (W, H), kind, C in (("gather_c5_1080p", (1920, 1080), R.FILTER_RGB, 3),
                                   ("ao_c5_2160p", (3840, 2160), R.FILTER_COUNT, 1)):
        n = W * H
        rgb = kind == R.FILTER_RGB
        vdtype, vshape = (torch.float32, (3,)) if rgb else (torch.int16, ())
        _, hits = records(ctx, W, H)
        n_hit = int((hits[:, 0] >= 0).sum())
        whole = torch.empty((n,) + vshape, dtype=vdtype, device="cuda")

        def signal(h, m, dst):
            if rgb:
                ctx.gather_device(h.data_ptr(), m, gp, table.data_ptr(), wt.data_ptr(), K,
                                  dst.data_ptr(), stack_size=S, stream=stream)
            else:
                ctx.ao_device(h.data_ptr(), m, ap, table.data_ptr(), K, dst.data_ptr(), stream)

        nbytes = R.upsample_scratch(W, H, True)
        scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
        lst = torch.empty((n,), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
        mixed = torch.empty((n, C), dtype=torch.float32, device="cuda")
        picked = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        own = torch.empty((n,) + vshape, dtype=vdtype, device="cuda")
        signal(hits, n, whole)
        torch.cuda.synchronize()
        ref = whole.to(torch.float32).reshape(n, C) if rgb else \
            (whole.to(torch.int32) & 0xFFFF).to(torch.float32).reshape(n, C)
        row = {"W": W, "H": H, "kind": int(kind), "hit_points": n_hit, "stack_size": S}
        for L in (1, 2):
            Wl, Hl = W >> L, H >> L
            nl = Wl * Hl
            lrays = torch.empty((nl, 6), dtype=torch.float32, device="cuda")
            low = torch.empty((nl, 8), dtype=torch.int32, device="cuda")
            lsig = torch.empty((nl,) + vshape, dtype=vdtype, device="cuda")
            p = R.upsample_params(L, kind, flags | (R.UPSAMPLE_SKIP_NONFINITE if rgb else 0), scale, nlog)

            def low_records():
                ctx.camera_rays(cam, Wl, Hl, lrays.data_ptr(), alias_factor=1.0, stream=stream)
                ctx.intersect_device(lrays.data_ptr(), nl, low.data_ptr(), stream)

            def up():
                ctx.upsample_device(hits.data_ptr(), W, H, p, low.data_ptr(), Wl, Hl, lsig.data_ptr(),
                                    mixed.data_ptr(), lst.data_ptr(), n, cnt.data_ptr(),
                                    scratch.data_ptr(), nbytes, stream=stream)

            low_records()
            signal(low, nl, lsig)
            up()
            torch.cuda.synchronize()
            m_holes = int(cnt.cpu().numpy().view(np.uint32)[0])
            fns = [lambda: signal(hits, n, whole), low_records, lambda: signal(low, nl, lsig), up,
                   lambda: ctx.hits_pick_device(hits.data_ptr(), n, lst.data_ptr(), m_holes,
                                                picked.data_ptr(), stream=stream),
                   lambda: signal(picked, m_holes, own),
                   lambda: ctx.values_place_device(kind, own.data_ptr(), lst.data_ptr(), m_holes, n,
                                                   mixed.data_ptr(), stream=stream)]
            names = ["full", "low_records", "low_signal", "upsample_list", "pick", "holes_signal", "place"]
            if rgb:  # the low frame through the unfused chain too
                prays = torch.empty((nl * K, 6), dtype=torch.float32, device="cuda")
                pcols = torch.empty((nl * K, 3), dtype=torch.float32, device="cuda")
                fns += [lambda: ctx.gather_rays_device(low.data_ptr(), nl, gp, table.data_ptr(), K,
                                                       prays.data_ptr(), stream),
                        lambda: ctx.raytrace_device(prays.data_ptr(), nl * K, pcols.data_ptr(), S, stream),
                        lambda: (pcols.view(nl, K, 3) * wt.view(1, K, 1)).sum(1),
                        # (and the holes: a few dozen points leave the fused call's lanes idle)
                        lambda: ctx.gather_rays_device(picked.data_ptr(), m_holes, gp, table.data_ptr(),
                                                       K, prays.data_ptr(), stream),
                        lambda: ctx.raytrace_device(prays.data_ptr(), m_holes * K, pcols.data_ptr(), S,
                                                    stream),
                        lambda: (pcols[:m_holes * K].view(m_holes, K, 3) * wt.view(1, K, 1)).sum(1)]
                names += ["low_rays", "low_raytrace", "low_fold", "holes_rays", "holes_raytrace",
                          "holes_fold"]
            raw = []
            m = measure(fns, args.rounds, raw=raw, min_reps=2,
                        names=[f"route {rname} L{L} {k}" for k in names])
            torch.cuda.synchronize()
            sums = {"mixed": [sum(v) for v in zip(*raw[1:7])]}
            if rgb:
                sums["mixed_low_unfused"] = [sum(v) for v in zip(raw[1], raw[7], raw[8], raw[9], *raw[3:7])]
                sums["mixed_unfused"] = [sum(v) for v in zip(raw[1], *raw[7:10], raw[3], raw[4],
                                                             *raw[10:13], raw[6])]
            rows = _spread_rows(sums)
            diff = (mixed - ref).abs()[hits[:, 0] >= 0]
            diff = diff[torch.isfinite(diff)]
            row[f"L{L}"] = {
                **dict(zip(names, m)), **rows,
                "holes": m_holes, "hole_share_of_hit_pixels": round(m_holes / max(n_hit, 1), 5),
                "full_over_mixed": round(m[0]["ms_median"] / rows["mixed"]["ms_median"], 3),
                **({"low_fused_over_low_unfused": round(
                    m[2]["ms_median"] / (m[7]["ms_median"] + m[8]["ms_median"] + m[9]["ms_median"]), 3),
                    "full_over_mixed_unfused": round(
                        m[0]["ms_median"] / rows["mixed_unfused"]["ms_median"], 3)}
                   if rgb else {}),
                "mean_abs_difference_from_full": float(diff.mean()) if diff.numel() else 0.0,
                "largest_abs_difference_from_full": float(diff.max()) if diff.numel() else 0.0,
                "mean_of_full_signal": float(ref[hits[:, 0] >= 0][torch.isfinite(ref[hits[:, 0] >= 0])].mean())}
            print(f"route {rname} L{L}: full {m[0]['ms_median']} ms, mixed "
                  f"{rows['mixed']['ms_median']} ms, holes {m_holes} of {n_hit}", file=sys.stderr,
                  flush=True)
            del lrays, low, lsig
            if rgb:
                del prays, pcols
        out["route"][rname] = row
        del hits, whole, scratch, lst, cnt, mixed, picked, own, ref
        torch.cuda.empty_cache()
    ctx.close()
    return out, ok


def matte_rows(args, W, H, rays, stream):
    """Direct light (csrc/rtg_matte.hip) of the frame's 8.3 M aa = 1 primary
    hits on C3 (3 lights) and C5 (4 lights).  Round by round in one process: the
    fused call with and without the mask, and the pieces of the unfused path on
    the same hits: torch building the n x m segments (P, L) (24 m bytes per
    point), rtg_visible_device over them, and a torch fold of the same
    arithmetic (direction, incidence, inverse square, sum over the lights).
    The unfused row is the per-round sum of its pieces.  Reported, not gated:
    whether the fused call is slower than the unfused row by more than that
    row's own min-max spread, and whether torch's fold gives the fused words
    (its division and square root are torch's).  Gated: the sums with and
    without the mask are the same words."""
    n = W * H
    hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    out_m = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    out_p = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    lit = torch.empty((n,), dtype=torch.int64, device="cuda")
    out, ok = {}, True
    for name in ("c3", "c5"):
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        m = len(lg)
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream)
        real = hits[:, 0] >= 0
        P = hits[:, 2:5].view(torch.float32)
        N = hits[:, 5:8].view(torch.float32)
        Lp = torch.from_numpy(np.ascontiguousarray(lg["pos"], F)).cuda()
        Lc = torch.from_numpy(np.ascontiguousarray(lg["col"], F)).cuda()
        segs = torch.empty((n, m, 6), dtype=torch.float32, device="cuda")
        vis = torch.empty((n * m,), dtype=torch.uint8, device="cuda")

        def build():
            segs[:, :, :3] = P[:, None, :]
            segs[:, :, 3:] = Lp[None, :, :]

        def fold():
            dist = Lp[None, :, :] - P[:, None, :]
            gap = (dist[..., 0] * dist[..., 0] + dist[..., 1] * dist[..., 1]) + dist[..., 2] * dist[..., 2]
            d = (1.0 / torch.sqrt(gap))[..., None] * dist
            inc = (N[:, None, 0] * d[..., 0] + N[:, None, 1] * d[..., 1]) + N[:, None, 2] * d[..., 2]
            on = (vis.view(n, m) != 0) & (inc > 0) & real[:, None]
            w = torch.where(on, inc / gap, torch.zeros_like(inc))
            total = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            for l in range(m):  # in order, as the definition adds them
                total = total + w[:, l, None] * Lc[l][None, :]
            return total, on

        raw = []
        fm, fp, bd, vs, fo = measure(
            [lambda: ctx.matte_device(hits.data_ptr(), n, out_m.data_ptr(), lit.data_ptr(), stream),
             lambda: ctx.matte_device(hits.data_ptr(), n, out_p.data_ptr(), 0, stream),
             build,
             lambda: ctx.visible_device(segs.data_ptr(), n * m, vis.data_ptr(), stream),
             fold], args.rounds, raw=raw)
        total, on = fold()
        equal = bool((out_m.view(torch.int32) == out_p.view(torch.int32)).all())
        ok = ok and equal
        bits = torch.zeros((n,), dtype=torch.int64, device="cuda")
        for l in range(m):
            bits |= on[:, l].to(torch.int64) << l
        rows = _spread_rows({"unfused": [a + b + c for a, b, c in zip(raw[2], raw[3], raw[4])]})
        spread = rows["unfused"]["ms_max"] - rows["unfused"]["ms_min"]
        nz = (out_p.view(torch.int32) << 1 != 0).any(1)
        out[name] = {
            "lights": m, "hit_points": int(real.sum()), "segment_bytes": n * m * 24,
            "fused_with_mask": fm, "fused": fp, "segments_torch": bd, "visible": vs,
            "fold_torch": fo, **rows,
            "unfused_over_fused": round(rows["unfused"]["ms_median"] / fp["ms_median"], 3),
            "unfused_over_fused_with_mask": round(rows["unfused"]["ms_median"] / fm["ms_median"], 3),
            "fused_slower_than_unfused_by_more_than_its_spread":
                bool(max(fp["ms_median"], fm["ms_median"]) - rows["unfused"]["ms_median"] > spread),
            "Mpoints_per_s": round(n / (fp["ms_median"] * 1e-3) / 1e6, 1),
            "lit_share_of_hit_points": round(float(nz[real].to(torch.float64).mean()), 4),
            "fused_equals_fused_with_mask": equal,
            "torch_fold_equals_fused_share_of_points": round(float(
                (total.view(torch.int32) == out_p.view(torch.int32)).all(1).to(torch.float64).mean()), 6),
            "torch_mask_equals_fused_share_of_points": round(float(
                (bits == lit).to(torch.float64).mean()), 6)}
        print(f"matte {name}: fused {fp['ms_median']} ms ({fm['ms_median']} with the mask), unfused "
              f"{rows['unfused']['ms_median']} ms", file=sys.stderr, flush=True)
        ctx.close()
        del segs, vis
    return out, ok


def contains_rows(args, W, H, rays, stream):
    """Containment (contains_kernel, csrc/rtg_matte.hip) of the refraction test
    points P + 0.01 d of the same primary hits, C3 and C5.  Recorded only."""
    n = W * H
    hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    idx = torch.empty((n,), dtype=torch.int32, device="cuda")
    out = {}
    for name in ("c3", "c5"):
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream)
        pts = (hits[:, 2:5].view(torch.float32) + 0.01 * rays[:, 3:6]).contiguous()
        (row,) = measure([lambda: ctx.contains_device(pts.data_ptr(), n, idx.data_ptr(), stream)],
                         args.rounds)
        real = hits[:, 0] >= 0
        out[name] = dict(row, Mpoints_per_s=round(n / (row["ms_median"] * 1e-3) / 1e6, 1),
                         hit_points=int(real.sum()),
                         contained_share_of_hit_points=round(
                             float((idx[real] >= 0).to(torch.float64).mean()), 4))
        print(f"contains {name}: {row['ms_median']} ms", file=sys.stderr, flush=True)
        ctx.close()
    return out


def probe_positions(sph, n, seed=42):
    """n seeded positions, uniform in the box of the scene's spheres."""
    c = sph["pos"].astype(np.float64)
    r = np.abs(sph["radius"].astype(np.float64))[:, None]
    lo, hi = (c - r).min(0), (c + r).max(0)
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3))


def views_rows(args, stream):
    """A probe bake on C3 (stack size 6) and C5 (stack size 8) at aa = 1: 256
    probe positions (probe_positions) x the 6 poses of rtg_camera_cube = 1536
    views of 32 x 32 at zoom -1, the pose table resident.  Round by round in
    one process:
      (a) views        one rtg_render_views_device;
      (b) per_view     1536 rtg_render_camera_device calls on one stream (the
                       C entry point through prepared ctypes arguments: the
                       time includes the host's enqueue of 1536 launches, which
                       is what a caller of that route pays);
      (c) unfused      1536 rtg_camera_rays_device calls into one ray buffer
                       (24 B per ray), one rtg_raytrace_device over it and a
                       torch fold (at aa = 1: one multiply by 1/nS); the row
                       is the per-round sum of the three;
      ceiling          one rtg_render_camera_device of a 1536 x 1024 frame (the
                       same pixel count) from the first pose.
    Reported, not gated: the ratios, and whether (a) is faster than (b) and
    than (c) by more than the slower one's min-max spread.  Gated: the frames of
    (a), (b) and (c) are the same words."""
    import ctypes
    nP, Wv, Hv, aa, zoom = 256, 32, 32, 1.0, -1.0
    nV, per = nP * 6, Wv * Hv
    fa = torch.empty((nV, Hv, Wv, 3), dtype=torch.float32, device="cuda")
    fb = torch.empty((nV, Hv, Wv, 3), dtype=torch.float32, device="cuda")
    fc = torch.empty((nV, Hv, Wv, 3), dtype=torch.float32, device="cuda")
    big = torch.empty((1024, 1536, 3), dtype=torch.float32, device="cuda")
    gen = torch.empty((nV * per, 6), dtype=torch.float32, device="cuda")
    col = torch.empty((nV * per, 3), dtype=torch.float32, device="cuda")
    L = R.lib()
    vp, q = ctypes.c_void_p, ctypes.c_void_p(stream) if stream else None
    out = {"probes": nP, "views": nV, "width": Wv, "height": Hv, "alias_factor": aa, "zoom": zoom,
           "pixels": nV * per, "ray_buffer_bytes": nV * per * 24}
    ok = True
    for name in ("c3", "c5"):
        S = CONFIGS[name][4] + 1
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        cams = np.concatenate([R.camera_cube(e) for e in probe_positions(sph, nP)])
        d_cams = torch.from_numpy(cams.view(F).reshape(nV, 12)).cuda()
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        h = ctx._h
        pose_p = [vp(cams.ctypes.data + 48 * v) for v in range(nV)]
        dst_p = [vp(fb.data_ptr() + 12 * per * v) for v in range(nV)]
        gen_p = [vp(gen.data_ptr() + 24 * per * v) for v in range(nV)]
        zf, af = ctypes.c_float(zoom), ctypes.c_float(aa)

        def per_view():
            for v in range(nV):
                if L.rtg_render_camera_device(h, pose_p[v], Wv, Hv, zf, af, S, dst_p[v], q):
                    raise R.RtgError(L.rtg_last_error().decode())

        def generate():
            for v in range(nV):
                if L.rtg_camera_rays_device(h, pose_p[v], Wv, Hv, zf, af, gen_p[v], q):
                    raise R.RtgError(L.rtg_last_error().decode())

        raw = []
        va, vb, vg, vt, vf, vc = measure(
            [lambda: ctx.render_views(d_cams.data_ptr(), nV, Wv, Hv, fa.data_ptr(), zoom, aa, S,
                                      stream),
             per_view, generate,
             lambda: ctx.raytrace_device(gen.data_ptr(), nV * per, col.data_ptr(), S, stream),
             lambda: torch.mul(col, 1.0 / (aa * aa), out=fc.view(-1, 3)),
             lambda: ctx.render_camera(cams[0], 1536, 1024, big.data_ptr(), zoom, aa, S, stream)],
            args.rounds, raw=raw, min_reps=1,  # (a per-view bake is 1536 launches: one a round)
            names=[f"views {name} {k}" for k in ("one launch", "per view", "generator per view",
                                                 "raytrace", "fold", "one frame")])
        ctx.close()
        words = lambda t: t.view(torch.int32)  # noqa: E731
        equal = bool((words(fa) == words(fb)).all()) and bool((words(fa) == words(fc)).all())
        ok = ok and equal
        rows = _spread_rows({"unfused": [a + b + c for a, b, c in zip(raw[2], raw[3], raw[4])]})
        un = rows["unfused"]

        def beats(x):
            return bool(x["ms_median"] - va["ms_median"] > x["ms_max"] - x["ms_min"])

        out[name] = {
            "stack_size": S, "views": va, "per_view": vb, "generator_per_view": vg,
            "raytrace": vt, "fold_torch": vf, **rows, "ceiling_one_frame": vc,
            "per_view_over_views": round(vb["ms_median"] / va["ms_median"], 3),
            "unfused_over_views": round(un["ms_median"] / va["ms_median"], 3),
            "views_over_ceiling": round(va["ms_median"] / vc["ms_median"], 3),
            "views_faster_than_per_view_by_more_than_its_spread": beats(vb),
            "views_faster_than_unfused_by_more_than_its_spread": beats(un),
            "Mpixels_per_s": round(nV * per / (va["ms_median"] * 1e-3) / 1e6, 1),
            "lit_share_of_pixels": round(float((fa != 0).any(-1).to(torch.float64).mean()), 4),
            "views_equal_per_view_and_unfused": equal}
        print(f"views {name}: one launch {va['ms_median']} ms, per view {vb['ms_median']} ms, "
              f"unfused {un['ms_median']} ms, one frame {vc['ms_median']} ms", file=sys.stderr,
              flush=True)
    return out, ok


def fold_rows(args, stream):
    """The bake of views_rows (256 probes x 6 faces of 32 x 32 at aa 1, C3 and
    C5) reduced to SH9 coefficients with rtg_cube_sh_weights' table (G = 6, K =
    9), round by round in one process:
      (a) fused        one rtg_render_views_fold_device: no frame anywhere;
      (b) unfused      rtg_render_views_device into a frame buffer, then
                       rtg_views_fold_device over it (the row is the per-round
                       sum; each part has a row of its own);
      (c) torch        the same frames, a torch mask of the non-finite pixels
                       and a torch einsum with the table (the per-round sum;
                       its summation order is torch's).
    All three with RTG_FOLD_SKIP_NONFINITE's rule: most probes of these scenes
    see a NaN or infinite pixel, which would otherwise spoil every coefficient.
    views is this session's rtg_render_views_device alone: what (a) is compared
    with.  Reported, not gated: the times, (a) minus views against views'
    min-max spread, and the bytes each route allocates besides the poses, the
    table and the nGroups * K coefficients (faces nViews * W * H * 12; partials
    nViews * tiles * (3K + 1) * 4; torch's peak above the faces during the
    einsum).  Gated: (a) and (b) are the same words."""
    nP, Wv, Hv, aa, zoom, bands = 256, 32, 32, 1.0, -1.0, 3
    K, nV = bands * bands, nP * 6
    frames = torch.empty((nV, Hv, Wv, 3), dtype=torch.float32, device="cuda")
    table = R.cube_sh_weights(Wv, bands, aa)
    d_w = torch.from_numpy(table).cuda()
    p = R.fold_params(6, K, R.FOLD_SKIP_NONFINITE)  # (most probes see a non-finite pixel)
    zero = torch.zeros((), dtype=torch.float32, device="cuda")
    skipped = torch.zeros((nP,), dtype=torch.int32, device="cuda")
    nbytes = R.views_fold_scratch(nV, Wv, Hv, K)
    scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
    oa = torch.zeros((nP, K, 3), dtype=torch.float32, device="cuda")
    ob = torch.zeros((nP, K, 3), dtype=torch.float32, device="cuda")
    oc = torch.zeros((nP, K, 3), dtype=torch.float32, device="cuda")
    out = {"probes": nP, "views": nV, "width": Wv, "height": Hv, "alias_factor": aa, "zoom": zoom,
           "weights": K, "views_per_group": 6,
           "bytes": {"faces": nV * Wv * Hv * 12, "partials": nbytes, "coefficients": nP * K * 12,
                     "table": table.nbytes, "fused": nbytes, "unfused": nV * Wv * Hv * 12 + nbytes}}
    ok = True
    for name in ("c3", "c5"):
        S = CONFIGS[name][4] + 1
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        cams = np.concatenate([R.camera_cube(e) for e in probe_positions(sph, nP)])
        d_cams = torch.from_numpy(cams.view(F).reshape(nV, 12)).cuda()
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)

        def einsum():
            fr = frames.view(nP, 6, Hv, Wv, 3)  # a pixel with a NaN or infinite word adds nothing
            fr = torch.where(torch.isfinite(fr).all(-1, keepdim=True), fr, zero)
            oc.copy_(torch.einsum("pfhwc,fhwk->pkc", fr, d_w))

        raw = []
        fu, vw, fo, es = measure(
            [lambda: ctx.render_views_fold(d_cams.data_ptr(), nV, Wv, Hv, p, d_w.data_ptr(),
                                           oa.data_ptr(), scratch.data_ptr(), nbytes,
                                           skipped_ptr=skipped.data_ptr(), zoom=zoom,
                                           alias_factor=aa, stack_size=S, stream=stream),
             lambda: ctx.render_views(d_cams.data_ptr(), nV, Wv, Hv, frames.data_ptr(), zoom, aa,
                                      S, stream),
             lambda: ctx.views_fold(frames.data_ptr(), nV, Wv, Hv, p, d_w.data_ptr(),
                                    ob.data_ptr(), scratch.data_ptr(), nbytes, stream=stream),
             einsum],
            args.rounds, raw=raw, names=[f"fold {name} {k}" for k in ("fused", "views",
                                                                      "views_fold", "einsum")])
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        einsum()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        ctx.close()
        equal = bool((oa.view(torch.int32) == ob.view(torch.int32)).all())
        ok = ok and equal
        rows = _spread_rows({"unfused": [a + b for a, b in zip(raw[1], raw[2])],
                             "torch": [a + b for a, b in zip(raw[1], raw[3])]})
        finite = torch.isfinite(oa) & torch.isfinite(oc)
        out[name] = {
            "stack_size": S, "fused": fu, "views": vw, "views_fold": fo, "einsum": es, **rows,
            "fused_minus_views_ms": round(fu["ms_median"] - vw["ms_median"], 5),
            "views_spread_ms": round(vw["ms_max"] - vw["ms_min"], 5),
            "fused_over_views": round(fu["ms_median"] / vw["ms_median"], 4),
            "fused_over_unfused": round(fu["ms_median"] / rows["unfused"]["ms_median"], 4),
            "fused_over_torch": round(fu["ms_median"] / rows["torch"]["ms_median"], 4),
            "einsum_peak_bytes_above_faces": int(peak),
            "fused_equals_unfused": equal,
            "non_finite_coefficients": int((~torch.isfinite(oa)).sum()),
            "skipped_share_of_pixels": round(float(skipped.sum()) / (nV * Wv * Hv), 4),
            "probes_with_a_skipped_pixel": int((skipped > 0).sum()),
            "max_abs_difference_from_einsum": float((oa - oc)[finite].abs().max()) if finite.any()
            else None}
        print(f"fold {name}: fused {fu['ms_median']} ms, views alone {vw['ms_median']} ms, "
              f"unfused {rows['unfused']['ms_median']} ms, torch {rows['torch']['ms_median']} ms",
              file=sys.stderr, flush=True)
    return out, ok


def irradiance_rows(args, stream):
    """The probe grid's lookup (csrc/rtg_irradiance.hip) at the aa = 1 primary
    hits of C3 at 3840 x 2160 and of C5 at 1920 x 1080.  The grid: 8 x 8 x 4 SH9
    probes over the box of the scene's spheres, baked as fold_rows bakes (32 x 32
    faces at aa 1, rtg_cube_sh_weights, RTG_FOLD_SKIP_NONFINITE, the config's
    stack size), validity from rtg_contains_device; bias 1e-3, RTG_IRR_LOBE_COSINE.
    Per flag set (none, VALID | FACING, all three), round by round in one process:
      fused          rtg_irradiance_device with the weight buffer;
      fused_no_weight the same without it;
      cells_torch    torch forming A, the cell, the eight weights, probe indices
                     and positions and the n x 8 segments (A, X_p) (192 bytes
                     per point), op by op as rtg.h orders them;
      visible        rtg_visible_device over the n x 8 segments (with VISIBLE);
      fold_torch     a torch gather and fold of the same arithmetic.
    The unfused row is the per-round sum of its pieces.  Reported, not gated:
    the times, the ratio to the floor at 6 TB/s (32 B in, 12 B out and 4 B of
    weight per point) and whether the fused call is faster than the chain by
    more than the chain's own min-max spread.  Gated: the fused call with and
    without the weight buffer and the torch chain give the same words (NaN
    canonicalised), colours and weights."""
    bands, K, res_, bias = 3, 9, 32, 1e-3
    dims = (8, 8, 4)
    nP = dims[0] * dims[1] * dims[2]
    lobe = R.IRR_LOBE_COSINE
    c0, c1, c2, c3, c4 = (float(F(v)) for v in (0.28209479177387814, 0.4886025119029199,
                                                  1.0925484305920792, 0.31539156525252005,
                                                  0.5462742152960396))
    l0, l1, l2 = (float(F(v)) for v in lobe)
    table = torch.from_numpy(R.cube_sh_weights(res_, bands, 1.0)).cuda()
    fp = R.fold_params(6, K, R.FOLD_SKIP_NONFINITE)
    nbytes = R.views_fold_scratch(6 * nP, res_, res_, K)
    scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
    out, ok = {"grid": list(dims), "bands": bands, "face": res_, "bias": bias,
               "lobe": [l0, l1, l2]}, True
    for name, (W, H) in (("c3", (3840, 2160)), ("c5", (1920, 1080))):
        n = W * H
        S = CONFIGS[name][4] + 1
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        c = sph["pos"].astype(F)
        r = np.abs(sph["radius"].astype(F))[:, None]
        lo, hi = (c - r).min(0), (c + r).max(0)
        step = np.array([(hi[q] - lo[q]) / F(dims[q] - 1) for q in range(3)], F)
        g = R.probe_grid(lo, step, dims, bands)
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        rays = torch.from_numpy(primary_rays(W, H)).cuda()
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream)
        d_cams = torch.from_numpy(R.probe_grid_poses(g).view(F).reshape(6 * nP, 12)).cuda()
        d_pts = torch.from_numpy(R.probe_grid_points(g)).cuda()
        coef = torch.zeros((nP * K, 3), dtype=torch.float32, device="cuda")
        inside = torch.zeros((nP,), dtype=torch.int32, device="cuda")
        ctx.render_views_fold(d_cams.data_ptr(), 6 * nP, res_, res_, fp, table.data_ptr(),
                              coef.data_ptr(), scratch.data_ptr(), nbytes, zoom=-1.0,
                              alias_factor=1.0, stack_size=S, stream=stream)
        ctx.contains_device(d_pts.data_ptr(), nP, inside.data_ptr(), stream)
        valid = (inside < 0).to(torch.uint8)
        real = hits[:, 0] >= 0
        P = hits[:, 2:5].view(torch.float32)
        N = hits[:, 5:8].view(torch.float32)
        o_t = torch.from_numpy(np.ascontiguousarray(g["origin"][0])).cuda()
        s_t = torch.from_numpy(np.ascontiguousarray(g["step"][0])).cuda()
        top = torch.tensor([d - 1 for d in dims], dtype=torch.float32, device="cuda")
        nm2 = torch.tensor([max(d - 2, 0) for d in dims], dtype=torch.int32, device="cuda")
        nm1 = torch.tensor([d - 1 for d in dims], dtype=torch.int32, device="cuda")
        zero = torch.zeros((), dtype=torch.float32, device="cuda")
        segs = torch.empty((n, 8, 6), dtype=torch.float32, device="cuda")
        vis = torch.empty((n * 8,), dtype=torch.uint8, device="cuda")
        state = {}

        def cells():
            A = P + bias * N
            gq = (A - o_t) / s_t  # (tensor / tensor: a true division, not a reciprocal)
            gq = torch.where(gq >= 0, gq, zero)
            gq = torch.where(gq > top, top, gq)
            i0 = torch.minimum(gq.to(torch.int32), nm2)
            f = gq - i0.to(torch.float32)
            i1 = torch.minimum(i0 + 1, nm1)
            g1 = 1.0 - f
            w = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            p = torch.empty((n, 8), dtype=torch.int64, device="cuda")
            for cnr in range(8):
                bit = (cnr & 1, (cnr >> 1) & 1, cnr >> 2)
                i = [(i1 if bit[q] else i0)[:, q] for q in range(3)]
                t = [(f if bit[q] else g1)[:, q] for q in range(3)]
                w[:, cnr] = (t[0] * t[1]) * t[2]
                p[:, cnr] = ((i[2] * dims[1] + i[1]) * dims[0] + i[0]).to(torch.int64)
                segs[:, cnr, :3] = A
                for q in range(3):
                    along = i[q].to(torch.float32) * s_t[q]
                    segs[:, cnr, 3 + q] = o_t[q] + along
            state["w"], state["p"] = w, p

        def fold(flags):
            w, p = state["w"], state["p"]
            x, y, z = N[:, 0], N[:, 1], N[:, 2]
            b = [torch.full((n,), float(F(l0) * F(c0)), dtype=torch.float32, device="cuda"),
                 l1 * (c1 * y), l1 * (c1 * z), l1 * (c1 * x),
                 l2 * (c2 * (x * y)), l2 * (c2 * (y * z)), l2 * (c3 * ((3.0 * (z * z)) - 1.0)),
                 l2 * (c2 * (x * z)), l2 * (c4 * ((x * x) - (y * y)))]
            acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            Wt = torch.zeros((n,), dtype=torch.float32, device="cuda")
            for cnr in range(8):
                keep = real & (w[:, cnr] > 0)
                if flags & R.IRR_VALID:
                    keep &= valid[p[:, cnr]] != 0
                if flags & R.IRR_FACING:
                    d = segs[:, cnr, 3:] - segs[:, cnr, :3]
                    sx = N[:, 0] * d[:, 0]
                    sy = N[:, 1] * d[:, 1]
                    sz = N[:, 2] * d[:, 2]
                    keep &= ((sx + sy) + sz) > 0
                if flags & R.IRR_VISIBLE:
                    keep &= vis.view(n, 8)[:, cnr] != 0
                e = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
                for k in range(K):
                    e = e + b[k][:, None] * coef[p[:, cnr] * K + k]
                Wt = torch.where(keep, Wt + w[:, cnr], Wt)
                acc = torch.where(keep[:, None], acc + w[:, cnr, None] * e, acc)
            res = torch.where((Wt > 0)[:, None], acc / Wt[:, None], zero)
            return res, Wt

        def words(t):
            bits = t.contiguous().view(torch.int32)  # NaN as 0xFFC00000, the records' form
            return torch.where(torch.isnan(t), torch.full_like(bits, -0x400000), bits)

        oa = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        ob = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        wa = torch.empty((n,), dtype=torch.float32, device="cuda")
        floor_ms = n * 48 / 6.0e12 * 1e3
        out[name] = {"W": W, "H": H, "points": n, "hit_points": int(real.sum()), "stack_size": S,
                     "valid_probes": int(valid.sum()), "segment_bytes": n * 8 * 24,
                     "floor_ms_at_6TBps_48B_per_point": round(floor_ms, 5)}
        for label, flags in (("none", 0), ("valid_facing", 3), ("all", 7)):
            pr = R.irradiance_params(bias, lobe, flags)
            fns = [lambda: ctx.irradiance_device(hits.data_ptr(), n, g, coef.data_ptr(), pr,
                                                 oa.data_ptr(), valid_ptr=valid.data_ptr(),
                                                 weight_ptr=wa.data_ptr(), stream=stream),
                   lambda: ctx.irradiance_device(hits.data_ptr(), n, g, coef.data_ptr(), pr,
                                                 ob.data_ptr(), valid_ptr=valid.data_ptr(),
                                                 stream=stream),
                   cells, lambda: fold(flags)]
            names = ["fused", "fused_no_weight", "cells_torch", "fold_torch"]
            if flags & R.IRR_VISIBLE:
                fns.append(lambda: ctx.visible_device(segs.data_ptr(), n * 8, vis.data_ptr(), stream))
                names.append("visible")
            cells()  # (fold and visible read its state in their warm-up launches)
            ctx.visible_device(segs.data_ptr(), n * 8, vis.data_ptr(), stream)
            raw = []
            rows = measure(fns, args.rounds, raw=raw, min_reps=2,
                           names=[f"irradiance {name} {label} {k}" for k in names])
            tw, tW = fold(flags)
            torch.cuda.synchronize()
            same = bool((words(oa) == words(ob)).all())
            chain = bool((words(oa) == words(tw)).all() and (words(wa) == words(tW)).all())
            ok = ok and same and chain
            sums = _spread_rows({"unfused": [sum(v) for v in zip(*raw[2:])]})
            spread = sums["unfused"]["ms_max"] - sums["unfused"]["ms_min"]
            fu = rows[0]
            out[name][label] = dict(
                zip(names, rows), **sums, flags=flags,
                unfused_over_fused=round(sums["unfused"]["ms_median"] / fu["ms_median"], 3),
                fused_faster_than_unfused_by_more_than_its_spread=bool(
                    sums["unfused"]["ms_median"] - fu["ms_median"] > spread),
                fused_over_floor=round(fu["ms_median"] / floor_ms, 2),
                Mpoints_per_s=round(n / (fu["ms_median"] * 1e-3) / 1e6, 1),
                zero_weight_share_of_hit_points=round(
                    float((wa[real] == 0).to(torch.float64).mean()), 4),
                fused_equals_fused_no_weight=same, fused_equals_torch_chain=chain,
                torch_chain_differing_points=int((words(oa) != words(tw)).any(1).sum()))
            print(f"irradiance {name} {label}: fused {fu['ms_median']} ms, unfused "
                  f"{sums['unfused']['ms_median']} ms, floor {floor_ms:.4f} ms", file=sys.stderr,
                  flush=True)
        ctx.close()
        del segs, vis, state
    return out, ok


def finish(args, res, ok):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays", "bench.json"))
    ap.add_argument("--parent-json", default="")
    ap.add_argument("--commit", default="", help="recorded as the commit the numbers are of")
    ap.add_argument("--only-camera", action="store_true", help="the posed camera's rows alone")
    ap.add_argument("--only-order", action="store_true", help="the ray order's rows alone")
    ap.add_argument("--only-ao", action="store_true",
                    help="the ambient occlusion's rows alone, put into FILE next to what it holds")
    ap.add_argument("--only-matte", action="store_true",
                    help="the direct light's and the containment's rows alone, put into FILE "
                         "next to what it holds")
    ap.add_argument("--only-views", action="store_true",
                    help="the many-views rows alone, put into FILE next to what it holds")
    ap.add_argument("--only-fold", action="store_true",
                    help="the rows of the views folded into SH coefficients alone, put into FILE "
                         "next to what it holds")
    ap.add_argument("--only-gather", action="store_true",
                    help="the gather's rows alone, put into FILE next to what it holds")
    ap.add_argument("--only-filter", action="store_true",
                    help="the filter's rows alone, put into FILE next to what it holds")
    ap.add_argument("--only-accumulate", action="store_true",
                    help="the temporal accumulation's rows alone, put into FILE next to what it holds")
    ap.add_argument("--only-svgf", action="store_true",
                    help="the variance estimate's and the variance-guided passes' rows alone, put into "
                         "FILE next to what it holds")
    ap.add_argument("--only-upsample", action="store_true",
                    help="the guided upsampling's rows and the mixed-resolution route alone, put into "
                         "FILE next to what it holds")
    ap.add_argument("--only-irradiance", action="store_true",
                    help="the probe grid's lookup rows alone, put into FILE next to what it holds")
    ap.add_argument("--parent-commit", default="",
                    help="recorded with --only-fold, --only-gather, --only-filter, --only-accumulate or "
                         "--only-svgf as the parent "
                         "of --commit")
    ap.add_argument("--order-label", default="origin-major b=10 c=10",
                    help="recorded as the library's key layout and bit counts")
    ap.add_argument("--order-alt-json", default=[], action="append",
                    help="an --only-order file of another key layout, for the side-by-side")
    ap.add_argument("--mapping", default="8x8", help="recorded as the library's lane-to-pixel mapping")
    ap.add_argument("--mapping-json", default="",
                    help="a --only-camera file of a build with another mapping, for the side-by-side")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rays: needs a GPU")
    if args.only_views:  # (before the frame's ray buffers: it needs none of them)
        res = {}
        if os.path.exists(args.out):  # the other sections stay as they were measured
            with open(args.out) as f:
                res = json.load(f)
        res["views_commit"] = args.commit
        res["views"], ok = views_rows(args, torch.cuda.current_stream().cuda_stream)
        res["views"]["rounds"] = args.rounds
        finish(args, res, ok)
    if args.only_fold:  # (the same: poses in, coefficients out)
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["fold_commit"], res["fold_parent_commit"] = args.commit, args.parent_commit
        res["fold"], ok = fold_rows(args, torch.cuda.current_stream().cuda_stream)
        res["fold"]["rounds"] = args.rounds
        finish(args, res, ok)
    if args.only_gather:  # (the same: it makes the hits of its own two frames)
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["gather_commit"], res["gather_parent_commit"] = args.commit, args.parent_commit
        res["gather"], ok = gather_rows(args, torch.cuda.current_stream().cuda_stream)
        res["gather"]["rounds"] = args.rounds
        finish(args, res, ok)
    if args.only_filter:  # (the same: it makes the hits and the signals of its own frames)
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["filter_commit"], res["filter_parent_commit"] = args.commit, args.parent_commit
        res["filter"], ok = filter_rows(args, torch.cuda.current_stream().cuda_stream)
        res["filter"]["rounds"] = args.rounds
        finish(args, res, ok)
    if args.only_accumulate:  # (the same: it makes the frames of its own poses)
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["accumulate_commit"], res["accumulate_parent_commit"] = args.commit, args.parent_commit
        res["accumulate"], ok = accumulate_rows(args, torch.cuda.current_stream().cuda_stream)
        res["accumulate"]["rounds"] = args.rounds
        finish(args, res, ok)
    if args.only_svgf:  # (the same: it makes the accumulated frames of its own)
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["svgf_commit"], res["svgf_parent_commit"] = args.commit, args.parent_commit
        res["svgf"], ok = svgf_rows(args, torch.cuda.current_stream().cuda_stream)
        res["svgf"]["rounds"] = args.rounds
        finish(args, res, ok)
    if args.only_upsample:  # (the same: it makes the low and the full frames of its own)
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["upsample_commit"], res["upsample_parent_commit"] = args.commit, args.parent_commit
        res["upsample"], ok = upsample_rows(args, torch.cuda.current_stream().cuda_stream)
        res["upsample"]["rounds"] = args.rounds
        finish(args, res, ok)
    if args.only_irradiance:  # (the same: it makes the hits and the grid of its own frames)
        res = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["irradiance_commit"], res["irradiance_parent_commit"] = args.commit, args.parent_commit
        res["irradiance"], ok = irradiance_rows(args, torch.cuda.current_stream().cuda_stream)
        res["irradiance"]["rounds"] = args.rounds
        finish(args, res, ok)
    W, H = CONFIGS["c3"][0], CONFIGS["c3"][1]
    assert (W, H) == CONFIGS["c5"][:2]
    n = W * H
    rays_np = primary_rays(W, H)
    perm = np.random.default_rng(42).permutation(n)
    rays = torch.from_numpy(rays_np).cuda()
    shuffled = torch.from_numpy(rays_np[perm]).cuda()
    hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    hits2 = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    gb = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    res = {"W": W, "H": H, "rays": n, "device": R.device_info(0), "rounds": args.rounds,
           "commit": args.commit, "batches": {}}

    if args.only_order:
        del hits, hits2, gb
        res["order"], ok = order_rows(args, n, rays, shuffled, stream)
        finish(args, res, ok)

    if args.only_ao:
        del hits, hits2, gb, shuffled
        if os.path.exists(args.out):  # the other sections stay as they were measured
            with open(args.out) as f:
                res = dict(json.load(f), ao_commit=args.commit)
        res["ao"], ok = ao_rows(args, W, H, rays, stream)
        finish(args, res, ok)

    if args.only_matte:
        del hits, hits2, gb, shuffled
        if os.path.exists(args.out):  # the other sections stay as they were measured
            with open(args.out) as f:
                res = dict(json.load(f), matte_commit=args.commit)
        res["matte"], ok = matte_rows(args, W, H, rays, stream)
        res["contains"] = contains_rows(args, W, H, rays, stream)
        finish(args, res, ok)

    if args.only_camera:
        del hits, hits2, gb, shuffled
        col = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        res["camera"], ok = camera_rows(args, W, H, rays, col, fb, stream)
        finish(args, res, ok)

    def rate(m):
        m["Mrays_per_s"] = round(n / (m["ms_median"] * 1e-3) / 1e6, 1)
        return m

    # C3: ordered batch and the G-buffer at aa = 1 of the same frame
    sph, lg = R.generate_scene(CONFIGS["c3"][2], CONFIGS["c3"][3], 42)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    q, g = measure([lambda: ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream),
                    lambda: ctx.gbuffer_device(W, H, gb.data_ptr(), alias_factor=1.0,
                                               stream=stream)], args.rounds)
    ctx.close()
    res["batches"]["c3_ordered"] = rate(q)
    same = bool((hits[:, :2] == gb[:, :2]).all() and (hits[:, 5:8] == gb[:, 4:7]).all())
    res["gbuffer_aa1_c3"] = dict(g, intersect_over_gbuffer=round(q["ms_median"] / g["ms_median"], 3),
                                 hits_equal_gbuffer=same,
                                 hit_rays=int((hits[:, 0] >= 0).sum()))

    # C5: ordered and shuffled
    sph, lg = R.generate_scene(CONFIGS["c5"][2], CONFIGS["c5"][3], 42)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    o, s = measure([lambda: ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream),
                    lambda: ctx.intersect_device(shuffled.data_ptr(), n, hits2.data_ptr(), stream)],
                   args.rounds)
    ctx.close()
    res["batches"]["c5_ordered"] = rate(o)
    res["batches"]["c5_shuffled"] = rate(s)
    res["c5_shuffled_over_ordered"] = round(s["ms_median"] / o["ms_median"], 3)
    permuted = bool((hits[torch.from_numpy(perm).cuda()] == hits2).all())
    res["c5_shuffled_hits_are_ordered_permuted"] = permuted
    res["c5_hit_rays"] = int((hits[:, 0] >= 0).sum())
    del hits, hits2, gb

    # the batch ray tracer next to the render of the same rays
    col = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    col2 = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    dperm = torch.from_numpy(perm).cuda()
    res["raytrace"] = {}
    ok = True
    for name in ("c3", "c5"):
        S = CONFIGS[name][4] + 1
        sph, lg = R.generate_scene(CONFIGS[name][2], CONFIGS[name][3], 42)
        ctx = R.Context(0)
        ctx.set_scene(sph, lg)
        o, s, r = measure(
            [lambda: ctx.raytrace_device(rays.data_ptr(), n, col.data_ptr(), S, stream),
             lambda: ctx.raytrace_device(shuffled.data_ptr(), n, col2.data_ptr(), S, stream),
             lambda: ctx.render_device(W, H, fb.data_ptr(), alias_factor=1.0, stack_size=S,
                                       stream=stream)], args.rounds)
        ctx.close()
        # NaNs as written (0xFFC00000 on both sides): compare the words
        frame = bool((col.view(torch.int32) == fb.view(-1, 3).view(torch.int32)).all())
        permuted = bool((col[dperm].view(torch.int32) == col2.view(torch.int32)).all())
        ok = ok and frame and permuted
        res["raytrace"][name] = {
            "stack_size": S, "ordered": rate(o), "shuffled": rate(s), "render_aa1": r,
            "ordered_over_render": round(o["ms_median"] / r["ms_median"], 3),
            "shuffled_over_render": round(s["ms_median"] / r["ms_median"], 3),
            "shuffled_over_ordered": round(s["ms_median"] / o["ms_median"], 3),
            "ordered_colours_equal_render": frame,
            "shuffled_colours_are_ordered_permuted": permuted}
    del col2
    res["order"], order_ok = order_rows(args, n, rays, shuffled, stream)
    for path in args.order_alt_json:
        with open(path) as f:
            other = json.load(f)["order"]
        res["order"].setdefault("alternatives", {})[other["label"]] = other
    del shuffled
    res["camera"], cam_ok = camera_rows(args, W, H, rays, col, fb, stream)
    del col, fb
    res["ao"], ao_ok = ao_rows(args, W, H, rays, stream)
    res["matte"], matte_ok = matte_rows(args, W, H, rays, stream)
    res["contains"] = contains_rows(args, W, H, rays, stream)
    del rays
    res["gather"], gather_ok = gather_rows(args, stream)
    res["views"], views_ok = views_rows(args, stream)
    res["fold"], fold_ok = fold_rows(args, stream)
    ok = ok and cam_ok and order_ok and ao_ok and matte_ok and gather_ok and views_ok and fold_ok
    if args.mapping_json:
        with open(args.mapping_json) as f:
            other = json.load(f)["camera"]
        for name in ("c3", "c5"):
            res["camera"][name]["mapping_" + other["mapping"]] = {
                k: other[name][k]["ms_median"] for k in ("camera_aa1", "camera_aa3", "orbit_aa3")}
    if args.parent_json:
        with open(args.parent_json) as f:
            res["parent_commit"] = json.load(f)
    finish(args, res, same and res["c5_shuffled_hits_are_ordered_permuted"] and ok)


if __name__ == "__main__":
    main()
