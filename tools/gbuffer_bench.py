#!/usr/bin/env python3
"""tools/gbuffer_bench.py [--configs c2,c3,c5] [--rounds N] [--out-dir DIR]

Times rtg_gbuffer_device (the primary-hit G-buffer, csrc/rtg_gbuffer.hip) on
bench.py's configurations with the scene resident, and in the same process,
interleaved round by round, rtg_render_device of the same frame.  Device
events around a few back-to-back launches on one stream, after a warm-up of
each; medians over the rounds.  Writes DIR/bench_<config>.json (default
profiles/gbuffer/) with both times, the bytes the G-buffer writes (32 per
pixel) and the resulting GB/s.

The sanity bound: on every configuration the G-buffer's median is below the
full render's (the render holds the same primary queries plus all shading
and recursion); the tool exits non-zero if it is not.  It also checks, on the
frames it timed, that every pixel without a hit is +0 in the rendered frame.
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


def timed(fn, stream, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, rounds, out_dir):
    W, H, n, m, depth = CONFIGS[name]
    sph, lg = R.generate_scene(n, m, 42)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gb = torch.empty((H * W * 8,), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()

    def render():
        ctx.render_device(W, H, fb.data_ptr(), stack_size=depth + 1, stream=s.cuda_stream)

    def gbuffer():
        ctx.gbuffer_device(W, H, gb.data_ptr(), stream=s.cuda_stream)

    for _ in range(3):  # warm-up: code objects, the render's launch-order feedback
        render()
        gbuffer()
    torch.cuda.synchronize()
    # a window of some milliseconds for each
    reps_r = max(2, min(10, int(20.0 / max(timed(render, s, 1), 1e-3))))
    reps_g = max(5, min(50, int(20.0 / max(timed(gbuffer, s, 1), 1e-3))))
    tr, tg = [], []
    for _ in range(rounds):
        tr.append(timed(render, s, reps_r))
        tg.append(timed(gbuffer, s, reps_g))
    ctx.close()

    rec = gb.view(H, W, 8)
    hits = rec[..., 2]
    black = (fb.view(torch.int32) == 0).all(dim=2)
    bad = int(((hits == 0) & ~black).sum())
    nbytes = W * H * R.GBUF_DTYPE.itemsize
    g_ms, r_ms = float(np.median(tg)), float(np.median(tr))
    res = {
        "config": name, "W": W, "H": H, "spheres": n, "alias_factor": 3.0,
        "stack_size": depth + 1, "device": R.device_info(0), "rounds": rounds,
        "gbuffer_ms_median": round(g_ms, 5), "gbuffer_ms_min": round(min(tg), 5),
        "gbuffer_ms_max": round(max(tg), 5), "gbuffer_launches_per_round": reps_g,
        "render_ms_median": round(r_ms, 5), "render_ms_min": round(min(tr), 5),
        "render_ms_max": round(max(tr), 5), "render_launches_per_round": reps_r,
        "gbuffer_bytes_written": nbytes,
        "gbuffer_GBps": round(nbytes / (g_ms * 1e-3) / 1e9, 2),
        "gbuffer_over_render": round(g_ms / r_ms, 4),
        "hit_pixels": int((hits > 0).sum()),
        "mixed_pixels": int((hits * (rec[..., 0] + 1) != rec[..., 7]).sum()),
        "missed_pixels_not_black_in_render": bad,
        "bound_gbuffer_below_render": g_ms < r_ms,
    }
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"bench_{name}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return res["bound_gbuffer_below_render"] and bad == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "gbuffer"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gbuffer_bench: needs a GPU")
    ok = True
    for name in args.configs.split(","):
        ok = run(name, args.rounds, args.out_dir) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
