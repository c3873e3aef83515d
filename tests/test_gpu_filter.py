"""GPU tests of the edge-stopping a-trous filter (rtg_filter*, include/rtg.h) on
an MI355X, against the host loops' words test_filter_host.py pins on the CPU
(filtergen.want), word for word.

Every destination and scratch is pre-filled and PAD words longer than the
call needs; the tail must stay.

  1. filter_device == filter_host on every frame, signal and parameter set of
     filtergen (passes 5 and 8 reach the steps the direct form takes);
  2. both pass-kernel forms, forced by RTG_FILTER_FORM, on the 67 x 35 frame;
  3. the one-shot form;
  4. a launch on a stream of its own between two renders of the context;
  5. intersect_device's records and ao_device's counts straight into the
     filter, against the host chain;
  6. rtg_main --ao-filter and --gather-filter, and rtg_main without them;
  7. the device entry point's argument checks.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import aogen
import filtergen as G
from conftest import PKG, ROOT
from filtergen import ALL, FRAMES, FULL, SCENES, SETS, SIGNALS
from test_gpu_order import PAD, _stream
from test_raytrace_host import THREADS, scene_with_lights

pytestmark = pytest.mark.gpu

F = np.float32
FILL32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def R(rtg):
    if rtg.device_count() < 1:
        pytest.fail("no GPU visible to librtg")
    return rtg


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)  # no scene: the filter needs none
    yield c
    c.close()


def _dev(torch, a):
    """A host array on the device as bytes, 16-byte aligned."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _filter(torch, R, ctx, d_hits, W, H, p, d_src, stream=None):
    """Context.filter_device into a pre-filled destination and scratch, PAD
    words longer each: the result's words."""
    words = W * H * (3 if int(p["kind"][0]) == R.FILTER_RGB else 1)
    nbytes = R.filter_scratch(W, H, p)
    assert nbytes % 16 == 0 and (nbytes >= words * 4 if int(p["passes"][0]) > 1 else nbytes == 0)
    dst = torch.full((words + PAD,), FILL32, dtype=torch.int32, device="cuda")
    scratch = torch.full((nbytes // 4 + PAD,), FILL32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    ctx.filter_device(d_hits.data_ptr(), W, H, p, d_src.data_ptr(), dst.data_ptr(),
                      scratch.data_ptr() if nbytes else 0, nbytes,
                      stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint32)
    assert (out[words:] == FILL32).all(), "words past the frame were written"
    assert (scratch.cpu().numpy().view(np.uint32)[nbytes // 4:] == FILL32).all(), \
        "words past the scratch were written"
    return out[:words]


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else \
        f"{len(bad)} differ, first at {bad[0]}: {got[bad[0]]:#x} vs {want[bad[0]]:#x}"


# ---- 1. every frame, signal and parameter set ----

@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_host(R, torch_cuda, ctx, name, kind):
    torch = torch_cuda
    for W, H in FRAMES:
        d_hits = _dev(torch, G.guides(name, W, H))
        d_src = _dev(torch, G.signal(name, W, H, kind))
        for st in SETS:
            got = _filter(torch, R, ctx, d_hits, W, H, G.params(R, name, kind, st), d_src)
            want = G.want(name, W, H, kind, st)
            assert got.tobytes() == want.tobytes(), (W, H, st, _first_bad(got, want))


# ---- 2. both forms of the pass kernel ----

@pytest.mark.parametrize("form", ["tiled", "direct"])
def test_forced_form_equals_host(R, torch_cuda, ctx, form, monkeypatch):
    """RTG_FILTER_FORM is read by every call: `tiled` stages steps 1 to 8 in LDS
    (step 8 needs more than 64 KiB of it), `direct` reads every tap from memory."""
    torch = torch_cuda
    monkeypatch.setenv("RTG_FILTER_FORM", form)
    W, H = FULL
    for name in SCENES:
        d_hits = _dev(torch, G.guides(name, W, H))
        for kind in SIGNALS:
            d_src = _dev(torch, G.signal(name, W, H, kind))
            for st in SETS:
                got = _filter(torch, R, ctx, d_hits, W, H, G.params(R, name, kind, st), d_src)
                want = G.want(name, W, H, kind, st)
                assert got.tobytes() == want.tobytes(), (name, kind, st, _first_bad(got, want))


# ---- 3. the one-shot form ----

def test_one_shot(R, torch_cuda):
    for name, (W, H), kind, st in (("reference", FULL, "count", SETS[2]), ("c5", FULL, "rgb", SETS[3]),
                                   (12, (33, 17), "gray", SETS[4]), (12, (1, 1), "rgb", SETS[1])):
        got = R.filter(G.guides(name, W, H), W, H, G.params(R, name, kind, st),
                       G.signal(name, W, H, kind))
        assert got.shape == ((H, W, 3) if kind == "rgb" else (H, W))
        want = G.want(name, W, H, kind, st)
        assert got.view(np.uint32).reshape(-1).tobytes() == want.tobytes(), (name, W, H, kind, st)


# ---- 4. a stream of its own, between two renders ----

def test_own_stream_between_renders(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    W, H = FULL
    name, kind, st = "reference", "rgb", SETS[3]
    d_hits, d_src = _dev(torch, G.guides(name, W, H)), _dev(torch, G.signal(name, W, H, kind))
    c = R.Context(0)
    try:
        c.set_scene(sph, lg)
        fb = [torch.zeros((48 * 36 * 3,), dtype=torch.float32, device="cuda") for _ in range(2)]
        own = torch.cuda.Stream()
        c.render_device(48, 36, fb[0].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        got = _filter(torch, R, c, d_hits, W, H, G.params(R, name, kind, st), d_src,
                      stream=own.cuda_stream)
        c.render_device(48, 36, fb[1].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        torch.cuda.synchronize()
        assert got.tobytes() == G.want(name, W, H, kind, st).tobytes()
        a, b = fb[0].cpu().numpy(), fb[1].cpu().numpy()
        assert (a != 0).any() and G.canon(a).tobytes() == G.canon(b).tobytes()
        want = R.render(sph, lg, 48, 36, alias_factor=2.0)
        assert G.canon(a).tobytes() == G.canon(want).tobytes()
    finally:
        c.close()


# ---- 5. device-made guides and counts ----

def test_device_chain_equals_host_chain(R, torch_cuda):
    torch = torch_cuda
    W, H, K = 67, 35, 7
    name = "c5"
    sph = aogen.scene(name)
    cam = R.camera_look_at(*G.POSES[name])
    table = aogen.dirs(8)
    ap = R.ao_params(K, aogen.radius(name), aogen.BIAS, aogen.SEED, R.AO_JITTER)
    fp = R.filter_params(5, R.FILTER_COUNT, R.FILTER_SAME_ID | R.FILTER_NORMAL | R.FILTER_PLANE,
                         G.plane_scale(name, None), 3)
    rays = R.camera_rays_host(cam, W, H, alias_factor=1.0)
    h = R.intersect_host(sph, rays, walk=0, threads=THREADS)
    counts = R.ao_host(sph, h, table, ap, walk=0, threads=THREADS)
    want = R.filter_host(h, W, H, fp, counts, threads=THREADS).view(np.uint32).reshape(-1)
    assert (counts < K).any() and (want != G.canon(counts.astype(F))).any()
    n = W * H
    c = R.Context(0)
    try:
        c.set_scene(sph, scene_with_lights(name)[1])
        d_rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        d_hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_counts = torch.empty((n,), dtype=torch.int16, device="cuda")
        d_dirs = _dev(torch, table)
        s = _stream(torch)
        c.camera_rays(cam, W, H, d_rays.data_ptr(), alias_factor=1.0, stream=s)
        c.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=s)
        c.ao_device(d_hits.data_ptr(), n, ap, d_dirs.data_ptr(), 8, d_counts.data_ptr(), stream=s)
        got = _filter(torch, R, c, d_hits, W, H, fp, d_counts)
        assert got.tobytes() == want.tobytes(), _first_bad(got, want)
    finally:
        c.close()


# ---- 6. the driver ----

def _pgm_of(v, K, W, H):
    x = F(255) * v.reshape(-1).astype(F) / F(K)
    x = np.where(x > 0, np.where(x < 255, x, F(255)), F(0))
    return b"P5\n%d %d\n255\n" % (W, H) + x.astype(np.uint8).tobytes()


def test_host_driver_filter_options(R, torch_cuda, tmp_path):
    scene_file = os.path.join(ROOT, "scenes", "reference.scene")
    sph, lg = R.load_scene_file(scene_file)
    W, H, K = 48, 36, 16
    base = [os.path.join(PKG, "rtg_main"), "--scene", scene_file, "--width", str(W), "--height",
            str(H), "--out", str(tmp_path / "frame.ppm")]
    pose = ["--camera", "3,2,-1,0,0,-10"]
    cam = R.camera_look_at((3, 2, -1), (0, 0, -10))
    h = R.intersect_host(sph, R.camera_rays_host(cam, W, H, alias_factor=1.0), walk=0,
                         threads=THREADS)
    table = R.ao_directions(K)
    flags = R.FILTER_SAME_ID | R.FILTER_NORMAL | R.FILTER_PLANE

    def run(extra):
        r = subprocess.run(base + pose + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr

    # --ao with and without the filter
    counts = R.ao_host(sph, h, table, R.ao_params(K, 12.5), walk=0, threads=THREADS)
    plain, smooth = str(tmp_path / "ao.pgm"), str(tmp_path / "ao_f.pgm")
    run(["--ao", "16,12.5", "--ao-out", plain])
    assert open(plain, "rb").read() == b"P5\n%d %d\n255\n" % (W, H) + (
        (255 * counts.astype(np.uint32)) // K).astype(np.uint8).tobytes()
    for spec, (passes, scale, nlog) in (("3", (3, 1.0, 3)), ("5,0.25,4", (5, 0.25, 4))):
        run(["--ao", "16,12.5", "--ao-out", smooth, "--ao-filter", spec])
        v = R.filter_host(h, W, H, R.filter_params(passes, R.FILTER_COUNT, flags, scale, nlog), counts)
        want = _pgm_of(v, K, W, H)
        assert want != open(plain, "rb").read()
        assert open(smooth, "rb").read() == want, spec
    # --gather with and without the filter
    gp = R.gather_params(K, flags=R.GATHER_SKIP_NONFINITE)
    light = R.gather_host(sph, lg, h, table, np.full(K, F(1) / F(K), F), gp, stack_size=6,
                          walk=0, threads=THREADS)
    light = np.asarray(light if not isinstance(light, tuple) else light[0], F).reshape(W * H, 3)
    plain, smooth = str(tmp_path / "g.ppm"), str(tmp_path / "g_f.ppm")
    run(["--gather", "16", "--gather-skip", "--gather-out", plain])
    assert open(plain, "rb").read() == R.ppm_file_bytes(light.reshape(H, W, 3))
    run(["--gather", "16", "--gather-skip", "--gather-out", smooth, "--gather-filter", "4,0.5"])
    v = R.filter_host(h, W, H, R.filter_params(4, R.FILTER_RGB, flags | R.FILTER_SKIP_NONFINITE,
                                                0.5, 3), light)
    want = R.ppm_file_bytes(v)
    assert want != open(plain, "rb").read()
    assert open(smooth, "rb").read() == want
    for bad in (["--ao-filter", "3"], ["--gather-filter", "3"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-filter", "0"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-filter", "9"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-filter", "3,1,9"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-filter", "3,1,2,7"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("Invalid filter" in r.stdout or "needs --" in r.stdout), r.stdout
    r = subprocess.run(base[:1] + ["--help"], capture_output=True, text=True, timeout=120)
    assert "--ao-filter" in r.stdout and "--gather-filter" in r.stdout


# ---- 7. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda, ctx):
    torch = torch_cuda
    W, H = 33, 17
    n = W * H
    d_hits = _dev(torch, G.guides("reference", W, H))
    d_src = _dev(torch, G.signal("reference", W, H, "gray"))
    out = torch.zeros((2 * n + PAD,), dtype=torch.int32, device="cuda")
    scratch = torch.zeros((n + PAD,), dtype=torch.int32, device="cuda")
    ok = R.filter_params(3, R.FILTER_GRAY, ALL, 1.0, 3)
    need = R.filter_scratch(W, H, ok)
    assert need == (n * 4 + 15) // 16 * 16
    hp, sp, op, cp = d_hits.data_ptr(), d_src.data_ptr(), out.data_ptr(), scratch.data_ptr()
    assert hp % 16 == 0 and cp % 16 == 0
    for a, msg in (((0, W, H, ok, sp, op, cp, need), "filter: null hit buffer"),
                   ((hp, W, H, ok, 0, op, cp, need), "filter: null source"),
                   ((hp, W, H, ok, sp, 0, cp, need), "filter: null destination"),
                   ((hp, W, H, ok, sp, op, 0, need), "filter: null scratch"),
                   ((hp, 0, H, ok, sp, op, cp, need), "filter: empty frame"),
                   ((hp, W, 0, ok, sp, op, cp, need), "filter: empty frame"),
                   ((hp, 1 << 16, 1 << 16, ok, sp, op, cp, need), "at most 2\\^32 - 1"),
                   ((hp, W, H, R.filter_params(0, 1), sp, op, cp, need), "0 passes"),
                   ((hp, W, H, R.filter_params(9, 1), sp, op, cp, need), "9 passes"),
                   ((hp, W, H, R.filter_params(2, 1, normal_log2=9), sp, op, cp, need), "normalLog2 9"),
                   ((hp, W, H, R.filter_params(2, 3), sp, op, cp, need), "kind 3"),
                   ((hp, W, H, R.filter_params(2, 1, 32), sp, op, cp, need), "unknown flags 0x20"),
                   ((hp + 4, W, H, ok, sp, op, cp, need), "hit buffer not 16-byte aligned"),
                   ((hp, W, H, ok, sp, op, cp, need - 1), "filter: scratch of"),
                   ((hp, W, H, ok, sp, op, cp + 4, need), "filter: scratch of"),
                   ((hp, W, H, ok, sp, sp, cp, need), "the destination overlaps the source"),
                   ((hp, W, H, ok, sp, sp + 4 * n - 4, cp, need), "the destination overlaps the source"),
                   ((hp, W, H, ok, sp, cp, cp, need), "the destination overlaps the scratch"),
                   ((hp, W, H, ok, sp, op + 4 * n, op + (8 * n - 64) // 16 * 16, need),
                    "the destination overlaps the scratch")):
        with pytest.raises(R.RtgError, match=msg):
            ctx.filter_device(*a)
    L = R.lib()
    assert L.rtg_filter_device(ctx._h, hp, W, H, None, sp, op, cp, need, None) == -1
    assert b"filter: null params" in L.rtg_last_error()
    assert L.rtg_filter_device(None, hp, W, H, R._ptr(ok), sp, op, cp, need, None) == -1
    assert b"filter: no context" in L.rtg_last_error()
    # (the grid check cannot fire behind the pixel check: a frame of at most 2^32 - 1 pixels
    # has at most 2^29 tiles, the 1 x (2^32 - 1) one.)  The address comparison takes that
    # frame's 16 GiB ranges as numbers; nothing is dereferenced
    tall = R.filter_params(1, R.FILTER_GRAY)
    with pytest.raises(R.RtgError, match="the destination overlaps the source"):
        ctx.filter_device(hp, 1, (1 << 32) - 1, tall, sp, sp + (1 << 34) - 8, 0, 0)
    torch.cuda.synchronize()
    assert int(out.count_nonzero()) == 0 and int(scratch.count_nonzero()) == 0  # nothing launched
    # one pass needs no scratch: null is legal
    ctx.filter_device(hp, W, H, R.filter_params(1, R.FILTER_GRAY, ALL, 1.0, 3), sp, op)
    torch.cuda.synchronize()
    assert int(out[:n].count_nonzero()) > 0 and int(out[n:].count_nonzero()) == 0
