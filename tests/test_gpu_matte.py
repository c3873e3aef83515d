"""GPU tests of direct light and containment (rtg_matte*, rtg_contains*,
include/rtg.h) on an MI355X, against the references test_matte_host.py pins on
the CPU (mattegen.py: the plain loops' sums, masks and indices), bit for bit
with NaN canonicalised.

Every destination is pre-filled and PAD records longer than its result; the
tail must stay.

  1. matte_device with and without the mask == matte_host(walk 0), and
     contains_device == contains_host(walk 0), for 1, 63, 64, 65 and 200
     points, every light set, on every scene of the CPU walk-1 list, one
     context per scene;
  2. every hostile scene (hostile.CASES), one context per size taking the
     mutations in turn;
  3. the white-scene frame: render_camera at aa 1 ==
     matte_device(intersect_device(camera_rays)), which ties the new kernel to
     the render kernels and not only to its own host form;
  4. the one-shot forms, a launch on a stream of its own and on the default one;
  5. rtg_main --matte;
  6. the device entry points' argument checks.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import aogen
import hostile
import mattegen as G
from conftest import PKG, ROOT
from hostile import CASES, IDS
from mattegen import LIGHT_SETS, SCENES, SIZES
from test_gpu_order import PAD, _stream
from test_raytrace_host import THREADS

pytestmark = pytest.mark.gpu

FILL32 = 0x5A5A5A5A
FILL64 = 0x5A5A5A5A5A5A5A5A


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


def _dev(torch, a):
    """A host array on the device as int32 words."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).cuda()


def _matte(torch, ctx, d_hits, n, mask=True, stream=None):
    """(sums, masks) of the first n records; masks None without a mask buffer."""
    dst = torch.full(((n + PAD) * 3,), FILL32, dtype=torch.int32, device="cuda")
    lit = torch.full((n + PAD,), FILL64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    ctx.matte_device(d_hits.data_ptr(), n, dst.data_ptr(), lit.data_ptr() if mask else 0,
                     stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint32)
    bits = lit.cpu().numpy().view(np.uint64)
    assert (out[3 * n:] == FILL32).all(), "sums past the batch were written"
    assert (bits[n:] == FILL64).all(), "masks past the batch were written"
    if not mask:
        assert (bits == FILL64).all(), "masks were written without a mask buffer"
    return out[:3 * n].view(np.float32).reshape(n, 3), (bits[:n] if mask else None)


def _contains(torch, ctx, d_pts, n, stream=None):
    dst = torch.full((n + PAD,), FILL32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.contains_device(d_pts.data_ptr(), n, dst.data_ptr(),
                        stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n:].view(np.uint32) == FILL32).all(), "indices past the batch were written"
    return out[:n]


# ---- 1. every path, size and light set ----

@pytest.mark.parametrize("name", SCENES)
def test_device_equals_plain_loops(R, torch_cuda, name):
    torch = torch_cuda
    sph = G.scene(name)
    d_hits = _dev(torch, G.hits(name))
    d_pts = _dev(torch, G.points(name))
    want_in = G.want_contains(name)
    ctx = R.Context(0)
    try:
        for kind in LIGHT_SETS:
            ctx.set_scene(sph, G.lights(name, kind))
            nodes = ctx.scene_stats()["bvh_nodes"]
            assert (nodes > 0) == (aogen.PATHS[name] == "bvh"), nodes
            want, want_lit = G.want(name, kind)
            for n in SIZES:
                got, lit = _matte(torch, ctx, d_hits, n)
                assert G.same_words(got, want[:n]) is None, (kind, n, G.same_words(got, want[:n]))
                assert G.same_masks(lit, want_lit[:n]) is None, (kind, n,
                                                                 G.same_masks(lit, want_lit[:n]))
                got, _ = _matte(torch, ctx, d_hits, n, mask=False)
                assert G.same_words(got, want[:n]) is None, (kind, n, "no mask")
        for n in SIZES:
            got = _contains(torch, ctx, d_pts, n)
            assert got.tobytes() == want_in[:n].tobytes(), (n, np.flatnonzero(got != want_in[:n])[:4])
    finally:
        ctx.close()


# ---- 2. hostile scenes ----

@pytest.fixture(scope="module")
def contexts(R):
    """One context per base size, made on first use and kept for the module."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = R.Context(0)
        return made[n]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.mark.parametrize("n,name", CASES, ids=IDS)
def test_hostile_scene(R, torch_cuda, contexts, n, name):
    torch = torch_cuda
    sph, lg = hostile.mutated(n, name)
    h = aogen.hostile_hits(n, name)
    assert (h["id"] >= 0).any() and (h["id"] < 0).any()
    ctx = contexts(n)
    ctx.set_scene(sph, lg)
    if n > 64:  # which query path the kernel takes (hostile.expect)
        nodes = ctx.scene_stats()["bvh_nodes"]
        assert (nodes == 0) == (hostile.expect(n, name)[1] == "flat"), nodes
    want, want_lit = R.matte_host(sph, lg, h, walk=0, threads=THREADS, mask=True)
    got, lit = _matte(torch, ctx, _dev(torch, h), len(h))
    assert G.same_words(got, want) is None, G.same_words(got, want)
    assert G.same_masks(lit, want_lit) is None, G.same_masks(lit, want_lit)
    pts = G.hostile_points(n)
    want_in = R.contains_host(sph, pts, walk=0, threads=THREADS)
    got_in = _contains(torch, ctx, _dev(torch, pts), len(pts))
    assert got_in.tobytes() == want_in.tobytes(), np.flatnonzero(got_in != want_in)[:4]


# ---- 3. the white-scene frame against the render kernels ----

@pytest.mark.parametrize("name", ["reference", 40, "base150"])
def test_white_scene_frame_equals_render_camera(R, torch_cuda, name):
    torch = torch_cuda
    white, lg = G.whitened(G.scene(name)), G.lights(name)
    W, H = 48, 36
    n = W * H
    ctx = R.Context(0)
    try:
        ctx.set_scene(white, lg)
        for cam in (R.camera_identity(), R.camera_look_at(*hostile.POSE)):
            frame = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
            hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
            ctx.render_camera(cam, W, H, frame.data_ptr(), alias_factor=1.0, stack_size=6,
                              stream=_stream(torch))
            ctx.camera_rays(cam, W, H, rays.data_ptr(), alias_factor=1.0, stream=_stream(torch))
            ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream=_stream(torch))
            got, _ = _matte(torch, ctx, hits, n, mask=False)
            want = frame.cpu().numpy()
            assert G.same_words(got, want) is None, G.same_words(got, want)
            assert (G.canon(want) << 1).any()  # not a black frame
    finally:
        ctx.close()


# ---- 4. the one-shot forms and the streams ----

def test_one_shot_and_streams(R, torch_cuda):
    torch = torch_cuda
    for name, kind in (("reference", "own"), ("base150", "m70")):
        sph, lg, h, pts = G.scene(name), G.lights(name, kind), G.hits(name), G.points(name)
        want, want_lit = G.want(name, kind)
        got, lit = R.matte(sph, lg, h, mask=True)
        assert G.same_words(got, want) is None and G.same_masks(lit, want_lit) is None, name
        assert G.same_words(R.matte(sph, lg, h), want) is None, name
        assert R.contains(sph, pts).tobytes() == G.want_contains(name).tobytes(), name
        d_hits, d_pts = _dev(torch, h), _dev(torch, pts)
        ctx = R.Context(0)
        try:
            ctx.set_scene(sph, lg)
            own = torch.cuda.Stream()
            for stream in (own.cuda_stream, 0):
                got, lit = _matte(torch, ctx, d_hits, len(h), stream=stream)
                assert G.same_words(got, want) is None and G.same_masks(lit, want_lit) is None
                got = _contains(torch, ctx, d_pts, len(pts), stream=stream)
                assert got.tobytes() == G.want_contains(name).tobytes()
        finally:
            ctx.close()
    assert R.matte(sph, lg, np.zeros(0, R.HIT_DTYPE)).shape == (0, 3)
    assert R.contains(sph, np.zeros((0, 3), np.float32)).shape == (0,)


# ---- 5. the driver ----

def _chain(R, torch, sph, lg, cam, W, H):
    """camera_rays -> intersect_device -> matte_device -> max_colour_device ->
    ppm_bytes_device through the binding: the file's bytes."""
    n = W * H
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        s = _stream(torch)
        rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        light = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        mx = torch.zeros(1, dtype=torch.float32, device="cuda")
        out = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
        ctx.camera_rays(cam, W, H, rays.data_ptr(), alias_factor=1.0, stream=s)
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream=s)
        ctx.matte_device(hits.data_ptr(), n, light.data_ptr(), stream=s)
        ctx.max_colour_device(light.data_ptr(), n, mx.data_ptr(), stream=s)
        ctx.ppm_bytes_device(light.data_ptr(), n, mx.data_ptr(), out.data_ptr(), stream=s)
        torch.cuda.synchronize()
        return b"P6\n%d %d\n255\n" % (W, H) + out.cpu().numpy().tobytes()
    finally:
        ctx.close()


def test_host_driver_matte_option(R, torch_cuda, tmp_path):
    torch = torch_cuda
    scene_file = os.path.join(ROOT, "scenes", "reference.scene")
    sph, lg = R.load_scene_file(scene_file)
    W, H = 48, 36
    frame = str(tmp_path / "frame.ppm")
    base = [os.path.join(PKG, "rtg_main"), "--scene", scene_file, "--width", str(W), "--height",
            str(H), "--out", frame]
    for extra, cam in (([], R.camera_identity()),
                       (["--camera", "3,2,-1,0,0,-10"], R.camera_look_at((3, 2, -1), (0, 0, -10)))):
        ppm = str(tmp_path / "matte.ppm")
        r = subprocess.run(base + ["--matte", ppm] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = _chain(R, torch, sph, lg, cam, W, H)
        body = np.frombuffer(want[-W * H * 3:], np.uint8)
        assert 0 < int((body > 0).sum()) < body.size  # lit and unlit pixels
        assert open(ppm, "rb").read() == want, extra
    for bad in (["--matte"], ["--matte", ""], ["--matte", frame]):  # usage errors: no GPU call
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("Missing value" in r.stdout or "Invalid matte" in r.stdout), \
            r.stdout
        assert "Device" not in r.stdout


# ---- 6. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    h, pts = G.hits("reference"), G.points("reference")
    d_hits, d_pts = _dev(torch, h), _dev(torch, pts)
    out = torch.zeros(((len(h) + PAD) * 3,), dtype=torch.int32, device="cuda")
    lit = torch.zeros((len(h) + PAD,), dtype=torch.int64, device="cuda")
    idx = torch.zeros((len(pts) + PAD,), dtype=torch.int32, device="cuda")
    hp, pp, op, lp, ip = (t.data_ptr() for t in (d_hits, d_pts, out, lit, idx))
    ctx = R.Context(0)
    try:
        with pytest.raises(R.RtgError, match="matte: no context/scene"):  # no scene yet
            ctx.matte_device(hp, len(h), op, lp)
        with pytest.raises(R.RtgError, match="contains: no context/scene"):
            ctx.contains_device(pp, len(pts), ip)
        ctx.set_scene(G.scene("reference"), G.lights("reference"))
        for a, msg in (((0, 8, op, lp), "matte: null hit buffer"),
                       ((hp, 8, 0, lp), "matte: null output buffer"),
                       ((hp, 1 << 32, op, lp), "at most 2\\^32 - 1")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.matte_device(*a)
        for a, msg in (((0, 8, ip), "contains: null point buffer"),
                       ((pp, 8, 0), "contains: null output buffer"),
                       ((pp, 1 << 32, ip), "at most 2\\^32 - 1")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.contains_device(*a)
        ctx.matte_device(hp, 0, op, lp)  # an empty batch: RTG_OK, no launch
        ctx.contains_device(pp, 0, ip)
        L = R.lib()
        assert L.rtg_matte_device(None, hp, 8, op, lp, None) == -1
        assert b"no context" in L.rtg_last_error()
        assert L.rtg_contains_device(None, pp, 8, ip, None) == -1
        assert b"no context" in L.rtg_last_error()
        torch.cuda.synchronize()
        assert int(out.count_nonzero()) == 0 and int(lit.count_nonzero()) == 0  # nothing launched
        assert int(idx.count_nonzero()) == 0
    finally:
        ctx.close()
