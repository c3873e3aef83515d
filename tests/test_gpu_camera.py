"""GPU tests of the posed camera (rtg_render_camera_device and the one-shot form,
rtg_camera_rays_device; csrc/rtg_camera.hip and the per-S camera kernels) on an
MI355X: the fused kernel against the host's plain loops (rtg_render_camera_host
with walk = 0, itself pinned to rtg_raytrace_host and to the reference's frames
in test_camera_host.py), bit for bit, over the kernel's paths (no sphere, the
flat loop, the 64-sphere query, the BVH), frames with edges inside a tile, on a
tile boundary and just past one, every stack-size family and both semantics.
Frames are small.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, bits_equal, first_mismatch
from test_camera_host import (ODD_BASES, PAA, PH, PS, PW, STACK_AA, STACK_POSE, pose, posed_cases,
                              posed_frame, stack_frame)
from test_raytrace_host import (STACK_H, STACK_SCENES, STACK_SIZES, STACK_W, THREADS, mixed_rays,
                                scene_with_lights)

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
PAD = 64  # records behind every destination that must stay as they were


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


def _frame(torch, ctx, cam, W, H, zoom, aa, S, stream=None):
    """The context path: the (H, W, 3) frame; the destination is pre-filled and
    PAD pixels longer, the tail must stay."""
    dst = torch.full(((W * H + PAD) * 3,), FILL, dtype=torch.int32, device="cuda")
    ctx.render_camera(cam, W, H, dst.data_ptr(), zoom, aa, S,
                      stream=(stream or torch.cuda.current_stream()).cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[W * H * 3:] == FILL).all(), "pixels past the frame were written"
    return out[:W * H * 3].view(np.float32).reshape(H, W, 3)


# ---- device == host plain loops ----
# (scene, pose, W, H, aa, S, semantics): every pose, frame, aa, S and semantics
# once against c5 (the BVH) and once against a scene without one
CASES = [
    ("c5", "orbit", 48, 36, 2.5, 6, 0),
    ("c5", "inside", 65, 9, 3.0, 16, 1),
    ("c5", "far", 9, 17, 1.0, 1, 0),
    ("c5", "in_clearest", 8, 8, 3.0, 5, 1),
    ("c5", "raw", 7, 5, 2.5, 6, 0),
    ("c5", "orbit", 1, 1, 1.0, 5, 1),
    ("reference", "orbit", 48, 36, 3.0, 6, 0),
    (12, "inside", 65, 9, 2.5, 16, 1),
    (40, "far", 9, 17, 1.0, 1, 0),
    (40, "in_clearest", 8, 8, 3.0, 5, 1),
    (12, "raw", 7, 5, 2.5, 6, 0),
    ("reference", "in_clearest", 1, 1, 1.0, 16, 0),
    (0, "orbit", 1, 1, 1.0, 5, 1),
    (0, "inside", 9, 17, 3.0, 6, 0),
]


@pytest.mark.parametrize("scene,name,W,H,aa,S,sem", CASES)
def test_device_equals_plain_loops(R, torch_cuda, scene, name, W, H, aa, S, sem):
    sph, lg = scene_with_lights(scene)
    cam, zoom = pose(name, scene)
    want = R.render_camera_host(sph, lg, cam, W, H, zoom, aa, S, semantics=sem, walk=0,
                                threads=THREADS)
    ctx = R.Context(0)
    try:
        ctx.set_semantics(sem)
        ctx.set_scene(sph, lg)
        got = _frame(torch_cuda, ctx, cam, W, H, zoom, aa, S)
    finally:
        ctx.close()
    assert got.tobytes() == want.tobytes(), first_mismatch(got, want)  # NaN words canonical
    if len(sph) and W * H >= 64:
        assert (want != 0).any(), "a black frame"


@pytest.mark.parametrize("scene", STACK_SCENES)
def test_every_stack_size(R, torch_cuda, scene):
    """The 9 x 9 posed frame of test_camera_host.stack_frame (four 8 x 8 tiles,
    three of them ragged) at every S, CPU semantics, and at S = 2 and 16 with
    the OpenCL kernel's: the kernel of each S comes from one table.  The host's
    walk 0 at that S is what tells neighbouring sizes apart
    (STACK_FRAMES_TOLD_APART there)."""
    sph, lg = scene_with_lights(scene)
    cam, zoom = pose(STACK_POSE, scene)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        for sem, sizes in ((0, STACK_SIZES), (1, (2, 16))):
            ctx.set_semantics(sem)
            for S in sizes:
                got = _frame(torch_cuda, ctx, cam, STACK_W, STACK_H, zoom, STACK_AA, S)
                want = stack_frame(scene, S, sem)
                assert got.tobytes() == want.tobytes(), (sem, S, first_mismatch(got, want))
    finally:
        ctx.close()
    assert stack_frame(scene, 2, 1).tobytes() != stack_frame(scene, 2).tobytes()


@pytest.mark.parametrize("scene", ["reference", 12, 200, "c5"])
def test_posed_frames_of_the_host_tests(R, torch_cuda, scene):
    """The 48 x 36 frames test_camera_host.py puts its conditions on (lit, not
    the identity pose's), every pose of a scene on one context."""
    sph, lg = scene_with_lights(scene)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        for name in (p for sc, p in posed_cases([scene])):
            cam, zoom = pose(name, scene)
            got = _frame(torch_cuda, ctx, cam, PW, PH, zoom, PAA, PS)
            want = posed_frame(scene, name)
            assert got.tobytes() == want.tobytes(), (name, first_mismatch(got, want))
    finally:
        ctx.close()


# ---- the identity pose == the render ----

@pytest.mark.parametrize("scene,W,H,aa,S", [("reference", 48, 36, 3.0, 6), (12, 65, 9, 2.5, 5),
                                            (200, 40, 30, 3.0, 6), ("c5", 40, 30, 2.0, 8)])
def test_identity_pose_is_the_render(R, torch_cuda, scene, W, H, aa, S):
    sph, lg = scene_with_lights(scene)
    want = R.render(sph, lg, W, H, -4.0, aa, S)
    got = R.render_camera(sph, lg, R.camera_identity(), W, H, -4.0, aa, S)  # the one-shot form
    assert bits_equal(got, want), first_mismatch(got, want)
    assert (np.nan_to_num(want) != 0).any()
    look = R.camera_look_at((0, 0, 0), (0, 0, -1))
    assert R.render_camera(sph, lg, look, W, H, -4.0, aa, S).tobytes() == got.tobytes()


# ---- the generator ----

def _rays(R, torch, ctx, cam, W, H, zoom, aa):
    n = W * H * R.camera_sample_count(aa) ** 2
    dst = torch.full(((n + PAD) * 6,), FILL, dtype=torch.int32, device="cuda")
    ctx.camera_rays(cam, W, H, dst.data_ptr(), zoom, aa,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n * 6:] == FILL).all(), "rays past the frame were written"
    return out[:n * 6].view(np.float32).reshape(n, 6)


def test_generator_equals_host(R, torch_cuda):
    ctx = R.Context(0)  # no scene: the generator needs none
    try:
        poses = [pose(name, "c5") for name in ("orbit", "inside", "far", "in_clearest", "raw")]
        poses += [(np.array(b, np.float32), -4.0) for b in ODD_BASES]
        for k, (cam, zoom) in enumerate(poses):
            W, H, aa = ((7, 5, 2.5), (65, 9, 1.0), (48, 36, 3.0), (1, 1, 2.0))[k % 4]
            got = _rays(R, torch_cuda, ctx, cam, W, H, zoom, aa)
            want = R.camera_rays_host(cam, W, H, zoom, aa)
            assert bits_equal(got, want), (k, W, H, aa, first_mismatch(got, want))
        assert _rays(R, torch_cuda, ctx, poses[0][0], 7, 5, -4.0, 0.0).shape == (0, 6)  # no launch
    finally:
        ctx.close()
    cam, zoom = poses[0]
    got = R.camera_rays(cam, 9, 17, zoom, 2.0)  # the module-level form
    assert got.tobytes() == R.camera_rays_host(cam, 9, 17, zoom, 2.0).tobytes()
    assert R.camera_rays(cam, 9, 17, zoom, 0.0).shape == (0, 6)


# ---- no interference ----

def test_one_context_two_streams(R, torch_cuda):
    """render_device, render_camera_device, gbuffer_device and raytrace_device
    interleaved on two streams of one context, a posed frame of the other
    stream between them: every result is its stand-alone result."""
    torch = torch_cuda
    sph, lg = scene_with_lights("c5")
    W, H, S, aa = 64, 48, 8, 2.0
    cam, zoom = pose("orbit", "c5")
    rays = mixed_rays(sph, lg, 3000, 5)
    want_fb = R.render(sph, lg, W, H, -4.0, aa, S)
    want_cam = R.render_camera_host(sph, lg, cam, W, H, zoom, aa, S, walk=0, threads=THREADS)
    want_gb = R.gbuffer_host(sph, W, H, -4.0, aa, threads=THREADS)
    want_col = R.raytrace_host(sph, lg, rays, stack_size=S, threads=THREADS)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        s = [torch.cuda.Stream(), torch.cuda.Stream()]
        new = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        fb = [new(H, W, 3), new(H, W, 3)]
        fc = [new(H, W, 3), new(H, W, 3)]
        fx = [new(H, W, 3), new(H, W, 3)]
        gb = [new(H * W * 8, dt=torch.int32), new(H * W * 8, dt=torch.int32)]
        col = [new(len(rays), 3), new(len(rays), 3)]
        dr = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        for k in (0, 1):
            q = s[k].cuda_stream
            ctx.render_device(W, H, fb[k].data_ptr(), alias_factor=aa, stack_size=S, stream=q)
            ctx.render_camera(cam, W, H, fc[k].data_ptr(), zoom, aa, S, stream=q)
            ctx.gbuffer_device(W, H, gb[k].data_ptr(), alias_factor=aa, stream=q)
            ctx.raytrace_device(dr.data_ptr(), len(rays), col[k].data_ptr(), stack_size=S, stream=q)
            ctx.render_camera(cam, W, H, fx[k].data_ptr(), zoom, aa, S, stream=s[1 - k].cuda_stream)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    for k in (0, 1):
        assert bits_equal(fb[k].cpu().numpy(), want_fb), k
        assert fc[k].cpu().numpy().tobytes() == want_cam.tobytes(), k
        assert fx[k].cpu().numpy().tobytes() == want_cam.tobytes(), k
        assert gb[k].cpu().numpy().tobytes() == want_gb.tobytes(), k
        assert col[k].cpu().numpy().tobytes() == want_col.tobytes(), k


# ---- the driver ----

def test_host_driver_camera_option(R, tmp_path):
    sph, lg = R.reference_scene()
    W, H = 80, 60
    base = [os.path.join(PKG, "rtg_main"), "--scene",
            os.path.join(ROOT, "scenes", "reference.scene"), "--width", str(W), "--height", str(H)]
    for spec, look in (("3,2,-1,0,0,-10", ((3, 2, -1), (0, 0, -10))),
                       ("3,2,-1,0,0,-10,0.2,1,0", ((3, 2, -1), (0, 0, -10), (0.2, 1, 0)))):
        ppm = str(tmp_path / "posed.ppm")
        r = subprocess.run(base + ["--out", ppm, "--camera", spec], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = R.render_camera(sph, lg, R.camera_look_at(*look), W, H)
        assert (np.nan_to_num(want) != 0).any()
        assert open(ppm, "rb").read() == R.ppm_file_bytes(want)
    for bad in (["--camera", "1,2,3"], ["--camera", "1,2,3,4,5,6", "--gpus", "1"]):  # no GPU call
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("Invalid camera" in r.stdout or "one device" in r.stdout)


# ---- entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    cam = R.camera_identity()
    ctx = R.Context(0)
    try:
        fb = torch.zeros((8, 8, 3), dtype=torch.float32, device="cuda")
        rays = torch.zeros((64 * 9, 6), dtype=torch.float32, device="cuda")
        with pytest.raises(R.RtgError, match="scene"):  # no scene yet
            ctx.render_camera(cam, 8, 8, fb.data_ptr())
        ctx.camera_rays(cam, 8, 8, rays.data_ptr(), alias_factor=1.0)  # needs none
        torch.cuda.synchronize()
        assert float(rays[:64, 3:].abs().sum()) > 0 and float(rays[64:].abs().sum()) == 0
        rays.zero_()
        ctx.set_scene(sph, lg)
        for a, kw, msg in (((cam, 8, 8, 0), {}, "null destination"),
                           ((cam, 0, 8, fb.data_ptr()), {}, "empty frame"),
                           ((cam, 8, 0, fb.data_ptr()), {}, "empty frame"),
                           ((cam, 8, 8, fb.data_ptr()), {"alias_factor": 257.0}, "aliasFactor"),
                           ((cam, 8, 8, fb.data_ptr()), {"alias_factor": float("nan")}, "aliasFactor"),
                           ((cam, 8, 8, fb.data_ptr()), {"stack_size": 0}, "stackSize 0"),
                           ((cam, 8, 8, fb.data_ptr()), {"stack_size": 17}, "stackSize 17"),
                           ((cam, 1 << 31, 1 << 10, fb.data_ptr()), {}, "too large")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.render_camera(*a, **kw)
        for a, kw, msg in (((cam, 8, 8, 0), {}, "null destination"),
                           ((cam, 0, 8, rays.data_ptr()), {}, "empty frame"),
                           ((cam, 8, 8, rays.data_ptr()), {"alias_factor": 300.0}, "aliasFactor"),
                           ((cam, 1 << 31, 1 << 16, rays.data_ptr()), {}, "too large")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.camera_rays(*a, **kw)
        L = R.lib()
        assert L.rtg_render_camera_device(ctx._h, None, 8, 8, -4.0, 3.0, 6, fb.data_ptr(), None) == -1
        assert b"null camera" in L.rtg_last_error()
        assert L.rtg_camera_rays_device(None, R._ptr(R._camera(cam)), 8, 8, -4.0, 3.0,
                                        rays.data_ptr(), None) == -1
        assert b"no context" in L.rtg_last_error()
        torch.cuda.synchronize()
        assert float(fb.abs().sum()) == 0 and float(rays.abs().sum()) == 0  # nothing was launched
        host = np.zeros((4, 4, 3), np.float32)
        with pytest.raises(R.RtgError, match="null camera"):  # the one-shot form's own check
            R._check(L.rtg_render_camera(0, R._ptr(sph), len(sph), R._ptr(lg), len(lg), None, 4, 4,
                                         -4.0, 3.0, 6, R._ptr(host)), "rtg_render_camera")
        with pytest.raises(R.RtgError, match="stackSize 0"):
            R.render_camera(sph, lg, cam, 4, 4, stack_size=0)
    finally:
        ctx.close()
