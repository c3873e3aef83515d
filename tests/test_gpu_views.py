"""GPU tests of many posed views in one launch (rtg_render_views_device and the
one-shot form; csrc/rtg_camera.hip and the per-S views kernels) on an MI355X:
a table of poses in device memory, one workgroup per 8 x 8 tile of one view,
against the host's plain loops (rtg_render_views_host with walk = 0, pinned view
by view to rtg_render_camera_host in test_views_host.py), bit for bit: over
the kernel's paths (no sphere, the flat loop, the 64-sphere query, the BVH),
ragged tiles next to another view's frame, more views than a wave has lanes,
every stack size and both semantics, hostile scenes, poses written on the
device, and mixed with other calls on one context.  Frames are small; every
destination is pre-filled and PAD pixels longer, and the tail must stay.
"""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import hostile
import raygen
from conftest import PKG, ROOT, bits_equal, first_mismatch
from test_camera_host import STACK_AA, STACK_POSE, cam12, pose, restate_look_at, stack_frame
from test_raytrace_host import (STACK_H, STACK_SCENES, STACK_SIZES, STACK_W, THREADS, mixed_rays,
                                scene_with_lights)
from test_views_host import VAA, VH, VS, VW, VZOOM, batch_poses, shared_zoom_pose, view_frames

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0x5A5A5A5A
PAD = 64  # pixels behind every destination that must stay as they were
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], F)


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


def _views(torch, ctx, cams, W, H, zoom, aa, S, stream=None):
    """The context path: (n, H, W, 3) frames of the poses `cams` ((n, 12)
    float32 on the host, uploaded here, or a device tensor)."""
    d_cams = cams if torch.is_tensor(cams) else torch.from_numpy(
        np.ascontiguousarray(cams, F).reshape(-1, 12)).cuda()
    n = d_cams.shape[0]
    dst = torch.full(((n * W * H + PAD) * 3,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.render_views(d_cams.data_ptr(), n, W, H, dst.data_ptr(), zoom, aa, S,
                     stream=(stream or torch.cuda.current_stream()).cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n * W * H * 3:] == FILL).all(), "pixels past the last view were written"
    return out[:n * W * H * 3].view(F).reshape(n, H, W, 3)


def _same(got, want, what=None):
    assert got.shape == want.shape
    for v in range(len(want)):  # NaN words canonical: bytes
        assert got[v].tobytes() == want[v].tobytes(), (what, "view", v,
                                                       first_mismatch(got[v], want[v]))


def _host(R, sph, lg, cams, W, H, zoom, aa, S, sem=0):
    return R.render_views_host(sph, lg, cams, W, H, zoom, aa, S, semantics=sem, walk=0,
                               threads=THREADS)


# ---- mixed views across the kernel's scene paths ----

def mixed_table(scene):
    """The poses of POSES at the shared zoom (without in_clearest where there is
    no sphere), a NaN basis in the middle, the identity pose at the end."""
    sph = scene_with_lights(scene)[0]
    names = ["orbit", "inside", "far"] + (["in_clearest"] if len(sph) else []) + ["raw"]
    cams = [shared_zoom_pose(p, scene).reshape(12) for p in names]
    nan = restate_look_at((1, 2, 3), (1, 2, 3)).reshape(12)  # eye == target
    assert np.isnan(nan).any()
    k = len(cams) // 2
    return np.stack(cams[:k] + [nan] + cams[k:] + [IDENTITY]), k


@pytest.mark.parametrize("W,H,aa,S,sem", [(9, 9, 2.5, 6, 0), (65, 9, 1.0, 16, 1)])
@pytest.mark.parametrize("scene", [0, 12, 40, "c5"])
def test_mixed_views(R, torch_cuda, scene, W, H, aa, S, sem):
    sph, lg = scene_with_lights(scene)
    cams, k = mixed_table(scene)
    want = _host(R, sph, lg, cams, W, H, VZOOM, aa, S, sem)
    ctx = R.Context(0)
    try:
        ctx.set_semantics(sem)
        ctx.set_scene(sph, lg)
        assert (ctx.scene_stats()["bvh_nodes"] > 0) == (scene == "c5")
        got = _views(torch_cuda, ctx, cams, W, H, VZOOM, aa, S)
    finally:
        ctx.close()
    _same(got, want, scene)
    # the NaN view's neighbours are their own frames, each from its own call
    for v in (k - 1, k + 1):
        own = R.render_camera_host(sph, lg, cams[v], W, H, VZOOM, aa, S, semantics=sem, walk=0,
                                   threads=THREADS)
        assert got[v].tobytes() == own.tobytes(), (scene, v)
    if len(sph):
        assert (np.nan_to_num(want) != 0).any(), "black frames"
        assert len({want[v].tobytes() for v in range(len(want))}) >= len(want) - 1


# ---- many tiny views, whole tiles, one tile ----

def ring_poses(scene, n):
    """n poses on a tilted ring round the scene, all looking at its centre."""
    import rtg_amd as Rm
    sph = scene_with_lights(scene)[0]
    lo, hi = raygen.bounds(sph)
    c, s = (lo + hi) * 0.5, float((hi - lo).max())
    a = 2 * np.pi * np.arange(n) / n
    eyes = c + 0.9 * s * np.stack([np.cos(a), 0.3 * np.sin(3 * a), np.sin(a)], 1)
    return np.stack([cam12(Rm.camera_look_at(e, c)).reshape(12) for e in eyes])


def aim_poses(scene, n):
    """n poses for 1 x 1 frames, whose one pixel is the frame's corner: right
    and up are zero vectors (the basis is used as given), so every sample's
    ray is vnorm(zoom * back), from the ring straight at the centre of a
    sphere of the pose's own."""
    sph = scene_with_lights(scene)[0]
    cams = ring_poses(scene, n).reshape(n, 4, 3)
    for v in range(n):
        d = cams[v, 0].astype(np.float64) - sph["pos"][(v * 13) % len(sph)]
        cams[v, 1:3] = 0
        cams[v, 3] = d / np.linalg.norm(d)
    return cams.reshape(n, 12)


@pytest.mark.parametrize("n,W,H", [(70, 1, 1), (3, 8, 8), (3, 16, 8), (3, 7, 5)])
def test_tiny_views(R, torch_cuda, n, W, H):
    """70 views of 1 x 1: more views than a wave has lanes, one live lane per
    wave; 8 x 8 and 16 x 8: no ragged tile; 7 x 5: inside one tile."""
    sph, lg = scene_with_lights("c5")
    cams = aim_poses("c5", n) if W == 1 else ring_poses("c5", n)
    zoom = -6.0
    want = _host(R, sph, lg, cams, W, H, zoom, 2.0, 8)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        got = _views(torch_cuda, ctx, cams, W, H, zoom, 2.0, 8)
    finally:
        ctx.close()
    _same(got, want, (n, W, H))
    # lit, and not one frame n times (every view is compared with its own
    # frame; the three-view cases, 35 to 128 pixels a view, are all distinct)
    distinct = len({want[v].tobytes() for v in range(n)})
    assert (want != 0).any() and (distinct == n if n == 3 else distinct > 1)


# ---- every stack size ----

@functools.lru_cache(maxsize=None)
def _second_stack_frame(scene, S, sem):
    import rtg_amd as Rm
    sph, lg = scene_with_lights(scene)
    cam, zoom = pose("inside", scene)
    assert zoom == pose(STACK_POSE, scene)[1]
    return Rm.render_camera_host(sph, lg, cam, STACK_W, STACK_H, zoom, STACK_AA, S, semantics=sem,
                                 walk=0, threads=THREADS)


@pytest.mark.parametrize("scene", STACK_SCENES)
def test_every_stack_size(R, torch_cuda, scene):
    """test_camera_host.stack_frame's 9 x 9 frame and a second pose as one
    batch at every S (CPU semantics) and at S = 2 and 16 with the OpenCL
    kernel's: the views kernel of each S comes from the same table as the
    camera kernel's.  The host's frames tell neighbouring sizes apart
    (STACK_FRAMES_TOLD_APART there)."""
    sph, lg = scene_with_lights(scene)
    cam0, zoom = pose(STACK_POSE, scene)
    cams = np.stack([cam0.reshape(12), pose("inside", scene)[0].reshape(12)])
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        for sem, sizes in ((0, STACK_SIZES), (1, (2, 16))):
            ctx.set_semantics(sem)
            for S in sizes:
                got = _views(torch_cuda, ctx, cams, STACK_W, STACK_H, zoom, STACK_AA, S)
                want = np.stack([stack_frame(scene, S, sem), _second_stack_frame(scene, S, sem)])
                _same(got, want, (sem, S))
    finally:
        ctx.close()


# ---- duplicates, and device against device ----

def test_duplicates_and_the_single_view_kernel(R, torch_cuda):
    torch = torch_cuda
    sph, lg = scene_with_lights("c5")
    five = batch_poses("c5")
    cams = np.stack([five[0], five[3], five[0], five[1], five[3]])
    W, H, aa, S = 17, 9, 2.0, 8
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        got = _views(torch, ctx, cams, W, H, VZOOM, aa, S)
        assert got[0].tobytes() == got[2].tobytes() and got[1].tobytes() == got[4].tobytes()
        assert got[0].tobytes() != got[1].tobytes()
        for v in range(5):
            one = torch.full(((W * H + PAD) * 3,), FILL, dtype=torch.int32, device="cuda")
            ctx.render_camera(cams[v], W, H, one.data_ptr(), VZOOM, aa, S,
                              stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert one.cpu().numpy()[:W * H * 3].tobytes() == got[v].tobytes(), v
    finally:
        ctx.close()
    _same(got, _host(R, sph, lg, cams, W, H, VZOOM, aa, S))


# ---- hostile scenes ----

def _hostile_poses(R, base_sph):
    lo, hi = raygen.bounds(base_sph)
    c = (lo + hi) * 0.5
    return np.stack([cam12(R.camera_look_at(*hostile.POSE)).reshape(12),
                     cam12(R.camera_look_at(c, c + np.array([1.0, -0.2, -0.5]))).reshape(12)])


@pytest.mark.parametrize("n", [8, 65, hostile.LARGE_N])
def test_hostile_scenes(R, torch_cuda, n):
    """hostile.all_ at a masked size and the first BVH size, and the large
    scene with a NaN centre: the pose of test_gpu_hostile.py and one from the
    middle of the base scene, as a two-view batch."""
    if n == hostile.LARGE_N:
        base_sph, sph, lg = hostile.large()
        W, H, S, aa = 24, 14, 4, 2.0
    else:
        sph, lg = hostile.mutated(n, "all")
        base_sph = hostile.mutated(n, "base")[0]
        W, H, S, aa = 32, 24, 6, 2.0
    cams = _hostile_poses(R, base_sph)
    want = _host(R, sph, lg, cams, W, H, -4.0, aa, S)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        got = _views(torch_cuda, ctx, cams, W, H, -4.0, aa, S)
    finally:
        ctx.close()
    _same(got, want, n)
    assert (got.view(np.uint32)[np.isnan(got)] == 0xFFC00000).all()
    assert (want != 0).any()


# ---- poses written on the device ----

def test_poses_written_on_the_device(R, torch_cuda):
    """A probe per primary hit: eyes from intersect_device's hit points plus a
    normal offset, by a torch op on the GPU, under the six bases of camera_cube;
    the table never visits the host before the launch.  The frames equal the
    same table passed through the one-shot form, and the host's."""
    torch = torch_cuda
    sph, lg = scene_with_lights("c5")
    cam, zoom = pose("orbit", "c5")
    rays = R.camera_rays_host(cam, 3, 2, zoom, 1.0)
    bases = R.camera_cube((0, 0, 0)).view(F).reshape(6, 12)[:, 3:]
    W = H = 8
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        q = torch.cuda.current_stream().cuda_stream
        d_rays = torch.from_numpy(rays).cuda()
        hits = torch.zeros((len(rays), 8), dtype=torch.float32, device="cuda")
        ctx.intersect_device(d_rays.data_ptr(), len(rays), hits.data_ptr(), stream=q)
        eyes = hits[:, 2:5] + 0.05 * hits[:, 5:8]
        table = torch.cat([eyes[:, None, :].expand(-1, 6, -1),
                           torch.from_numpy(bases).cuda()[None].expand(len(rays), -1, -1)],
                          dim=2).reshape(-1, 12).contiguous()
        got = _views(torch, ctx, table, W, H, -1.0, 1.0, 8)
    finally:
        ctx.close()
    cams = table.cpu().numpy()
    assert cams.shape == (36, 12) and (hits[:, 0].cpu().numpy().view(np.int32) >= 0).any()
    one_shot = R.render_views(sph, lg, cams, W, H, -1.0, 1.0, 8)
    _same(got, one_shot, "one-shot")
    _same(got, _host(R, sph, lg, cams, W, H, -1.0, 1.0, 8), "host")
    assert (np.nan_to_num(got) != 0).any()


# ---- no views, a stream, other calls on the context ----

def test_no_views_streams_and_other_calls(R, torch_cuda):
    torch = torch_cuda
    sph, lg = scene_with_lights("c5")
    cams = batch_poses("c5")
    want = view_frames("c5", 0, VW, VH, VAA, 8)
    W, H, S, aa = 40, 30, 8, 2.0
    rays = mixed_rays(sph, lg, 2000, 5)
    want_fb = R.render(sph, lg, W, H, -4.0, aa, S)
    want_col = R.raytrace_host(sph, lg, rays, stack_size=S, threads=THREADS)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        # no views: nothing launched, the pattern stays; the table may be null
        dst = torch.full((PAD * 3,), FILL, dtype=torch.int32, device="cuda")
        d_cams = torch.from_numpy(cams).cuda()
        for table in (d_cams.data_ptr(), 0):
            ctx.render_views(table, 0, VW, VH, dst.data_ptr(), VZOOM, VAA, 8)
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == FILL).all()
        # a stream of the caller's
        _same(_views(torch, ctx, cams, VW, VH, VZOOM, VAA, 8, stream=torch.cuda.Stream()), want)
        # between a render and a batch of rays on one context and stream
        s = torch.cuda.Stream()
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        col = torch.zeros((len(rays), 3), dtype=torch.float32, device="cuda")
        vw = [torch.full(((5 * VW * VH + PAD) * 3,), FILL, dtype=torch.int32, device="cuda")
              for _ in (0, 1)]
        d_rays = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        q = s.cuda_stream
        ctx.render_views(d_cams.data_ptr(), 5, VW, VH, vw[0].data_ptr(), VZOOM, VAA, 8, stream=q)
        ctx.render_device(W, H, fb.data_ptr(), alias_factor=aa, stack_size=S, stream=q)
        ctx.render_views(d_cams.data_ptr(), 5, VW, VH, vw[1].data_ptr(), VZOOM, VAA, 8, stream=q)
        ctx.raytrace_device(d_rays.data_ptr(), len(rays), col.data_ptr(), stack_size=S, stream=q)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert bits_equal(fb.cpu().numpy(), want_fb)
    assert col.cpu().numpy().tobytes() == want_col.tobytes()
    for k in (0, 1):
        out = vw[k].cpu().numpy()
        assert (out[5 * VW * VH * 3:] == FILL).all()
        assert out[:5 * VW * VH * 3].tobytes() == want.tobytes(), k


# ---- entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    ctx = R.Context(0)
    try:
        fb = torch.zeros((2, 8, 8, 3), dtype=torch.float32, device="cuda")
        cams = torch.from_numpy(np.stack([IDENTITY, IDENTITY, IDENTITY])).cuda()
        p, d = cams.data_ptr(), fb.data_ptr()
        with pytest.raises(R.RtgError, match="scene"):  # no scene yet
            ctx.render_views(p, 2, 8, 8, d)
        ctx.set_scene(sph, lg)
        for a, kw, msg in (((0, 2, 8, 8, d), {}, "null pose table"),
                           ((p, 2, 8, 8, 0), {}, "null destination"),
                           ((p + 2, 2, 8, 8, d), {}, "4-byte aligned"),
                           ((p, 2, 0, 8, d), {}, "empty frame"),
                           ((p, 2, 8, 0, d), {}, "empty frame"),
                           ((p, 2, 8, 8, d), {"alias_factor": 257.0}, "aliasFactor"),
                           ((p, 2, 8, 8, d), {"alias_factor": float("nan")}, "aliasFactor"),
                           ((p, 2, 8, 8, d), {"stack_size": 0}, "stackSize 0"),
                           ((p, 2, 8, 8, d), {"stack_size": 17}, "stackSize 17"),
                           ((p, 0, 8, 8, d), {"stack_size": 17}, "stackSize 17"),
                           ((p, 1 << 20, 4096, 4096, d), {}, "2\\^31-1 workgroups"),
                           ((p, 1 << 31, 1, 1, d), {}, "2\\^31-1 workgroups")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.render_views(*a, **kw)
        # 4-byte aligned is aligned enough: a table one float into an allocation
        off = torch.from_numpy(np.concatenate([[7.0], IDENTITY, IDENTITY]).astype(F)).cuda()
        ctx.render_views(off.data_ptr() + 4, 2, 8, 8, d, -4.0, 1.0, 6)
        torch.cuda.synchronize()
        want = R.render_camera_host(sph, lg, IDENTITY, 8, 8, -4.0, 1.0, 6)
        got = fb.cpu().numpy()
        assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == want.tobytes()
        with pytest.raises(R.RtgError, match="stackSize 0"):  # the one-shot form's own check
            R.render_views(sph, lg, IDENTITY.reshape(1, 12), 4, 4, stack_size=0)
    finally:
        ctx.close()


# ---- the driver ----

def test_host_driver_views_and_cube(R, tmp_path):
    sph, lg = R.reference_scene()
    W, H = 40, 30
    scene = ["--scene", os.path.join(ROOT, "scenes", "reference.scene")]
    base = [os.path.join(PKG, "rtg_main")] + scene + ["--width", str(W), "--height", str(H),
                                                       "--aa", "2"]
    specs = ["3,2,-1,0,0,-10", "3,2,-1,0,0,-10,0.2,1,0", "-2,0.5,1,0,0,-10"]
    listing = tmp_path / "views.txt"
    listing.write_text("\n".join(specs[:2]) + "\n\n" + specs[2] + "\n")
    r = subprocess.run(base + ["--out", str(tmp_path / "v.ppm"), "--views", str(listing)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for k, spec in enumerate(specs):
        single = str(tmp_path / "single.ppm")
        r = subprocess.run(base + ["--out", single, "--camera", spec], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = open(tmp_path / f"v.{k}.ppm", "rb").read()
        assert got == open(single, "rb").read(), k
        assert len(set(got[-W * H * 3:])) > 2, "a flat image"
    assert not os.path.exists(tmp_path / "v.3.ppm")
    # the cube: six square faces at zoom -1
    exe = [os.path.join(PKG, "rtg_main")] + scene
    r = subprocess.run(exe + ["--out", str(tmp_path / "c.ppm"), "--cube", "0,0,-4", "--width", "16",
                              "--aa", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = R.render_views(sph, lg, R.camera_cube((0, 0, -4)), 16, 16, -1.0, 1.0, 6)
    for k in range(6):
        assert open(tmp_path / f"c.{k}.ppm", "rb").read() == R.ppm_file_bytes(want[k]), k
    for bad, msg in ((["--cube", "0,0,0", "--zoom", "-4"], "square frames at --zoom -1"),
                     (["--cube", "0,0,0", "--width", "16", "--height", "8"], "square frames"),
                     (["--cube", "0,0"], "Invalid cube"),
                     (["--cube", "0,0,0", "--views", str(listing)], "renders alone"),
                     (["--views", str(listing), "--camera", specs[0]], "renders alone")):
        r = subprocess.run(exe + bad, capture_output=True, text=True, timeout=120)  # no GPU call
        assert r.returncode == 1 and msg in r.stdout, (bad, r.stdout)
