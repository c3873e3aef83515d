"""GPU tests of the batch ray tracer (rtg_raytrace_device and the one-shot form,
csrc/rtg_raytrace.hip and the per-S raytrace kernels) on an MI355X: the kernel
against the host's plain loops (rtg_raytrace_host with walk = 0, itself pinned
to the reference in test_raytrace_host.py), byte for byte, over the kernel's
paths: no sphere, the 64-sphere query, the BVH with origins inside and far
outside its origin box in one wave, ragged last waves, both semantics, and
the other entry points.  Batches are small.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import raygen
from conftest import GOLDEN, PKG, ROOT, bits_equal, first_mismatch, load_f32, load_scene
from test_gpu_rays import PAD, _intersect, _mixed, _odd_rays
from test_raytrace_host import (STACK_SCENES, STACK_SIZES, THREADS, fold, mixed_rays, sample_rays,
                                scene_with_lights, stack_batch, stack_colours)

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A


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


def _raytrace(torch, ctx, rays, S, order=None):
    """The context path: colours of `rays` ((N, 6) float32) as (N, 3) float32;
    the destination is pre-filled and PAD records longer, the tail must stay.
    order: N uint32 indices for the _indexed launch."""
    n = len(rays)
    src = torch.from_numpy(np.ascontiguousarray(rays, np.float32).reshape(-1, 6)).cuda()
    dst = torch.full(((n + PAD) * 3,), FILL, dtype=torch.int32, device="cuda")
    idx = None if order is None else torch.from_numpy(np.asarray(order, np.uint32).view(np.int32)).cuda()
    ctx.raytrace_device(src.data_ptr() if n else dst.data_ptr(), n, dst.data_ptr(), stack_size=S,
                        stream=torch.cuda.current_stream().cuda_stream,
                        order=0 if idx is None else idx.data_ptr())
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n * 3:] == FILL).all(), "colours past the batch were written"
    return out[:n * 3].view(np.float32).reshape(n, 3)


def _diff(got, want, rays):
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    if not len(bad):
        return None
    k = int(bad[0])
    return f"{len(bad)} of {len(got)} colours differ; first at {k}: ray {rays[k]} {got[k]} vs {want[k]}"


# ---- 5. device == host plain loops ----

@pytest.mark.parametrize("name", [0, 1, 12, 64, 65, 200, "c5"])
def test_device_equals_plain_loops(R, torch_cuda, name):
    """Batches of 1, 63, 64, 65 and 4097 rays (a single-lane wave, ragged last
    waves, more than one workgroup) of the mix of test_raytrace_host.py: rays
    from inside and from far outside the scene in one wave."""
    sph, lg = scene_with_lights(name)
    S = 8 if name == "c5" else 6
    big = mixed_rays(sph, lg, 4097, 500 + len(sph))
    want = R.raytrace_host(sph, lg, big, stack_size=S, walk=0, threads=THREADS)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        for n in (1, 63, 64, 65, 4097):  # prefixes: a ray's colour does not depend on its batch
            got = _raytrace(torch_cuda, ctx, big[:n], S)
            assert got.tobytes() == want[:n].tobytes(), (n, _diff(got, want[:n], big))
        if name == 12:
            for S2 in (1, 16):
                got = _raytrace(torch_cuda, ctx, big[:1000], S2)
                w2 = R.raytrace_host(sph, lg, big[:1000], stack_size=S2, walk=0, threads=THREADS)
                assert got.tobytes() == w2.tobytes(), (S2, _diff(got, w2, big))
            ctx.set_semantics(1)  # the OpenCL kernel's semantics
            got = _raytrace(torch_cuda, ctx, big[:1000], S)
            w2 = R.raytrace_host(sph, lg, big[:1000], stack_size=S, semantics=1, walk=0,
                                 threads=THREADS)
            assert got.tobytes() == w2.tobytes(), ("opencl", _diff(got, w2, big))
            assert w2.tobytes() != want[:1000].tobytes()  # the two semantics differ here
    finally:
        ctx.close()
    if len(sph) >= 2:
        assert (np.nan_to_num(want) > 0).any()


# ---- 5b. every stack size (the kernel of each S comes from one table) ----

@pytest.mark.parametrize("name", STACK_SCENES)
def test_every_stack_size(R, torch_cuda, name):
    """The 130 rays of test_raytrace_host.stack_batch (two full waves and a
    two-lane tail) at every S, CPU semantics, and at S = 2 and 16 with the
    OpenCL kernel's; one _indexed launch with the order reversed.  The host's
    walk 0 at that S is what tells neighbouring sizes apart (STACK_TOLD_APART
    there)."""
    sph, lg, rays = stack_batch(name)
    assert len(rays) == 130
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        for S in STACK_SIZES:
            got = _raytrace(torch_cuda, ctx, rays, S)
            want = stack_colours(name, S)
            assert got.tobytes() == want.tobytes(), (S, _diff(got, want, rays))
        got = _raytrace(torch_cuda, ctx, rays, 6, order=np.arange(len(rays))[::-1])
        assert got.tobytes() == stack_colours(name, 6).tobytes(), "indexed"
        ctx.set_semantics(1)  # the OpenCL kernel's semantics
        for S in (2, 16):
            got = _raytrace(torch_cuda, ctx, rays, S)
            want = stack_colours(name, S, 1)
            assert got.tobytes() == want.tobytes(), ("opencl", S, _diff(got, want, rays))
    finally:
        ctx.close()
    assert stack_colours(name, 2, 1).tobytes() != stack_colours(name, 2).tobytes()


# ---- 6. a wave of only `odd` rays ----

@pytest.mark.parametrize("name", [200, "c5"])
def test_waves_outside_the_walks_range(R, torch_cuda, name):
    """BVH scenes: a wave whose 64 rays are all outside the BVH walk's range
    (every level-0 query takes the plain loop) followed by a wave with one
    ordinary ray, in one launch, and the 64 alone."""
    sph, lg = scene_with_lights(name)
    S = 8 if name == "c5" else 6
    rays = np.concatenate([_odd_rays(sph, 31), raygen.inside(np.random.default_rng(77), sph, 1)])
    want = R.raytrace_host(sph, lg, rays, stack_size=S, walk=0)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        for n in (65, 64):
            got = _raytrace(torch_cuda, ctx, rays[:n], S)
            assert got.tobytes() == want[:n].tobytes(), (n, _diff(got, want[:n], rays))
    finally:
        ctx.close()


# ---- 7. sample rays of a frame == the render ----

def test_sample_rays_fold_to_the_render(R, golden, torch_cuda):
    torch = torch_cuda
    c = golden["configs"]["c3"]
    sph, lg = load_scene("c3", c["spheres"], c["lights"])
    W, H = c["small"]["W"], c["small"]["H"]
    aa = golden["aliasFactor"]
    rays, nS = sample_rays(W, H, aa, golden["zoom"])
    want = load_f32(os.path.join(GOLDEN, "c3.small.f32"), (H, W, 3))
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        ctx.render_device(W, H, fb.data_ptr(), zoom=golden["zoom"], alias_factor=aa,
                          stack_size=c["stack_size"],
                          stream=torch.cuda.current_stream().cuda_stream)
        col = _raytrace(torch, ctx, rays, c["stack_size"])
    finally:
        ctx.close()
    fb = fb.cpu().numpy()
    mine = fold(col, W, H, nS, aa)
    assert bits_equal(fb, want), first_mismatch(fb, want)
    assert bits_equal(mine, fb), first_mismatch(mine, fb)


# ---- 8. no interference ----

def test_no_interference_with_renders(R, golden, torch_cuda):
    """render, raytrace, render, intersect on one context and one stream: both
    frames the golden bits, both batches the host's."""
    torch = torch_cuda
    c = golden["configs"]["c3"]
    sph, lg = load_scene("c3", c["spheres"], c["lights"])
    W, H, S = c["small"]["W"], c["small"]["H"], c["stack_size"]
    want = load_f32(os.path.join(GOLDEN, "c3.small.f32"), (H, W, 3))
    rays = mixed_rays(sph, lg, 3000, 5)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        fb1 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        fb2 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        dr = torch.from_numpy(rays).cuda()
        col = torch.zeros((len(rays), 3), dtype=torch.float32, device="cuda")
        hits = torch.zeros((len(rays) * 8,), dtype=torch.int32, device="cuda")
        ctx.render_device(W, H, fb1.data_ptr(), stack_size=S, stream=stream)
        ctx.raytrace_device(dr.data_ptr(), len(rays), col.data_ptr(), stack_size=S, stream=stream)
        ctx.render_device(W, H, fb2.data_ptr(), stack_size=S, stream=stream)
        ctx.intersect_device(dr.data_ptr(), len(rays), hits.data_ptr(), stream=stream)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    for fb in (fb1.cpu().numpy(), fb2.cpu().numpy()):
        assert bits_equal(fb, want), first_mismatch(fb, want)
    w = R.raytrace_host(sph, lg, rays, stack_size=S, threads=THREADS)
    assert col.cpu().numpy().tobytes() == w.tobytes(), _diff(col.cpu().numpy(), w, rays)
    assert hits.cpu().numpy().tobytes() == R.intersect_host(sph, rays, threads=THREADS).tobytes()


# ---- 9. one-shot form and the driver ----

def test_one_shot_and_host_driver(R, torch_cuda, tmp_path):
    sph, lg = R.reference_scene()
    rays = np.concatenate([raygen.primary(40, 30), _mixed(sph, 1000, 9)])
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        want = _raytrace(torch_cuda, ctx, rays, 6)
        want_hits = _intersect(R, torch_cuda, ctx, rays)
    finally:
        ctx.close()
    assert want.tobytes() == R.raytrace_host(sph, lg, rays, threads=THREADS).tobytes()
    got = R.raytrace(sph, lg, rays)
    assert got.shape == (len(rays), 3) and got.tobytes() == want.tobytes()
    assert R.raytrace(sph, lg, rays[:0]).shape == (0, 3)
    W, H = 160, 120
    fin, fhit, frad = (str(tmp_path / f) for f in ("rays.bin", "hits.bin", "radiance.bin"))
    ppm, ppm0 = str(tmp_path / "o.ppm"), str(tmp_path / "o0.ppm")
    rays.tofile(fin)
    base = [os.path.join(PKG, "rtg_main"), "--scene",
            os.path.join(ROOT, "scenes", "reference.scene"), "--width", str(W), "--height", str(H)]
    r = subprocess.run(base + ["--out", ppm, "--rays", fin, "--hits", fhit, "--radiance", frad],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(frad, "rb").read() == want.tobytes()
    assert open(fhit, "rb").read() == want_hits.tobytes()  # --hits next to it: unchanged
    os.remove(frad)
    r = subprocess.run(base + ["--out", ppm0, "--rays", fin, "--radiance", frad],
                       capture_output=True, text=True, timeout=120)  # --radiance alone
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(frad, "rb").read() == want.tobytes()
    # the frame the driver wrote next to it is the render's, unchanged by the option
    assert open(ppm, "rb").read() == open(ppm0, "rb").read()
    assert open(ppm, "rb").read() == R.ppm_file_bytes(R.render(sph, lg, W, H))
    for extra in (["--rays", fin], ["--radiance", frad], ["--hits", fhit]):  # no GPU call
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("go together" in r.stdout or "needs --rays" in r.stdout)


# ---- 10. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    ctx = R.Context(0)
    try:
        rays = torch.from_numpy(raygen.primary(8, 8)).cuda()
        col = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
        with pytest.raises(R.RtgError, match="scene"):  # no scene yet
            ctx.raytrace_device(rays.data_ptr(), 64, col.data_ptr())
        ctx.set_scene(sph, lg)
        for args, kw, msg in (((0, 64, col.data_ptr()), {}, "null ray"),
                              ((rays.data_ptr(), 64, 0), {}, "null colour"),
                              ((rays.data_ptr(), 64, col.data_ptr()), {"stack_size": 0}, "stackSize 0"),
                              ((rays.data_ptr(), 64, col.data_ptr()), {"stack_size": 17}, "stackSize 17"),
                              ((rays.data_ptr(), 1 << 37, col.data_ptr()), {}, "too large")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.raytrace_device(*args, **kw)
        ctx.raytrace_device(rays.data_ptr(), 0, col.data_ptr())  # n == 0: RTG_OK, no launch
        torch.cuda.synchronize()
        assert int(col.abs().sum()) == 0  # nothing was launched
        host = np.zeros((4, 3), np.float32)
        with pytest.raises(R.RtgError, match="null ray"):  # the one-shot form's own check
            R._check(R.lib().rtg_raytrace(0, R._ptr(sph), len(sph), R._ptr(lg), len(lg), None, 4, 6,
                                          R._ptr(host)), "rtg_raytrace")
    finally:
        ctx.close()
