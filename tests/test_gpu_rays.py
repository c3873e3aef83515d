"""GPU tests of the batch ray queries (rtg_intersect_device / rtg_visible_device
and the one-shot forms, csrc/rtg_rays.hip) on an MI355X: the kernels against
the host's plain loops (rtg_intersect_host / rtg_visible_host with walk = 0,
themselves checked against the definition in test_rays_host.py), byte for
byte, over the kernels' paths: no sphere, the 64-sphere query, the BVH with
origins inside and far outside its origin box in one wave, ragged last waves,
and the other entry points.  Batches are small.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import raygen
from conftest import GOLDEN, PKG, ROOT, bits_equal, first_mismatch, load_f32, load_scene
from raygen import diff_hits as _diff, scene

pytestmark = pytest.mark.gpu

PAD = 64  # records the destinations are longer than the batch


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


def _intersect(R, torch, ctx, rays):
    """The context path: hits of `rays` ((N, 6) float32); the destination is
    pre-filled with 0x5A bytes and PAD records longer, the tail must stay."""
    n = len(rays)
    src = torch.from_numpy(np.ascontiguousarray(rays, np.float32).reshape(-1, 6)).cuda()
    dst = torch.full(((n + PAD) * 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.intersect_device(src.data_ptr() if n else dst.data_ptr(), n, dst.data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n * 8:] == 0x5A5A5A5A).all(), "records past the batch were written"
    return out[:n * 8].view(R.HIT_DTYPE)


def _visible(R, torch, ctx, segs):
    n = len(segs)
    src = torch.from_numpy(np.ascontiguousarray(segs, np.float32).reshape(-1, 6)).cuda()
    dst = torch.full((n + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.visible_device(src.data_ptr() if n else dst.data_ptr(), n, dst.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n:] == 0x5A).all(), "bytes past the batch were written"
    return out[:n]


def _mixed(sph, n, seed):
    """n rays: generators (b) to (f) mixed, inside and outside origins
    interleaved lane by lane."""
    rng = np.random.default_rng(seed)
    q = n // 2 + 1
    parts = [raygen.inside(rng, sph, q), raygen.scaled(rng, sph, q)]
    if len(sph) >= 2:
        parts += [raygen.interleave(raygen.inside(rng, sph, q), raygen.outside(rng, sph, q)),
                  raygen.surface(rng, sph, q), raygen.outside(rng, sph, q)]
    rays = np.concatenate(parts)
    return rays[rng.permutation(len(rays))[:n]]


def _mixed_segments(sph, n, seed):
    rng = np.random.default_rng(seed)
    if len(sph) < 2:
        return raygen.inside(rng, sph, n)
    segs = np.concatenate([raygen.segments(rng, sph, n), raygen.scaled(rng, sph, n // 4 + 1)])
    return segs[rng.permutation(len(segs))[:n]]


# ---- 6. device == host plain loops ----

@pytest.mark.parametrize("name", [0, 1, 12, 64, 65, 200, "c5"])
def test_device_equals_plain_loops(R, torch_cuda, name):
    """Batches of 1, 63, 64, 65 and 4097 rays: a single-lane wave, ragged last
    waves, more than one workgroup."""
    sph = scene(name)
    ctx = R.Context(0)
    ctx.set_scene(sph, np.zeros(0, R.LIGHT_DTYPE))
    try:
        for n in (1, 63, 64, 65, 4097):
            rays = _mixed(sph, n, 100 + n)
            got = _intersect(R, torch_cuda, ctx, rays)
            want = R.intersect_host(sph, rays, walk=0, threads=8)
            assert got.tobytes() == want.tobytes(), (n, _diff(got, want))
            segs = _mixed_segments(sph, n, 200 + n)
            vis = _visible(R, torch_cuda, ctx, segs)
            assert vis.tobytes() == R.visible_host(sph, segs, walk=0, threads=8).tobytes(), n
        if len(sph) >= 12:
            assert (want["id"] >= 0).mean() > 0.1
    finally:
        ctx.close()


# ---- 6b. waves with no lane in the walk's range ----

def _odd_rays(sph, seed):
    """64 rays outside the BVH walk's range (rtg_rays.hip, `odd`), k % 4: a
    zero direction, a NaN / +-inf origin component, direction lengths 2^-40
    and 2^40 (2 d.d outside [2^-60, 2^60])."""
    rng = np.random.default_rng(seed)
    out = raygen.inside(rng, sph, 64).astype(np.float64)
    unit = out[:, 3:] / np.linalg.norm(out[:, 3:], axis=1, keepdims=True)
    k = np.arange(64)
    out[k % 4 == 0, 3:] = 0
    out[k % 4 == 2, 3:] = unit[k % 4 == 2] * 2.0 ** -40
    out[k % 4 == 3, 3:] = unit[k % 4 == 3] * 2.0 ** 40
    bad = np.flatnonzero(k % 4 == 1)
    out[bad, (bad // 4) % 3] = np.asarray([np.nan, np.inf, -np.inf])[(bad // 12) % 3]
    out = out.astype(np.float32)
    o, d = out[:, :3], out[:, 3:].astype(np.float64)
    a2 = 2.0 * (d * d).sum(1)
    assert (~(np.abs(o) <= 2.0 ** 56).all(1) | ~((a2 >= 2.0 ** -60) & (a2 <= 2.0 ** 60))).all()
    return out


def _odd_segments(sph, seed):
    """The same for segments, whose direction is normalised (a length alone
    puts none outside the range), k % 4: a == b, a NaN / +-inf component of a,
    one of b, a component of a at +-2^60 (finite, beyond the slab range 2^56)."""
    rng = np.random.default_rng(seed)
    out = raygen.inside(rng, sph, 64)
    out[:, 3:] = raygen.inside(rng, sph, 64)[:, :3]
    k = np.arange(64)
    out[k % 4 == 0, 3:] = out[k % 4 == 0, :3]
    vals = np.asarray([np.nan, np.inf, -np.inf], np.float32)
    for kind, col0 in ((1, 0), (2, 3)):
        bad = np.flatnonzero(k % 4 == kind)
        out[bad, col0 + (bad // 4) % 3] = vals[(bad // 12) % 3]
    far = np.flatnonzero(k % 4 == 3)
    out[far, (far // 4) % 3] = np.where(far % 8 == 3, 2.0 ** 60, -2.0 ** 60)
    with np.errstate(invalid="ignore"):  # inf - inf
        a, dist = out[:, :3], out[:, 3:].astype(np.float64) - out[:, :3]
        gap = (dist * dist).sum(1)
    assert (~(np.abs(a) <= 2.0 ** 56).all(1) | ~np.isfinite(gap) | (gap == 0)).all()
    return out


@pytest.mark.parametrize("name", [200, "c5"])
def test_waves_outside_the_walks_range(R, torch_cuda, name):
    """BVH scenes: a wave whose 64 lanes are all outside the walk's range (the
    walk returns at once, every lane takes the plain loop) followed by a wave
    with one ordinary ray (the normal walk) in one launch, and the 64 alone;
    hits and visibility are the host's plain loops, byte for byte, and nothing
    is written past the batch (_intersect, _visible).  visible_device also
    takes the ray arrays as segments, as the other tests do."""
    sph = scene(name)
    rng = np.random.default_rng(77)
    rays = np.concatenate([_odd_rays(sph, 31), raygen.inside(rng, sph, 1)])
    segs = np.concatenate([_odd_segments(sph, 32), raygen.segments(rng, sph, 4)[:1]])
    ctx = R.Context(0)
    ctx.set_scene(sph, np.zeros(0, R.LIGHT_DTYPE))
    try:
        for n in (65, 64):
            got = _intersect(R, torch_cuda, ctx, rays[:n])
            want = R.intersect_host(sph, rays[:n], walk=0)
            assert got.tobytes() == want.tobytes(), (n, _diff(got, want))
            for s in (segs[:n], rays[:n]):
                vis = _visible(R, torch_cuda, ctx, s)
                assert vis.tobytes() == R.visible_host(sph, s, walk=0).tobytes(), n
    finally:
        ctx.close()


# ---- 7. primary rays == G-buffer ----

@pytest.mark.parametrize("name", [12, 200])
def test_primary_rays_equal_gbuffer(R, torch_cuda, name):
    torch = torch_cuda
    sph = scene(name)
    W, H = 64, 48
    ctx = R.Context(0)
    ctx.set_scene(sph, np.zeros(0, R.LIGHT_DTYPE))
    try:
        hits = _intersect(R, torch, ctx, raygen.primary(W, H))
        g = torch.zeros((H * W * 8,), dtype=torch.int32, device="cuda")
        ctx.gbuffer_device(W, H, g.data_ptr(), alias_factor=1.0,
                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    g = g.cpu().numpy().view(R.GBUF_DTYPE)
    assert (hits["id"] == g["id"]).all()
    assert hits["t"].tobytes() == g["t"].tobytes()
    assert hits["normal"].tobytes() == g["normal"].tobytes()
    assert (g["hits"] == (hits["id"] >= 0)).all() and (hits["id"] >= 0).any()


# ---- 8. no interference ----

def test_no_interference_with_renders(R, golden, torch_cuda):
    """render, intersect, render, visible on one context and one stream: both
    frames the golden bits, both query results the host's."""
    torch = torch_cuda
    c = golden["configs"]["c3"]
    sph, lg = load_scene("c3", c["spheres"], c["lights"])
    W, H = c["small"]["W"], c["small"]["H"]
    want = load_f32(os.path.join(GOLDEN, "c3.small.f32"), (H, W, 3))
    rays, segs = _mixed(sph, 3000, 5), _mixed_segments(sph, 3000, 6)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        fb1 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        fb2 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        dr, ds = torch.from_numpy(rays).cuda(), torch.from_numpy(segs).cuda()
        hits = torch.zeros((len(rays) * 8,), dtype=torch.int32, device="cuda")
        vis = torch.zeros((len(segs),), dtype=torch.uint8, device="cuda")
        ctx.render_device(W, H, fb1.data_ptr(), stack_size=c["stack_size"], stream=stream)
        ctx.intersect_device(dr.data_ptr(), len(rays), hits.data_ptr(), stream=stream)
        ctx.render_device(W, H, fb2.data_ptr(), stack_size=c["stack_size"], stream=stream)
        ctx.visible_device(ds.data_ptr(), len(segs), vis.data_ptr(), stream=stream)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    for fb in (fb1.cpu().numpy(), fb2.cpu().numpy()):
        assert bits_equal(fb, want), first_mismatch(fb, want)
    assert hits.cpu().numpy().tobytes() == R.intersect_host(sph, rays, threads=8).tobytes()
    assert vis.cpu().numpy().tobytes() == R.visible_host(sph, segs, threads=8).tobytes()


# ---- 9. one-shot forms and the driver ----

def test_one_shot_and_host_driver(R, torch_cuda, tmp_path):
    sph, lg = R.reference_scene()
    rays = np.concatenate([raygen.primary(40, 30), _mixed(sph, 1000, 9)])
    segs = _mixed_segments(sph, 1000, 10)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        want = _intersect(R, torch_cuda, ctx, rays)
        want_vis = _visible(R, torch_cuda, ctx, segs)
    finally:
        ctx.close()
    assert R.intersect(sph, rays).tobytes() == want.tobytes()
    assert R.visible(sph, segs).tobytes() == want_vis.tobytes()
    assert len(R.intersect(sph, rays[:0])) == 0 and len(R.visible(sph, segs[:0])) == 0
    W, H = 160, 120
    fin, fout = str(tmp_path / "rays.bin"), str(tmp_path / "hits.bin")
    ppm, ppm0 = str(tmp_path / "o.ppm"), str(tmp_path / "o0.ppm")
    rays.tofile(fin)
    base = [os.path.join(PKG, "rtg_main"), "--scene",
            os.path.join(ROOT, "scenes", "reference.scene"), "--width", str(W), "--height", str(H)]
    r = subprocess.run(base + ["--out", ppm, "--rays", fin, "--hits", fout],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(fout, "rb").read() == want.tobytes()
    # the frame the driver wrote next to it is the render's, unchanged by the option
    r = subprocess.run(base + ["--out", ppm0], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(ppm, "rb").read() == open(ppm0, "rb").read()
    assert open(ppm, "rb").read() == R.ppm_file_bytes(R.render(sph, lg, W, H))


# ---- 10. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    ctx = R.Context(0)
    try:
        rays = torch.from_numpy(raygen.primary(8, 8)).cuda()
        hits = torch.zeros((64 * 8,), dtype=torch.int32, device="cuda")
        vis = torch.zeros((64,), dtype=torch.uint8, device="cuda")
        with pytest.raises(R.RtgError, match="scene"):  # no scene yet
            ctx.intersect_device(rays.data_ptr(), 64, hits.data_ptr())
        with pytest.raises(R.RtgError, match="scene"):
            ctx.visible_device(rays.data_ptr(), 64, vis.data_ptr())
        ctx.set_scene(sph, lg)
        for args, msg in (((0, 64, hits.data_ptr()), "null"),
                          ((rays.data_ptr(), 64, 0), "null"),
                          ((rays.data_ptr(), 64, hits.data_ptr() + 4), "aligned")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.intersect_device(*args)
        for args in ((0, 64, vis.data_ptr()), (rays.data_ptr(), 64, 0)):
            with pytest.raises(R.RtgError, match="null"):
                ctx.visible_device(*args)
        with pytest.raises(R.RtgError, match="too large"):  # 2^31 workgroups
            ctx.intersect_device(rays.data_ptr(), 1 << 37, hits.data_ptr())
        with pytest.raises(R.RtgError, match="too large"):
            ctx.visible_device(rays.data_ptr(), 1 << 37, vis.data_ptr())
        ctx.intersect_device(rays.data_ptr(), 0, hits.data_ptr())  # n == 0: RTG_OK, no launch
        ctx.visible_device(rays.data_ptr(), 0, vis.data_ptr())
        torch.cuda.synchronize()
        assert int(hits.abs().sum()) == 0 and int(vis.sum()) == 0  # nothing was launched
    finally:
        ctx.close()
