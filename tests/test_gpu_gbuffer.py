"""GPU tests of the primary-hit G-buffer (rtg_gbuffer_device / rtg_gbuffer,
csrc/rtg_gbuffer.hip) on an MI355X: the device kernel against the host form
(rtg_gbuffer_host, itself checked against the record definition in
test_gbuffer_host.py), byte for byte, over the kernel's paths: the masked
query (<= 64 spheres), the BVH (> 64), the sample-parallel mapping for every
nAA it takes and the one-lane-per-pixel fallback, shards, and the other entry
points.  Frames are small.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT, bits_equal, first_mismatch, load_f32, load_scene, random_scene

pytestmark = pytest.mark.gpu


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


def _records(R, t, rows, W):
    return t.cpu().numpy().view(R.GBUF_DTYPE).reshape(rows, W)


def _device(R, torch, ctx, W, H, zoom=-4.0, aa=3.0, row_block=16, shard=0, n_shards=1):
    """The context path: records of one shard as an (rows, W) array."""
    rows = R.shard_rows(H, row_block, shard, n_shards)
    t = torch.full((max(rows * W, 1) * 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.gbuffer_device(W, H, t.data_ptr(), zoom=zoom, alias_factor=aa, row_block=row_block,
                       shard=shard, n_shards=n_shards,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _records(R, t[:rows * W * 8], rows, W)


def _diff(a, b):
    bad = np.argwhere(a.view(np.uint32).reshape(a.shape + (8,))
                      != b.view(np.uint32).reshape(b.shape + (8,)))
    if not len(bad):
        return None
    y, x, _ = bad[0]
    return f"{len(bad)} words differ; first at ({y}, {x}): {a[y, x]} vs {b[y, x]}"


def _check(R, torch, sph, lg, frames):
    """Device == host for every (W, H, zoom, aa) of `frames`, one resident scene."""
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        for W, H, zoom, aa in frames:
            got = _device(R, torch, ctx, W, H, zoom, aa)
            want = R.gbuffer_host(sph, W, H, zoom, aa, threads=8)
            assert got.tobytes() == want.tobytes(), ((W, H, zoom, aa), _diff(got, want))
    finally:
        ctx.close()


def test_reference_scene(R, torch_cuda):
    sph, lg = R.reference_scene()
    # 2743 / 1200 / 300 pixel groups: many waves of 64 groups, a ragged last one
    _check(R, torch_cuda, sph, lg, [(160, 120, -4.0, 3.0), (160, 120, 4.0, 3.0),
                                    (160, 120, -4.0, 2.0), (160, 120, -4.0, 1.0)])


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c4", "c5"])
def test_golden_scenes_small(R, golden, torch_cuda, name):
    """c5: 1024 spheres, the BVH query."""
    c = golden["configs"][name]
    sph, lg = load_scene(name, c["spheres"], c["lights"])
    _check(R, torch_cuda, sph, lg, [(c["small"]["W"], c["small"]["H"], -4.0, 3.0)])


def test_random_scenes(R, torch_cuda):
    rng = np.random.default_rng(2031)
    for _ in range(12):
        n = int(rng.integers(0, 20))
        sph, lg = random_scene(rng, n, 2)
        W, H = int(rng.integers(1, 80)), int(rng.integers(1, 60))
        aa = float(rng.choice([1.0, 2.0, 3.0, 4.0]))
        zoom = float(rng.choice([-4.0, -4.0, -4.0, 4.0, -1.5]))
        _check(R, torch_cuda, sph, lg, [(W, H, zoom, aa)])


@pytest.mark.parametrize("n", [64, 65, 200])
def test_mask_bvh_boundary(R, torch_cuda, n):
    """64 spheres: the last masked scene; 65 and 200: the BVH, through both kernels."""
    sph, lg = random_scene(np.random.default_rng(n), n, 2)
    _check(R, torch_cuda, sph, lg, [(64, 48, -4.0, 3.0), (64, 48, -4.0, 2.0), (23, 17, -4.0, 9.0)])


@pytest.mark.parametrize("aa", [1.0, 2.0, 2.5, 3.0, 4.0, 8.0, 9.0, 0.0])
def test_alias_factors_and_odd_frames(R, torch_cuda, aa):
    """Pixels per group 64, 16, 7, 7, 4, 1; aa 9 and 0 take the fallback.  37x29:
    W*H no multiple of the pixels per group, groups straddling rows; 1x1."""
    sph, lg = random_scene(np.random.default_rng(77), 12, 2)
    _check(R, torch_cuda, sph, lg, [(37, 29, -4.0, aa), (1, 1, -4.0, aa), (37, 29, 4.0, aa)])


def test_shards(R, torch_cuda):
    """H = 30 in blocks of 4 over 3 shards: a ragged last block."""
    sph, lg = R.reference_scene()
    W, H, B, G = 37, 30, 4, 3
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        full = _device(R, torch_cuda, ctx, W, H)
        assert full.tobytes() == R.gbuffer_host(sph, W, H).tobytes()
        seen = 0
        for g in range(G):
            part = _device(R, torch_cuda, ctx, W, H, row_block=B, shard=g, n_shards=G)
            rows = R.shard_row_indices(H, B, g, G)
            assert part.tobytes() == full[rows].tobytes(), g
            seen += len(rows)
        assert seen == H
    finally:
        ctx.close()


def test_no_interference_with_renders(R, golden, torch_cuda):
    """render, gbuffer, render, gbuffer at another size on one context and one
    stream: both frames the golden bits, both G-buffers the host's, and no
    pixel without a hit is anything but +0 in the GPU's own frame."""
    torch = torch_cuda
    c = golden["configs"]["c3"]
    sph, lg = load_scene("c3", c["spheres"], c["lights"])
    W, H = c["small"]["W"], c["small"]["H"]
    want = load_f32(os.path.join(GOLDEN, "c3.small.f32"), (H, W, 3))
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        fb1 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        fb2 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        g1 = torch.zeros((H * W * 8,), dtype=torch.int32, device="cuda")
        g2 = torch.zeros((29 * 37 * 8,), dtype=torch.int32, device="cuda")
        ctx.render_device(W, H, fb1.data_ptr(), stack_size=c["stack_size"], stream=stream)
        ctx.gbuffer_device(W, H, g1.data_ptr(), stream=stream)
        ctx.render_device(W, H, fb2.data_ptr(), stack_size=c["stack_size"], stream=stream)
        ctx.gbuffer_device(37, 29, g2.data_ptr(), alias_factor=2.0, stream=stream)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    for fb in (fb1.cpu().numpy(), fb2.cpu().numpy()):
        assert bits_equal(fb, want), first_mismatch(fb, want)
    a, b = _records(R, g1, H, W), _records(R, g2, 29, 37)
    assert a.tobytes() == R.gbuffer_host(sph, W, H).tobytes()
    assert b.tobytes() == R.gbuffer_host(sph, 37, 29, alias_factor=2.0).tobytes()
    miss = a["hits"] == 0
    assert miss.any() and (fb1.cpu().numpy().view(np.uint32)[miss] == 0).all()


def test_one_shot_and_host_driver(R, torch_cuda, tmp_path):
    sph, lg = R.reference_scene()
    W, H = 160, 120
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        want = _device(R, torch_cuda, ctx, W, H)
    finally:
        ctx.close()
    assert R.gbuffer(sph, W, H).tobytes() == want.tobytes()
    out, ppm = str(tmp_path / "g.bin"), str(tmp_path / "o.ppm")
    r = subprocess.run([os.path.join(PKG, "rtg_main"), "--scene",
                        os.path.join(ROOT, "scenes", "reference.scene"), "--width", str(W),
                        "--height", str(H), "--out", ppm, "--gbuffer", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out, "rb").read() == want.tobytes()
    # the frame the driver wrote next to it is the render's, unchanged by the option
    fb = R.render(sph, lg, W, H)
    assert open(ppm, "rb").read() == R.ppm_file_bytes(fb)
    assert (fb.view(np.uint32)[want["hits"] == 0] == 0).all()


def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    ctx = R.Context(0)
    try:
        t = torch.zeros((64 * 8,), dtype=torch.int32, device="cuda")
        with pytest.raises(R.RtgError, match="scene"):  # no scene yet
            ctx.gbuffer_device(8, 8, t.data_ptr())
        ctx.set_scene(sph, lg)
        for kw, msg in ((dict(width=0), "empty frame"), (dict(alias_factor=300.0), "aliasFactor"),
                        (dict(row_block=0), "sharding"), (dict(shard=2, n_shards=2), "sharding"),
                        (dict(dst_ptr=0), "null destination"),
                        (dict(dst_ptr=t.data_ptr() + 4), "aligned")):
            args = dict(width=8, height=8, dst_ptr=t.data_ptr())
            args.update(kw)
            with pytest.raises(R.RtgError, match=msg):
                ctx.gbuffer_device(**args)
        torch.cuda.synchronize()
        assert int(t.abs().sum()) == 0  # nothing was launched
    finally:
        ctx.close()
