"""GPU tests of views folded into per-group coefficients (rtg_views_fold_device,
rtg_render_views_fold_device and the one-shot form; csrc/rtg_fold.hip and the
per-S views_fold kernels) on an MI355X, against the host's plain loops
(rtg_views_fold_host, pinned to a numpy restatement in
test_views_fold_host.py), byte for byte: the device fold on that file's random
and hostile frames, the fused call over the kernel's scene paths (no sphere,
the flat loop, the 64-sphere query, the BVH), ragged tiles, cube tables with
non-finite pixels, every stack size and both semantics, fused against unfused
on the device, weights written on the device, streams and other calls on one
context, the entry-point errors and the driver.  Every destination and the
scratch are pre-filled; every destination is PAD words longer than needed and
the tail must stay.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, bits_equal
from test_camera_host import STACK_AA, STACK_FRAMES_TOLD_APART, STACK_POSE, pose, stack_frame
from test_gpu_views import IDENTITY, _second_stack_frame, mixed_table
from test_raytrace_host import (STACK_H, STACK_SCENES, STACK_SIZES, STACK_W, THREADS, mixed_rays,
                                scene_with_lights)
from test_views_fold_host import SKIP, fold_cases, hostile_cases, random_weights
from test_views_host import VAA, VH, VW, VZOOM, batch_poses, view_frames

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0x5A5A5A5A
PAD = 64  # words behind every destination that must stay as they were


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


class Buffers:
    """Pre-filled destinations and scratch of one fold of n views: `out`
    (nGroups * K * 3 + PAD words), `cnt` (nGroups + PAD) and `scratch`."""

    def __init__(self, torch, R, n, W, H, G, K):
        self.torch, self.groups, self.K = torch, n // G, K
        self.bytes = R.views_fold_scratch(n, W, H, K)
        assert self.bytes == n * ((W + 7) // 8) * ((H + 7) // 8) * (3 * K + 1) * 4
        fill = lambda words: torch.full((words,), FILL, dtype=torch.int32, device="cuda")  # noqa: E731
        self.out = fill(self.groups * K * 3 + PAD)
        self.cnt = fill(self.groups + PAD)
        self.scratch = fill(max(self.bytes // 4, 1) + PAD)

    def result(self, counted=True):
        self.torch.cuda.synchronize()
        out, cnt, scr = (t.cpu().numpy().view(np.uint32) for t in (self.out, self.cnt, self.scratch))
        m = self.groups * self.K * 3
        assert (out[m:] == FILL).all(), "words past the last coefficient were written"
        assert (cnt[self.groups if counted else 0:] == FILL).all(), "counts past the last group"
        assert (scr[self.bytes // 4:] == FILL).all(), "words past the scratch were written"
        return out[:m].reshape(self.groups, self.K, 3), cnt[:self.groups]


def _stream(torch, stream=None):
    return (stream or torch.cuda.current_stream()).cuda_stream


def _fold(torch, R, ctx, frames, w, G, K, flags=0, counted=True, stream=None):
    """Context.views_fold of host or device frames: (words, counts)."""
    d_fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.array(frames, F)).cuda()
    d_w = w if torch.is_tensor(w) else torch.from_numpy(np.array(w, F)).cuda()
    n, H, W = d_fr.shape[:3]
    b = Buffers(torch, R, n, W, H, G, K)
    torch.cuda.synchronize()
    ctx.views_fold(d_fr.data_ptr(), n, W, H, R.fold_params(G, K, flags), d_w.data_ptr(),
                   b.out.data_ptr(), b.scratch.data_ptr(), b.bytes,
                   skipped_ptr=b.cnt.data_ptr() if counted else 0, stream=_stream(torch, stream))
    return b.result(counted)


def _fused(torch, R, ctx, cams, W, H, zoom, aa, S, w, G, K, flags=0, counted=True, stream=None):
    """Context.render_views_fold of the poses `cams` ((n, 12) on the host, or a
    device tensor): (words, counts)."""
    d_cams = cams if torch.is_tensor(cams) else torch.from_numpy(
        np.ascontiguousarray(cams, F).reshape(-1, 12)).cuda()
    d_w = w if torch.is_tensor(w) else torch.from_numpy(np.array(w, F)).cuda()
    n = d_cams.shape[0]
    b = Buffers(torch, R, n, W, H, G, K)
    torch.cuda.synchronize()
    ctx.render_views_fold(d_cams.data_ptr(), n, W, H, R.fold_params(G, K, flags), d_w.data_ptr(),
                          b.out.data_ptr(), b.scratch.data_ptr(), b.bytes,
                          skipped_ptr=b.cnt.data_ptr() if counted else 0, zoom=zoom,
                          alias_factor=aa, stack_size=S, stream=_stream(torch, stream))
    return b.result(counted)


def _host_fold(R, frames, w, G, K, flags=0):
    out, cnt = R.views_fold_host(frames, w, R.fold_params(G, K, flags), threads=THREADS,
                                 skipped=True)
    return out.view(np.uint32), cnt


def _same(got, want, what):
    assert got[0].shape == want[0].shape, what
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), (what, "first (group, k, q)", bad[0], hex(got[0][tuple(bad[0])]),
                          hex(want[0][tuple(bad[0])]))
    assert (got[1] == want[1]).all(), (what, got[1], want[1])


def cams12(table):
    return np.ascontiguousarray(table).view(F).reshape(-1, 12)


# ---- the device fold against the host fold ----

def test_device_fold_equals_the_host_fold(R, torch_cuda):
    """Every case of test_views_fold_host.py, 70 groups x K = 16 among them
    (3430 stage-2 lanes: 14 workgroups of four waves); a context with no scene."""
    ctx = R.Context(0)
    try:
        for name, fr, w, G, K in fold_cases():
            _same(_fold(torch_cuda, R, ctx, fr, w, G, K), _host_fold(R, fr, w, G, K), name)
        for name, fr, w, G, K in hostile_cases():
            for flags in (0, SKIP):
                want = _host_fold(R, fr, w, G, K, flags)
                _same(_fold(torch_cuda, R, ctx, fr, w, G, K, flags), want, (name, flags))
                got = _fold(torch_cuda, R, ctx, fr, w, G, K, flags, counted=False)  # a null count
                assert (got[0] == want[0]).all(), (name, flags)
                assert ((want[1] > 0).any()) == bool(flags), name
    finally:
        ctx.close()


# ---- the fused call over the kernel's scene paths ----

@pytest.mark.parametrize("W,H,aa,S,sem", [(9, 9, 2.5, 6, 0), (65, 9, 1.0, 16, 1)])
@pytest.mark.parametrize("scene", [0, 12, 40, "c5"])
def test_fused_mixed_views(R, torch_cuda, scene, W, H, aa, S, sem):
    sph, lg = scene_with_lights(scene)
    cams, k = mixed_table(scene)
    w = random_weights(np.random.default_rng(11), 1, W, H, 9)
    frames = R.render_views_host(sph, lg, cams, W, H, VZOOM, aa, S, semantics=sem, walk=0,
                                 threads=THREADS)
    ctx = R.Context(0)
    try:
        ctx.set_semantics(sem)
        ctx.set_scene(sph, lg)
        assert (ctx.scene_stats()["bvh_nodes"] > 0) == (scene == "c5")
        for flags in (0, SKIP):
            want = _host_fold(R, frames, w, 1, 9, flags)
            _same(_fused(torch_cuda, R, ctx, cams, W, H, VZOOM, aa, S, w, 1, 9, flags), want,
                  (scene, flags))
            composed = R.render_views_fold_host(sph, lg, cams, W, H, w, R.fold_params(1, 9, flags),
                                                VZOOM, aa, S, semantics=sem, threads=THREADS)
            assert composed.view(np.uint32).tobytes() == want[0].tobytes()
    finally:
        ctx.close()
    # the NaN pose (whose rays hit nothing: a frame of zeros) spoils no other
    # group: its neighbours are the folds of their own frames, each from its own call
    assert (want[0][k] == 0).all()
    for v in (k - 1, k + 1):
        own = R.render_camera_host(sph, lg, cams[v], W, H, VZOOM, aa, S, semantics=sem, walk=0,
                                   threads=THREADS)
        assert _host_fold(R, own[None], w, 1, 9, SKIP)[0].tobytes() == want[0][v].tobytes()
    if len(sph):
        assert (want[0] != 0).any(), "black frames"


# ---- cube tables ----

@pytest.mark.parametrize("W,H", [(8, 8), (7, 5)])
def test_fused_cube_tables(R, torch_cuda, W, H):
    """Three probes of six faces in c5, two of them at sphere centres: G = 6."""
    sph, lg = scene_with_lights("c5")
    eyes = [sph["pos"][170], sph["pos"][425], (0.07, -0.03, -22.8)]
    cams = cams12(np.concatenate([R.camera_cube(e) for e in eyes]))
    w = (R.cube_sh_weights(W, 3, 1.0) if W == H
         else random_weights(np.random.default_rng(5), 6, W, H, 9))
    frames = R.render_views_host(sph, lg, cams, W, H, -1.0, 1.0, 8, threads=THREADS)
    bad = (~np.isfinite(frames)).any(-1).reshape(3, -1)
    assert bad.any() and (~bad).any(1).all(), "no non-finite pixel in the batch"
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        for flags in (0, SKIP):
            want = _host_fold(R, frames, w, 6, 9, flags)
            _same(_fused(torch_cuda, R, ctx, cams, W, H, -1.0, 1.0, 8, w, 6, 9, flags), want,
                  (W, H, flags))
    finally:
        ctx.close()
    assert (want[1] == bad.sum(1)).all() and np.isfinite(want[0].view(F)).all()
    assert (want[0] != 0).reshape(3, -1).any(1).all(), "a probe of zeros"


# ---- every stack size ----

@pytest.mark.parametrize("scene", STACK_SCENES)
def test_every_stack_size(R, torch_cuda, scene):
    """test_gpu_views.test_every_stack_size's two-view batch folded as one group:
    the fold kernel of each S comes from the same table as the views kernel's."""
    sph, lg = scene_with_lights(scene)
    cam0, zoom = pose(STACK_POSE, scene)
    cams = np.stack([cam0.reshape(12), pose("inside", scene)[0].reshape(12)])
    w = random_weights(np.random.default_rng(2), 2, STACK_W, STACK_H, 4)
    want = {}
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        for sem, sizes in ((0, STACK_SIZES), (1, (2, 16))):
            ctx.set_semantics(sem)
            for S in sizes:
                frames = np.stack([stack_frame(scene, S, sem), _second_stack_frame(scene, S, sem)])
                want[sem, S] = _host_fold(R, frames, w, 2, 4, SKIP)
                _same(_fused(torch_cuda, R, ctx, cams, STACK_W, STACK_H, zoom, STACK_AA, S, w, 2, 4,
                             SKIP), want[sem, S], (sem, S))
    finally:
        ctx.close()
    for k in STACK_FRAMES_TOLD_APART:  # the host's folds tell neighbouring sizes apart
        assert want[0, k][0].tobytes() != want[0, k + 1][0].tobytes(), k


# ---- fused against unfused, and no frame anywhere ----

def test_fused_equals_unfused_on_the_device(R, torch_cuda):
    torch = torch_cuda
    sph, lg = scene_with_lights("c5")
    cams = np.concatenate([batch_poses("c5"), batch_poses("c5")[::-1][:1]])  # six views
    W, H, aa, S, G, K = 17, 9, 2.0, 8, 3, 16
    w = random_weights(np.random.default_rng(8), G, W, H, K)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        d_cams = torch.from_numpy(cams).cuda()
        frames = torch.full((6, H, W, 3), 7.0, dtype=torch.float32, device="cuda")
        sentinel = torch.full((6 * H * W * 3,), FILL, dtype=torch.int32, device="cuda")
        ctx.render_views(d_cams.data_ptr(), 6, W, H, frames.data_ptr(), VZOOM, aa, S,
                         stream=_stream(torch))
        for flags in (0, SKIP):
            two = _fold(torch, R, ctx, frames, w, G, K, flags)
            one = _fused(torch, R, ctx, d_cams, W, H, VZOOM, aa, S, w, G, K, flags)
            _same(one, two, flags)
        torch.cuda.synchronize()
        # a buffer the size of the frames, passed nowhere, is as it was
        assert (sentinel.cpu().numpy().view(np.uint32) == FILL).all()
        host = frames.cpu().numpy()
    finally:
        ctx.close()
    _same(one, _host_fold(R, host, w, G, K, SKIP), "host")
    assert (one[0] != 0).any()


# ---- weights written on the device ----

def test_weights_written_on_the_device(R, torch_cuda):
    """The table scaled per weight by a torch op on the GPU; it never visits the
    host before the launch.  The result is the host's fold with the table read
    back afterwards."""
    torch = torch_cuda
    sph, lg = scene_with_lights(40)
    cams = cams12(np.concatenate([R.camera_cube(e) for e in ((0, 0, -8), (1, 1, -12))]))
    res = 9
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        base = torch.from_numpy(R.cube_sh_weights(res, 2, 1.0)).cuda()
        gain = torch.tensor([1.0, 0.5, -3.0, 1.0 / 3.0], dtype=torch.float32, device="cuda")
        table = (base * gain).contiguous()
        got = _fused(torch, R, ctx, cams, res, res, -1.0, 1.0, 6, table, 6, 4)
    finally:
        ctx.close()
    w = table.cpu().numpy()
    assert w.shape == (6, res, res, 4) and (w[..., 2] != R.cube_sh_weights(res, 2, 1.0)[..., 2]).any()
    frames = R.render_views_host(sph, lg, cams, res, res, -1.0, 1.0, 6, threads=THREADS)
    _same(got, _host_fold(R, frames, w, 6, 4), "device table")
    assert (got[0] != 0).any()


# ---- no views, a stream, other calls on the context ----

def test_no_views_streams_and_other_calls(R, torch_cuda):
    torch = torch_cuda
    sph, lg = scene_with_lights("c5")
    cams = batch_poses("c5")
    frames = view_frames("c5", 0, VW, VH, VAA, 8)
    w = random_weights(np.random.default_rng(4), 5, VW, VH, 9)
    want = _host_fold(R, frames, w, 5, 9, SKIP)
    W, H, S, aa = 40, 30, 8, 2.0
    rays = mixed_rays(sph, lg, 2000, 5)
    want_fb = R.render(sph, lg, W, H, -4.0, aa, S)
    want_col = R.raytrace_host(sph, lg, rays, stack_size=S, threads=THREADS)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        d_cams = torch.from_numpy(cams).cuda()
        d_w = torch.from_numpy(w).cuda()
        # no views: nothing launched, every pattern stays; tables and scratch may be null
        b = Buffers(torch, R, 5, VW, VH, 5, 9)
        p = R.fold_params(5, 9, SKIP)
        for table, scratch in ((d_cams.data_ptr(), b.scratch.data_ptr()), (0, 0)):
            ctx.render_views_fold(table, 0, VW, VH, p, d_w.data_ptr(), b.out.data_ptr(), scratch,
                                  0, skipped_ptr=b.cnt.data_ptr(), zoom=VZOOM, alias_factor=VAA,
                                  stack_size=8)
            ctx.views_fold(table, 0, VW, VH, p, d_w.data_ptr(), b.out.data_ptr(), scratch, 0,
                           skipped_ptr=b.cnt.data_ptr())
        torch.cuda.synchronize()
        for t in (b.out, b.cnt, b.scratch):
            assert (t.cpu().numpy().view(np.uint32) == FILL).all()
        # a stream of the caller's
        _same(_fused(torch, R, ctx, cams, VW, VH, VZOOM, VAA, 8, w, 5, 9, SKIP,
                     stream=torch.cuda.Stream()), want, "stream")
        # between a render, a batch of views and a batch of rays on one context and stream
        s = torch.cuda.Stream()
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        col = torch.zeros((len(rays), 3), dtype=torch.float32, device="cuda")
        vw = torch.full(((5 * VW * VH + PAD) * 3,), FILL, dtype=torch.int32, device="cuda")
        folds = [Buffers(torch, R, 5, VW, VH, 5, 9) for _ in (0, 1)]
        d_rays = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        q = s.cuda_stream

        def fold(bf):
            ctx.render_views_fold(d_cams.data_ptr(), 5, VW, VH, p, d_w.data_ptr(),
                                  bf.out.data_ptr(), bf.scratch.data_ptr(), bf.bytes,
                                  skipped_ptr=bf.cnt.data_ptr(), zoom=VZOOM, alias_factor=VAA,
                                  stack_size=8, stream=q)

        fold(folds[0])
        ctx.render_device(W, H, fb.data_ptr(), alias_factor=aa, stack_size=S, stream=q)
        ctx.render_views(d_cams.data_ptr(), 5, VW, VH, vw.data_ptr(), VZOOM, VAA, 8, stream=q)
        fold(folds[1])
        ctx.raytrace_device(d_rays.data_ptr(), len(rays), col.data_ptr(), stack_size=S, stream=q)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert bits_equal(fb.cpu().numpy(), want_fb)
    assert col.cpu().numpy().tobytes() == want_col.tobytes()
    out = vw.cpu().numpy()
    assert (out[5 * VW * VH * 3:] == FILL).all()
    assert out[:5 * VW * VH * 3].tobytes() == frames.tobytes()
    for k in (0, 1):
        _same(folds[k].result(), want, k)


# ---- entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    ctx = R.Context(0)
    try:
        cams = torch.from_numpy(np.stack([IDENTITY] * 6)).cuda()
        frames = torch.ones((6, 8, 8, 3), dtype=torch.float32, device="cuda")
        wt = torch.ones((3, 8, 8, 2), dtype=torch.float32, device="cuda")
        b = Buffers(torch, R, 6, 8, 8, 3, 2)
        c, fr, w, o, s, nb = (cams.data_ptr(), frames.data_ptr(), wt.data_ptr(), b.out.data_ptr(),
                              b.scratch.data_ptr(), b.bytes)
        assert nb == 6 * 7 * 4 and s % 16 == 0
        P = R.fold_params
        with pytest.raises(R.RtgError, match="scene"):  # the fused call needs one
            ctx.render_views_fold(c, 6, 8, 8, P(3, 2), w, o, s, nb)
        # the fold of frames does not: word for word the host's
        ctx.views_fold(fr, 6, 8, 8, P(3, 2), w, o, s, nb, skipped_ptr=b.cnt.data_ptr())
        got = b.result()
        assert (got[0].view(F) == 192.0).all() and (got[1] == 0).all()
        ctx.set_scene(sph, lg)
        shared = (((6, 8, 8, P(3, 2), 0, o, s, nb), {}, "null weight table"),
                  ((6, 8, 8, P(3, 2), w, 0, s, nb), {}, "null output"),
                  ((6, 8, 8, P(3, 2), w, o, 0, nb), {}, "null scratch"),
                  ((6, 8, 8, P(0, 2), w, o, s, nb), {}, "viewsPerGroup 0"),
                  ((6, 8, 8, P(4, 2), w, o, s, nb), {}, "not a multiple of viewsPerGroup 4"),
                  ((6, 8, 8, P(3, 0), w, o, s, nb), {}, "weights 0 outside"),
                  ((6, 8, 8, P(3, 17), w, o, s, nb), {}, "weights 17 outside"),
                  ((6, 8, 8, P(3, 2, 4), w, o, s, nb), {}, "unknown flag 0x4"),
                  ((6, 8, 8, P(3, 2), w, o, s, nb - 1), {}, "scratch of 167 bytes, 168 needed"),
                  ((6, 8, 8, P(3, 2), w, o, s, 0), {}, "scratch of 0 bytes"),
                  ((6, 8, 8, P(3, 2), w, o, s + 4, nb), {}, "16-byte aligned"),
                  ((6, 8, 8, P(3, 2), w, o, s + 8, nb), {}, "16-byte aligned"),
                  ((6, 0, 8, P(3, 2), w, o, s, nb), {}, "empty frame"),
                  ((6, 8, 0, P(3, 2), w, o, s, nb), {}, "empty frame"),
                  ((3 << 20, 4096, 4096, P(3, 2), w, o, s, nb), {}, "2\\^31-1 workgroups"),
                  ((0, 8, 8, P(3, 17), w, o, s, nb), {}, "weights 17 outside"),
                  ((0, 65536, 65536, P(0xFFFFFFFF, 16), w, o, s, nb), {}, "weight table too large"))
        for a, kw, msg in shared:
            with pytest.raises(R.RtgError, match=msg):
                ctx.views_fold(fr, *a, **kw)
            with pytest.raises(R.RtgError, match=msg):
                ctx.render_views_fold(c, *a, **kw)
        with pytest.raises(R.RtgError, match="null frames"):
            ctx.views_fold(0, 6, 8, 8, P(3, 2), w, o, s, nb)
        for a, kw, msg in (((0, 6, 8, 8, P(3, 2), w, o, s, nb), {}, "null pose table"),
                           ((c + 2, 6, 8, 8, P(3, 2), w, o, s, nb), {}, "4-byte aligned"),
                           ((c, 6, 8, 8, P(3, 2), w, o, s, nb), {"alias_factor": 257.0}, "aliasFactor"),
                           ((c, 6, 8, 8, P(3, 2), w, o, s, nb), {"stack_size": 0}, "stackSize 0"),
                           ((c, 6, 8, 8, P(3, 2), w, o, s, nb), {"stack_size": 17}, "stackSize 17"),
                           ((c, 0, 8, 8, P(3, 2), w, o, s, nb), {"stack_size": 17}, "stackSize 17")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.render_views_fold(*a, **kw)
        with pytest.raises(R.RtgError, match="weights 17"):  # the one-shot form's own check
            R.render_views_fold(sph, lg, IDENTITY.reshape(1, 12), 4, 4, np.ones((4, 4, 17), F),
                                R.fold_params(1, 17))
        # all of them refused before any launch: the patterns and the first result stand
        again = b.result()
        assert (again[0] == got[0]).all() and (again[1] == got[1]).all()
        # a scratch of exactly the bytes asked for, 16 bytes into an allocation, is enough
        b2 = Buffers(torch, R, 6, 8, 8, 3, 2)
        ctx.render_views_fold(c, 6, 8, 8, P(3, 2), w, b2.out.data_ptr(), b2.scratch.data_ptr() + 16,
                              nb, zoom=-4.0, alias_factor=1.0)
        torch.cuda.synchronize()
        want = R.render_views_fold_host(sph, lg, np.stack([IDENTITY] * 6), 8, 8,
                                        np.ones((3, 8, 8, 2), F), P(3, 2), -4.0, 1.0, 6)
        words = b2.out.cpu().numpy().view(np.uint32)
        assert words[:12].tobytes() == want.tobytes() and (words[12:] == FILL).all()
        scr = b2.scratch.cpu().numpy().view(np.uint32)
        assert (scr[:4] == FILL).all() and (scr[4 + nb // 4:] == FILL).all()
        # the one-shot form, counts and all
        one = R.render_views_fold(sph, lg, np.stack([IDENTITY] * 6), 8, 8, np.ones((3, 8, 8, 2), F),
                                  P(3, 2, SKIP), -4.0, 1.0, 6, skipped=True)
        host = R.render_views_fold_host(sph, lg, np.stack([IDENTITY] * 6), 8, 8,
                                        np.ones((3, 8, 8, 2), F), P(3, 2, SKIP), -4.0, 1.0, 6,
                                        skipped=True)
        assert one[0].tobytes() == host[0].tobytes() and (one[1] == host[1]).all()
        assert (one[0] != 0).any()
    finally:
        ctx.close()


# ---- the driver ----

def test_host_driver_sh(R, tmp_path):
    sph, lg = R.reference_scene()
    exe = [os.path.join(PKG, "rtg_main"), "--scene", os.path.join(ROOT, "scenes", "reference.scene")]
    out = tmp_path / "probe.txt"
    r = subprocess.run(exe + ["--cube", "0,0,-4", "--width", "16", "--aa", "1", "--sh", "3",
                              "--sh-out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([[F(t) for t in line.split()] for line in out.read_text().splitlines()], F)
    want = R.render_views_fold_host(sph, lg, R.camera_cube((0, 0, -4)), 16, 16,
                                    R.cube_sh_weights(16, 3, 1.0), R.fold_params(6, 9), -1.0, 1.0, 6)
    assert got.shape == (9, 3) and got.tobytes() == want[0].tobytes(), (got, want)
    assert (got != 0).any()
    for bad, msg in ((["--cube", "0,0,0", "--sh", "3"], "go together"),
                     (["--cube", "0,0,0", "--sh-out", str(out)], "go together"),
                     (["--sh", "3", "--sh-out", str(out)], "go together"),
                     (["--cube", "0,0,0", "--sh", "5", "--sh-out", str(out)], "Invalid SH band")):
        r = subprocess.run(exe + bad, capture_output=True, text=True, timeout=120)  # no GPU call
        assert r.returncode == 1 and msg in r.stdout, (bad, r.stdout)
