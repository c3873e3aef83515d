"""GPU tests over hostile SCENES (tests/hostile.py) on an MI355X: every device
entry point that reads the scene tables, against the references that
test_hostile_host.py pins on the CPU (the oracle's frames, the plain loops'
hits, visibilities and colours, the host forms of the G-buffer, the ray order
and the posed camera), bit for bit.

One context per base size takes every mutation in turn (set_scene), so it
alternates between scenes with and without masks, sphere lists or a BVH: the
kernels launched with null tables, the scalar loads over NaN records and the
flat queries at n > 64 all run whole frames and batches here, and table
teardown runs between them.  hostile.expect states which path a scene takes;
the BVH half of it is asserted from Context.scene_stats.

Every destination is pre-filled and PAD records longer than its result; the
tail must stay.

The second part feeds the output kernels (max_kernel, ppm_kernel) the hostile
frames and a buffer of special floats at sizes where their grid-stride loops
wrap, against the host forms that test_host.py pins to the oracle.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import hostile
from conftest import bits_equal, first_mismatch
from hostile import CASES, IDS
from raygen import diff_hits
from test_gpu_order import FILL, PAD, _run, _same_as_host, _stream
from test_hostile_host import AA, H, S, W, check_non_vacuous, colours0, oracle_frame, semantics_of, walk0
from test_host import _special_floats
from test_raytrace_host import THREADS

pytestmark = pytest.mark.gpu

CW, CH, CAA = 32, 24, 2.0  # the posed camera's frame and its rays' alias factor


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


def _words(torch, call, n_words):
    """`call(dst_ptr)` into n_words pre-filled int32 words plus PAD; the tail
    must stay."""
    dst = torch.full((n_words + PAD,), FILL, dtype=torch.int32, device="cuda")
    call(dst.data_ptr())
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n_words:] == FILL).all(), "words past the result were written"
    return out[:n_words]


def _frame(torch, ctx, w, h, s, aa, variant=0):
    ctx.set_variant(variant)
    try:
        out = _words(torch, lambda p: ctx.render_device(w, h, p, alias_factor=aa, stack_size=s,
                                                        stream=_stream(torch)), w * h * 3)
    finally:
        ctx.set_variant(0)
    return out.view(np.float32).reshape(h, w, 3)


def _check_frame(got, want, what):
    assert bits_equal(got, want), (what, first_mismatch(got, want))
    assert (got.view(np.uint32)[np.isnan(got)] == 0xFFC00000).all(), (what, "NaN words")


def _sharded(torch, ctx, w, h, s, aa, G=3, B=4):
    from rtg_amd import dist
    rmax = dist.padded_rows(h, B, G)
    buf = torch.zeros((G, rmax, w, 3), dtype=torch.float32, device="cuda")
    for g in range(G):
        ctx.render_device(w, h, buf[g].data_ptr(), alias_factor=aa, stack_size=s, row_block=B,
                          shard=g, n_shards=G, stream=_stream(torch))
    torch.cuda.synchronize()
    return dist.assemble(buf, h, B).cpu().numpy()


def _output_side(R, torch, ctx, fb):
    """max_colour_device and ppm_bytes_device of a frame against the host forms."""
    n = fb.size // 3
    src = torch.from_numpy(np.array(fb, np.float32).reshape(-1)).cuda()
    mx = _words(torch, lambda p: ctx.max_colour_device(src.data_ptr(), n, p, stream=_stream(torch)),
                1)
    want = np.float32(R.max_colour_value(fb))
    assert mx[0] == want.view(np.int32), (mx.view(np.float32)[0], want)
    _ppm(R, torch, ctx, src, fb, want)


def _ppm(R, torch, ctx, src, fb, mx):
    n = fb.size // 3
    d_mx = torch.from_numpy(np.array([mx], np.float32)).cuda()
    out = torch.full((3 * n + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.ppm_bytes_device(src.data_ptr(), n, d_mx.data_ptr(), out.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[3 * n:] == 0x5A).all(), "bytes past the frame were written"
    want = R.ppm_bytes(fb, mx)
    bad = np.flatnonzero(got[:3 * n] != want)
    assert not len(bad), (mx, f"{len(bad)} bytes differ, first {bad[0]}: value "
                          f"{fb.reshape(-1)[bad[0]]!r}: {got[bad[0]]} vs {want[bad[0]]}")


# ---- 1. every mutation, on one context per base size ----

@pytest.mark.parametrize("n,name", CASES, ids=IDS)
def test_hostile_scene(R, oracle, torch_cuda, contexts, n, name):
    torch = torch_cuda
    sph, lg = hostile.mutated(n, name)
    rays, segs = (a.copy() for a in hostile.batches(n))  # (the shared ones are read-only)
    check_non_vacuous(n, name)
    hits, vis = walk0(n, name)
    ctx = contexts(n)
    ctx.set_scene(sph, lg)
    if n > 64:  # which query path the kernels below take (hostile.expect)
        nodes = ctx.scene_stats()["bvh_nodes"]
        assert (nodes == 0) == (hostile.expect(n, name)[1] == "flat"), nodes
        assert (nodes == 0) == (name in hostile.NO_BVH)

    # frames: the sample kernel and the tile kernel
    want = oracle_frame(oracle, n, name)
    for variant in (0, 9):
        got = _frame(torch, ctx, W, H, S, AA, variant)
        _check_frame(got, want, ("variant", variant))
    if name in ("col", "mat", "all"):
        _output_side(R, torch, ctx, got)
    if name == "all":
        for s, aa in ((S, 1.0), (S, 2.5), (S, 9.0), (1, AA), (16, AA)):
            _check_frame(_frame(torch, ctx, W, H, s, aa), oracle_frame(oracle, n, name, s=s, aa=aa),
                         (s, aa))
        _check_frame(_sharded(torch, ctx, W, H, S, AA), want, "3 shards")
        ctx.set_semantics(R.Context.SEMANTICS_OPENCL)
        try:
            _check_frame(_frame(torch, ctx, W, H, 5, AA),
                         oracle_frame(oracle, n, name, s=5, cl=True), "OpenCL semantics")
        finally:
            ctx.set_semantics(R.Context.SEMANTICS_CPU)

    # the G-buffer
    got = _words(torch, lambda p: ctx.gbuffer_device(W, H, p, alias_factor=AA,
                                                     stream=_stream(torch)), W * H * 8)
    want = R.gbuffer_host(sph, W, H, -4.0, AA, threads=THREADS)
    assert got.tobytes() == want.tobytes(), "G-buffer"

    # the ray order, then the batch queries plain and indexed
    d_rays, d_segs = torch.from_numpy(rays).cuda(), torch.from_numpy(segs).cuda()
    o_rays, _ = _same_as_host(R, torch, ctx, sph, rays)
    o_segs, _ = _same_as_host(R, torch, ctx, sph, segs, kind=R.ORDER_SEGMENTS)
    d_or = torch.from_numpy(o_rays.view(np.int32)).cuda()
    d_os = torch.from_numpy(o_segs.view(np.int32)).cuda()
    for label, o_r, o_s in (("plain", None, None), ("indexed", d_or, d_os)):
        got = _run(torch, ctx.intersect_device, d_rays, len(rays), 8, o_r)
        assert got.tobytes() == hits.tobytes(), (label, diff_hits(got.view(R.HIT_DTYPE), hits))
        got = _run(torch, ctx.visible_device, d_segs, len(segs), 0, o_s)
        bad = np.flatnonzero(got != vis)
        assert not len(bad), (label, f"{len(bad)} segments differ, first {bad[0]}")
        for sem in semantics_of(name):
            ctx.set_semantics(sem)
            try:
                got = _run(torch, functools.partial(ctx.raytrace_device, stack_size=S), d_rays,
                           len(rays), 3, o_r)
            finally:
                ctx.set_semantics(R.Context.SEMANTICS_CPU)
            want = colours0(n, name, S, sem)
            assert got.tobytes() == want.tobytes(), (
                label, sem, first_mismatch(got.view(np.float32).reshape(-1, 3), want))

    # the posed camera
    if n > 64:
        cam = R.camera_look_at(*hostile.POSE)
        got = _words(torch, lambda p: ctx.render_camera(cam, CW, CH, p, stack_size=S,
                                                        stream=_stream(torch)), CW * CH * 3)
        want = R.render_camera_host(sph, lg, cam, CW, CH, stack_size=S, walk=0, threads=THREADS)
        assert got.tobytes() == want.tobytes(), (
            "camera", first_mismatch(got.view(np.float32).reshape(CH, CW, 3), want))
        host_rays = R.camera_rays_host(cam, CW, CH, alias_factor=CAA, threads=THREADS)
        k = len(host_rays)
        d_cam = torch.full(((k + PAD) * 6,), FILL, dtype=torch.int32, device="cuda")
        ctx.camera_rays(cam, CW, CH, d_cam.data_ptr(), alias_factor=CAA, stream=_stream(torch))
        got = _run(torch, ctx.intersect_device, d_cam, k, 8, None)
        assert (d_cam.cpu().numpy()[6 * k:] == FILL).all(), "rays past the frame were written"
        want = R.intersect_host(sph, host_rays, walk=0, threads=THREADS)
        assert got.tobytes() == want.tobytes(), ("camera rays",
                                                 diff_hits(got.view(R.HIT_DTYPE), want))
        assert (want["id"] >= 0).any()


def test_large_scene(R, oracle, torch_cuda):
    """1100 spheres with a NaN centre: global materials, no BVH, flat queries."""
    torch = torch_cuda
    n = hostile.LARGE_N
    sph, lg = hostile.mutated(n, "cnan")
    rays, segs = hostile.batches(n)
    check_non_vacuous(n, "cnan")
    hits, vis = walk0(n, "cnan")
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        assert ctx.scene_stats()["bvh_nodes"] == 0
        _check_frame(_frame(torch, ctx, 24, 14, 4, AA), oracle_frame(oracle, n, "cnan", 24, 14, 4),
                     "large")
        d_rays = torch.from_numpy(rays.copy()).cuda()
        d_segs = torch.from_numpy(segs.copy()).cuda()
        got = _run(torch, ctx.intersect_device, d_rays, len(rays), 8, None)
        assert got.tobytes() == hits.tobytes(), diff_hits(got.view(R.HIT_DTYPE), hits)
        got = _run(torch, ctx.visible_device, d_segs, len(segs), 0, None)
        assert (got == vis).all()
        got = _run(torch, functools.partial(ctx.raytrace_device, stack_size=4), d_rays, len(rays),
                   3, None)
        assert got.tobytes() == colours0(n, "cnan", 4).tobytes()
    finally:
        ctx.close()


# ---- 2. the output side ----

PIXELS = (1, 85, 86, 349527)  # 255 and 258 values; above 4096 x 256 values: both loops wrap
MAXES = (6.955025e-05, 1.0, 1e-30, 2.5, 7e-41, np.inf, np.nan)


@functools.lru_cache(maxsize=None)
def _specials():
    v = _special_floats(np.random.default_rng(12), 3 * PIXELS[-1])
    # the special values again past the first wrap of the max kernel's loop
    # (2048 x 256 values) and in the last, partial stride of the ppm kernel's
    v[2048 * 256 + 5:2048 * 256 + 5 + 16] = v[:16]
    v[-3:] = (3e38, np.nan, -np.inf)
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("pixels", PIXELS)
def test_output_kernels_on_special_floats(R, torch_cuda, pixels):
    torch = torch_cuda
    assert 3 * PIXELS[-1] > 4096 * 256
    # a prefix of the buffer; the one-pixel case is (+inf, -inf, 1.0)
    base = (_specials()[4:7] if pixels == 1 else _specials()[:3 * pixels]).copy()
    assert (base == np.inf).any()
    finite = base.copy()
    finite[np.isinf(finite)] = 0
    buffers = {"as is": base, "no inf": finite,
               "NaN": np.full(3 * pixels, np.nan, np.float32),
               "negative": -np.abs(finite) - np.float32(1),
               "-0": np.full(3 * pixels, -0.0, np.float32),
               "subnormal": np.full(3 * pixels, 7e-41, np.float32)}
    assert 0 < buffers["subnormal"][0] < np.finfo(np.float32).tiny
    ctx = R.Context(0)
    try:
        for label, buf in buffers.items():
            fb = buf.reshape(-1, 3)
            src = torch.from_numpy(buf).cuda()
            mx = _words(torch, lambda p: ctx.max_colour_device(src.data_ptr(), pixels, p,
                                                               stream=_stream(torch)), 1)
            want = np.float32(R.max_colour_value(fb))
            assert mx[0] == want.view(np.int32), (label, mx.view(np.float32)[0], want)
        assert R.max_colour_value(base.reshape(-1, 3)) == np.inf
        assert np.float32(R.max_colour_value(buffers["subnormal"].reshape(-1, 3))) == np.float32(7e-41)
        src = torch.from_numpy(base).cuda()
        for mx in MAXES:
            _ppm(R, torch, ctx, src, base.reshape(-1, 3), np.float32(mx))
    finally:
        ctx.close()
