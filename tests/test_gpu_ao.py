"""GPU tests of ambient occlusion (rtg_ao*, include/rtg.h) on an MI355X, against
the references test_ao_host.py pins on the CPU (aogen.py: the plain loops'
counts and the host generator's segments), bit for bit.

Every destination is pre-filled and PAD records longer than its result; the
tail must stay.

  1. the fused kernel == ao_host(walk 0) and segments_device == segments_host,
     for 1, 63, 64, 65 and 200 points, every (K, nDirs) of aogen.PROBES, jitter
     off and on (seed + i wraps), on every scene of the CPU walk-1 list, one
     context per scene;
  2. every hostile scene (hostile.CASES), one context per size taking the
     mutations in turn;
  3. the one-shot form, and a launch on a stream of its own;
  4. rtg_main --ao;
  5. the device entry points' argument checks.
"""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import aogen
import hostile
from aogen import SCENES, SETS
from conftest import PKG, ROOT
from hostile import CASES, IDS
from test_gpu_order import PAD, _stream
from test_raytrace_host import THREADS

pytestmark = pytest.mark.gpu

FILL16 = 0x5A5A
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


def _dev(torch, a):
    """A host array on the device as int32 words."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).cuda()


def _counts(torch, ctx, d_hits, n, p, d_dirs, nd, stream=None):
    dst = torch.full((n + PAD,), FILL16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()  # the fill, before a launch on another stream
    ctx.ao_device(d_hits.data_ptr(), n, p, d_dirs.data_ptr(), nd, dst.data_ptr(),
                  stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint16)
    assert (out[n:] == FILL16).all(), "counts past the batch were written"
    return out[:n]


def _segments(torch, ctx, d_hits, n, p, d_dirs, nd):
    k = int(p["samples"][0])
    dst = torch.full(((n * k + PAD) * 6,), FILL32, dtype=torch.int32, device="cuda")
    ctx.ao_segments_device(d_hits.data_ptr(), n, p, d_dirs.data_ptr(), nd, dst.data_ptr(),
                           stream=_stream(torch))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n * k * 6:] == FILL32).all(), "segments past the batch were written"
    return out[:n * k * 6].view(np.float32).reshape(n * k, 6)


def _first_bad(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return None if not len(bad) else f"{len(bad)} differ, first at {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


# ---- 1. every path, size and parameter set ----

@pytest.mark.parametrize("name", SCENES)
def test_device_equals_plain_loops(R, torch_cuda, name):
    torch = torch_cuda
    aogen.assert_non_vacuous(name)  # on the walk-0 answer
    sph = aogen.scene(name)
    d_hits = _dev(torch, aogen.hits(name))
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, hostile.base(8)[1])
        nodes = ctx.scene_stats()["bvh_nodes"]
        assert (nodes > 0) == (aogen.PATHS[name] == "bvh"), nodes
        for k, nd, flags in SETS:
            p = aogen.params(R, name, k, flags)
            d_dirs = _dev(torch, aogen.dirs(nd))
            want = aogen.want(name, k, nd, flags)
            want_segs = aogen.want_segments(name, k, nd, flags)
            for n in aogen.SIZES:
                got = _counts(torch, ctx, d_hits, n, p, d_dirs, nd)
                assert got.tobytes() == want[:n].tobytes(), (k, nd, flags, n,
                                                             _first_bad(got, want[:n]))
                got = _segments(torch, ctx, d_hits, n, p, d_dirs, nd)
                assert got.tobytes() == want_segs[:n * k].tobytes(), (k, nd, flags, n)
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


@functools.lru_cache(maxsize=None)
def _hostile_radius(n):
    return float(np.float32(2.5 * np.abs(hostile.base(n)[0]["radius"]).max()))


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
    d_hits, d_dirs = _dev(torch, h), _dev(torch, aogen.dirs(8))
    for flags in (0, 1):
        p = R.ao_params(7, _hostile_radius(n), aogen.BIAS, aogen.SEED, flags)
        want = R.ao_host(sph, h, aogen.dirs(8), p, walk=0, threads=THREADS)
        got = _counts(torch, ctx, d_hits, len(h), p, d_dirs, 8)
        assert got.tobytes() == want.tobytes(), (flags, _first_bad(got, want))


# ---- 3. the one-shot form and a stream of its own ----

def test_one_shot_and_streams(R, torch_cuda):
    torch = torch_cuda
    for name, (k, nd, flags) in (("reference", (7, 8, 1)), ("base150", (64, 97, 0))):
        sph, h = aogen.scene(name), aogen.hits(name)
        p = aogen.params(R, name, k, flags)
        want = aogen.want(name, k, nd, flags)
        assert R.ao(sph, h, aogen.dirs(nd), p).tobytes() == want.tobytes(), name
        d_hits, d_dirs = _dev(torch, h), _dev(torch, aogen.dirs(nd))
        ctx = R.Context(0)
        try:
            ctx.set_scene(sph, hostile.base(8)[1])
            own = torch.cuda.Stream()
            got = _counts(torch, ctx, d_hits, len(h), p, d_dirs, nd, stream=own.cuda_stream)
            assert got.tobytes() == want.tobytes(), (name, "own stream")
            got = _counts(torch, ctx, d_hits, len(h), p, d_dirs, nd, stream=0)
            assert got.tobytes() == want.tobytes(), (name, "default stream")
        finally:
            ctx.close()
    assert R.ao(sph, np.zeros(0, R.HIT_DTYPE), aogen.dirs(8), R.ao_params(7, 1.0)).shape == (0,)


# ---- 4. the driver ----

def _chain(R, torch, sph, lg, cam, W, H, p, table):
    """camera_rays -> intersect_device -> ao_device through the binding."""
    n = W * H
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        ctx.camera_rays(cam, W, H, rays.data_ptr(), alias_factor=1.0, stream=_stream(torch))
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream=_stream(torch))
        return _counts(torch, ctx, hits, n, p, _dev(torch, table), len(table))
    finally:
        ctx.close()


def test_host_driver_ao_option(R, torch_cuda, tmp_path):
    torch = torch_cuda
    scene_file = os.path.join(ROOT, "scenes", "reference.scene")
    sph, lg = R.load_scene_file(scene_file)
    W, H, K = 48, 36, 16
    base = [os.path.join(PKG, "rtg_main"), "--scene", scene_file, "--width", str(W), "--height",
            str(H), "--out", str(tmp_path / "frame.ppm")]
    table = R.ao_directions(K)
    for spec, p, cam in (("16,12.5", R.ao_params(K, 12.5), R.camera_identity()),
                         ("16,12.5,0.01,77", R.ao_params(K, 12.5, 0.01, 77, R.AO_JITTER),
                          R.camera_look_at((3, 2, -1), (0, 0, -10)))):
        pgm = str(tmp_path / "ao.pgm")
        extra = [] if spec == "16,12.5" else ["--camera", "3,2,-1,0,0,-10"]
        r = subprocess.run(base + ["--ao", spec, "--ao-out", pgm] + extra, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        counts = _chain(R, torch, sph, lg, cam, W, H, p, table)
        assert 0 < int((counts < K).sum()) < W * H  # some pixels occluded, some open
        want = b"P5\n%d %d\n255\n" % (W, H) + ((255 * counts.astype(np.uint32)) // K).astype(
            np.uint8).tobytes()
        assert open(pgm, "rb").read() == want, spec
    for bad in (["--ao", "16"], ["--ao", "0,1"], ["--ao", "16,1,0,1,9"], ["--ao", "16,1"],
                ["--ao-out", "x.pgm"]):  # usage errors: no GPU call
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("Invalid ao" in r.stdout or "go together" in r.stdout), r.stdout


# ---- 5. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    h = aogen.hits("reference")
    d_hits, d_dirs = _dev(torch, h), _dev(torch, aogen.dirs(8))
    out = torch.zeros((len(h) + PAD,), dtype=torch.int16, device="cuda")
    segs = torch.zeros(((len(h) * 7 + PAD) * 6,), dtype=torch.int32, device="cuda")
    ok = R.ao_params(7, 1.0)
    ctx = R.Context(0)
    try:
        with pytest.raises(R.RtgError, match="scene"):  # no scene yet (the fused call only)
            ctx.ao_device(d_hits.data_ptr(), len(h), ok, d_dirs.data_ptr(), 8, out.data_ptr())
        ctx.ao_segments_device(d_hits.data_ptr(), len(h), ok, d_dirs.data_ptr(), 8, segs.data_ptr())
        torch.cuda.synchronize()
        assert int(segs.count_nonzero()) > 0
        segs.zero_()
        ctx.set_scene(aogen.scene("reference"), hostile.base(8)[1])
        hp, dp, op, sp = d_hits.data_ptr(), d_dirs.data_ptr(), out.data_ptr(), segs.data_ptr()
        for call, dst in ((ctx.ao_device, op), (ctx.ao_segments_device, sp)):
            for a, msg in (((0, 8, ok, dp, 8, dst), "null hit buffer"),
                           ((hp, 8, ok, 0, 8, dst), "null direction table"),
                           ((hp, 8, ok, dp, 8, 0), "null output buffer"),
                           ((hp, 8, R.ao_params(0, 1.0), dp, 8, dst), "0 samples"),
                           ((hp, 8, R.ao_params(1025, 1.0), dp, 2000, dst), "1025 samples"),
                           ((hp, 8, ok, dp, 6, dst), "6 directions"),
                           ((hp, 8, ok, dp, 65537, dst), "65537 directions"),
                           ((hp, 8, R.ao_params(7, 1.0, flags=4), dp, 8, dst), "unknown flags 0x4"),
                           ((hp, 1 << 32, ok, dp, 8, dst), "at most 2\\^32 - 1")):
                with pytest.raises(R.RtgError, match=msg):
                    call(*a)
            call(hp, 0, ok, dp, 8, dst)  # an empty batch: RTG_OK, no launch
        with pytest.raises(R.RtgError, match="overflows size_t"):
            ctx.ao_segments_device(hp, 1 << 62, R.ao_params(1024, 1.0), dp, 1024, sp)
        with pytest.raises(R.RtgError, match="too large"):  # 2^42 lanes: above 2^31-1 workgroups
            ctx.ao_segments_device(hp, (1 << 32) - 1, R.ao_params(1024, 1.0), dp, 1024, sp)
        L = R.lib()
        assert L.rtg_ao_device(ctx._h, hp, 8, None, dp, 8, op, None) == -1
        assert b"null params" in L.rtg_last_error()
        assert L.rtg_ao_segments_device(None, hp, 8, R._ptr(ok), dp, 8, sp, None) == -1
        assert b"no context" in L.rtg_last_error()
        torch.cuda.synchronize()
        assert int(out.count_nonzero()) == 0 and int(segs.count_nonzero()) == 0  # nothing launched
    finally:
        ctx.close()
