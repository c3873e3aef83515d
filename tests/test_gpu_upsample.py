"""GPU tests of the guided upsampling (rtg_upsample*, rtg_hits_pick*,
rtg_values_place*; include/rtg.h, "upsample") on an MI355X, against the host
loops' words test_upsample_host.py pins on the CPU, word for word.

dst, holes and holeCount are pre-filled and dst and holes PAD words longer than
the call needs; the tails, and the list's entries past min(count, cap), must
stay.

  1. upsample_device == upsample_host (dst, list, count) on 48 x 32 at
     L = 1, 2, 3 and on the frames that cross a wave or are smaller than one,
     three kinds, flag sets none / SAME_ID / all, with and without the list,
     a capacity below the count; and on a frame of 3000 workgroups, more than
     one step of the scan over their counts;
  2. hostile guides and values: NaN and infinite points and normals, ids >=
     sphNum, a frame of background, a low frame of background under a frame of
     hits, non-finite low values with and without SKIP_NONFINITE;
  3. calling forms: two runs, a stream of its own between two renders, a
     context without a scene (every test), the one-shot form;
  4. pick and place against the host forms, an index >= n among them;
  5. the chain on c5 at 96 x 64, L = 1, device against host;
  6. rtg_main --ao ... --ao-scale 1 against that chain's bytes;
  7. the device entry points' argument checks, nothing launched.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import aogen
import upgen as U
from conftest import PKG, ROOT
from test_gpu_order import PAD, _stream
from test_raytrace_host import THREADS, scene_with_lights

pytestmark = pytest.mark.gpu

F = np.float32
FILL = U.FILL
# (W, H, L): the 48 x 32 frame; a low width of 65, so a row crosses the wave
# boundary with an odd low row; one low pixel under 2 x 2 and under 8 x 8; a
# low frame one row high under two full rows of two waves
SHAPES = [(48, 32, 1), (48, 32, 2), (48, 32, 3), (130, 6, 1), (2, 2, 1), (8, 8, 3), (128, 2, 1)]
FLAG_SETS = (0, U.SAME_ID, U.ALL)


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
    c = R.Context(0)  # no scene: none of the calls needs one
    yield c
    c.close()


def _dev(torch, a):
    """A host array on the device as bytes, 16-byte aligned."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _upsample(torch, R, ctx, d_hits, W, H, L, p, d_low, d_src, cap=None, stream=None):
    """Context.upsample_device into pre-filled outputs: (dst words, list of `cap`
    entries, count), the list parts None when cap is None."""
    words = W * H * (3 if int(p["kind"][0]) == R.FILTER_RGB else 1)
    dst = torch.full((words + PAD,), FILL, dtype=torch.int32, device="cuda")
    lst = cnt = scratch = None
    nbytes = 0
    if cap is not None:
        lst = torch.full((cap + PAD,), FILL, dtype=torch.int32, device="cuda")
        cnt = torch.full((1 + PAD,), FILL, dtype=torch.int32, device="cuda")
        nbytes = R.upsample_scratch(W, H, True)
        scratch = torch.full((nbytes // 4 + PAD,), FILL, dtype=torch.int32, device="cuda")
    assert R.upsample_scratch(W, H, False) == 0
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    ctx.upsample_device(d_hits.data_ptr(), W, H, p, d_low.data_ptr(), W >> L, H >> L,
                        d_src.data_ptr(), dst.data_ptr(),
                        holes_ptr=lst.data_ptr() if cap is not None else 0, hole_cap=cap or 0,
                        hole_count_ptr=cnt.data_ptr() if cap is not None else 0,
                        scratch_ptr=scratch.data_ptr() if cap is not None else 0,
                        scratch_bytes=nbytes, stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    dst = dst.cpu().numpy().view(np.uint32)
    assert (dst[words:] == FILL).all(), "words past the frame were written"
    if cap is None:
        return dst[:words], None, None
    lst, cnt = lst.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    scratch = scratch.cpu().numpy().view(np.uint32)
    assert (lst[cap:] == FILL).all() and (cnt[1:] == FILL).all(), "the list's tail was written"
    assert (scratch[nbytes // 4:] == FILL).all(), "words past the scratch were written"
    return dst[:words], lst[:cap], int(cnt[0])


def _check(got, want, cap, what):
    words, holes, count = want
    bad = np.flatnonzero(got[0] != words)
    assert not len(bad), (what, f"{len(bad)} words differ, first at {bad[0]}: "
                          f"{got[0][bad[0]]:#x} vs {words[bad[0]]:#x}")
    if cap is None:
        return
    k = min(count, cap)
    assert got[2] == count, (what, got[2], count)
    assert (got[1][:k] == holes[:k]).all(), (what, "the list differs")
    assert (got[1][k:] == FILL).all(), (what, "entries past min(count, cap) were written")


def _host(R, full, low, W, H, L, p, src):
    out, lst, cnt = R.upsample_host(full, W, H, p, low, W >> L, H >> L, src, holes=W * H,
                                    threads=THREADS)
    return out.view(np.uint32).reshape(-1), lst[:cnt], cnt


# ---- 1. every shape, kind and flag set, with and without the list ----

@pytest.mark.parametrize("name", U.SCENES)
def test_device_equals_host(R, torch_cuda, ctx, name):
    torch = torch_cuda
    holes_seen = 0
    for W, H, L in SHAPES:
        full, low = U.frames(name, W, H, L)
        d_hits, d_low = _dev(torch, full), _dev(torch, low)
        for signal in U.SIGNALS:
            src = U.low_signal(name, W >> L, H >> L, signal)
            d_src = _dev(torch, src)
            for flags in FLAG_SETS:
                p = U.params(R, name, signal, L, flags)
                want = U.want(name, W, H, L, signal, flags) if (W, H) == U.FULL else \
                    _host(R, full, low, W, H, L, p, src)
                holes_seen += want[2]
                caps = [None, W * H] + ([want[2] - 1] if want[2] > 1 else []) + \
                    ([0] if flags == U.ALL else [])
                for cap in caps:
                    got = _upsample(torch, R, ctx, d_hits, W, H, L, p, d_low, d_src, cap)
                    _check(got, want, cap, (name, W, H, L, signal, flags, cap))
    assert holes_seen > 0


def test_more_workgroups_than_one_scan_step(R, torch_cuda, ctx):
    """1200 x 640 pixels are 3000 workgroups: the scan over their counts takes
    three steps of 1024, the last one partial, and carries its sum across them;
    1200 is no multiple of 64, so waves end one row and begin the next.  A third
    of the low ids is changed by hand, so holes lie in every part of the frame
    and the list is long (53614 entries)."""
    torch = torch_cuda
    name, W, H, L = "reference", 1200, 640, 1
    full = U.records(name, W, H)
    low = U.records(name, W >> L, H >> L).copy()
    rng = np.random.default_rng(31)
    moved = (rng.random(len(low)) < 1 / 3) & (low["id"] >= 0)
    low["id"][moved] += 7
    src = low["t"].astype(F)
    p = U.params(R, name, "gray", L, U.GEOM)
    want = _host(R, full, low, W, H, L, p, src)
    n, count = W * H, want[2]
    groups = (n + 255) // 256
    assert groups > 2048 and groups % 1024 and count > 20000
    spread = np.bincount(want[1] // 256 // 1024, minlength=3)
    assert (spread > 1000).all(), spread  # every step of the scan carries holes
    d_hits, d_low, d_src = _dev(torch, full), _dev(torch, low), _dev(torch, src)
    for cap in (n, count - 1, None):
        got = _upsample(torch, R, ctx, d_hits, W, H, L, p, d_low, d_src, cap)
        _check(got, want, cap, ("many workgroups", cap))


# ---- 2. hostile guides and values ----

def test_hostile_guides_and_values(R, torch_cuda, ctx):
    torch = torch_cuda
    W, H = U.FULL
    for name in U.SCENES:
        for L in (1, 3):
            full, low = U.frames(name, W, H, L, True)
            assert not np.isfinite(full["point"]).all() and (full["id"] == 1 << 30).any()
            d_hits, d_low = _dev(torch, full), _dev(torch, low)
            for signal in ("rgb", "gray"):
                src = U.low_signal(name, W >> L, H >> L, signal, True)
                assert not np.isfinite(src).all()
                d_src = _dev(torch, src)
                for flags, nl, scale in ((0, 0, 0.0), (U.ALL, 3, None), (U.SKIP, 0, 0.0),
                                         (U.GEOM, 8, None), (U.PLANE, 0, float("inf")),
                                         (U.PLANE, 0, float("nan"))):
                    sc = U.plane_scale(name) if scale is None else scale
                    p = U.params(R, name, signal, L, flags, sc, nl)
                    want = _host(R, full, low, W, H, L, p, src)
                    got = _upsample(torch, R, ctx, d_hits, W, H, L, p, d_low, d_src, W * H)
                    _check(got, want, W * H, (name, L, signal, flags, nl, scale))
    # a frame of background; a low frame of background under a frame of hits
    name, L = "c5", 2
    full, low = U.frames(name, W, H, L)
    src = U.low_signal(name, W >> L, H >> L, "rgb")
    p = U.params(R, name, "rgb", L, U.GEOM)
    none, lnone = full.copy(), low.copy()
    none["id"], lnone["id"] = -1, -1
    for f_, l_, count in ((none, low, 0), (none, lnone, 0), (full, lnone, int((full["id"] >= 0).sum()))):
        want = _host(R, f_, l_, W, H, L, p, src)
        assert want[2] == count and not want[0].any()  # every hit pixel is a hole; dst is +0
        got = _upsample(torch, R, ctx, _dev(torch, f_), W, H, L, p, _dev(torch, l_),
                        _dev(torch, src), W * H)
        _check(got, want, W * H, "background")


# ---- 3. calling forms ----

def test_two_runs_and_own_stream_between_renders(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    W, H = U.FULL
    name, L, signal = "c5", 2, "count"
    full, low = U.frames(name, W, H, L)
    d_hits, d_low = _dev(torch, full), _dev(torch, low)
    d_src = _dev(torch, U.low_signal(name, W >> L, H >> L, signal))
    p = U.params(R, name, signal, L, U.GEOM)
    want = U.want(name, W, H, L, signal, U.GEOM)
    c = R.Context(0)
    try:
        c.set_scene(sph, lg)
        fb = [torch.zeros((48 * 36 * 3,), dtype=torch.float32, device="cuda") for _ in range(2)]
        own = torch.cuda.Stream()
        c.render_device(48, 36, fb[0].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        a = _upsample(torch, R, c, d_hits, W, H, L, p, d_low, d_src, W * H, stream=own.cuda_stream)
        c.render_device(48, 36, fb[1].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        b = _upsample(torch, R, c, d_hits, W, H, L, p, d_low, d_src, W * H, stream=own.cuda_stream)
        torch.cuda.synchronize()
        _check(a, want, W * H, "first run")
        _check(b, want, W * H, "second run")
        assert a[1].tobytes() == b[1].tobytes() and want[2] > 1
        x, y = fb[0].cpu().numpy(), fb[1].cpu().numpy()
        assert (x != 0).any() and U.canon(x).tobytes() == U.canon(y).tobytes()
    finally:
        c.close()


def test_one_shot(R, torch_cuda):
    W, H = U.FULL
    for name, L, signal, flags in (("reference", 1, "count", U.GEOM), ("c5", 3, "rgb", U.ALL),
                                   ("c5", 2, "gray", 0)):
        full, low = U.frames(name, W, H, L)
        src = U.low_signal(name, W >> L, H >> L, signal)
        p = U.params(R, name, signal, L, flags)
        want = U.want(name, W, H, L, signal, flags)
        out = R.upsample(full, W, H, p, low, W >> L, H >> L, src)
        assert out.shape == ((H, W, 3) if signal == "rgb" else (H, W))
        assert out.view(np.uint32).reshape(-1).tobytes() == want[0].tobytes()
        for cap in (W * H, max(want[2] - 1, 0), 0):
            lst = np.full(cap, FILL, np.uint32)
            out, lst, cnt = R.upsample(full, W, H, p, low, W >> L, H >> L, src, holes=lst)
            _check((out.view(np.uint32).reshape(-1), lst, cnt), want, cap, (name, L, cap))


# ---- 4. pick and place ----

def test_pick_and_place(R, torch_cuda, ctx):
    torch = torch_cuda
    W, H = U.FULL
    h = U.frames("c5", W, H, 1, True)[0]
    n = len(h)
    rng = np.random.default_rng(78)
    d_hits = _dev(torch, h)
    for m in (1, 63, 257, 700):
        idx = rng.permutation(n)[:m].astype(np.uint32)
        if m > 3:
            idx[[1, m // 2, m - 1]] = (n, n + 9, 0xFFFFFFFF)
        d_idx = _dev(torch, idx)
        out = torch.full((8 * (m + PAD),), FILL, dtype=torch.int32, device="cuda")
        ctx.hits_pick_device(d_hits.data_ptr(), n, d_idx.data_ptr(), m, out.data_ptr(),
                             stream=_stream(torch))
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert (got[8 * m:] == FILL).all(), "records past the list were written"
        assert got[:8 * m].tobytes() == R.hits_pick_host(h, idx).tobytes(), m
        for kind, C, dt in ((R.FILTER_RGB, 3, F), (R.FILTER_GRAY, 1, F), (R.FILTER_COUNT, 1, np.uint16)):
            vals = rng.integers(0, 60000, size=(m, C)).astype(dt)
            if dt is F:
                vals[0, 0] = np.nan
                vals.view(np.uint32)[m - 1, C - 1] = 0x7FA00001
            want = np.full((n, C), 9.0, F)
            R.values_place_host(kind, vals, idx, want)
            dst = torch.full((n * C + PAD,), 9.0, dtype=torch.float32, device="cuda")
            d_vals = _dev(torch, vals)
            ctx.values_place_device(kind, d_vals.data_ptr(), d_idx.data_ptr(), m, n, dst.data_ptr(),
                                    stream=_stream(torch))
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            assert (got[n * C:] == 9.0).all()
            assert got[:n * C].view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (m, kind)
    # m == 0: nothing is launched
    ctx.hits_pick_device(d_hits.data_ptr(), n, d_idx.data_ptr(), 0, out.data_ptr())
    ctx.values_place_device(R.FILTER_GRAY, d_vals.data_ptr(), d_idx.data_ptr(), 0, n, dst.data_ptr())


# ---- 5. the chain ----

CHAIN = dict(name="c5", W=96, H=64, L=1, K=8, pose=((0.0, 0.0, -2.0), (0.0, 0.0, -12.0)))


def _host_chain(R, sph, cam, W, H, L, K, radius, bias, seed, plane_scale, normal_log2, ao_flags):
    """(float frame, holes) of the mixed-resolution AO through the host forms."""
    table = R.ao_directions(K)
    ap = R.ao_params(K, radius, bias, seed, ao_flags)
    full = R.intersect_host(sph, R.camera_rays_host(cam, W, H, alias_factor=1.0), walk=0,
                            threads=THREADS)
    low = R.intersect_host(sph, R.camera_rays_host(cam, W >> L, H >> L, alias_factor=1.0), walk=0,
                           threads=THREADS)
    counts = R.ao_host(sph, low, table, ap, walk=0, threads=THREADS)
    p = R.upsample_params(L, R.FILTER_COUNT, U.GEOM, plane_scale, normal_log2)
    out, lst, cnt = R.upsample_host(full, W, H, p, low, W >> L, H >> L, counts, holes=W * H,
                                    threads=THREADS)
    out = np.ascontiguousarray(out.reshape(-1))
    if cnt:
        picked = R.hits_pick_host(full, lst[:cnt], threads=THREADS)
        own = R.ao_host(sph, picked, table, ap, walk=0, threads=THREADS)
        R.values_place_host(R.FILTER_COUNT, own, lst[:cnt], out, threads=THREADS)
    return out, lst[:cnt]


def test_device_chain_equals_host_chain(R, torch_cuda):
    torch = torch_cuda
    name, W, H, L, K = (CHAIN[k] for k in ("name", "W", "H", "L", "K"))
    n, nl = W * H, (W >> L) * (H >> L)
    sph = aogen.scene(name)
    cam = R.camera_look_at(*CHAIN["pose"])
    radius, sc = aogen.radius(name), U.plane_scale(name)
    want, holes = _host_chain(R, sph, cam, W, H, L, K, radius, aogen.BIAS, 5, sc, 3, R.AO_JITTER)
    assert 0 < len(holes) < n // 2 and (want != 0).any()
    ap = R.ao_params(K, radius, aogen.BIAS, 5, R.AO_JITTER)
    p = R.upsample_params(L, R.FILTER_COUNT, U.GEOM, sc, 3)
    c = R.Context(0)
    try:
        c.set_scene(sph, scene_with_lights(name)[1])
        s = _stream(torch)
        d_dirs = _dev(torch, R.ao_directions(K))
        d_rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        d_hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        d_low = torch.empty((nl, 8), dtype=torch.int32, device="cuda")
        d_counts = torch.empty((nl,), dtype=torch.int16, device="cuda")
        d_out = torch.full((n + PAD,), FILL, dtype=torch.int32, device="cuda")
        d_list = torch.full((n + PAD,), FILL, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((1,), FILL, dtype=torch.int32, device="cuda")
        nbytes = R.upsample_scratch(W, H, True)
        d_scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
        c.camera_rays(cam, W >> L, H >> L, d_rays.data_ptr(), alias_factor=1.0, stream=s)
        c.intersect_device(d_rays.data_ptr(), nl, d_low.data_ptr(), stream=s)
        c.camera_rays(cam, W, H, d_rays.data_ptr(), alias_factor=1.0, stream=s)
        c.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=s)
        c.ao_device(d_low.data_ptr(), nl, ap, d_dirs.data_ptr(), K, d_counts.data_ptr(), stream=s)
        c.upsample_device(d_hits.data_ptr(), W, H, p, d_low.data_ptr(), W >> L, H >> L,
                          d_counts.data_ptr(), d_out.data_ptr(), d_list.data_ptr(), n,
                          d_cnt.data_ptr(), d_scratch.data_ptr(), nbytes, stream=s)
        m = int(d_cnt.cpu().numpy().view(np.uint32)[0])  # the 4-byte copy back
        assert m == len(holes)
        d_picked = torch.empty((m, 8), dtype=torch.int32, device="cuda")
        d_own = torch.empty((m,), dtype=torch.int16, device="cuda")
        c.hits_pick_device(d_hits.data_ptr(), n, d_list.data_ptr(), m, d_picked.data_ptr(), stream=s)
        c.ao_device(d_picked.data_ptr(), m, ap, d_dirs.data_ptr(), K, d_own.data_ptr(), stream=s)
        c.values_place_device(R.FILTER_COUNT, d_own.data_ptr(), d_list.data_ptr(), m, n,
                              d_out.data_ptr(), stream=s)
        torch.cuda.synchronize()
        out, lst = d_out.cpu().numpy().view(np.uint32), d_list.cpu().numpy().view(np.uint32)
        assert (out[n:] == FILL).all() and (lst[m:] == FILL).all()
        assert (lst[:m] == holes).all()
        assert out[:n].tobytes() == want.view(np.uint32).tobytes()
    finally:
        c.close()


# ---- 6. the driver ----

def _pgm_of(v, K, W, H):
    x = F(255) * v.reshape(-1).astype(F) / F(K)
    x = np.where(x > 0, np.where(x < 255, x, F(255)), F(0))
    return b"P5\n%d %d\n255\n" % (W, H) + x.astype(np.uint8).tobytes()


def test_host_driver_scale_options(R, torch_cuda, tmp_path):
    scene_file = os.path.join(ROOT, "scenes", "reference.scene")
    sph, lg = R.load_scene_file(scene_file)
    W, H, K = 48, 36, 8
    base = [os.path.join(PKG, "rtg_main"), "--scene", scene_file, "--width", str(W), "--height",
            str(H), "--out", str(tmp_path / "frame.ppm"), "--camera", "3,2,-1,0,0,-10"]
    cam = R.camera_look_at((3, 2, -1), (0, 0, -10))
    out = str(tmp_path / "ao.pgm")

    def run(extra, code=0):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == code, r.stdout + r.stderr
        return r.stdout

    seen = set()
    for spec, scale, nl in (("1", 1.0, 3), ("2,4,2", 4.0, 2)):
        L = int(spec[0])
        want, holes = _host_chain(R, sph, cam, W, H, L, K, 12.5, 1e-3, 5, scale, nl, R.AO_JITTER)
        text = run(["--ao", "8,12.5,0.001,5", "--ao-out", out, "--ao-scale", spec])
        assert f"on {len(holes)} holes" in text, text
        assert open(out, "rb").read() == _pgm_of(want, K, W, H), spec
        seen.add(_pgm_of(want, K, W, H))
    run(["--ao", "8,12.5,0.001,5", "--ao-out", out])  # the full-resolution frame is another one
    seen.add(open(out, "rb").read())
    assert len(seen) == 3
    # the upsampled frame goes on through the filter as floats
    want, _ = _host_chain(R, sph, cam, W, H, 1, K, 12.5, 1e-3, 5, 1.0, 3, R.AO_JITTER)
    full = R.intersect_host(sph, R.camera_rays_host(cam, W, H, alias_factor=1.0), walk=0,
                            threads=THREADS)
    flags = R.FILTER_SAME_ID | R.FILTER_NORMAL | R.FILTER_PLANE
    sm = R.filter_host(full, W, H, R.filter_params(2, R.FILTER_GRAY, flags, 0.5, 3), want)
    run(["--ao", "8,12.5,0.001,5", "--ao-out", out, "--ao-scale", "1", "--ao-filter", "2,0.5"])
    assert open(out, "rb").read() == _pgm_of(sm, K, W, H)
    # --gather-scale runs and says what it did
    g = str(tmp_path / "g.ppm")
    text = run(["--gather", "4", "--gather-out", g, "--gather-scale", "1"])
    assert "gathered at 24x18" in text and os.path.getsize(g) == len(b"P6\n48 36\n255\n") + 3 * W * H
    for bad, msg in ((["--ao-scale", "1"], "--ao-scale needs --ao"),
                     (["--gather-scale", "1"], "--gather-scale needs --gather"),
                     (["--ao", "8,1", "--ao-out", out, "--ao-scale", "0"], "Invalid scale"),
                     (["--ao", "8,1", "--ao-out", out, "--ao-scale", "4"], "Invalid scale"),
                     (["--ao", "8,1", "--ao-out", out, "--ao-scale", "3"], "does not divide")):
        assert msg in run(bad, code=1)
    assert "--ao-scale" in run(["--help"]) and "--gather-scale" in run(["--help"])


# ---- 7. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda, ctx):
    torch = torch_cuda
    W, H, L = 32, 16, 1
    n, nl = W * H, (W >> L) * (H >> L)
    # one arena, 32 n bytes per buffer: a range laid over another buffer meets that buffer
    slot = 32 * n
    arena = torch.zeros((8 * slot,), dtype=torch.uint8, device="cuda")
    base = arena.data_ptr()
    hp, lp, sp, dp, op, cp, xp, ip = (base + k * slot for k in range(8))
    full, low = U.frames("reference", W, H, L)
    arena[:32 * n].copy_(_dev(torch, full))
    arena[slot:slot + 32 * nl].copy_(_dev(torch, low))
    arena[2 * slot:2 * slot + 4 * nl].copy_(_dev(torch, U.low_signal("reference", W >> L, H >> L, "gray")))
    nbytes = R.upsample_scratch(W, H, True)
    assert 0 < nbytes <= slot and hp % 16 == 0 and xp % 16 == 0
    ok = R.upsample_params(L, R.FILTER_GRAY, U.ALL, 1.0, 3)
    par = R.upsample_params

    def call(hits=hp, w=W, h=H, p=ok, lhits=lp, wl=W >> L, hl=H >> L, src=sp, dst=dp, holes=op,
             cap=n, count=cp, scratch=xp, sbytes=nbytes):
        ctx.upsample_device(hits, w, h, p, lhits, wl, hl, src, dst, holes, cap, count, scratch, sbytes)

    for kw, msg in ((dict(hits=0), "upsample: null hit buffer"),
                    (dict(lhits=0), "upsample: null low hit buffer"),
                    (dict(src=0), "upsample: null low source"),
                    (dict(dst=0), "upsample: null destination"),
                    (dict(w=0), "upsample: empty frame"),
                    (dict(hl=0), "upsample: empty low frame"),
                    (dict(w=(1 << 24) + 1), "at most 2\\^24"),
                    (dict(w=1 << 16, h=1 << 16), "at most 2\\^32 - 1 pixels"),
                    (dict(p=par(0, 1, 0, 0.0, 0)), "scaleLog2 0"),
                    (dict(p=par(4, 1, 0, 0.0, 0)), "scaleLog2 4"),
                    (dict(wl=W), "is not 2 times the low frame"),
                    (dict(hl=H >> 2), "is not 2 times the low frame"),
                    (dict(p=par(1, 1, 0, 0.0, 9)), "normalLog2 9"),
                    (dict(p=par(1, 3, 0, 0.0, 0)), "kind 3"),
                    (dict(p=par(1, 1, 16, 0.0, 0)), "unknown flags 0x10"),
                    (dict(holes=0), "holeCount without holes"),
                    (dict(count=0), "holes without holeCount"),
                    (dict(hits=hp + 4), "upsample: hit buffer not 16-byte aligned"),
                    (dict(lhits=lp + 8), "upsample: low hit buffer not 16-byte aligned"),
                    (dict(scratch=0), "scratch is null"),
                    (dict(sbytes=nbytes - 1), "scratch too small"),
                    (dict(scratch=xp + 4), "scratch misaligned"),
                    (dict(dst=hp + 32 * n - 4), "dst overlaps hits"),
                    (dict(dst=lp), "dst overlaps lowHits"),
                    (dict(dst=sp), "dst overlaps lowSrc"),
                    (dict(holes=dp), "dst overlaps holes"),
                    (dict(count=dp + 4 * n - 4), "dst overlaps holeCount"),
                    (dict(scratch=dp), "dst overlaps the scratch"),
                    (dict(holes=hp), "holes overlaps hits"),
                    (dict(holes=lp), "holes overlaps lowHits"),
                    (dict(holes=sp), "holes overlaps lowSrc"),
                    (dict(count=op), "holes overlaps holeCount"),
                    (dict(scratch=op), "holes overlaps the scratch"),
                    (dict(count=hp), "holeCount overlaps hits"),
                    (dict(count=lp), "holeCount overlaps lowHits"),
                    (dict(count=sp), "holeCount overlaps lowSrc"),
                    (dict(count=xp), "holeCount overlaps the scratch"),
                    (dict(scratch=hp), "the scratch overlaps hits"),
                    (dict(scratch=lp), "the scratch overlaps lowHits"),
                    (dict(scratch=sp), "the scratch overlaps lowSrc")):
        with pytest.raises(R.RtgError, match=msg):
            call(**kw)
    lib = R.lib()
    assert lib.rtg_upsample_device(ctx._h, hp, W, H, None, lp, W >> L, H >> L, sp, dp, op, n, cp, xp,
                                   nbytes, None) == -1
    assert b"upsample: null params" in lib.rtg_last_error()
    assert lib.rtg_upsample_device(None, hp, W, H, R._ptr(ok), lp, W >> L, H >> L, sp, dp, op, n, cp,
                                   xp, nbytes, None) == -1
    assert b"upsample: no context" in lib.rtg_last_error()
    for a, msg in (((0, n, ip, 4, dp), "hits_pick: null input"),
                   ((hp, n, 0, 4, dp), "hits_pick: null index buffer"),
                   ((hp, n, ip, 4, 0), "hits_pick: null output"),
                   ((hp, 0, ip, 4, dp), "hits_pick: n is 0"),
                   ((hp + 8, n, ip, 4, dp), "hits_pick: hit buffer not 16-byte aligned"),
                   ((hp, n, ip, 4, dp + 8), "hits_pick: output not 16-byte aligned"),
                   ((hp, n, ip, 4, hp + 32), "hits_pick: the output overlaps an input"),
                   ((hp, n, ip, 4, ip), "hits_pick: the output overlaps an input"),
                   # (nothing is dereferenced: the ranges lie far apart as numbers)
                   ((16, n, 1 << 56, 1 << 40, 1 << 58), "hits_pick: list too large")):
        with pytest.raises(R.RtgError, match=msg):
            ctx.hits_pick_device(*a)
    for a, msg in (((3, sp, ip, 4, n, dp), "values_place: kind 3"),
                   ((1, 0, ip, 4, n, dp), "values_place: null input"),
                   ((1, sp, 0, 4, n, dp), "values_place: null index buffer"),
                   ((1, sp, ip, 4, n, 0), "values_place: null output"),
                   ((1, sp, ip, 4, 0, dp), "values_place: n is 0"),
                   ((1, sp, ip, 4, n, sp), "values_place: the output overlaps an input"),
                   ((1, sp, ip, 4, n, ip), "values_place: the output overlaps an input"),
                   ((1, 1 << 56, 1 << 58, 1 << 40, n, dp), "values_place: list too large")):
        with pytest.raises(R.RtgError, match=msg):
            ctx.values_place_device(*a)
    assert lib.rtg_hits_pick_device(None, hp, n, ip, 4, dp, None) == -1
    assert b"hits_pick: no context" in lib.rtg_last_error()
    assert lib.rtg_values_place_device(None, 1, sp, ip, 4, n, dp, None) == -1
    assert b"values_place: no context" in lib.rtg_last_error()
    torch.cuda.synchronize()
    assert int(arena[3 * slot:].count_nonzero()) == 0  # nothing launched
    # ranges that touch do not overlap; no list: one launch, a null scratch
    ctx.upsample_device(hp, W, H, ok, lp, W >> L, H >> L, sp, dp)
    ctx.upsample_device(hp, W, H, ok, lp, W >> L, H >> L, sp, op, op + 4 * n, 8, op + 4 * n + 32,
                        xp, nbytes)
    torch.cuda.synchronize()
    want = _host(R, full, low, W, H, L, ok, U.low_signal("reference", W >> L, H >> L, "gray"))
    host = arena.cpu().numpy()
    for at in (3, 4):
        assert host[at * slot:at * slot + 4 * n].view(np.uint32).tobytes() == want[0].tobytes()
    k = min(8, want[2])
    lst = host[4 * slot + 4 * n:4 * slot + 4 * n + 32].view(np.uint32)
    assert (lst[:k] == want[1][:k]).all() and not lst[k:].any()
    assert host[4 * slot + 4 * n + 32:4 * slot + 4 * n + 36].view(np.uint32)[0] == want[2]
