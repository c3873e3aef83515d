"""GPU tests of the gather (rtg_gather*, include/rtg.h) on an MI355X, against the
references test_gather_host.py pins on the CPU (gathergen.py: the plain loops'
sums and skip counts and the host generator's rays), word for word.

Every destination is pre-filled and PAD records longer than its result; the
tail must stay.

  1. the fused kernel == gather_host(walk 0) for 1, 63, 64, 65 and 200 points
     and every parameter set of gathergen.cases (probe sets, jitter, the skip
     flag, stack sizes, semantics), on every scene of the CPU walk-1 list, one
     context per scene;
  2. gather_rays_device == gather_rays_host;
  3. the fused call == gather_rays_device + raytrace_device folded on the host;
  4. every hostile scene (hostile.CASES) at (7, 8) and S = 6;
  5. the one-shot form, and two streams on one context;
  6. a render before and after a gather on one context is unchanged;
  7. rtg_main --gather against the chain through the binding;
  8. the device entry points' argument checks, with no launch made.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import aogen
import gathergen as G
import hostile
from conftest import PKG, ROOT
from gathergen import JITTER, SCENES, SKIP
from hostile import CASES, IDS
from test_gpu_order import PAD, _stream

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


def _gather(torch, ctx, d_hits, n, p, d_dirs, d_w, nd, S=6, stream=None, counts=True):
    """(sums, skipped) of the fused call."""
    dst = torch.full(((n + PAD) * 3,), FILL32, dtype=torch.int32, device="cuda")
    skp = torch.full((n + PAD,), FILL16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    ctx.gather_device(d_hits.data_ptr(), n, p, d_dirs.data_ptr(), d_w.data_ptr(), nd,
                      dst.data_ptr(), skipped_ptr=skp.data_ptr() if counts else 0, stack_size=S,
                      stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    out, sk = dst.cpu().numpy(), skp.cpu().numpy().view(np.uint16)
    assert (out[n * 3:] == FILL32).all(), "sums past the batch were written"
    assert (sk[n if counts else 0:] == FILL16).all(), "counts past the batch were written"
    return out[:n * 3].view(np.float32).reshape(n, 3), sk[:n]


def _rays(torch, ctx, d_hits, n, p, d_dirs, nd):
    k = int(p["samples"][0])
    dst = torch.full(((n * k + PAD) * 6,), FILL32, dtype=torch.int32, device="cuda")
    ctx.gather_rays_device(d_hits.data_ptr(), n, p, d_dirs.data_ptr(), nd, dst.data_ptr(),
                           stream=_stream(torch))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n * k * 6:] == FILL32).all(), "rays past the batch were written"
    return out[:n * k * 6].view(np.float32).reshape(n * k, 6)


def _same(got, want, got_skp, want_skp, what):
    assert G.same_words(got, want) is None, (what, G.same_words(got, want))
    assert got.view(np.uint32).tobytes() == G.canon(got).tobytes(), (what, "a NaN is not canonical")
    assert got_skp.tobytes() == want_skp.tobytes(), (what, np.flatnonzero(got_skp != want_skp)[:4])


# ---- 1, 2. every path, size and parameter set; the generator ----

@pytest.mark.parametrize("name", SCENES)
def test_device_equals_plain_loops(R, torch_cuda, name):
    torch = torch_cuda
    G.assert_non_vacuous(name)  # on the walk-0 answer
    d_hits = _dev(torch, G.hits(name))
    ctx = R.Context(0)
    try:
        ctx.set_scene(G.scene(name), G.lights(name))
        nodes = ctx.scene_stats()["bvh_nodes"]
        assert (nodes > 0) == (G.PATHS[name] == "bvh"), nodes
        generated = set()
        for k, nd, flags, S, sem in G.cases(name):
            ctx.set_semantics(sem)
            p = G.params(R, name, k, flags)
            d_dirs, d_w = _dev(torch, G.dirs(nd)), _dev(torch, G.weights(nd))
            want, want_skp = G.want(name, k, nd, flags, S, sem)
            case = G.case_id((k, nd, flags, S, sem))
            for n in G.SIZES:
                got, skp = _gather(torch, ctx, d_hits, n, p, d_dirs, d_w, nd, S)
                _same(got, want[:n], skp, want_skp[:n], (case, n))
            if (k, nd, flags & JITTER) not in generated:
                generated.add((k, nd, flags & JITTER))
                want_rays = G.want_rays(name, k, nd, flags)
                for n in G.SIZES:
                    got = _rays(torch, ctx, d_hits, n, p, d_dirs, nd)
                    assert got.tobytes() == want_rays[:n * k].tobytes(), (case, n)
    finally:
        ctx.close()


# ---- 3. fused == generator + raytrace_device + the fold on the host ----

@pytest.mark.parametrize("name", ["reference", 40, "base150", "c5"])
def test_fused_equals_the_unfused_chain(R, torch_cuda, name):
    torch = torch_cuda
    h = G.hits(name)
    n = len(h)
    d_hits = _dev(torch, h)
    ctx = R.Context(0)
    try:
        ctx.set_scene(G.scene(name), G.lights(name))
        for k, nd, flags, S in ((16, 97, 0, 6), (7, 8, JITTER | SKIP, 6), (16, 97, JITTER | SKIP, 2)):
            p = G.params(R, name, k, flags)
            d_dirs, d_w = _dev(torch, G.dirs(nd)), _dev(torch, G.weights(nd))
            rays = torch.full(((n * k + PAD) * 6,), FILL32, dtype=torch.int32, device="cuda")
            cols = torch.full(((n * k + PAD) * 3,), FILL32, dtype=torch.int32, device="cuda")
            ctx.gather_rays_device(d_hits.data_ptr(), n, p, d_dirs.data_ptr(), nd, rays.data_ptr(),
                                   stream=_stream(torch))
            ctx.raytrace_device(rays.data_ptr(), n * k, cols.data_ptr(), stack_size=S,
                                stream=_stream(torch))
            torch.cuda.synchronize()
            col = cols.cpu().numpy()[:n * k * 3].view(np.float32).reshape(n * k, 3)
            acc, skp_want = G.fold(h, col, G.weights(nd), k, G.SEED, flags)
            got, skp = _gather(torch, ctx, d_hits, n, p, d_dirs, d_w, nd, S)
            _same(got, acc, skp, skp_want, (name, k, nd, flags, S))
    finally:
        ctx.close()


# ---- 4. hostile scenes ----

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
    from test_raytrace_host import THREADS
    sph, lg = hostile.mutated(n, name)
    h = aogen.hostile_hits(n, name)
    assert (h["id"] >= 0).any() and (h["id"] < 0).any()
    ctx = contexts(n)
    ctx.set_scene(sph, lg)
    if n > 64:  # which query path the kernel takes (hostile.expect)
        nodes = ctx.scene_stats()["bvh_nodes"]
        assert (nodes == 0) == (hostile.expect(n, name)[1] == "flat"), nodes
    d_hits, d_dirs, d_w = _dev(torch, h), _dev(torch, G.dirs(8)), _dev(torch, G.weights(8))
    for flags in (0, JITTER | SKIP):
        p = R.gather_params(7, aogen.BIAS, G.SEED, flags)
        want, want_skp = R.gather_host(sph, lg, h, G.dirs(8), G.weights(8), p, stack_size=6,
                                       walk=0, threads=THREADS, skipped=True)
        got, skp = _gather(torch, ctx, d_hits, len(h), p, d_dirs, d_w, 8)
        _same(got, want, skp, want_skp, flags)


# ---- 5. the one-shot form and two streams ----

def test_one_shot_and_streams(R, torch_cuda):
    torch = torch_cuda
    for name, (k, nd, flags) in (("reference", (7, 8, JITTER | SKIP)), ("base150", (16, 97, 0))):
        sph, lg, h = G.scene(name), G.lights(name), G.hits(name)
        p = G.params(R, name, k, flags)
        want, want_skp = G.want(name, k, nd, flags)
        got, skp = R.gather(sph, lg, h, G.dirs(nd), G.weights(nd), p, skipped=True)
        _same(got, want, skp, want_skp, (name, "one-shot"))
        assert G.same_words(R.gather(sph, lg, h, G.dirs(nd), G.weights(nd), p), want) is None
        d_hits, d_dirs, d_w = _dev(torch, h), _dev(torch, G.dirs(nd)), _dev(torch, G.weights(nd))
        ctx = R.Context(0)
        try:
            ctx.set_scene(sph, lg)
            # two launches in flight on two streams of one context, then each checked
            a, b = torch.cuda.Stream(), torch.cuda.Stream()
            outs = [torch.full((len(h) * 3,), FILL32, dtype=torch.int32, device="cuda")
                    for _ in range(2)]
            torch.cuda.synchronize()
            for st, dst in zip((a, b), outs):
                ctx.gather_device(d_hits.data_ptr(), len(h), p, d_dirs.data_ptr(), d_w.data_ptr(),
                                  nd, dst.data_ptr(), stream=st.cuda_stream)
            torch.cuda.synchronize()
            for dst in outs:
                got = dst.cpu().numpy().view(np.float32).reshape(-1, 3)
                assert G.same_words(got, want) is None, (name, "two streams")
            got, skp = _gather(torch, ctx, d_hits, len(h), p, d_dirs, d_w, nd, stream=0,
                               counts=False)  # the default stream, no counts asked for
            assert G.same_words(got, want) is None, (name, "default stream")
        finally:
            ctx.close()
    out, skp = R.gather(sph, lg, np.zeros(0, R.HIT_DTYPE), G.dirs(8), G.weights(8),
                        R.gather_params(7), skipped=True)
    assert out.shape == (0, 3) and skp.shape == (0,)


# ---- 6. no interference with the renders ----

def test_render_is_unchanged_by_a_gather(R, torch_cuda):
    torch = torch_cuda
    W, H = 64, 48
    for name in ("reference", "base150"):
        h = G.hits(name)
        d_hits, d_dirs, d_w = _dev(torch, h), _dev(torch, G.dirs(97)), _dev(torch, G.weights(97))
        ctx = R.Context(0)
        try:
            ctx.set_scene(G.scene(name), G.lights(name))
            frames = []
            for _ in range(2):
                fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
                ctx.render_device(W, H, fb.data_ptr(), stream=_stream(torch))
                torch.cuda.synchronize()
                frames.append(fb.cpu().numpy())
                got, skp = _gather(torch, ctx, d_hits, len(h), G.params(R, name, 16, JITTER),
                                   d_dirs, d_w, 97)
                want, want_skp = G.want(name, 16, 97, JITTER)
                _same(got, want, skp, want_skp, name)
            assert G.same_words(frames[1], frames[0]) is None, name
            assert (G.canon(frames[0]) << 1).any()  # not a black frame
        finally:
            ctx.close()


# ---- 7. the driver ----

def _chain(R, torch, sph, lg, cam, W, H, p, S):
    """camera_rays -> intersect_device -> gather_device -> max_colour_device ->
    ppm_bytes_device through the binding: the file's bytes."""
    n = W * H
    k = int(p["samples"][0])
    table = R.ao_directions(k)
    wt = np.full(k, np.float32(1) / np.float32(k), np.float32)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        s = _stream(torch)
        rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        light = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        mx = torch.zeros(1, dtype=torch.float32, device="cuda")
        out = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
        d_dirs, d_w = _dev(torch, table), _dev(torch, wt)
        ctx.camera_rays(cam, W, H, rays.data_ptr(), alias_factor=1.0, stream=s)
        ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream=s)
        ctx.gather_device(hits.data_ptr(), n, p, d_dirs.data_ptr(), d_w.data_ptr(), k,
                          light.data_ptr(), stack_size=S, stream=s)
        ctx.max_colour_device(light.data_ptr(), n, mx.data_ptr(), stream=s)
        ctx.ppm_bytes_device(light.data_ptr(), n, mx.data_ptr(), out.data_ptr(), stream=s)
        torch.cuda.synchronize()
        return b"P6\n%d %d\n255\n" % (W, H) + out.cpu().numpy().tobytes()
    finally:
        ctx.close()


def test_host_driver_gather_option(R, torch_cuda, tmp_path):
    torch = torch_cuda
    scene_file = os.path.join(ROOT, "scenes", "reference.scene")
    sph, lg = R.load_scene_file(scene_file)
    W, H, K = 48, 36, 16
    frame = str(tmp_path / "frame.ppm")
    base = [os.path.join(PKG, "rtg_main"), "--scene", scene_file, "--width", str(W), "--height",
            str(H), "--out", frame]
    for spec, extra, p, cam, S in (
            ("16", [], R.gather_params(K), R.camera_identity(), 6),
            ("16,0.01,77", ["--gather-skip", "--camera", "3,2,-1,0,0,-10", "--depth", "2"],
             R.gather_params(K, 0.01, 77, JITTER | SKIP), R.camera_look_at((3, 2, -1), (0, 0, -10)),
             3)):
        ppm = str(tmp_path / "gather.ppm")
        r = subprocess.run(base + ["--gather", spec, "--gather-out", ppm] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = _chain(R, torch, sph, lg, cam, W, H, p, S)
        body = np.frombuffer(want[-W * H * 3:], np.uint8)
        assert 0 < int((body > 0).sum()) < body.size  # lit and unlit pixels
        assert open(ppm, "rb").read() == want, spec
    for bad in (["--gather", "16"], ["--gather", "0", "--gather-out", "x.ppm"],
                ["--gather", "16,1,2,3", "--gather-out", "x.ppm"], ["--gather-out", "x.ppm"],
                ["--gather-skip"], ["--gather", "16", "--gather-out", frame]):  # usage: no GPU call
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("Invalid gather" in r.stdout or "go together" in r.stdout), \
            r.stdout
        assert "Device" not in r.stdout


# ---- 8. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    h = G.hits("reference")
    d_hits, d_dirs, d_w = _dev(torch, h), _dev(torch, G.dirs(8)), _dev(torch, G.weights(8))
    out = torch.zeros(((len(h) + PAD) * 3,), dtype=torch.int32, device="cuda")
    skp = torch.zeros((len(h) + PAD,), dtype=torch.int16, device="cuda")
    rays = torch.zeros(((len(h) * 7 + PAD) * 6,), dtype=torch.int32, device="cuda")
    ok = R.gather_params(7)
    hp, dp, wp, op, sp, rp = (t.data_ptr() for t in (d_hits, d_dirs, d_w, out, skp, rays))
    ctx = R.Context(0)
    try:
        with pytest.raises(R.RtgError, match="gather: no context/scene"):  # the fused call only
            ctx.gather_device(hp, len(h), ok, dp, wp, 8, op, skipped_ptr=sp)
        ctx.gather_rays_device(hp, len(h), ok, dp, 8, rp)
        torch.cuda.synchronize()
        assert int(rays.count_nonzero()) > 0
        rays.zero_()
        ctx.set_scene(G.scene("reference"), G.lights("reference"))

        def fused(hits=hp, n=8, p=ok, dirs=dp, wt=wp, nd=8, dst=op, S=6):
            ctx.gather_device(hits, n, p, dirs, wt, nd, dst, skipped_ptr=sp, stack_size=S)

        def gen(hits=hp, n=8, p=ok, dirs=dp, nd=8, dst=rp, **_):
            ctx.gather_rays_device(hits, n, p, dirs, nd, dst)

        for call in (fused, gen):
            for kw, msg in ((dict(hits=0), "null hit buffer"),
                            (dict(dirs=0), "null direction table"),
                            (dict(dst=0), "null output buffer"),
                            (dict(p=R.gather_params(0)), "0 samples"),
                            (dict(p=R.gather_params(1025), nd=2000), "1025 samples"),
                            (dict(nd=6), "6 directions"),
                            (dict(nd=65537), "65537 directions"),
                            (dict(p=R.gather_params(7, flags=4)), "unknown flags 0x4"),
                            (dict(n=1 << 32), "at most 2\\^32 - 1")):
                with pytest.raises(R.RtgError, match=msg):
                    call(**kw)
            call(n=0)  # an empty batch: RTG_OK, no launch
        for kw, msg in ((dict(wt=0), "null weight table"), (dict(S=0), "stackSize 0"),
                        (dict(S=17), "stackSize 17")):
            with pytest.raises(R.RtgError, match=msg):
                fused(**kw)
        with pytest.raises(R.RtgError, match="overflows size_t"):
            gen(n=1 << 62, p=R.gather_params(1024), dirs=dp, nd=1024)
        with pytest.raises(R.RtgError, match="too large"):  # 2^42 lanes: above 2^31-1 workgroups
            gen(n=(1 << 32) - 1, p=R.gather_params(1024), nd=1024)
        L = R.lib()
        assert L.rtg_gather_device(ctx._h, hp, 8, None, dp, wp, 8, 6, op, sp, None) == -1
        assert b"null params" in L.rtg_last_error()
        assert L.rtg_gather_rays_device(None, hp, 8, R._ptr(ok), dp, 8, rp, None) == -1
        assert b"no context" in L.rtg_last_error()
        torch.cuda.synchronize()
        assert int(out.count_nonzero()) == 0 and int(skp.count_nonzero()) == 0 and \
            int(rays.count_nonzero()) == 0  # nothing launched
    finally:
        ctx.close()
