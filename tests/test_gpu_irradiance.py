"""GPU tests of the probe grid's lookup (rtg_irradiance*, include/rtg.h) on an
MI355X, against the references test_irradiance_host.py pins on the CPU
(irrgen.py: the plain loops' colours and weights), bit for bit with NaN
canonicalised.

Every destination is pre-filled and PAD records longer than its result; the
tail must stay.

  1. irradiance_device == irradiance_host(walk 0) for 1, 63, 64, 65 and 200
     points, every subset of the flags and 1..3 bands, with and without the
     weight buffer, on every scene of the CPU walk-1 list, one context per
     scene;
  2. every hostile scene (hostile.CASES) with all three flags, one context per
     size taking the mutations in turn;
  3. the real chain on a 2 x 2 x 2 grid over the reference scene:
     probe_grid_poses -> render_views_fold_device, contains_device, then
     irradiance_device over the primary hits of a frame, against the same chain
     through the host forms;
  4. the one-shot form, a launch on a stream of its own and on the default one,
     and a context without a scene where RTG_IRR_VISIBLE is not set;
  5. rtg_main --probe-grid --irradiance;
  6. the device entry point's argument checks.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import aogen
import hostile
import irrgen as G
from conftest import PKG, ROOT
from hostile import CASES, IDS
from irrgen import BANDS, BIAS, FLAG_SETS, GRIDS, N_POINTS, SCENES, SIZES
from test_gpu_order import PAD, _stream
from test_raytrace_host import THREADS

pytestmark = pytest.mark.gpu

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


def _dev_bytes(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).cuda()


def _irr(torch, ctx, d_hits, n, g, d_coef, d_valid, p, weight=True, stream=None):
    """(colours, weights) of the first n records; weights None without a buffer."""
    dst = torch.full(((n + PAD) * 3,), FILL32, dtype=torch.int32, device="cuda")
    wgt = torch.full((n + PAD,), FILL32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    ctx.irradiance_device(d_hits.data_ptr(), n, g, d_coef.data_ptr(), p, dst.data_ptr(),
                          valid_ptr=d_valid.data_ptr() if d_valid is not None else 0,
                          weight_ptr=wgt.data_ptr() if weight else 0,
                          stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint32)
    w = wgt.cpu().numpy().view(np.uint32)
    assert (out[3 * n:] == FILL32).all(), "colours past the batch were written"
    assert (w[n:] == FILL32).all(), "weights past the batch were written"
    if not weight:
        assert (w == FILL32).all(), "weights were written without a weight buffer"
    return out[:3 * n].view(np.float32).reshape(n, 3), (w[:n].view(np.float32) if weight else None)


# ---- 1. every path, size, flag subset and band count ----

@pytest.mark.parametrize("name", SCENES)
def test_device_equals_plain_loops(R, torch_cuda, name):
    torch = torch_cuda
    d_hits = _dev(torch, G.hits(name))
    ctx = R.Context(0)
    try:
        ctx.set_scene(G.scene(name), G.mattegen.lights(name))
        nodes = ctx.scene_stats()["bvh_nodes"]
        assert (nodes > 0) == (aogen.PATHS[name] == "bvh"), nodes
        for kind in GRIDS:
            d_valid = _dev_bytes(torch, G.valid(name, kind))
            for bands in BANDS:
                g = G.grid(name, kind, bands)
                d_coef = _dev(torch, G.coeffs(name, kind, bands))
                for flags in FLAG_SETS:
                    want, want_w = G.want(name, kind, bands, flags)
                    p = G.params(R, flags)
                    for n in (SIZES if kind == "lattice" else (N_POINTS,)):
                        got, w = _irr(torch, ctx, d_hits, n, g, d_coef, d_valid, p)
                        where = (kind, bands, flags, n)
                        assert G.same_words(got, want[:n]) is None, \
                            (where, G.same_words(got, want[:n]))
                        assert G.same_words(w, want_w[:n]) is None, \
                            (where, G.same_words(w, want_w[:n]))
                    got, _ = _irr(torch, ctx, d_hits, N_POINTS, g, d_coef, d_valid, p, weight=False)
                    assert G.same_words(got, want) is None, (kind, bands, flags, "no weight")
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


def _hostile_tables(n):
    """A 3 x 3 x 3 lattice over hostile base scene n with seeded tables."""
    g = G.lattice_over(hostile.base(n)[0], (3, 3, 3), 3)
    rng = np.random.default_rng(5200 + n)
    coef = rng.uniform(-1, 1, size=(27 * 9, 3)).astype(np.float32)
    valid = (rng.random(27) >= 0.25).astype(np.uint8)
    return g, coef, valid


@pytest.mark.parametrize("n,name", CASES, ids=IDS)
def test_hostile_scene(R, torch_cuda, contexts, n, name):
    torch = torch_cuda
    sph, lg = hostile.mutated(n, name)
    h = aogen.hostile_hits(n, name)
    assert (h["id"] >= 0).any() and (h["id"] < 0).any()
    g, coef, valid = _hostile_tables(n)
    p = G.params(R, 7)
    ctx = contexts(n)
    ctx.set_scene(sph, lg)
    if n > 64:  # which query path the kernel takes (hostile.expect)
        nodes = ctx.scene_stats()["bvh_nodes"]
        assert (nodes == 0) == (hostile.expect(n, name)[1] == "flat"), nodes
    want, want_w = R.irradiance_host(sph, h, g, coef, p, valid, walk=0, threads=THREADS,
                                     weight=True)
    got, w = _irr(torch, ctx, _dev(torch, h), len(h), g, _dev(torch, coef),
                  _dev_bytes(torch, valid), p)
    assert G.same_words(got, want) is None, G.same_words(got, want)
    assert G.same_words(w, want_w) is None, G.same_words(w, want_w)


# ---- 3. the real chain: bake, validity, lookup ----

W, H, RES = 48, 36, 8
DRIVER_DIMS = (2, 2, 2)


def _host_chain(R, sph, lg, g, cam, p):
    """(colours, weights) of a W x H frame through the host forms, walk 0."""
    poses = R.probe_grid_poses(g)
    fold = R.fold_params(6, 9, R.FOLD_SKIP_NONFINITE)
    coef = R.render_views_fold_host(sph, lg, poses, RES, RES, R.cube_sh_weights(RES, 3), fold,
                                    zoom=-1.0, alias_factor=1.0, stack_size=6, walk=0,
                                    threads=THREADS)
    valid = (R.contains_host(sph, R.probe_grid_points(g), walk=0) < 0).astype(np.uint8)
    rays = R.camera_rays_host(cam, W, H, alias_factor=1.0, threads=THREADS)
    h = R.intersect_host(sph, rays, walk=0, threads=THREADS)
    return R.irradiance_host(sph, h, g, coef.reshape(-1, 3), p, valid, walk=0, threads=THREADS,
                             weight=True)


def _device_chain(R, torch, ctx, g, cam, p, ppm=False):
    """The same on the device; ppm: the P6 file's bytes instead."""
    n, s = W * H, _stream(torch)
    n_probes = G.probes(g)
    poses = _dev(torch, R.probe_grid_poses(g))
    wts = _dev(torch, R.cube_sh_weights(RES, 3))
    pts = _dev(torch, R.probe_grid_points(g))
    fold = R.fold_params(6, 9, R.FOLD_SKIP_NONFINITE)
    bytes_ = R.views_fold_scratch(6 * n_probes, RES, RES, 9)
    scratch = torch.zeros(bytes_ // 4 + 4, dtype=torch.int32, device="cuda")
    coef = torch.zeros((n_probes * 9, 3), dtype=torch.float32, device="cuda")
    inside = torch.zeros(n_probes, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.render_views_fold(poses.data_ptr(), 6 * n_probes, RES, RES, fold, wts.data_ptr(),
                          coef.data_ptr(), scratch.data_ptr(), bytes_, zoom=-1.0, alias_factor=1.0,
                          stack_size=6, stream=s)
    ctx.contains_device(pts.data_ptr(), n_probes, inside.data_ptr(), stream=s)
    valid = (inside < 0).to(torch.uint8)
    rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    ctx.camera_rays(cam, W, H, rays.data_ptr(), alias_factor=1.0, stream=s)
    ctx.intersect_device(rays.data_ptr(), n, hits.data_ptr(), stream=s)
    if not ppm:
        return _irr(torch, ctx, hits, n, g, coef, valid, p)
    light = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    mx = torch.zeros(1, dtype=torch.float32, device="cuda")
    out = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    ctx.irradiance_device(hits.data_ptr(), n, g, coef.data_ptr(), p, light.data_ptr(),
                          valid_ptr=valid.data_ptr(), stream=s)
    ctx.max_colour_device(light.data_ptr(), n, mx.data_ptr(), stream=s)
    ctx.ppm_bytes_device(light.data_ptr(), n, mx.data_ptr(), out.data_ptr(), stream=s)
    torch.cuda.synchronize()
    return b"P6\n%d %d\n255\n" % (W, H) + out.cpu().numpy().tobytes()


def test_bake_validity_and_lookup_equal_the_host_chain(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    g = G.driver_grid(R, sph, DRIVER_DIMS, 3)
    p = R.irradiance_params(BIAS, R.IRR_LOBE_COSINE, 7)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        for cam in (R.camera_identity(), R.camera_look_at(*hostile.POSE)):
            want, want_w = _host_chain(R, sph, lg, g, cam, p)
            got, w = _device_chain(R, torch, ctx, g, cam, p)
            assert G.same_words(got, want) is None, G.same_words(got, want)
            assert G.same_words(w, want_w) is None, G.same_words(w, want_w)
            assert (want_w > 0).any() and (G.canon(want) << 1).any()  # not a black frame
    finally:
        ctx.close()


# ---- 4. the one-shot form, the streams, no scene without RTG_IRR_VISIBLE ----

def test_one_shot_streams_and_no_scene(R, torch_cuda):
    torch = torch_cuda
    for name, bands in (("reference", 3), ("base150", 2)):
        sph, h, g = G.scene(name), G.hits(name), G.grid(name, "lattice", bands)
        coef, valid = G.coeffs(name, "lattice", bands), G.valid(name, "lattice")
        d_hits, d_coef, d_valid = _dev(torch, h), _dev(torch, coef), _dev_bytes(torch, valid)
        for flags in (7, 3):
            want, want_w = G.want(name, "lattice", bands, flags)
            p = G.params(R, flags)
            got, w = R.irradiance(sph, h, g, coef, p, valid, weight=True)
            assert G.same_words(got, want) is None and G.same_words(w, want_w) is None, name
            assert G.same_words(R.irradiance(sph, h, g, coef, p, valid), want) is None, name
            ctx = R.Context(0)
            try:
                if flags & G.VISIBLE:
                    ctx.set_scene(sph, G.mattegen.lights(name))
                own = torch.cuda.Stream()
                for stream in (own.cuda_stream, 0):  # flags 3: a context with no scene
                    got, w = _irr(torch, ctx, d_hits, len(h), g, d_coef, d_valid, p, stream=stream)
                    assert G.same_words(got, want) is None and G.same_words(w, want_w) is None
            finally:
                ctx.close()
        want = G.want(name, "lattice", bands, 6)[0]  # no validity table without RTG_IRR_VALID
        assert G.same_words(R.irradiance(sph, h, g, coef, G.params(R, 6)), want) is None
    assert R.irradiance(sph, np.zeros(0, R.HIT_DTYPE), g, coef, p, valid).shape == (0, 3)


# ---- 5. the driver ----

def test_host_driver_irradiance_option(R, torch_cuda, tmp_path):
    torch = torch_cuda
    scene_file = os.path.join(ROOT, "scenes", "reference.scene")
    sph, lg = R.load_scene_file(scene_file)
    g = G.driver_grid(R, sph, DRIVER_DIMS, 3)
    frame = str(tmp_path / "frame.ppm")
    base = [os.path.join(PKG, "rtg_main"), "--scene", scene_file, "--width", str(W), "--height",
            str(H), "--out", frame]
    spec = "%d,%d,%d,%d" % (*DRIVER_DIMS, RES)
    ctx = R.Context(0)
    try:
        ctx.set_scene(sph, lg)
        for extra, cam, flags in (
                ([], R.camera_identity(), 7),
                (["--camera", "3,2,-1,0,0,-10", "--irr-flags", "facing,valid", "--irr-bias",
                  "0.01"], R.camera_look_at((3, 2, -1), (0, 0, -10)), 3)):
            ppm = str(tmp_path / "irr.ppm")
            r = subprocess.run(base + ["--probe-grid", spec, "--irradiance", ppm] + extra,
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            p = R.irradiance_params(0.01 if extra else BIAS, R.IRR_LOBE_COSINE, flags)
            want = _device_chain(R, torch, ctx, g, cam, p, ppm=True)
            body = np.frombuffer(want[-W * H * 3:], np.uint8)
            assert 0 < int((body > 0).sum()) < body.size  # lit and unlit pixels
            assert open(ppm, "rb").read() == want, extra
    finally:
        ctx.close()
    ppm = str(tmp_path / "irr.ppm")
    for bad in (["--probe-grid", spec], ["--irradiance", ppm],
                ["--probe-grid", spec, "--irradiance", frame],
                ["--probe-grid", "2,2", "--irradiance", ppm],
                ["--probe-grid", "2,2,2,8,4", "--irradiance", ppm],
                ["--probe-grid", spec, "--irradiance", ppm, "--irr-flags", "valid,seen"],
                ["--probe-grid", spec, "--irradiance"]):  # usage errors: no GPU call
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("go together" in r.stdout or "Invalid" in r.stdout or
                                      "Missing value" in r.stdout), r.stdout
        assert "Device" not in r.stdout


# ---- 6. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    name = "reference"
    h, g0 = G.hits(name), G.grid(name).copy()
    d_hits, d_coef = _dev(torch, h), _dev(torch, G.coeffs(name, "lattice", 3))
    d_valid = _dev_bytes(torch, G.valid(name, "lattice"))
    out = torch.zeros(((len(h) + PAD) * 3,), dtype=torch.int32, device="cuda")
    wgt = torch.zeros((len(h) + PAD,), dtype=torch.int32, device="cuda")
    hp, cp, vp, op, wp = (t.data_ptr() for t in (d_hits, d_coef, d_valid, out, wgt))
    p7, p3 = G.params(R, 7), G.params(R, 3)

    def grid_with(**kw):
        g = g0.copy()
        for k, v in kw.items():
            g[k][0] = v
        return g

    def flags_of(f):
        p = p7.copy()
        p["flags"][0] = f
        return p

    ctx = R.Context(0)
    try:
        with pytest.raises(R.RtgError, match="RTG_IRR_VISIBLE on a context without a scene"):
            ctx.irradiance_device(hp, len(h), g0, cp, p7, op, valid_ptr=vp, weight_ptr=wp)
        ctx.set_scene(G.scene(name), G.mattegen.lights(name))
        for kw, msg in (
                (dict(hits_ptr=0), "irradiance: null hit buffer"),
                (dict(coeffs_ptr=0), "irradiance: null coefficient table"),
                (dict(dst_ptr=0), "irradiance: null output buffer"),
                (dict(valid_ptr=0), "RTG_IRR_VALID with a null validity table"),
                (dict(grid=grid_with(step=(1.0, 0.0, 1.0))), "is not finite and > 0"),
                (dict(grid=grid_with(step=(1.0, np.inf, 1.0))), "is not finite and > 0"),
                (dict(grid=grid_with(origin=(np.nan, 0.0, 0.0))), "origin is not finite"),
                (dict(grid=grid_with(ny=0)), "outside \\[1, 2\\^20\\]"),
                (dict(grid=grid_with(nx=1 << 20, ny=1 << 11)), "at most 2\\^31 - 1 in all"),
                (dict(grid=grid_with(bands=4)), "4 bands outside \\[1, 3\\]"),
                (dict(params=flags_of(16)), "unknown flag bits 0x10"),
                (dict(n=1 << 32), "at most 2\\^32 - 1")):
            a = dict(hits_ptr=hp, n=len(h), grid=g0, coeffs_ptr=cp, params=p7, dst_ptr=op,
                     valid_ptr=vp, weight_ptr=wp)
            a.update(kw)
            with pytest.raises(R.RtgError, match=msg):
                ctx.irradiance_device(**a)
        ctx.irradiance_device(hp, 0, g0, cp, p7, op, valid_ptr=vp, weight_ptr=wp)  # empty: no launch
        L = R.lib()
        assert L.rtg_irradiance_device(None, hp, 8, R._ptr(g0), cp, vp, R._ptr(p3), op, wp,
                                       None) == -1
        assert b"irradiance: no context" in L.rtg_last_error()
        assert L.rtg_irradiance_device(ctx._h, hp, 8, None, cp, vp, R._ptr(p3), op, wp, None) == -1
        assert b"null grid" in L.rtg_last_error()
        assert L.rtg_irradiance_device(ctx._h, hp, 8, R._ptr(g0), cp, vp, None, op, wp, None) == -1
        assert b"null params" in L.rtg_last_error()
        torch.cuda.synchronize()
        assert int(out.count_nonzero()) == 0 and int(wgt.count_nonzero()) == 0  # nothing launched
    finally:
        ctx.close()
