"""GPU tests of calculateRefraction's float-only sinA1 (rtg_trace.h
sin_from_cos2 / clamp_cos_sin, raytracer.h:671-683) on an MI355X:

  1. exhaustive: for EVERY float c in [0, 1) the float sequence gives
     (float)sqrt(1.0 - (double)(c * c)) bit for bit (tests/fpcheck/
     fpcheck_exact_gpu.hip; -c squares to the same float);
  2. the clamp cases (c = +-1 and beyond, both zeros, the last floats inside
     (-1, 1)) bit for bit and NaN as NaN, against the reference's branch;
  3. frames and a caller's rays over scenes whose refractive indices are
     hostile (0, negative, denormal, infinite, NaN, equal pairs) and whose
     spheres overlap, so that a source material other than the background
     occurs: the masked path (n = 5) and the BVH path (n = 70), S in {1, 2, 6},
     bit for bit against the oracle's frame and the plain loops' colours.

The references are computed once per case and left unchanged.
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import pytest

import raygen
from conftest import bits_equal, first_mismatch, random_scene
from test_gpu_order import _run, _stream
from test_raytrace_host import THREADS

pytestmark = pytest.mark.gpu

F = np.float32
W, H, AA = 64, 48, 3.0


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
def fplib():
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fpcheck",
                      "libfpcheck_exact_gpu.so")
    return ctypes.CDLL(so)


def test_sin_exhaustive(torch_cuda, fplib):
    out = (ctypes.c_ulonglong * 3)()
    assert fplib.fpcheck_sin_run(ctypes.c_ulonglong(0), out) == 0
    operands, bad, first = list(out)
    print(f"sinA1: {operands} operands, {bad} mismatches, first {first:#x}")
    assert operands == 0x3F800000
    assert bad == 0, f"{bad} cosines differ, first bit pattern {first:#010x}"


def test_clamp_cases(torch_cuda, fplib):
    one = np.array([1.0], F).view(np.uint32)[0]
    vals = np.array([1.0, -1.0, 1.5, -1.5, np.inf, -np.inf, 0.0, -0.0, 0.5, -0.5, 1e-30, 1e-45,
                     np.nan], F).view(np.uint32)
    pats = np.concatenate([vals, [one - 1, one + 1, (one - 1) | 0x80000000, (one + 1) | 0x80000000,
                                  0xFFC00000, 0x7F800001]]).astype(np.uint32)
    n = len(pats)
    got = np.zeros(2 * n, np.uint32)
    want = np.zeros(2 * n, np.uint32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert fplib.fpcheck_clamp_run(P(pats), n, P(got), P(want)) == 0
    gf, wf = got.view(F), want.view(F)
    nan = np.isnan(wf)
    print("clamp cases (cos, sin) got:", [hex(v) for v in got], "want:", [hex(v) for v in want])
    assert (np.isnan(gf) == nan).all(), "NaN positions"
    assert (got[~nan] == want[~nan]).all(), (got, want)
    assert nan[2 * (len(vals) - 1) + 1], "the NaN cosine's sine is NaN in the reference"
    assert want[1] == 0 and want[3] == 0 and wf[0] == 1.0 and wf[2] == -1.0


def test_pair_table(torch_cuda, fplib):
    """The host-built material-pair records (rtg_scene_pack.h pair_consts)
    hold the bits of the device's own nSrc / nTgt and 1.f - 1.f / (r * r), for
    65 indices with 0, -1.5, denormals, infinities, NaN, 1 and equal pairs."""
    rng = np.random.default_rng(65)
    idx = np.concatenate([
        np.array([0.0, -0.0, -1.5, 1e-40, -1e-42, 1.4e-45, 1.1754942e-38, 1.1754944e-38, np.inf,
                  -np.inf, np.nan, 1.0, 1.0, 1.5, 1.5, 1.33, 2.4, 3.4e38, 1e-20, 1e20, 1e-19, 6e18],
                 F),
        rng.uniform(0.5, 3.0, 65 - 22).astype(F)])
    k = len(idx)
    assert k == 65
    host = np.zeros(2 * k * k, F)
    dev = np.zeros(2 * k * k, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert fplib.fpcheck_pair_run(P(idx), k, P(host), P(dev)) == 0
    hb, db = host.view(np.uint32), dev.view(np.uint32)
    nan = np.isnan(dev)
    print(f"pair table: {int(nan.sum())} NaN words, {int(np.isinf(dev).sum())} infinite, "
          f"{int((hb != db)[~nan].sum())} differ")
    assert (np.isnan(host) == nan).all(), "NaN positions"
    assert (hb[~nan] == db[~nan]).all(), np.flatnonzero((hb != db) & ~nan)[:8]
    # (non-vacuity: denormal quotients, infinities and NaN are all there)
    assert nan.any() and np.isinf(dev).any()
    assert ((np.abs(dev) > 0) & (np.abs(dev) < F(1.1754944e-38))).any()


# ---- frames and a caller's rays over hostile refractive indices ----

INDICES = (0.0, -1.5, 1e-40, -1e-42, np.inf, -np.inf, np.nan, 1.0, 1.0, 1.5, 1.5, 1.33, 2.4, 0.75)
SCENES = {"n5a": (5, 0), "n5b": (5, 5), "n5c": (5, 10), "n70": (70, 0)}
STACKS = (1, 2, 6)


@functools.lru_cache(maxsize=None)
def _scene(name):
    n, first = SCENES[name]
    sph, lg = random_scene(np.random.default_rng(4100 + n + first), n, 2)
    m = sph["material"]
    if n == 5:  # one overlapping cluster in view: each sphere reaches into its neighbours
        for i in range(n):
            sph["pos"][i] = (-3.0 + 1.5 * i, 0.6 * (-1) ** i, -11.0 - 0.5 * i)
            sph["radius"][i] = 1.6 + 0.1 * i
    else:
        sph["radius"] *= F(0.6)  # overlaps remain, and a tree to walk
    for i in range(n):
        m["opacity"][i] = (0.2, 0.5, 0.35)[i % 3]  # translucent: every index is used
        m["refractiveIndex"][i] = INDICES[(first + i) % len(INDICES)]
    sph.setflags(write=False)
    lg.setflags(write=False)
    return sph, lg


@functools.lru_cache(maxsize=None)
def _rays():
    rays = np.ascontiguousarray(raygen.primary(W, H), F)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _oracle_frame(oracle, name, s):
    sph, lg = _scene(name)
    fb = oracle.render(sph.copy(), lg.copy(), W, H, s, aa=AA)
    fb.setflags(write=False)
    return fb


@functools.lru_cache(maxsize=None)
def _plain_colours(name, s):
    import rtg_amd
    sph, lg = _scene(name)
    return rtg_amd.raytrace_host(sph.copy(), lg.copy(), _rays(), stack_size=s, semantics=0, walk=0,
                                 threads=THREADS)


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("s", STACKS)
@pytest.mark.parametrize("name", list(SCENES))
def test_hostile_indices(R, oracle, torch_cuda, ctx, name, s):
    torch = torch_cuda
    sph, lg = (a.copy() for a in _scene(name))
    ctx.set_scene(sph, lg)
    if len(sph) > 64:
        assert ctx.scene_stats()["bvh_nodes"] > 0, "the BVH path"

    want = _oracle_frame(oracle, name, s)
    if s > 1:  # (non-vacuity, on the reference: refraction reaches the frame)
        assert not bits_equal(want, _oracle_frame(oracle, name, 1))
    dst = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    ctx.render_device(W, H, dst.data_ptr(), alias_factor=AA, stack_size=s, stream=_stream(torch))
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert bits_equal(got, want), ("frame", first_mismatch(got, want))

    rays = _rays()
    d_rays = torch.from_numpy(rays.copy()).cuda()
    got = _run(torch, functools.partial(ctx.raytrace_device, stack_size=s), d_rays, len(rays), 3,
               None).view(F).reshape(-1, 3)
    want = _plain_colours(name, s)
    assert bits_equal(got, want), ("rays", first_mismatch(got, want))


def test_hostile_scenes_hold_nan_and_sources(oracle):
    """On the references: a NaN reaches some frame, and the clustered scenes'
    spheres overlap (a refraction there starts inside another sphere)."""
    assert any(np.isnan(_oracle_frame(oracle, name, 6)).any() for name in SCENES)
    sph, _ = _scene("n5a")
    d = np.linalg.norm(sph["pos"][1:] - sph["pos"][:-1], axis=1)
    assert (d < sph["radius"][1:] + sph["radius"][:-1]).all()
