"""GPU frames over the masked scenes' query forms (rtg_trace.h: the lazy shadow
and cone queries, the entering rays' overlap loop, the select loops, the
refraction target's containment loop), bit for bit against the oracle, NaNs at
the oracle's positions.

Frames of 64x48 at 3x3 supersampling; the stack capacity S of each frame is
drawn from 1..6 by a seeded generator.  Seeded random scenes of 1, 2, 3, 16 and
64 spheres with 1 to 4 lights; a scene of nested translucent spheres, whose
overlap masks are all full; and a scene whose second sphere lies so far behind
the light that no shadow mask holds another sphere, so every shadow selection
is empty once the wave drops the hit sphere.  The counting build (variant 120)
tells that the last two scenes reach what they are for.  test_query_forms_host.py
holds the host forms to the plain loops.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import bits_equal, first_mismatch, random_scene
from test_gpu_order import FILL, PAD, _stream

pytestmark = pytest.mark.gpu

W, H, AA = 64, 48, 3.0
# (spheres, lights) of the random scenes; S comes from the scene's generator
RANDOM = [(1, 1), (2, 2), (3, 3), (16, 4), (64, 2)]


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
    c = R.Context(0)
    yield c
    c.close()


def nested_scene(R):
    """Eight translucent spheres, each inside the next: every overlap mask holds
    all eight."""
    n = 8
    sph = np.zeros(n, R.SPHERE_DTYPE)
    for i in range(n):
        sph[i]["pos"] = [0.05 * i, -0.03 * i, -14.0]
        sph[i]["radius"] = 0.8 + 0.55 * i
        sph[i]["material"] = R.make_material(0.2, 0.3, [0.9, 0.5 + 0.05 * i, 0.3], [0.4, 0.6, 0.8],
                                             [1.0, 1.33, 1.55, 2.4][i % 4])
    lg = np.zeros(2, R.LIGHT_DTYPE)
    lg[0]["pos"], lg[0]["col"] = [20.0, 30.0, 5.0], [1.0, 0.9, 0.8]
    lg[1]["pos"], lg[1]["col"] = [-25.0, 4.0, -2.0], [0.3, 0.5, 1.0]
    return sph, lg


def lone_shadow_scene(R):
    """A sphere in view, one light above it, and a second sphere 170 beyond the
    light: neither sphere's shadow mask holds the other."""
    sph = np.zeros(2, R.SPHERE_DTYPE)
    sph[0]["pos"], sph[0]["radius"] = [0.0, 0.0, -10.0], 3.0
    sph[0]["material"] = R.make_material(0.7, 0.4, [0.8, 0.6, 0.2], [0.5, 0.5, 0.5], 1.33)
    sph[1]["pos"], sph[1]["radius"] = [0.0, 200.0, -10.0], 2.0
    sph[1]["material"] = R.make_material(1.0, 0.2, [0.2, 0.6, 0.8], [0.5, 0.5, 0.5], 1.0)
    lg = np.zeros(1, R.LIGHT_DTYPE)
    lg[0]["pos"], lg[0]["col"] = [0.0, 30.0, -10.0], [1.0, 1.0, 1.0]
    return sph, lg


def _frame(torch, ctx, s, variant=0):
    """A W x H frame into a pre-filled buffer; the words past it must stay."""
    n = W * H * 3
    dst = torch.full((n + PAD,), FILL, dtype=torch.int32, device="cuda")
    ctx.set_variant(variant)
    try:
        ctx.render_device(W, H, dst.data_ptr(), alias_factor=AA, stack_size=s, stream=_stream(torch))
        torch.cuda.synchronize()
    finally:
        ctx.set_variant(0)
    out = dst.cpu().numpy()
    assert (out[n:] == FILL).all(), "words past the frame were written"
    return out[:n].view(np.float32).reshape(H, W, 3)


def _check(torch, ctx, oracle, sph, lg, s, what):
    want = oracle.render(sph, lg, W, H, s, aa=AA)
    assert (np.ascontiguousarray(want).view(np.uint32) << 1).any(), (what, "black oracle frame")
    ctx.set_scene(sph, lg)
    got = _frame(torch, ctx, s)
    assert bits_equal(got, want), (what, s, first_mismatch(got, want))  # NaN positions included


@pytest.mark.parametrize("n,m", RANDOM, ids=[f"n{n}-m{m}" for n, m in RANDOM])
def test_random_scene_frames(R, oracle, torch_cuda, ctx, n, m):
    rng = np.random.default_rng(5000 + n)
    sph, lg = random_scene(rng, n, m)
    for s in sorted({int(rng.integers(1, 7)), int(rng.integers(1, 7)), 6}):
        _check(torch_cuda, ctx, oracle, sph, lg, s, f"n{n}-m{m}")


def _counts(R, torch, ctx, s):
    ctx.diag_counts(reset=True)
    _frame(torch, ctx, s, variant=120)
    wv, _ = ctx.diag_counts(reset=True)
    return {nm: int(wv[k]) for k, nm in enumerate(R.UNIT_NAMES)}


def test_nested_spheres_full_overlap_masks(R, oracle, torch_cuda, ctx):
    sph, lg = nested_scene(R)
    rng = np.random.default_rng(5100)
    for s in sorted({int(rng.integers(2, 7)), 6}):
        _check(torch_cuda, ctx, oracle, sph, lg, s, "nested")
    c = _counts(R, torch_cuda, ctx, 6)
    # entering rays walk the overlap loop and run its exact test; the
    # refraction target's containment loop runs
    assert c["U.enterIter"] > 0 and c["U.enterExact"] > 0 and c["U.contIter"] > 0, c


def test_every_shadow_selection_empty(R, oracle, torch_cuda, ctx):
    sph, lg = lone_shadow_scene(R)
    rng = np.random.default_rng(5200)
    for s in sorted({int(rng.integers(1, 7)), 6}):
        _check(torch_cuda, ctx, oracle, sph, lg, s, "lone shadow")
    c = _counts(R, torch_cuda, ctx, 6)
    # shadow queries ran, and waves whose lanes all dropped their hit sphere
    # returned on the empty selection (a wave with a grazing lane keeps it)
    assert c["shadowQ"] > 0 and c["D.shdEmpty"] > 0, c
