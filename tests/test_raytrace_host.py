"""CPU tests of the batch ray tracer's host forms (rtg_raytrace_host,
csrc/rtg_raytrace.hip): rayTrace's colour for a caller's own rays.

  1. walk 0 (plain loops) of a frame's primary rays, folded, is the oracle's
     frame, CPU and OpenCL semantics;
  2. walk 0 of the nine sample rays per pixel of the golden small frames,
     folded as main.cpp:442-445 does, is the reference's own frame;
  3. walk 1 (the device kernel's path compiled for the host) equals walk 0 byte
     for byte on rays from anywhere, with conditions that keep it from passing
     vacuously; and for every stack size 1 .. 16 on a small batch, each size
     pinned to the plain loops and the oracle at that size;
  4. the argument errors of the contract.

All comparisons are bit for bit, NaN canonicalised as conftest.bits_equal does
(the library writes NaN words as 0xFFC00000 already).
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import pytest

import raygen
from conftest import GOLDEN, bits_equal, first_mismatch, load_f32, load_scene, random_scene
from test_gpu_rays import _mixed, _odd_rays

F = np.float32
THREADS = min(16, os.cpu_count() or 1)


# ---- the rays of a frame and the fold of a pixel (shared with test_gpu_raytrace.py) ----

def sample_rays(W, H, aa=3.0, zoom=-4.0):
    """The primary rays of every sample of a W x H frame, formed in numpy
    float32 exactly as main.cpp:411-436 forms them (raygen.primary is the aa = 1
    case): pixel order, a pixel's samples in the reference's loop order (i
    outer: the y step, j inner: the x step).  (H*W*nAA*nAA, 6) float32."""
    aa, zoom = F(aa), F(zoom)
    xs, ys, asp = F(16) / F(W), F(12) / F(H), F(16) / F(12)
    st = xs / aa
    halfW, halfH = F(W) * F(0.5), F(H) * F(0.5)
    nAA = 0
    while F(nAA) < aa:  # `for (int i = 0; i < aliasFactor; ++i)`
        nAA += 1
    y, x, i, j = np.meshgrid(np.arange(H), np.arange(W), np.arange(nAA), np.arange(nAA),
                             indexing="ij")
    pxX = (x.astype(F) - halfW) * xs
    pxY = (halfH - y.astype(F)) * ys
    v = [(pxX + j.astype(F) * st) * asp, pxY + i.astype(F) * st, np.full(x.shape, zoom, F)]
    assert all(q.dtype == F for q in v)
    l = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    out = np.zeros((x.size, 6), F)
    for q in range(3):
        out[:, 3 + q] = (l * v[q]).reshape(-1)
    return out, nAA * nAA


def fold(cols, W, H, nS, aa):
    """main.cpp:442-445: pix = 0; for each sample in order: pix += col * (1/nS),
    in float32, 1/nS the float quotient 1 / (aa * aa)."""
    inv = F(1) / (F(aa) * F(aa))
    c = np.ascontiguousarray(cols, F).reshape(H, W, nS, 3)
    pix = np.zeros((H, W, 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(nS):
            pix = pix + c[:, :, s] * inv
    return pix


@functools.lru_cache(maxsize=None)
def scene_with_lights(name):
    """raygen.scene's spheres with their lights."""
    import rtg_amd as R
    if name == "reference":
        return R.reference_scene()
    if name == "c5":
        return load_scene("c5", 1024, 4)
    return random_scene(np.random.default_rng(1000 + name), name, 2)


# ---- 1. pinned to the reference through the oracle ----

@pytest.mark.parametrize("name", ["reference", 12, 200])
def test_primary_rays_fold_to_the_oracle_frame(rtg, oracle, name):
    sph, lg = scene_with_lights(name)
    assert len(lg) == 2
    W, H = 64, 48
    rays = raygen.primary(W, H)
    lit = False
    for S in (1, 2, 3, 6, 16):
        for sem, render in ((0, oracle.render), (1, oracle.render_cl)):
            col = rtg.raytrace_host(sph, lg, rays, stack_size=S, semantics=sem, walk=0,
                                    threads=THREADS)
            with np.errstate(invalid="ignore"):
                fb = (F(0) + col * F(1)).reshape(H, W, 3)
            want = render(sph, lg, W, H, S, aa=1.0)
            assert bits_equal(fb, want), (S, sem, first_mismatch(fb, want))
            lit = lit or bool((np.nan_to_num(fb) != 0).any())
    assert lit, "black frames"


# ---- 2. pinned to the reference's own frames ----

@pytest.mark.parametrize("cfg", ["ref800", "c2", "c3", "c5"])
def test_sample_rays_fold_to_the_golden_small_frame(rtg, golden, cfg):
    c = golden["configs"][cfg]
    sph, lg = load_scene(cfg, c["spheres"], c["lights"])
    W, H = c["small"]["W"], c["small"]["H"]
    aa, zoom = golden["aliasFactor"], golden["zoom"]
    rays, nS = sample_rays(W, H, aa, zoom)
    assert (W, H, nS) == (96, 54, 9)
    col = rtg.raytrace_host(sph, lg, rays, stack_size=c["stack_size"], walk=0, threads=THREADS)
    fb = fold(col, W, H, nS, aa)
    want = load_f32(os.path.join(GOLDEN, f"{cfg}.small.f32"), (H, W, 3))
    assert bits_equal(fb, want), first_mismatch(fb, want)


# ---- 3. walk 1 == walk 0 ----

def extra_rays(sph, lg, seed):
    """Rays the generator mix of test_gpu_rays._mixed does not hold: origins at
    sphere centres and at light positions, origins 1 to 8 scene diagonals from
    the scene aimed at silhouettes with raygen.DISPLACEMENTS (where a promotion
    of distant rays to the renderer's table paths by a distance bound would
    change sides), and the `odd` rays (zero, NaN and infinite components, |d|
    of 2^-40 and 2^40)."""
    rng = np.random.default_rng(seed)
    parts = []
    if len(sph):
        c = sph["pos"].astype(np.float64)
        r = np.abs(sph["radius"].astype(np.float64))
        k = 24
        i = rng.integers(0, len(sph), k)
        centre = np.concatenate([c[i], raygen._unit(rng, k)], axis=1)
        parts.append(centre.astype(F))
        if len(lg):
            # from each light towards spheres, as a shadow ray runs backwards
            l = rng.integers(0, len(lg), k)
            lp = lg["pos"].astype(np.float64)[l]
            aim = c[i] + 0.7 * r[i][:, None] * raygen._unit(rng, k)
            parts.append(np.concatenate([lp, aim - lp], axis=1).astype(F))
        # the band: 1 to 8 diagonals out, tangent to sphere i up to the displacement
        lo, hi = raygen.bounds(sph)
        diag = float(np.linalg.norm(hi - lo))
        k = 96
        i = rng.integers(0, len(sph), k)
        u = raygen._unit(rng, k)
        w = raygen._perp(u, rng)
        dist = diag * rng.uniform(1.0, 8.0, k)
        eps = np.asarray(raygen.DISPLACEMENTS)[np.arange(k) % len(raygen.DISPLACEMENTS)]
        sin_a = r[i] / dist
        cos_a = np.sqrt(1.0 - sin_a * sin_a)
        o = c[i] + dist[:, None] * u
        aim = c[i] + (r[i] * (1.0 + eps))[:, None] * (sin_a[:, None] * u + cos_a[:, None] * w)
        parts.append(np.concatenate([o, aim - o], axis=1).astype(F))
    parts.append(_odd_rays(sph, seed + 1))
    return np.concatenate(parts)


def mixed_rays(sph, lg, n, seed):
    """n rays (n >= 256): the mix of test_gpu_rays._mixed with extra_rays
    shuffled in, so that a wave holds every kind."""
    rng = np.random.default_rng(seed)
    extra = extra_rays(sph, lg, seed + 7)
    rays = np.concatenate([_mixed(sph, max(n - len(extra), 1), seed), extra])
    return rays[rng.permutation(len(rays))[:n]]


WALK_SCENES = [0, 1, 12, 64, 65, 200, "c5"]


def walk_batch(name):
    sph, lg = scene_with_lights(name)
    return sph, lg, mixed_rays(sph, lg, 1500 if name == "c5" else 3000, 300 + len(sph))


@functools.lru_cache(maxsize=None)
def plain_colours(name, S, sem=0):
    """walk 0 of the scene's batch, computed once and left unchanged."""
    import rtg_amd as R
    sph, lg, rays = walk_batch(name)
    col = R.raytrace_host(sph, lg, rays, stack_size=S, semantics=sem, walk=0, threads=THREADS)
    col.setflags(write=False)
    return col


def deep_stack(name):
    return 8 if name == "c5" else 6


@pytest.mark.parametrize("name", WALK_SCENES)
def test_kernel_path_equals_plain_loops(rtg, name):
    sph, lg, rays = walk_batch(name)
    cols = {}
    for S in (1, 2, deep_stack(name)):
        for sem in ((0, 1) if S == 2 else (0,)):
            want = plain_colours(name, S, sem)
            got = rtg.raytrace_host(sph, lg, rays, stack_size=S, semantics=sem, walk=1,
                                    threads=THREADS)
            bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
            assert not len(bad), (S, sem, len(bad), int(bad[0]), rays[bad[0]], got[bad[0]],
                                  want[bad[0]])
            if sem == 0:
                cols[S] = want
    deep = cols[deep_stack(name)]
    # the conditions: the batch hits, the recursion is reached, colours are lit
    if len(sph) >= 12:
        hits = rtg.intersect_host(sph, rays, walk=0, threads=THREADS)
        assert (hits["id"] >= 0).mean() > 0.1
    if len(sph) >= 2:
        assert (deep.view(np.uint32) != cols[2].view(np.uint32)).any(), "no ray went deeper than S = 2"
        assert (np.nan_to_num(deep) > 0).any()


# ---- 3b. every stack size (the dispatch by S is a table: stack_kernels, with_stack) ----

STACK_SIZES = tuple(range(1, 17))
STACK_SCENES = [12, 65]  # flat, and the smallest scene with a BVH
STACK_N = 130  # on the device: two full waves and a two-lane tail
STACK_W = STACK_H = 9  # the frame of the primary rays; test_camera_host.py poses the same frame
# Neighbouring sizes S = k and k + 1 whose walk-0 colours of stack_batch differ
# in at least one word, so that the batch catches a swap of the two table
# entries.  A condition on the inputs, looked up when the batches were chosen
# (scene 12: k = 1 .. 12, scene 65: k = 1 .. 10) and kept by the assert below
# for k = 1 .. 10 on both; S = 6 is the reference's size.  For larger k every
# size is still pinned to the plain loops and, on the primary rays, to the
# oracle at that S, but no ray of these batches goes that deep, so the test
# cannot catch a swap of two sizes above 11 that trace these rays alike.
STACK_TOLD_APART = range(1, 11)


def stack_batch(name):
    """(spheres, lights, the first STACK_N rays of the scene's walk batch)."""
    sph, lg, rays = walk_batch(name)
    return sph, lg, rays[:STACK_N]


@functools.lru_cache(maxsize=None)
def stack_colours(name, S, sem=0):
    """walk 0 of stack_batch at stack size S, computed once and left unchanged
    (test_gpu_raytrace.py compares the device against it)."""
    import rtg_amd as R
    sph, lg, rays = stack_batch(name)
    col = R.raytrace_host(sph, lg, rays, stack_size=S, semantics=sem, walk=0, threads=THREADS)
    col.setflags(write=False)
    return col


@pytest.mark.parametrize("S", STACK_SIZES)
@pytest.mark.parametrize("name", STACK_SCENES)
def test_every_stack_size(rtg, oracle, name, S):
    sph, lg, rays = stack_batch(name)
    assert len(rays) == STACK_N
    want = stack_colours(name, S)
    got = rtg.raytrace_host(sph, lg, rays, stack_size=S, walk=1, threads=THREADS)
    assert got.tobytes() == want.tobytes(), (S, first_mismatch(got, want))
    prim = raygen.primary(STACK_W, STACK_H)
    col = rtg.raytrace_host(sph, lg, prim, stack_size=S, walk=0, threads=THREADS)
    with np.errstate(invalid="ignore"):
        fb = (F(0) + col * F(1)).reshape(STACK_H, STACK_W, 3)
    ref = oracle.render(sph, lg, STACK_W, STACK_H, S, aa=1.0)
    assert bits_equal(fb, ref), (S, first_mismatch(fb, ref))
    if S in STACK_TOLD_APART:
        assert want.tobytes() != stack_colours(name, S + 1).tobytes(), \
            f"S = {S} and {S + 1} trace this batch alike"


def test_some_colour_of_the_batches_has_a_nan_word(rtg):
    """Across the scenes of the test above some colour holds a NaN word (the
    reference's frames hold thousands: golden.json nan_values), so walk 1's
    NaNs are compared too."""
    assert any(np.isnan(plain_colours(name, deep_stack(name))).any() for name in WALK_SCENES)


def test_nan_words_are_canonical(rtg):
    """NaN words come out as 0xFFC00000, every other word as computed (the
    golden comparison of test 2 covers those; a -0 cannot be provoked here:
    every sum of rayTrace starts from +0, and +0 + -0 is +0)."""
    sph, lg = scene_with_lights("reference")
    rays, _ = sample_rays(96, 54)
    for walk in (0, 1):
        col = rtg.raytrace_host(sph, lg, rays, stack_size=6, walk=walk, threads=THREADS)
        nan = np.isnan(col)
        assert nan.any() and (col.view(np.uint32)[nan] == 0xFFC00000).all()


# ---- 4. argument errors ----

def test_argument_errors(rtg):
    L = rtg.lib()
    sph, lg = scene_with_lights("reference")
    rays = raygen.primary(4, 4)
    out = np.full((16, 3), 7.0, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def call(spheres=P(sph), n_sph=len(sph), lights=P(lg), n_lg=len(lg), src=P(rays), n=16, S=6,
             sem=0, dst=P(out), walk=0, threads=1):
        rc = L.rtg_raytrace_host(spheres, n_sph, lights, n_lg, src, n, S, sem, dst, walk, threads)
        return rc, L.rtg_last_error().decode()

    for kw, msg in ((dict(src=None), "null ray buffer"),
                    (dict(dst=None), "null colour buffer"),
                    (dict(spheres=None), "null scene array"),
                    (dict(lights=None), "null scene array"),
                    (dict(S=0), "stackSize 0 outside"),
                    (dict(S=17), "stackSize 17 outside"),
                    (dict(sem=2), "semantics 2"),
                    (dict(sem=-1), "semantics -1"),
                    (dict(walk=2), "walk 2"),
                    (dict(walk=-1), "walk -1")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)  # RTG_ERR_INVALID
    assert (out == 7.0).all()
    rc, err = call(n=0)  # an empty batch: RTG_OK, nothing written
    assert rc == 0 and err == "" and (out == 7.0).all()
    rc, err = call(n_sph=0, spheres=None, n_lg=0, lights=None)  # an empty scene is a scene
    assert rc == 0 and (out == 0).all()
    with pytest.raises(rtg.RtgError, match="walk 5"):
        rtg.raytrace_host(sph, lg, rays, walk=5)
    assert rtg.raytrace_host(sph, lg, rays[:0]).shape == (0, 3)
    # record arrays and (N, 6) floats are the same batch
    a = rtg.raytrace_host(sph, lg, rays)
    b = rtg.raytrace_host(sph, lg, rays.view(rtg.RAY_DTYPE).reshape(-1))
    assert a.shape == (16, 3) and a.dtype == F and a.tobytes() == b.tobytes()
