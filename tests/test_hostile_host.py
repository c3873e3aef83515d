"""CPU tests over hostile SCENES (tests/hostile.py): NaN, infinite, zero,
negative and huge spheres, the camera or a light inside a sphere, coincident
spheres, out-of-range materials and colours.  Scene data decides which tables
rtg_scene_pack.h builds (masks or none, BVH or none, sphere lists or none), so
these scenes run whole frames and batches down paths that finite scenes reach
only lane by lane.  No GPU:

  1. the kernel's traversal compiled for the host (tests/hostsim, the sample
     and the tile kernel's variants) equals the oracle's frame;
  2. the batch queries' kernel path (walk 1) equals the plain loops (walk 0);
  3. the posed camera's walk 1 equals walk 0;
  4. the G-buffer's host form equals its numpy restatement;
  5. the ray order's keys equal a numpy restatement over the mutated scene;
  6. a scene file round-trips every mutated scene bit for bit;
  7. the 1100-sphere scene (global materials, no BVH).

Every comparison is bit for bit.  test_gpu_hostile.py holds the device to the
same references.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import hostile
from conftest import bits_equal, first_mismatch
from hostile import CASES, IDS
from raygen import diff_hits
from test_gbuffer_host import _diff, _same, restate
from test_oracle import _hostsim_render, hostsim  # noqa: F401  (the fixture)
from test_raytrace_host import THREADS

W, H, AA, S = 40, 30, 3.0, 6


# ---- references, computed once and left unchanged ----

_frames = {}


def oracle_frame(oracle, n, name, w=W, h=H, s=S, aa=AA, cl=False):
    """The oracle's frame of a mutated scene, lit (hostile.assert_lit)."""
    key = (n, name, w, h, s, aa, cl)
    if key not in _frames:
        sph, lg = hostile.mutated(n, name)
        fb = (oracle.render_cl if cl else oracle.render)(sph, lg, w, h, s, aa=aa)
        hostile.assert_lit(fb)
        fb.setflags(write=False)
        _frames[key] = fb
    return _frames[key]


@functools.lru_cache(maxsize=None)
def walk0(n, name):
    """(hits, visible) of base scene n's batches against the mutated scene by
    the plain loops."""
    import rtg_amd as R
    sph, _ = hostile.mutated(n, name)
    rays, segs = hostile.batches(n)
    return (R.intersect_host(sph, rays, walk=0, threads=THREADS),
            R.visible_host(sph, segs, walk=0, threads=THREADS))


@functools.lru_cache(maxsize=None)
def colours0(n, name, s=S, sem=0):
    import rtg_amd as R
    sph, lg = hostile.mutated(n, name)
    return R.raytrace_host(sph, lg, hostile.batches(n)[0], stack_size=s, semantics=sem, walk=0,
                           threads=THREADS)


def semantics_of(name):
    return (0, 1) if name in ("mat", "all") else (0,)


def check_non_vacuous(n, name):
    """hostile.py's conditions on the plain-loop answers of (n, name)."""
    hits, vis = walk0(n, name)
    hostile.assert_fractions(hits, vis)
    hostile.assert_hits_differ(name, hits, walk0(n, "base")[0])


# ---- 1. hostsim == oracle ----

@pytest.mark.parametrize("n,name", CASES, ids=IDS)
def test_kernel_traversal_equals_oracle(hostsim, oracle, rtg, n, name):  # noqa: F811
    sph, lg = hostile.mutated(n, name)
    runs = [(S, AA)] + ([(1, AA), (12, AA), (S, 2.5)] if name == "all" else [])
    try:
        for variant in (0, 9):
            hostsim.hostsim_set_variant(variant)
            for s, aa in runs:
                want = oracle_frame(oracle, n, name, s=s, aa=aa)
                got = _hostsim_render(hostsim, sph, lg, W, H, s, aa=aa)
                assert bits_equal(got, want), (variant, s, aa, first_mismatch(got, want))
    finally:
        hostsim.hostsim_set_variant(0)


def test_some_reference_answers_hold_nan(oracle, rtg):
    """The set is not NaN-free: the oracle's frames and the plain loops'
    colours of `mat` and `col` carry NaN words the code under test must place."""
    frames = sum(hostile.nan_words(oracle_frame(oracle, n, name))
                 for n in hostile.SIZES for name in ("mat", "col"))
    cols = sum(hostile.nan_words(colours0(n, name)) for n in hostile.SIZES
               for name in ("mat", "col"))
    assert frames > 0 and cols > 0, (frames, cols)


# ---- 2. walk 1 == walk 0 ----

@pytest.mark.parametrize("n,name", CASES, ids=IDS)
def test_walk1_equals_walk0(rtg, n, name):
    """With closest_hit4 giving ties to the higher index (`sm <= minT`), the
    cases that fail are n65-all, n150-rnan, -rinf, -cnan, -cinf, -big31,
    -big2_57 and -all, the posed camera's n65-all and the large scene: the
    scenes without a BVH above 64 spheres, and no other."""
    sph, lg = hostile.mutated(n, name)
    rays, segs = hostile.batches(n)
    check_non_vacuous(n, name)
    hits, vis = walk0(n, name)
    got = rtg.intersect_host(sph, rays, walk=1, threads=THREADS)
    assert got.tobytes() == hits.tobytes(), diff_hits(got, hits)
    got = rtg.visible_host(sph, segs, walk=1, threads=THREADS)
    bad = np.flatnonzero(got != vis)
    assert not len(bad), f"{len(bad)} segments differ, first {bad[0]}: {segs[bad[0]]}"
    for sem in semantics_of(name):
        want = colours0(n, name, S, sem)
        got = rtg.raytrace_host(sph, lg, rays, stack_size=S, semantics=sem, walk=1,
                                threads=THREADS)
        assert got.tobytes() == want.tobytes(), (sem, first_mismatch(got, want))
        assert (want.view(np.uint32) << 1).any(), "black batch"


# ---- 3. the posed camera ----

@pytest.mark.parametrize("n,name", [c for c in CASES if c[0] > 64],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] > 64])
def test_posed_camera_walk1_equals_walk0(rtg, n, name):
    sph, lg = hostile.mutated(n, name)
    cam = rtg.camera_look_at(*hostile.POSE)
    want = rtg.render_camera_host(sph, lg, cam, 32, 24, stack_size=S, walk=0, threads=THREADS)
    got = rtg.render_camera_host(sph, lg, cam, 32, 24, stack_size=S, walk=1, threads=THREADS)
    assert got.tobytes() == want.tobytes(), first_mismatch(got, want)
    assert (want.view(np.uint32) << 1).any(), "black frame"


# ---- 4. the G-buffer ----

@pytest.mark.parametrize("name", hostile.NAMES)
def test_gbuffer_host_equals_restatement(rtg, name):
    sph, _ = hostile.mutated(8, name)
    got = rtg.gbuffer_host(sph, 24, 18, -4.0, 2.0)
    want = restate(rtg, sph, 24, 18, -4.0, 2.0)
    assert _same(got, want), _diff(got, want)
    assert (want["hits"] > 0).any()


# ---- 5. the ray order ----

def _check_keys(rtg, sph, n):
    rays, segs = hostile.batches(n)
    for kind, batch in ((rtg.ORDER_RAYS, rays), (rtg.ORDER_SEGMENTS, segs)):
        order, keys = rtg.ray_order_host(sph, batch, kind=kind, keys=True, threads=THREADS)
        want = hostile.restate_keys(sph, batch, kind)
        bad = np.flatnonzero(keys != want)
        assert not len(bad), (kind, f"{len(bad)} keys differ, first {bad[0]}: {batch[bad[0]]}")
        assert (order == hostile.restate_order(want)).all(), kind
        assert len(np.unique(want)) > len(batch) // 8  # not a constant key


@pytest.mark.parametrize("n,name", CASES, ids=IDS)
def test_ray_order_keys_equal_restatement(rtg, n, name):
    """With key_bounds taking non-finite spheres into the box, rnan, rinf, cnan
    and cinf fail at every size."""
    _check_keys(rtg, hostile.mutated(n, name)[0], n)


def test_ray_order_keys_of_a_nan_sphere(rtg):
    """Every sphere non-finite: the key box is [-1, 1]^3, the empty scene's."""
    sph, _ = hostile.nan_sphere_scene()
    _check_keys(rtg, sph, 8)
    rays = hostile.batches(8)[0]
    none = np.zeros(0, rtg.SPHERE_DTYPE)
    assert (rtg.ray_order_host(sph, rays, keys=True)[1]
            == rtg.ray_order_host(none, rays, keys=True)[1]).all()
    lo, hi = hostile.restate_key_bounds(sph)
    assert (lo == -1).all() and (hi == 1).all()
    # a non-finite sphere is skipped: `cnan` keeps the box of the other seven
    lo, hi = hostile.restate_key_bounds(hostile.mutated(8, "cnan")[0])
    want = hostile.restate_key_bounds(hostile.base(8)[0][1:])
    assert (lo == want[0]).all() and (hi == want[1]).all() and np.isfinite(lo).all()


# ---- 6. the scene file ----

@pytest.mark.parametrize("n,name", CASES, ids=IDS)
def test_scene_file_round_trip(rtg, tmp_path, n, name):
    sph, lg = hostile.mutated(n, name)
    path = str(tmp_path / "s.scene")
    rtg.save_scene_file(path, sph, lg)
    sph2, lg2 = rtg.load_scene_file(path)
    assert sph2.tobytes() == sph.tobytes() and lg2.tobytes() == lg.tobytes()


def test_scene_file_carries_the_special_values(rtg):
    """The set above holds NaN, both infinities and the negative zero."""
    words = np.concatenate([np.concatenate([a.view(np.uint32) for a in hostile.mutated(8, name)])
                            for name in hostile.NAMES])
    for bits in (0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000):
        assert (words == bits).any(), hex(bits)


# ---- 7. the large scene ----

def test_large_scene(hostsim, oracle, rtg):  # noqa: F811
    n = hostile.LARGE_N
    _, sph, lg = hostile.large()
    rays, segs = hostile.batches(n)
    assert len(sph) == n and len(rays) == 2000
    hostsim.hostsim_set_variant(0)
    want = oracle_frame(oracle, n, "cnan", 24, 14, 4)
    got = _hostsim_render(hostsim, sph, lg, 24, 14, 4)
    assert bits_equal(got, want), first_mismatch(got, want)
    check_non_vacuous(n, "cnan")
    hits, vis = walk0(n, "cnan")
    got = rtg.intersect_host(sph, rays, walk=1, threads=THREADS)
    assert got.tobytes() == hits.tobytes(), diff_hits(got, hits)
    assert (rtg.visible_host(sph, segs, walk=1, threads=THREADS) == vis).all()
    want = colours0(n, "cnan", 4)
    got = rtg.raytrace_host(sph, lg, rays, stack_size=4, walk=1, threads=THREADS)
    assert got.tobytes() == want.tobytes(), first_mismatch(got, want)
