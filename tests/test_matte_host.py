"""CPU tests of direct light and containment (rtg_matte*, rtg_contains*,
include/rtg.h): no GPU.  Every comparison is on words with NaN canonicalised,
bit for bit.

  1. the definition: matte_host(walk 0) equals a numpy float32 restatement,
     one operation a line, with the line of sight taken from
     visible_host(walk 0) on the segments (P, L): sums and masks;
  2. the pin to the reference: on a scene whose spheres are opaque, white and
     matte, rayTrace is calculateMatte of its first hit, so raytrace_host ==
     matte_host(intersect_host) ray by ray and render_camera_host(aa 1) ==
     the matte of camera_rays_host's hits for a whole frame;
  3. the kernel's own path (walk 1) equals the plain loops (walk 0) on every
     scene, light set and size, and on every hostile scene;
  4. non-vacuity, on the walk-0 answers alone;
  5. containment: restatement, walk 1 == walk 0, its own non-vacuity;
  6. argument checks, thread independence, the empty batch.

Scenes, records, light sets, points and the plain-loop answers are
mattegen.py's; test_gpu_matte.py holds the device to the same answers.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import hostile
import mattegen as G
import raygen
from mattegen import LIGHT_SETS, N_POINTS, SCENES, SIZES
from test_raytrace_host import THREADS

PAD = 64
FILL32 = 0x5A5A5A5A
FILL64 = 0x5A5A5A5A5A5A5A5A
WITH_SPHERES = [s for s in SCENES if s != "none"]
PINNED = ["reference", 12, 40, "base65", "base150", "c5"]


def _raw_matte(rtg, sph, lg, h, n, walk, threads=THREADS, mask=True):
    """rtg_matte_host on the first n records into pre-filled destinations PAD
    records longer than the result; the tails must stay."""
    sph = np.ascontiguousarray(sph, rtg.SPHERE_DTYPE)
    lg = np.ascontiguousarray(lg, rtg.LIGHT_DTYPE)
    h = np.ascontiguousarray(h, rtg.HIT_DTYPE)
    out = np.full((n + PAD) * 3, FILL32, np.uint32)
    lit = np.full(n + PAD, FILL64, np.uint64)
    rc = rtg.lib().rtg_matte_host(rtg._ptr(sph), len(sph), rtg._ptr(lg), len(lg), rtg._ptr(h), n,
                                  rtg._ptr(out), rtg._ptr(lit) if mask else None, walk, threads)
    assert rc == 0, rtg.lib().rtg_last_error()
    assert (out[3 * n:] == FILL32).all(), "sums past the batch were written"
    assert (lit[n:] == FILL64).all(), "masks past the batch were written"
    if not mask:
        assert (lit == FILL64).all(), "masks were written without a mask buffer"
    return out[:3 * n].view(np.float32).reshape(n, 3), lit[:n]


def _raw_contains(rtg, sph, pts, n, walk, threads=THREADS):
    sph = np.ascontiguousarray(sph, rtg.SPHERE_DTYPE)
    pts = np.ascontiguousarray(pts, np.float32)
    out = np.full(n + PAD, FILL32, np.uint32)
    rc = rtg.lib().rtg_contains_host(rtg._ptr(sph), len(sph), rtg._ptr(pts), n, rtg._ptr(out), walk,
                                     threads)
    assert rc == 0, rtg.lib().rtg_last_error()
    assert (out[n:] == FILL32).all(), "indices past the batch were written"
    return out[:n].view(np.int32)


def _restated(rtg, sph, lg, h):
    vis = rtg.visible_host(sph, G.segments(h, lg), walk=0, threads=THREADS)
    return G.restate(h, lg, vis.reshape(len(h), len(lg)))


# ---- 1. the definition ----

@pytest.mark.parametrize("name", SCENES)
def test_plain_loops_equal_the_numpy_restatement(rtg, name):
    sph, h = G.scene(name), G.hits(name)
    for kind in LIGHT_SETS:
        lg = G.lights(name, kind)
        out, lit = G.want(name, kind)
        sums, masks, _ = _restated(rtg, sph, lg, h)
        assert G.same_words(out, sums) is None, (kind, G.same_words(out, sums))
        assert G.same_masks(lit, masks) is None, (kind, G.same_masks(lit, masks))
        assert not out[h["id"] < 0].view(np.uint32).any() and not lit[h["id"] < 0].any()


def test_batches_hold_what_they_should(rtg):
    """Hits and misses in every wave, the hand-made records, the 70-light set's
    special entries, and lights past the mask that reach a point."""
    for name in SCENES:
        h = G.hits(name)
        for w0 in (0, 64, 128):
            ids = h["id"][w0:w0 + 64]
            assert (ids >= 0).any() and (ids < 0).any(), (name, w0)
        assert h[1]["id"] == -1 and np.isnan(h[1]["point"]).all()
        assert tuple(h[2]["normal"]) == (0.0, 0.0, -1.0) and h[2]["id"] >= 0
        assert tuple(h[4]["normal"]) == (0.5, 2.0, -0.25)  # not a unit normal
        assert h[G.BIG_ID_AT]["id"] == 1 << 30 and np.isfinite(h[G.BIG_ID_AT]["point"]).all()
        lg = G.lights(name, "m70")
        assert len(lg) == 70
        assert (lg["pos"][G.AT_CENTRE] == G.aogen.ray_scene(name)["pos"][0]).all()
        assert (lg["col"][G.ODD_COLOUR] < 0).any() and (lg["col"][G.ODD_COLOUR] == 0).any()
        assert ((h["point"] == lg["pos"][G.AT_POINT]).all(1) & (h["id"] >= 0)).any()
        # lights 64..69 add to the sum and set no bit: dropping them changes sums only
        out, lit = G.want(name, "m70")
        out64, lit64 = rtg.matte_host(G.scene(name), lg[:64], h, walk=0, threads=THREADS, mask=True)
        assert G.same_masks(lit, lit64) is None
        assert G.same_words(out, out64) is not None, name
        assert (lit >> np.uint64(32)).any()  # the mask's high word is used


# ---- 2. the pin to the reference ----

@pytest.mark.parametrize("name", PINNED)
def test_white_scene_raytrace_is_the_matte_of_the_first_hit(rtg, name):
    white, lg = G.whitened(G.scene(name)), G.lights(name)
    rng = np.random.default_rng(77)
    rays = np.concatenate([raygen.surface(rng, white, 300), raygen.primary(16, 12)])
    col = rtg.raytrace_host(white, lg, rays, stack_size=6, semantics=0, walk=0, threads=THREADS)
    h = rtg.intersect_host(white, rays, walk=0, threads=THREADS)
    got = rtg.matte_host(white, lg, h, walk=0, threads=THREADS)
    assert G.same_words(got, col) is None, G.same_words(got, col)
    assert not col[h["id"] < 0].view(np.uint32).any()  # a miss is (0, 0, 0) on both sides
    lit = int((G.canon(col) << 1).any(1).sum())
    assert lit >= 20, lit  # the identity is about lit points, not about zeros


@pytest.mark.parametrize("name", PINNED)
def test_white_scene_frame_is_the_matte_of_its_primary_hits(rtg, name):
    white, lg = G.whitened(G.scene(name)), G.lights(name)
    W, H = 40, 30
    for cam in (rtg.camera_identity(), rtg.camera_look_at(*hostile.POSE)):
        frame = rtg.render_camera_host(white, lg, cam, W, H, alias_factor=1.0, stack_size=6,
                                       walk=0, threads=THREADS)
        rays = rtg.camera_rays_host(cam, W, H, alias_factor=1.0, threads=THREADS)
        h = rtg.intersect_host(white, rays, walk=0, threads=THREADS)
        got = rtg.matte_host(white, lg, h, walk=0, threads=THREADS)
        assert G.same_words(got, frame.reshape(-1, 3)) is None, G.same_words(got, frame)
        assert (G.canon(frame) << 1).any()  # not a black frame


# ---- 3. walk 1 == walk 0 ----

@pytest.mark.parametrize("name", SCENES)
def test_kernel_path_equals_plain_loops(rtg, name):
    sph, h = G.scene(name), G.hits(name)
    for kind in LIGHT_SETS:
        lg = G.lights(name, kind)
        want, want_lit = G.want(name, kind)
        for n in SIZES:
            got, lit = _raw_matte(rtg, sph, lg, h, n, walk=1)
            assert G.same_words(got, want[:n]) is None, (kind, n, G.same_words(got, want[:n]))
            assert G.same_masks(lit, want_lit[:n]) is None, (kind, n)
        got, _ = _raw_matte(rtg, sph, lg, h, N_POINTS, walk=1, mask=False)
        assert G.same_words(got, want) is None, (kind, "no mask")


@pytest.mark.parametrize("n", hostile.SIZES)
def test_kernel_path_equals_plain_loops_on_hostile_scenes(rtg, n):
    """Every hostile.CASES mutation of size n with its own lights, the batch
    test_gpu_matte.py runs."""
    for name in hostile.NAMES:
        sph, lg = hostile.mutated(n, name)
        h = G.aogen.hostile_hits(n, name)
        assert (h["id"] >= 0).any() and (h["id"] < 0).any()
        want, want_lit = rtg.matte_host(sph, lg, h, walk=0, threads=THREADS, mask=True)
        got, lit = rtg.matte_host(sph, lg, h, walk=1, threads=THREADS, mask=True)
        assert G.same_words(got, want) is None, (name, G.same_words(got, want))
        assert G.same_masks(lit, want_lit) is None, (name, G.same_masks(lit, want_lit))
        pts = G.hostile_points(n)
        want_in = rtg.contains_host(sph, pts, walk=0, threads=THREADS)
        got_in = rtg.contains_host(sph, pts, walk=1, threads=THREADS)
        assert got_in.tobytes() == want_in.tobytes(), (name, np.flatnonzero(got_in != want_in)[:4])
        first, count = G.restate_contains(sph, pts)
        assert want_in.tobytes() == first.tobytes(), name
        if name == "dup":  # index ties: the lower index wins
            tied = (count >= 2) & ((want_in == 0) | (want_in == 2))
            assert tied.any() and not np.isin(want_in, (1, 3)).any()


# ---- 4. non-vacuity, on the walk-0 answer with the scene's own lights ----

@pytest.mark.parametrize("name", WITH_SPHERES)
def test_plain_loop_answers_are_not_vacuous(rtg, name):
    sph, h, lg = G.scene(name), G.hits(name), G.lights(name)
    out, _ = G.want(name)
    real = h["id"] >= 0
    lit_share = float((G.canon(out)[real] << 1).any(1).mean())
    assert 0.2 < lit_share < 0.8, lit_share
    vis = rtg.visible_host(sph, G.segments(h, lg), walk=0, threads=THREADS).reshape(len(h), len(lg))
    _, _, facing = G.restate(h, lg, vis)
    shadowed = facing & (vis == 0)
    if name == "reference":
        assert shadowed.sum() >= 1
    else:
        assert shadowed.sum() / facing.sum() >= 0.1, shadowed.sum() / facing.sum()


# ---- 5. containment ----

@pytest.mark.parametrize("name", SCENES)
def test_containment(rtg, name):
    sph, pts = G.scene(name), G.points(name)
    want = G.want_contains(name)
    first, count = G.restate_contains(sph, pts)
    assert want.tobytes() == first.tobytes(), np.flatnonzero(want != first)[:4]
    for n in SIZES:
        for walk in (0, 1):
            got = _raw_contains(rtg, sph, pts, n, walk)
            assert got.tobytes() == want[:n].tobytes(), (n, walk, np.flatnonzero(got != want[:n])[:4])
    assert want[np.isnan(pts).any(1)].tolist() == [-1] and want[-1] == -1  # NaN; 1e30 away
    if name == "none":
        assert (want == -1).all()
        return
    assert 0.3 < float((want >= 0).mean()) < 0.95, float((want >= 0).mean())
    if name in (40, "base150", "c5"):
        assert (count >= 2).any()
        assert (want[count >= 2] >= 0).all()


# ---- 6. argument checks, threads, the empty batch ----

def test_argument_errors(rtg):
    L = rtg.lib()
    P = rtg._ptr
    sph, lg = G.scene("reference"), G.lights("reference")
    h = G.hits("reference").copy()
    pts = G.points("reference").copy()
    out = np.zeros((len(h), 3), np.float32)
    lit = np.zeros(len(h), np.uint64)
    idx = np.zeros(len(pts), np.int32)

    def matte(hits=h, n=len(h), dst=out, mask=lit, walk=0, spheres=sph, lights=lg):
        return L.rtg_matte_host(P(spheres) if spheres is not None else None, len(sph),
                                P(lights) if lights is not None else None, len(lg),
                                P(hits) if hits is not None else None, n,
                                P(dst) if dst is not None else None,
                                P(mask) if mask is not None else None, walk, 1)

    def contains(points=pts, n=len(pts), dst=idx, walk=0, spheres=sph):
        return L.rtg_contains_host(P(spheres) if spheres is not None else None, len(sph),
                                   P(points) if points is not None else None, n,
                                   P(dst) if dst is not None else None, walk, 1)

    def bad(rc, msg):
        assert rc == -1
        text = L.rtg_last_error().decode()
        assert text and msg in text, text

    assert matte() == 0 and contains() == 0 and L.rtg_last_error() == b""
    assert out.any() and lit.any() and idx.any()
    out[:], lit[:], idx[:] = 0, 0, 0
    bad(matte(hits=None), "matte: null hit buffer")
    bad(matte(dst=None), "matte: null output buffer")
    bad(matte(n=1 << 32), "points (at most 2^32 - 1)")
    bad(matte(walk=2), "walk 2")
    bad(matte(walk=-1), "walk -1")
    bad(matte(spheres=None), "null scene array")
    bad(matte(lights=None), "null scene array")
    bad(contains(points=None), "contains: null point buffer")
    bad(contains(dst=None), "contains: null output buffer")
    bad(contains(n=1 << 32), "points (at most 2^32 - 1)")
    bad(contains(walk=2), "walk 2")
    bad(contains(spheres=None), "null scene array")
    assert matte(n=0) == 0 and contains(n=0) == 0
    assert not out.any() and not lit.any() and not idx.any()  # nothing written by a refused call
    assert matte(mask=None) == 0 and out.any() and not lit.any()  # the mask is optional
    with pytest.raises(rtg.RtgError, match="walk 3"):
        rtg.matte_host(sph, lg, h, walk=3)
    with pytest.raises(rtg.RtgError, match="walk 3"):
        rtg.contains_host(sph, pts, walk=3)


def test_result_does_not_depend_on_threads(rtg):
    for name in ("reference", "base65"):
        sph, lg, h = G.scene(name), G.lights(name, "m70"), G.hits(name)
        want, want_lit = G.want(name, "m70")
        for walk in (0, 1):
            for threads in (1, 3, 0, -2):
                got, lit = rtg.matte_host(sph, lg, h, walk=walk, threads=threads, mask=True)
                assert G.same_words(got, want) is None and G.same_masks(lit, want_lit) is None
                got = rtg.contains_host(sph, G.points(name), walk=walk, threads=threads)
                assert got.tobytes() == G.want_contains(name).tobytes()


def test_empty_batch(rtg):
    sph, lg = G.scene("reference"), G.lights("reference")
    empty = np.zeros(0, rtg.HIT_DTYPE)
    for walk in (0, 1):
        out, lit = rtg.matte_host(sph, lg, empty, walk=walk, mask=True)
        assert out.shape == (0, 3) and lit.shape == (0,)
        assert rtg.contains_host(sph, np.zeros((0, 3), np.float32), walk=walk).shape == (0,)
    assert ctypes.sizeof(ctypes.c_ulonglong) == 8
