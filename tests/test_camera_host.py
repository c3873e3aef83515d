"""CPU tests of the posed camera's host forms (rtg_camera_*, rtg_render_camera_host,
csrc/rtg_camera.hip): rays and frames from any viewpoint.

  1. the identity pose's rays are the render's sample rays, word for word;
  2. rtg_camera_look_at and the generator equal a numpy float32 restatement of
     the two formulas of rtg.h, for ordinary poses and for NaN, infinite and
     zero basis vectors;
  3. the identity pose's frame, walk 0 and walk 1, is the reference's own
     golden small frame;
  4. posed frames: walk 0 is the fold of rtg_raytrace_host(walk 0) over the
     restated rays (the normative yardstick), walk 1 equals walk 0, with
     conditions that keep both from passing on black frames; and a 9 x 9
     frame at every stack size 1 .. 16, each size pinned to the plain loops
     and the oracle at that size;
  5. picking from a pose: the generator plus rtg_intersect_host;
  6. the argument errors of the contract;
  7. aliasFactor <= 0: a +0 frame and no rays.

All comparisons are bit for bit (conftest.bits_equal).  test_gpu_camera.py
shares the poses, the restatement and the host frames of this file.
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import pytest

import raygen
from conftest import GOLDEN, bits_equal, first_mismatch, load_f32, load_scene
from test_raytrace_host import (STACK_H, STACK_SCENES, STACK_SIZES, STACK_W, THREADS, fold,
                                sample_rays, scene_with_lights)

F = np.float32


# ---- the two formulas of rtg.h in numpy float32 ----

def _vnorm(v):
    with np.errstate(all="ignore"):
        l = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return [l * v[0], l * v[1], l * v[2]]


def _cross(a, b):
    with np.errstate(all="ignore"):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def restate_look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """back = vnorm(eye - target), right = vnorm(cross(up, back)), up' =
    cross(back, right), all in float32: (4, 3) float32 (eye, right, up, back)."""
    e, t, u = ([F(q) for q in v] for v in (eye, target, up))
    with np.errstate(all="ignore"):
        back = _vnorm([e[q] - t[q] for q in range(3)])
    right = _vnorm(_cross(u, back))
    return np.array([e, right, _cross(back, right), back], F)


def restate_rays(cam, W, H, aa, zoom, rows=None):
    """v.q = (rx * right.q + ry * up.q) + zoom * back.q, dir = vnorm(v), origin
    = eye, with (rx, ry) as test_raytrace_host.sample_rays forms them; pixel
    order, samples i outer, j inner.  (H*W*nAA*nAA, 6) float32 and nAA*nAA.
    rows: only those rows of the frame, in the order given."""
    cam = np.asarray(cam, F).reshape(4, 3)
    aa, zoom = F(aa), F(zoom)
    xs, ys, asp = F(16) / F(W), F(12) / F(H), F(16) / F(12)
    with np.errstate(all="ignore"):
        st = xs / aa
    halfW, halfH = F(W) * F(0.5), F(H) * F(0.5)
    nAA = 0
    while F(nAA) < aa:
        nAA += 1
    y, x, i, j = np.meshgrid(np.arange(H) if rows is None else np.asarray(rows, np.int64),
                             np.arange(W), np.arange(nAA), np.arange(nAA), indexing="ij")
    with np.errstate(all="ignore"):
        rx = ((x.astype(F) - halfW) * xs + j.astype(F) * st) * asp
        ry = (halfH - y.astype(F)) * ys + i.astype(F) * st
        eye, right, up, back = cam
        v = [(rx * right[q] + ry * up[q]) + zoom * back[q] for q in range(3)]
        assert all(c.dtype == F for c in v)
        d = _vnorm(v)
    out = np.zeros((x.size, 6), F)
    out[:, :3] = eye
    for q in range(3):
        out[:, 3 + q] = d[q].reshape(-1)
    return out, nAA * nAA


def cam12(rec):
    """A CAMERA_DTYPE record as (4, 3) float32."""
    return np.asarray(rec).reshape(1).view(F).reshape(4, 3).copy()


# ---- the poses of the posed-frame tests (shared with test_gpu_camera.py) ----

POSES = ("orbit", "inside", "far", "in_clearest", "raw")


def pose(name, scene):
    """(12 floats of the pose, zoom) for the scene's spheres.  The geometry is
    laid out in float64 and rounded to float32 once; look_at is the library's
    (test 2 pins it to the restatement)."""
    import rtg_amd as R
    sph = scene_with_lights(scene)[0]
    lo, hi = raygen.bounds(sph)
    c = (lo + hi) * 0.5
    s = float((hi - lo).max())
    if name == "orbit":
        return cam12(R.camera_look_at(c + 1.2 * s * np.array([0.6, 0.35, 0.72]), c)), -12.0
    if name == "inside":
        return cam12(R.camera_look_at(c, c + np.array([1.0, -0.2, -0.5]))), -4.0
    if name == "far":
        u = np.array([0.3, 0.2, 1.0])
        return cam12(R.camera_look_at(c + 8.0 * s * u / np.linalg.norm(u), c)), -96.0
    if name == "in_clearest":
        k = int(np.argmin(sph["material"]["opacity"]))
        return cam12(R.camera_look_at(sph["pos"][k], c + np.array([0.3, 0.1, 0.2]))), -4.0
    assert name == "raw"  # a rolled, scaled, non-unit basis, not run through look_at
    return np.array([c + s * np.array([0.0, 0.0, 1.0]), [0, 2, 0], [-1, 0, 0], [0, 0, 0.5]], F), -12.0


POSED_SCENES = ["reference", 12, 200, "c5"]
PW, PH, PAA, PS = 48, 36, 2.0, 6


def posed_cases(scenes=POSED_SCENES):
    return [(sc, p) for sc in scenes for p in POSES if not (p == "in_clearest" and sc == 200)]


@functools.lru_cache(maxsize=None)
def posed_frame(scene, name, sem=0, W=PW, H=PH, aa=PAA, S=PS):
    """render_camera_host(walk 0) of a pose, computed once and left unchanged."""
    import rtg_amd as R
    sph, lg = scene_with_lights(scene)
    cam, zoom = pose(name, scene)
    fb = R.render_camera_host(sph, lg, cam, W, H, zoom, aa, S, semantics=sem, walk=0,
                              threads=THREADS)
    fb.setflags(write=False)
    return fb


@functools.lru_cache(maxsize=None)
def identity_frame(scene, zoom, sem=0):
    import rtg_amd as R
    sph, lg = scene_with_lights(scene)
    fb = R.render_camera_host(sph, lg, R.camera_identity(), PW, PH, zoom, PAA, PS, semantics=sem,
                              walk=0, threads=THREADS)
    fb.setflags(write=False)
    return fb


def lit_fraction(fb):
    """Pixels with a nonzero (or NaN) word."""
    return float((fb != 0).any(-1).mean())


# ---- 1. the identity pose's rays are the render's ----

@pytest.mark.parametrize("W,H", [(96, 54), (7, 5)])
@pytest.mark.parametrize("aa,zoom", [(1.0, -4.0), (2.0, -4.0), (2.5, -4.0), (3.0, -4.0),
                                     (3.0, -1.5)])
def test_identity_rays_are_the_renders(rtg, W, H, aa, zoom):
    want, nS = sample_rays(W, H, aa, zoom)
    assert rtg.camera_sample_count(aa) ** 2 == nS
    for threads in (1, THREADS):
        got = rtg.camera_rays_host(rtg.camera_identity(), W, H, zoom, aa, threads=threads)
        assert got.shape == want.shape
        assert got.tobytes() == want.tobytes(), first_mismatch(got, want)  # every zero +0 too


# ---- 2. look_at and the generator against the restatement ----

def test_identity_and_look_at_down_minus_z(rtg):
    ident = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    assert cam12(rtg.camera_identity()).tobytes() == ident.tobytes()
    got = cam12(rtg.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0)))
    assert got.tobytes() == ident.tobytes(), got  # every zero +0


@pytest.mark.parametrize("scene", POSED_SCENES)
def test_look_at_and_rays_equal_the_restatement(rtg, scene):
    sph = scene_with_lights(scene)[0]
    lo, hi = raygen.bounds(sph)
    c, s = (lo + hi) * 0.5, float((hi - lo).max())
    u = np.array([0.3, 0.2, 1.0])
    looks = [(c + 1.2 * s * np.array([0.6, 0.35, 0.72]), c, (0, 1, 0)),
             (c, c + np.array([1.0, -0.2, -0.5]), (0, 1, 0)),
             (c + 8.0 * s * u / np.linalg.norm(u), c, (0.1, 0.9, -0.3)),
             (c, c, (0, 1, 0)),                       # eye == target: a NaN basis, RTG_OK
             (c, c + np.array([0, 3.0, 0]), (0, 1, 0))]  # up parallel to the view
    for eye, target, up in looks:
        got = cam12(rtg.camera_look_at(eye, target, up))
        want = restate_look_at(eye, target, up)
        assert bits_equal(got, want), (eye, target, up, got, want)
    assert np.isnan(cam12(rtg.camera_look_at(c, c))).any()
    for name in POSES:
        if (scene, name) not in posed_cases():
            continue
        cam, zoom = pose(name, scene)
        for W, H, aa in ((PW, PH, PAA), (7, 5, 2.5)):
            got = rtg.camera_rays_host(cam, W, H, zoom, aa, threads=THREADS)
            want, _ = restate_rays(cam, W, H, aa, zoom)
            assert bits_equal(got, want), (name, W, H, aa, first_mismatch(got, want))
            assert np.isfinite(got).all() and (got[:, :3] == cam[0]).all()


# a NaN, an infinite and a zero basis vector (and a NaN eye)
ODD_BASES = [
    [[1, 2, 3], [np.nan, 0, 0], [0, 1, 0], [0, 0, 1]],
    [[1, 2, 3], [1, 0, 0], [0, np.inf, 0], [0, 0, 1]],
    [[1, 2, 3], [1, 0, 0], [0, 1, 0], [0, 0, 0]],
    [[1, 2, 3], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
    [[np.nan, 2, -np.inf], [1, 0, 0], [0, 1, 0], [0, 0, -np.inf]],
]


@pytest.mark.parametrize("k", range(len(ODD_BASES)))
def test_odd_bases_follow_the_arithmetic(rtg, k):
    cam = np.array(ODD_BASES[k], F)
    got = rtg.camera_rays_host(cam, 9, 7, -4.0, 2.0)
    want, nS = restate_rays(cam, 9, 7, 2.0, -4.0)
    assert nS == 4 and bits_equal(got, want), first_mismatch(got, want)
    # (a zero `back` alone leaves the finite direction vnorm((rx, ry, -0)))
    assert np.isfinite(got[:, 3:]).all() == (k == 2)


# ---- 3. pinned to the reference's own frames ----

@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("cfg", ["ref800", "c2", "c3", "c5"])
def test_identity_frame_is_the_golden_small_frame(rtg, golden, cfg, walk):
    c = golden["configs"][cfg]
    sph, lg = load_scene(cfg, c["spheres"], c["lights"])
    W, H = c["small"]["W"], c["small"]["H"]
    assert (W, H, golden["aliasFactor"]) == (96, 54, 3.0)
    fb = rtg.render_camera_host(sph, lg, rtg.camera_identity(), W, H, golden["zoom"],
                                golden["aliasFactor"], c["stack_size"], walk=walk,
                                threads=THREADS)
    want = load_f32(os.path.join(GOLDEN, f"{cfg}.small.f32"), (H, W, 3))
    assert bits_equal(fb, want), first_mismatch(fb, want)


# ---- 4. posed frames ----

@pytest.mark.parametrize("scene,name", posed_cases())
def test_posed_frame_is_the_fold_of_the_batch_call(rtg, scene, name):
    sph, lg = scene_with_lights(scene)
    cam, zoom = pose(name, scene)
    rays, nS = restate_rays(cam, PW, PH, PAA, zoom)
    assert nS == 4
    for sem in (0, 1):
        fb = posed_frame(scene, name, sem)
        col = rtg.raytrace_host(sph, lg, rays, stack_size=PS, semantics=sem, walk=0,
                                threads=THREADS)
        want = fold(col, PW, PH, nS, PAA)
        assert bits_equal(fb, want), (sem, first_mismatch(fb, want))
        nan = np.isnan(fb)
        assert (fb.view(np.uint32)[nan] == 0xFFC00000).all()
        fb1 = rtg.render_camera_host(sph, lg, cam, PW, PH, zoom, PAA, PS, semantics=sem, walk=1,
                                     threads=THREADS)
        assert fb1.tobytes() == fb.tobytes(), (sem, first_mismatch(fb1, fb))
    # the conditions (CPU semantics): lit, and not the identity pose's frame
    fb = posed_frame(scene, name, 0)
    assert lit_fraction(fb) >= (0.02 if name == "raw" else 0.10), lit_fraction(fb)
    ident = identity_frame(scene, zoom)
    differ = float((fb.view(np.uint32) != ident.view(np.uint32)).any(-1).mean())
    assert differ >= 0.05, differ


# ---- 4b. every stack size (the dispatch by S is a table: stack_kernels, with_stack) ----

STACK_POSE, STACK_AA = "in_clearest", 1.0  # from inside the clearest sphere: deep trees
# Neighbouring sizes S = k and k + 1 whose posed walk-0 frames differ in at
# least one word (as STACK_TOLD_APART of test_raytrace_host.py; looked up when
# the pose was chosen: scene 12 k = 1 .. 9, scene 65 k = 1 .. 12).  Above that
# every size is still pinned to the plain loops and the oracle, but the test
# cannot catch a swap of two sizes that trace these 81 pixels alike.
STACK_FRAMES_TOLD_APART = range(1, 10)


@functools.lru_cache(maxsize=None)
def stack_frame(scene, S, sem=0):
    """render_camera_host(walk 0) of the 9 x 9 posed frame at stack size S,
    computed once and left unchanged (test_gpu_camera.py compares the device
    against it): four 8 x 8 tiles on the device, three of them ragged."""
    return posed_frame(scene, STACK_POSE, sem, STACK_W, STACK_H, STACK_AA, S)


@pytest.mark.parametrize("S", STACK_SIZES)
@pytest.mark.parametrize("scene", STACK_SCENES)
def test_every_stack_size(rtg, oracle, scene, S):
    sph, lg = scene_with_lights(scene)
    cam, zoom = pose(STACK_POSE, scene)
    want = stack_frame(scene, S)
    got = rtg.render_camera_host(sph, lg, cam, STACK_W, STACK_H, zoom, STACK_AA, S, walk=1,
                                 threads=THREADS)
    assert got.tobytes() == want.tobytes(), (S, first_mismatch(got, want))
    # the primary rays: the identity pose's frame is the oracle's at that S
    fb = rtg.render_camera_host(sph, lg, rtg.camera_identity(), STACK_W, STACK_H, -4.0, STACK_AA,
                                S, walk=0, threads=THREADS)
    ref = oracle.render(sph, lg, STACK_W, STACK_H, S, aa=1.0)
    assert bits_equal(fb, ref), (S, first_mismatch(fb, ref))
    if S in STACK_FRAMES_TOLD_APART:
        assert want.tobytes() != stack_frame(scene, S + 1).tobytes(), \
            f"S = {S} and {S + 1} trace this frame alike"


# ---- 5. picking from a pose ----

@pytest.mark.parametrize("scene", [12, "c5"])
def test_generator_plus_intersect(rtg, scene):
    sph = scene_with_lights(scene)[0]
    W, H = 64, 48
    rays = rtg.camera_rays_host(rtg.camera_identity(), W, H, -4.0, 1.0, threads=THREADS)
    hits = rtg.intersect_host(sph, rays, walk=0, threads=THREADS).reshape(H, W)
    gb = rtg.gbuffer_host(sph, W, H, -4.0, 1.0, threads=THREADS)
    assert (hits["id"] == gb["id"]).all() and (hits["id"] >= 0).any()
    assert hits["t"].tobytes() == gb["t"].tobytes()
    cam, zoom = pose("orbit", scene)
    rays = rtg.camera_rays_host(cam, W, H, zoom, 1.0, threads=THREADS)
    h0 = rtg.intersect_host(sph, rays, walk=0, threads=THREADS)
    h1 = rtg.intersect_host(sph, rays, walk=1, threads=THREADS)
    assert raygen.diff_hits(h1, h0) is None
    assert (h0["id"] >= 0).mean() > 0.05 and (h0["id"].reshape(H, W) != gb["id"]).any()


# ---- 6. argument errors ----

def test_argument_errors(rtg):
    L = rtg.lib()
    sph, lg = scene_with_lights("reference")
    cam = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    out = np.full((4, 4, 3), 7.0, F)
    rays = np.full((16 * 9, 6), 7.0, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    f = ctypes.c_float

    def render(spheres=P(sph), n_sph=len(sph), lights=P(lg), n_lg=len(lg), c=P(cam), W=4, H=4,
               zoom=-4.0, aa=3.0, S=6, sem=0, dst=P(out), walk=0, threads=1):
        rc = L.rtg_render_camera_host(spheres, n_sph, lights, n_lg, c, W, H, f(zoom), f(aa), S,
                                      sem, dst, walk, threads)
        return rc, L.rtg_last_error().decode()

    def gen(c=P(cam), W=4, H=4, zoom=-4.0, aa=3.0, dst=P(rays), threads=1):
        rc = L.rtg_camera_rays_host(c, W, H, f(zoom), f(aa), dst, threads)
        return rc, L.rtg_last_error().decode()

    for kw, msg in ((dict(c=None), "null camera"),
                    (dict(dst=None), "null destination"),
                    (dict(spheres=None), "null scene array"),
                    (dict(lights=None), "null scene array"),
                    (dict(W=0), "empty frame"),
                    (dict(H=0), "empty frame"),
                    (dict(aa=257.0), "aliasFactor"),
                    (dict(aa=float("nan")), "aliasFactor"),
                    (dict(S=0), "stackSize 0 outside"),
                    (dict(S=17), "stackSize 17 outside"),
                    (dict(sem=2), "semantics 2"),
                    (dict(sem=-1), "semantics -1"),
                    (dict(walk=2), "walk 2"),
                    (dict(walk=-1), "walk -1")):
        rc, err = render(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)  # RTG_ERR_INVALID
    for kw, msg in ((dict(c=None), "null camera"),
                    (dict(dst=None), "null destination"),
                    (dict(W=0), "empty frame"),
                    (dict(H=0), "empty frame"),
                    (dict(aa=256.5), "aliasFactor"),
                    (dict(aa=float("nan")), "aliasFactor")):
        rc, err = gen(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert (out == 7.0).all() and (rays == 7.0).all()
    n = ctypes.c_uint(99)
    for args in ((f(3.0), None), (f(257.0), ctypes.byref(n)), (f(float("nan")), ctypes.byref(n))):
        assert L.rtg_camera_sample_count(*args) == -1 and L.rtg_last_error() != b""
    assert n.value == 99
    assert [rtg.camera_sample_count(a) for a in (-1.0, 0.0, 0.5, 1.0, 2.5, 3.0, 256.0)] == \
        [0, 0, 1, 1, 3, 3, 256]
    v = np.zeros(3, F)
    for args in ((None, P(v), P(v), P(cam)), (P(v), None, P(v), P(cam)),
                 (P(v), P(v), None, P(cam)), (P(v), P(v), P(v), None)):
        assert L.rtg_camera_look_at(*args) == -1 and L.rtg_last_error() != b""
    L.rtg_camera_identity(None)  # nothing to write: returns
    rc, err = render(n_sph=0, spheres=None, n_lg=0, lights=None)  # an empty scene is a scene
    assert rc == 0 and err == "" and (out == 0).all()
    with pytest.raises(rtg.RtgError, match="walk 5"):
        rtg.render_camera_host(sph, lg, cam, 4, 4, walk=5)
    # a record and 12 floats are the same pose
    a = rtg.render_camera_host(sph, lg, cam, 8, 6)
    b = rtg.render_camera_host(sph, lg, rtg.camera_identity(), 8, 6)
    assert a.shape == (6, 8, 3) and a.dtype == F and a.tobytes() == b.tobytes()


# ---- 7. no samples ----

@pytest.mark.parametrize("aa", [0.0, -2.0])
def test_no_samples(rtg, aa):
    sph, lg = scene_with_lights("reference")
    cam, zoom = pose("orbit", "reference")
    assert rtg.camera_rays_host(cam, 8, 6, zoom, aa).shape == (0, 6)
    for walk in (0, 1):
        fb = rtg.render_camera_host(sph, lg, cam, 8, 6, zoom, aa, walk=walk)
        assert fb.shape == (6, 8, 3) and not fb.view(np.uint32).any()  # +0 in every word
