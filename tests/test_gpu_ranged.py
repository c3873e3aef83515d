"""The masked render kernel without the rare-path guards that value-range
proofs rule out (rtg_trace.h IsRangedScene), on the GPU:

  1. the proofs' float facts, exhaustively or over 2^28 seeded draws
     (tests/fpcheck/fpcheck_ranged_gpu.hip; below the frames in this file):
     the call sites' square root on refraction's two operand domains and on
     all negatives against sqrtf, unit_dir_query's case analysis, and the
     Fresnel quotient without its `fast` test;
  2. 64 x 48 frames (nAA 3, S in 2..6, seeded scenes of 4-16 spheres) against
     the oracle, bit for bit with NaNs at the same positions, no pixel left
     out: one set of scenes that pass scene_ranged (the guard-free kernel) and
     the same scenes with one hostile refractive index each, which fail it
     (the guarded kernel).  Each set holds scenes built for total internal
     reflection (sinA2 > 1), for |rad| < 0.001 in the refraction quadratic
     and for grazing hits; the builder's own arithmetic checks that those
     cases occur among the primary samples.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from conftest import bits_equal, first_mismatch, random_scene

pytestmark = pytest.mark.gpu

W, H, AA = 64, 48, 3.0
HOSTILE = [2.0 ** 120, 0.0, float("inf"), float("nan")]


# ------------------------------------------------------------------ frames
def _sphere(R, pos, radius, opacity, index, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros(1, R.SPHERE_DTYPE)
    s[0]["pos"] = pos
    s[0]["radius"] = radius
    s[0]["material"] = R.make_material(opacity, 0.5, rng.uniform(0.2, 1, 3),
                                       rng.uniform(0.2, 1, 3), index)
    return s


def _lights(R, positions):
    lg = np.zeros(len(positions), R.LIGHT_DTYPE)
    for l, p in enumerate(positions):
        lg[l]["pos"] = p
        lg[l]["col"] = [1.0, 0.9 - 0.2 * l, 0.6 + 0.1 * l]
    return lg


def _sample_dirs():
    """Primary sample directions of a W x H frame (main.cpp:411-426), f64."""
    n = int(AA)
    xs, ys, st = 16.0 / W, 12.0 / H, (16.0 / W) / AA
    x, y, i, j = np.meshgrid(np.arange(W), np.arange(H), np.arange(n), np.arange(n),
                             indexing="ij")
    rx = ((x - W / 2) * xs + j * st) * (16.0 / 12.0)
    ry = (H / 2 - y) * ys + i * st
    d = np.stack([rx, ry, np.full(rx.shape, -4.0)], -1).reshape(-1, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _first_hit(d, c, r, far):
    """t, cos(D, N) of each direction's hit of sphere (c, r) from the origin
    (far: the second root, the camera inside the sphere), NaN where it misses."""
    b = d @ c
    disc = b * b - (c @ c - r * r)
    t = np.where(disc >= 0, b + (1 if far else -1) * np.sqrt(np.abs(disc)), np.nan)
    t = np.where(t > 1e-5, t, np.nan)
    N = (t[:, None] * d - c) / r
    return t, np.einsum("ij,ij->i", d, N)


def _tir_scene(R):
    """A sphere less dense than the background in front of the camera: a
    primary hit has ratio = 1 / 0.5, so sinA2 = 2 sinA1 > 1 past 30 degrees."""
    c, r = np.array([0.5, 0.3, -7.0]), 5.5
    _, cos = _first_hit(_sample_dirs(), c, r, far=False)
    sin_a2 = 2.0 * np.sqrt(1 - np.minimum(cos * cos, 1.0))
    assert (sin_a2 > 1.001).sum() > 1000 and (sin_a2 < 0.999).sum() > 500
    sph = np.concatenate([_sphere(R, c, r, 0.3, 0.5, 1),
                          _sphere(R, [-5.0, -2.0, -14.0], 3.0, 0.6, 1.5, 2),
                          _sphere(R, [4.0, 3.0, -6.0], 1.0, 0.0, 2.4, 3),
                          _sphere(R, [0.0, -104.0, -20.0], 100.0, 1.0, 1.0, 4)])
    return sph, _lights(R, [[10.0, 30.0, 10.0], [-20.0, 5.0, 0.0]])


def _small_rad_scene(R):
    """The camera inside sphere 0, a little behind its centre on the view
    axis, itself inside the far thinner sphere 1: a primary ray meets sphere 0
    from inside almost along its normal (sin^2 A1 <= 3.7e-4, growing from the
    frame's centre) and leaves into sphere 1 with ratio = 1 / 0.0173, so
    rad = 4 (cos^2 A1 - qc) = 4 (0.0173^2 - sin^2 A1): above 0.001 in the
    middle of the frame, in (0, 0.001) around it (the single-root branch, no
    total internal reflection), negative with |rad| < 0.001 towards the
    corners (total internal reflection)."""
    c, r, n1 = np.array([0.0, 0.0, 0.1]), 5.0, 0.0173
    _, cos = _first_hit(_sample_dirs(), c, r, far=True)
    rad = 4.0 * (n1 * n1 - (1 - np.minimum(cos * cos, 1.0)))
    assert (rad > 0.0011).sum() > 200
    assert ((rad > 0) & (rad < 0.0009)).sum() > 5000
    assert ((rad < 0) & (rad > -0.0009)).sum() > 5000
    sph = np.concatenate([_sphere(R, c, r, 0.3, 1.5, 5),
                          _sphere(R, [0.0, 0.0, 0.0], 50.0, 0.5, n1, 6),
                          _sphere(R, [2.0, 1.0, -3.0], 0.5, 0.4, 1.33, 7),
                          _sphere(R, [-1.5, -1.0, -3.5], 0.7, 1.0, 1.0, 8)])
    return sph, _lights(R, [[1.0, 2.0, 1.0], [-2.0, -1.0, -1.0], [0.0, 20.0, -20.0]])


def _grazing_scene(R):
    """Silhouettes through the frame's middle (the view axis is tangent to
    sphere 0 and the rays around it graze it), two spheres that touch, and a
    light in the tangent plane at sphere 2's top, whose shadow rays graze
    their own sphere."""
    c, r = np.array([5.0, 0.0, -8.0]), 5.0
    t, cos = _first_hit(_sample_dirs(), c, r, far=False)
    assert (np.abs(cos[~np.isnan(t)]) < 0.05).sum() > 20
    sph = np.concatenate([_sphere(R, c, r, 0.5, 1.5, 9),
                          _sphere(R, [-3.0, 0.0, -8.0], 3.0, 0.2, 1.33, 10),
                          _sphere(R, [0.0, -4.0, -8.0], 2.0, 0.8, 2.4, 11),
                          _sphere(R, [0.0, 3.5, -12.0], 1.5, 0.0, 1.1, 12)])
    return sph, _lights(R, [[0.0, -2.0, 0.0], [0.0, 5.0, -12.0], [40.0, 0.0, -10.0]])


@pytest.fixture(scope="module")
def scenes(rtg):
    """(name, spheres, lights, S) of the passing set; the builders' premises
    are checked as they run."""
    rng = np.random.default_rng(20261)
    out = [("tir", *_tir_scene(rtg), 6), ("small_rad", *_small_rad_scene(rtg), 5),
           ("grazing", *_grazing_scene(rtg), 4)]
    for k in range(5):
        n, m = int(rng.integers(4, 17)), int(rng.integers(1, 4))
        sph, lg = random_scene(rng, n, m)
        out.append((f"seeded{k}", sph, lg, 2 + k))  # S = 2 .. 6
    return out


@pytest.fixture(scope="module")
def wanted(scenes, oracle):
    """The oracle's frames of both sets, rendered once: [set][scene]."""
    want = {"pass": {}, "fail": {}}
    for k, (name, sph, lg, S) in enumerate(scenes):
        want["pass"][name] = (sph, oracle.render(sph, lg, W, H, S, aa=AA))
        bad = sph.copy()
        # the hostile index on the last sphere: the built scenes' special
        # cases, around their first spheres, stay as they are
        bad[-1]["material"]["refractiveIndex"] = HOSTILE[k % len(HOSTILE)]
        want["fail"][name] = (bad, oracle.render(bad, lg, W, H, S, aa=AA))
    return want


@pytest.mark.parametrize("which", ["pass", "fail"])
def test_frames_vs_oracle(rtg, scenes, wanted, which):
    assert rtg.device_count() >= 1
    for name, _, lg, S in scenes:
        sph, want = wanted[which][name]
        assert rtg.scene_ranged(sph) == (which == "pass"), name
        got = rtg.render(sph, lg, W, H, alias_factor=AA, stack_size=S)
        nan = int(np.isnan(want).sum())
        print(f"{which}/{name}: S {S}, {len(sph)} spheres, {nan} NaN values, "
              f"{int((want != 0).sum())} non-zero")
        assert bits_equal(got, want), (which, name, first_mismatch(got, want))
        assert (want != 0).any(), name


# ------------------------------------------------------------------ float facts
@pytest.fixture(scope="module")
def fplib():
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fpcheck",
                      "libfpcheck_ranged_gpu.so")
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def sqrt_domain(fplib):
    """One exhaustive pass, shared by the two tests below."""
    out = (ctypes.c_ulonglong * 7)()
    assert fplib.fpcheck_sqrt_domain_run(out) == 0
    unit, rad, neg, neg_sub, nan, bad, bad_neg_sub = list(out)
    print(f"sqrt_fast: unit {unit}, rad {rad}, negative normal {neg}, -0 and negative "
          f"subnormal {neg_sub}, NaN {nan}; {bad} mismatches, "
          f"{bad_neg_sub} among -0 and the negative subnormals")
    assert unit == 1 + (0x3F800000 - 0x33800000 + 1)  # 0 and [2^-24, 1]
    assert rad == 0x7F800000 - 0x3A83126F + 1  # [0.001f, +inf]
    assert neg == 0xFF800000 - 0x80800000 + 1  # -2^-126 .. -inf
    assert neg_sub == 0x00800000  # -0 and the negative subnormals
    assert nan == 2 * 0x7FFFFF
    return bad, bad_neg_sub


def test_sqrt_fast_on_refraction_domains(sqrt_domain):
    """Every operand refraction's two square roots can meet: 0, [2^-24, 1],
    [0.001, +inf], the negative normals, -inf and the NaNs.  (1 - y is 0 or at
    least 2^-24 in magnitude, and a radicand whose root is used is at least
    0.001 in magnitude: neither is ever -0 or a negative subnormal.)"""
    bad, _ = sqrt_domain
    assert bad == 0


def test_sqrt_fast_on_all_negatives(sqrt_domain):
    """The wider set: ALL negatives, -0 and the negative subnormals included.
    v_sqrt_f32 reads a subnormal operand as a zero, so sqrt_fast alone returns
    -0 for the 8388607 negative subnormals 0x80000001 .. 0x807FFFFF where sqrtf
    returns a NaN (measured on an MI355X; -0 agrees); the call sites' function
    (sqrt_fast_signed) turns every negative operand into a NaN, and is what
    the kernel checks here."""
    bad, bad_neg_sub = sqrt_domain
    assert bad + bad_neg_sub == 0, (bad, bad_neg_sub)


def test_unit_dir_query_cases(fplib):
    out = (ctypes.c_ulonglong * 6)()
    n = 1 << 28
    assert fplib.fpcheck_unit_dir_run(ctypes.c_ulonglong(n), out) == 0
    in_range, nan, zero, inf, outside, quot_bad = list(out)
    print(f"unit_dir: {in_range} in [0.92, 5.24], NaN {nan}, 0 {zero}, +inf {inf}, "
          f"elsewhere {outside}, quotients off {quot_bad}")
    assert in_range + nan + zero + inf + outside == n
    # every case of the analysis is met, in numbers
    assert min(in_range, nan, zero, inf) > 100_000
    assert outside == 0
    assert quot_bad == 0


def test_fresnel_quotient_without_fast_test(fplib):
    out = (ctypes.c_ulonglong * 4)()
    n = 1 << 28
    assert fplib.fpcheck_fresnel_ranged_run(ctypes.c_ulonglong(n), out) == 0
    used, nan, bad, not_fast = list(out)
    print(f"fresnel: {used} operand pairs, {nan} NaN, {bad} mismatches, {not_fast} not fast")
    assert used > n // 2 and nan > n // 64
    assert not_fast == 0
    assert bad == 0
