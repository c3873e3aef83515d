"""The scene fact behind the masked render kernel's guard-free build
(scene_ranged, rtg_scene_pack.h, through rtg_scene_ranged): every refractive
index finite with 2^-96 <= |n| <= 2^96.  Host only.

The kernel's proof (polarised_reflection, rtg_trace.h) needs |n| <= 2^100 and
no NaN; the fact keeps a margin of 2^4, so the scenes that must fail it here
are the ones the proof cannot take plus the margin's own."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import load_scene, random_scene

HOSTILE = [2.0 ** 120, 0.0, -0.0, float("inf"), float("-inf"), float("nan"), 2.0 ** -120,
           -(2.0 ** 120), float(np.nextafter(np.float32(2.0 ** 96), np.float32(np.inf))),
           float(np.nextafter(np.float32(2.0 ** -96), np.float32(0))), 1e-45]
BENIGN = [1.0, 1.33, -1.5, 2.4, 1e-3, 2.0 ** 96, -(2.0 ** 96), 2.0 ** -96]


def _passing(rtg, golden):
    out = {"reference": rtg.reference_scene()[0]}
    for name in ("c2", "c3", "c4"):
        c = golden["configs"][name]
        out[name] = load_scene(name, c["spheres"], c["lights"])[0]
    return out


def test_benchmark_scenes_pass(rtg, golden):
    for name, sph in _passing(rtg, golden).items():
        assert rtg.scene_ranged(sph), name
    # the generated scenes bench.py renders are the golden ones' generator's
    for n in (4, 16, 64):
        assert rtg.scene_ranged(rtg.generate_scene(n, 3, seed=7)[0]), n
    assert rtg.scene_ranged(np.zeros(0, rtg.SPHERE_DTYPE))  # the background alone


@pytest.mark.parametrize("bad", HOSTILE, ids=[repr(v) for v in HOSTILE])
def test_hostile_index_fails_and_fact_is_monotone(rtg, golden, bad):
    for name, sph in _passing(rtg, golden).items():
        # appended to a passing scene, at its head and alone
        last = np.concatenate([sph, sph[:1]])
        last[-1]["material"]["refractiveIndex"] = bad
        assert not rtg.scene_ranged(last), (name, bad)
        first = last[::-1].copy()
        assert not rtg.scene_ranged(first), (name, bad)
        assert not rtg.scene_ranged(last[-1:]), (name, bad)
        # monotone: no sphere appended to a failing scene makes it pass
        again = np.concatenate([last, sph])
        assert not rtg.scene_ranged(again), (name, bad)


def test_bounds_are_inclusive(rtg):
    rng = np.random.default_rng(5)
    sph, _ = random_scene(rng, 8, 1)
    for v in BENIGN:
        s = sph.copy()
        s[3]["material"]["refractiveIndex"] = v
        assert rtg.scene_ranged(s), v


def test_only_the_index_counts(rtg):
    """Geometry and the other material fields are not part of the fact: a
    non-finite centre (a scene without masks, which never runs the masked
    kernel) leaves it true."""
    rng = np.random.default_rng(6)
    sph, _ = random_scene(rng, 5, 1)
    sph[1]["pos"] = [np.nan, 0, -10]
    sph[2]["material"]["opacity"] = np.inf
    assert rtg.scene_ranged(sph)
