"""Inputs and references shared by the direct-light and containment tests
(test_matte_host.py, test_gpu_matte.py): the scenes (aogen.SCENES), hit
records (aogen.hits plus one record with id = 2^30), the light sets, the
containment points, numpy float32 restatements of both definitions
(include/rtg.h, "direct light" and "containment") and the plain-loop answers,
computed once and left unchanged.

Light sets per scene: "own" (the scene's own lights), "m0" (none), "m1" (the
first of its own) and "m70" (70 seeded lights, so that indices pass the mask's
64; one at a sphere's centre, one colour with a negative and a zero component,
one at a record's own point).
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import aogen
import hostile
import raygen
from aogen import N_POINTS, SCENES, SIZES  # noqa: F401  (re-exported)
from conftest import GOLDEN, load_scene, random_scene
from test_raytrace_host import THREADS

F = np.float32
LIGHT_SETS = ("own", "m0", "m1", "m70")
AT_CENTRE, ODD_COLOUR, AT_POINT = 3, 5, 66  # special entries of the 70-light set
BIG_ID_AT = 5  # the record whose id is 2^30


def scene(name):
    return aogen.scene(name)


@functools.lru_cache(maxsize=None)
def hits(name):
    """aogen.hits(name) with record BIG_ID_AT a real point under id = 2^30: read-only."""
    h = aogen.hits(name).copy()
    real = np.flatnonzero(h["id"] >= 0)
    h[BIG_ID_AT] = h[real[real > BIG_ID_AT][3]]
    h[BIG_ID_AT]["id"] = 1 << 30
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def _own_lights(name):
    import rtg_amd as R
    if name in ("reference", "none"):
        return R.reference_scene()[1]
    if name == "c5":
        with open(os.path.join(GOLDEN, "golden.json")) as f:
            c = json.load(f)["configs"]["c5"]
        return load_scene("c5", c["spheres"], c["lights"])[1]
    if name == "base65":
        return hostile.base(65)[1]
    if name == "base150":
        return hostile.base(150)[1]
    if name == "cnan150":
        return hostile.mutated(150, "cnan")[1]
    return random_scene(np.random.default_rng(1000 + name), name, 2)[1]  # raygen.scene's seed


@functools.lru_cache(maxsize=None)
def _lights(name, kind):
    import rtg_amd as R
    own = _own_lights(name)
    if kind == "own":
        lg = own.copy()
    elif kind == "m0":
        lg = own[:0].copy()
    elif kind == "m1":
        lg = own[:1].copy()
    else:
        assert kind == "m70"
        geo = aogen.ray_scene(name)
        lo, hi = raygen.bounds(geo)
        span = (hi - lo).max()
        rng = np.random.default_rng(7000 + len(geo))
        lg = np.zeros(70, R.LIGHT_DTYPE)
        lg["pos"] = rng.uniform(lo - 0.5 * span, hi + 0.5 * span, size=(70, 3))
        lg["col"] = rng.uniform(0, 1, size=(70, 3))
        lg["pos"][AT_CENTRE] = geo["pos"][0]
        lg["col"][ODD_COLOUR] = (-0.5, 0.0, 0.75)
        h = hits(name)
        real = np.flatnonzero(h["id"] >= 0)
        lg["pos"][AT_POINT] = h["point"][real[real >= 8][0]]  # (not a hand-made record)
    lg.setflags(write=False)
    return lg


def lights(name, kind="own"):
    return _lights(name, kind).copy()


@functools.lru_cache(maxsize=None)
def want(name, kind="own"):
    """(sums, masks) of hits(name) by the plain loops (matte_host walk 0), read-only."""
    import rtg_amd as R
    out, lit = R.matte_host(scene(name), _lights(name, kind), hits(name), walk=0, threads=THREADS,
                            mask=True)
    out.setflags(write=False)
    lit.setflags(write=False)
    return out, lit


def canon(a):
    return aogen.canon(a)


def same_words(got, want_):
    """None, or where two float arrays differ as words with NaN canonicalised."""
    g, w = canon(got).reshape(-1), canon(want_).reshape(-1)
    if g.shape != w.shape:
        return f"shapes {np.shape(got)} vs {np.shape(want_)}"
    bad = np.flatnonzero(g != w)
    return None if not len(bad) else \
        f"{len(bad)} words differ, first at {bad[0]}: {g[bad[0]]:#x} vs {w[bad[0]]:#x}"


def same_masks(got, want_):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want_))
    return None if not len(bad) else \
        f"{len(bad)} masks differ, first at {bad[0]}: {int(got[bad[0]]):#x} vs {int(want_[bad[0]]):#x}"


# ---- the definition restated in numpy float32, one operation a line ----

def segments(h, lg):
    """The (n * m, 6) float32 shadow segments (P, L), point-major."""
    n, m = len(h), len(lg)
    out = np.zeros((n, m, 6), F)
    out[..., :3] = h["point"].astype(F)[:, None, :]
    out[..., 3:] = lg["pos"].astype(F)[None, :, :]
    return out.reshape(n * m, 6)


def restate(h, lg, vis):
    """(sums, masks, facing) of HIT_DTYPE records `h` under lights `lg`, with the
    line of sight `vis` ((n, m), nonzero: clear) taken from rtg_visible on
    segments(h, lg).  facing: (n, m) incidence > 0."""
    n, m = len(h), len(lg)
    P = h["point"].astype(F)
    N = h["normal"].astype(F)
    real = h["id"] >= 0
    total = np.zeros((n, 3), F)
    mask = np.zeros(n, np.uint64)
    facing = np.zeros((n, m), bool)
    one = F(1)
    with np.errstate(all="ignore"):
        for l in range(m):
            L = lg["pos"][l].astype(F)
            col = lg["col"][l].astype(F)
            dx = L[0] - P[:, 0]
            dy = L[1] - P[:, 1]
            dz = L[2] - P[:, 2]
            xx = dx * dx
            yy = dy * dy
            zz = dz * dz
            xy = xx + yy
            gap = xy + zz
            root = np.sqrt(gap)
            inv = one / root
            ux = inv * dx
            uy = inv * dy
            uz = inv * dz
            nx = N[:, 0] * ux
            ny = N[:, 1] * uy
            nz = N[:, 2] * uz
            nxy = nx + ny
            incidence = nxy + nz
            facing[:, l] = incidence > 0
            lit = (np.asarray(vis)[:, l] != 0) & facing[:, l] & real
            intensity = incidence / gap
            for q in range(3):
                term = intensity * col[q]
                added = total[:, q] + term
                total[:, q] = np.where(lit, added, total[:, q])
            if l < 64:
                mask |= np.where(lit, np.uint64(1) << np.uint64(l), np.uint64(0))
    assert total.dtype == F and root.dtype == F if m else True
    total[~real] = 0
    facing[~real] = False
    return total, mask, facing


# ---- the white scene: rayTrace reduces to calculateMatte of its first hit ----

def whitened(sph):
    """A copy with every sphere opaque, white and matte."""
    w = sph.copy()
    w["material"]["opacity"] = 1.0
    w["material"]["matteColour"] = 1.0
    w["material"]["glossColour"] = 0.0
    return w


# ---- containment ----

@functools.lru_cache(maxsize=None)
def _points(key, seed):
    geo = aogen.ray_scene(key) if not isinstance(key, tuple) else hostile.base(key[0])[0]
    rng = np.random.default_rng(seed + len(geo))
    c = geo["pos"].astype(np.float64)
    r = np.abs(geo["radius"].astype(np.float64))
    lo, hi = raygen.bounds(geo)
    parts = []
    i = rng.integers(0, len(geo), 20)
    parts.append(c[i])  # centres
    i = rng.integers(0, len(geo), 30)
    parts.append(c[i] + 0.5 * r[i][:, None] * raygen._unit(rng, 30))  # half radius
    for f in (1 - 1e-3, 1.0, 1 + 1e-6, 1 + 1e-3):  # around the surface
        i = rng.integers(0, len(geo), 20)
        parts.append(c[i] + f * r[i][:, None] * raygen._unit(rng, 20))
    pts = np.concatenate(parts)
    fill = rng.uniform(lo, hi, size=(N_POINTS - 2 - len(pts), 3))  # uniform in the bounds
    pts = np.concatenate([pts, fill, [[np.nan, 0.0, -10.0]], [[1e30, 0.0, 0.0]]]).astype(F)
    pts = pts[np.concatenate([rng.permutation(N_POINTS - 2), [N_POINTS - 2, N_POINTS - 1]])]
    assert pts.shape == (N_POINTS, 3)
    pts.setflags(write=False)
    return np.ascontiguousarray(pts)


POINT_SEED = 4100


def points(name):
    """N_POINTS containment points laid out over scene `name` (of aogen.SCENES), read-only."""
    return _points(name, POINT_SEED)


def hostile_points(n):
    """The same over hostile base scene n, for every mutation of it."""
    return _points((n,), POINT_SEED)


@functools.lru_cache(maxsize=None)
def want_contains(name):
    import rtg_amd as R
    out = R.contains_host(scene(name), points(name), walk=0, threads=THREADS)
    out.setflags(write=False)
    return out


def restate_contains(sph, pts):
    """(first index or -1, number of containing spheres) per point."""
    pts = np.asarray(pts, F)
    n = len(pts)
    first = np.full(n, -1, np.int32)
    count = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for s in range(len(sph) - 1, -1, -1):
            c = sph["pos"][s].astype(F)
            r = F(sph["radius"][s]) + F(1e-6)
            rr = r * r
            dx = pts[:, 0] - c[0]
            dy = pts[:, 1] - c[1]
            dz = pts[:, 2] - c[2]
            xx = dx * dx
            yy = dy * dy
            zz = dz * dz
            xy = xx + yy
            d2 = xy + zz
            inside = d2 <= rr
            first = np.where(inside, np.int32(s), first)
            count += inside
    return first, count
