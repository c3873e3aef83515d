"""Seeded ray and segment generators shared by the batch ray query tests
(test_rays_host.py, test_gpu_rays.py).  Every generator returns an (N, 6)
float32 array: origin and direction of a ray, or the end points a and b of a
segment.  Geometry is laid out in float64 and rounded to float32 once.

  primary   (a) the aa = 1 primary rays of a W x H frame (origin 0)
  inside    (b) origins uniform in the scene's bounds, random directions
  outside   (c) origins 1e2 .. 1e5 from the scene, aimed near a sphere's
                silhouette, half of them with a larger sphere behind it
  scaled    (d) direction lengths 1e-3, 7, 2^-40, 2^40, a zero direction,
                NaN / +-inf in one component of the origin or the direction
  surface   (e) origins on sphere surfaces and 0.01 along the direction
  interleave(f) two batches lane by lane
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from conftest import GOLDEN, load_scene, random_scene

F = np.float32


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(u, rng):
    """A unit vector perpendicular to each row of u."""
    v = _unit(rng, len(u))
    w = v - (v * u).sum(1, keepdims=True) * u
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def bounds(sph):
    if not len(sph):
        return np.full(3, -1.0), np.full(3, 1.0)
    c = sph["pos"].astype(np.float64)
    r = np.abs(sph["radius"].astype(np.float64))[:, None]
    return (c - r).min(0), (c + r).max(0)


def primary(W, H, zoom=-4.0):
    """(a): directions in numpy float32 exactly as test_gbuffer_host.restate
    forms them for aa = 1 (one sample, i = j = 0), pixel order."""
    aa, zoom = F(1), F(zoom)
    xs, ys, asp = F(16) / F(W), F(12) / F(H), F(16) / F(12)
    st = xs / aa
    halfW, halfH = F(W) * F(0.5), F(H) * F(0.5)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    zero = np.zeros(x.shape, F)
    pxX = (x.astype(F) - halfW) * xs
    pxY = (halfH - y.astype(F)) * ys
    v = [(pxX + zero * st) * asp, pxY + zero * st, np.full(x.shape, zoom, F)]
    l = F(1) / np.sqrt(_dot(v, v))
    out = np.zeros((H * W, 6), F)
    for q in range(3):
        out[:, 3 + q] = (l * v[q]).reshape(-1)
    return out


def inside(rng, sph, n):
    """(b)"""
    lo, hi = bounds(sph)
    out = np.empty((n, 6))
    out[:, :3] = rng.uniform(lo, hi, size=(n, 3))
    out[:, 3:] = _unit(rng, n) * rng.uniform(0.5, 2.0, size=(n, 1))
    return out.astype(F)


DISTANCES = (1e2, 1e3, 1e4, 1e5)
DISPLACEMENTS = (0.0, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3)


def outside(rng, sph, n, as_segments=False):
    """(c): ray k starts `dist` from sphere i's centre and is aimed at the point
    of i's silhouette (seen from the origin) displaced by eps r_i: inside the
    silhouette for eps < 0 (a grazing hit), outside for eps > 0.  Every second
    ray starts on the axis through a larger sphere j and i, so that j lies
    directly behind i and catches what grazes past.  The direction is the
    unnormalised aim - origin, so the hit is near t = 1 (a unit direction from
    that far could not hit: calcIntersection's minT starts at 1000)."""
    assert len(sph) >= 2
    c = sph["pos"].astype(np.float64)
    r = np.abs(sph["radius"].astype(np.float64))
    i = rng.integers(0, len(sph), n)
    u = _unit(rng, n)
    order = np.argsort(r)
    for k in range(0, n, 2):  # a larger sphere behind: origin on the axis j -> i
        rank = int(np.searchsorted(r[order], r[i[k]] * 1.1))
        if rank < len(sph):
            j = order[rng.integers(rank, len(sph))]
            ax = c[i[k]] - c[j]
            if np.linalg.norm(ax) > 0:
                u[k] = ax / np.linalg.norm(ax)
    dist = np.asarray(DISTANCES)[rng.integers(0, len(DISTANCES), n)]
    eps = np.asarray(DISPLACEMENTS)[rng.integers(0, len(DISPLACEMENTS), n)]
    w = _perp(u, rng)
    sin_a = r[i] / dist
    cos_a = np.sqrt(1.0 - sin_a * sin_a)
    o = c[i] + dist[:, None] * u
    aim = c[i] + (r[i] * (1.0 + eps))[:, None] * (sin_a[:, None] * u + cos_a[:, None] * w)
    out = np.empty((n, 6))
    out[:, :3] = o
    out[:, 3:] = (aim + (aim - o) * 0.5) if as_segments else (aim - o)
    return out.astype(F)


def scaled(rng, sph, n):
    """(d)"""
    out = inside(rng, sph, n).astype(np.float64)
    scale = np.asarray([1e-3, 7.0, 2.0 ** -40, 2.0 ** 40])[rng.integers(0, 4, n)]
    out[:, 3:] *= scale[:, None]
    out = out.astype(F)
    k = np.arange(n)
    out[k % 9 == 4, 3:] = 0  # a zero direction
    bad = np.flatnonzero(k % 9 == 7)
    vals = np.asarray([np.nan, np.inf, -np.inf], F)
    out[bad, rng.integers(0, 6, len(bad))] = vals[rng.integers(0, 3, len(bad))]
    return out


def surface(rng, sph, n):
    """(e): the renderer's own kind of origin: a point P on a sphere, and P +
    0.01 d for the direction d it leaves with."""
    assert len(sph)
    c = sph["pos"].astype(np.float64)
    r = np.abs(sph["radius"].astype(np.float64))
    i = rng.integers(0, len(sph), n)
    nrm = _unit(rng, n)
    d = _unit(rng, n)
    P = c[i] + r[i][:, None] * nrm
    out = np.empty((n, 6))
    out[:, :3] = np.where((np.arange(n) % 2 == 0)[:, None], P, P + 0.01 * d)
    out[:, 3:] = d
    return out.astype(F)


def interleave(a, b):
    """(f): a[0], b[0], a[1], b[1], ...: one wave holds both kinds."""
    n = min(len(a), len(b))
    out = np.empty((2 * n, 6), F)
    out[0::2] = a[:n]
    out[1::2] = b[:n]
    return out


def segments(rng, sph, n):
    """Light-to-surface pairs, a == b, b just before and just behind a
    blocker's surface (+-1e-4 along the segment), and the (c) origins as a."""
    assert len(sph) >= 2
    c = sph["pos"].astype(np.float64)
    r = np.abs(sph["radius"].astype(np.float64))
    lo, hi = bounds(sph)
    span = (hi - lo).max()
    q = n // 4
    light = rng.uniform(lo - span, hi + span, size=(n, 3))
    i = rng.integers(0, len(sph), n)
    X = c[i] + r[i][:, None] * _unit(rng, n)  # surface points
    out = np.empty((n, 6))
    out[:, :3] = light
    out[:, 3:] = X
    # b before / behind the surface of blocker i, on the side facing the light
    k = np.arange(q, 2 * q)
    toward = light[k] - c[i[k]]
    toward /= np.linalg.norm(toward, axis=1, keepdims=True)
    Xf = c[i[k]] + r[i[k]][:, None] * toward
    along = Xf - light[k]
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    out[k, 3:] = Xf + np.where(k % 2 == 0, 1e-4, -1e-4)[:, None] * along
    out = out.astype(F)
    out[2 * q:3 * q] = outside(rng, sph, q, as_segments=True)
    same = np.arange(3 * q, n, 5)
    out[same, 3:] = out[same, :3]  # a == b
    return out


def diff_hits(a, b):
    """The first differing record of two HIT_DTYPE arrays, or None."""
    wa = a.view(np.uint32).reshape(len(a), 8)
    wb = b.view(np.uint32).reshape(len(b), 8)
    bad = np.flatnonzero((wa != wb).any(1))
    if not len(bad):
        return None
    return f"{len(bad)} of {len(a)} records differ; first at {bad[0]}: {a[bad[0]]} vs {b[bad[0]]}"


@functools.lru_cache(maxsize=None)
def scene(name):
    """Spheres of the reference scene, golden scene c5 (1024 spheres) or a seeded
    random scene of `name` spheres."""
    import rtg_amd as R
    if name == "reference":
        return R.reference_scene()[0]
    if name == "c5":
        with open(os.path.join(GOLDEN, "golden.json")) as f:
            c = json.load(f)["configs"]["c5"]
        return load_scene("c5", c["spheres"], c["lights"])[0]
    return random_scene(np.random.default_rng(1000 + name), name, 2)[0]
