"""CPU tests of the primary-hit G-buffer's host form (rtg_gbuffer_host, rtg.h).

The yardstick is `restate` below: the record definition of rtg_gbuf_px written
again in numpy float32, elementwise and in the reference's operation order
(camera and primary ray as main.cpp:384-436, the raySphere root test and
calcIntersection as rtg_trace.h's closest_hit states them).  numpy's float32
sqrt and / are correctly rounded and nothing contracts, so every field is
compared as bits.  No GPU calls.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from conftest import random_scene

F = np.float32


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def restate(rtg, sph, W, H, zoom, aa, rows=None):
    """(H, W) GBUF_DTYPE records from the definition, all samples at once.
    rows: only those rows of the frame, (len(rows), W) records."""
    aa, zoom = F(aa), F(zoom)
    xs, ys, asp = F(16) / F(W), F(12) / F(H), F(16) / F(12)
    st = xs / aa
    halfW, halfH = F(W) * F(0.5), F(H) * F(0.5)
    nAA = 0
    while F(nAA) < aa:  # `for (int i = 0; i < aliasFactor; ++i)`
        nAA += 1
    ys_ = np.arange(H) if rows is None else np.asarray(rows, np.int64)
    out = np.zeros((len(ys_), W), rtg.GBUF_DTYPE)
    out["id"] = -1
    out["t"] = F(1000)
    if nAA == 0:
        return out
    S = nAA * nAA
    y, x, s = np.meshgrid(ys_, np.arange(W), np.arange(S), indexing="ij")
    i, j = (s // nAA).astype(F), (s % nAA).astype(F)
    pxX = (x.astype(F) - halfW) * xs
    pxY = (halfH - y.astype(F)) * ys
    v = [(pxX + j * st) * asp, pxY + i * st, np.full(x.shape, zoom, F)]
    with np.errstate(all="ignore"):
        l = F(1) / np.sqrt(_dot(v, v))
        d = [l * c for c in v]
        a = _dot(d, d)
        a4, den = F(4) * a, F(2) * a
        minT = np.full(x.shape, F(1000))
        best = np.full(x.shape, -1, np.int32)
        for k in range(len(sph)):
            c = [F(sph["pos"][k][q]) for q in range(3)]
            r2 = F(sph["radius"][k]) * F(sph["radius"][k])
            disp = [F(0) - c[q] for q in range(3)]
            b = F(2) * _dot(d, disp)
            cc = _dot(disp, disp) - r2
            rad = b * b - a4 * cc
            root = np.sqrt(rad)
            u0, u1 = (-b + root) / den, (-b - root) / den
            sm = np.full(x.shape, F(10000))
            ok = rad >= F(0)  # false for NaN, whose roots then never count
            t0 = ok & (u0 > F(1.0e-5)) & (u0 < sm)
            sm = np.where(t0, u0, sm)
            t1 = ok & (u1 > F(1.0e-5)) & (u1 < sm)
            sm = np.where(t1, u1, sm)
            take = (t0 | t1) & (sm < minT)
            minT = np.where(take, sm, minT)
            best = np.where(take, np.int32(k), best)
        hit = best >= 0
        out["hits"] = hit.sum(axis=2)
        out["idSum"] = (best + 1).astype(np.uint64).sum(axis=2).astype(np.uint32)
        win = np.argmin(np.where(hit, minT, F(np.inf)), axis=2)  # first of equal minima
        any_hit = out["hits"] > 0
        pick = lambda arr: np.take_along_axis(arr, win[..., None], axis=2)[..., 0]  # noqa: E731
        out["id"] = np.where(any_hit, pick(best), -1)
        out["t"] = np.where(any_hit, pick(minT), F(1000))
        out["sample"] = np.where(any_hit, win, 0)
        idc = np.maximum(out["id"], 0)
        N = np.zeros((len(ys_), W, 3), F)
        if len(sph):
            t = out["t"]
            e = [(F(0) + t * pick(d[q])) - sph["pos"][idc, q] for q in range(3)]
            ln = F(1) / np.sqrt(_dot(e, e))
            N = np.stack([ln * e[q] for q in range(3)], axis=-1).astype(F)
            N[~any_hit] = 0
        bits = N.view(np.uint32)
        bits[np.isnan(N)] = 0xFFC00000
        out["normal"] = N
    return out


def _same(a, b):
    """Every field equal, floats as bits."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _diff(a, b):
    bad = np.argwhere(a.view(np.uint32).reshape(a.shape + (8,))
                      != b.view(np.uint32).reshape(b.shape + (8,)))
    if not len(bad):
        return None
    y, x, _ = bad[0]
    return f"{len(bad)} words differ; first at ({y}, {x}): {a[y, x]} vs {b[y, x]}"


# (name, spheres, W, H, zoom, aa): the reference scene at 160x120, seeded random
# scenes of n in {0, 1, 12, 40, 80}, aa in {1, 2, 2.5, 3, 9}, both zoom signs,
# and 37x29 (W*H no multiple of the device kernel's pixels per group, groups
# straddling rows).
CASES = [("reference", None, 160, 120, -4.0, 3.0)]
for _n, _seed in ((0, 1), (1, 2), (12, 3), (40, 4), (80, 5)):
    for _aa, _zoom, _w, _h in ((3.0, -4.0, 37, 29), (2.0, 4.0, 37, 29), (1.0, -4.0, 64, 48),
                               (2.5, -4.0, 37, 29), (9.0, -4.0, 13, 11)):
        CASES.append((f"n{_n}-aa{_aa}-z{_zoom}-{_w}x{_h}", (_n, _seed), _w, _h, _zoom, _aa))
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(k):
    import rtg_amd as R
    _, scene, W, H, zoom, aa = CASES[k]
    if scene is None:
        sph, lg = R.reference_scene()
    else:
        sph, lg = random_scene(np.random.default_rng(scene[1]), scene[0], 2)
    return sph, lg, R.gbuffer_host(sph, W, H, zoom, aa, threads=4)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_host_matches_restatement(rtg, k):
    _, _, W, H, zoom, aa = CASES[k]
    sph, _, got = _case(k)
    want = restate(rtg, sph, W, H, zoom, aa)
    assert _same(got, want), _diff(got, want)
    if zoom > 0 and len(sph):  # random_scene's spheres are all at z < 0: behind this camera
        assert (got["hits"] == 0).all()


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_pixels_without_hits_are_black_in_the_reference(rtg, oracle, k):
    """A sample that misses returns I (x) background matte = +0, so a pixel no
    sample of which hits is +0 in every channel of the reference's frame.  (The
    converse does not hold: hit pixels can be +0 too.)"""
    _, _, W, H, zoom, aa = CASES[k]
    sph, lg, g = _case(k)
    fb = oracle.render(sph, lg, W, H, 6, aa=aa, zoom=zoom)
    miss = g["hits"] == 0
    assert (fb.view(np.uint32)[miss] == 0).all()


def _spheres(rtg, rows):
    sph = np.zeros(len(rows), rtg.SPHERE_DTYPE)
    for k, (x, y, z, r) in enumerate(rows):
        sph[k]["pos"] = [x, y, z]
        sph[k]["radius"] = r
    return sph


def test_ties_and_edges(rtg):
    W, H, aa = 40, 30, 3.0
    # two identical spheres: the lower index wins every tie
    sph = _spheres(rtg, [(0, 0, -10, 3), (0, 0, -10, 3)])
    g = rtg.gbuffer_host(sph, W, H, -4.0, aa)
    assert _same(g, restate(rtg, sph, W, H, -4.0, aa))
    hit = g["hits"] > 0
    assert hit.any() and (g["id"][hit] == 0).all()
    assert (g["idSum"][hit] == g["hits"][hit]).all()
    # the camera inside a sphere: every sample hits it from inside
    sph = _spheres(rtg, [(0.5, -0.25, 1, 5), (0, 0, -30, 2)])
    g = rtg.gbuffer_host(sph, W, H, -4.0, aa)
    assert _same(g, restate(rtg, sph, W, H, -4.0, aa))
    assert (g["hits"] == 9).all() and (g["id"] == 0).all() and (g["t"] > 3).all()
    # every sphere behind the camera: all misses, the record's miss values
    sph = _spheres(rtg, [(0, 0, 10, 3), (4, 1, 25, 6)])
    g = rtg.gbuffer_host(sph, W, H, -4.0, aa)
    assert _same(g, restate(rtg, sph, W, H, -4.0, aa))
    miss = np.zeros((H, W), rtg.GBUF_DTYPE)
    miss["id"], miss["t"] = -1, 1000.0
    assert _same(g, miss)
    # a root at t >= 1000 is no hit (minT starts at 1000); one just below is
    sph = _spheres(rtg, [(0, 0, -2000, 500), (0, 0, -1100, 120)])
    g = rtg.gbuffer_host(sph, W, H, -4.0, aa)
    assert _same(g, restate(rtg, sph, W, H, -4.0, aa))
    assert (g["id"] != 0).all() and (g["id"] == 1).any()
    assert g["t"][g["id"] == 1].min() > 970 and (g["t"] <= 1000).all()


def test_sizes_errors_and_threads(rtg):
    assert rtg.GBUF_DTYPE.itemsize == 32
    L = rtg.lib()
    sph, _ = rtg.reference_scene()
    out = np.zeros((8, 8), rtg.GBUF_DTYPE)
    f, vp = ctypes.c_float, ctypes.c_void_p
    for args in ((vp(sph.ctypes.data), 3, 8, 8, f(-4), f(3), None, 1),             # null destination
                 (vp(sph.ctypes.data), 3, 0, 8, f(-4), f(3), vp(out.ctypes.data), 1),  # W = 0
                 (vp(sph.ctypes.data), 3, 8, 8, f(-4), f(300), vp(out.ctypes.data), 1)):  # aa
        assert L.rtg_gbuffer_host(*args) == -1
        assert L.rtg_last_error() != b""
    # the device entry points validate before any GPU call
    assert L.rtg_gbuffer_device(None, 8, 8, f(-4), f(3), 16, 0, 1, None, None) == -1
    assert L.rtg_gbuffer(0, None, 0, 8, 8, f(-4), f(3), None) == -1
    assert b"null" in L.rtg_last_error()
    with pytest.raises(rtg.RtgError):
        rtg.gbuffer_host(sph, 8, 8, alias_factor=300.0)
    a = rtg.gbuffer_host(sph, 61, 47, threads=1)
    b = rtg.gbuffer_host(sph, 61, 47, threads=4)
    assert a.tobytes() == b.tobytes()
    assert rtg.gbuffer_host(sph, 61, 47, threads=0).tobytes() == a.tobytes()
