"""CPU tests of the batch ray queries' host forms (rtg_intersect_host,
rtg_visible_host, rtg.h).

The yardstick is `restate_hits` / `restate_visible` below: raySphere,
calcIntersection and hasClearLineOfSight (raytracer.h:81-194, 272-309) written
again in numpy float32, elementwise and in the reference's operation order.
numpy's float32 sqrt and / are correctly rounded and nothing contracts, so
every field is compared as bits.  walk = 1 (the device kernel's query path
compiled for the host: the BVH with the outside-origin treatment, the
64-sphere query, the flat loop) must equal walk = 0 (plain loops) byte for
byte; the near-tangent rays from far outside the scene (raygen.outside) are the
ones that catch a BVH box that is too small.  No GPU calls.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import raygen
from raygen import diff_hits as _diff, scene

F = np.float32


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _calc(sph, o, d):
    """calcIntersection for rays (o, d), lists of three float32 arrays: the
    winner's index (-1: none) and minT."""
    a = _dot(d, d)
    a4, den = F(4) * a, F(2) * a
    minT = np.full(o[0].shape, F(1000))
    best = np.full(o[0].shape, -1, np.int32)
    for k in range(len(sph)):
        c = [F(sph["pos"][k][q]) for q in range(3)]
        r2 = F(sph["radius"][k]) * F(sph["radius"][k])
        disp = [o[q] - c[q] for q in range(3)]
        b = F(2) * _dot(d, disp)
        cc = _dot(disp, disp) - r2
        rad = b * b - a4 * cc
        root = np.sqrt(rad)
        u0, u1 = (-b + root) / den, (-b - root) / den
        sm = np.full(o[0].shape, F(10000))
        ok = rad >= F(0)  # false for NaN, whose roots then never count
        t0 = ok & (u0 > F(1.0e-5)) & (u0 < sm)
        sm = np.where(t0, u0, sm)
        t1 = ok & (u1 > F(1.0e-5)) & (u1 < sm)
        sm = np.where(t1, u1, sm)
        take = (t0 | t1) & (sm < minT)
        minT = np.where(take, sm, minT)
        best = np.where(take, np.int32(k), best)
    return best, minT


def _canon(x):
    x = np.ascontiguousarray(x, F)
    x.view(np.uint32)[np.isnan(x)] = 0xFFC00000
    return x


def restate_hits(rtg, sph, rays):
    rays = np.asarray(rays, F).reshape(-1, 6)
    out = np.zeros(len(rays), rtg.HIT_DTYPE)
    o = [rays[:, q].copy() for q in range(3)]
    d = [rays[:, 3 + q].copy() for q in range(3)]
    with np.errstate(all="ignore"):
        best, minT = _calc(sph, o, d)
        out["id"], out["t"] = best, minT
        hit = best >= 0
        if len(sph):
            idc = np.maximum(best, 0)
            P = [o[q] + minT * d[q] for q in range(3)]
            e = [P[q] - sph["pos"][idc, q] for q in range(3)]
            ln = F(1) / np.sqrt(_dot(e, e))
            N = [ln * e[q] for q in range(3)]
            for q in range(3):
                out["point"][:, q] = np.where(hit, P[q], F(0))
                out["normal"][:, q] = np.where(hit, N[q], F(0))
    out["point"] = _canon(out["point"])
    out["normal"] = _canon(out["normal"])
    return out


def _segment_rays(segs):
    """(a, vnorm(b - a)) and the gap |b - a|^2 of hasClearLineOfSight."""
    segs = np.asarray(segs, F).reshape(-1, 6)
    with np.errstate(all="ignore"):
        dist = [segs[:, 3 + q] - segs[:, q] for q in range(3)]
        gap = _dot(dist, dist)
        l = F(1) / np.sqrt(gap)
        rays = segs.copy()
        for q in range(3):
            rays[:, 3 + q] = l * dist[q]
    return rays, gap


def _compose(rays, gap, ids, t):
    """visible == !(id >= 0 && |t dir|^2 < gap)"""
    with np.errstate(all="ignore"):
        td = [t * rays[:, 3 + q] for q in range(3)]
        return (~((ids >= 0) & (_dot(td, td) < gap))).astype(np.uint8)


def restate_visible(sph, segs):
    rays, gap = _segment_rays(segs)
    with np.errstate(all="ignore"):
        best, minT = _calc(sph, [rays[:, q].copy() for q in range(3)],
                           [rays[:, 3 + q].copy() for q in range(3)])
    return _compose(rays, gap, best, minT)


# ---- 1. walk 0 against the restatement ----

@pytest.mark.parametrize("name", [0, 1, 12, 80, "reference"])
def test_plain_loops_match_restatement(rtg, name):
    sph = scene(name)
    rng = np.random.default_rng(7)
    batches = [raygen.primary(37, 29), raygen.inside(rng, sph, 1500),
               raygen.scaled(rng, sph, 1500)]
    if len(sph):
        batches.append(raygen.surface(rng, sph, 1500))
    rays = np.concatenate(batches)
    got = rtg.intersect_host(sph, rays, walk=0, threads=4)
    want = restate_hits(rtg, sph, rays)
    assert got.tobytes() == want.tobytes(), _diff(got, want)
    if len(sph) >= 12:
        assert (got["id"] >= 0).mean() > 0.1
    else:
        miss = got["id"] < 0
        assert (got["t"][miss] == 1000).all() and (got["point"][miss] == 0).all()
    # the same rays as segments (o -> o + d): hasClearLineOfSight
    segs = rays.copy()
    with np.errstate(all="ignore"):
        segs[:, 3:] = rays[:, :3] + rays[:, 3:]
    vis = rtg.visible_host(sph, segs, walk=0, threads=4)
    assert vis.tobytes() == restate_visible(sph, segs).tobytes()
    if len(sph) == 0:
        assert (vis == 1).all()


# ---- 2. tie to the G-buffer ----

@pytest.mark.parametrize("n", [12, 80, 200])
@pytest.mark.parametrize("W,H", [(37, 29), (64, 48)])
def test_primary_rays_match_gbuffer(rtg, n, W, H):
    sph = scene(n)
    hits = rtg.intersect_host(sph, raygen.primary(W, H), walk=0, threads=4)
    g = rtg.gbuffer_host(sph, W, H, -4.0, 1.0, threads=4).reshape(-1)
    assert (hits["id"] == g["id"]).all()
    assert hits["t"].tobytes() == g["t"].tobytes()
    assert hits["normal"].tobytes() == g["normal"].tobytes()
    assert (g["hits"] == (hits["id"] >= 0)).all()
    assert (hits["id"] >= 0).any()


# ---- 3. visible_host against the composition ----

@pytest.mark.parametrize("name", [12, 80, "reference"])
def test_visible_is_the_composition(rtg, name):
    sph = scene(name)
    segs = raygen.segments(np.random.default_rng(11), sph, 4000)
    rays, gap = _segment_rays(segs)
    hits = rtg.intersect_host(sph, rays, walk=0, threads=4)
    vis = rtg.visible_host(sph, segs, walk=0, threads=4)
    assert vis.tobytes() == _compose(rays, gap, hits["id"], hits["t"]).tobytes()
    assert 0.02 < vis.mean() < 0.98  # both answers occur
    assert vis.tobytes() == restate_visible(sph, segs).tobytes()


# ---- 4. walk 1 == walk 0 ----

def _walk_batches(sph, per):
    rng = np.random.default_rng(23)
    ins, outs = raygen.inside(rng, sph, per), raygen.outside(rng, sph, per)
    return {"inside": ins, "outside": outs, "scaled": raygen.scaled(rng, sph, per // 4),
            "surface": raygen.surface(rng, sph, per),
            "interleaved": raygen.interleave(raygen.inside(rng, sph, per // 2),
                                             raygen.outside(rng, sph, per // 2))}


@pytest.mark.parametrize("name", [64, 65, 200, "c5"])
def test_kernel_walk_equals_plain_loops(rtg, name):
    """64: the two-pass query; 65, 200, c5: the BVH, with origins far outside
    its origin box (at least 20 000 rays per BVH scene)."""
    sph = scene(name)
    b = _walk_batches(sph, 8000 if name == 64 else 7000)
    rays = np.concatenate(list(b.values()))
    assert name == 64 or len(rays) >= 20000
    plain = rtg.intersect_host(sph, rays, walk=0, threads=8)
    walk = rtg.intersect_host(sph, rays, walk=1, threads=8)
    assert walk.tobytes() == plain.tobytes(), _diff(walk, plain)
    # not an all-miss batch: a quarter of the far near-tangent rays hit
    far = rtg.intersect_host(sph, b["outside"], walk=0, threads=8)
    assert (far["id"] >= 0).mean() >= 0.25
    segs = np.concatenate([raygen.segments(np.random.default_rng(29), sph, 8000),
                           raygen.outside(np.random.default_rng(31), sph, 2000, as_segments=True)])
    vp = rtg.visible_host(sph, segs, walk=0, threads=8)
    vw = rtg.visible_host(sph, segs, walk=1, threads=8)
    assert vw.tobytes() == vp.tobytes(), np.flatnonzero(vw != vp)[:8]
    assert 0.02 < vp.mean() < 0.98


# ---- 5. argument errors, n == 0, threads ----

def test_errors_empty_batches_and_threads(rtg):
    assert rtg.RAY_DTYPE.itemsize == 24 and rtg.SEGMENT_DTYPE.itemsize == 24
    assert rtg.HIT_DTYPE.itemsize == 32
    L = rtg.lib()
    vp = ctypes.c_void_p
    sph = scene(80)
    rays = raygen.inside(np.random.default_rng(3), sph, 1001)
    hits = np.zeros(len(rays), rtg.HIT_DTYPE)
    vis = np.zeros(len(rays), np.uint8)
    S, Rp, Hp, Vp = vp(sph.ctypes.data), vp(rays.ctypes.data), vp(hits.ctypes.data), vp(vis.ctypes.data)
    for fn, outp in ((L.rtg_intersect_host, Hp), (L.rtg_visible_host, Vp)):
        for args in ((S, len(sph), None, 8, outp, 0, 1),      # null input
                     (S, len(sph), Rp, 8, None, 0, 1),        # null output
                     (None, len(sph), Rp, 8, outp, 0, 1),     # null scene array
                     (S, len(sph), Rp, 8, outp, 2, 1),        # walk
                     (S, len(sph), Rp, 8, outp, -1, 1)):
            assert fn(*args) == -1
            assert L.rtg_last_error() != b""
        for walk in (0, 1):  # n == 0: RTG_OK, nothing written
            assert fn(S, len(sph), Rp, 0, outp, walk, 1) == 0
    assert not hits.view(np.uint8).any() and not vis.any()
    # the device entry points validate before any GPU call
    assert L.rtg_intersect_device(None, Rp, 8, Hp, None) == -1
    assert L.rtg_visible_device(None, Rp, 8, Vp, None) == -1
    assert L.rtg_intersect(0, S, len(sph), None, 8, Hp) == -1
    assert L.rtg_visible(0, S, len(sph), Rp, 8, None) == -1
    assert b"null" in L.rtg_last_error()
    with pytest.raises(rtg.RtgError, match="walk"):
        rtg.intersect_host(sph, rays, walk=3)
    assert len(rtg.intersect_host(sph, rays[:0])) == 0
    assert len(rtg.visible_host(sph, rays[:0], walk=1)) == 0
    # record arrays and (N, 6) floats are the same batch
    assert (rtg.intersect_host(sph, rays.view(rtg.RAY_DTYPE).reshape(-1)).tobytes()
            == rtg.intersect_host(sph, rays).tobytes())
    for walk in (0, 1):
        a = rtg.intersect_host(sph, rays, walk=walk, threads=1)
        assert rtg.intersect_host(sph, rays, walk=walk, threads=4).tobytes() == a.tobytes()
        assert rtg.intersect_host(sph, rays, walk=walk, threads=0).tobytes() == a.tobytes()
        v = rtg.visible_host(sph, rays, walk=walk, threads=1)
        assert rtg.visible_host(sph, rays, walk=walk, threads=4).tobytes() == v.tobytes()
