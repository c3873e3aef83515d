"""CPU tests of the ray order's host form (rtg_ray_order_host, csrc/rtg_order.hip
with the key of csrc/rtg_order.h): a stable sort of a batch's indices by the
coherence key.  No GPU: the device sort is held to this form word for word in
test_gpu_order.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import raygen
from raygen import scene

SIZES = (0, 1, 2, 63, 64, 65, 4097)


def host_mix(sph, n, seed):
    """n rays of raygen.interleave(inside, outside): origins in the key box and
    1e2 .. 1e5 outside it, lane by lane."""
    rng = np.random.default_rng(seed)
    q = n // 2 + 1
    return raygen.interleave(raygen.inside(rng, sph, q), raygen.outside(rng, sph, q))[:n]


def check_order(order, keys, n):
    """order is a permutation of 0..n-1, keys[order] is non-decreasing, and
    among equal keys the indices increase (the sort is stable)."""
    assert order.dtype == np.uint32 and order.shape == (n,) and keys.shape == (n,)
    assert (np.sort(order) == np.arange(n)).all(), "not a permutation"
    ks = keys[order]
    assert (ks[1:] >= ks[:-1]).all(), "keys not sorted"
    same = ks[1:] == ks[:-1]
    assert (order[1:][same] > order[:-1][same]).all(), "equal keys out of index order"


# ---- 1. permutation and stability ----

@pytest.mark.parametrize("name", ["reference", 200, "c5"])
def test_permutation_and_stability(rtg, name):
    sph = scene(name)
    for n in SIZES:
        rays = host_mix(sph, n, 10 + n)
        order, keys = rtg.ray_order_host(sph, rays, keys=True)
        check_order(order, keys, n)
        assert (keys >> np.uint64(rtg.ORDER_KEY_BITS) == 0).all()
        if n >= 4097:
            assert len(np.unique(keys)) > n // 4  # the mix spreads over the key space


# ---- 2. one ray repeated ----

def test_repeated_ray_keeps_batch_order(rtg):
    sph = scene(200)
    rays = np.repeat(host_mix(sph, 4, 3)[2:3], 1000, axis=0)
    order, keys = rtg.ray_order_host(sph, rays, keys=True)
    assert (keys == keys[0]).all()
    assert (order == np.arange(1000)).all()


# ---- 3. degenerate rays, an empty scene ----

@pytest.mark.parametrize("name", [0, 200])
def test_degenerate_rays_and_empty_scene(rtg, name):
    """Zero directions, NaN / +-inf in a component, lengths 2^-40 .. 2^40; with
    no sphere the key box is [-1, 1]^3.  Keys are reproducible."""
    sph = scene(name)
    rays = raygen.scaled(np.random.default_rng(5), sph, 2000)
    assert np.isnan(rays).any() and np.isinf(rays).any() and (rays[:, 3:] == 0).all(1).any()
    order, keys = rtg.ray_order_host(sph, rays, keys=True)
    check_order(order, keys, len(rays))
    order2, keys2 = rtg.ray_order_host(sph, rays, keys=True)
    assert (keys == keys2).all() and (order == order2).all()
    zero = (rays[:, 3:] == 0).all(1) & np.isfinite(rays[:, :3]).all(1)
    dir_mask = np.uint64((1 << 2 * rtg.ORDER_DIR_BITS) - 1)
    assert (keys[zero] & dir_mask == 0).all()  # a zero direction: bin 0
    assert len(np.unique(keys)) >= 64


# ---- 4. the key box ----

def test_key_box(rtg):
    sph = scene(200)
    DIR = np.uint64(2 * rtg.ORDER_DIR_BITS)  # the origin's code lies above the direction's
    rays = raygen.primary(64, 48)
    perm = np.random.default_rng(7).permutation(len(rays))
    shuffled = rays[perm]
    order, keys = rtg.ray_order_host(sph, shuffled, keys=True)
    check_order(order, keys, len(rays))
    assert not (order == np.arange(len(rays))).all()
    distinct = len(np.unique(keys))
    assert distinct >= 64, distinct  # not a constant key
    # one origin: every origin bit is shared
    assert len(np.unique(keys >> DIR)) == 1
    # origins spread over the scene use the origin bits
    ins = raygen.inside(np.random.default_rng(8), sph, 3000)
    k_in = rtg.ray_order_host(sph, ins, keys=True)[1]
    assert len(np.unique(k_in >> DIR)) >= 1000
    # every origin 1e5 away: the cells clamp, the batch still sorts
    far = shuffled.copy()
    far[:, :3] += np.float32(1e5)
    order_f, keys_f = rtg.ray_order_host(sph, far, keys=True)
    check_order(order_f, keys_f, len(rays))
    assert len(np.unique(keys_f >> DIR)) == 1  # the last cell of each axis
    assert len(np.unique(keys_f)) >= 64


# ---- 5. segments ----

@pytest.mark.parametrize("name", [200, "c5"])
def test_segments_are_rays_to_b_minus_a(rtg, name):
    sph = scene(name)
    rng = np.random.default_rng(9)
    segs = np.concatenate([raygen.segments(rng, sph, 3000), raygen.scaled(rng, sph, 500)])
    as_rays = segs.copy()
    with np.errstate(invalid="ignore"):  # inf - inf
        as_rays[:, 3:] = segs[:, 3:] - segs[:, :3]  # float32
    o_s, k_s = rtg.ray_order_host(sph, segs, kind=rtg.ORDER_SEGMENTS, keys=True)
    o_r, k_r = rtg.ray_order_host(sph, as_rays, kind=rtg.ORDER_RAYS, keys=True)
    assert (k_s == k_r).all() and (o_s == o_r).all()
    assert not (rtg.ray_order_host(sph, segs, keys=True)[1] == k_s).all()  # the kind matters
    # SEGMENT_DTYPE records are taken as they are
    rec = np.ascontiguousarray(segs).view(rtg.SEGMENT_DTYPE).reshape(-1)
    assert (rtg.ray_order_host(sph, rec, kind=rtg.ORDER_SEGMENTS) == o_s).all()


# ---- 5b. the key, restated from the text of include/rtg.h ----

F = np.float32
LADDER = range(-149, 128)  # every power of two a float32 holds


def restate_key_box(sph):
    """(lo, hi, scale), three float32 each: lo = min(c - |r|), hi = max(c + |r|)
    over the spheres whose centre and radius are finite, [-1, 1]^3 when none is
    left; scale = 1024 / (hi - lo), or 0 when hi <= lo or the width or the
    quotient is not finite."""
    c, r = sph["pos"].astype(F).reshape(-1, 3), np.abs(sph["radius"].astype(F)).reshape(-1)
    keep = np.isfinite(c).all(1) & np.isfinite(r)
    c, r = c[keep], r[keep]
    if not len(c):
        lo, hi = np.full(3, -1, F), np.full(3, 1, F)
    else:
        with np.errstate(over="ignore"):
            lo, hi = (c - r[:, None]).min(0), (c + r[:, None]).max(0)
    with np.errstate(all="ignore"):
        w = hi - lo
        q = F(1024) / w
    ok = (hi > lo) & np.isfinite(w) & np.isfinite(q)
    assert lo.dtype == F and q.dtype == F
    return lo, hi, np.where(ok, q, F(0)).astype(F)


def _clamp_int(x):
    """(int)clamp(x, 0, 1023), the clamp in float with NaN going to 0."""
    x = np.where(np.isnan(x), F(0), x)
    x = np.minimum(np.maximum(x, F(0)), F(1023))
    return x.astype(np.int64).astype(np.uint64)


def _spread(v, stride, at):
    out = np.zeros(v.shape, np.uint64)
    for i in range(10):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(at + stride * i)
    return out


def restate_bins(d):
    """(u, v) octahedral bins of float32 directions (n, 3)."""
    dx, dy, dz = (d[:, q].astype(F) for q in range(3))
    one = F(1)
    with np.errstate(all="ignore"):
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        px, py = dx / s, dy / s
        sx = np.where(dx < 0, -one, one)  # sign(0) = +1, and -0 is a zero
        sy = np.where(dy < 0, -one, one)
        fx = (one - np.abs(py)) * sx
        fy = (one - np.abs(px)) * sy
        low = dz < 0
        px, py = np.where(low, fx, px), np.where(low, fy, py)
        u = _clamp_int((px + one) * F(512))
        v = _clamp_int((py + one) * F(512))
    none = (s == 0) | ~np.isfinite(s)
    assert s.dtype == F and px.dtype == F
    return np.where(none, np.uint64(0), u), np.where(none, np.uint64(0), v)


def restate_keys(sph, rays, kind=0):
    """uint64 keys of (n, 6) float32 rays, or of segments (a, b) as the rays
    (a, b - a) with the difference taken in float."""
    r = np.ascontiguousarray(rays, F).reshape(-1, 6)
    o, d = r[:, :3], r[:, 3:]
    if kind:
        with np.errstate(all="ignore"):
            d = (d - o).astype(F)
    lo, _, scale = restate_key_box(sph)
    key = np.zeros(len(r), np.uint64)
    with np.errstate(all="ignore"):
        for q in range(3):
            cell = _clamp_int((o[:, q] - lo[q]) * scale[q])
            key |= _spread(cell, 3, 20 + q)
    u, v = restate_bins(d)
    return key | _spread(u, 2, 0) | _spread(v, 2, 1)


def key_scenes():
    """name -> spheres: reference, 200, c5, no sphere; 200 with a NaN centre, an
    infinite centre component and an infinite and a NaN radius added (all four
    skipped); one point sphere (every axis degenerate); two point spheres apart
    in x only (y and z degenerate); two spheres whose box is wider than FLT_MAX."""
    out = {name: scene(name) for name in ("reference", 200, "c5", 0)}
    odd = np.concatenate([scene(200), scene(12)[:4]])
    odd[200]["pos"][1] = np.nan
    odd[201]["pos"][2] = -np.inf
    odd[202]["radius"] = np.inf
    odd[203]["radius"] = np.nan
    out["skipped"] = odd
    point = scene(12)[:1].copy()
    point["radius"] = 0
    out["point"] = point
    line = scene(12)[:2].copy()
    line["radius"] = 0
    line["pos"][1] = line["pos"][0]
    line["pos"][1][0] += F(3)
    out["line"] = line
    wide = scene(12)[:2].copy()
    wide["pos"][0] = (-3e38, 0, -1)
    wide["pos"][1] = (3e38, 1, -2)
    out["wide"] = wide
    return out


def ladder_batch(sph, seed=77):
    """64 rays of raygen.inside per k of LADDER with origins and directions
    x 2^k, then 3840 rays with edges planted: zero directions, -0 components,
    components of 3e38 (the sum overflows) and 1e-45, NaN and +-inf origin
    components, the six axis directions, and every 3rd of the whole batch with
    dz < 0 by construction of raygen.inside.  (21 568, 6) float32."""
    rng = np.random.default_rng(seed)
    geo = sph if len(sph) and np.isfinite(sph["pos"]).all() and np.isfinite(sph["radius"]).all() \
        else scene(200)
    base = raygen.inside(rng, geo, 64 * len(LADDER)).astype(np.float64)
    k = np.repeat(np.asarray(LADDER), 64)
    with np.errstate(over="ignore", under="ignore"):
        lad = (base * np.ldexp(1.0, k)[:, None]).astype(F)
    e = raygen.inside(rng, geo, 3840)
    i = np.arange(len(e))
    e[i % 16 == 0, 3:] = 0
    e[i % 16 == 1, 3 + (i[i % 16 == 1] // 16) % 3] = -0.0
    e[i % 16 == 2, 3 + (i[i % 16 == 2] // 16) % 3] = 3e38
    e[i % 16 == 3, 3:] = (3e38, -3e38, 3e38)
    e[i % 16 == 4, 3 + (i[i % 16 == 4] // 16) % 3] = 1e-45
    e[i % 16 == 5, 3:] = (1e-45, 0, -1e-45)
    vals = np.asarray([np.nan, np.inf, -np.inf], F)
    at = np.flatnonzero(i % 16 == 6)
    e[at, (at // 16) % 3] = vals[(at // 48) % 3]
    at = np.flatnonzero(i % 16 == 7)
    e[at, 3:] = 0
    e[at, 3 + (at // 16) % 3] = np.where((at // 48) % 2 == 0, 1, -1)
    at = np.flatnonzero(i % 16 == 8)  # -0 in x or y under dz < 0: the fold's sign(0)
    e[at, 3 + (at // 16) % 2] = -0.0
    e[at, 5] = -np.abs(e[at, 5])
    at = np.flatnonzero(i % 16 == 9)  # on the fold line: dz = -0 and +0
    e[at, 5] = np.where((at // 16) % 2 == 0, -0.0, 0.0)
    out = np.concatenate([lad, e]).astype(F)
    assert (out[:, 5] < 0).mean() > 0.3 and np.signbit(out[:, 3:5][out[:, 3:5] == 0]).any()
    return out


@pytest.mark.parametrize("name", list(key_scenes()))
def test_keys_equal_the_restatement(rtg, name):
    sph = key_scenes()[name]
    rays = ladder_batch(sph)
    lo, hi, scale = restate_key_box(sph)
    if name in ("point", "line", "wide"):
        assert (scale == 0).any()
    if name == 0:
        assert (lo == -1).all() and (hi == 1).all() and (scale == 512).all()
    if name == "skipped":
        assert all((a == b).all() for a, b in zip((lo, hi, scale), restate_key_box(scene(200))))
    for kind in (0, 1):
        order, keys = rtg.ray_order_host(sph, rays, kind=kind, threads=4, keys=True)
        want = restate_keys(sph, rays, kind)
        bad = np.flatnonzero(keys != want)
        assert not len(bad), (kind, len(bad), rays[bad[0]], hex(int(keys[bad[0]])), hex(int(want[bad[0]])))
        assert (order == np.argsort(want, kind="stable")).all()
    if name in ("reference", 200, "c5"):
        assert len(np.unique(want >> np.uint64(20))) > 500 and len(np.unique(want & np.uint64(0xFFFFF))) > 5000


def _unspread(key, stride, at):
    out = np.zeros(key.shape, np.int64)
    for i in range(10):
        out |= (((key >> np.uint64(at + stride * i)) & np.uint64(1)) << np.uint64(i)).astype(np.int64)
    return out


def test_bin_centre_lies_within_a_bin_of_the_direction(rtg):
    """In float64: the centre of a ray's bin, taken back through the inverse
    octahedral map, is within one bin of the ray's direction.  A bin is 2^-9
    wide in p, so the centre is at most 2^-10 from p in each coordinate; on the
    octahedron |x| + |y| + |z| = 1 the point then moves by at most (du, dv, |du|
    + |dv|), a length of sqrt(6) 2^-10, on either side of the fold (the fold
    swaps and reflects the coordinates and is continuous across its edges).
    The octahedron's points are at least 1 / sqrt(3) from the centre, so the
    angle is at most asin(sqrt(18) 2^-10); the float32 rounding of s, dx / s
    and (p + 1) 512 moves p by a few 2^-24, far less than the 1e-5 allowed here."""
    sph = scene(200)
    rays = ladder_batch(sph)
    keys = rtg.ray_order_host(sph, rays, keys=True)[1]
    d32 = rays[:, 3:]
    with np.errstate(all="ignore"):
        s32 = (np.abs(d32[:, 0]) + np.abs(d32[:, 1])) + np.abs(d32[:, 2])
    ok = np.isfinite(s32) & (s32 > 0)
    assert ok.mean() > 0.9
    d = d32[ok].astype(np.float64)
    d /= np.abs(d).max(1, keepdims=True)  # (keeps the squares in range)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    u, v = _unspread(keys[ok], 2, 0), _unspread(keys[ok], 2, 1)
    pu, pv = (u + 0.5) / 512 - 1, (v + 0.5) / 512 - 1
    z = 1 - np.abs(pu) - np.abs(pv)
    x = np.where(z < 0, (1 - np.abs(pv)) * np.where(pu < 0, -1.0, 1.0), pu)
    y = np.where(z < 0, (1 - np.abs(pu)) * np.where(pv < 0, -1.0, 1.0), pv)
    c = np.stack([x, y, z], 1)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    angle = np.arccos(np.clip((c * d).sum(1), -1, 1))
    bound = np.arcsin(np.sqrt(18.0) * 2.0 ** -10) + 1e-5
    assert angle.max() <= bound, (angle.max(), bound, rays[ok][np.argmax(angle)])
    assert angle.max() > bound / 8  # and the bound is not slack by an order of magnitude


# ---- 6. thread independence ----

def test_thread_independence(rtg):
    sph = scene("c5")
    rays = host_mix(sph, 4097, 11)
    o1, k1 = rtg.ray_order_host(sph, rays, threads=1, keys=True)
    o8, k8 = rtg.ray_order_host(sph, rays, threads=8, keys=True)
    assert (o1 == o8).all() and (k1 == k8).all()
    assert (rtg.ray_order_host(sph, rays, threads=8) == o1).all()  # without the keys buffer


# ---- 7. argument errors, the scratch size ----

def test_argument_errors_and_scratch(rtg):
    sph = scene(200)
    rays = host_mix(sph, 8, 1)
    order = np.zeros(8, np.uint32)
    L = rtg.lib()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for args, msg in (((P(sph), len(sph), None, 8, 0, P(order), None, 1), "null ray"),
                      ((P(sph), len(sph), P(rays), 8, 0, None, None, 1), "null order"),
                      ((None, 3, P(rays), 8, 0, P(order), None, 1), "null scene"),
                      ((P(sph), len(sph), P(rays), 8, 2, P(order), None, 1), "kind 2"),
                      ((P(sph), len(sph), P(rays), 8, -1, P(order), None, 1), "kind -1"),
                      ((P(sph), len(sph), P(rays), 1 << 32, 0, P(order), None, 1), "2\\^32")):
        with pytest.raises(rtg.RtgError, match=msg):
            rtg._check(L.rtg_ray_order_host(*args), "rtg_ray_order_host")
    assert (order == 0).all()
    # the scratch grows with n, holds two (key, index) buffer pairs and the
    # 256-bin table of every tile, and is refused past 2^32 - 1 rays
    T = rtg.ORDER_TILE_RAYS
    assert T % 64 == 0 and rtg.ORDER_SCAN_TILES == 256
    # the binding's copies of the sort's geometry are the header's
    import os
    import re
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "rtg.h")).read()
    for name in ("TILE_RAYS", "SCAN_TILES", "KEY_GRID"):
        value = re.search(rf"^#define RTG_ORDER_{name} (\d+)$", header, re.M)
        assert value and int(value.group(1)) == getattr(rtg, f"ORDER_{name}"), name
    prev = rtg.ray_order_scratch(0)
    for n in (1, T, T + 1, 100 * T, 300000):
        b = rtg.ray_order_scratch(n)
        tiles = -(-n // T)
        assert b % 16 == 0 and b >= prev
        assert b >= 24 * n + 256 * 4 * tiles
        prev = b
    assert rtg.ray_order_scratch((1 << 32) - 1) > 24 * ((1 << 32) - 1)
    with pytest.raises(rtg.RtgError, match="2\\^32"):
        rtg.ray_order_scratch(1 << 32)
