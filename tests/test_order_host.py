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
