"""CPU tests of views folded into per-group coefficients (rtg_views_fold_host,
rtg_render_views_fold_host, rtg_cube_sh_weights; csrc/rtg_fold.hip and
csrc/rtg_camera.hip): a weighted sum of groups of frames in rtg.h's float
summation order.

  1. rtg_views_fold_host equals a numpy float32 restatement of the definition
     (terms laid out as (tiles, 64), the six-step tree, the sequential tile
     loop) byte for byte, on random frames whose exponents are spread so that
     the order matters: a plain sequential sum of the same terms differs in at
     least one word of every case whose frames have more than one pixel (a
     1 x 1 frame's tile is its one term, so there the defined order IS the
     sequential one, and the test asserts that too);
  2. hostile frames (NaN, +-inf, -0 words) with and without
     RTG_FOLD_SKIP_NONFINITE, the skip counts, canonical NaN words;
  3. thread counts;
  4. rtg_render_views_fold_host against the fold of rtg_render_views_host(walk
     0), both walks and semantics, G = 1 on four scenes and G = 6 on a cube;
  5. rtg_cube_sh_weights against a numpy double restatement (<= 1 ulp), its
     k = 0 column, and the fold of an all-ones cube;
  6. the argument errors of the contract, host and one-shot forms, with no GPU
     call (this tier has no GPU).

test_gpu_views_fold.py shares the cases of this file.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest

from test_raytrace_host import THREADS, scene_with_lights
from test_views_host import (CUBE, VAA, VH, VIEW_SCENES, VS, VW, VZOOM, batch_poses, view_frames)

F = np.float32
CANON = 0xFFC00000
SHAPES = [(1, 1), (8, 8), (9, 9), (16, 8), (7, 5), (17, 9)]  # W, H
GROUP_SIZES = [1, 2, 6]
WEIGHT_COUNTS = [1, 9, 16]
SKIP = 1  # RTG_FOLD_SKIP_NONFINITE


# ---- the cases ----

def random_frames(rng, n, W, H):
    """Magnitudes over 2^-6 .. 2^6 with both signs: sums whose roundings depend
    on the order of their terms."""
    mant = rng.uniform(1.0, 2.0, (n, H, W, 3))
    expo = rng.integers(-6, 7, (n, H, W, 3))
    sign = rng.choice([-1.0, 1.0], (n, H, W, 3))
    return (sign * mant * np.exp2(expo)).astype(F)


def random_weights(rng, G, W, H, K):
    return rng.normal(0.0, 1.0, (G, H, W, K)).astype(F)


def hostile_frames(rng, n, W, H, G):
    """random_frames with NaN, +inf, -inf and -0 words sprinkled in; texel 0 of
    every group's first view stays finite, so each group keeps a texel."""
    fr = random_frames(rng, n, W, H)
    flat = fr.reshape(-1)
    bad = np.array([np.nan, np.inf, -np.inf, -0.0], F)
    hit = rng.random(flat.size) < 0.08
    flat[hit] = bad[rng.integers(0, 4, int(hit.sum()))]
    assert G * W * H > 1, "no room for a spoilt texel besides the kept one"
    fr[n - 1, H - 1, W - 1, 1] = np.nan  # (never a kept texel)
    fr[::G, 0, 0] = F(1.5)
    return fr


@functools.lru_cache(maxsize=None)
def fold_cases():
    """(name, frames, weights, G, K) of every shape, group size and weight count,
    with one and three groups, and 70 groups of 1 x 1: computed once, read-only."""
    rng = np.random.default_rng(20261020)
    out = []
    for W, H in SHAPES:
        for G in GROUP_SIZES:
            for groups in (1, 3):
                for K in WEIGHT_COUNTS:
                    out.append((f"{W}x{H} G{G} g{groups} K{K}", random_frames(rng, G * groups, W, H),
                                random_weights(rng, G, W, H, K), G, K))
    for K in (1, 16):
        out.append((f"1x1 G1 g70 K{K}", random_frames(rng, 70, 1, 1),
                    random_weights(rng, 1, 1, 1, K), 1, K))
    for _, fr, w, _, _ in out:
        fr.setflags(write=False)
        w.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hostile_cases():
    """The same tuples over frames with non-finite and -0 words."""
    rng = np.random.default_rng(7)
    out = []
    for (W, H), G, groups, K in (((9, 9), 1, 3, 9), ((17, 9), 2, 3, 16), ((7, 5), 6, 1, 1),
                                 ((16, 8), 6, 3, 9), ((8, 8), 2, 1, 16), ((1, 1), 6, 3, 9),
                                 ((1, 1), 2, 35, 16)):
        fr = hostile_frames(rng, G * groups, W, H, G)
        w = random_weights(rng, G, W, H, K)
        fr.setflags(write=False)
        w.setflags(write=False)
        out.append((f"hostile {W}x{H} G{G} g{groups} K{K}", fr, w, G, K))
    return tuple(out)


# ---- the restatement ----

def nonfinite_pixels(frames):
    """(n, H, W) bool: a word whose exponent field is all ones."""
    return ((frames.view(np.uint32) & 0x7F800000) == 0x7F800000).any(-1)


def terms_of(frames, weights, G, skip):
    """(n, H, W, K, 3) float32 terms w * pix, +0 for a skipped pixel."""
    n = frames.shape[0]
    w = np.tile(weights, (n // G, 1, 1, 1))  # view v takes table f = v % G
    with np.errstate(all="ignore"):
        t = (w[..., :, None] * frames[..., None, :]).astype(F)
    if skip:
        t[nonfinite_pixels(frames)] = F(0)
    return t


def canon(a):
    b = np.ascontiguousarray(a, F).view(np.uint32).copy()
    b[np.isnan(a)] = CANON
    return b


def restate_fold(frames, weights, G, K, skip=False):
    """rtg.h's order in numpy float32: ((nGroups, K, 3) uint32 words, counts)."""
    n, H, W = frames.shape[:3]
    tx, ty = (W + 7) // 8, (H + 7) // 8
    pad = np.zeros((n, ty * 8, tx * 8, K, 3), F)  # a lane outside the frame holds +0.f
    pad[:, :H, :W] = terms_of(frames, weights, G, skip)
    v = pad.reshape(n, ty, 8, tx, 8, 3 * K).transpose(0, 1, 3, 2, 4, 5).reshape(n * ty * tx, 64,
                                                                                3 * K).copy()
    with np.errstate(all="ignore"):
        s = 1
        while s < 64:
            v[:, ::2 * s] += v[:, s::2 * s]
            s *= 2
        sums = v[:, 0].reshape(n // G, G * ty * tx, 3 * K)  # a group's tiles, view by view
        acc = np.zeros((n // G, 3 * K), F)
        for t in range(sums.shape[1]):
            acc = acc + sums[:, t]
    counts = (nonfinite_pixels(frames).reshape(n // G, -1).sum(1) if skip
              else np.zeros(n // G, np.int64)).astype(np.uint32)
    return canon(acc).reshape(n // G, K, 3), counts


def sequential_fold(frames, weights, G, K, skip=False):
    """The same terms added one after another in texel order."""
    n = frames.shape[0]
    t = terms_of(frames, weights, G, skip).reshape(n // G, -1, 3 * K)
    acc = np.zeros((n // G, 3 * K), F)
    with np.errstate(all="ignore"):
        for e in range(t.shape[1]):
            acc = acc + t[:, e]
    return canon(acc).reshape(n // G, K, 3)


def host_fold(R, frames, weights, G, K, flags=0, threads=1):
    out, cnt = R.views_fold_host(frames, weights, R.fold_params(G, K, flags), threads=threads,
                                 skipped=True)
    assert out.shape == (frames.shape[0] // G, K, 3) and out.dtype == F
    return out.view(np.uint32), cnt


# ---- 1. the definition ----

def test_fold_equals_the_restatement(rtg):
    for name, fr, w, G, K in fold_cases():
        got, cnt = host_fold(rtg, fr, w, G, K)
        want, _ = restate_fold(fr, w, G, K)
        assert got.tobytes() == want.tobytes(), name
        assert (cnt == 0).all(), name
        seq = sequential_fold(fr, w, G, K)
        if fr.shape[1] * fr.shape[2] > 1:
            assert (seq != want).any(), (name, "the sequential sum is the same words")
        else:  # 1 x 1: a tile is its one term, and the tile loop IS the sequential sum
            assert (seq == want).all(), name
        assert np.isfinite(got.view(F)).all() and (got.view(F) != 0).all(), name


def test_fold_without_a_count(rtg):
    name, fr, w, G, K = fold_cases()[40]
    out = rtg.views_fold_host(fr, w, rtg.fold_params(G, K))
    assert out.view(np.uint32).tobytes() == restate_fold(fr, w, G, K)[0].tobytes(), name


# ---- 2. hostile frames ----

def test_hostile_frames(rtg):
    for name, fr, w, G, K in hostile_cases():
        n = fr.shape[0]
        bad = nonfinite_pixels(fr).reshape(n // G, -1)
        assert bad.any(), name
        assert (~bad).any(1).all(), (name, "a group without a texel")
        for flags in (0, SKIP):
            got, cnt = host_fold(rtg, fr, w, G, K, flags)
            want, wcnt = restate_fold(fr, w, G, K, bool(flags))
            assert got.tobytes() == want.tobytes(), (name, flags)
            assert (cnt == wcnt).all() and cnt.dtype == np.uint32, (name, flags, cnt, wcnt)
            nan = np.isnan(got.view(F))
            assert (got[nan] == CANON).all()
            if flags:
                assert cnt.sum() >= 1 and np.isfinite(got.view(F)).all(), name
            else:  # inf * w and NaN * w reach the sums
                assert not np.isfinite(got.view(F)).all(), name
    # a frame of -0 words with positive weights: +0 lanes and +0 accumulators make +0
    fr = np.full((1, 3, 3, 3), -0.0, F)
    got, _ = host_fold(rtg, fr, np.ones((1, 3, 3, 2), F), 1, 2)
    assert (got == 0).all(), got


# ---- 3. thread counts ----

def test_thread_counts(rtg):
    for name, fr, w, G, K in fold_cases()[-2:] + hostile_cases()[:2] + fold_cases()[50:53]:
        for flags in (0, SKIP):
            one = host_fold(rtg, fr, w, G, K, flags, 1)
            many = host_fold(rtg, fr, w, G, K, flags, THREADS)
            assert one[0].tobytes() == many[0].tobytes() and (one[1] == many[1]).all(), name


# ---- 4. host render + fold ----

@pytest.mark.parametrize("scene", VIEW_SCENES)
def test_render_fold_equals_the_composition(rtg, scene):
    sph, lg = scene_with_lights(scene)
    cams = batch_poses(scene)
    w = random_weights(np.random.default_rng(3), 1, VW, VH, 9)
    p = rtg.fold_params(1, 9, SKIP)
    for sem in (0, 1):
        want = rtg.views_fold_host(view_frames(scene, sem), w, p, skipped=True)
        for walk in (0, 1):
            got = rtg.render_views_fold_host(sph, lg, cams, VW, VH, w, p, VZOOM, VAA, VS,
                                             semantics=sem, walk=walk, threads=THREADS,
                                             skipped=True)
            assert got[0].tobytes() == want[0].tobytes(), (sem, walk)
            assert (got[1] == want[1]).all(), (sem, walk)
    assert (want[0] != 0).any()


def test_render_fold_of_a_cube(rtg):
    sph, lg = scene_with_lights("reference")
    res, aa = 8, 2.0
    cams = np.concatenate([rtg.camera_cube(e) for e in ((0, 0, -4), (1.0, 0.5, -6.0))])
    w = rtg.cube_sh_weights(res, 3, aa)
    p = rtg.fold_params(6, 9)
    frames = rtg.render_views_host(sph, lg, cams, res, res, -1.0, aa, 6, threads=THREADS)
    want = rtg.views_fold_host(frames, w, p)
    assert want.shape == (2, 9, 3) and (want != 0).any() and want[0].tobytes() != want[1].tobytes()
    for walk in (0, 1):
        got = rtg.render_views_fold_host(sph, lg, cams, res, res, w, p, -1.0, aa, 6, walk=walk,
                                         threads=THREADS)
        assert got.tobytes() == want.tobytes(), walk
    assert want.view(np.uint32).tobytes() == restate_fold(frames, w, 6, 9)[0].tobytes()


# ---- 5. the SH weights ----

SH_C = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005,
        0.5462742152960396, 0.5900435899266435, 2.890611442640554, 0.4570457994644658,
        0.3731763325901154, 1.445305721320277)


def real_sh(x, y, z):
    """The 16 real SH of bands 0..3, k = l(l+1)+m, in double."""
    c = SH_C
    return [c[0] + 0 * x, c[1] * y, c[1] * z, c[1] * x,
            c[2] * (x * y), c[2] * (y * z), c[3] * (3.0 * (z * z) - 1.0), c[2] * (x * z),
            c[4] * (x * x - y * y),
            c[5] * (y * (3.0 * (x * x) - y * y)), c[6] * ((x * y) * z),
            c[7] * (y * (5.0 * (z * z) - 1.0)), c[8] * (z * (5.0 * (z * z) - 3.0)),
            c[7] * (x * (5.0 * (z * z) - 1.0)), c[9] * (z * (x * x - y * y)),
            c[5] * (x * (x * x - 3.0 * (y * y)))]


def restate_sh_weights(res, bands, aa):
    """rtg.h's table in numpy double, rounded once: (6, res, res, bands^2)."""
    n_aa = 0
    while F(n_aa) < F(aa):
        n_aa += 1
    cell = 2.0 / res
    mean = 0.5 * (n_aa - 1) if n_aa > 0 else 0.0
    du = mean * (2.0 / (float(res) * float(F(aa))))
    dv = mean * ((8.0 / 3.0) / (float(res) * float(F(aa))))
    x, y = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64))
    u0, v0 = -1.0 + cell * x, 1.0 - cell * y
    u1, v1 = u0 + cell, v0 + cell

    def corner(u, v):
        return np.arctan2(u * v, np.sqrt((u * u + v * v) + 1.0))

    omega = ((corner(u1, v1) - corner(u0, v1)) - corner(u1, v0)) + corner(u0, v0)
    scale = (4.0 * math.pi) / (6.0 * math.fsum(omega.reshape(-1)))
    out = np.zeros((6, res, res, bands * bands), F)
    for f, (fw, r, up) in enumerate(CUBE):
        u, v = u0 + du, v0 + dv
        d = [(float(fw[q]) + u * float(r[q])) + v * float(up[q]) for q in range(3)]
        ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        Y = real_sh(d[0] / ln, d[1] / ln, d[2] / ln)
        for k in range(bands * bands):
            out[f, :, :, k] = (Y[k] * (omega * scale)).astype(F)
    return out, omega * scale


def ulps_apart(a, b):
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("res,bands,aa", [(1, 1, 1.0), (4, 2, 1.0), (8, 3, 2.5), (16, 4, 3.0),
                                          (32, 3, 1.0)])
def test_cube_sh_weights(rtg, res, bands, aa):
    got = rtg.cube_sh_weights(res, bands, aa)
    want, omega = restate_sh_weights(res, bands, aa)
    assert got.shape == want.shape == (6, res, res, bands * bands) and got.dtype == F
    assert ulps_apart(got, want).max() <= 1
    assert abs(6.0 * math.fsum(omega.reshape(-1)) - 4.0 * math.pi) < 1e-12
    # the k = 0 column: Y_0 * 4 pi = 2 sqrt(pi), each value rounded once
    col = math.fsum(got[..., 0].reshape(-1).astype(np.float64))
    assert abs(col - 2.0 * math.sqrt(math.pi)) <= 2.0 ** -24 * 2.0 * math.sqrt(math.pi)
    # an all-ones cube folds to c0 = 2 sqrt(pi): six tree levels and one add per
    # tile of the group, each within 2^-24 relative
    tiles = 6 * ((res + 7) // 8) ** 2
    out = rtg.views_fold_host(np.ones((6, res, res, 3), F), got, rtg.fold_params(6, bands * bands))
    bound = (6 + tiles) * 2.0 ** -24 * 2.0 * math.sqrt(math.pi)
    assert (np.abs(out[0, 0].astype(np.float64) - 2.0 * math.sqrt(math.pi)) <= bound).all(), out


def test_cube_sh_weights_errors(rtg):
    L = rtg.lib()
    out = np.full(6 * 16, 7.0, F)
    P = ctypes.c_void_p(out.ctypes.data)
    f = ctypes.c_float
    for args, msg in (((2, 2, f(1.0), None), "null pointer"), ((0, 2, f(1.0), P), "empty frame"),
                      ((2, 0, f(1.0), P), "bands 0"), ((2, 5, f(1.0), P), "bands 5"),
                      ((2, 2, f(257.0), P), "aliasFactor"),
                      ((2, 2, f(float("nan")), P), "aliasFactor")):
        assert L.rtg_cube_sh_weights(*args) == -1 and msg.encode() in L.rtg_last_error(), args
    assert (out == 7.0).all()


# ---- 6. argument errors ----

def test_argument_errors(rtg):
    L = rtg.lib()
    sph, lg = scene_with_lights("reference")
    cams = np.concatenate([rtg.camera_cube((0, 0, -4))] * 2).view(F).reshape(12, 12)
    frames = np.ones((12, 4, 4, 3), F)
    w = np.ones((6, 4, 4, 2), F)
    out = np.full((2, 2, 3), 7.0, F)
    cnt = np.full(2, 7, np.uint32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    f = ctypes.c_float

    def params(G=6, K=2, flags=0):
        return rtg.fold_params(G, K, flags)

    def fold(fr=P(frames), n=12, W=4, H=4, p=params(), wt=P(w), dst=P(out), sk=P(cnt), **_):
        rc = L.rtg_views_fold_host(fr, n, W, H, P(p) if p is not None else None, wt, dst, sk, 2)
        return rc, L.rtg_last_error().decode()

    def host(c=P(cams), n=12, W=4, H=4, p=params(), wt=P(w), dst=P(out), sk=P(cnt), aa=1.0, S=6,
             sem=0, walk=0, spheres=P(sph), lights=P(lg), **_):
        rc = L.rtg_render_views_fold_host(spheres, len(sph), lights, len(lg), c, n, W, H, f(-1.0),
                                          f(aa), S, sem, P(p) if p is not None else None, wt, dst,
                                          sk, walk, 2)
        return rc, L.rtg_last_error().decode()

    def one_shot(c=P(cams), n=12, W=4, H=4, p=params(), wt=P(w), dst=P(out), sk=P(cnt), aa=1.0,
                 S=6, spheres=P(sph), lights=P(lg), **_):
        rc = L.rtg_render_views_fold(0, spheres, len(sph), lights, len(lg), c, n, W, H, f(-1.0),
                                     f(aa), S, P(p) if p is not None else None, wt, dst, sk)
        return rc, L.rtg_last_error().decode()

    shared = ((dict(p=None), "null params"),
              (dict(wt=None), "null weight table"),
              (dict(dst=None), "null output"),
              (dict(p=params(G=0)), "viewsPerGroup 0"),
              (dict(p=params(G=5)), "not a multiple of viewsPerGroup 5"),
              (dict(n=11), "11 views are not a multiple"),
              (dict(p=params(K=0)), "weights 0 outside"),
              (dict(p=params(K=17)), "weights 17 outside"),
              (dict(p=params(flags=2)), "unknown flag 0x2"),
              (dict(p=params(flags=0x80000001)), "unknown flag"),
              (dict(W=0), "empty frame"),
              (dict(H=0), "empty frame"),
              (dict(n=0, p=params(K=17)), "weights 17 outside"),  # no views, and still an argument
              (dict(n=0, p=params(G=0)), "viewsPerGroup 0"),
              (dict(n=0, dst=None), "null output"),
              (dict(n=3 << 20, W=4096, H=4096, p=params(G=3)), "2^31-1 workgroups"),
              (dict(n=1 << 31, W=1, H=1, p=params(G=2)), "2^31-1 workgroups"),
              # no views, and a table of 2^32 - 1 faces of 2^32 texels and 16 weights
              (dict(n=0, W=65536, H=65536, p=params(G=0xFFFFFFFF, K=16)), "weight table too large"))
    for call in (fold, host, one_shot):
        for kw, msg in shared:
            rc, err = call(**kw)
            assert rc == -1 and msg in err, (call.__name__, kw, rc, err)  # RTG_ERR_INVALID
    # what rtg_render_views* rejects
    for call in (host, one_shot):
        for kw, msg in ((dict(c=None), "null pose table"), (dict(spheres=None), "null scene array"),
                        (dict(lights=None), "null scene array"), (dict(aa=257.0), "aliasFactor"),
                        (dict(aa=float("nan")), "aliasFactor"), (dict(S=0), "stackSize 0 outside"),
                        (dict(S=17), "stackSize 17 outside"),
                        (dict(n=0, S=0), "stackSize 0 outside")):
            rc, err = call(**kw)
            assert rc == -1 and msg in err, (call.__name__, kw, rc, err)
    for kw, msg in ((dict(sem=2), "semantics 2"), (dict(walk=2), "walk 2"), (dict(walk=-1), "walk -1")):
        rc, err = host(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    rc, err = fold(fr=None)
    assert rc == -1 and "null frames" in err
    assert (out == 7.0).all() and (cnt == 7).all()  # nothing was written, on any form
    # no views: nothing to do, and no table of poses or frames is needed
    for call, kw in ((fold, dict(fr=None)), (host, dict(c=None)), (one_shot, dict(c=None))):
        rc, err = call(n=0, **kw)
        assert rc == 0 and err == "", (call.__name__, err)
    assert (out == 7.0).all() and (cnt == 7).all()
    # the count is optional
    rc, err = fold(sk=None)
    assert rc == 0 and err == "" and (out != 7.0).all()

    # the scratch size
    size = ctypes.c_size_t(7)
    B = ctypes.byref(size)
    for args, msg in (((12, 4, 4, 2, None), "null pointer"), ((12, 0, 4, 2, B), "empty frame"),
                      ((12, 4, 4, 0, B), "weights 0 outside"), ((12, 4, 4, 17, B), "weights 17"),
                      ((1 << 31, 1, 1, 1, B), "2^31-1 workgroups")):
        assert L.rtg_views_fold_scratch(*args) == -1 and msg.encode() in L.rtg_last_error(), args
    assert size.value == 7
    assert rtg.views_fold_scratch(0, 4, 4, 2) == 0
    assert rtg.views_fold_scratch(12, 4, 4, 2) == 12 * 1 * 7 * 4
    assert rtg.views_fold_scratch(5, 17, 9, 16) == 5 * 6 * 49 * 4
    with pytest.raises(rtg.RtgError, match="weights 17"):
        rtg.views_fold_host(frames, w, rtg.fold_params(6, 17))
