"""Inputs and references shared by the probe-grid lookup's tests
(test_irradiance_host.py, test_gpu_irradiance.py): the scenes (aogen.SCENES),
hit records (mattegen.hits with eight more hand-made ones), the grids, seeded
coefficients and validity bytes, a numpy float32 restatement of the definition
(include/rtg.h, "irradiance"), one operation per line, and the plain-loop
answers, computed once and left unchanged.

Records 6..13 of a scene's batch are real points moved by hand: one exactly on
a lattice plane of the scene's lattice (so that it has corners of weight 0),
one far outside the lattice on each of its six sides, and one with a NaN
coordinate under id >= 0.

Grids per scene: "lattice" (DIMS[name] probes over raygen.bounds of the scene,
origin and step multiples of 1/8 so that lattice planes are exact in float),
"flat" (the same with ny = 1: a floor plan) and "one" (1 x 1 x 1).
"""
from __future__ import annotations

import functools

import numpy as np

import aogen
import mattegen
import raygen
from aogen import N_POINTS, PATHS, SCENES, SIZES  # noqa: F401  (re-exported)
from test_raytrace_host import THREADS

F = np.float32
BIAS = 1e-3
BANDS = (1, 2, 3)
VALID, FACING, VISIBLE = 1, 2, 4
FLAG_SETS = tuple(range(8))  # every subset of the three flags
GRIDS = ("lattice", "flat", "one")
LOBE = (1.0, 0.75, -0.5)  # the tests' own: neither of the header's two
ON_PLANE, OUTSIDE, NAN_POINT = 6, range(7, 13), 13  # the hand-made records
# The lattice of each scene, chosen so that with RTG_IRR_VISIBLE alone the share
# of positive-weight (point, corner) pairs that visible_host(walk 0) reports
# blocked lies in [0.1, 0.9] (the measured share is noted).
DIMS = {
    "none": (3, 3, 3),       # 0.000: no sphere, nothing is blocked
    "reference": (3, 3, 3),  # 0.584
    12: (3, 3, 3),           # 0.570
    40: (3, 3, 3),           # 0.699
    "base65": (3, 3, 3),     # 0.543
    "base150": (3, 3, 3),    # 0.634
    "c5": (12, 12, 12),      # 0.829 (0.862 at 6 per axis, 0.818 at 16)
    "cnan150": (3, 3, 3),    # 0.633
}
C0, C1, C2, C3, C4 = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792,
                      0.31539156525252005, 0.5462742152960396)  # real_sh's doubles


def scene(name):
    return aogen.scene(name)


def _eighths(v, up):
    return (np.ceil if up else np.floor)(np.asarray(v, np.float64) * 8) / 8


def lattice_over(geo, dims, bands, centred=False):
    """A PROBE_GRID_DTYPE record of dims probes over raygen.bounds(geo), origin
    and step multiples of 1/8; centred: the origin in the middle of the bounds."""
    import rtg_amd as R
    lo, hi = raygen.bounds(geo)
    origin = _eighths(lo, False)
    step = np.array([_eighths((hi[q] - origin[q]) / (dims[q] - 1), True) if dims[q] > 1 else 1.0
                     for q in range(3)])
    if centred:
        origin = _eighths(0.5 * (lo + hi), False)
    g = R.probe_grid(origin, step, dims, bands)
    assert (g["origin"][0].astype(np.float64) == origin).all() and (g["step"][0] == step).all()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _grid(name, kind, bands):
    dims = {"lattice": DIMS[name], "flat": (DIMS[name][0], 1, DIMS[name][2]), "one": (1, 1, 1)}[kind]
    return lattice_over(aogen.ray_scene(name), dims, bands, centred=kind == "one")


def grid(name, kind="lattice", bands=3):
    """One PROBE_GRID_DTYPE record, read-only."""
    return _grid(name, kind, bands)


def probes(g):
    return int(g["nx"][0]) * int(g["ny"][0]) * int(g["nz"][0])


@functools.lru_cache(maxsize=None)
def hits(name):
    """mattegen.hits(name) with records 6..13 moved by hand, read-only."""
    h = mattegen.hits(name).copy()
    g = grid(name)
    o, s = g["origin"][0].astype(np.float64), g["step"][0].astype(np.float64)
    dims = np.array(DIMS[name])
    real = np.flatnonzero(h["id"] >= 0)
    real = real[real > NAN_POINT]
    span = s * (dims - 1)
    h[ON_PLANE] = h[real[0]]
    h[ON_PLANE]["normal"] = (0.0, 1.0, 0.0)  # A.x = P.x: bias * 0 adds nothing
    h[ON_PLANE]["point"] = o + s * (1.0, 0.4, 1.6)  # x on the lattice plane ix = 1
    for k, at in enumerate(OUTSIDE):
        q, side = k // 2, k % 2
        h[at] = h[real[1 + k]]
        p = o + 0.37 * span
        p[q] = o[q] + span[q] + 1.0e4 * span.max() if side else o[q] - 1.0e4 * span.max()
        h[at]["point"] = p
    h[NAN_POINT] = h[real[8]]
    h[NAN_POINT]["point"][0] = np.nan
    assert (h["id"][[ON_PLANE, NAN_POINT, *OUTSIDE]] >= 0).all()
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def coeffs(name, kind, bands):
    """(probes * K, 3) float32 in [-1, 1) with one NaN, one -0 and one infinite
    word, each in band 0 of a probe that a record with a point uses (the three
    channels of the one probe of a 1 x 1 x 1 grid)."""
    g = grid(name, kind, bands)
    n = probes(g) * bands * bands
    rng = np.random.default_rng(3100 + 7 * n + bands)
    c = rng.uniform(-1, 1, size=(n, 3)).astype(F)
    flat = c.reshape(-1)
    h = hits(name)
    _, p, w, _ = corners(h, g, BIAS)
    used = np.unique(p[(w > 0) & (h["id"] >= 0)[:, None]])
    at = [3 * bands * bands * int(used[(j * len(used)) // 3]) + j for j in range(3)]
    assert len(set(at)) == 3
    flat[at[0]], flat[at[1]], flat[at[2]] = np.nan, -0.0, np.inf
    assert np.signbit(flat[at[1]])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def valid(name, kind):
    """One byte per probe, about a quarter zero (a single probe is valid)."""
    n = probes(grid(name, kind))
    v = (np.random.default_rng(3300 + n).random(n) >= 0.25).astype(np.uint8)
    if n == 1:
        v[:] = 1
    else:
        assert 0 < int((v == 0).sum()) < n
    v.setflags(write=False)
    return v


def params(R, flags, lobe=LOBE, bias=BIAS):
    return R.irradiance_params(bias, lobe, flags)


@functools.lru_cache(maxsize=None)
def want(name, kind, bands, flags):
    """(colours, weights) of hits(name) by the plain loops (irradiance_host walk
    0), read-only."""
    import rtg_amd as R
    out, w = R.irradiance_host(scene(name), hits(name), grid(name, kind, bands),
                               coeffs(name, kind, bands), params(R, flags), valid(name, kind),
                               walk=0, threads=THREADS, weight=True)
    out.setflags(write=False)
    w.setflags(write=False)
    return out, w


def canon(a):
    return aogen.canon(a)


def same_words(got, want_):
    return mattegen.same_words(got, want_)


# ---- the definition restated in numpy float32, one operation a line ----

def _axis(a, origin, step, n):
    """(i0, i1, f) of rtg.h's `cell` for one axis."""
    with np.errstate(all="ignore"):
        diff = a - F(origin)
        g = diff / F(step)
        g = np.where(g >= F(0), g, F(0))  # NaN goes to 0
        top = F(n - 1)
        g = np.where(g > top, top, g)
        i0 = g.astype(np.int64)
        if n >= 2:
            i0 = np.minimum(i0, n - 2)
        f = g - i0.astype(F)
        i1 = np.where(i0 + 1 < n, i0 + 1, i0)
    assert g.dtype == F and f.dtype == F
    return i0, i1, f


def corners(h, g, bias):
    """The start points A (n, 3), and per corner c = 0..7 the probe index p
    (n, 8), the trilinear weight w (n, 8) and the probe position X (n, 8, 3),
    all float32 as rtg.h forms them."""
    P = h["point"].astype(F)
    N = h["normal"].astype(F)
    bias = F(bias)
    o, s = g["origin"][0], g["step"][0]
    dims = (int(g["nx"][0]), int(g["ny"][0]), int(g["nz"][0]))
    n = len(h)
    with np.errstate(all="ignore"):
        A = np.zeros((n, 3), F)
        for q in range(3):
            off = bias * N[:, q]
            A[:, q] = P[:, q] + off
        ax = [_axis(A[:, q], o[q], s[q], dims[q]) for q in range(3)]
        p = np.zeros((n, 8), np.int64)
        w = np.zeros((n, 8), F)
        X = np.zeros((n, 8, 3), F)
        for c in range(8):
            bit = (c & 1, (c >> 1) & 1, c >> 2)
            i = [ax[q][1] if bit[q] else ax[q][0] for q in range(3)]
            t = [ax[q][2] if bit[q] else F(1) - ax[q][2] for q in range(3)]
            txy = t[0] * t[1]
            w[:, c] = txy * t[2]
            p[:, c] = (i[2] * dims[1] + i[1]) * dims[0] + i[0]
            for q in range(3):
                along = i[q].astype(F) * s[q]
                X[:, c, q] = o[q] + along
    assert (p >= 0).all() and (p < dims[0] * dims[1] * dims[2]).all()
    return A, p, w, X


def segments(h, g, bias):
    """The (n * 8, 6) float32 segments (A, X_p), point-major."""
    A, _, _, X = corners(h, g, bias)
    out = np.zeros((len(h), 8, 6), F)
    out[..., :3] = A[:, None, :]
    out[..., 3:] = X
    return out.reshape(len(h) * 8, 6)


def basis(N, lobe, bands):
    """b_0 .. b_{K-1}, each (n,) float32."""
    l0, l1, l2 = (F(v) for v in lobe)
    c0, c1, c2, c3, c4 = F(C0), F(C1), F(C2), F(C3), F(C4)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    with np.errstate(all="ignore"):
        b = [np.full(len(N), l0 * c0, F)]
        if bands >= 2:
            b.append(l1 * (c1 * y))
            b.append(l1 * (c1 * z))
            b.append(l1 * (c1 * x))
        if bands >= 3:
            xy = x * y
            yz = y * z
            zz = z * z
            xz = x * z
            xx = x * x
            yy = y * y
            b.append(l2 * (c2 * xy))
            b.append(l2 * (c2 * yz))
            zz3 = F(3) * zz
            b.append(l2 * (c3 * (zz3 - F(1))))
            b.append(l2 * (c2 * xz))
            b.append(l2 * (c4 * (xx - yy)))
    assert all(v.dtype == F for v in b)
    return b


def restate(h, g, coef, valid_, lobe, bias, flags, vis):
    """(colours (n, 3), weights (n,), kept (n, 8)) of HIT_DTYPE records `h`, with
    the line of sight `vis` ((n, 8), nonzero: clear) taken from rtg_visible on
    segments(h, g, bias); `vis` may be None without VISIBLE."""
    bands = int(g["bands"][0])
    K = bands * bands
    n = len(h)
    N = h["normal"].astype(F)
    real = h["id"] >= 0
    A, p, w, X = corners(h, g, bias)
    b = basis(N, lobe, bands)
    coef = np.asarray(coef, F).reshape(-1, 3)
    acc = np.zeros((n, 3), F)
    W = np.zeros(n, F)
    kept = np.zeros((n, 8), bool)
    with np.errstate(all="ignore"):
        for c in range(8):
            keep = real & (w[:, c] > F(0))
            if flags & VALID:
                keep &= np.asarray(valid_)[p[:, c]] != 0
            if flags & FACING:
                dx = X[:, c, 0] - A[:, 0]
                dy = X[:, c, 1] - A[:, 1]
                dz = X[:, c, 2] - A[:, 2]
                sx = N[:, 0] * dx
                sy = N[:, 1] * dy
                sz = N[:, 2] * dz
                sxy = sx + sy
                s = sxy + sz
                keep &= s > F(0)
            if flags & VISIBLE:
                keep &= np.asarray(vis)[:, c] != 0
            kept[:, c] = keep
            Wn = W + w[:, c]
            W = np.where(keep, Wn, W)
            for q in range(3):
                e = np.zeros(n, F)
                for k in range(K):
                    term = b[k] * coef[p[:, c] * K + k, q]
                    e = e + term
                we = w[:, c] * e
                added = acc[:, q] + we
                acc[:, q] = np.where(keep, added, acc[:, q])
        out = np.zeros((n, 3), F)
        for q in range(3):
            quot = acc[:, q] / W
            out[:, q] = np.where(W > F(0), quot, F(0))
    assert out.dtype == F and W.dtype == F
    return out, W, kept


# ---- the host driver's grid (rtg_main --probe-grid), restated in numpy float32 ----

def driver_grid(R, sph, dims, bands):
    """The lattice rtg_main lays over a scene's bounds: per axis lo = the least
    pos - |radius|, hi = the greatest pos + |radius|, origin = lo, step = (hi -
    lo) / (float)(n - 1) for n >= 2, else 1 (and 1 for a step that is not > 0)."""
    c = sph["pos"].astype(F)
    r = np.abs(sph["radius"].astype(F))[:, None]
    low = c - r
    high = c + r
    lo = low.min(0) if len(sph) else np.full(3, -1, F)
    hi = high.max(0) if len(sph) else np.full(3, 1, F)
    step = np.ones(3, F)
    for q in range(3):
        if dims[q] >= 2:
            span = hi[q] - lo[q]
            step[q] = span / F(dims[q] - 1)
        if not step[q] > 0:
            step[q] = 1
    assert lo.dtype == F and step.dtype == F
    return R.probe_grid(lo, step, dims, bands)
