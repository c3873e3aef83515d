"""Inputs and references shared by the variance and svgf tests
(test_svgf_host.py, test_gpu_svgf.py): accumulated state, variance fields, the
parameter sets, a numpy float32 restatement of rtg_variance* and rtg_svgf*
(include/rtg.h, "variance and svgf"), one operation a line, and the host
loops' answers, computed once and left unchanged.

Guides, frames and the float signals are filtergen's: 1 x 1, 5 x 1, 1 x 7,
8 x 8, 33 x 17 and 67 x 35 on `reference`, 12 and c5, with the planted records.
The thin frames are narrower than the 7 x 7 window and the 3 x 3 prefilter;
33 x 17 and 67 x 35 have partial tiles.
"""
from __future__ import annotations

import functools

import numpy as np

import filtergen as G
from filtergen import ALL, FRAMES, FULL, NORMAL, PLANE, SAME_ID, SCENES, SKIP  # noqa: F401
from test_raytrace_host import THREADS

F = np.float32
INF, NAN = float("inf"), float("nan")
LUMA = 16
SIGNALS = ["rgb", "gray"]  # the states are floats: no counts
KINDS = G.KINDS

# ---- rtg_svgf*'s parameter sets ----
# (passes, flags, normalLog2, planeScale, luma, sigmaL, epsL): every set of
# filtergen with LUMA off and with LUMA at (4, 1e-6); then sigmaL 0 (only equal
# luminances pass), +inf and NaN (no tap passes: the pixel keeps its value),
# epsL 0, and both 0 (0 * inf: a NaN, which the clamp sends to 0).
SVGF_SETS = [st + (False, 4.0, 1e-6) for st in G.SETS] + [st + (True, 4.0, 1e-6) for st in G.SETS] + [
    (2, ALL, 3, None, True, 0.0, 1e-6), (2, SAME_ID, 0, 0.0, True, INF, 1e-6),
    (2, ALL, 3, None, True, NAN, 1e-6), (5, ALL, 3, None, True, 4.0, 0.0),
    (2, 0, 0, 0.0, True, 0.0, 0.0),
]
# the same-step sets the forced forms and the thread counts take
SVGF_FEW = [SVGF_SETS[2], SVGF_SETS[18 + 2], SVGF_SETS[18 + 3], SVGF_SETS[18 + 5], SVGF_SETS[-2]]

# ---- rtg_variance*'s parameter sets ----
# (flags, normalLog2, planeScale, minHistory): minHistory 0, 4 and 65535 with
# each flag alone, all and none.
VAR_SETS = [(f, 3 if f & NORMAL else 0, None if f & PLANE else 0.0, mh)
            for mh in (0, 4, 65535) for f in (0, SAME_ID, NORMAL, PLANE, SKIP, ALL)]
# The len fields: seeded in 0 .. 8; every history long (no tile stages); every
# history 0 (every tile with a hit stages); exactly one short hit pixel.
LEN_FIELDS = ["seeded", "long", "zero", "one"]
# what the three constructed fields run with
VAR_FEW = [(ALL, 3, None, 4), (0, 0, 0.0, 4), (SAME_ID, 0, 0.0, 65535)]


def variance_cases():
    return [(lf, st) for lf in LEN_FIELDS for st in (VAR_SETS if lf == "seeded" else VAR_FEW)]


def svgf_params(R, name, kind, st):
    p, f, n, s, luma, sigma, eps = st
    return R.svgf_params(p, KINDS[kind], f | (LUMA if luma else 0), G.plane_scale(name, s), n,
                         sigma, eps)


def variance_params(R, name, kind, st):
    f, n, s, mh = st
    return R.variance_params(KINDS[kind], f, G.plane_scale(name, s), n, mh)


def _real(name, W, H):
    return np.flatnonzero(G.guides(name, W, H)["id"] >= 0)


def _inner_block(ids):
    """(x, y) of the centre of the last 3 x 3 block of one id >= 0, or None."""
    H, W = ids.shape
    for y in range(H - 2, 0, -1):
        for x in range(W - 2, 0, -1):
            b = ids[y - 1:y + 2, x - 1:x + 2]
            if b[0, 0] >= 0 and (b == b[0, 0]).all():
                return x, y
    return None


@functools.lru_cache(maxsize=None)
def var_field(name, W, H):
    """(n,) float32 variances for rtg_svgf*: seeded in [0, 0.5) with a NaN, a
    +inf and a -0 planted on hit pixels (none in a frame with fewer than 12)."""
    rng = np.random.default_rng(8100 + W * 64 + H)
    v = rng.uniform(0.0, 0.5, size=W * H).astype(F)
    real = _real(name, W, H)
    if len(real) >= 12:
        v[real[7]] = np.nan
        v[real[len(real) // 3]] = np.inf
        v[real[-4]] = -0.0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def state(name, W, H, kind):
    """(acc, m2) of a frame for rtg_variance*, (n, C) float32 each, read-only: a
    seeded acc in [0, 2); m2 = acc^2 + seeded noise in [0, 0.5) with a NaN, a
    +inf and a -0 planted on hit pixels and, where the frame has one, a 3 x 3
    block inside a sphere with m2 < acc^2 (the clamp sends it to 0)."""
    C = 3 if kind == "rgb" else 1
    rng = np.random.default_rng(8200 + W * 64 + H + 17 * C)
    acc = rng.uniform(0.0, 2.0, size=(W * H, C)).astype(F)
    m2 = (acc * acc + rng.uniform(0.0, 0.5, size=(W * H, C)).astype(F)).astype(F)
    real = _real(name, W, H)
    if len(real) >= 12:
        m2[real[5], C - 1] = np.nan
        m2[real[len(real) // 2], 0] = np.inf
        m2[real[-2], 0] = -0.0
        acc[real[9], 0] = np.nan
    at = _inner_block(G.guides(name, W, H)["id"].reshape(H, W))
    if at is not None:
        x, y = at
        blk = (slice(y - 1, y + 2), slice(x - 1, x + 2))
        m2.reshape(H, W, C)[blk] = acc.reshape(H, W, C)[blk] ** 2 * F(0.5)
    acc.setflags(write=False)
    m2.setflags(write=False)
    return acc, m2


@functools.lru_cache(maxsize=None)
def len_field(name, W, H, which):
    """(n,) uint16 history lengths of a frame, read-only."""
    h = G.guides(name, W, H)
    real, miss = np.flatnonzero(h["id"] >= 0), np.flatnonzero(h["id"] < 0)
    if which == "seeded":
        ln = np.random.default_rng(8300 + W * 64 + H).integers(0, 9, size=W * H).astype(np.uint16)
        if len(real) >= 12:
            ln[real[-3]] = 65535
        if len(miss):
            ln[miss[len(miss) // 2]] = 3  # a short history on a background pixel: not read
    elif which == "long":
        ln = np.full(W * H, 65535, np.uint16)
        ln[miss] = 0  # background pixels have no history and stage nothing
    elif which == "zero":
        ln = np.zeros(W * H, np.uint16)
    else:
        ln = np.full(W * H, 65535, np.uint16)
        ln[real[len(real) // 2]] = 0
    ln.setflags(write=False)
    return ln


@functools.lru_cache(maxsize=None)
def want_variance(name, W, H, kind, which, st):
    """variance_host's words of a case, read-only."""
    import rtg_amd as R
    acc, m2 = state(name, W, H, kind)
    out = R.variance_host(G.guides(name, W, H), W, H, variance_params(R, name, kind, st), acc, m2,
                          len_field(name, W, H, which), threads=THREADS).view(np.uint32).reshape(-1)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_svgf(name, W, H, kind, st):
    """svgf_host's (value words, variance words) of a case, read-only."""
    import rtg_amd as R
    v, var = R.svgf_host(G.guides(name, W, H), W, H, svgf_params(R, name, kind, st),
                         G.signal(name, W, H, kind), var_field(name, W, H), threads=THREADS)
    res = (v.view(np.uint32).reshape(-1), var.view(np.uint32).reshape(-1))
    for a in res:
        a.setflags(write=False)
    return res


# ---- the host chain: ao -> accumulate (M2) -> variance -> svgf ----

CHAIN = dict(name="c5", W=67, H=35, K=7, frames=4, max_history=3, min_history=4, passes=3,
             sigma=4.0, eps=1e-6)


def chain_path(name, frames):
    eye, target = (np.array(v, np.float64) for v in G.POSES[name])
    d = np.array((0.3, 0.1, 0.0))
    return [(tuple(eye + k * d), tuple(target + k * d)) for k in range(frames)]


def chain_params(R):
    import aogen
    c = CHAIN
    flags = SAME_ID | NORMAL | PLANE
    scale = G.plane_scale(c["name"], None)
    return dict(
        cams=[R.camera_look_at(*p) for p in chain_path(c["name"], c["frames"])],
        aos=[R.ao_params(c["K"], aogen.radius(c["name"]), aogen.BIAS, (aogen.SEED + k) & 0xFFFFFFFF,
                         R.AO_JITTER) for k in range(c["frames"])],
        accum=R.accumulate_params(R.FILTER_COUNT, flags, scale, 3, c["max_history"]),
        variance=R.variance_params(R.FILTER_GRAY, flags, scale, 3, c["min_history"]),
        svgf=R.svgf_params(c["passes"], R.FILTER_GRAY, flags | LUMA, scale, 3, c["sigma"], c["eps"]))


@functools.lru_cache(maxsize=None)
def chain_host():
    """The host chain's (hits, acc, len, m2, var, dst, dstVar) of the last frame."""
    import aogen
    import rtg_amd as R
    c, p = CHAIN, chain_params(R)
    W, H = c["W"], c["H"]
    sph, table = aogen.scene(c["name"]), aogen.dirs(8)
    prev = None
    for cam, ap in zip(p["cams"], p["aos"]):
        h = R.intersect_host(sph, R.camera_rays_host(cam, W, H, alias_factor=1.0), walk=0,
                             threads=THREADS)
        counts = R.ao_host(sph, h, table, ap, walk=0, threads=THREADS)
        acc, ln, m2 = R.accumulate_host(h, W, H, p["accum"], counts, prev, zoom=-4.0, m2=True,
                                        threads=THREADS)
        prev = (cam, h, acc, ln, m2)
    _, h, acc, ln, m2 = prev
    var = R.variance_host(h, W, H, p["variance"], acc, m2, ln, threads=THREADS)
    dst, dvar = R.svgf_host(h, W, H, p["svgf"], acc, var, threads=THREADS)
    return h, acc, ln, m2, var, dst, dvar


# ---- both calls restated in numpy float32, one operation a line ----

HW = G.HW
KW = np.array([1 / 4, 1 / 2, 1 / 4], F)
_dot = G._dot
canon = G.canon


def _lum(v):
    """lum(v) of (..., C) float32."""
    if v.shape[-1] == 1:
        return v[..., 0]
    rg = F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1]
    return rg + F(0.0722) * v[..., 2]


def _weight(hw, flags, normal_log2, scale, P, N, Pq, Nq):
    """rtg_filter*'s weight of a tap over the frame, from `hw`."""
    zero, one = F(0), F(1)
    w = np.full(N.shape[:2], hw, F)
    if flags & NORMAL:
        c = _dot(N, Nq)
        c = np.where(c > zero, c, zero)
        for _ in range(normal_log2):
            c = c * c
        w = w * c
    if flags & PLANE:
        e = Pq - P
        d = np.abs(_dot(N, e))
        z = d * F(scale)
        z = one - z
        z = np.where(z > zero, z, zero)
        w = w * z
    return w


def _tap(H, W, dy, dx, s):
    """(inside the frame, clipped row, clipped column) of tap (dx s, dy s)."""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    yq, xq = y + dy * s, x + dx * s
    keep = (yq >= 0) & (yq < H) & (xq >= 0) & (xq < W)
    return keep, np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)


def _guides(h, W, H):
    return (h["id"].reshape(H, W), h["point"].astype(F).reshape(H, W, 3),
            h["normal"].astype(F).reshape(H, W, 3))


def restate_variance(h, W, H, st, scale, acc, m2, ln, facts=None):
    """The canonical words of rtg_variance*; vectorised over pixels, a loop over
    the 49 taps.  facts["spatial"]: the pixels that took the spatial branch."""
    flags, normal_log2, _, min_history = st
    ids, P, N = _guides(h, W, H)
    A = np.asarray(acc, F).reshape(H, W, -1)
    M = np.asarray(m2, F).reshape(H, W, -1)
    C = A.shape[-1]
    L = np.asarray(ln).astype(np.int64).reshape(H, W)
    zero = F(0)
    short = (ids >= 0) & (L < min_history)
    if facts is not None:
        facts["spatial"] = short.reshape(-1)
    with np.errstate(all="ignore"):
        m, e = A, M
        if short.any():
            s1 = np.zeros((H, W, C), F)
            s2 = np.zeros((H, W, C), F)
            sw = np.zeros((H, W), F)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    keep, yc, xc = _tap(H, W, dy, dx, 1)
                    idq, Aq, Mq = ids[yc, xc], A[yc, xc], M[yc, xc]
                    keep &= idq >= 0
                    if flags & SAME_ID:
                        keep &= idq == ids
                    if flags & SKIP:
                        keep &= np.isfinite(Aq).all(-1) & np.isfinite(Mq).all(-1)
                    w = _weight(F(1), flags, normal_log2, scale, P, N, P[yc, xc], N[yc, xc])
                    keep &= w > zero
                    for q in range(C):
                        term = w * Aq[..., q]
                        s1[..., q] = np.where(keep, s1[..., q] + term, s1[..., q])
                        term = w * Mq[..., q]
                        s2[..., q] = np.where(keep, s2[..., q] + term, s2[..., q])
                    sw = np.where(keep, sw + w, sw)
            got = (short & (sw > zero))[..., None]
            m = np.where(got, s1 / sw[..., None], A)
            e = np.where(got, s2 / sw[..., None], M)
        mm = m * m
        d = e - mm
        d = np.where(d > zero, d, zero)
        var = _lum(d)
    assert var.dtype == F and d.dtype == F
    return canon(np.where(ids < 0, zero, var)).reshape(-1)


def restate_svgf_pass(ids, P, N, img, var, s, st, scale, facts=None):
    """One pass of step s over img (H, W, C) and var (H, W); a loop over the 9
    and the 25 taps.  facts["z1"] stays True while every accepted tap has
    z == 1.f."""
    _, flags, normal_log2, _, luma, sigma, eps = st
    H, W, C = img.shape
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        if luma:
            gs = np.zeros((H, W), F)
            gw = np.zeros((H, W), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    keep, yc, xc = _tap(H, W, dy, dx, 1)
                    idq, vq = ids[yc, xc], var[yc, xc]
                    keep &= idq >= 0
                    if flags & SAME_ID:
                        keep &= idq == ids
                    if flags & SKIP:
                        keep &= np.isfinite(vq)
                    kw = KW[dy + 1] * KW[dx + 1]
                    term = kw * vq
                    gs = np.where(keep, gs + term, gs)
                    gw = np.where(keep, gw + kw, gw)
            g = np.where(gw > zero, gs / gw, var)
            den = np.sqrt(g)
            den = F(sigma) * den
            den = den + F(eps)
            ls = one / den
            lp = _lum(img)
            assert ls.dtype == F and lp.dtype == F and gw.dtype == F
        acc = np.zeros((H, W, C), F)
        sv = np.zeros((H, W), F)
        sw = np.zeros((H, W), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                keep, yc, xc = _tap(H, W, dy, dx, s)
                idq, vq, varq = ids[yc, xc], img[yc, xc], var[yc, xc]
                keep &= idq >= 0
                if flags & SAME_ID:
                    keep &= idq == ids
                if flags & SKIP:
                    keep &= np.isfinite(vq).all(-1) & np.isfinite(varq)
                w = _weight(HW[dy + 2] * HW[dx + 2], flags, normal_log2, scale, P, N, P[yc, xc],
                            N[yc, xc])
                if luma:
                    l = _lum(vq) - lp  # noqa: E741
                    l = np.abs(l)  # noqa: E741
                    z = l * ls
                    z = one - z
                    z = np.where(z > zero, z, zero)
                    w = w * z
                keep &= w > zero
                if luma and facts is not None:
                    facts["z1"] = facts.get("z1", True) and bool((z[keep & (ids >= 0)] == one).all())
                for q in range(C):
                    term = w * vq[..., q]
                    acc[..., q] = np.where(keep, acc[..., q] + term, acc[..., q])
                ww = w * w
                term = ww * varq
                sv = np.where(keep, sv + term, sv)
                sw = np.where(keep, sw + w, sw)
        got = (sw > zero) & (ids >= 0)
        out = np.where(got[..., None], acc / sw[..., None], img)
        sw2 = sw * sw
        vout = np.where(got, sv / sw2, var)
    assert out.dtype == F and vout.dtype == F and acc.dtype == F and sv.dtype == F
    return out, vout


def restate_svgf(h, W, H, st, scale, src, var, facts=None):
    """The canonical (value words, variance words) of rtg_svgf*."""
    ids, P, N = _guides(h, W, H)
    img = np.asarray(src).astype(F).reshape(H, W, -1)
    v = np.asarray(var).astype(F).reshape(H, W)
    for i in range(st[0]):
        img, v = restate_svgf_pass(ids, P, N, img, v, 1 << i, st, scale, facts)
    return canon(img).reshape(-1), canon(v).reshape(-1)
