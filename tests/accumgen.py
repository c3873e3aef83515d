"""Inputs and references shared by the accumulation tests
(test_accumulate_host.py, test_gpu_accumulate.py): current and previous
records, signals, previous state, the parameter sets, a numpy float32
restatement of rtg_camera_project* and rtg_accumulate* (include/rtg.h) and the
host loops' answers, computed once and left unchanged.

The current frame is filtergen's: its guides (pose A = filtergen.POSES[name],
windows of the 67 x 35 frame, hand-made records planted) and its signals.
The previous frame is the same window of intersect_host(walk 0) from one of
PREV_KINDS' poses, with the same hand-made records planted, a seeded prevAcc
and prevM2 with non-finite words planted, and a seeded prevLen.
"""
from __future__ import annotations

import functools

import numpy as np

import aogen
import filtergen as G
from filtergen import ALL, FRAMES, FULL, NORMAL, PLANE, SAME_ID, SCENES, SKIP  # noqa: F401
from test_raytrace_host import THREADS

F = np.float32
ZOOM = -4.0
SIGNALS = G.SIGNALS
INF, NAN = float("inf"), float("nan")

PREV_KINDS = ["same", "pan", "roll", "dolly", "away", "nan"]
# The pan per scene, (d eye, d target), moved until facts() holds
# (test_accumulate_host.py): the image shifts by a fraction of a pixel to a
# few pixels, depending on depth.
PANS = {
    "reference": ((0.35, 0.1, 0.0), (0.2, 0.05, 0.0)),
    12: ((0.5, 0.15, 0.0), (0.3, 0.1, 0.0)),
    "c5": ((0.3, 0.1, 0.0), (0.2, 0.05, 0.0)),
}


def pose_args(name, kind):
    """(eye, target, up) of a previous pose."""
    eye, target = (np.array(v, np.float64) for v in G.POSES[name])
    up = (0.0, 1.0, 0.0)
    if kind == "pan":
        de, dt = PANS[name]
        eye, target = eye + de, target + dt
    elif kind == "roll":
        up = (0.2, 1.0, 0.0)
    elif kind == "dolly":
        eye = eye + 0.08 * (target - eye)
    elif kind == "away":
        target = eye - (target - eye)
    elif kind == "nan":
        eye = eye.copy()
        eye[0] = np.nan
    return tuple(eye), tuple(target), up


@functools.lru_cache(maxsize=None)
def pose(name, kind):
    import rtg_amd as R
    c = R.camera_look_at(*pose_args(name, kind))
    c.setflags(write=False)
    return c


# (flags, normalLog2, planeScale, maxHistory, with M2, reset frame); planeScale
# None: filtergen's 1 / (largest radius).  Every single flag, all and none,
# normalLog2 0, 3 and 8, planeScale 0, finite, +inf and NaN, maxHistory 1, 3 and
# 65535, with and without M2, the reset frame.
SETS = [
    (ALL, 3, None, 3, True, False), (ALL, 3, None, 65535, False, False),
    (0, 0, 0.0, 65535, True, False), (SAME_ID, 0, 0.0, 3, False, False),
    (SKIP, 0, 0.0, 1, True, False),
    (NORMAL, 0, None, 3, False, False), (NORMAL, 3, None, 65535, True, False),
    (NORMAL, 8, None, 3, False, False),
    (PLANE, 0, None, 3, True, False), (PLANE, 0, 0.0, 3, False, False),
    (PLANE, 0, INF, 65535, False, False), (PLANE, 0, NAN, 3, True, False),
    (ALL, 8, INF, 1, False, False),
    (ALL, 3, None, 3, True, True), (0, 0, 0.0, 3, False, True),
]
SET_IDS = [f"f{f}-n{n}-s{'r' if s is None else s}-h{h}-m{int(m)}-r{int(r)}"
           for f, n, s, h, m, r in SETS]


def cases():
    """(previous pose kind, set) pairs: a reset frame has no previous pose."""
    return [(k, st) for st in SETS for k in (PREV_KINDS if not st[5] else PREV_KINDS[:1])]


def params(R, name, signal, st):
    f, n, s, h, _, _ = st
    return R.accumulate_params(G.KINDS[signal], f, G.plane_scale(name, s), n, h)


@functools.lru_cache(maxsize=None)
def raw_prev(name, kind):
    """The 67 x 35 walk-0 records from a previous pose, nothing planted."""
    import rtg_amd as R
    W, H = FULL
    rays = R.camera_rays_host(pose(name, kind), W, H, alias_factor=1.0)
    h = R.intersect_host(aogen.scene(name), rays, walk=0, threads=THREADS).reshape(H, W)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def prev_hits(name, W, H, kind):
    """(H * W,) previous records of a frame: the current frame's window, the
    hand-made records of filtergen.guides planted the same way, and where the
    frame has room a 3 x 3 block of changed ids (every bilinear tap of some
    pixel)."""
    x0, y0 = G.window(name, W, H)
    h = raw_prev(name, kind)[y0:y0 + H, x0:x0 + W].copy()
    if (W, H) == FULL:
        x, y = G.island_at(name)
        h[y, x]["id"] = 1 << 30
        h[y, x]["point"] = (0.5, -0.25, -3.0)
        h[y, x]["normal"] = (0.0, 0.6, 0.8)
    at, other = _inner_block(h["id"], 1, 1), _inner_block(h["id"], H // 2, W // 2)
    if at and other and max(abs(at[0] - other[0]), abs(at[1] - other[1])) > 3:
        x, y = at  # a surface whose id changed between the frames
        h["id"][y - 1:y + 2, x - 1:x + 2] += 1000
    h = h.reshape(-1)
    real = np.flatnonzero(h["id"] >= 0)
    if len(real) >= 8:
        h[real[1]]["normal"] = np.nan
        h[real[2]]["point"] = (np.nan, h[real[2]]["point"][1], np.nan)
        h[real[3]]["normal"] = h[real[3]]["normal"] * F(2.5)
    h.setflags(write=False)
    return h


def _inner_block(ids, y0, x0):
    """(x, y) of the centre of the first 3 x 3 block of one id >= 0 from row
    y0 and column x0 on, or None."""
    H, W = ids.shape
    for y in range(max(y0, 1), H - 1):
        for x in range(max(x0, 1), W - 1):
            b = ids[y - 1:y + 2, x - 1:x + 2]
            if b[0, 0] >= 0 and (b == b[0, 0]).all():
                return x, y
    return None


@functools.lru_cache(maxsize=None)
def prev_state(name, W, H, kind, C, max_history):
    """(prevAcc (n, C), prevLen (n,), prevM2 (n, C)) of a previous frame,
    read-only.  prevAcc: seeded in [0, 2) with a NaN, a +inf and a -0 on hit
    pixels and, where the frame has one, a 3 x 3 block of NaN inside a sphere
    (every bilinear tap of some pixel).  prevLen: seeded in 0 .. maxHistory,
    zeros on every 7th hit pixel, a nonzero on a background pixel, 65535 on a
    hit pixel."""
    h = prev_hits(name, W, H, kind)
    n = W * H
    rng = np.random.default_rng(9000 + W * 64 + H + 17 * C + PREV_KINDS.index(kind))
    acc = rng.uniform(0.0, 2.0, size=(n, C)).astype(F)
    m2 = rng.uniform(0.0, 4.0, size=(n, C)).astype(F)
    ln = rng.integers(0, max_history + 1, size=n).astype(np.uint16)
    real, miss = np.flatnonzero(h["id"] >= 0), np.flatnonzero(h["id"] < 0)
    ln[real[::7]] = 0
    if len(miss):
        ln[miss[len(miss) // 2]] = 5
    if len(real) >= 12:
        acc[real[5], C - 1] = np.nan
        acc[real[len(real) // 2], 0] = np.inf
        acc[real[-2], 0] = -0.0
        m2[real[6], 0] = np.nan
        ln[real[-3]] = 65535
    at = _inner_block(h["id"].reshape(H, W), H // 2, W // 2)
    if at is not None:
        x, y = at
        acc.reshape(H, W, C)[y - 1:y + 2, x - 1:x + 2] = np.nan
    for a in (acc, ln, m2):
        a.setflags(write=False)
    return acc, ln, m2


def prev(name, W, H, kind, signal, st):
    """accumulate_host's `prev` of a case, or None on a reset frame."""
    if st[5]:
        return None
    C = 3 if signal == "rgb" else 1
    acc, ln, m2 = prev_state(name, W, H, kind, C, st[3])
    return (pose(name, kind), prev_hits(name, W, H, kind), acc, ln, m2 if st[4] else None)


@functools.lru_cache(maxsize=None)
def want(name, W, H, signal, kind, st):
    """accumulate_host's (acc words, len, m2 words or None) of a case, read-only."""
    import rtg_amd as R
    out = R.accumulate_host(G.guides(name, W, H), W, H, params(R, name, signal, st),
                            G.signal(name, W, H, signal), prev(name, W, H, kind, signal, st),
                            zoom=ZOOM, m2=st[4], threads=THREADS)
    res = (out[0].view(np.uint32).reshape(-1), out[1].reshape(-1),
           out[2].view(np.uint32).reshape(-1) if st[4] else None)
    for a in res:
        if a is not None:
            a.setflags(write=False)
    return res


def facts(name, kind):
    """Of the 67 x 35 frame against a previous pose with every prevLen >= 1:
    (hit pixels, those that find history under all flags, and per single flag
    the pixels that find history without any flag but not with it)."""
    import rtg_amd as R
    W, H = FULL
    h, src = G.guides(name, W, H), G.signal(name, W, H, "rgb")
    acc, _, _ = prev_state(name, W, H, kind, 3, 3)
    ones = np.ones(W * H, np.uint16)
    pv = (pose(name, kind), prev_hits(name, W, H, kind), acc, ones)

    def found(flags):
        p = R.accumulate_params(0, flags, G.plane_scale(name, None), 3, 3)
        ln = R.accumulate_host(h, W, H, p, src, pv, zoom=ZOOM)[1].reshape(-1)
        # (prevLen 1: a found pixel ends at 2, or stays at 1 when its own value is skipped)
        fin = np.isfinite(src).all(-1) | (flags & SKIP == 0)
        return np.where(fin, ln == 2, ln == 1) & (h["id"] >= 0)

    free = found(0)
    return (int((h["id"] >= 0).sum()), int(found(ALL).sum()),
            {f: int((free & ~found(f)).sum()) for f in (SAME_ID, NORMAL, PLANE, SKIP)})


# ---- both calls restated in numpy float32, one operation a line ----

_dot = G._dot


def restate_project(cam, W, H, zoom, P):
    """(fx, fy, k) of points P (..., 3) float32 under a CAMERA_DTYPE pose."""
    c = np.asarray(cam).reshape(-1)[0]
    eye, right, up, back = (np.asarray(c[k], F) for k in ("eye", "right", "up", "back"))
    with np.errstate(all="ignore"):
        e = P.astype(F) - eye
        a = _dot(e, right)
        b = _dot(e, up)
        d = _dot(e, back)
        k = F(zoom) / d
        rx = a * k
        ry = b * k
        kx = F(W) * F(0.046875)
        ky = F(H) / F(12)
        half_w = F(W) * F(0.5)
        half_h = F(H) * F(0.5)
        fx = rx * kx
        fx = fx + half_w
        fy = ry * ky
        fy = half_h - fy
    assert fx.dtype == F and fy.dtype == F and k.dtype == F
    return fx, fy, k


def restate(h, W, H, st, scale, src, pv, zoom=ZOOM):
    """The canonical (acc words, len, m2 words) of rtg_accumulate* over
    HIT_DTYPE records `h`; vectorised over pixels, a loop over the 4 taps."""
    flags, normal_log2, _, max_history, _, _ = st
    ids = h["id"].reshape(H, W)
    P = h["point"].astype(F).reshape(H, W, 3)
    N = h["normal"].astype(F).reshape(H, W, 3)
    cur = np.asarray(src).astype(F).reshape(H, W, -1)
    C = cur.shape[-1]
    scale, zero, one = F(scale), F(0), F(1)
    with np.errstate(all="ignore"):
        cur2 = cur * cur
        acc = np.zeros((H, W, C), F)
        s2 = np.zeros((H, W, C), F)
        sw = np.zeros((H, W), F)
        nmin = np.full((H, W), 65535, np.int64)
        if pv is not None:
            cam, ph, pacc, plen, pm2 = pv
            pid = ph["id"].reshape(H, W)
            pP = ph["point"].astype(F).reshape(H, W, 3)
            pN = ph["normal"].astype(F).reshape(H, W, 3)
            pacc = np.asarray(pacc, F).reshape(H, W, C)
            pm2 = pacc if pm2 is None else np.asarray(pm2, F).reshape(H, W, C)
            plen = np.asarray(plen).astype(np.int64).reshape(H, W)
            fx, fy, k = restate_project(cam, W, H, zoom, P)
            ok = (k > zero) & (fx > -one) & (fx < F(W)) & (fy > -one) & (fy < F(H))
            xf, yf = np.floor(fx), np.floor(fy)
            tx = fx - xf
            ty = fy - yf
            x0 = np.where(ok, xf, zero).astype(np.int64)
            y0 = np.where(ok, yf, zero).astype(np.int64)
            for dy in (0, 1):
                for dx in (0, 1):
                    yq, xq = y0 + dy, x0 + dx
                    keep = ok & (yq >= 0) & (yq < H) & (xq >= 0) & (xq < W)
                    yc, xc = np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)
                    wx = tx if dx else one - tx
                    wy = ty if dy else one - ty
                    w = wy * wx
                    idq, Pq, Nq, vq = pid[yc, xc], pP[yc, xc], pN[yc, xc], pacc[yc, xc]
                    keep &= idq >= 0
                    keep &= plen[yc, xc] != 0
                    if flags & SAME_ID:
                        keep &= idq == ids
                    if flags & SKIP:
                        keep &= np.isfinite(vq).all(-1)
                    if flags & NORMAL:
                        c = _dot(N, Nq)
                        c = np.where(c > zero, c, zero)
                        for _ in range(normal_log2):
                            c = c * c
                        w = w * c
                    if flags & PLANE:
                        e = Pq - P
                        d = np.abs(_dot(N, e))
                        z = d * scale
                        z = one - z
                        z = np.where(z > zero, z, zero)
                        w = w * z
                    keep &= w > zero
                    for q in range(C):
                        term = w * vq[..., q]
                        acc[..., q] = np.where(keep, acc[..., q] + term, acc[..., q])
                        term = w * pm2[yc, xc][..., q]
                        s2[..., q] = np.where(keep, s2[..., q] + term, s2[..., q])
                    sw = np.where(keep, sw + w, sw)
                    nmin = np.where(keep, np.minimum(nmin, plen[yc, xc]), nmin)
        found = sw > zero
        hist = acc / sw[..., None]
        hist2 = s2 / sw[..., None]
        cur_ok = np.isfinite(cur).all(-1) if flags & SKIP else np.ones((H, W), bool)
        n = np.minimum(nmin + 1, max_history)
        alpha = one / n.astype(F)
        step = cur - hist
        step = alpha[..., None] * step
        blend = hist + step
        step = cur2 - hist2
        step = alpha[..., None] * step
        blend2 = hist2 + step
    assert blend.dtype == F and blend2.dtype == F and alpha.dtype == F and hist.dtype == F
    both, miss = (found & cur_ok)[..., None], ids < 0
    out = np.where(both, blend, np.where(found[..., None], hist, cur))
    out2 = np.where(both, blend2, np.where(found[..., None], hist2, cur2))
    ln = np.where(found & cur_ok, n, np.where(found, nmin, np.where(cur_ok, 1, 0)))
    out = np.where(miss[..., None], cur, out)
    out2 = np.where(miss[..., None], cur2, out2)
    ln = np.where(miss, 0, ln)
    return canon(out).reshape(-1), ln.astype(np.uint16).reshape(-1), canon(out2).reshape(-1)


def canon(a):
    """uint32 words, NaN as 0xFFC00000."""
    return aogen.canon(a)
