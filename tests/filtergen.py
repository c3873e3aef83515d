"""Inputs and references shared by the filter tests (test_filter_host.py,
test_gpu_filter.py): guide records, signals, the parameter sets, a numpy
float32 restatement of rtg_filter* (include/rtg.h, "filter") and the host
loops' answers, computed once and left unchanged.

Guides are intersect_host(walk 0) of camera_rays_host at aa 1 from POSES[name]
at 67 x 35, for the scenes `reference`, 12 and c5 of raygen / aogen.  The
smaller frames are windows of that frame's records, anchored so that the
window's first pixel is the frame's first hit next to a miss: a 1 x 1 frame
then holds a real point, and the thin frames cross an edge.  Hand-made records
are planted from the second pixel on, as aogen does: a NaN normal, a NaN
point, a scaled normal and, in the 67 x 35 frame, an island of id >= 0 inside
the background.
"""
from __future__ import annotations

import functools

import numpy as np

import aogen
from test_raytrace_host import THREADS

F = np.float32
SCENES = ["reference", 12, "c5"]
# (eye, target) per scene: moved until guide_facts() holds (test_filter_host.py)
POSES = {
    "reference": ((-6.0, 0.0, -2.0), (-3.0, 0.0, -7.0)),
    12: ((-2.0, 1.0, -14.0), (-2.0, 1.0, -25.0)),
    "c5": ((0.0, 0.0, 0.0), (0.0, 0.0, -10.0)),
}
FULL = (67, 35)
# one pixel; thinner than the kernel; smaller than a step; a partial 32 x 8
# tile in both directions; more than two tiles across
FRAMES = [(1, 1), (5, 1), (1, 7), (8, 8), (33, 17), FULL]
SIGNALS = ["count", "rgb", "gray"]
AO_K = 7

SAME_ID, NORMAL, PLANE, SKIP = 1, 2, 4, 8
ALL = SAME_ID | NORMAL | PLANE | SKIP
INF, NAN = float("inf"), float("nan")
# (passes, flags, normalLog2, planeScale); planeScale None: 1 / (largest radius).
# Passes 1, 2, 5 and 8 (steps beyond every frame, both ping-pong parities),
# every single flag, all and none, normalLog2 0, 3 and 8, planeScale 0, finite,
# +inf and NaN.
SETS = [
    (1, ALL, 3, None), (2, ALL, 3, None), (5, ALL, 3, None), (8, ALL, 3, None),
    (1, 0, 0, 0.0), (5, 0, 0, 0.0),
    (2, SAME_ID, 0, 0.0), (5, SKIP, 0, 0.0),
    (2, NORMAL, 0, None), (2, NORMAL, 3, None), (5, NORMAL, 8, None),
    (2, PLANE, 0, None), (2, PLANE, 0, 0.0), (2, PLANE, 0, INF), (2, PLANE, 0, NAN),
    (5, ALL, 0, INF), (8, ALL, 8, NAN), (8, SAME_ID | PLANE, 0, None),
]
SET_IDS = [f"p{p}-f{f}-n{n}-s{'r' if s is None else s}" for p, f, n, s in SETS]
KINDS = {"rgb": 0, "gray": 1, "count": 2}  # RTG_FILTER_RGB / GRAY / COUNT


def plane_scale(name, s):
    if s is not None:
        return s
    r = np.abs(aogen.ray_scene(name)["radius"].astype(np.float64))
    return float(F(1.0 / r.max()))


def params(R, name, signal, st):
    p, f, n, s = st
    return R.filter_params(p, KINDS[signal], f, plane_scale(name, s), n)


@functools.lru_cache(maxsize=None)
def raw_guides(name):
    """The 67 x 35 frame's walk-0 records, nothing planted: (35, 67) HIT_DTYPE."""
    import rtg_amd as R
    W, H = FULL
    eye, target = POSES[name]
    rays = R.camera_rays_host(R.camera_look_at(eye, target), W, H, alias_factor=1.0)
    h = R.intersect_host(aogen.scene(name), rays, walk=0, threads=THREADS).reshape(H, W)
    h.setflags(write=False)
    return h


def guide_facts(name):
    """(different ids >= 0, share of hits, share of misses, pixels with a
    4-neighbour of another id) of the raw 67 x 35 records."""
    ids = raw_guides(name)["id"]
    other = np.zeros(ids.shape, bool)
    other[:, 1:] |= ids[:, 1:] != ids[:, :-1]
    other[:, :-1] |= ids[:, :-1] != ids[:, 1:]
    other[1:, :] |= ids[1:, :] != ids[:-1, :]
    other[:-1, :] |= ids[:-1, :] != ids[1:, :]
    return (len(np.unique(ids[ids >= 0])), float((ids >= 0).mean()), float((ids < 0).mean()),
            int(other.sum()))


def _anchor(ids):
    """The first hit pixel with a miss to its left or above it."""
    H, W = ids.shape
    for y in range(1, H):
        for x in range(1, W):
            if ids[y, x] >= 0 and (ids[y, x - 1] < 0 or ids[y - 1, x] < 0):
                return x, y
    raise AssertionError("no edge")


@functools.lru_cache(maxsize=None)
def window(name, W, H):
    """(x0, y0) of the W x H window of the 67 x 35 frame."""
    if (W, H) == FULL:
        return 0, 0
    x, y = _anchor(raw_guides(name)["id"])
    return min(x, FULL[0] - W), min(y, FULL[1] - H)


def island_at(name):
    """A background pixel of the 67 x 35 frame whose 8 neighbours are background."""
    ids = raw_guides(name)["id"]
    H, W = ids.shape
    for y in range(H - 2, 0, -1):
        for x in range(W - 2, 0, -1):
            if (ids[y - 1:y + 2, x - 1:x + 2] < 0).all():
                return x, y
    raise AssertionError("no background")


@functools.lru_cache(maxsize=None)
def guides(name, W, H):
    """(H * W,) HIT_DTYPE records of a frame, read-only."""
    x0, y0 = window(name, W, H)
    h = raw_guides(name)[y0:y0 + H, x0:x0 + W].copy()
    if (W, H) == FULL:
        x, y = island_at(name)
        h[y, x]["id"] = 1 << 30  # an id >= sphNum is legal
        h[y, x]["point"] = (0.5, -0.25, -3.0)
        h[y, x]["normal"] = (0.0, 0.6, 0.8)
    h = h.reshape(-1)
    real = np.flatnonzero(h["id"] >= 0)
    if len(real) >= 8:  # hand-made records on real points, the first kept as it is
        h[real[1]]["normal"] = np.nan
        h[real[2]]["point"] = (np.nan, h[real[2]]["point"][1], np.nan)
        h[real[3]]["normal"] = h[real[3]]["normal"] * F(2.5)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def planted(name, W, H):
    """Indices of the three hit pixels of the RGB signal that hold the planted
    NaN, +inf and -0 (none in a frame with fewer than 12 hits)."""
    real = np.flatnonzero(guides(name, W, H)["id"] >= 0)
    return tuple(int(i) for i in real[[5, len(real) // 2, len(real) - 2]]) if len(real) >= 12 else ()


@functools.lru_cache(maxsize=None)
def signal(name, W, H, kind):
    """The frame's source values of a kind, read-only: (n,) uint16 ao_host counts
    at K = 7, (n, 3) float32 seeded colours with a NaN, a +inf and a -0 planted
    on hit pixels, or (n,) float32 t of the records."""
    import rtg_amd as R
    h = guides(name, W, H)
    if kind == "count":
        p = R.ao_params(AO_K, aogen.radius(name), aogen.BIAS, aogen.SEED, 1)
        out = R.ao_host(aogen.scene(name), h, aogen.dirs(8), p, walk=0, threads=THREADS)
    elif kind == "gray":
        out = h["t"].astype(F).copy()
    else:
        rng = np.random.default_rng(7000 + W * 64 + H)
        out = rng.uniform(0.0, 2.0, size=(W * H, 3)).astype(F)
        at = planted(name, W, H)
        if at:
            out[at[0], 1] = np.nan
            out[at[1], 0] = np.inf
            out[at[2], 2] = -0.0
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(name, W, H, kind, st):
    """filter_host's words of a frame, signal and parameter set, read-only."""
    import rtg_amd as R
    out = R.filter_host(guides(name, W, H), W, H, params(R, name, kind, st), signal(name, W, H, kind),
                        threads=THREADS).view(np.uint32).reshape(-1)
    out.setflags(write=False)
    return out


# ---- rtg_filter* restated in numpy float32, one operation a line ----

HW = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)


def _dot(a, b):
    xy = a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]
    return xy + a[..., 2] * b[..., 2]


def restate_pass(ids, P, N, img, s, flags, normal_log2, scale):
    """One pass of step s over img, (H, W, C) float32; vectorised over pixels,
    a loop over the 25 taps."""
    H, W, C = img.shape
    scale, zero, one = F(scale), F(0), F(1)
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    acc = np.zeros((H, W, C), F)
    sw = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                yq, xq = y + dy * s, x + dx * s
                keep = (yq >= 0) & (yq < H) & (xq >= 0) & (xq < W)
                yc, xc = np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)
                idq, Pq, Nq, vq = ids[yc, xc], P[yc, xc], N[yc, xc], img[yc, xc]
                keep &= idq >= 0
                if flags & SAME_ID:
                    keep &= idq == ids
                if flags & SKIP:
                    keep &= np.isfinite(vq).all(-1)
                w = np.full((H, W), HW[dy + 2] * HW[dx + 2], F)
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
                sw = np.where(keep, sw + w, sw)
        out = np.where((sw > zero)[..., None], acc / sw[..., None], img)
    assert out.dtype == F and w.dtype == F and acc.dtype == F
    return np.where((ids < 0)[..., None], img, out)


def restate(h, W, H, st, scale, src):
    """The canonical words of rtg_filter* over HIT_DTYPE records `h`."""
    passes, flags, normal_log2, _ = st
    ids = h["id"].reshape(H, W)
    P = h["point"].astype(F).reshape(H, W, 3)
    N = h["normal"].astype(F).reshape(H, W, 3)
    img = np.asarray(src).astype(F).reshape(H, W, -1)
    for i in range(passes):
        img = restate_pass(ids, P, N, img, 1 << i, flags, normal_log2, scale)
    return canon(img).reshape(-1)


def canon(a):
    """uint32 words, NaN as 0xFFC00000."""
    return aogen.canon(a)
