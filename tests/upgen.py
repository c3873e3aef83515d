"""Inputs and references shared by the upsampling tests (test_upsample_host.py,
test_gpu_upsample.py): full and low records of one pose, low signals, the
parameter sets, a numpy float32 restatement of rtg_upsample* (include/rtg.h,
"upsample"), hole list included, and the host loops' answers, computed once
and left unchanged.

Records are intersect_host(walk 0) of camera_rays_host at aa 1 from
POSES[name], at the full size and at the low size: two independent calls, so
the correspondence of the two frames (low (X, Y) is full (f X, f Y)) is a fact
the tests check, not one the inputs assume.  Scenes: `reference` (no BVH) and
c5 (BVH) of raygen / aogen.

POSES, PLANE_MULTIPLE and NORMAL_LOG2 were moved until, with SAME_ID | NORMAL |
PLANE, the 48 x 32 frame at L = 1, 2, 3 meets test_upsample_host.py's
non-vacuity facts (holes exist and are the minority, pixels with 1, 2, 3 and 4
accepted taps occur, each flag changes a word); the measured shares of holes
among the hit pixels (host form, L = 1 / 2 / 3):
    reference  0.003 / 0.024 / 0.079   (788 hit pixels)
    c5         0.017 / 0.083 / 0.273   (1517 hit pixels)
"""
from __future__ import annotations

import functools

import numpy as np

import aogen
import filtergen as G
from filtergen import ALL, NORMAL, PLANE, SAME_ID, SKIP  # noqa: F401
from test_raytrace_host import THREADS

F = np.float32
SCENES = ["reference", "c5"]
# (eye, target) per scene: filtergen's poses moved a fifth of the way to their targets
POSES = {
    "reference": ((-5.4, 0.0, -3.0), (-2.4, 0.0, -8.0)),
    "c5": ((0.0, 0.0, -2.0), (0.0, 0.0, -12.0)),
}
FULL = (48, 32)
LS = (1, 2, 3)
SIGNALS = ["count", "rgb", "gray"]
KINDS = G.KINDS
AO_K = 7
GEOM = SAME_ID | NORMAL | PLANE
# the plane term as a multiple of 1 / (largest radius), and the normal term's power
PLANE_MULTIPLE = {"reference": 16.0, "c5": 4.0}
NORMAL_LOG2 = 3
FILL = 0x5A5A5A5A


def plane_scale(name):
    return float(F(PLANE_MULTIPLE[name] * G.plane_scale(name, None)))


def params(R, name, signal, L, flags, scale=None, normal_log2=NORMAL_LOG2):
    return R.upsample_params(L, KINDS[signal], flags, plane_scale(name) if scale is None else scale,
                             normal_log2)


@functools.lru_cache(maxsize=None)
def records(name, W, H):
    """(H * W,) walk-0 records of the W x H frame from POSES[name], read-only."""
    import rtg_amd as R
    eye, target = POSES[name]
    rays = R.camera_rays_host(R.camera_look_at(eye, target), W, H, alias_factor=1.0)
    h = R.intersect_host(aogen.scene(name), rays, walk=0, threads=THREADS).reshape(-1)
    h.setflags(write=False)
    return h


def _plant(h):
    """Hand-made records on real points from the second on, as filtergen plants
    them: a NaN normal, a NaN point, a scaled normal, an infinite point, an
    infinite normal and an id >= sphNum."""
    h = h.copy()
    real = np.flatnonzero(h["id"] >= 0)
    if len(real) >= 12:
        h[real[1]]["normal"] = np.nan
        h[real[2]]["point"] = (np.nan, h[real[2]]["point"][1], np.nan)
        h[real[3]]["normal"] = h[real[3]]["normal"] * F(2.5)
        h[real[len(real) // 3]]["point"] = (np.inf, 0.0, -np.inf)
        h[real[len(real) // 2]]["normal"] = (0.0, np.inf, 0.0)
        h[real[-4]]["id"] = 1 << 30
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def frames(name, W, H, L, hostile=False):
    """(full records, low records) of one pose; `hostile`: hand-made records
    planted in both."""
    full, low = records(name, W, H), records(name, W >> L, H >> L)
    return (_plant(full), _plant(low)) if hostile else (full, low)


@functools.lru_cache(maxsize=None)
def low_signal(name, Wl, Hl, kind, hostile=False):
    """The low frame's values of a kind, read-only: (n,) uint16 ao_host counts at
    K = 7, (n, 3) float32 seeded colours, or (n,) float32 t of the records;
    `hostile`: a NaN, a +inf and a -0 planted on hit pixels of the floats."""
    import rtg_amd as R
    h = records(name, Wl, Hl)
    if kind == "count":
        p = R.ao_params(AO_K, aogen.radius(name), aogen.BIAS, aogen.SEED, 1)
        out = R.ao_host(aogen.scene(name), h, aogen.dirs(8), p, walk=0, threads=THREADS)
    elif kind == "gray":
        out = h["t"].astype(F).copy()
    else:
        rng = np.random.default_rng(7100 + Wl * 64 + Hl)
        out = rng.uniform(0.0, 2.0, size=(Wl * Hl, 3)).astype(F)
    real = np.flatnonzero(h["id"] >= 0)
    if hostile and kind != "count" and len(real) >= 6:
        flat = out.reshape(Wl * Hl, -1)
        flat[real[len(real) // 4], -1] = np.nan
        flat[real[len(real) // 2], 0] = np.inf
        flat[real[-2], 0] = -0.0
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(name, W, H, L, signal, flags, hostile=False):
    """upsample_host's (dst words, the whole list, count) of a case, read-only."""
    import rtg_amd as R
    full, low = frames(name, W, H, L, hostile)
    out, lst, cnt = R.upsample_host(full, W, H, params(R, name, signal, L, flags), low, W >> L,
                                    H >> L, low_signal(name, W >> L, H >> L, signal, hostile),
                                    holes=W * H, threads=THREADS)
    res = (out.view(np.uint32).reshape(-1), lst[:cnt].copy(), cnt)
    for a in res[:2]:
        a.setflags(write=False)
    return res


# ---- rtg_upsample* restated in numpy float32, one operation a line ----

_dot = G._dot


def restate(h, lh, W, H, L, flags, normal_log2, scale, low_src, taps=False):
    """The canonical dst words and the hole list (ascending pixel indices) of
    rtg_upsample* over HIT_DTYPE records; vectorised over pixels, a loop over
    the 4 taps.  `taps`: also the number of accepted taps per pixel."""
    f = 1 << L
    Wl, Hl = W >> L, H >> L
    ids = h["id"].reshape(H, W)
    P = h["point"].astype(F).reshape(H, W, 3)
    N = h["normal"].astype(F).reshape(H, W, 3)
    lid = lh["id"].reshape(Hl, Wl)
    lP = lh["point"].astype(F).reshape(Hl, Wl, 3)
    lN = lh["normal"].astype(F).reshape(Hl, Wl, 3)
    img = np.asarray(low_src).astype(F).reshape(Hl, Wl, -1)
    C = img.shape[-1]
    scale, zero, one = F(scale), F(0), F(1)
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    inv = one / F(f)
    x0 = x >> L
    y0 = y >> L
    tx = (x & (f - 1)).astype(F) * inv
    ty = (y & (f - 1)).astype(F) * inv
    acc = np.zeros((H, W, C), F)
    sw = np.zeros((H, W), F)
    count = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for dy in (0, 1):
            for dx in (0, 1):
                yq, xq = y0 + dy, x0 + dx
                keep = (yq < Hl) & (xq < Wl)
                yc, xc = np.clip(yq, 0, Hl - 1), np.clip(xq, 0, Wl - 1)
                wx = tx if dx else one - tx
                wy = ty if dy else one - ty
                w = wy * wx
                idq, Pq, Nq, vq = lid[yc, xc], lP[yc, xc], lN[yc, xc], img[yc, xc]
                keep &= idq >= 0
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
                sw = np.where(keep, sw + w, sw)
                count += keep
        found = sw > zero
        out = np.where(found[..., None], acc / sw[..., None], zero)
    assert out.dtype == F and w.dtype == F and acc.dtype == F and tx.dtype == F
    hit = ids >= 0
    out = np.where(hit[..., None], out, zero)
    holes = np.flatnonzero((hit & ~found).reshape(-1)).astype(np.uint32)
    res = (canon(out).reshape(-1), holes)
    return res + (np.where(hit, count, -1),) if taps else res


def canon(a):
    """uint32 words, NaN as 0xFFC00000."""
    return aogen.canon(a)
