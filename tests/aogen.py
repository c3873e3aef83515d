"""Inputs and references shared by the ambient-occlusion tests (test_ao_host.py,
test_gpu_ao.py): direction tables, hit records, the parameter sets, the scenes,
a numpy float32 restatement of the probe segment (include/rtg.h, "ambient
occlusion") and the plain-loop answers, computed once and left unchanged.

Direction tables are the tests' own, not rtg_ao_directions': seeded unit
vectors over the WHOLE sphere (below the horizon too) and, from 7 entries on,
one zero vector, one NaN vector and one of length 1e3.  Hit records come from
the plain loops (intersect_host walk 0) over surface, primary and inside rays
interleaved, so that every wave holds hits and misses side by side, plus four
hand-made records near the front.
"""
from __future__ import annotations

import functools

import numpy as np

import hostile
import raygen
from test_raytrace_host import THREADS

F = np.float32
N_POINTS = 200
SIZES = (1, 63, 64, 65, 200)  # points: one lane, a wave less one, a wave, one more, a tail
PROBES = ((1, 1), (7, 7), (7, 8), (64, 97))  # (K, nDirs)
SEED = 0xFFFFFF9C  # seed + i wraps past 2^32 at i = 100
SETS = [(k, nd, j) for k, nd in PROBES for j in (0, 1)]  # (K, nDirs, flags)
SET_IDS = [f"K{k}-of-{nd}-{'jitter' if j else 'plain'}" for k, nd, j in SETS]
BIAS = 1e-3
# The scenes of the walk-1 list, one per path the tables select: no spheres,
# the 64-sphere query (reference, 12, 40), the BVH (65, 150, c5) and the flat
# query above 64 spheres (a hostile.NO_BVH mutation at 150).
SCENES = ["none", "reference", 12, 40, "base65", "base150", "c5", "cnan150"]
PATHS = {"none": "64", "reference": "64", 12: "64", 40: "64", "base65": "bvh", "base150": "bvh",
         "c5": "bvh", "cnan150": "flat"}
# The probe length as a multiple of the largest |radius| of the scene (the
# non-vacuity condition of the two test files; the measured walk-0 share of
# blocked probes at (K, nDirs) = (64, 97) without jitter is noted per scene).
RADIUS_MULTIPLE = {
    "reference": 2.5,  # 0.546
    12: 2.5,           # 0.539
    40: 2.5,           # 0.654
    "base65": 2.5,     # 0.538
    "base150": 2.5,    # 0.573
    "c5": 2.5,         # 0.868
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "none":
        return raygen.scene("reference")[:0].copy()
    if name == "base65":
        return hostile.base(65)[0]
    if name == "base150":
        return hostile.base(150)[0]
    if name == "cnan150":
        return hostile.mutated(150, "cnan")[0]
    return raygen.scene(name)


def scene(name):
    return _scene(name).copy()


def ray_scene(name):
    """The scene whose geometry lays out the rays (finite, not empty)."""
    return _scene({"none": "reference", "cnan150": "base150"}.get(name, name))


def radius(name):
    r = np.abs(ray_scene(name)["radius"].astype(np.float64))
    return float(F(RADIUS_MULTIPLE.get(name, 2.5) * r.max()))


@functools.lru_cache(maxsize=None)
def dirs(n_dirs):
    rng = np.random.default_rng(500 + n_dirs)
    d = raygen._unit(rng, n_dirs).astype(F)
    if n_dirs >= 7:
        d[2] = 0
        d[4] = (np.nan, 0.5, np.nan)
        d[5] *= F(1e3)
        assert (d[:, 2] < 0).any() and (d[:, 2] > 0).any()
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def hits(name):
    """N_POINTS hit records against scene `name`, read-only."""
    import rtg_amd as R
    geo = ray_scene(name)
    rng = np.random.default_rng(900 + len(geo))
    k = N_POINTS // 4
    rays = np.concatenate([raygen.interleave(raygen.surface(rng, geo, k), raygen.primary(12, 9)[:k]),
                           raygen.interleave(raygen.surface(rng, geo, k), raygen.inside(rng, geo, k))])
    h = R.intersect_host(_scene(name) if name != "none" else geo, rays, walk=0, threads=THREADS)
    assert len(h) == N_POINTS
    hit = np.flatnonzero(h["id"] >= 0)
    assert 0.2 * N_POINTS <= len(hit) <= 0.9 * N_POINTS, len(hit)
    assert (h["id"][:64] >= 0).any() and (h["id"][:64] < 0).any()
    # hand-made records, from the second on (the one-point batch keeps a real one)
    h[1]["id"] = -1
    h[1]["point"] = np.nan
    h[1]["normal"] = np.nan
    for at, nrm in ((2, (0.0, 0.0, -1.0)), (3, (0.6, -0.8, -0.0)), (4, (0.5, 2.0, -0.25))):
        h[at] = h[hit[at]]
        h[at]["normal"] = nrm
    assert np.signbit(h[3]["normal"][2])
    h.setflags(write=False)
    return h


def hostile_hits(n, name):
    """N_POINTS of the plain-loop hits of hostile.batches(n) against (n, name)."""
    from test_hostile_host import walk0
    h = walk0(n, name)[0]
    return np.ascontiguousarray(h[::len(h) // N_POINTS][:N_POINTS])


def params(R, name, k, flags, radius_=None):
    return R.ao_params(k, radius(name) if radius_ is None else radius_, BIAS, SEED, flags)


@functools.lru_cache(maxsize=None)
def want(name, k, n_dirs, flags):
    """The plain-loop counts (ao_host walk 0) of hits(name), read-only."""
    import rtg_amd as R
    out = R.ao_host(_scene(name), hits(name), dirs(n_dirs), params(R, name, k, flags), walk=0,
                    threads=THREADS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_segments(name, k, n_dirs, flags):
    import rtg_amd as R
    out = R.ao_segments_host(hits(name), dirs(n_dirs), params(R, name, k, flags), threads=THREADS)
    out.setflags(write=False)
    return out


def blocked_share(h, counts, k):
    """The share of blocked probes over the records with a point."""
    real = h["id"] >= 0
    return 1.0 - float(counts[real].astype(np.float64).sum()) / (k * int(real.sum()))


def assert_non_vacuous(name):
    """On the WALK-0 answer only: over the records with id >= 0, the blocked
    share of all probes lies strictly between 25 % and 95 %, for every
    non-hostile scene with a sphere, at (K, nDirs) = (64, 97) without jitter."""
    if name not in RADIUS_MULTIPLE:
        return
    share = blocked_share(hits(name), want(name, 64, 97, 0), 64)
    assert 0.25 < share < 0.95, (name, share)


# ---- the segment arithmetic restated in numpy float32, one operation a line ----

def mix32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def restate_segments(h, table, k, radius_, bias, seed, flags):
    """(n * K, 6) float32 segments of HIT_DTYPE records `h`, point-major."""
    n, n_dirs = len(h), len(table)
    radius_, bias = F(radius_), F(bias)
    i = np.arange(n, dtype=np.uint64)
    s_i = mix32(np.uint64(seed) + i) % np.uint64(n_dirs) if flags & 1 else np.zeros(n, np.uint64)
    j = s_i[:, None] + np.arange(k, dtype=np.uint64)[None, :]
    j = np.where(j >= n_dirs, j - np.uint64(n_dirs), j).astype(np.int64)
    l = table[j]  # (n, K, 3)
    lx, ly, lz = l[..., 0], l[..., 1], l[..., 2]
    P = h["point"].astype(F)
    N = h["normal"].astype(F)
    Nx, Ny, Nz = N[:, 0], N[:, 1], N[:, 2]
    one = F(1)
    with np.errstate(all="ignore"):
        s = np.copysign(one, Nz)
        den = s + Nz
        a = -one / den
        nxy = Nx * Ny
        b = nxy * a
        nxx = Nx * Nx
        nxxa = nxx * a
        snxxa = s * nxxa
        t1x = one + snxxa
        t1y = s * b
        snx = s * Nx
        t1z = -snx
        nyy = Ny * Ny
        t2x = b
        nyya = nyy * a
        t2y = s + nyya
        t2z = -Ny
        out = np.zeros((n, k, 6), F)
        for q, (t1, t2, nq) in enumerate(((t1x, t2x, Nx), (t1y, t2y, Ny), (t1z, t2z, Nz))):
            u = lx * t1[:, None]
            v = ly * t2[:, None]
            uv = u + v
            ln = lz * nq[:, None]
            w = uv + ln
            off = bias * nq
            aq = P[:, q] + off
            step = radius_ * w
            out[..., q] = aq[:, None]
            out[..., 3 + q] = aq[:, None] + step
    assert out.dtype == F
    out[h["id"] < 0] = 0
    return out.reshape(n * k, 6)


def canon(a):
    """uint32 words, NaN as 0xFFC00000."""
    a = np.ascontiguousarray(a, F)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0xFFC00000
    return b
