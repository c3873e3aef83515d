"""Inputs and references shared by the gather tests (test_gather_host.py,
test_gpu_gather.py): the parameter sets, the weight tables, a numpy float32
restatement of the probe ray and of the sum (include/rtg.h, "gather") and the
plain-loop answers, computed once and left unchanged.

Scenes, hit records, direction tables, the size prefixes and the seed are
aogen's (the tables hold a zero, a NaN and a x1000 entry and both signs of z),
the lights mattegen's.  The weights are a seeded float table; from 7 entries on
it holds one 0, one negative, one NaN and one +inf, all of them past entry 15
of the 97-entry table, so that the window of the non-vacuity set (K = 16, no
jitter) has ordinary weights and a jittered window reaches the special ones.
"""
from __future__ import annotations

import functools

import numpy as np

import aogen
import mattegen
from aogen import N_POINTS, PATHS, SCENES, SEED, SIZES  # noqa: F401  (re-exported)
from test_raytrace_host import THREADS

F = np.float32
PROBES = ((1, 1), (7, 8), (16, 97))  # (K, nDirs)
JITTER, SKIP = 1, 2  # RTG_GATHER_*
# Non-vacuity (checked on the walk-0 answer, S = 6, (K, nDirs) = (16, 97), no
# jitter): records with a finite non-zero sum, records whose words differ
# between S = 2 and S = 6 (the recursion below the first hit is reached), and,
# with the skip flag, records with a skipped probe: at least 20 of them on c5
# and none on reference.  The probes' start offset is the input chosen per
# scene to meet them (as aogen.RADIUS_MULTIPLE is for the probe length): half
# of the table's directions point below the horizon, and a probe that starts
# 1e-3 off a transparent sphere and enters it at a grazing angle comes back
# NaN from the reference's own arithmetic, which with K = 16 leaves most sums
# of c5 NaN and a few probes of reference non-finite.  Measured walk-0 values
# (records with a point / finite non-zero / differing S 2 vs 6 / skipped > 0):
BIAS = {
    "reference": 5.5,  # 78 / 64 / 61 / 0    (at 1e-3: 73 / 78 / 5; none skipped from 5.0 to 6.25)
    12: 1e-3,          # 69 / 44 / 64 / 20
    40: 1e-3,          # 93 / 41 / 85 / 49
    "base65": 1e-3,    # 69 / 61 / 54 / 1
    "base150": 1e-3,   # 91 / 73 / 82 / 16
    "c5": 1.0,         # 165 / 29 / 156 / 129  (at 1e-3: 12 / 150 / 139)
}
MIN_NONZERO, MIN_DEEPER, MIN_SKIPPED = 20, 15, 20
NON_VACUOUS = ("reference", 12, 40, "base65", "base150", "c5")


def stacks(name):
    return (1, 2, 6, 16) if name in ("reference", "base65") else (1, 2, 6)


def semantics(name):
    return (0, 1) if name in ("reference", 40) else (0,)


def cases(name):
    """(K, nDirs, flags, S, semantics) of scene `name`: every probe set with and
    without jitter and the skip flag at S = 6; the other stack sizes and the
    OpenCL semantics on the largest set plain and on (7, 8) with both flags."""
    out = [(k, nd, fl, 6, 0) for k, nd in PROBES for fl in (0, JITTER, SKIP, JITTER | SKIP)]
    for S in stacks(name):
        if S != 6:
            out += [(16, 97, 0, S, 0), (7, 8, JITTER | SKIP, S, 0)]
    for sem in semantics(name):
        if sem:
            out += [(16, 97, 0, 6, sem), (7, 8, JITTER | SKIP, 6, sem), (16, 97, JITTER, 2, sem)]
    return out


def case_id(c):
    k, nd, fl, S, sem = c
    return f"K{k}-of-{nd}-f{fl}-S{S}-{'cl' if sem else 'cpu'}"


scene = aogen.scene
hits = aogen.hits
dirs = aogen.dirs


def lights(name):
    return mattegen.lights(name)


@functools.lru_cache(maxsize=None)
def weights(n_dirs):
    rng = np.random.default_rng(700 + n_dirs)
    w = rng.uniform(0.1, 1.0, n_dirs).astype(F)
    if n_dirs >= 7:
        w[n_dirs // 4] = 0
        w[n_dirs // 2] = -w[n_dirs // 2]
        w[3 * n_dirs // 4] = np.nan
        w[n_dirs - 1] = np.inf
        assert n_dirs < 16 or n_dirs // 4 >= 16
    w.setflags(write=False)
    return w


def bias(name):
    return BIAS.get(name, aogen.BIAS)


def params(R, name, k, flags):
    return R.gather_params(k, bias(name), SEED, flags)


@functools.lru_cache(maxsize=None)
def want_rays(name, k, n_dirs, flags):
    """gather_rays_host of hits(name), (n * K, 6) float32, read-only."""
    import rtg_amd as R
    out = R.gather_rays_host(hits(name), dirs(n_dirs), params(R, name, k, flags & JITTER),
                             threads=THREADS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(name, k, n_dirs, flags, S=6, sem=0):
    """(sums, skipped) of hits(name) by the plain loops (gather_host walk 0), read-only."""
    import rtg_amd as R
    out, skp = R.gather_host(scene(name), lights(name), hits(name), dirs(n_dirs), weights(n_dirs),
                             params(R, name, k, flags), stack_size=S, semantics=sem, walk=0,
                             threads=THREADS, skipped=True)
    out.setflags(write=False)
    skp.setflags(write=False)
    return out, skp


def canon(a):
    return aogen.canon(a)


def same_words(got, want_):
    return mattegen.same_words(got, want_)


def assert_non_vacuous(name):
    """The issue's conditions, on the walk-0 answer only."""
    if name not in NON_VACUOUS:
        return
    s6, skp = want(name, 16, 97, 0, 6)
    s2, _ = want(name, 16, 97, 0, 2)
    assert not skp.any()  # no flag: no count
    nonzero = int((np.isfinite(s6).all(1) & (s6 != 0).any(1)).sum())
    deeper = int((canon(s6) != canon(s2)).any(1).sum())
    assert nonzero >= MIN_NONZERO, (name, nonzero)
    assert deeper >= MIN_DEEPER, (name, deeper)
    _, skp = want(name, 16, 97, SKIP, 6)
    if name == "c5":
        assert int((skp > 0).sum()) >= MIN_SKIPPED, int((skp > 0).sum())
    if name == "reference":
        assert not skp.any()


# ---- the definition restated in numpy float32, one operation a line ----

def window(n, n_dirs, k, seed, flags):
    """(n, K) table indices j of probe k of point i."""
    i = np.arange(n, dtype=np.uint64)
    s_i = aogen.mix32(np.uint64(seed) + i) % np.uint64(n_dirs) if flags & JITTER \
        else np.zeros(n, np.uint64)
    j = s_i[:, None] + np.arange(k, dtype=np.uint64)[None, :]
    return np.where(j >= n_dirs, j - np.uint64(n_dirs), j).astype(np.int64)


def restate_rays(h, table, k, bias, seed, flags):
    """(n * K, 6) float32 rays of HIT_DTYPE records `h`, point-major."""
    n = len(h)
    bias = F(bias)
    l = table[window(n, len(table), k, seed, flags)]  # (n, K, 3)
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
        w = []
        for q, (t1, t2, nq) in enumerate(((t1x, t2x, Nx), (t1y, t2y, Ny), (t1z, t2z, Nz))):
            u = lx * t1[:, None]
            v = ly * t2[:, None]
            uv = u + v
            ln = lz * nq[:, None]
            w.append(uv + ln)
            off = bias * nq
            aq = P[:, q] + off
            out[..., q] = aq[:, None]
        xx = w[0] * w[0]
        yy = w[1] * w[1]
        xy = xx + yy
        zz = w[2] * w[2]
        dot = xy + zz
        root = np.sqrt(dot)
        inv = one / root
        for q in range(3):
            out[..., 3 + q] = inv * w[q]
    assert out.dtype == F and root.dtype == F
    out[h["id"] < 0] = 0
    return out.reshape(n * k, 6)


def fold(h, colours, table, k, seed, flags):
    """(sums, skipped) of the (n * K, 3) float32 `colours` of the probe rays, in
    the defined order: acc = acc + w * c for k = 0 .. K-1."""
    n = len(h)
    col = np.ascontiguousarray(colours, F).reshape(n, k, 3)
    wt = table[window(n, len(table), k, seed, flags)]  # (n, K)
    acc = np.zeros((n, 3), F)
    skipped = np.zeros(n, np.uint16)
    with np.errstate(all="ignore"):
        for kk in range(k):
            c = col[:, kk, :]
            t = wt[:, kk][:, None] * c
            if flags & SKIP:
                bad = ((c.view(np.uint32) & 0x7F800000) == 0x7F800000).any(1)
                t[bad] = 0
                skipped += bad.astype(np.uint16)
            acc = acc + t
    assert acc.dtype == F
    none = h["id"] < 0
    acc[none] = 0
    skipped[none] = 0
    return acc, skipped
