"""Hostile scenes shared by test_hostile_host.py and test_gpu_hostile.py: four
seeded base scenes and a table of named one- or two-record mutations (NaN,
infinite, zero, negative and huge radii and centres, the camera or a light
inside a sphere, coincident spheres, out-of-range materials and colours).

Scene data decides which tables rtg_scene_pack.h builds and so which kernel
instantiation a context launches; `expect(n, name)` states that choice from the
builders' own conditions (shadow_masks, build_bvh, sphere_lists), and the GPU
test checks the BVH half of it against Context.scene_stats().

Ray and segment batches come from the BASE scene (raygen.bounds of a mutated
scene would be NaN, and the geometry hardly moves); the mutated scene is then
queried with them.  The non-vacuity helpers at the end are asserted on the
reference answers (the oracle, the plain loops), never on the code under test.
"""
from __future__ import annotations

import functools

import numpy as np

import raygen
from conftest import random_scene

F = np.float32
SIZES = (8, 64, 65, 150)  # masks; the last mask size; the first BVH size; a deeper tree
NAN, INF = F(np.nan), F(np.inf)


# Seeds 1000 + n, but 3000 + n for 64 spheres: both lights of seed 1064 lie below
# y = -5, under `huge`'s surface, and the reference's depth-0 frame of `all` is black.
SEEDS = {8: 1008, 64: 3064, 65: 1065, 150: 1150}


@functools.lru_cache(maxsize=None)
def _base(n):
    sph, lg = random_scene(np.random.default_rng(SEEDS[n]), n, 2)
    if n > 64:
        sph["radius"] *= F(0.4)  # not one blob
    return sph, lg


def base(n):
    sph, lg = _base(n)
    return sph.copy(), lg.copy()


# ---- the mutations: (sph, lg) -> (sph, lg), in place on the caller's copies ----

def _place(sph, i, pos, r):
    sph["pos"][i] = pos
    sph["radius"][i] = r


def inside(sph, lg, i=0):
    """The camera inside a refractive sphere."""
    _place(sph, i, (0.5, -0.25, 1.0), 5.0)
    sph["material"]["opacity"][i] = 0.2
    return sph, lg


def inside_opaque(sph, lg, i=1):
    _place(sph, i, (0.0, 0.0, -1.0), 30.0)
    sph["material"]["opacity"][i] = 1.0
    return sph, lg


def dup(sph, lg, a=0, b=1, c=2, d=3):
    """Index ties: b is a's whole record, d takes c's centre and radius only."""
    sph[b] = sph[a]
    sph["pos"][d] = sph["pos"][c]
    sph["radius"][d] = sph["radius"][c]
    return sph, lg


def r0(sph, lg, i=0, j=2):
    sph["radius"][i] = 0.0
    sph["radius"][j] = -sph["radius"][j]
    return sph, lg


def rnan(sph, lg, i=0):
    sph["radius"][i] = NAN
    return sph, lg


def rinf(sph, lg, i=0):
    sph["radius"][i] = INF
    return sph, lg


def cnan(sph, lg, i=0):
    sph["pos"][i, 1] = NAN
    return sph, lg


def cinf(sph, lg, i=0, j=1):
    sph["pos"][i, 0] = INF
    sph["pos"][j, 2] = -INF
    return sph, lg


def huge(sph, lg, i=0):
    """A ground plane."""
    _place(sph, i, (0.0, -10005.0, -20.0), 1.0e4)
    return sph, lg


def tiny(sph, lg, i=0, j=1):
    sph["radius"][i] = 1.0e-20  # below 2^-60: its square is 0
    sph["radius"][j] = 1.0e-6
    return sph, lg


def big31(sph, lg, i=0):
    """Finite, but above the builders' 1e30."""
    _place(sph, i, (1.0e31, 0.0, -1.0e31), 1.0e31)
    return sph, lg


def big2_57(sph, lg, i=0):
    """Passes the builders' `finite`, fails build_bvh's omax <= 2^56."""
    _place(sph, i, (2.0 ** 57, 0.0, 0.0), 2.0 ** 56)
    return sph, lg


def czero(sph, lg, i=0):
    _place(sph, i, (0.0, 0.0, 0.0), 0.5)
    return sph, lg


def light_in(sph, lg, i=0, l=0):
    lg["pos"][l] = sph["pos"][i]
    return sph, lg


def light_near(sph, lg, i=0):
    u = np.array([0.6, 0.64, 0.48])
    lg["pos"][0] = sph["pos"][i].astype(np.float64) + 0.1 * float(sph["radius"][i]) * u
    return sph, lg


def light_inf(sph, lg):
    lg["pos"][0, 0] = INF
    return sph, lg


def light_nan(sph, lg):
    lg["pos"][0, 1] = NAN
    return sph, lg


def light_cam(sph, lg):
    """Light 0 at the camera; one coordinate is the negative zero, which
    compares and adds as zero (and gives the scene file a -0 to carry)."""
    lg["pos"][0] = (0.0, -0.0, 0.0)
    return sph, lg


def mat(sph, lg, hi=0, lo=1, n0=2, nhalf=3, nnan=4):
    """Opacity 2.0 and -0.5; refractive index 0, 0.5 and NaN on spheres made
    translucent, so that the index is used."""
    m = sph["material"]
    m["opacity"][hi] = 2.0
    m["opacity"][lo] = -0.5
    for i, v in ((n0, 0.0), (nhalf, 0.5), (nnan, NAN)):
        m["opacity"][i] = 0.2
        m["refractiveIndex"][i] = v
    return sph, lg


def col(sph, lg):
    sph["material"]["matteColour"][0] = (INF, 1.0e30, -1.0)
    sph["material"]["glossColour"][1] = (NAN, 0.0, 5.0)
    lg["col"][0] = (1.0e38, -1.0, NAN)
    return sph, lg


def all_(sph, lg):
    """inside, dup (on other indices), r0, cnan, huge, light_in and mat at once,
    on the first eight records.  The material values go to the spheres that
    can still be a closest hit (0, 2, 4 and 5: 1 has no surface, 3 is NaN, 6
    and 7 lose their ties)."""
    inside(sph, lg, 0)
    r0(sph, lg, 1, 2)
    cnan(sph, lg, 3)
    huge(sph, lg, 4)
    dup(sph, lg, 5, 6, 2, 7)  # 7 ties with the negated radius of 2
    # the lower light moves (the one `huge` is likeliest to bury); the other stays
    light_in(sph, lg, 5, l=int(np.argmin(lg["pos"][:, 1])))
    m = sph["material"]
    m["refractiveIndex"][0] = 0.5  # (opacity 0.2 from `inside`)
    m["opacity"][2], m["refractiveIndex"][2] = -0.5, 0.0
    m["opacity"][4] = 2.0
    m["opacity"][5], m["refractiveIndex"][5] = 0.2, NAN
    return sph, lg


MUTATIONS = {
    "inside": inside, "inside_opaque": inside_opaque, "dup": dup, "r0": r0, "rnan": rnan,
    "rinf": rinf, "cnan": cnan, "cinf": cinf, "huge": huge, "tiny": tiny, "big31": big31,
    "big2_57": big2_57, "czero": czero, "light_in": light_in, "light_near": light_near,
    "light_inf": light_inf, "light_nan": light_nan, "light_cam": light_cam, "mat": mat,
    "col": col, "all": all_,
}
NAMES = tuple(MUTATIONS)
GEOMETRY = NAMES[:NAMES.index("czero") + 1]  # the mutations that move or remove a surface
# build_bvh's `finite` (NaN, infinite or above 1e30) or omax <= 2^56 fails: no BVH at n > 64
NO_BVH = ("rnan", "rinf", "cnan", "cinf", "big31", "big2_57", "all")
# shadow_masks' / sphere_lists' `finite` fails (spheres or lights): no masks at
# n <= 64, no sphere lists at n > 64
NO_MASKS = ("rnan", "rinf", "cnan", "cinf", "big31", "light_inf", "light_nan", "all")
CASES = [(n, name) for n in SIZES for name in NAMES]
IDS = [f"n{n}-{name}" for n, name in CASES]


@functools.lru_cache(maxsize=None)
def _mutated(n, name):
    return MUTATIONS[name](*base(n))


def mutated(n, name):
    """The mutated scene (copies; "base" is the base scene itself; n = LARGE_N
    is the large scene, "base" or "cnan")."""
    if n == LARGE_N:
        base_sph, sph, lg = large()
        assert name in ("base", "cnan")
        return (base_sph if name == "base" else sph), lg
    sph, lg = _base(n) if name == "base" else _mutated(n, name)
    return sph.copy(), lg.copy()


def expect(n, name):
    """(tables, query path) a context takes for the scene, from the builders'
    conditions: "masks" / "no masks" (n <= 64: shadow, overlap and cone masks),
    "lists" / "no lists" (BVH scenes: capsule and overlap lists); and the
    closest-hit / shadow query: "64" (n4 <= 64), "bvh" or "flat"."""
    if n <= 64:
        return ("no masks" if name in NO_MASKS else "masks"), "64"
    if name in NO_BVH:
        return "no lists", "flat"
    return ("no lists" if name in NO_MASKS else "lists"), "bvh"


LARGE_N = 1100


@functools.lru_cache(maxsize=None)
def _large():
    sph, lg = random_scene(np.random.default_rng(99), LARGE_N, 2)
    sph["radius"] *= F(0.3)
    base_sph = sph.copy()
    cnan(sph, lg)
    return base_sph, sph, lg


def large():
    """1100 spheres with `cnan`: above 1025 materials (the global-material
    path) and no BVH (the flat queries): (base spheres, spheres, lights)."""
    return tuple(a.copy() for a in _large())


def nan_sphere_scene():
    """A scene of one NaN sphere only (key_bounds falls back to [-1, 1]^3)."""
    sph, lg = base(8)
    sph = sph[:1].copy()
    sph["pos"][0] = NAN
    sph["radius"][0] = NAN
    return sph, lg


# ---- rays and segments, from the base scene ----

N_RAYS = 1500 + 600 + 300 + 1500 + 432
N_SEGS = 2000


def _rays_of(sph, seed, n_inside=1500, n_outside=600, n_scaled=300, n_surface=1500, prim=(24, 18)):
    rng = np.random.default_rng(seed)
    rays = np.concatenate([raygen.inside(rng, sph, n_inside), raygen.outside(rng, sph, n_outside),
                           raygen.scaled(rng, sph, n_scaled), raygen.surface(rng, sph, n_surface),
                           raygen.primary(*prim)])
    return np.ascontiguousarray(rays, F)


@functools.lru_cache(maxsize=None)
def _batches(n):
    sph = _base(n)[0] if n != LARGE_N else _large()[0]
    if n == LARGE_N:
        rays = _rays_of(sph, 7000 + n, 700, 300, 150, 700, (15, 10))
        segs = raygen.segments(np.random.default_rng(8000 + n), sph, 1000)
    else:
        rays = _rays_of(sph, 7000 + n)
        segs = raygen.segments(np.random.default_rng(8000 + n), sph, N_SEGS)
    rays.setflags(write=False)
    segs.setflags(write=False)
    return rays, segs


def batches(n):
    """(rays, segments) of base scene n (or of the large scene), (N, 6)
    float32, read-only and shared."""
    return _batches(n)


POSE = ((3.0, 2.0, 4.0), (0.0, 0.0, -15.0))  # look_at(eye, target): one non-identity pose


# ---- the sort key, restated in numpy float32 (rtg_order.h, key_bounds) ----

def restate_key_bounds(sph):
    c = sph["pos"].astype(F).reshape(-1, 3)
    r = np.abs(sph["radius"].astype(F)).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(c) < INF).all(1) & (r < INF)  # NaN compares false
    if not ok.any():
        return np.full(3, -1, F), np.full(3, 1, F)
    c, r = c[ok], r[ok][:, None]
    with np.errstate(over="ignore"):
        return (c - r).min(0), (c + r).max(0)


def _quantise(v, top):
    with np.errstate(invalid="ignore"):
        c = np.where(v >= 0, v, F(0))  # NaN: 0
        c = np.where(c <= top, c, top)
    return c.astype(np.int64).astype(np.uint64)


def _spread(v, step, bits):
    out = np.zeros(v.shape, np.uint64)
    for i in range(bits):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(step * i)
    return out


def restate_keys(sph, rays, kind=0, origin_bits=10, dir_bits=10):
    """uint64 keys of an (N, 6) float32 batch over the scene's key box: bits
    49..20 the Morton code of the origin's cell, bits 19..0 of the direction's
    octahedral bin; a segment (a, b) is the ray (a, b - a).  Every operation is
    the float32 one rtg_order.h names."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    lo, hi = restate_key_bounds(sph)
    with np.errstate(all="ignore"):
        w = hi - lo
        s = np.where((w > 0) & (w < INF), F(1 << origin_bits) / np.where(w > 0, w, F(1)), F(0))
        s = np.where(s < INF, s, F(0)).astype(F)
        o, d = rays[:, :3], rays[:, 3:]
        if kind == 1:
            d = d - o
        cell = _quantise((o - lo) * s, F((1 << origin_bits) - 1))
        sm = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        ok = (sm > 0) & (sm < INF)
        div = np.where(ok, sm, F(1))
        px, py = d[:, 0] / div, d[:, 1] / div
        qx, qy = F(1) - np.abs(py), F(1) - np.abs(px)
        low = d[:, 2] < 0
        px, py = (np.where(low, np.where(d[:, 0] < 0, -qx, qx), px),
                  np.where(low, np.where(d[:, 1] < 0, -qy, qy), py))
        half, top = F(1 << (dir_bits - 1)), F((1 << dir_bits) - 1)
        u = np.where(ok, _quantise((px + F(1)) * half, top), np.uint64(0))
        v = np.where(ok, _quantise((py + F(1)) * half, top), np.uint64(0))
    om = (_spread(cell[:, 0], 3, origin_bits) | (_spread(cell[:, 1], 3, origin_bits) << np.uint64(1))
          | (_spread(cell[:, 2], 3, origin_bits) << np.uint64(2)))
    dm = _spread(u, 2, dir_bits) | (_spread(v, 2, dir_bits) << np.uint64(1))
    return (om << np.uint64(2 * dir_bits)) | dm


def restate_order(keys):
    return np.argsort(keys, kind="stable").astype(np.uint32)


# ---- non-vacuity: conditions on the REFERENCE answers ----

def assert_hits_differ(name, hits, base_hits):
    """A geometry mutation changes the plain-loop hits of the base scene's rays."""
    if name in GEOMETRY:
        assert hits.tobytes() != base_hits.tobytes(), f"{name}: the plain-loop hits did not move"


def assert_fractions(hits, vis):
    """The walk-0 answers of a batch are neither all hits nor all misses."""
    hit = float((hits["id"] >= 0).mean())
    seen = float((np.asarray(vis) == 1).mean())
    assert 0.2 <= hit <= 0.9, f"hit fraction {hit:.3f}"
    assert 0.1 <= seen <= 0.9, f"visible fraction {seen:.3f}"


def assert_lit(frame):
    """An oracle frame has a nonzero pixel (NaN counts: it is not black)."""
    assert (np.ascontiguousarray(frame, F).view(np.uint32) << 1).any(), "black oracle frame"


def nan_words(a):
    return int(np.isnan(np.ascontiguousarray(a, F)).sum())
