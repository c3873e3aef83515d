"""Structured scenes for the BVH paths, shared by test_bvh_shapes_host.py and
test_gpu_bvh_shapes.py: inputs that give build_bvh (csrc/rtg_scene_pack.h)
something other than the uniform, clustered and golden scenes of the rest of
the suite.  Seeded and cached, arrays read-only, references computed once.

Scenes (2 to 3 lights each unless said, materials mixed opaque, translucent
and refractive):

  deep19            134 concentric shells at (-3, 1, -15), radius 0.05 * 1.25^i:
                    the area-weighted split peels them one or two at a time, a
                    tree 19 deep (132 shells give 15, 136 give 22: refused)
  deep20            136 shells of radius 0.06 * 1.25^i: exactly 20, the limit
                    (found by scanning n, q in 1.2 .. 2 and r0 in 0.03 .. 0.1
                    with hostsim_bvh_stats; q = 1.3, r0 = 0.05, n = 116 is another)
  refused           deep20 and one more shell: a tree 23 deep, so no BVH and
                    the flat queries, in a finite scene
  coincident        100 identical records among 30 random ones: a tree 50
                    deep, refused; every ray that reaches them ties on index
  wide_deep         a funnel built to fill the traversal stack (chain(), below)
  mirror_x,         40 pairs mirrored in the plane x = 0 with r > a: the two
  mirror_x_swapped  of a pair tie bit for bit for every ray in the plane (the
  mirror_y,         +-0 products vanish in the sums) and sit in different
  mirror_z          subtrees; the lower index on the positive side, or on the
                    negative one when swapped.  mirror_z adds 24 ordinary
                    spheres in front of the camera.
  lattice           5 x 5 x 5, spacing 2, r = 0.6: equal centroids and equal
  lattice_kiss      split costs everywhere; r = 1: exact tangency;
  lattice_overlap   r = 1.3, all translucent: container_bvh, the overlap lists
  many_lights       C5's 1024 spheres under 256 seeded lights: sphere_lists
                    gives up ((m + 1) n^2 > 2^28), BVH queries without lists

Stack occupancy.  BvhStack's host form (rtg_trace.h, under RTG_BVH_STACK_STATS,
which tests/hostsim alone defines) counts the most entries held at once.  At
aa 1: wide_deep holds 19 at 32 x 24, S 6 (20 at aa 2), in a tree 7 deep, whose
structural ceiling is 3 * depth + 3 = 24; C5 holds 13 (at 32 x 24, S 6 and at
48 x 27, S 8), hostile.base(150) 5 and 6; deep19 and deep20 hold 4 in the
sample kernel's form and 15 and 14 in the tile kernel's.  What limits wide_deep:
build_bvh grows every box by 2^-8 of the scene's extent, so structure smaller
than about 1/256 of the scene looks alike to the split, which then peels single
spheres (deep, thin nodes that push nothing); the funnel repeats itself over
some seven levels of three waiting siblings each before that, whatever its
ratio (a seeded search over ratios 0.5 .. 0.95, 1 to 4 pairs per level and 6 to
40 levels found 21 at best without the backdrop spheres, in trees 7 and 8
deep).  A tree that is both 20 deep and three siblings wide at every level has
not been built; the bound 3 * depth + 3 <= 63 is asserted on every scene here.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os

import numpy as np

import raygen
from conftest import GOLDEN, P, load_scene, random_scene

F = np.float32
THREADS = min(16, os.cpu_count() or 1)
MAX_BATCH = 4097


# ---- scenes ----

def _materials(sph, seed, opacities=(0.0, 0.2, 0.5, 0.8, 1.0)):
    """Mixed opaque, translucent and refractive materials, as conftest.random_scene draws them."""
    import rtg_amd as R
    rng = np.random.default_rng(seed)
    for i in range(len(sph)):
        sph[i]["material"] = R.make_material(
            float(rng.choice(opacities)), float(rng.uniform(0, 1)), rng.uniform(0, 1, 3),
            rng.uniform(0, 1, 3), float(rng.choice([1.0, 1.33, 1.55, 2.4])))
    return sph


def _lights(rows):
    import rtg_amd as R
    lg = np.zeros(len(rows), R.LIGHT_DTYPE)
    for l, (pos, col) in enumerate(rows):
        lg[l]["pos"] = pos
        lg[l]["col"] = col
    return lg


CENTRE = (-3.0, 1.0, -15.0)
# Two lights in the gap between the shells on either side of the camera (|CENTRE|
# = 15.3 and theirs, 14.6, lie between the radii 13.2 and 15.9 that bound that gap for
# r0 = 0.05 and 0.06 at q = 1.25), one far outside.
SHELL_LIGHTS = (((1.0, 2.0, -1.0), (1.0, 0.9, 0.8)), ((-6.0, -2.0, -1.0), (0.5, 0.7, 1.0)),
                ((40.0, 60.0, 20.0), (0.8, 0.8, 0.8)))


def shells(n, q=1.25, r0=0.05, seed=5000):
    """n concentric spheres at CENTRE, radius r0 q^i (float64 powers, rounded once)."""
    import rtg_amd as R
    sph = np.zeros(n, R.SPHERE_DTYPE)
    sph["pos"] = CENTRE
    sph["radius"] = (r0 * q ** np.arange(n, dtype=np.float64)).astype(F)
    return _materials(sph, seed), _lights(SHELL_LIGHTS)


def chain(levels, g, L, a, rho, betas=(1.0,), backdrop=True, seed=5100):
    """`wide_deep`: pairs of spheres at (+-a s, 0, -L s), radius rho s, for the
    scales s = g^k beta, k < levels, beta of `betas`: a self-similar funnel
    whose apex is the camera.  A ray down the axis passes between the spheres
    of every pair, through the box of every group of pairs."""
    import rtg_amd as R
    s = (g ** np.arange(levels, dtype=np.float64)[:, None] * np.asarray(betas)[None, :]).reshape(-1)
    sph = np.zeros(2 * len(s), R.SPHERE_DTYPE)
    for side, sign in ((0, 1.0), (1, -1.0)):
        sph["pos"][side::2, 0] = sign * a * s
        sph["pos"][side::2, 2] = -L * s
        sph["radius"][side::2] = rho * s
    if backdrop:  # four large spheres beside the funnel, so that a frame shows something
        sph = np.concatenate([sph, np.zeros(4, R.SPHERE_DTYPE)])
        sph["pos"][-4:] = [(x, y, -1.2 * L) for x in (-0.7 * L, 0.7 * L) for y in (-0.45 * L, 0.45 * L)]
        sph["radius"][-4:] = 0.4 * L
    lg = _lights((((0.0, 30.0, -5.0), (1.0, 1.0, 0.9)), ((12.0, -6.0, 2.0), (0.6, 0.8, 1.0)),
                  ((-5.0, 8.0, 6.0), (0.7, 0.7, 0.7))))
    return _materials(sph, seed), lg


def mirrored(axis, swapped=False, pairs=40, extra=0, seed=5200):
    """`pairs` pairs of spheres mirrored in the plane {coordinate `axis` = 0},
    centres +a and -a off it with r > a, so the two tie bit for bit for every
    ray in the plane.  Pair p is (p, p + pairs): the lower index lies on the
    positive side, or on the negative side when `swapped`.  `extra` ordinary
    spheres follow (the z scene needs them in front of the camera)."""
    import rtg_amd as R
    rng = np.random.default_rng(seed + axis)
    sph = np.zeros(2 * pairs + extra, R.SPHERE_DTYPE)
    lo, hi = np.array([-9.0, -6.0, -20.0]), np.array([9.0, 6.0, -5.0])
    if axis == 2:  # around the plane z = 0, clear of the camera
        lo, hi = np.array([-14.0, -10.0, 0.0]), np.array([14.0, 10.0, 0.0])
    c = rng.uniform(lo, hi, size=(pairs, 3))
    if axis == 2:
        near = np.hypot(c[:, 0], c[:, 1]) < 4.0
        c[near, 0] += np.where(c[near, 0] < 0, -5.0, 5.0)
    a = rng.uniform(0.4, 1.2, pairs)
    r = a * 1.2 + rng.uniform(0.2, 1.8, pairs)
    c[:, axis] = a
    pos, neg = (pairs, 0) if swapped else (0, pairs)
    sph["pos"][pos:pos + pairs] = c
    c[:, axis] = -a
    sph["pos"][neg:neg + pairs] = c
    sph["radius"][:pairs] = r
    sph["radius"][pairs:2 * pairs] = r
    if extra:
        more, _ = random_scene(rng, extra, 0)
        more["radius"] *= F(0.5)
        sph[2 * pairs:] = more
    _materials(sph, seed + 10 + axis)  # (the two of a pair differ in material: a frame shows the tie)
    lg = _lights((((30.0, 40.0, 10.0), (1.0, 0.9, 0.8)), ((-25.0, 5.0, 20.0), (0.5, 0.7, 1.0)),
                  ((0.0, -30.0, -10.0), (0.4, 0.4, 0.4))))
    return sph, lg


def lattice(r, spacing=2.0, seed=5300, opacities=(0.0, 0.2, 0.5, 0.8, 1.0)):
    """5 x 5 x 5 spheres of radius r on a grid of `spacing` around (0, 0, -9)."""
    import rtg_amd as R
    k = np.arange(5, dtype=np.float64) - 2.0
    z, y, x = np.meshgrid(k, k, k, indexing="ij")
    sph = np.zeros(125, R.SPHERE_DTYPE)
    sph["pos"][:, 0] = (x * spacing).reshape(-1)
    sph["pos"][:, 1] = (y * spacing).reshape(-1)
    sph["pos"][:, 2] = (z * spacing).reshape(-1) - 9.0
    sph["radius"] = r
    lg = _lights((((20.0, 30.0, 5.0), (1.0, 0.9, 0.8)), ((-15.0, 4.0, 10.0), (0.5, 0.7, 1.0))))
    return _materials(sph, seed, opacities), lg


def coincident(seed=5400):
    """100 identical records among 30 random ones (15 before, 15 after)."""
    rng = np.random.default_rng(seed)
    rnd, lg = random_scene(rng, 31, 2)
    one = rnd[30:31].copy()
    one["pos"] = (1.0, -1.0, -9.0)
    one["radius"] = 4.0
    one["material"]["opacity"] = 0.5
    return np.concatenate([rnd[:15], np.repeat(one, 100), rnd[15:30]]), lg


def c5():
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        c = json.load(f)["configs"]["c5"]
    return load_scene("c5", c["spheres"], c["lights"])


def many_lights(seed=5500, m=256):
    """C5's spheres under 256 seeded lights, colours scaled by 8 / m."""
    import rtg_amd as R
    sph, _ = c5()
    lo, hi = raygen.bounds(sph)
    span = (hi - lo).max()
    rng = np.random.default_rng(seed)
    lg = np.zeros(m, R.LIGHT_DTYPE)
    lg["pos"] = rng.uniform(lo - 0.5 * span, hi + 0.5 * span, size=(m, 3))
    lg["col"] = rng.uniform(0, 1, size=(m, 3)) * (8.0 / m)
    return sph, lg


# ---- the scene table ----

DEEP20 = dict(n=136, q=1.25, r0=0.06)
WIDE = dict(levels=120, g=0.85, L=20.0, a=1.0, rho=1.0 / 3.0)
# BvhStack's high-water marks on the host (hostsim_bvh_stack), aa 1: wide_deep at
# 32 x 24, S 6; C5 and hostile.base(150), each at 32 x 24, S 6 and at 48 x 27, S 8
WIDE_HIGH_WATER = 19
OTHER_HIGH_WATER = (13, 13, 5, 6)

BUILDERS = {
    "deep19": lambda: shells(134),
    "deep20": lambda: shells(**DEEP20),
    "refused": lambda: shells(**dict(DEEP20, n=DEEP20["n"] + REFUSED_EXTRA)),
    "coincident": coincident,
    "wide_deep": lambda: chain(**WIDE),
    "mirror_x": lambda: mirrored(0),
    "mirror_x_swapped": lambda: mirrored(0, swapped=True),
    "mirror_y": lambda: mirrored(1),
    "mirror_z": lambda: mirrored(2, extra=24),
    "lattice": lambda: lattice(0.6),
    "lattice_kiss": lambda: lattice(1.0),
    "lattice_overlap": lambda: lattice(1.3, opacities=(0.2, 0.5)),
    "many_lights": many_lights,
}
NAMES = tuple(BUILDERS)
REFUSED_EXTRA = 1  # one more shell: a tree 23 deep
# build_bvh's answer per scene: the depth of the tree it keeps, None where it refuses
DEPTH = {"deep19": 19, "deep20": 20, "refused": None, "coincident": None}
MIRRORS = {"mirror_x": 0, "mirror_x_swapped": 0, "mirror_y": 1, "mirror_z": 2}
PAIRS = 40
DEEP = ("deep19", "deep20", "refused")
LATTICES = {"lattice": 0.6, "lattice_kiss": 1.0, "lattice_overlap": 1.3}


@functools.lru_cache(maxsize=None)
def _scene(name):
    sph, lg = BUILDERS[name]()
    sph.setflags(write=False)
    lg.setflags(write=False)
    return sph, lg


def scene(name):
    """(spheres, lights) of a scene, copies."""
    sph, lg = _scene(name)
    return sph.copy(), lg.copy()


def frame_args(name):
    """(W, H, [(aa, S), ...]) of the scene's frames."""
    if name == "many_lights":
        return 16, 12, [(1.0, 3)]
    return 32, 24, [(2.0, 6), (1.0, 1), (1.0, 12)]


def trace_stack(name):
    return 3 if name == "many_lights" else 6


def core(name):
    """The spheres that lay out the batches: every sphere, or the shells below radius 40."""
    sph = _scene(name)[0]
    return sph[sph["radius"] < 40] if name in DEEP else sph


# ---- batches ----

def _in_plane(rng, sph, axis, n):
    """Rays in the mirror plane aimed at the pairs' lenses (the disc of radius
    sqrt(r^2 - a^2) the two spheres share in the plane): three quarters from
    outside, a quarter from inside the pair.  Component `axis` of origin and
    direction is an exact zero."""
    c = sph["pos"][:PAIRS].astype(np.float64)
    a = np.abs(c[:, axis])
    r = sph["radius"][:PAIRS].astype(np.float64)
    lens = np.sqrt(r * r - a * a)
    p = rng.integers(0, PAIRS, n)
    mid = c[p]
    mid[:, axis] = 0.0

    def flat(v):
        v[:, axis] = 0.0
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    aim = mid + flat(rng.normal(size=(n, 3))) * (lens[p] * rng.uniform(0, 0.9, n))[:, None]
    out = np.empty((n, 6))
    o = aim + flat(rng.normal(size=(n, 3))) * rng.uniform(5, 40, n)[:, None]
    inside = np.arange(n) % 4 == 3
    o[inside] = (mid + flat(rng.normal(size=(n, 3))) * (lens[p] * rng.uniform(0, 0.5, n))[:, None])[inside]
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[inside] = flat(rng.normal(size=(n, 3)))[inside]
    d *= np.where(np.arange(n) % 3 == 0, rng.uniform(0.5, 2.0, n), 1.0)[:, None]
    out[:, :3], out[:, 3:] = o, d
    out = out.astype(F)
    out[:, axis] = 0.0
    out[:, 3 + axis] = 0.0
    return out


def _shell_rays(rng, sph, n):
    """A third from 50 .. 300 outside aimed within the sixth shell (half of them
    unnormalised, t near 1); a third from between two shells in a random
    direction; a third from between two shells with a direction so short that
    the query's reach of 1000 ends before the next shell: a miss that still
    walks the tree."""
    c = np.asarray(CENTRE)
    r = sph["radius"].astype(np.float64)
    k = n // 3
    out = np.empty((n, 6))
    o = c + raygen._unit(rng, k) * rng.uniform(50, 300, (k, 1))
    aim = c + raygen._unit(rng, k) * rng.uniform(0, r[5], (k, 1))
    d = aim - o
    d[::2] /= np.linalg.norm(d[::2], axis=1, keepdims=True)
    out[:k, :3], out[:k, 3:] = o, d
    i = rng.integers(0, 60, n - k)
    out[k:, :3] = c + raygen._unit(rng, n - k) * np.sqrt(r[i] * r[i + 1])[:, None]
    d = raygen._unit(rng, n - k)
    d[k:] *= (5e-5 * r[i[k:]])[:, None]
    out[k:, 3:] = d
    return out.astype(F)


def _shell_segments(rng, sph, n):
    """Both ends between the same two shells and near each other (clear), or
    the second end two gaps further out (blocked)."""
    c = np.asarray(CENTRE)
    r = sph["radius"].astype(np.float64)
    i = rng.integers(0, 60, n)
    u = raygen._unit(rng, n)
    a = c + u * np.sqrt(r[i] * r[i + 1])[:, None]
    b = a + raygen._perp(u, rng) * (0.05 * r[i])[:, None]
    far = np.arange(n) % 3 == 0
    b[far] = (c + u * np.sqrt(r[i + 2] * r[i + 3])[:, None])[far]
    return np.concatenate([a, b], axis=1).astype(F)


def _funnel_rays(rng, n):
    """Rays of `wide_deep` in and near the plane x = 0 and down the axis, from
    the apex, from behind it and from the far end looking back."""
    L, a, rho = WIDE["L"], WIDE["a"], WIDE["rho"]
    half = 0.8 * (a - rho) / L  # the slope that still passes between every pair
    out = np.zeros((n, 6))
    k = np.arange(n)
    out[:, 3] = rng.uniform(-half, half, n) * (k % 2)
    out[:, 4] = rng.uniform(-0.5 * rho / L, 0.5 * rho / L, n) * (k % 4 >= 2)
    out[:, 5] = -1.0
    back = k % 5 == 4  # from the far end, towards the apex
    out[back, 0:3] = out[back, 3:6] * (1.5 * L)
    out[back, 3:6] *= -1.0
    behind = k % 5 == 3
    out[behind, 2] = rng.uniform(0.0, 5.0, int(behind.sum()))
    out[behind, 3:5] = 0.0
    return out.astype(F)


def _lattice_rays(rng, sph, spacing, n):
    """Axis-parallel rays along the lattice's lines of centres, through its
    contact points (the midpoints of neighbours, where kissing spheres meet)
    and just beside them."""
    c = sph["pos"].astype(np.float64)
    i = rng.integers(0, len(sph), n)
    ax = rng.integers(0, 3, n)
    side = rng.integers(0, 3, n)  # the line of centres / through the contact point / beside it
    perp = (ax + 1 + rng.integers(0, 2, n)) % 3
    o = c[i].copy()
    o[np.arange(n), perp] += np.where(side == 0, 0.0, 0.5 * spacing) + np.where(side == 2, 1e-4, 0.0)
    d = np.zeros((n, 3))
    sign = np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)
    d[np.arange(n), ax] = sign
    o -= d * rng.uniform(6, 20, n)[:, None]
    return np.concatenate([o, d], axis=1).astype(F)


def _mix(sph, seed, sizes=(700, 300, 150, 700)):
    rng = np.random.default_rng(seed)
    return np.concatenate([raygen.inside(rng, sph, sizes[0]), raygen.outside(rng, sph, sizes[1]),
                           raygen.scaled(rng, sph, sizes[2]), raygen.surface(rng, sph, sizes[3]),
                           raygen.primary(16, 12)]).astype(F)


@functools.lru_cache(maxsize=None)
def _batches(name):
    k = NAMES.index(name)
    sph = core(name)
    rng = np.random.default_rng(6100 + k)
    rays = [_mix(sph, 6000 + k)]
    segs = [raygen.segments(np.random.default_rng(6200 + k), sph, 1500)]
    if name in MIRRORS:
        plane = _in_plane(rng, _scene(name)[0], MIRRORS[name], 2000)
        rays.append(plane)
        far = plane[:800].copy()  # segments in the plane: through the lens and half as far again
        far[:, 3:] = far[:, :3] + far[:, 3:] * rng.uniform(5, 60, (800, 1)).astype(F)
        far[:, MIRRORS[name]] = 0.0
        far[:, 3 + MIRRORS[name]] = 0.0
        segs.append(far)
    if name in DEEP:
        rays.append(_shell_rays(rng, _scene(name)[0], 1800))
        segs.append(_shell_segments(rng, _scene(name)[0], 1500))
    if name == "wide_deep":
        fun = _funnel_rays(rng, 1200)
        rays.append(fun)
        seg = fun[:600].copy()
        seg[:, 3:] = seg[:, :3] + seg[:, 3:] * rng.uniform(1, 1.2 * WIDE["L"], (600, 1)).astype(F)
        segs.append(seg)
    if name in LATTICES:
        lat = _lattice_rays(rng, sph, 2.0, 1200)
        rays.append(lat)
        seg = lat[:600].copy()
        seg[:, 3:] = seg[:, :3] + seg[:, 3:] * rng.uniform(4, 30, (600, 1)).astype(F)
        segs.append(seg)
    rays, segs = (np.ascontiguousarray(np.concatenate(b), F) for b in (rays, segs))
    assert len(rays) <= MAX_BATCH and len(segs) <= MAX_BATCH, (len(rays), len(segs))
    rays.setflags(write=False)
    segs.setflags(write=False)
    return rays, segs


def batches(name):
    """(rays, segments) of a scene, (N, 6) float32, read-only and shared: the
    raygen mix over the scene's bounds, then the family's directed rays."""
    return _batches(name)


def plane_rays(name):
    """The slice of batches(name)[0] that lies in the mirror plane."""
    n = len(_batches(name)[0])
    return slice(n - 2000, n)


@functools.lru_cache(maxsize=None)
def points(name):
    """Containment points: centres, half radii, around the surfaces, uniform in
    the bounds, between the shells, at the lattice's contact points, a NaN and
    a far point; (N, 3) float32, read-only."""
    geo = core(name)
    rng = np.random.default_rng(6300 + NAMES.index(name))
    c = geo["pos"].astype(np.float64)
    r = np.abs(geo["radius"].astype(np.float64))
    lo, hi = raygen.bounds(geo)
    i = rng.integers(0, len(geo), 20)
    parts = [c[i]]
    i = rng.integers(0, len(geo), 30)
    parts.append(c[i] + 0.5 * r[i][:, None] * raygen._unit(rng, 30))
    for f in (1 - 1e-3, 1.0, 1 + 1e-6, 1 + 1e-3):
        i = rng.integers(0, len(geo), 20)
        parts.append(c[i] + f * r[i][:, None] * raygen._unit(rng, 20))
    parts.append(rng.uniform(lo, hi, size=(150, 3)))
    if name in DEEP:
        full = _scene(name)[0]["radius"].astype(np.float64)
        i = rng.integers(0, len(full) - 1, 100)
        parts.append(np.asarray(CENTRE) + raygen._unit(rng, 100) * np.sqrt(full[i] * full[i + 1])[:, None])
    if name in LATTICES:
        i = rng.integers(0, len(geo), 100)
        step = np.zeros((100, 3))
        step[np.arange(100), rng.integers(0, 3, 100)] = 1.0  # the contact point towards a neighbour
        parts.append(c[i] + step * np.where(np.arange(100) % 2, 1.0, 1.0 + 1e-7)[:, None])
    pts = np.concatenate(parts + [[[np.nan, 0.0, -10.0]], [[1e30, 0.0, 0.0]]]).astype(F)
    pts.setflags(write=False)
    return np.ascontiguousarray(pts)


POSES = {  # (outside, between shells or inside the structure)
    "default": (((3.0, 2.0, 4.0), (0.0, 0.0, -15.0)), ((-1.0, 0.5, -6.0), (-3.0, 1.0, -15.0))),
    "many_lights": (((3.0, 2.0, 4.0), (0.0, 0.0, -15.0)), ((2.0, 3.0, -3.0), (0.0, 0.0, -20.0))),
}


def poses(name):
    """Two look_at poses: one outside the scene's core, one within it (between
    two shells for the deep scenes)."""
    if name in DEEP:  # 14.3 from CENTRE: in the gap that holds the camera and two lights
        return ((3.0, 2.0, 4.0), CENTRE), ((-3.0, 7.0, -2.0), CENTRE)
    return POSES.get(name, POSES["default"])


# ---- references: the oracle and the plain loops, computed once ----

_frames = {}


def lit_fraction(fb):
    return float(((np.ascontiguousarray(fb, F).view(np.uint32) << 1) != 0).mean())


def oracle_frame(oracle, name, w, h, s, aa):
    """The oracle's frame, lit in at least 5 % of its words."""
    key = (name, w, h, s, aa)
    if key not in _frames:
        sph, lg = _scene(name)
        fb = oracle.render(sph, lg, w, h, s, aa=aa)
        assert lit_fraction(fb) >= 0.05, (key, lit_fraction(fb))
        fb.setflags(write=False)
        _frames[key] = fb
    return _frames[key]


HITS_N = {"many_lights": 600}


@functools.lru_cache(maxsize=None)
def walk0(name):
    """(hits, visible) of the scene's batches by the plain loops."""
    import rtg_amd as R
    sph = _scene(name)[0]
    rays, segs = _batches(name)
    out = (R.intersect_host(sph, rays, walk=0, threads=THREADS),
           R.visible_host(sph, segs, walk=0, threads=THREADS))
    for a in out:
        a.setflags(write=False)
    return out


def hits(name):
    """The hit records the point queries take: the plain-loop hits of the batch
    (the first 600 of many_lights, whose 256 lights make each record dear)."""
    return walk0(name)[0][:HITS_N.get(name, MAX_BATCH)]


def trace_rays(name):
    return _batches(name)[0][:HITS_N.get(name, MAX_BATCH)]


@functools.lru_cache(maxsize=None)
def colours0(name, sem=0):
    import rtg_amd as R
    sph, lg = _scene(name)
    out = R.raytrace_host(sph, lg, trace_rays(name), stack_size=trace_stack(name), semantics=sem,
                          walk=0, threads=THREADS)
    out.setflags(write=False)
    return out


AO_K, AO_DIRS = 7, 8


def ao_params(R, name, flags):
    import aogen
    r = np.abs(core(name)["radius"].astype(np.float64))
    return R.ao_params(AO_K, float(F(2.5 * r.max())), aogen.BIAS, aogen.SEED, flags)


@functools.lru_cache(maxsize=None)
def ao0(name, flags):
    import aogen
    import rtg_amd as R
    out = R.ao_host(_scene(name)[0], hits(name), aogen.dirs(AO_DIRS), ao_params(R, name, flags),
                    walk=0, threads=THREADS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def matte0(name):
    """(sums, masks) of hits(name) by the plain loops."""
    import rtg_amd as R
    sph, lg = _scene(name)
    out, lit = R.matte_host(sph, lg, hits(name), walk=0, threads=THREADS, mask=True)
    out.setflags(write=False)
    lit.setflags(write=False)
    return out, lit


@functools.lru_cache(maxsize=None)
def contains0(name):
    import rtg_amd as R
    out = R.contains_host(_scene(name)[0], points(name), walk=0, threads=THREADS)
    out.setflags(write=False)
    return out


VW, VH, VS = 32, 24, 6


def view_table(R, name):
    """(4, 12) float32 poses: outside, within, the identity and a NaN pose."""
    out, within = poses(name)
    cams = np.concatenate([np.asarray(c).reshape(1) for c in (
        R.camera_look_at(*out), R.camera_look_at(*within), R.camera_identity(),
        R.camera_look_at(*out))])
    table = np.ascontiguousarray(cams.view(F).reshape(4, 12)).copy()
    table[3, 1] = np.nan
    return table


@functools.lru_cache(maxsize=None)
def views0(name, sem=0):
    import rtg_amd as R
    sph, lg = _scene(name)
    out = R.render_views_host(sph, lg, view_table(R, name), VW, VH, alias_factor=2.0,
                              stack_size=trace_stack(name), semantics=sem, walk=0,
                              threads=THREADS)
    out.setflags(write=False)
    return out


# The gather over hits(name): K = 7 of gathergen.dirs(8) (a zero, a NaN and a
# x1000 direction among them), plain finite weights (gathergen.weights plants a
# NaN weight, which turns most sums into NaN), plain and with both flags.
GATHER_K, GATHER_DIRS = 7, 8
GATHER_FLAGS = (0, 1 | 2)  # RTG_GATHER_JITTER | RTG_GATHER_SKIP_NONFINITE
GATHER_SKIP = 2


def gather_weights():
    w = np.full(GATHER_DIRS, 1.0 / GATHER_DIRS, F)
    w.setflags(write=False)
    return w


def gather_params(R, flags):
    import aogen
    return R.gather_params(GATHER_K, aogen.BIAS, aogen.SEED, flags)


@functools.lru_cache(maxsize=None)
def gather0(name, flags, sem=0):
    """(sums, skip counts) of hits(name) by the plain loops."""
    import gathergen
    import rtg_amd as R
    sph, lg = _scene(name)
    out, skp = R.gather_host(sph, lg, hits(name), gathergen.dirs(GATHER_DIRS), gather_weights(),
                             gather_params(R, flags), stack_size=trace_stack(name), semantics=sem,
                             walk=0, threads=THREADS, skipped=True)
    out.setflags(write=False)
    skp.setflags(write=False)
    return out, skp


# The fold of views0(name)'s four frames: two groups of two views (the NaN pose
# is the second view of the second group), K = 4 seeded weights a texel.
FOLD_G, FOLD_K = 2, 4
FOLD_SKIP = 1  # RTG_FOLD_SKIP_NONFINITE
NAN_GROUP = 1


@functools.lru_cache(maxsize=None)
def fold_weights():
    from test_views_fold_host import random_weights
    w = random_weights(np.random.default_rng(6500), FOLD_G, VW, VH, FOLD_K)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def fold0(name, flags, sem=0):
    """(coefficients (2, FOLD_K, 3) float32, skip counts) of views_fold_host
    over views0(name, sem)."""
    import rtg_amd as R
    out, cnt = R.views_fold_host(views0(name, sem), fold_weights(),
                                 R.fold_params(FOLD_G, FOLD_K, flags), threads=THREADS,
                                 skipped=True)
    out.setflags(write=False)
    cnt.setflags(write=False)
    return out, cnt


def gather_shares(name):
    """Of the points with id >= 0: the share with a finite non-zero sum with
    flags 0, the same with both flags, and the points with a skipped probe."""
    real = hits(name)["id"] >= 0

    def share(s):
        return float((np.isfinite(s).all(1) & (s != 0).any(1))[real].mean())
    plain, none = gather0(name, GATHER_FLAGS[0])
    both, skp = gather0(name, GATHER_FLAGS[1])
    assert not none.any()  # no flag: no count
    return share(plain), share(both), int((skp[real] > 0).sum())


def check_gather_fold_non_vacuous(name):
    """On the REFERENCE answers: at least 5 % of the points with a finite
    non-zero sum plain and 15 % with the skip flag; coefficients that are not
    all zero; without the flag no count, with it each group's count is the
    number of its pixels with a non-finite word, counted here in numpy.  (The
    NaN pose's rays meet nothing, so its own frame is black, not NaN: the
    non-finite pixels of a group are the scene's, and the deep scenes,
    wide_deep and many_lights have none in the NaN pose's group.  The counts
    across the scenes: test_bvh_shapes_host.py.)"""
    from test_views_fold_host import nonfinite_pixels
    plain, both, _ = gather_shares(name)
    assert plain >= 0.05 and both >= 0.15, (name, plain, both)
    bad = nonfinite_pixels(views0(name)).reshape(2, -1).sum(1)
    for flags in (0, FOLD_SKIP):
        out, cnt = fold0(name, flags)
        assert (out.view(np.uint32) << 1).any(), (name, flags, "the coefficients are all zero")
        assert (cnt == (bad if flags else 0)).all(), (name, flags, cnt, bad)


# ---- non-vacuity: conditions on the REFERENCE answers ----

def check_non_vacuous(name):
    """hostile.assert_fractions on the plain-loop answers; for a mirror scene,
    at least 200 of the in-plane rays reach both spheres of a pair at a
    bit-equal t and the plain loop names the lower index; for lattice_overlap,
    points inside at least two spheres."""
    import hostile
    import rtg_amd as R
    h, vis = walk0(name)
    hostile.assert_fractions(h, vis)
    if name in MIRRORS:
        assert tie_count(name) >= 200, tie_count(name)
    if name == "lattice_overlap":
        sph = _scene(name)[0]
        first = contains0(name)
        inside = np.flatnonzero(first >= 0)
        # the literal loop over the reversed scene names the LAST container
        again = R.contains_host(sph[::-1].copy(), points(name), walk=0, threads=THREADS)
        last = np.where(again >= 0, len(sph) - 1 - again, -1)
        assert int((last[inside] != first[inside]).sum()) >= 20, "points inside two spheres"


@functools.lru_cache(maxsize=None)
def tie_count(name):
    """In-plane rays whose plain-loop hit is a paired sphere p < PAIRS and whose
    t against sphere p alone and against sphere p + PAIRS alone is bit-equal."""
    import rtg_amd as R
    sph = _scene(name)[0]
    rays = _batches(name)[0][plane_rays(name)]
    h = walk0(name)[0][plane_rays(name)]
    ties = 0
    for p in np.unique(h["id"]):
        if not 0 <= p < PAIRS:
            continue
        sel = np.flatnonzero(h["id"] == p)
        a = R.intersect_host(sph[p:p + 1].copy(), rays[sel], walk=0)
        b = R.intersect_host(sph[p + PAIRS:p + PAIRS + 1].copy(), rays[sel], walk=0)
        both = (a["id"] == 0) & (b["id"] == 0)
        ties += int((both & (a["t"].view(np.uint32) == b["t"].view(np.uint32))
                     & (a["t"].view(np.uint32) == h["t"][sel].view(np.uint32))).sum())
    return ties


# ---- the builder's answer and the host stack's occupancy (tests/hostsim) ----

def bvh_stats(hs, name_or_scene):
    """{built, nodes, depth, lists} of hostsim_bvh_stats: `depth` is that of the
    tree build_bvh made, kept or refused."""
    sph, lg = _scene(name_or_scene) if isinstance(name_or_scene, str) else name_or_scene
    out = (ctypes.c_long * 4)()
    hs.hostsim_bvh_stats(P(sph), len(sph), P(lg), len(lg), out)
    return {"built": bool(out[0]), "nodes": int(out[1]), "depth": int(out[2]), "lists": bool(out[3])}


def stack_marks(hs, reset=True):
    """(high-water mark, overflow flag) of BvhStack's host form since the last reset."""
    out = (ctypes.c_long * 2)()
    hs.hostsim_bvh_stack(out, int(reset))
    return int(out[0]), int(out[1])
