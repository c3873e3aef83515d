"""Inputs and references shared by the scale tests (test_scale_host.py,
test_gpu_scale.py): the scenes, ray batches, hit records and frame signals of
the other modules multiplied by powers of two, with the plain-loop answers,
computed once and left unchanged.

Every other test input lives at one magnitude (scenes about 10 units across,
signals of order 1).  The code that exists only in the device build, the
hardware square root, reciprocal and reciprocal square root with their
refinements, range tests and wave-uniform fallback branches (csrc/rtg_trace.h),
and the frame passes' plain `/` and sqrtf compiled for the device, is where
the magnitude matters; so the same calls are repeated here on

  scene(name, j)     sphere positions and radii and light positions x 2^j
  rays(name, j, d)   test_raytrace_host.mixed_rays with origins x 2^j and
                     directions x 2^j (d = "scaled") or as they are ("unit")
  laned(name, j)     rays(name, j, "unit") with the direction of lane l of every
                     64 x 2^delta(l): every wave holds lanes on both sides of
                     the quotient's range test and of the square root's
                     (LANE_EXPONENTS)
  segments(name, j)  from the walk-0 hits of rays(name, j, "scaled"): for a hit
                     (o, o + 2 t d), (o, o + t d / 2) and a segment through the
                     hit point (segments_of), for a miss (o, o + d)
  hits(name, j)      those walk-0 records, for rtg_ao*, rtg_matte*, rtg_gather*
  frame signals      filtergen / svgfgen / accumgen signals x 2^k, second
                     moments and variances x 2^2k

All scalings are float32 products by a power of two: exact unless the result
leaves the normal range, and then still a legal input.
"""
from __future__ import annotations

import functools

import numpy as np

import accumgen
import aogen
import filtergen as G
import gathergen
import svgfgen
from test_raytrace_host import THREADS, mixed_rays, scene_with_lights

F = np.float32

SCENES = [12, 64, 65, 200, "c5"]  # 12, 64: the masked kernel; 65, 200, c5: the BVH with lists
J_SCALED = (-60, -40, -24, -12, 12, 24, 30)
J_UNIT = (-12, 6)
BATCHES = [(j, "scaled") for j in J_SCALED] + [(j, "unit") for j in J_UNIT]
BATCH_IDS = [f"j{j}-{d}" for j, d in BATCHES]
J_LANED = (-60, -24, -12, 12, 30)
FRAMES = [(64, -20), (64, -8), (65, -20), (65, -8), (200, -20), (200, -8), (200, 8)]
FRAME_W, FRAME_H, FRAME_AA, FRAME_S = 48, 36, 2.0, 6
K_SIGNAL = (-149, -140, -126, -64, 63, 64, 120, 127)
J_POSE = (-60, -24, 24, 60)
PASS_SCENES = ["reference", "c5"]
PASS_FRAMES = [(33, 17), (67, 35)]
STACK = 6
N_RAYS = 2048  # 32 waves
N_POINTS = 256  # hit records of the fused passes
AO_K, AO_DIRS = 7, 8
GATHER_K, GATHER_DIRS = 5, 8  # entries 0 .. 4: a zero and a negative weight, a zero and a NaN direction

# The non-vacuity floors, on the plain loops' and the oracle's answers only.
MIN_HIT, MIN_LIT, MIN_BLOCKED, MIN_FRAME = 0.10, 0.05, 0.05, 0.15


def pow2(j):
    """2^j as a float32; j from -149 to 127."""
    return F(np.ldexp(1.0, j))


def times(a, j):
    """a x 2^j in float32, in two steps where 2^j alone is not a float32
    factor that keeps the product exact (|j| up to 149 here)."""
    a = np.asarray(a, F)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if -126 <= j <= 127:
            return (a * pow2(j)).astype(F)
        return ((a * pow2(-126)).astype(F) * pow2(j + 126)).astype(F)


# ---- scenes and batches ----

@functools.lru_cache(maxsize=None)
def scene(name, j):
    """(spheres, lights) of test_raytrace_host.scene_with_lights(name) x 2^j, read-only."""
    sph, lg = (a.copy() for a in scene_with_lights(name))
    sph["pos"] = times(sph["pos"], j)
    sph["radius"] = times(sph["radius"], j)
    lg["pos"] = times(lg["pos"], j)
    sph.setflags(write=False)
    lg.setflags(write=False)
    return sph, lg


@functools.lru_cache(maxsize=None)
def _base_rays(name):
    sph, lg = scene_with_lights(name)
    r = mixed_rays(sph, lg, N_RAYS, 4300 + len(sph))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def rays(name, j, d="scaled"):
    """(N_RAYS, 6) float32, read-only."""
    assert d in ("scaled", "unit")
    r = _base_rays(name).copy()
    r[:, :3] = times(r[:, :3], j)
    if d == "scaled":
        r[:, 3:] = times(r[:, 3:], j)
    r.setflags(write=False)
    return r


# Lane l of every 64 has its direction multiplied by 2^(LANE_EXPONENTS[l] - h),
# h = floor(log2(d.d) / 2) of the ray itself, so that a = d.d lands in
# [2^2E, 2^(2E + 2)) whatever the ray's own length was (a zero, NaN or infinite
# a keeps h = 0).  The quotient's den = 2 a is then in
#   E = -31: [2^-61, 2^-59)  both sides of the range test's 2^-60, within a binade
#   E =  29: [2^59, 2^61)    both sides of its 2^60, within a binade
#   E = -30, 30, -33, 32:    the binades next to those, inside and outside
#   E =   0: [2, 8)          the ordinary lane
#   E = -63, -70:            a = d.d at the least normal floats and subnormal: den is
#                            below the reciprocal's 2^-125, and against a scene
#                            x 2^-60 such a ray still has roots inside the window
#                            of 1e-5 to 1000, whose quotients are divisions of
#                            subnormal operands
#   E = -45, -52:            below the range; the radicand b b - 4 a cc, of order
#                            2^(2 E + 2 j) against a scene x 2^j, falls below the
#                            square root's 2^-96 for j up to -12 (while E = 0 keeps
#                            it above for j down to -40, and E = 29 for -60)
# The table is the list below taken with a stride of 37 lanes, so that every
# quarter of a wave holds every kind.
_KINDS = [-31] * 8 + [29] * 8 + [0] * 28 + [-63] * 3 + [-70] * 2 + [-30] * 4 + [30] * 3 + [-33] * 2 + [32] * 2 \
    + [-45] * 2 + [-52] * 2
LANE_EXPONENTS = tuple(_KINDS[(l * 37) % 64] for l in range(64))
assert sorted(LANE_EXPONENTS) == sorted(_KINDS)


@functools.lru_cache(maxsize=None)
def laned(name, j):
    """(N_RAYS, 6) float32, read-only; laned_facts() states what each wave holds."""
    r = rays(name, j, "unit").copy()
    a = (den32(r) * F(0.5)).astype(np.float64)
    ok = np.isfinite(a) & (a > 0)
    h = np.zeros(len(r), np.int64)
    h[ok] = np.floor(np.log2(a[ok]) / 2).astype(np.int64)
    e = np.asarray(LANE_EXPONENTS)[np.arange(len(r)) % 64] - h
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for step in (np.clip(e, -100, 100), e - np.clip(e, -100, 100)):  # each a float32 factor
            r[:, 3:] = (r[:, 3:] * np.ldexp(1.0, step).astype(F)[:, None]).astype(F)
    r.setflags(write=False)
    return r


def den32(r):
    """2 (d.d) of every ray in float32, as make_query forms it."""
    d = np.asarray(r, F)[:, 3:]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return F(2) * a


def radicands32(sph, r):
    """(rays, spheres) float32 radicands b b - 4 a cc as ray_sphere forms them."""
    r = np.asarray(r, F)
    o, d = r[:, None, :3], r[:, None, 3:]
    c = sph["pos"].astype(F)[None]
    rad = sph["radius"].astype(F)
    with np.errstate(all="ignore"):
        disp = o - c
        a = (r[:, 3] * r[:, 3] + r[:, 4] * r[:, 4]) + r[:, 5] * r[:, 5]
        b = F(2) * ((d[..., 0] * disp[..., 0] + d[..., 1] * disp[..., 1]) + d[..., 2] * disp[..., 2])
        cc = ((disp[..., 0] * disp[..., 0] + disp[..., 1] * disp[..., 1])
              + disp[..., 2] * disp[..., 2]) - (rad * rad)[None]
        out = b * b - (F(4) * a)[:, None] * cc
    assert out.dtype == F
    return out


def laned_facts(name, j):
    """Of laned(name, j), in float32 as the kernel computes a and den = 2 a:
    the least count over the waves of lanes with den in (0, 2^-60), in
    [2^-60, 2^60], in (2^60, inf), in [2^-61, 2^-59) and in (2^59, 2^61]; of
    the whole batch the lanes in [2^-61, 2^-60), [2^-60, 2^-59), (2^59, 2^60]
    and (2^60, 2^61]; and the number of radicands (of the first 512 rays
    against every sphere) in (0, 2^-96) and in [2^-96, inf)."""
    r = laned(name, j)
    den = den32(r).astype(np.float64).reshape(-1, 64)
    lo, hi = 2.0 ** -60, 2.0 ** 60
    waves = [(den > 0) & (den < lo), (den >= lo) & (den <= hi), (den > hi) & np.isfinite(den),
             (den >= lo / 2) & (den < 2 * lo), (den > hi / 2) & (den <= 2 * hi)]
    sides = [(den >= lo / 2) & (den < lo), (den >= lo) & (den < 2 * lo),
             (den > hi / 2) & (den <= hi), (den > hi) & (den <= 2 * hi)]
    rad = radicands32(scene(name, j)[0], r[:512]).astype(np.float64)
    return ([int(s.sum(1).min()) for s in waves], [int(s.sum()) for s in sides],
            (int(((rad > 0) & (rad < 2.0 ** -96)).sum()), int((rad >= 2.0 ** -96).sum())))


@functools.lru_cache(maxsize=None)
def want_hits(name, j, d="scaled"):
    """intersect_host(walk 0) of rays(name, j, d), read-only."""
    import rtg_amd as R
    h = R.intersect_host(scene(name, j)[0], _batch(name, j, d), walk=0, threads=THREADS)
    h.setflags(write=False)
    return h


def _batch(name, j, d):
    return laned(name, j) if d == "laned" else rays(name, j, d)


@functools.lru_cache(maxsize=None)
def want_colours(name, j, d="scaled", sem=0):
    """raytrace_host(walk 0, S = 6) of the batch, read-only."""
    import rtg_amd as R
    sph, lg = scene(name, j)
    c = R.raytrace_host(sph, lg, _batch(name, j, d), stack_size=STACK, semantics=sem, walk=0,
                        threads=THREADS)
    c.setflags(write=False)
    return c


def segments_of(r, h, j):
    """The segments of a batch and its walk-0 records, in float32.  Record k
    with a hit gives, by k % 16,
      0: (o, o + 2 t d)           ends behind the hit
      8: (o, o + t d / 2)         ends before it
      the others: (P + L s e, P - L s e), through the hit point P along the axis
            e of P's smallest component, from the side s the normal points to, L = 2^-10
            against a scene scaled down (j < 0) and 512 against one scaled up
            (coordinates near 2^32 are 512 apart, and t stays below 1000: at j = 30
            only the smallest component of a point is still that fine)
    and a miss gives (o, o + d).  rtg_visible normalises b - a and keeps the
    reference's window of 1e-5 to 1000 in world units, so the first two kinds
    are blocked or clear by the hit only while the scene is of order 1; the
    third keeps its hit L from a at every scale (against a scene far smaller
    than L it is the exact case a = L e, disp = a, radicand 0, t = L)."""
    r = np.asarray(r, F)
    o, d = r[:, :3], r[:, 3:]
    n = len(r)
    hit = h["id"] >= 0
    k = np.arange(n)
    with np.errstate(all="ignore"):
        f = np.where(hit, np.where(k % 16 == 0, F(2), F(0.5)) * h["t"].astype(F), F(1)).astype(F)
        out = np.concatenate([o, (o + f[:, None] * d).astype(F)], axis=1).astype(F)
        L = F(2.0 ** -10 if j < 0 else 512.0)
        P, N = h["point"].astype(F), h["normal"].astype(F)
        axis = np.argmin(np.abs(np.nan_to_num(P)), axis=1)
        s = np.where(np.signbit(N[k, axis]), -L, L).astype(F)
        step = np.zeros((n, 3), F)
        step[k, axis] = s
        thru = hit & (k % 8 != 0)
        out[thru, :3] = (P + step)[thru]
        out[thru, 3:] = (P - step)[thru]
    return out


@functools.lru_cache(maxsize=None)
def segments(name, j, d="scaled"):
    """(N_RAYS, 6) float32 end points, read-only."""
    s = segments_of(_batch(name, j, d), want_hits(name, j, d), j)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def want_visible(name, j, d="scaled"):
    import rtg_amd as R
    v = R.visible_host(scene(name, j)[0], segments(name, j, d), walk=0, threads=THREADS)
    v.setflags(write=False)
    return v


def batch_facts(name, j, d):
    """(hit share, non-zero colour share, blocked share of the segments built
    on hits) of the walk-0 answers."""
    h, c, v = want_hits(name, j, d), want_colours(name, j, d), want_visible(name, j, d)
    return (float((h["id"] >= 0).mean()), float((np.nan_to_num(c) != 0).any(1).mean()),
            float((v == 0).mean()))


# ---- hit records of the fused passes ----

@functools.lru_cache(maxsize=None)
def hits(name, j, d="scaled"):
    """The first N_POINTS walk-0 records of the batch, read-only."""
    h = want_hits(name, j, d)[:N_POINTS].copy()
    h.setflags(write=False)
    return h


def _radius_unit(name):
    return np.abs(scene_with_lights(name)[0]["radius"].astype(np.float64)).max()


def ao_params(R, name, j, flags=0):
    """K = 7 of 8 directions, probe length 2.5 largest radii and bias 1e-3, both x 2^j."""
    return R.ao_params(AO_K, float(times(F(2.5 * _radius_unit(name)), j)),
                       float(times(F(aogen.BIAS), j)), aogen.SEED, flags)


def gather_params(R, name, j, flags=0):
    return R.gather_params(GATHER_K, float(times(F(1e-3), j)), aogen.SEED, flags)


@functools.lru_cache(maxsize=None)
def want_ao(name, j, d="scaled", flags=0):
    import rtg_amd as R
    out = R.ao_host(scene(name, j)[0], hits(name, j, d), aogen.dirs(AO_DIRS), ao_params(R, name, j, flags),
                    walk=0, threads=THREADS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_matte(name, j, d="scaled"):
    """(sums, masks) of matte_host(walk 0), read-only."""
    import rtg_amd as R
    sph, lg = scene(name, j)
    out, lit = R.matte_host(sph, lg, hits(name, j, d), walk=0, threads=THREADS, mask=True)
    out.setflags(write=False)
    lit.setflags(write=False)
    return out, lit


@functools.lru_cache(maxsize=None)
def want_gather(name, j, d="scaled", flags=0):
    """(sums, skipped) of gather_host(walk 0, S = 6), read-only."""
    import rtg_amd as R
    sph, lg = scene(name, j)
    out, skp = R.gather_host(sph, lg, hits(name, j, d), aogen.dirs(GATHER_DIRS),
                             gathergen.weights(GATHER_DIRS), gather_params(R, name, j, flags),
                             stack_size=STACK, walk=0, threads=THREADS, skipped=True)
    out.setflags(write=False)
    skp.setflags(write=False)
    return out, skp


@functools.lru_cache(maxsize=None)
def points(name, j, d="scaled"):
    """(N_RAYS, 3) float32 containment points: the origins of the batch and,
    for every second hit, the hit point."""
    h = want_hits(name, j, d)
    p = _batch(name, j, d)[:, :3].copy()
    at = np.flatnonzero(h["id"] >= 0)[::2]
    p[at] = h["point"][at]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want_contains(name, j, d="scaled"):
    import rtg_amd as R
    out = R.contains_host(scene(name, j)[0], points(name, j, d), walk=0, threads=THREADS)
    out.setflags(write=False)
    return out


# ---- frames ----

@functools.lru_cache(maxsize=None)
def _oracle():
    from conftest import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def want_frame(name, j, sem=0):
    """The oracle's 48 x 36 frame at aa 2, S = 6, of scene(name, j), read-only;
    sem 1: the OpenCL kernel's semantics."""
    o = _oracle()
    sph, lg = (a.copy() for a in scene(name, j))
    fb = (o.render_cl if sem else o.render)(sph, lg, FRAME_W, FRAME_H, FRAME_S, aa=FRAME_AA)
    fb.setflags(write=False)
    return fb


def lit_share(fb):
    return float((np.nan_to_num(fb) != 0).any(-1).mean())


# ---- the frame passes' signals ----

def signal(name, W, H, kind, k):
    """filtergen.signal x 2^k (counts stay as they are)."""
    s = G.signal(name, W, H, kind)
    return s if kind == "count" else times(s, k)


def var_field(name, W, H, k):
    return times(times(svgfgen.var_field(name, W, H), k), k)


def state(name, W, H, kind, k):
    """svgfgen.state's (acc x 2^k, m2 x 2^2k)."""
    acc, m2 = svgfgen.state(name, W, H, kind)
    return times(acc, k), times(times(m2, k), k)


def prev(name, W, H, kind, signal_kind, st, k):
    """accumgen.prev with prevAcc x 2^k and prevM2 x 2^2k."""
    pv = accumgen.prev(name, W, H, kind, signal_kind, st)
    if pv is None:
        return None
    cam, h, acc, ln, m2 = pv
    return cam, h, times(acc, k), ln, None if m2 is None else times(times(m2, k), k)


# ---- poses and points ----

def scaled_pose(cam, j):
    """A CAMERA_DTYPE record or (4, 3) floats with the eye x 2^j."""
    c = np.array(cam, copy=True)
    if c.dtype.names:
        c["eye"] = times(c["eye"], j)
    else:
        c[0] = times(c[0], j)
    return c


def project_points(name, j):
    """The hit points of filtergen's 67 x 35 guides x 2^j, the first the eye itself."""
    pts = times(G.guides(name, *G.FULL)["point"].astype(F), j)
    pts[0] = scaled_pose(accumgen.pose(name, "same"), j)["eye"]
    return pts


# ---- rtg_views_fold*: frames and weights ----

FOLD_SHAPE = (6, 9, 9, 9)  # views (one group of six), H, W, K


@functools.lru_cache(maxsize=None)
def fold_inputs(k):
    """(frames (12, 9, 9, 3), weights x 2^k (6, 9, 9, 9)): two groups of
    test_views_fold_host's random frames and weights, read-only."""
    from test_views_fold_host import random_frames, random_weights
    rng = np.random.default_rng(5150)
    G_, H, W, K = FOLD_SHAPE
    fr = random_frames(rng, 2 * G_, W, H)
    w = times(random_weights(rng, G_, W, H, K), k)
    fr.setflags(write=False)
    w.setflags(write=False)
    return fr, w


# ---- the frame passes' host answers (each pinned to its restatement in test_scale_host.py) ----

FILTER_SETS = [(2, G.ALL, 3, None), (5, 0, 0, 0.0), (2, G.SKIP | G.PLANE, 0, None), (1, G.NORMAL, 8, 0.0)]
VAR_SETS = [(G.ALL, 3, None, 4), (0, 0, 0.0, 4), (G.SKIP, 0, 0.0, 65535)]
VAR_FIELDS = ("seeded", "zero")
SVGF_SETS = [(2, G.ALL, 3, None, True, 4.0, 1e-6), (5, 0, 0, 0.0, True, 4.0, 1e-6),
             (2, G.SAME_ID, 0, 0.0, True, 0.0, 0.0), (2, G.ALL, 3, None, False, 4.0, 1e-6)]
ACCUM_CASES = [("pan", accumgen.SETS[0]), ("roll", accumgen.SETS[2]), ("same", accumgen.SETS[4]),
               ("dolly", accumgen.SETS[8])]
assert all(st[4] for _, st in ACCUM_CASES)  # every one with M2
PASS_SIGNALS = ("rgb", "gray")


def _w(a):
    out = np.ascontiguousarray(a, F).view(np.uint32).reshape(-1)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_filter(name, W, H, kind, st, k):
    import rtg_amd as R
    return _w(R.filter_host(G.guides(name, W, H), W, H, G.params(R, name, kind, st),
                            signal(name, W, H, kind, k), threads=THREADS))


@functools.lru_cache(maxsize=None)
def want_variance(name, W, H, kind, which, st, k):
    import rtg_amd as R
    acc, m2 = state(name, W, H, kind, k)
    return _w(R.variance_host(G.guides(name, W, H), W, H, svgfgen.variance_params(R, name, kind, st),
                              acc, m2, svgfgen.len_field(name, W, H, which), threads=THREADS))


@functools.lru_cache(maxsize=None)
def want_svgf(name, W, H, kind, st, k):
    import rtg_amd as R
    v, dv = R.svgf_host(G.guides(name, W, H), W, H, svgfgen.svgf_params(R, name, kind, st),
                        signal(name, W, H, kind, k), var_field(name, W, H, k), threads=THREADS)
    return _w(v), _w(dv)


@functools.lru_cache(maxsize=None)
def want_accumulate(name, W, H, kind, pk, st, k):
    """(acc words, len, m2 words), with M2."""
    import rtg_amd as R
    out = R.accumulate_host(G.guides(name, W, H), W, H, accumgen.params(R, name, kind, st),
                            signal(name, W, H, kind, k), prev(name, W, H, pk, kind, st, k),
                            zoom=accumgen.ZOOM, m2=True, threads=THREADS)
    ln = out[1].reshape(-1)
    ln.setflags(write=False)
    return _w(out[0]), ln, _w(out[2])


@functools.lru_cache(maxsize=None)
def want_fold(k, flags):
    """(words (2, 9, 3), counts) of fold_inputs(k)."""
    import rtg_amd as R
    fr, w = fold_inputs(k)
    G_, _, _, K = FOLD_SHAPE
    out, cnt = R.views_fold_host(fr, w, R.fold_params(G_, K, flags), threads=THREADS, skipped=True)
    return _w(out), cnt
