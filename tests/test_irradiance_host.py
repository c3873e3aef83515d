"""CPU tests of the probe grid's lookup (rtg_irradiance*, rtg_probe_grid_points,
rtg_probe_grid_poses, include/rtg.h): no GPU.  Every comparison of the defined
arithmetic is on words with NaN canonicalised, bit for bit.

  1. the definition: irradiance_host(walk 0) equals a numpy float32
     restatement, one operation a line, with the lines of sight taken from
     visible_host(walk 0) over the n x 8 segments (A, X_p): colours and weights,
     on every scene, grid, band count and subset of the three flags;
  2. the kernel's own path (walk 1) equals the plain loops (walk 0);
  3. non-vacuity, on the walk-0 answers alone;
  4. the conventions against the bake: a cube of 0.5 + 0.5 d.y folded by
     views_fold_host and cube_sh_weights, looked up on a 1 x 1 x 1 grid;
  5. a coefficient that is linear in the probe position comes back linear;
  6. probe_grid_points and probe_grid_poses;
  7. argument checks; 8. thread independence; the empty batch.

Scenes, records, grids, tables and the plain-loop answers are irrgen.py's;
test_gpu_irradiance.py holds the device to the same answers.
"""
from __future__ import annotations

import numpy as np
import pytest

import irrgen as G
from irrgen import BANDS, BIAS, FLAG_SETS, GRIDS, N_POINTS, SCENES, SIZES
from test_raytrace_host import THREADS

PAD = 64
FILL32 = 0x5A5A5A5A
WITH_SPHERES = [s for s in SCENES if s != "none"]
U = 2.0 ** -24  # one rounding to float, relative


def _raw(rtg, sph, h, n, g, coef, valid, p, walk, threads=THREADS, weight=True):
    """rtg_irradiance_host on the first n records into pre-filled destinations
    PAD records longer than the result; the tails must stay."""
    sph = np.ascontiguousarray(sph, rtg.SPHERE_DTYPE)
    h = np.ascontiguousarray(h, rtg.HIT_DTYPE)
    out = np.full((n + PAD) * 3, FILL32, np.uint32)
    w = np.full(n + PAD, FILL32, np.uint32)
    rc = rtg.lib().rtg_irradiance_host(rtg._ptr(sph), len(sph), rtg._ptr(h), n, rtg._ptr(g),
                                       rtg._ptr(coef), rtg._ptr(valid), rtg._ptr(p), rtg._ptr(out),
                                       rtg._ptr(w) if weight else None, walk, threads)
    assert rc == 0, rtg.lib().rtg_last_error()
    assert (out[3 * n:] == FILL32).all(), "colours past the batch were written"
    assert (w[n:] == FILL32).all(), "weights past the batch were written"
    if not weight:
        assert (w == FILL32).all(), "weights were written without a weight buffer"
    return out[:3 * n].view(np.float32).reshape(n, 3), w[:n].view(np.float32)


def _sight(rtg, name, kind):
    """visible_host(walk 0) over the n x 8 segments of hits(name): (n, 8)."""
    h = G.hits(name)
    seg = G.segments(h, G.grid(name, kind), BIAS)
    return rtg.visible_host(G.scene(name), seg, walk=0, threads=THREADS).reshape(len(h), 8)


# ---- 1. the definition ----

@pytest.mark.parametrize("name", SCENES)
def test_plain_loops_equal_the_numpy_restatement(rtg, name):
    h = G.hits(name)
    for kind in GRIDS:
        vis = _sight(rtg, name, kind)
        for bands in BANDS:
            g, coef = G.grid(name, kind, bands), G.coeffs(name, kind, bands)
            for flags in FLAG_SETS:
                out, w = G.want(name, kind, bands, flags)
                col, wgt, _ = G.restate(h, g, coef, G.valid(name, kind), G.LOBE, BIAS, flags, vis)
                where = (kind, bands, flags)
                assert G.same_words(out, col) is None, (where, G.same_words(out, col))
                assert G.same_words(w, wgt) is None, (where, G.same_words(w, wgt))
                assert not out[h["id"] < 0].view(np.uint32).any(), where
                assert not w[h["id"] < 0].view(np.uint32).any(), where  # +0.f, not -0.f


def test_batches_hold_what_they_should(rtg):
    """The hand-made records, the weight-0 corners, the special coefficient
    words, and a NaN coefficient that reaches an output."""
    for name in SCENES:
        h, g = G.hits(name), G.grid(name)
        assert h[1]["id"] == -1 and np.isnan(h[1]["point"]).all()
        assert tuple(h[4]["normal"]) == (0.5, 2.0, -0.25)
        assert h[G.mattegen.BIG_ID_AT]["id"] == 1 << 30
        _, _, w, _ = G.corners(h, g, BIAS)
        assert (w[G.ON_PLANE] == 0).sum() == 4 and (w[G.ON_PLANE] > 0).sum() == 4, w[G.ON_PLANE]
        for at in G.OUTSIDE:  # clamped to a face of the lattice: four corners left
            assert (w[at] > 0).sum() == 4 and (w[at] == 0).sum() == 4, (at, w[at])
        assert np.isnan(h[G.NAN_POINT]["point"][0]) and h[G.NAN_POINT]["id"] >= 0
        assert (w[G.NAN_POINT] > 0).sum() == 4  # NaN goes to plane 0 of x
        for kind in GRIDS:
            c = G.coeffs(name, kind, 3).reshape(-1)
            assert np.isnan(c).sum() == 1 and np.isinf(c).sum() == 1
            assert (np.signbit(c) & (c == 0)).sum() == 1
            v = G.valid(name, kind)
            assert len(v) == 1 or 0.1 < float((v == 0).mean()) < 0.45, float((v == 0).mean())
        out, _ = G.want(name, "lattice", 3, 0)
        assert np.isnan(out).any() and np.isfinite(out).any(), name
        flat = G.grid(name, "flat")
        assert flat["ny"][0] == 1 and G.grid(name, "one")["nx"][0] == 1
        _, p, w, _ = G.corners(h, flat, BIAS)
        assert (w[:, [2, 3, 6, 7]] == 0).all()  # the second corner along y is never fetched


# ---- 2. walk 1 == walk 0 ----

@pytest.mark.parametrize("name", SCENES)
def test_kernel_path_equals_plain_loops(rtg, name):
    sph, h = G.scene(name), G.hits(name)
    for kind in GRIDS:
        for bands in BANDS:
            g, coef = G.grid(name, kind, bands), G.coeffs(name, kind, bands)
            for flags in FLAG_SETS:
                want, want_w = G.want(name, kind, bands, flags)
                p = G.params(rtg, flags)
                sizes = SIZES if (kind, bands) == ("lattice", 3) else (N_POINTS,)
                for n in sizes:
                    got, w = _raw(rtg, sph, h, n, g, coef, G.valid(name, kind), p, walk=1)
                    where = (kind, bands, flags, n)
                    assert G.same_words(got, want[:n]) is None, (where,
                                                                 G.same_words(got, want[:n]))
                    assert G.same_words(w, want_w[:n]) is None, where
        got, _ = _raw(rtg, sph, h, N_POINTS, G.grid(name), G.coeffs(name, "lattice", 3),
                      G.valid(name, "lattice"), G.params(rtg, 7), walk=1, weight=False)
        assert G.same_words(got, G.want(name, "lattice", 3, 7)[0]) is None, "no weight buffer"


# ---- 3. non-vacuity, on the walk-0 answers ----

@pytest.mark.parametrize("name", WITH_SPHERES)
def test_plain_loop_answers_are_not_vacuous(rtg, name):
    """With RTG_IRR_VISIBLE alone the share of positive-weight (point, corner)
    pairs that visible_host(walk 0) reports blocked lies in [0.1, 0.9], and some
    point has W = 0.  Some point keeps all eight corners under RTG_IRR_VALID
    alone and under no flag; under RTG_IRR_VISIBLE no surface point can: a plane
    through a point strictly inside its cell has corners on both sides, and the
    segment to a corner behind the tangent plane enters the point's own sphere
    (the bias of 1e-3 clears it only within about sqrt(2 bias / r) of the
    plane), which the test states as a condition too."""
    h, g = G.hits(name), G.grid(name)
    real = h["id"] >= 0
    vis = _sight(rtg, name, "lattice")
    _, _, w, _ = G.corners(h, g, BIAS)
    pairs = (w > 0) & real[:, None]
    share = float((vis[pairs] == 0).mean())
    assert 0.1 <= share <= 0.9, share
    coef, valid = G.coeffs(name, "lattice", 3), G.valid(name, "lattice")
    _, W, kept = G.restate(h, g, coef, valid, G.LOBE, BIAS, G.VISIBLE, vis)
    assert G.same_words(W, G.want(name, "lattice", 3, G.VISIBLE)[1]) is None
    assert ((W == 0) & real).any() and ((W > 0) & real).any()
    assert not (kept.sum(1) == 8).any()
    for flags in (0, G.VALID):
        _, W, kept = G.restate(h, g, coef, valid, G.LOBE, BIAS, flags, vis)
        assert (kept.sum(1) == 8).any(), flags
    assert (kept.sum(1)[real] < 8).any()  # VALID leaves some corner out somewhere
    _, W, kept = G.restate(h, g, coef, valid, G.LOBE, BIAS, 7, vis)
    assert ((W == 0) & real).any() and ((W > 0) & real).any()
    # every flag changes the answer
    base = G.want(name, "lattice", 3, 0)[1]
    for flag in (G.VALID, G.FACING, G.VISIBLE):
        assert G.same_words(G.want(name, "lattice", 3, flag)[1], base) is not None, flag


# ---- 4. the conventions against the bake ----

def _baked_probe(rtg):
    """SH9 of the radiance 0.5 + 0.5 d.y around the origin: six 16 x 16 faces of
    camera_cube, directions from camera_rays_host, folded by views_fold_host."""
    res = 16
    frames = np.zeros((6, res, res, 3), np.float32)
    for f, cam in enumerate(rtg.camera_cube((0.0, 0.0, 0.0))):
        rays = rtg.camera_rays_host(cam, res, res, zoom=-1.0, alias_factor=1.0, threads=THREADS)
        d = rays[:, 3:].astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        frames[f] = (0.5 + 0.5 * d[:, 1]).astype(np.float32).reshape(res, res, 1)
    return rtg.views_fold_host(frames, rtg.cube_sh_weights(res, 3), rtg.fold_params(6, 9),
                               threads=THREADS)[0]


def _sh64(N, lobe):
    x, y, z = (float(v) for v in N)
    Y = [G.C0, G.C1 * y, G.C1 * z, G.C1 * x, G.C2 * (x * y), G.C2 * (y * z),
         G.C3 * (3.0 * (z * z) - 1.0), G.C2 * (x * z), G.C4 * (x * x - y * y)]
    band = (0, 1, 1, 1, 2, 2, 2, 2, 2)
    return np.array([float(np.float32(lobe[band[k]])) * Y[k] for k in range(9)])


def test_conventions_against_the_bake(rtg):
    """The looked-up value against a float64 evaluation of the same nine
    polynomials on the same coefficients, within 32 * 2^-24 of the largest
    |term|.  The count for the six axis normals used here: N's components are
    0 or +-1, so c * N, the squares and 3 z z - 1 are exact; a term then has the
    constant's rounding, at most two for the lobe factor's product and one for
    b_k * coefficient (4), at most four terms are not zero (16), their three
    sums round partial sums of at most 2, 3 and 4 terms (9), and w = W = 1: 25
    roundings of at most the largest |term| each."""
    coef = _baked_probe(rtg)
    assert coef.shape == (9, 3)
    g = rtg.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), 3)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
                    np.float32)
    h = np.zeros(len(axes), rtg.HIT_DTYPE)
    h["point"] = (0.25, -0.5, 0.125)
    h["normal"] = axes
    got = {}
    for label, lobe in (("radiance", rtg.IRR_LOBE_RADIANCE), ("cosine", rtg.IRR_LOBE_COSINE)):
        out, w = rtg.irradiance_host(np.zeros(0, rtg.SPHERE_DTYPE), h, g, coef,
                                     rtg.irradiance_params(BIAS, lobe, 0), walk=0, weight=True)
        assert (w == 1).all()
        for i, N in enumerate(axes):
            terms = _sh64(N, lobe)[:, None] * coef.astype(np.float64)  # (9, 3)
            bound = 32 * U * np.abs(terms).max()
            assert (np.abs(out[i].astype(np.float64) - terms.sum(0)) <= bound).all(), (label, i)
        got[label] = out[:, 0].astype(np.float64)
    px, nx, py, ny = (got["radiance"][k] for k in range(4))
    assert py - ny > 0.5 and abs(px - nx) < 0.05, (py, ny, px, nx)  # ideal: 1 and 0
    assert 0 < got["cosine"][2] - got["cosine"][3] < py - ny


# ---- 5. a linear field comes back linear ----

def test_linear_coefficients_interpolate_exactly(rtg):
    """Band 0 of probe p holds L(X_p) = 1 + 0.01 (q + 1) u . X_p per channel q;
    trilinear weights reproduce a linear function, so a point inside the grid
    gets c0 L(A) up to rounding: within 32 * 2^-24 of the largest |b0 c_p| of
    its corners.  The count (bias 0, so A = P): A - o and / step move f by at
    most 2 * 2^-24 g, g < 4, which moves L by less than 3 axes x 0.03 x 0.8 x
    8 * 2^-24 < 0.6 * 2^-24, under 3 roundings of a term of at least 0.28; 1 - f
    and the two products of w (3); c_p's rounding, c0's and their product (3);
    w * e (1); the eight sums of acc and of W, whose partial sums stay below the
    largest term and below 1 (8 + 8); the division (1): 27."""
    g = rtg.probe_grid((-1.0, 0.5, -2.0), (0.75, 1.25, 0.5), (4, 3, 5), 1)
    X = rtg.probe_grid_points(g).astype(np.float64)
    u = np.array([0.6, -0.64, 0.48])
    slope = 0.01 * np.arange(1, 4)
    coef = (1.0 + (X @ u)[:, None] * slope[None, :]).astype(np.float32)
    rng = np.random.default_rng(11)
    lo, span = np.array([-1.0, 0.5, -2.0]), np.array([0.75, 1.25, 0.5]) * (3, 2, 4)
    h = np.zeros(300, rtg.HIT_DTYPE)
    h["point"] = lo + span * rng.uniform(0.01, 0.99, size=(300, 3))
    h["normal"] = (0.0, 0.0, 1.0)
    out, w = rtg.irradiance_host(np.zeros(0, rtg.SPHERE_DTYPE), h, g, coef,
                                 rtg.irradiance_params(0.0, rtg.IRR_LOBE_RADIANCE, 0), walk=0,
                                 weight=True)
    A = h["point"].astype(np.float64)
    want = G.C0 * (1.0 + (A @ u)[:, None] * slope[None, :])
    bound = 32 * U * G.C0 * np.abs(coef).max()
    err = np.abs(out.astype(np.float64) - want).max()
    assert err <= bound, (err, bound)
    assert np.abs(w.astype(np.float64) - 1).max() <= 8 * U
    assert np.ptp(want[:, 2]) > 1000 * bound  # the field is not flat at this precision


# ---- 6. the two conveniences ----

def test_probe_grid_points_and_poses(rtg):
    for g in (G.grid("reference"), G.grid("c5", "flat", 2), G.grid(40, "one", 1),
              rtg.probe_grid((0.1, -7.3, 1e3), (0.3, 1e-3, 17.0), (5, 2, 3), 3)):
        nx, ny, nz = int(g["nx"][0]), int(g["ny"][0]), int(g["nz"][0])
        o, s = g["origin"][0], g["step"][0]
        pts = rtg.probe_grid_points(g)
        assert pts.shape == (nx * ny * nz, 3)
        iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        for q, i in enumerate((ix, iy, iz)):
            along = i.reshape(-1).astype(np.float32) * s[q]
            want = o[q] + along
            assert want.dtype == np.float32 and pts[:, q].tobytes() == want.tobytes(), q
        poses = rtg.probe_grid_poses(g)
        assert poses.shape == (6 * len(pts),)
        for p in (0, len(pts) // 2, len(pts) - 1):
            assert poses[6 * p:6 * p + 6].tobytes() == rtg.camera_cube(pts[p]).tobytes(), p


# ---- 7. argument checks ----

def test_argument_errors(rtg):
    L = rtg.lib()
    P = rtg._ptr
    name = "reference"
    sph, h = G.scene(name), G.hits(name).copy()
    g0, coef, valid = G.grid(name).copy(), G.coeffs(name, "lattice", 3).copy(), \
        G.valid(name, "lattice").copy()
    p0 = G.params(rtg, 7)
    out = np.zeros((len(h), 3), np.float32)
    wgt = np.zeros(len(h), np.float32)
    NONE = object()

    def call(hits=h, n=len(h), grid=g0, c=coef, v=valid, p=p0, dst=out, w=wgt, walk=0,
             spheres=sph):
        ptr = lambda a: None if a is NONE or a is None else P(a)  # noqa: E731
        return L.rtg_irradiance_host(ptr(spheres), len(sph), ptr(hits), n, ptr(grid), ptr(c),
                                     ptr(v), ptr(p), ptr(dst), ptr(w), walk, 1)

    def bad(rc, msg):
        assert rc == -1
        text = L.rtg_last_error().decode()
        assert text.startswith("irradiance: ") and msg in text, text

    def grid_with(**kw):
        g = g0.copy()
        for k, v in kw.items():
            g[k][0] = v
        return g

    def params_with(**kw):
        p = p0.copy()
        for k, v in kw.items():
            p[k][0] = v
        return p

    assert call() == 0 and L.rtg_last_error() == b""
    assert out.any() and wgt.any()
    out[:], wgt[:] = 0, 0
    bad(call(hits=NONE), "null hit buffer")
    bad(call(c=NONE), "null coefficient table")
    bad(call(p=NONE), "null params")
    bad(call(dst=NONE), "null output buffer")
    bad(call(grid=NONE), "null grid")
    bad(call(v=NONE), "RTG_IRR_VALID with a null validity table")
    for step in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, np.nan), (np.inf, 1.0, 1.0)):
        bad(call(grid=grid_with(step=step)), "is not finite and > 0")
    for origin in ((np.nan, 0.0, 0.0), (0.0, -np.inf, 0.0)):
        bad(call(grid=grid_with(origin=origin)), "origin is not finite")
    bad(call(grid=grid_with(nx=0)), "outside [1, 2^20]")
    bad(call(grid=grid_with(nz=(1 << 20) + 1)), "outside [1, 2^20]")
    bad(call(grid=grid_with(nx=1 << 20, ny=1 << 10, nz=1)), "at most 2^31 - 1 in all")  # 9 * 2^30
    bad(call(grid=grid_with(nx=1 << 20, ny=1 << 20, nz=1 << 20)), "at most 2^31 - 1 in all")
    bad(call(grid=grid_with(bands=0)), "0 bands outside [1, 3]")
    bad(call(grid=grid_with(bands=4)), "4 bands outside [1, 3]")
    bad(call(p=params_with(flags=8)), "unknown flag bits 0x8")
    bad(call(p=params_with(flags=0x80000001)), "unknown flag bits 0x80000000")
    bad(call(n=1 << 32), "points (at most 2^32 - 1)")
    bad(call(walk=2), "walk 2")
    bad(call(walk=-1), "walk -1")
    bad(call(spheres=NONE), "null scene array")
    assert call(n=0) == 0
    assert not out.any() and not wgt.any()  # nothing written by a refused call
    assert call(v=NONE, p=params_with(flags=6)) == 0  # no table without RTG_IRR_VALID
    out[:], wgt[:] = 0, 0
    assert call(w=NONE) == 0 and out.any() and not wgt.any()  # the weight is optional
    with pytest.raises(rtg.RtgError, match="walk 3"):
        rtg.irradiance_host(sph, h, g0, coef, p0, valid, walk=3)
    out[:] = 0
    for fn, what in ((L.rtg_probe_grid_points, "probe_grid_points"),
                     (L.rtg_probe_grid_poses, "probe_grid_poses")):
        assert fn(P(g0), None) == -1 and f"{what}: null output".encode() in L.rtg_last_error()
        assert fn(None, P(out)) == -1 and f"{what}: null grid".encode() in L.rtg_last_error()
        assert fn(P(grid_with(ny=0)), P(out)) == -1 and b"outside [1, 2^20]" in L.rtg_last_error()
    assert not out.any()


# ---- 8. threads, the empty batch ----

def test_result_does_not_depend_on_threads(rtg):
    for name in ("reference", "base65"):
        sph, h = G.scene(name), G.hits(name)
        want, want_w = G.want(name, "lattice", 3, 7)
        for walk in (0, 1):
            for threads in (1, 3, 0, -2):
                got, w = rtg.irradiance_host(sph, h, G.grid(name), G.coeffs(name, "lattice", 3),
                                             G.params(rtg, 7), G.valid(name, "lattice"), walk=walk,
                                             threads=threads, weight=True)
                assert G.same_words(got, want) is None and G.same_words(w, want_w) is None


def test_empty_batch(rtg):
    sph = G.scene("reference")
    empty = np.zeros(0, rtg.HIT_DTYPE)
    for walk in (0, 1):
        out, w = rtg.irradiance_host(sph, empty, G.grid("reference"),
                                     G.coeffs("reference", "lattice", 3), G.params(rtg, 7),
                                     G.valid("reference", "lattice"), walk=walk, weight=True)
        assert out.shape == (0, 3) and w.shape == (0,)
