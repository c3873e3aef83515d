"""CPU tests of the host forms on scenes, rays and signals scaled by powers of
two (scalegen.py): what test_gpu_scale.py then holds the device calls to.

  1. the scaled inputs are not vacuous (on the plain loops' and the oracle's
     answers only) and the `laned` batches hold what they are built to hold;
  2. walk 1 (the kernels' traversal and indexing compiled for the host) equals
     walk 0 for every ray and hit-point call on every batch;
  3. the oracle's frame of a scaled scene equals rtg_render_camera_host of the
     identity pose at walk 1, in both semantics;
  4. homogeneity: scene and rays scaled together by 2^j give the same id, t and
     normal words and 2^j times the point (rtg_intersect_host, walk 0), and the
     same visibility where the reference's absolute window allows it;
  5. the frame passes' host loops equal their numpy restatements on signals
     x 2^k, and rtg_filter_host commutes with the scaling where no intermediate
     leaves the normal range.

Everything is compared word for word; NaN words are canonical on both sides.
"""
from __future__ import annotations

import numpy as np
import pytest

import accumgen as A
import aogen
import filtergen as G
import gathergen
import scalegen as X
import svgfgen as S
from conftest import bits_equal, first_mismatch
from raygen import diff_hits
from scalegen import BATCHES, BATCH_IDS, FRAMES, J_LANED, J_POSE, K_SIGNAL, SCENES
from test_camera_host import pose, restate_rays
from test_raytrace_host import THREADS
from test_views_fold_host import restate_fold

F = np.float32
LANED = [(j, "laned") for j in J_LANED]
EVERY_BATCH = BATCHES + LANED
EVERY_ID = BATCH_IDS + [f"j{j}-laned" for j in J_LANED]


def _words(a):
    return np.ascontiguousarray(a, F).view(np.uint32).reshape(-1)


# ---- 1. the inputs ----

@pytest.mark.parametrize("j,d", BATCHES, ids=BATCH_IDS)
@pytest.mark.parametrize("name", SCENES)
def test_batches_are_not_vacuous(rtg, name, j, d):
    """On the plain loops' answers: hit share, non-zero colour share and the
    blocked share of the derived segments."""
    hit, lit, blocked = X.batch_facts(name, j, d)
    assert hit >= X.MIN_HIT and lit >= X.MIN_LIT and blocked >= X.MIN_BLOCKED, (hit, lit, blocked)
    assert blocked <= 0.95  # and some segment is clear


@pytest.mark.parametrize("j", J_LANED)
@pytest.mark.parametrize("name", SCENES)
def test_laned_waves_hold_every_kind(rtg, name, j):
    """Every wave of 64 holds lanes with den = 2 d.d below 2^-60, inside
    [2^-60, 2^60] and above 2^60, and lanes within one binade of either edge;
    the batch holds lanes in each of the four binades next to the edges; the
    lanes outside the range are the minority of every wave; radicands of the
    batch lie above 2^-96 and, against the scenes scaled down, below it too (of
    order 2^(2 E + 2 j), E >= -52 in the table: against a scene scaled up only
    a subnormal d.d would bring one that low)."""
    per_wave, sides, (small, large) = X.laned_facts(name, j)
    assert min(per_wave) >= 1, per_wave
    assert min(sides) >= 16, sides
    assert large > 0 and (small > 0 or j > -12), (small, large)
    fast = X.den32(X.laned(name, j)).reshape(-1, 64)
    fast = (fast >= F(2.0 ** -60)) & (fast <= F(2.0 ** 60))
    assert (fast.sum(1) > 32).all(), "the out-of-range lanes are the minority of every wave"
    # on the plain loops' answer: lanes outside the quotient's range find spheres,
    # and against the scene x 2^-60 so do lanes whose den is below 2^-120
    den = X.den32(X.laned(name, j)).astype(np.float64)
    hit = X.want_hits(name, j, "laned")["id"] >= 0
    assert hit[((den > 0) & (den < 2.0 ** -60)) | ((den > 2.0 ** 60) & np.isfinite(den))].sum() >= 5
    assert j != -60 or hit[(den > 0) & (den < 2.0 ** -120)].sum() >= 20


# ---- 2. walk 1 == walk 0 ----

@pytest.mark.parametrize("j,d", EVERY_BATCH, ids=EVERY_ID)
@pytest.mark.parametrize("name", SCENES)
def test_kernel_path_equals_plain_loops(rtg, name, j, d):
    sph, lg = X.scene(name, j)
    rays, segs = X._batch(name, j, d), X.segments(name, j, d)
    got = rtg.intersect_host(sph, rays, walk=1, threads=THREADS)
    assert diff_hits(got, X.want_hits(name, j, d)) is None, diff_hits(got, X.want_hits(name, j, d))
    for s in (segs, rays):  # the rays taken as segments too, as test_gpu_rays.py does
        vis = rtg.visible_host(sph, s, walk=1, threads=THREADS)
        want = X.want_visible(name, j, d) if s is segs else rtg.visible_host(sph, s, walk=0,
                                                                             threads=THREADS)
        assert vis.tobytes() == want.tobytes(), np.flatnonzero(vis != want)[:4]
    for sem in (0, 1) if j in (-24, 12) else (0,):
        col = rtg.raytrace_host(sph, lg, rays, stack_size=X.STACK, semantics=sem, walk=1,
                                threads=THREADS)
        want = X.want_colours(name, j, d, sem)
        bad = np.flatnonzero((_words(col) != _words(want)).reshape(-1, 3).any(1))
        assert not len(bad), (sem, len(bad), rays[bad[0]], col[bad[0]], want[bad[0]])
    h = X.hits(name, j, d)
    got = rtg.ao_host(sph, h, aogen.dirs(X.AO_DIRS), X.ao_params(rtg, name, j), walk=1,
                      threads=THREADS)
    assert got.tobytes() == X.want_ao(name, j, d).tobytes(), np.flatnonzero(got != X.want_ao(name, j, d))[:4]
    got, lit = rtg.matte_host(sph, lg, h, walk=1, threads=THREADS, mask=True)
    want, want_lit = X.want_matte(name, j, d)
    assert (_words(got) == _words(want)).all() and (lit == want_lit).all()
    got, skp = rtg.gather_host(sph, lg, h, aogen.dirs(X.GATHER_DIRS),
                               gathergen.weights(X.GATHER_DIRS), X.gather_params(rtg, name, j),
                               stack_size=X.STACK, walk=1, threads=THREADS, skipped=True)
    want, want_skp = X.want_gather(name, j, d)
    assert (_words(got) == _words(want)).all() and (skp == want_skp).all()
    got = rtg.contains_host(sph, X.points(name, j, d), walk=1, threads=THREADS)
    assert got.tobytes() == X.want_contains(name, j, d).tobytes()


@pytest.mark.parametrize("name", SCENES)
def test_hit_point_passes_are_not_vacuous(rtg, name):
    """On the walk-0 answers, per scale of the scaled batches: rtg_matte* lights
    some point and rtg_contains* finds a point inside a sphere (an origin of
    raygen.inside).  rtg_ao* probes a segment of 2.5 radii x 2^j with a unit
    direction and rtg_gather* traces unit rays (rtg.h normalises both), so
    under the reference's window of 1e-5 to 1000 in world units they find
    blocked and clear probes and non-zero sums at j = -12 and 12 only; at the
    other scales every probe is clear and every sum is zero on both sides."""
    for j in X.J_SCALED:
        real = X.hits(name, j)["id"] >= 0
        assert real.sum() >= 0.1 * X.N_POINTS
        assert (np.nan_to_num(X.want_matte(name, j)[0]) != 0).any(), j
        assert (X.want_contains(name, j) >= 0).any(), j
        if j in (-12, 12):
            ao = X.want_ao(name, j)[real]
            assert (ao < X.AO_K).any() and (ao > 0).any(), j
            assert (np.nan_to_num(X.want_gather(name, j)[0]) != 0).any(1).sum() >= 20, j


# ---- 3. frames ----

@pytest.mark.parametrize("name,j", FRAMES)
def test_frame_equals_the_oracle(rtg, name, j):
    sph, lg = X.scene(name, j)
    assert X.lit_share(X.want_frame(name, j)) >= X.MIN_FRAME  # on the oracle's frame
    for sem in (0, 1):
        want = X.want_frame(name, j, sem)
        got = rtg.render_camera_host(sph, lg, rtg.camera_identity(), X.FRAME_W, X.FRAME_H,
                                     alias_factor=X.FRAME_AA, stack_size=X.FRAME_S, semantics=sem,
                                     walk=1, threads=THREADS)
        assert bits_equal(got, want), (sem, first_mismatch(got, want))
    g0 = rtg.gbuffer_host(sph, X.FRAME_W, X.FRAME_H, alias_factor=X.FRAME_AA, threads=THREADS)
    assert (g0["id"] >= 0).mean() >= X.MIN_FRAME


# ---- 4. homogeneity of the plain loops ----

HOMOGENEOUS_J = (-24, -12, 12)
# rtg_visible normalises b - a and keeps the window of 1e-5 to 1000 in world
# units, so it is homogeneous only while no root crosses either end of it.
# Tried on the segments of scenes 12, 65 and c5 for j = -24, -12, -6, -3, -2,
# -1, 1, 2, 3, 6, 12: walk 0 alone satisfies it at j = -3, -2 and -1 (no byte
# of 2048 differs) and at no other of them (8 to 129 bytes differ among the
# segments that start at a ray's origin alone: origins 1e5 away have their
# roots near 1000, and a == b and grazing roots lie near 1e-5).
VISIBLE_HOMOGENEOUS_J = (-3, -2, -1)


def _finite(rays):
    return np.isfinite(rays).all(1)


@pytest.mark.parametrize("j", HOMOGENEOUS_J)
@pytest.mark.parametrize("name", [12, 65, "c5"])
def test_intersect_is_homogeneous(rtg, name, j):
    """Scene and rays x 2^j (exact in float32 at these j): the same id, t and
    normal words and 2^j times the point, on every finite ray."""
    keep = _finite(X.rays(name, 0))
    base = X.want_hits(name, 0)[keep]
    got = X.want_hits(name, j)[keep]
    assert (base["id"] >= 0).mean() >= X.MIN_HIT
    assert (got["id"] == base["id"]).all(), np.flatnonzero(got["id"] != base["id"])[:4]
    assert (_words(got["t"]) == _words(base["t"])).all()
    assert (_words(got["normal"]) == _words(base["normal"])).all()
    assert (_words(got["point"]) == _words(X.times(base["point"], j))).all()


@pytest.mark.parametrize("j", VISIBLE_HOMOGENEOUS_J)
@pytest.mark.parametrize("name", [12, 65, "c5"])
def test_visible_is_homogeneous_just_below_one(rtg, name, j):
    segs = X.segments(name, 0)
    keep = np.isfinite(segs).all(1)
    sph = X.scene(name, j)[0]
    got = rtg.visible_host(sph, X.times(segs, j), walk=0, threads=THREADS)
    want = X.want_visible(name, 0)
    assert (got[keep] == want[keep]).all(), int((got[keep] != want[keep]).sum())
    assert (want[keep] == 0).mean() >= X.MIN_BLOCKED


# ---- 5. the frame passes ----

FILTER_SETS, VAR_SETS, SVGF_SETS, ACCUM_CASES = X.FILTER_SETS, X.VAR_SETS, X.SVGF_SETS, X.ACCUM_CASES


def _bad(got, ref):
    bad = np.flatnonzero(got != ref)
    return None if not len(bad) else (len(bad), bad[:4], got[bad[:4]], ref[bad[:4]])


@pytest.mark.parametrize("k", K_SIGNAL)
@pytest.mark.parametrize("name", X.PASS_SCENES)
def test_filter_host_equals_restatement(rtg, name, k):
    for W, H in X.PASS_FRAMES:
        h = G.guides(name, W, H)
        for kind in ("rgb", "gray"):
            src = X.signal(name, W, H, kind, k)
            for st in FILTER_SETS:
                got = X.want_filter(name, W, H, kind, st, k)
                ref = G.restate(h, W, H, st, G.plane_scale(name, st[3]), src)
                assert _bad(got, ref) is None, (W, H, kind, st, _bad(got, ref))


@pytest.mark.parametrize("k", K_SIGNAL)
@pytest.mark.parametrize("name", X.PASS_SCENES)
def test_variance_host_equals_restatement(rtg, name, k):
    for W, H in X.PASS_FRAMES:
        h = G.guides(name, W, H)
        for kind in S.SIGNALS:
            acc, m2 = X.state(name, W, H, kind, k)
            for which in X.VAR_FIELDS:
                ln = S.len_field(name, W, H, which)
                for st in VAR_SETS:
                    got = X.want_variance(name, W, H, kind, which, st, k)
                    ref = S.restate_variance(h, W, H, st, G.plane_scale(name, st[2]), acc, m2, ln)
                    assert _bad(got, ref) is None, (W, H, kind, which, st, _bad(got, ref))


@pytest.mark.parametrize("k", K_SIGNAL)
@pytest.mark.parametrize("name", X.PASS_SCENES)
def test_svgf_host_equals_restatement(rtg, name, k):
    for W, H in X.PASS_FRAMES:
        h, var = G.guides(name, W, H), X.var_field(name, W, H, k)
        for kind in S.SIGNALS:
            src = X.signal(name, W, H, kind, k)
            for st in SVGF_SETS:
                v, dv = X.want_svgf(name, W, H, kind, st, k)
                ref = S.restate_svgf(h, W, H, st, G.plane_scale(name, st[3]), src, var)
                assert _bad(v, ref[0]) is None, (W, H, kind, st, _bad(v, ref[0]))
                assert _bad(dv, ref[1]) is None, (W, H, kind, st, _bad(dv, ref[1]))


@pytest.mark.parametrize("k", K_SIGNAL)
@pytest.mark.parametrize("name", X.PASS_SCENES)
def test_accumulate_host_equals_restatement(rtg, name, k):
    for W, H in X.PASS_FRAMES:
        h = G.guides(name, W, H)
        for kind in ("rgb", "gray"):
            src = X.signal(name, W, H, kind, k)
            for pk, st in ACCUM_CASES:
                pv = X.prev(name, W, H, pk, kind, st, k)
                got = X.want_accumulate(name, W, H, kind, pk, st, k)
                ref = A.restate(h, W, H, st, G.plane_scale(name, st[2]), src, pv)
                for what, g, r in zip(("acc", "len", "m2"), got, ref):
                    assert _bad(g, r) is None, (W, H, kind, pk, st, what, _bad(g, r))


@pytest.mark.parametrize("k", K_SIGNAL)
def test_views_fold_host_equals_restatement(rtg, k):
    fr, w = X.fold_inputs(k)
    G_, _, _, K = X.FOLD_SHAPE
    for flags in (0, 1):
        got, cnt = X.want_fold(k, flags)
        want, wcnt = restate_fold(fr, w, G_, K, bool(flags))
        assert got.tobytes() == want.tobytes(), flags
        assert (cnt == wcnt).all()


@pytest.mark.parametrize("j", J_POSE)
def test_camera_rays_host_equals_restatement(rtg, j):
    for scene in (12, "c5"):
        for name in ("orbit", "raw"):
            cam, zoom = pose(name, scene)
            cam = X.scaled_pose(cam, j)
            got = rtg.camera_rays_host(cam.reshape(-1), 9, 7, zoom=zoom, alias_factor=2.0,
                                       threads=THREADS)
            want, _ = restate_rays(cam, 9, 7, 2.0, zoom)
            assert (_words(got) == aogen.canon(want).reshape(-1)).all(), (scene, name)
            assert np.isfinite(got).all()


@pytest.mark.parametrize("j", J_POSE)
@pytest.mark.parametrize("name", X.PASS_SCENES)
def test_camera_project_host_equals_restatement(rtg, name, j):
    W, H = G.FULL
    pts = X.project_points(name, j)
    for pk in ("same", "pan", "roll"):
        cam = X.scaled_pose(A.pose(name, pk), j)
        got = rtg.camera_project_host(cam, W, H, pts, zoom=A.ZOOM, threads=THREADS)
        ref = np.stack(A.restate_project(cam, W, H, A.ZOOM, pts), -1)
        assert (_words(got) == A.canon(ref).reshape(-1)).all(), pk
        inside = (got[:, 0] >= 0) & (got[:, 0] < W) & (got[:, 1] >= 0) & (got[:, 1] < H)
        assert inside.any() or abs(j) >= 60  # (there the dot products leave the float range)


FILTER_HOMOGENEOUS_K = (-100, -30, 30, 100)


@pytest.mark.parametrize("k", FILTER_HOMOGENEOUS_K)
@pytest.mark.parametrize("name", X.PASS_SCENES)
def test_filter_is_homogeneous(rtg, name, k):
    """rtg_filter_host(2^k v) == 2^k rtg_filter_host(v): every product and sum
    scales exactly while it stays in the normal range, and the quotient acc / sw
    sees the same significands."""
    W, H = G.FULL
    h = G.guides(name, W, H)
    for kind in ("rgb", "gray"):
        for st in FILTER_SETS:
            p = G.params(rtg, name, kind, st)
            base = rtg.filter_host(h, W, H, p, G.signal(name, W, H, kind), threads=THREADS)
            got = rtg.filter_host(h, W, H, p, X.signal(name, W, H, kind, k), threads=THREADS)
            assert _bad(_words(got), _words(X.times(base, k))) is None, (kind, st)
