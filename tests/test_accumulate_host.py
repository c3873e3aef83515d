"""CPU tests of temporal accumulation by reprojection (rtg_accumulate_host,
rtg_camera_project_host; include/rtg.h, "accumulate"): no GPU needed.

  1. accumulate_host == the numpy float32 restatement (accumgen.restate), word
     for word, on every frame, previous pose, signal and parameter set of
     accumgen; camera_project_host == its restatement;
  2. thread counts give the same words;
  3. the projection round trip: a pixel's own hit point lands on the pixel;
  4. a four-frame sequence with maxHistory 3: lengths reach 3 and stop,
     background stays 0, a newly visible pixel starts at 1;
  5. the host chain over three seeds equals the float64 mean of the three
     count frames within the derived bound;
  6. non-vacuity of the inputs (accumgen.facts);
  7. every argument error, with its message.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import accumgen as A
import aogen
import filtergen as G
from accumgen import FRAMES, FULL, SCENES, SIGNALS
from test_raytrace_host import THREADS

F = np.float32


def _words(a):
    return np.ascontiguousarray(a, F).view(np.uint32).reshape(-1)


# ---- 1. the definition ----

@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_host_equals_restatement(rtg, name, kind):
    for W, H in FRAMES:
        h, src = G.guides(name, W, H), G.signal(name, W, H, kind)
        for pk, st in A.cases():
            got = A.want(name, W, H, kind, pk, st)
            ref = A.restate(h, W, H, st, G.plane_scale(name, st[2]), src,
                            A.prev(name, W, H, pk, kind, st))
            for what, g, r in zip(("acc", "len", "m2"), got, ref):
                if g is None:
                    continue
                bad = np.flatnonzero(g != r)
                assert not len(bad), (W, H, pk, st, what, len(bad), bad[:4], g[bad[:4]], r[bad[:4]])


@pytest.mark.parametrize("name", SCENES)
def test_project_equals_restatement(rtg, name):
    W, H = FULL
    pts = G.guides(name, W, H)["point"].astype(F).copy()
    pts[0] = A.pose_args(name, "same")[0]  # the eye itself: d = 0
    assert np.isnan(pts).any()
    for pk in A.PREV_KINDS:
        cam = A.pose(name, pk)
        for (w, h), zoom in (((W, H), A.ZOOM), ((1, 1), -1.0), ((1 << 24, 3), 2.5)):
            got = rtg.camera_project_host(cam, w, h, pts, zoom=zoom, threads=THREADS)
            ref = np.stack(A.restate_project(cam, w, h, zoom, pts), -1)
            assert (_words(got) == A.canon(ref).reshape(-1)).all(), (pk, w, h)


# ---- 2. threads ----

@pytest.mark.parametrize("name", SCENES)
def test_thread_counts_agree(rtg, name):
    W, H = FULL
    for kind in SIGNALS:
        for pk, st in (("pan", A.SETS[0]), ("roll", A.SETS[2])):
            p = A.params(rtg, name, kind, st)
            want = A.want(name, W, H, kind, pk, st)
            for threads in (0, 1, 3, 64):
                got = rtg.accumulate_host(G.guides(name, W, H), W, H, p, G.signal(name, W, H, kind),
                                          A.prev(name, W, H, pk, kind, st), zoom=A.ZOOM, m2=True,
                                          threads=threads)
                assert (_words(got[0]) == want[0]).all() and (got[1].reshape(-1) == want[1]).all()
                assert (_words(got[2]) == want[2]).all(), (kind, pk, threads)
    pts = G.raw_guides(name)["point"].reshape(-1, 3)
    one = rtg.camera_project_host(A.pose(name, "pan"), W, H, pts, zoom=A.ZOOM, threads=1)
    for threads in (0, 3, 64):
        got = rtg.camera_project_host(A.pose(name, "pan"), W, H, pts, zoom=A.ZOOM, threads=threads)
        assert (_words(got) == _words(one)).all()


# ---- 3. the round trip ----

def _round_trip(rtg, name):
    """(largest |fx - x| or |fy - y| over the hits, smallest k) of the unplanted
    67 x 35 records projected into their own pose."""
    W, H = FULL
    h = G.raw_guides(name).reshape(-1)
    hit = h["id"] >= 0
    out = rtg.camera_project_host(A.pose(name, "same"), W, H, h["point"], zoom=A.ZOOM)[hit]
    y, x = np.divmod(np.flatnonzero(hit), W)
    off = np.maximum(np.abs(out[:, 0].astype(np.float64) - x), np.abs(out[:, 1].astype(np.float64) - y))
    return float(off.max()), float(out[:, 2].min())


@pytest.mark.parametrize("name", SCENES)
def test_projection_round_trip(rtg, name):
    """A pixel's own hit point projects to within 1/16 pixel of the pixel, in
    front of the camera: the own pixel then holds more than 0.87 of the
    bilinear weight.  (Measured on the host: 1.9e-5 pixels at most over the
    three scenes)"""
    off, kmin = _round_trip(rtg, name)
    print(f"round trip {name}: max offset {off:.3g} px, min k {kmin:.3g}")
    assert off <= 1.0 / 16 and kmin > 0


def test_pan_is_small(rtg):
    """The pan poses shift the image by a fraction of a pixel to a few pixels."""
    W, H = FULL
    for name in SCENES:
        h = G.raw_guides(name).reshape(-1)
        hit = h["id"] >= 0
        out = rtg.camera_project_host(A.pose(name, "pan"), W, H, h["point"], zoom=A.ZOOM)[hit]
        y, x = np.divmod(np.flatnonzero(hit), W)
        shift = np.hypot(out[:, 0] - x, out[:, 1] - y)
        print(f"pan {name}: shift {shift.min():.3g} .. {shift.max():.3g} px")
        assert 0 < shift.min() and shift.max() < 8 and (out[:, 2] > 0).all()
        assert (shift % 1 > 0.05).any()  # not whole pixels: the bilinear weights matter


# ---- 4. a sequence ----

def test_four_frame_sequence(rtg):
    """Four poses a small pan apart, maxHistory 3, SAME_ID alone: a hit pixel's
    length is 1 exactly when none of its four taps in the previous frame holds
    its id, and otherwise one more than the smallest tap's, capped at 3."""
    name = "c5"
    W, H = FULL
    sph = aogen.scene(name)
    eye, target = (np.array(v, np.float64) for v in G.POSES[name])
    p = rtg.accumulate_params(rtg.FILTER_GRAY, rtg.ACCUM_SAME_ID, max_history=3)
    prev, top, new = None, [], 0
    for i in range(4):
        d = i * np.array((0.3, 0.1, 0.0))
        cam = rtg.camera_look_at(tuple(eye + d), tuple(target + d))
        h = rtg.intersect_host(sph, rtg.camera_rays_host(cam, W, H, alias_factor=1.0), walk=0,
                               threads=THREADS)
        acc, ln = rtg.accumulate_host(h, W, H, p, h["t"].astype(F), prev, zoom=A.ZOOM)
        ln = ln.reshape(-1)
        hit = h["id"] >= 0
        assert (ln[~hit] == 0).all() and (ln[hit] >= 1).all()
        top.append(int(ln.max()))
        if prev is not None:
            fx, fy, k = A.restate_project(prev[0], W, H, A.ZOOM, h["point"].astype(F))
            ok = (k > 0) & (fx > -1) & (fx < W) & (fy > -1) & (fy < H)
            x0, y0 = (np.where(ok, np.floor(v), 0).astype(np.int64) for v in (fx, fy))
            pid = prev[1]["id"].reshape(H, W)
            same = np.zeros(W * H, bool)
            for dy in (0, 1):
                for dx in (0, 1):
                    xq, yq = x0 + dx, y0 + dy
                    w = (fx - x0 if dx else 1 - (fx - x0)) * (fy - y0 if dy else 1 - (fy - y0))
                    inside = ok & (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H) & (w > 0)
                    same |= inside & (pid[np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)] == h["id"])
            assert ((ln == 1) == ~same)[hit].all()
            new = int((hit & ~same & ok).sum())  # on screen before, behind another id
        prev = (cam, h, acc, ln)
    assert top == [1, 2, 3, 3]
    assert new > 0, "no pixel of the last frame appears from behind an edge"


# ---- 5. the host chain ----

def test_host_chain_is_the_mean(rtg):
    """Three frames of jittered AO counts (K = 7) from ONE pose, accumulated with
    SAME_ID | NORMAL | PLANE and maxHistory 65535, against the float64 mean of
    the three count frames on the pixels that end with length 3.

    The bound, from the arithmetic, in u = ulp(K) (the float spacing at K, >=
    K 2^-24) and e = the largest round-trip offset of the RESTATED projection:
      * a lookup returns a convex combination of values in [0, K] in which
        the taps other than the pixel's own weigh at most 2e / (1 - 2e - 2^-18)
        <= 3e of the total (e <= 1/16; the own tap's terms are dot(N, N)^8 >=
        1 - 2^-18 and z = 1 exactly, a neighbour's are <= 1 + 2^-18): it is
        off the pixel's own previous value by at most 3 e K;
      * its weights carry at most 12 roundings each (wy * wx, a dot of 5, 3
        squarings, 2 products, the plane term's), which move a convex
        combination by at most 2 * 12 * 2^-24 K <= 24 u, and the 4 products,
        4 sums and 1 quotient of values <= K add 9 half ulps: 28.5 u a lookup;
      * a blend is one subtraction, one multiply and one add of values <= K,
        1.5 u, and alpha = 1 / 3's own rounding moves it by less than 0.5 u.
    Two lookups and two blends (the first frame is a reset, exact), every error
    passing through later blends with a factor <= 1:
        tol = (2 * 28.5 + 2 * 1.5 + 0.5) u + 2 * 3 e K."""
    name, K = "c5", 7
    W, H = FULL
    sph, table = aogen.scene(name), aogen.dirs(8)
    cam = A.pose(name, "same")
    h = G.raw_guides(name).reshape(-1)
    hit = h["id"] >= 0
    fx, fy, k = A.restate_project(cam, W, H, A.ZOOM, h["point"].astype(F))
    y, x = np.divmod(np.arange(W * H), W)
    e = float(np.maximum(np.abs(fx.astype(np.float64) - x), np.abs(fy.astype(np.float64) - y))[hit].max())
    assert e <= 1.0 / 16 and (k[hit] > 0).all()
    u = float(np.spacing(F(K)))
    tol = (2 * 28.5 + 2 * 1.5 + 0.5) * u + 2 * 3 * e * K
    p = rtg.accumulate_params(rtg.FILTER_COUNT, rtg.ACCUM_SAME_ID | rtg.ACCUM_NORMAL | rtg.ACCUM_PLANE,
                              G.plane_scale(name, None), 3, 65535)
    prev, frames = None, []
    for seed in (aogen.SEED, aogen.SEED + 1, aogen.SEED + 2):
        ap = rtg.ao_params(K, aogen.radius(name), aogen.BIAS, seed & 0xFFFFFFFF, rtg.AO_JITTER)
        counts = rtg.ao_host(sph, h, table, ap, walk=0, threads=THREADS)
        frames.append(counts.astype(np.float64))
        acc, ln = rtg.accumulate_host(h, W, H, p, counts, prev, zoom=A.ZOOM, threads=THREADS)
        prev = (cam, h, acc, ln)
    acc, ln = prev[2].reshape(-1).astype(np.float64), prev[3].reshape(-1)
    full = ln == 3
    assert full.sum() >= hit.sum() // 2 and not (full & ~hit).any()
    mean = (frames[0] + frames[1] + frames[2]) / 3
    assert (frames[0] != frames[1]).any() and (np.abs(frames[2] - mean)[full] > 0.3).any()
    err = float(np.abs(acc - mean)[full].max())
    print(f"host chain: max |acc - mean| {err:.3g}, tol {tol:.3g} (e = {e:.3g}, u = {u:.3g})")
    assert err <= tol


# ---- 6. non-vacuity ----

@pytest.mark.parametrize("name", SCENES)
def test_inputs_are_not_vacuous(rtg, name):
    for pk in ("same", "pan"):
        hits, found, rejected = A.facts(name, pk)
        print(f"facts {name} {pk}: {hits} hits, {found} find history, rejected by flag {rejected}")
        assert 2 * found >= hits > 100, (pk, hits, found)
        assert all(v >= 1 for v in rejected.values()), (pk, rejected)
    for pk in ("away", "nan"):  # every k <= 0, or every comparison false: nothing is found
        ln = A.want(name, *FULL, "gray", pk, A.SETS[2])[1]
        real = G.guides(name, *FULL)["id"] >= 0
        assert (ln[real] == 1).all() and (ln[~real] == 0).all()
    k = rtg.camera_project_host(A.pose(name, "away"), *FULL, G.raw_guides(name)["point"])[:, 2]
    assert (k[G.raw_guides(name).reshape(-1)["id"] >= 0] <= 0).all()
    ln = A.prev_state(name, *FULL, "pan", 1, 65535)[1]
    ids = A.prev_hits(name, *FULL, "pan")["id"]
    assert (ln[ids >= 0] == 0).any() and (ln[ids < 0] != 0).any() and (ln == 65535).any()
    assert (ids >= 1000).sum() >= 9


# ---- 7. errors ----

def test_entry_point_errors(rtg):
    R = rtg
    W, H = 33, 17
    n = W * H
    L = R.lib()

    def roomy(a):
        """`a` as the first half of an allocation twice its size: a range that
        starts inside it and runs past its end (the straddling cases below)
        lies in memory of its own, not in whichever argument the heap put next
        (which named that argument in the message, on some runs)."""
        return np.concatenate([a, np.zeros_like(a)])[:len(a)]

    h = roomy(np.ascontiguousarray(G.guides("reference", W, H)))
    ph = roomy(np.ascontiguousarray(A.prev_hits("reference", W, H, "pan")))
    src = np.zeros(n, F)
    pacc, pm2, plen = roomy(np.zeros(n, F)), np.zeros(n, F), np.ones(n, np.uint16)
    acc, m2, ln = np.full(n, 7, F), roomy(np.full(n, 7, F)), np.full(n, 7, np.uint16)
    cam = np.ascontiguousarray(A.pose("reference", "pan"))
    ok = R.accumulate_params(R.FILTER_GRAY, A.ALL, 1.0, 3, 3)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(hits=h, w=W, hh=H, p=ok, s=src, c=cam, prev=(ph, pacc, plen, pm2), out=(acc, ln, m2)):
        v = [x if isinstance(x, (int, type(None))) else P(x) for x in
             (hits, p, s, c, *prev, *out)]
        return L.rtg_accumulate_host(v[0], w, hh, v[1], v[2], v[3], ctypes.c_float(A.ZOOM), v[4],
                                     v[5], v[6], v[7], v[8], v[9], v[10], 1)

    par = R.accumulate_params
    for kw, msg in ((dict(hits=None), "accumulate: null hit buffer"),
                    (dict(s=None), "accumulate: null source"),
                    (dict(p=None), "accumulate: null params"),
                    (dict(out=(None, ln, m2)), "accumulate: null outAcc"),
                    (dict(out=(acc, None, m2)), "accumulate: null outLen"),
                    (dict(prev=(None, pacc, plen, pm2)), "all null or all non-null"),
                    (dict(prev=(ph, None, plen, pm2)), "all null or all non-null"),
                    (dict(prev=(ph, pacc, None, None)), "all null or all non-null"),
                    (dict(c=None), "accumulate: null previous pose"),
                    (dict(prev=(ph, pacc, plen, None)), "accumulate: outM2 without prevM2"),
                    (dict(out=(acc, ln, None)), "accumulate: prevM2 without outM2"),
                    (dict(w=0), "accumulate: empty frame"),
                    (dict(hh=0), "accumulate: empty frame"),
                    (dict(w=(1 << 24) + 1), "at most 2^24"),
                    (dict(hh=(1 << 24) + 1), "at most 2^24"),
                    (dict(p=par(1, 0, 0.0, 9, 3)), "normalLog2 9"),
                    (dict(p=par(3, 0, 0.0, 0, 3)), "kind 3"),
                    (dict(p=par(1, 16, 0.0, 0, 3)), "unknown flags 0x10"),
                    (dict(p=par(1, 0, 0.0, 0, 0)), "maxHistory 0"),
                    (dict(p=par(1, 0, 0.0, 0, 65536)), "maxHistory 65536"),
                    (dict(out=(src, ln, m2)), "outAcc overlaps src"),
                    (dict(out=(pacc, ln, m2)), "outAcc overlaps prevAcc"),
                    (dict(out=(P(pacc) + 4 * n - 4, ln, m2)), "outAcc overlaps prevAcc"),
                    (dict(out=(pm2, ln, m2)), "outAcc overlaps prevM2"),
                    (dict(out=(P(h) + 32 * n - 4, ln, m2)), "outAcc overlaps hits"),
                    (dict(out=(P(ph) + 8, ln, m2)), "outAcc overlaps prevHits"),
                    (dict(out=(acc, P(acc) + 2, m2)), "outAcc overlaps outLen"),
                    (dict(out=(acc, ln, acc)), "outAcc overlaps outM2"),
                    (dict(out=(acc, plen, m2)), "outLen overlaps prevLen"),
                    (dict(out=(acc, P(m2) + 4 * n - 2, m2)), "outLen overlaps outM2"),
                    (dict(out=(acc, ln, pm2)), "outM2 overlaps prevM2"),
                    (dict(out=(acc, ln, pacc)), "outM2 overlaps prevAcc")):
        assert call(**kw) == -1, kw
        assert msg.encode() in L.rtg_last_error(), (msg, L.rtg_last_error())
    assert (acc == 7).all() and (m2 == 7).all() and (ln == 7).all()  # nothing was written
    # a reset frame may carry outM2 alone, and needs no pose
    assert call(c=None, prev=(None, None, None, None)) == 0
    assert (ln == (h["id"] >= 0)).all() and (m2 == 0).all()
    # ranges that touch do not overlap
    both = np.zeros(2 * n, F)
    assert call(out=(both[:n], ln, both[n:])) == 0
    # the wrappers' own checks
    with pytest.raises(ValueError, match="hit records"):
        R.accumulate_host(h[:-1], W, H, ok, src)
    with pytest.raises(ValueError, match="previous state"):
        R.accumulate_host(h, W, H, ok, src, (cam, ph, pacc[:-1], plen))

    pts = np.zeros((4, 3), F)
    out = np.full((4, 3), 7, F)

    def proj(c=cam, w=W, hh=H, p=pts, cnt=4, o=out):
        return L.rtg_camera_project_host(P(c), w, hh, ctypes.c_float(A.ZOOM), P(p), cnt, P(o), 1)

    for kw, msg in ((dict(c=None), "camera_project: null camera"),
                    (dict(p=None), "camera_project: null points"),
                    (dict(o=None), "camera_project: null destination"),
                    (dict(w=0), "camera_project: empty frame"),
                    (dict(hh=0), "camera_project: empty frame"),
                    (dict(w=(1 << 24) + 1), "at most 2^24"),
                    (dict(hh=(1 << 24) + 1), "at most 2^24")):
        assert proj(**kw) == -1, kw
        assert msg.encode() in L.rtg_last_error(), (msg, L.rtg_last_error())
    assert (out == 7).all()
    assert proj(p=None, cnt=0, o=None) == 0  # no points: nothing to read or write
    assert R.camera_project_host(cam, W, H, np.zeros((0, 3), F)).shape == (0, 3)
