"""Host tests of the guided upsampling (rtg_upsample_host, rtg_hits_pick_host,
rtg_values_place_host; include/rtg.h, "upsample"); no GPU needed.

  1. upsample_host == upgen.restate (numpy float32, one operation a line) word
     for word, dst and list: three kinds, every subset of the four flags,
     L = 1, 2, 3 on the 48 x 32 frame, 1 and 3 threads; and on the frames with
     hand-made records and non-finite values;
  2. the correspondence the header claims: the low record (X, Y) is the full
     record (f X, f Y) bit for bit, at an orbit pose;
  3. a constant low signal: 0.5 comes back exactly, 0.3 within 8 * 2^-24 * 0.3;
  4. non-vacuity of the frames used, asserted;
  5. the list's capacity: 0, count - 1 and n;
  6. pick and place against numpy indexing, an index >= n among them;
  7. every argument error.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import aogen
import upgen as U
from upgen import FULL, LS, SCENES, SIGNALS
from test_raytrace_host import THREADS

F = np.float32
SUBSETS = list(range(16))


@pytest.fixture(scope="module")
def R(rtg):
    return rtg


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else \
        f"{len(bad)} words differ, first at {bad[0]}: {got[bad[0]]:#x} vs {want[bad[0]]:#x}"


def _run(R, full, low, W, H, L, p, src, threads, cap=None):
    """(dst words, list, count) of upsample_host; the list pre-filled."""
    lst = np.full(W * H if cap is None else cap, U.FILL, np.uint32)
    out, lst, cnt = R.upsample_host(full, W, H, p, low, W >> L, H >> L, src, holes=lst,
                                    threads=threads)
    return out.view(np.uint32).reshape(-1), lst, cnt


# ---- 1. the host form is the header's text ----

@pytest.mark.parametrize("signal", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_host_equals_restatement(R, name, signal):
    W, H = FULL
    for L in LS:
        full, low = U.frames(name, W, H, L)
        src = U.low_signal(name, W >> L, H >> L, signal)
        for flags in SUBSETS:
            want, holes = U.restate(full, low, W, H, L, flags, U.NORMAL_LOG2, U.plane_scale(name), src)
            for threads in (1, 3):
                got, lst, cnt = _run(R, full, low, W, H, L, U.params(R, name, signal, L, flags), src,
                                     threads)
                assert _first_bad(got, want) is None, (L, flags, threads, _first_bad(got, want))
                assert cnt == len(holes) and (lst[:cnt] == holes).all(), (L, flags, threads)
                assert (lst[cnt:] == U.FILL).all(), "entries past the count were written"
            # without a list: the same frame
            plain = R.upsample_host(full, W, H, U.params(R, name, signal, L, flags), low, W >> L,
                                    H >> L, src, threads=THREADS)
            assert plain.shape == ((H, W, 3) if signal == "rgb" else (H, W))
            assert plain.view(np.uint32).reshape(-1).tobytes() == want.tobytes()


@pytest.mark.parametrize("signal", ["rgb", "gray"])
@pytest.mark.parametrize("name", SCENES)
def test_hostile_frames_equal_restatement(R, name, signal):
    W, H = FULL
    seen_nan = False
    for L in LS:
        full, low = U.frames(name, W, H, L, True)
        src = U.low_signal(name, W >> L, H >> L, signal, True)
        assert not np.isfinite(src).all() and not np.isfinite(full["normal"]).all()
        for flags, nl, scale in ((0, 0, 0.0), (U.ALL, 3, None), (U.SKIP, 0, 0.0), (U.GEOM, 8, None),
                                 (U.PLANE, 0, float("inf")), (U.PLANE, 0, float("nan")),
                                 (U.NORMAL, 0, 0.0)):
            sc = U.plane_scale(name) if scale is None else scale
            want, holes = U.restate(full, low, W, H, L, flags, nl, sc, src)
            got, lst, cnt = _run(R, full, low, W, H, L, U.params(R, name, signal, L, flags, sc, nl),
                                 src, THREADS)
            assert _first_bad(got, want) is None, (L, flags, _first_bad(got, want))
            assert cnt == len(holes) and (lst[:cnt] == holes).all(), (L, flags)
            seen_nan |= bool((got == 0xFFC00000).any())
    assert seen_nan  # without the flag the NaN reaches some pixel, in its canonical form


# ---- 2. the two frames' correspondence ----

@pytest.mark.parametrize("name", SCENES)
def test_low_record_is_the_full_record(R, name):
    W, H = FULL
    poses = [U.POSES[name], ((3.0, 2.0, -1.0), (0.0, 0.0, -10.0)), ((-7.0, 4.0, -30.0), (0.5, 0.0, -12.0))]
    sph = aogen.scene(name)
    hits = 0
    for eye, target in poses:
        cam = R.camera_look_at(eye, target, (0.1, 1.0, 0.05))
        rays = R.camera_rays_host(cam, W, H, alias_factor=1.0).reshape(H, W, -1)
        full = R.intersect_host(sph, rays.reshape(-1, rays.shape[-1]), walk=0, threads=THREADS)
        full = full.reshape(H, W)
        for L in LS:
            f = 1 << L
            lr = R.camera_rays_host(cam, W >> L, H >> L, alias_factor=1.0).reshape(H >> L, W >> L, -1)
            assert lr.tobytes() == np.ascontiguousarray(rays[::f, ::f]).tobytes(), (eye, L)
            low = R.intersect_host(sph, lr.reshape(-1, lr.shape[-1]), walk=0, threads=THREADS)
            assert low.tobytes() == np.ascontiguousarray(full[::f, ::f]).tobytes(), (eye, L)
            hits += int((low["id"] >= 0).sum())
    assert hits > 0


# ---- 3. a constant signal ----

@pytest.mark.parametrize("name", SCENES)
def test_constant_signal(R, name):
    W, H = FULL
    for L in LS:
        full, low = U.frames(name, W, H, L)
        hit = (full["id"] >= 0).reshape(H, W)
        for flags in (0, U.GEOM):
            for signal, C in (("gray", 1), ("rgb", 3)):
                p = U.params(R, name, signal, L, flags)
                nl = (W >> L) * (H >> L)
                out, lst, cnt = R.upsample_host(full, W, H, p, low, W >> L, H >> L,
                                                np.full((nl, C), 0.5, F), holes=W * H)
                solid = hit.copy()
                solid.reshape(-1)[lst[:cnt]] = False
                out = out.reshape(H, W, C)
                # every w * 0.5 is w's exponent moved, so sum is sw's and the quotient 0.5
                assert (out[solid] == F(0.5)).all() and solid.any()
                assert (out[~solid].view(np.uint32) == 0).all()  # +0.f on misses and holes
                out = R.upsample_host(full, W, H, p, low, W >> L, H >> L,
                                      np.full((nl, C), 0.3, F)).reshape(H, W, C)
                # four products, three adds on each side and one division, 2^-24 each
                c = np.float64(F(0.3))
                err = np.abs(out[solid].astype(np.float64) - c)
                assert err.max() <= 8 * 2.0 ** -24 * c, err.max()


# ---- 4. non-vacuity ----

@pytest.mark.parametrize("name", SCENES)
def test_frames_are_not_vacuous(R, name):
    W, H = FULL
    shares = []
    for L in LS:
        full, low = U.frames(name, W, H, L)
        src = U.low_signal(name, W >> L, H >> L, "gray")
        sc = U.plane_scale(name)
        words, holes, cnt = U.want(name, W, H, L, "gray", U.GEOM)
        hit = int((full["id"] >= 0).sum())
        shares.append(cnt / hit)
        assert 0 < cnt / hit < 0.5, (L, cnt, hit)
        taps = U.restate(full, low, W, H, L, U.GEOM, U.NORMAL_LOG2, sc, src, taps=True)[2]
        for k in (1, 2, 3, 4):
            assert (taps == k).any(), (L, k)
        assert int((taps == 0).sum()) == cnt
        for flag in (U.SAME_ID, U.NORMAL, U.PLANE):
            other = U.want(name, W, H, L, "gray", U.GEOM & ~flag)[0]
            assert (other != words).any(), (L, flag)
        # SKIP_NONFINITE on the frame with planted values
        a = U.want(name, W, H, L, "gray", U.GEOM, True)[0]
        b = U.want(name, W, H, L, "gray", U.GEOM | U.SKIP, True)[0]
        assert (a != b).any(), L
    print(f"{name}: hole shares {['%.3f' % s for s in shares]}")


# ---- 5. the capacity ----

@pytest.mark.parametrize("name", SCENES)
def test_hole_capacity(R, name):
    W, H = FULL
    L = 2
    full, low = U.frames(name, W, H, L)
    src = U.low_signal(name, W >> L, H >> L, "count")
    p = U.params(R, name, "count", L, U.GEOM)
    words, holes, count = U.want(name, W, H, L, "count", U.GEOM)
    assert count >= 2 and (np.diff(holes.astype(np.int64)) > 0).all()
    for cap in (0, count - 1, W * H):
        got, lst, cnt = _run(R, full, low, W, H, L, p, src, THREADS, cap=cap)
        k = min(count, cap)
        assert cnt == count and got.tobytes() == words.tobytes()
        assert len(lst) == cap and (lst[:k] == holes[:k]).all() and (lst[k:] == U.FILL).all()


# ---- 6. pick and place ----

def test_pick_and_place(R):
    W, H = FULL
    h = U.frames("c5", W, H, 1, True)[0]
    n = len(h)
    rng = np.random.default_rng(77)
    idx = rng.permutation(n)[:301].astype(np.uint32)
    idx[[5, 100, 300]] = (n, n + 7, 0xFFFFFFFF)
    inside = idx < n
    for threads in (1, 3):
        got = R.hits_pick_host(h, idx, threads=threads)
        assert got[inside].tobytes() == h[idx[inside]].tobytes()
        miss = got[~inside]
        assert (miss["id"] == -1).all()
        words = miss.view(np.uint32).reshape(len(miss), 8)
        assert (words[:, 1:] == 0).all()
        for kind, C, dt in ((R.FILTER_RGB, 3, F), (R.FILTER_GRAY, 1, F), (R.FILTER_COUNT, 1, np.uint16)):
            vals = rng.integers(0, 60000, size=(len(idx), C)).astype(dt)
            if dt is F:
                vals[3, 0], vals[4, C - 1] = np.nan, -0.0
                vals.view(np.uint32)[7, 0] = 0x7FA00001  # a signalling NaN keeps its words
            dst = np.full((n, C), 9.0, F)
            want = dst.copy()
            want[idx[inside]] = vals[inside].astype(F) if dt is not F else vals[inside]
            R.values_place_host(kind, vals, idx, dst, threads=threads)
            assert dst.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), kind
    assert len(R.hits_pick_host(h, np.zeros(0, np.uint32))) == 0  # m == 0
    dst = np.ones(4, F)
    R.values_place_host(R.FILTER_GRAY, np.zeros(0, F), np.zeros(0, np.uint32), dst)
    assert (dst == 1).all()


# ---- 7. argument errors ----

def test_argument_errors(R):
    W, H, L = 16, 8, 1
    full, low = U.frames("reference", W, H, L)
    src = U.low_signal("reference", W >> L, H >> L, "gray")
    ok = R.upsample_params(L, R.FILTER_GRAY, U.ALL, 1.0, 3)
    par = R.upsample_params
    lib = R.lib()
    h, lh, s = (np.ascontiguousarray(a) for a in (full, low, src))
    out = np.zeros(W * H * 3, F)
    lst, cnt = np.zeros(W * H, np.uint32), np.zeros(1, np.uint32)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def call(hits=h, w=W, hh=H, p=ok, lhits=lh, wl=W >> L, hl=H >> L, lsrc=s, dst=out, holes=lst,
             cap=W * H, count=cnt):
        return lib.rtg_upsample_host(P(hits), w, hh, P(p), P(lhits), wl, hl, P(lsrc), P(dst),
                                     P(holes), cap, P(count), 1)

    assert call() == 0 and out.any()
    out[:], lst[:], cnt[:] = 0, 0, 0
    for kw, msg in ((dict(hits=None), b"upsample: null hit buffer"),
                    (dict(p=None), b"upsample: null params"),
                    (dict(lhits=None), b"upsample: null low hit buffer"),
                    (dict(lsrc=None), b"upsample: null low source"),
                    (dict(dst=None), b"upsample: null destination"),
                    (dict(w=0), b"upsample: empty frame"),
                    (dict(hh=0), b"upsample: empty frame"),
                    (dict(wl=0), b"upsample: empty low frame"),
                    (dict(hl=0), b"upsample: empty low frame"),
                    (dict(w=(1 << 24) + 1), b"at most 2^24"),
                    (dict(hh=(1 << 24) + 1), b"at most 2^24"),
                    (dict(w=1 << 16, hh=1 << 16), b"at most 2^32 - 1 pixels"),
                    (dict(p=par(0, 1, 0, 0.0, 0)), b"scaleLog2 0"),
                    (dict(p=par(4, 1, 0, 0.0, 0)), b"scaleLog2 4"),
                    (dict(w=W + 1), b"is not 2 times the low frame"),
                    (dict(hh=H + 2), b"is not 2 times the low frame"),
                    (dict(p=par(2, 1, 0, 0.0, 0)), b"is not 4 times the low frame"),
                    (dict(p=par(1, 1, 0, 0.0, 9)), b"normalLog2 9"),
                    (dict(p=par(1, 3, 0, 0.0, 0)), b"kind 3"),
                    (dict(p=par(1, 1, 16, 0.0, 0)), b"unknown flags 0x10"),
                    (dict(holes=None), b"holeCount without holes"),
                    (dict(count=None), b"holes without holeCount"),
                    (dict(dst=h), b"dst overlaps hits"),
                    (dict(dst=lh), b"dst overlaps lowHits"),
                    (dict(dst=s), b"dst overlaps lowSrc"),
                    (dict(holes=out), b"dst overlaps holes"),
                    (dict(count=out), b"dst overlaps holeCount"),
                    (dict(holes=h), b"holes overlaps hits"),
                    (dict(holes=lh), b"holes overlaps lowHits"),
                    (dict(holes=s, cap=4), b"holes overlaps lowSrc"),
                    (dict(count=lst), b"holes overlaps holeCount"),
                    (dict(count=h), b"holeCount overlaps hits"),
                    (dict(count=lh), b"holeCount overlaps lowHits"),
                    (dict(count=s), b"holeCount overlaps lowSrc")):
        assert call(**kw) == -1, kw
        assert msg in lib.rtg_last_error(), (kw, lib.rtg_last_error())
    assert not out.any() and not lst.any() and not cnt.any()  # nothing was written
    size = ctypes.c_size_t(7)
    assert lib.rtg_upsample_scratch(W, H, 0, ctypes.byref(size)) == 0 and size.value == 0
    assert lib.rtg_upsample_scratch(W, H, 1, ctypes.byref(size)) == 0
    assert size.value >= 36 and size.value % 8 == 0
    assert lib.rtg_upsample_scratch(W, H, 1, None) == -1
    assert lib.rtg_upsample_scratch(0, H, 1, ctypes.byref(size)) == -1
    assert lib.rtg_upsample_scratch(1 << 16, 1 << 16, 1, ctypes.byref(size)) == -1
    # the index calls
    idx, rec = np.zeros(4, np.uint32), np.zeros(4, R.HIT_DTYPE)
    vals, dst = np.zeros(4, F), np.zeros(W * H, F)
    for a, msg in (((None, 8, P(idx), 4, P(rec), 1), b"hits_pick: null input"),
                   ((P(h), 8, None, 4, P(rec), 1), b"hits_pick: null index buffer"),
                   ((P(h), 8, P(idx), 4, None, 1), b"hits_pick: null output"),
                   ((P(h), 0, P(idx), 4, P(rec), 1), b"hits_pick: n is 0"),
                   ((P(h), 8, P(idx), 4, P(h), 1), b"hits_pick: the output overlaps an input")):
        assert lib.rtg_hits_pick_host(*a) == -1 and msg in lib.rtg_last_error(), msg
    for a, msg in (((3, P(vals), P(idx), 4, 8, P(dst), 1), b"values_place: kind 3"),
                   ((1, None, P(idx), 4, 8, P(dst), 1), b"values_place: null input"),
                   ((1, P(vals), None, 4, 8, P(dst), 1), b"values_place: null index buffer"),
                   ((1, P(vals), P(idx), 4, 8, None, 1), b"values_place: null output"),
                   ((1, P(vals), P(idx), 4, 0, P(dst), 1), b"values_place: n is 0"),
                   ((1, P(vals), P(idx), 4, 4, P(vals), 1), b"the output overlaps an input"),
                   ((1, P(vals), P(dst), 4, 4, P(dst), 1), b"the output overlaps an input")):
        assert lib.rtg_values_place_host(*a) == -1 and msg in lib.rtg_last_error(), msg
