"""CPU tests of the edge-stopping a-trous filter (rtg_filter_host,
rtg_filter_scratch; include/rtg.h, "filter"): no GPU needed.

  1. filter_host == the numpy float32 restatement (filtergen.restate), word
     for word, on every frame, signal and parameter set of filtergen;
  2. thread counts give the same words;
  3. independence: with SAME_ID the values of other ids never reach a sphere's
     pixels; a NaN spreads without SKIP_NONFINITE and is filled with it;
  4. pixels with id < 0 pass through, a frame of misses is the identity;
  5. a constant signal comes back within the derived rounding bound;
  6. non-vacuity of the inputs and of the filter on them;
  7. every argument error, with its message.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import filtergen as G
from filtergen import ALL, FRAMES, FULL, NORMAL, PLANE, SAME_ID, SCENES, SETS, SIGNALS, SKIP

F = np.float32


def _words(a):
    return np.ascontiguousarray(a, F).view(np.uint32).reshape(-1)


# ---- 1. the definition ----

@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_host_equals_restatement(rtg, name, kind):
    for W, H in FRAMES:
        h, src = G.guides(name, W, H), G.signal(name, W, H, kind)
        for st in SETS:
            got = G.want(name, W, H, kind, st)
            ref = G.restate(h, W, H, st, G.plane_scale(name, st[3]), src)
            bad = np.flatnonzero(got != ref)
            assert not len(bad), (W, H, st, len(bad), bad[:4], got[bad[:4]], ref[bad[:4]])


# ---- 2. threads ----

@pytest.mark.parametrize("name", SCENES)
def test_thread_counts_agree(rtg, name):
    W, H = FULL
    for kind in SIGNALS:
        for st in (SETS[2], SETS[5]):
            p = G.params(rtg, name, kind, st)
            for threads in (0, 1, 3, 64):
                got = rtg.filter_host(G.guides(name, W, H), W, H, p, G.signal(name, W, H, kind),
                                      threads=threads)
                assert (_words(got) == G.want(name, W, H, kind, st)).all(), (kind, st, threads)


# ---- 3. independence ----

def _biggest_id(h):
    ids, counts = np.unique(h["id"][h["id"] >= 0], return_counts=True)
    return int(ids[np.argmax(counts)])


@pytest.mark.parametrize("name", SCENES)
def test_same_id_keeps_other_spheres_out(rtg, name):
    W, H = FULL
    h = G.guides(name, W, H)
    mine = h["id"] == _biggest_id(h)
    assert 20 < mine.sum() < W * H - 20
    for kind in ("rgb", "gray"):
        src = G.signal(name, W, H, kind).copy()
        other = src.copy()
        rng = np.random.default_rng(11)
        other[~mine] = rng.uniform(-1e6, 1e6, size=other[~mine].shape).astype(F)
        other[np.flatnonzero(~mine)[::3]] = np.nan
        for flags in (SAME_ID, SAME_ID | NORMAL | PLANE, ALL):
            p = rtg.filter_params(5, G.KINDS[kind], flags, G.plane_scale(name, None), 3)
            a = _words(rtg.filter_host(h, W, H, p, src)).reshape(W * H, -1)
            b = _words(rtg.filter_host(h, W, H, p, other)).reshape(W * H, -1)
            assert (a[mine] == b[mine]).all(), (kind, flags)
        p = rtg.filter_params(5, G.KINDS[kind], NORMAL | PLANE, G.plane_scale(name, None), 3)
        a = _words(rtg.filter_host(h, W, H, p, src)).reshape(W * H, -1)
        b = _words(rtg.filter_host(h, W, H, p, other)).reshape(W * H, -1)
        assert (a[mine] != b[mine]).any(), (kind, "without SAME_ID the other ids do reach it")


def _finite_same_id_tap(h, W, H, src):
    """Per pixel: one of its 25 step-1 taps is inside the frame, of its id and finite."""
    ids = h["id"].reshape(H, W)
    ok = np.isfinite(src.reshape(H, W, -1)).all(-1)
    out = np.zeros((H, W), bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] |= ok[ys, xs] & (ids[ys, xs] == ids[yd, xd])
    return out.reshape(-1)


@pytest.mark.parametrize("name", SCENES)
def test_nonfinite_values_spread_or_are_skipped(rtg, name):
    W, H = FULL
    h, src = G.guides(name, W, H), G.signal(name, W, H, "rgb")
    at_nan, at_inf, _ = G.planted(name, W, H)
    assert np.isnan(src[at_nan]).any() and np.isinf(src[at_inf]).any()
    real = h["id"] >= 0
    # without the flag the NaN reaches its same-id neighbours
    out = rtg.filter_host(h, W, H, rtg.filter_params(1, 0, SAME_ID), src).reshape(W * H, 3)
    reached = np.isnan(out).any(-1) & (h["id"] == h["id"][at_nan])
    assert reached[at_nan] and reached.sum() >= 3, reached.sum()
    # with it, one pass: finite wherever one finite same-id tap exists
    out = rtg.filter_host(h, W, H, rtg.filter_params(1, 0, SAME_ID | SKIP), src).reshape(W * H, 3)
    can = _finite_same_id_tap(h, W, H, src) & real
    assert can[at_nan] and can[at_inf] and can.sum() > 0.9 * real.sum()
    assert np.isfinite(out[can]).all()
    assert np.isfinite(out[at_nan]).all() and np.isfinite(out[at_inf]).all()  # filled
    # and after five passes
    out = rtg.filter_host(h, W, H, rtg.filter_params(5, 0, SAME_ID | SKIP), src).reshape(W * H, 3)
    assert np.isfinite(out[can]).all()


# ---- 4. pass-through ----

@pytest.mark.parametrize("name", SCENES)
def test_background_passes_through(rtg, name):
    W, H = FULL
    h = G.guides(name, W, H)
    miss = h["id"] < 0
    assert miss.sum() > 0.1 * W * H
    for kind in SIGNALS:
        src = G.signal(name, W, H, kind)
        first = G.canon(src.astype(F)).reshape(W * H, -1)
        for st in SETS:
            got = G.want(name, W, H, kind, st).reshape(W * H, -1)
            assert (got[miss] == first[miss]).all(), (kind, st)
    none = h.copy()
    none["id"] = -1 - (np.arange(W * H) % 3)
    for kind in SIGNALS:
        src = G.signal(name, W, H, kind)
        for passes in (1, 2, 8):
            got = rtg.filter_host(none, W, H, rtg.filter_params(passes, G.KINDS[kind], ALL, 1.0, 3),
                                  src)
            assert (_words(got) == G.canon(src.astype(F)).reshape(-1)).all(), (kind, passes)


# ---- 5. a constant signal ----

@pytest.mark.parametrize("name", SCENES)
def test_constant_signal_stays_constant(rtg, name):
    """Per pass at most 25 products, 24 + 24 additions and one quotient, each
    within half an ulp, all weights positive: at most 51 * 2^-24 relative error
    per pass; the bound asserted is 64 * 2^-24 * passes * c.  The derivation
    needs finite weights, so the guides are the frame's records as intersect_host
    wrote them: the planted normal of length 2.5 has a cosine of 6.25, which
    squared eight times is +inf (and inf / inf a NaN, as the arithmetic says)."""
    W, H = FULL
    h = G.raw_guides(name).reshape(-1)
    real = h["id"] >= 0
    for c in (0.5, 1.2345678, 2.0):
        src = np.full(W * H, 7.0, F)
        src[real] = F(c)
        for st in SETS:
            passes = st[0]
            p = rtg.filter_params(passes, 1, st[1], G.plane_scale(name, st[3]), st[2])
            out = rtg.filter_host(h, W, H, p, src).reshape(-1)
            err = np.abs(out[real].astype(np.float64) - float(F(c))).max()
            assert err <= 64 * 2.0 ** -24 * passes * c, (c, st, err)


# ---- 6. non-vacuity ----

@pytest.mark.parametrize("name", SCENES)
def test_inputs_and_filter_are_not_vacuous(rtg, name):
    ids, hit_share, miss_share, edges = G.guide_facts(name)
    assert ids >= 3 and hit_share >= 0.2 and miss_share >= 0.1 and edges >= 30, G.guide_facts(name)
    W, H = FULL
    h = G.guides(name, W, H)
    assert np.isnan(h["normal"]).any() and np.isnan(h["point"]).any() and (h["id"] == 1 << 30).sum() == 1
    real = h["id"] >= 0
    st = SETS[2]
    assert st[:2] == (5, ALL)
    for kind in SIGNALS:
        src = G.signal(name, W, H, kind).astype(F).reshape(W * H, -1)
        out = G.want(name, W, H, kind, st).view(F).reshape(W * H, -1)
        changed = (G.canon(src) != G.canon(out)).any(-1)
        assert changed[real].sum() >= 0.3 * real.sum(), (kind, changed[real].mean())
    src = G.signal(name, W, H, "count").astype(np.float64)
    out = G.want(name, W, H, "count", st).view(F).astype(np.float64)
    assert out[real].var() < src[real].var(), (out[real].var(), src[real].var())


# ---- 7. argument errors ----

def test_argument_errors(rtg):
    R = rtg
    W, H = 8, 8
    h, src = G.guides("reference", W, H), G.signal("reference", W, H, "gray")
    ok = R.filter_params(2, 1, ALL, 1.0, 3)
    assert R.filter_scratch(W, H, ok) == W * H * 4
    assert R.filter_scratch(W, H, R.filter_params(1, 0)) == 0
    assert R.filter_scratch(5, 1, R.filter_params(8, 0)) == 64  # 60 bytes, 16-byte units
    assert R.filter_scratch(5, 1, R.filter_params(3, 2)) == 32
    cases = ((W, H, R.filter_params(0, 1), "0 passes"),
             (W, H, R.filter_params(9, 1), "9 passes"),
             (W, H, R.filter_params(2, 1, normal_log2=9), "normalLog2 9"),
             (W, H, R.filter_params(2, 3), "kind 3"),
             (W, H, R.filter_params(2, 1, 16), "unknown flags 0x10"),
             (0, H, ok, "empty frame"), (W, 0, ok, "empty frame"),
             (1 << 16, 1 << 16, ok, "at most 2\\^32 - 1"))
    for w, hh, p, msg in cases:
        with pytest.raises(R.RtgError, match="filter_scratch: .*" + msg):
            R.filter_scratch(w, hh, p)
    L = R.lib()
    out = np.zeros(W * H, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    okp = P(ok)
    for w, hh, p, msg in cases:
        assert L.rtg_filter_host(P(h), w, hh, P(p), P(src), P(out), 1) == -1
        text = L.rtg_last_error().decode()
        assert text.startswith("filter: ") and msg.replace("\\", "") in text, text
    for args, msg in (((None, W, H, okp, P(src), P(out), 1), "filter: null hit buffer"),
                      ((P(h), W, H, okp, None, P(out), 1), "filter: null source"),
                      ((P(h), W, H, okp, P(src), None, 1), "filter: null destination"),
                      ((P(h), W, H, None, P(src), P(out), 1), "filter: null params")):
        assert L.rtg_filter_host(*args) == -1
        assert L.rtg_last_error().decode().startswith(msg), L.rtg_last_error()
    assert L.rtg_filter_scratch(W, H, okp, None) == -1
    assert L.rtg_last_error().decode().startswith("filter_scratch: null size")
    assert L.rtg_filter_scratch(W, H, None, ctypes.byref(ctypes.c_size_t())) == -1
    assert L.rtg_last_error().decode().startswith("filter_scratch: null params")
    # the destination's bytes may not touch the source's
    buf = np.zeros(2 * W * H, F)
    buf[:W * H] = src
    for off in (0, 1, W * H - 1):
        assert L.rtg_filter_host(P(h), W, H, okp, P(buf), P(buf[off:]), 1) == -1
        assert L.rtg_last_error().decode().startswith("filter: the destination overlaps the source")
    counts = np.zeros(4 * W * H, np.uint16)  # a COUNT source is half as long as its destination
    cp = R.filter_params(2, 2)
    assert L.rtg_filter_host(P(h), W, H, P(cp), P(counts[W * H - 1:]), P(counts.view(F)), 1) == -1
    assert L.rtg_last_error().decode().startswith("filter: the destination overlaps the source")
    assert L.rtg_filter_host(P(h), W, H, P(cp), P(counts[2 * W * H:]), P(counts.view(F)), 1) == 0
    assert L.rtg_filter_host(P(h), W, H, okp, P(buf), P(buf[W * H:]), 1) == 0  # adjacent: legal
    assert L.rtg_last_error() == b""
    with pytest.raises(ValueError):
        R.filter_host(h, W, H + 1, ok, src)
