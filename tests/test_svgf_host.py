"""CPU tests of the variance estimate and the variance-guided a-trous passes
(rtg_variance_host, rtg_svgf_host, rtg_svgf_scratch; include/rtg.h, "variance
and svgf"): no GPU needed.

  1. both host forms == the numpy float32 restatement (svgfgen), word for word,
     on every frame, signal and parameter set of svgfgen;
  2. thread counts give the same words;
  3. with LUMA off and a finite variance the value words are filter_host's;
  4. a step inside one id survives LUMA exactly, and not the plain filter;
  5. the wide limit: a sigmaL so large that every z is 1 gives filter_host's words;
  6. one pass scales a constant variance by (70/256)^2;
  7. non-vacuity of the inputs and of both calls on them;
  8. the host chain ao -> accumulate (M2) -> variance -> svgf;
  9. every argument error, with its message.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import filtergen as G
import svgfgen as S
from filtergen import ALL, FRAMES, FULL, SCENES
from svgfgen import SIGNALS, SVGF_SETS

F = np.float32


def _words(a):
    return np.ascontiguousarray(a, F).view(np.uint32).reshape(-1)


def _bad(got, ref):
    bad = np.flatnonzero(got != ref)
    return None if not len(bad) else (len(bad), bad[:4], got[bad[:4]], ref[bad[:4]])


# ---- 1. the definitions ----

@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_variance_host_equals_restatement(rtg, name, kind):
    for W, H in FRAMES:
        h = G.guides(name, W, H)
        acc, m2 = S.state(name, W, H, kind)
        for which, st in S.variance_cases():
            got = S.want_variance(name, W, H, kind, which, st)
            ref = S.restate_variance(h, W, H, st, G.plane_scale(name, st[2]), acc, m2,
                                     S.len_field(name, W, H, which))
            assert _bad(got, ref) is None, (W, H, which, st, _bad(got, ref))


@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_svgf_host_equals_restatement(rtg, name, kind):
    for W, H in FRAMES:
        h, src, var = G.guides(name, W, H), G.signal(name, W, H, kind), S.var_field(name, W, H)
        for st in SVGF_SETS:
            got = S.want_svgf(name, W, H, kind, st)
            ref = S.restate_svgf(h, W, H, st, G.plane_scale(name, st[3]), src, var)
            assert _bad(got[0], ref[0]) is None, (W, H, st, "value", _bad(got[0], ref[0]))
            assert _bad(got[1], ref[1]) is None, (W, H, st, "variance", _bad(got[1], ref[1]))


# ---- 2. threads ----

@pytest.mark.parametrize("name", SCENES)
def test_thread_counts_agree(rtg, name):
    W, H = FULL
    h = G.guides(name, W, H)
    for kind in SIGNALS:
        acc, m2 = S.state(name, W, H, kind)
        for threads in (0, 1, 3, 64):
            for st in S.SVGF_FEW[:3]:
                v, var = rtg.svgf_host(h, W, H, S.svgf_params(rtg, name, kind, st),
                                       G.signal(name, W, H, kind), S.var_field(name, W, H),
                                       threads=threads)
                want = S.want_svgf(name, W, H, kind, st)
                assert (_words(v) == want[0]).all() and (_words(var) == want[1]).all(), (kind, st)
            for which, st in (("seeded", S.VAR_FEW[0]), ("zero", S.VAR_FEW[1])):
                got = rtg.variance_host(h, W, H, S.variance_params(rtg, name, kind, st), acc, m2,
                                        S.len_field(name, W, H, which), threads=threads)
                assert (_words(got) == S.want_variance(name, W, H, kind, which, st)).all()


# ---- 3. LUMA off is the filter ----

@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_luma_off_equals_filter(rtg, name, kind):
    W, H = FULL
    h, src = G.guides(name, W, H), G.signal(name, W, H, kind)
    var = np.abs(S.var_field(name, W, H))
    var = np.where(np.isfinite(var), var, F(0.25)).astype(F)
    for st in G.SETS:
        p = S.svgf_params(rtg, name, kind, st + (False, 4.0, 1e-6))
        got = _words(rtg.svgf_host(h, W, H, p, src, var)[0])
        assert _bad(got, G.want(name, W, H, kind, st)) is None, st


# ---- 4. a step inside one id ----

def _biggest_id(h):
    ids, counts = np.unique(h["id"][h["id"] >= 0], return_counts=True)
    return int(ids[np.argmax(counts)])


@pytest.mark.parametrize("name", SCENES)
def test_step_inside_one_id_is_preserved(rtg, name):
    """Variance 0 and epsL 1e-6: ls = 1e6, a tap across the step has z = 1 - 1e6
    clamped to 0, a tap on the centre's side z = 1, so every accepted tap has
    the centre's value c, sum = sw * c with c in {0, 1}, and out = c exactly."""
    W, H = FULL
    h = G.raw_guides(name).reshape(-1)
    ids = h["id"].reshape(H, W)
    mine = ids == _biggest_id(h)
    cols = np.flatnonzero(mine.any(0))
    x0 = int(cols[len(cols) // 2])
    beside = mine[:, x0 - 1] & mine[:, x0]
    assert beside.any(), "the step does not cross the id"
    src = np.zeros((H, W), F)
    src[:, x0:] = 1
    var = np.zeros((H, W), F)
    flags, scale = G.SAME_ID | G.NORMAL | G.PLANE, G.plane_scale(name, None)
    p = rtg.svgf_params(5, rtg.FILTER_GRAY, flags | rtg.SVGF_LUMA, scale, 3, 4.0, 1e-6)
    out, vout = rtg.svgf_host(h, W, H, p, src, var)
    assert (_words(out) == _words(src)).all()
    assert (_words(vout) == 0).all()
    plain = rtg.filter_host(h, W, H, rtg.filter_params(5, rtg.FILTER_GRAY, flags, scale, 3), src)
    changed = _words(plain).reshape(H, W) != _words(src).reshape(H, W)
    assert (changed[:, x0 - 1:x0 + 1] & mine[:, x0 - 1:x0 + 1]).any()


# ---- 5. the wide limit ----

WIDE_VAR, WIDE_SIGMA = 1e30, 1e4


@pytest.mark.parametrize("name", SCENES)
def test_wide_limit_equals_filter(rtg, name):
    """On paper: den = 1e4 * sqrt(v) with v >= 1e30 * (1/25)^8 after eight passes
    (a pass scales the variance by at least the least sum w^2 / (sum w)^2 of 25
    taps), so ls <= 4e-14 and l * ls < 2^-25 for every |l| < 7e5: z = 1.f.  The
    restatement confirms it tap by tap."""
    W, H = FULL
    h = G.raw_guides(name).reshape(-1)
    t = h["t"].astype(F)
    src = np.where(np.isfinite(t), t, F(0)).astype(F)
    assert np.abs(src).max() < 7e5
    var = np.full(W * H, WIDE_VAR, F)
    for st in G.SETS:
        full = st + (True, WIDE_SIGMA, 1e-6)
        scale = G.plane_scale(name, st[3])
        facts = {}
        ref = S.restate_svgf(h, W, H, full, scale, src, var, facts)
        assert facts["z1"], (st, "a z below 1: take a wider sigmaL")
        got = rtg.svgf_host(h, W, H, S.svgf_params(rtg, name, "gray", full), src, var)
        assert _bad(_words(got[0]), ref[0]) is None and _bad(_words(got[1]), ref[1]) is None, st
        want = rtg.filter_host(h, W, H, rtg.filter_params(st[0], rtg.FILTER_GRAY, st[1], scale, st[2]),
                               src)
        assert _bad(_words(got[0]), _words(want)) is None, st


# ---- 6. variance propagation ----

def test_one_pass_scales_a_constant_variance(rtg):
    """All 25 taps of an interior pixel are accepted with w = h h', multiples of
    2^-8 that sum to exactly 1, so vout = sum (w w) c.  w w is exact; each of
    the 25 products (w w) c and each of the 25 additions (the first onto +0 is
    exact, counted anyway) is within half an ulp of a value no larger than the
    result: at most 50 half-ulps, 25 ulps of the result, 25 * 2^-23 relative."""
    W = H = 9
    h = np.zeros(W * H, rtg.HIT_DTYPE)
    h["normal"] = (0.0, 0.0, 1.0)
    src = np.random.default_rng(5).uniform(0, 1, size=(H, W)).astype(F)
    for c in (1.0, 0.3, 1e-20, 3e20):
        var = np.full((H, W), c, F)
        for flags in (0, rtg.SVGF_LUMA):
            p = rtg.svgf_params(1, rtg.FILTER_GRAY, flags, 0.0, 0, 1e30, 1.0)
            _, vout = rtg.svgf_host(h, W, H, p, src, var)
            want = (70.0 / 256.0) ** 2 * float(F(c))
            err = np.abs(vout[2:-2, 2:-2].astype(np.float64) - want).max()
            assert err <= 25 * 2.0 ** -23 * want, (c, flags, err / want)
            assert (vout[0, 0] > vout[4, 4]), "a corner has fewer taps: less averaging"


# ---- 7. non-vacuity ----

@pytest.mark.parametrize("name", SCENES)
def test_inputs_and_calls_are_not_vacuous(rtg, name):
    W, H = FULL
    h = G.guides(name, W, H)
    real = h["id"] >= 0
    off, on = SVGF_SETS[2], SVGF_SETS[18 + 2]
    assert off[:2] == on[:2] == (5, ALL) and not off[4] and on[4]
    for kind in SIGNALS:
        a = S.want_svgf(name, W, H, kind, off)[0].reshape(W * H, -1)
        b = S.want_svgf(name, W, H, kind, on)[0].reshape(W * H, -1)
        changed = (a != b).any(-1)
        assert changed[real].sum() >= 0.1 * real.sum(), (kind, changed[real].mean())
        va, vb = S.want_svgf(name, W, H, kind, off)[1], S.want_svgf(name, W, H, kind, on)[1]
        assert (va[real] != vb[real]).any()
        src_var = S.canon(S.var_field(name, W, H))
        assert (va[real] != src_var[real]).mean() > 0.9 and (va[~real] == src_var[~real]).all()
    var = S.var_field(name, W, H)
    assert np.isnan(var[real]).sum() == 1 and np.isinf(var[real]).sum() == 1
    for kind in SIGNALS:
        acc, m2 = S.state(name, W, H, kind)
        assert np.isnan(m2[real]).any() and np.isinf(m2[real]).any() and np.isnan(acc[real]).any()
        below = (m2 < acc * acc).all(-1) & real
        assert below.sum() >= 9, "the 3 x 3 block below acc^2"
        temporal = S.want_variance(name, W, H, kind, "seeded", (ALL, 3, None, 0))
        assert (temporal[below] == 0).all() and (temporal[~real] == 0).all()
        assert (temporal[real] != 0).mean() > 0.9
        spatial = S.want_variance(name, W, H, kind, "seeded", (ALL, 3, None, 4))
        assert (spatial != temporal).any()
        # the four len fields take the branch they are meant to
        took = {}
        for which in S.LEN_FIELDS:
            facts = {}
            st = S.VAR_FEW[0]
            S.restate_variance(h, W, H, st, G.plane_scale(name, st[2]), acc, m2,
                               S.len_field(name, W, H, which), facts)
            took[which] = facts["spatial"]
        assert 0 < took["seeded"].sum() < real.sum()
        assert took["long"].sum() == 0
        assert (took["zero"] == real).all()
        assert took["one"].sum() == 1
        st = S.VAR_FEW[0]
        long_, one = (S.want_variance(name, W, H, kind, w, st) for w in ("long", "one"))
        assert (long_ == S.want_variance(name, W, H, kind, "seeded", (ALL, 3, None, 0))).all()
        assert ((long_ != one) & ~took["one"]).sum() == 0 and (long_ != one).sum() == 1
        assert (S.want_variance(name, W, H, kind, "zero", st) != long_).mean() > 0.2
    ln = S.len_field(name, W, H, "seeded")
    assert (ln[real] == 65535).any() and (ln[~real] != 0).any() and ln[real].min() == 0


# ---- 8. the host chain ----

def test_host_chain(rtg):
    h, acc, ln, m2, var, dst, dvar = S.chain_host()
    real = h["id"] >= 0
    c = S.CHAIN
    assert ln.max() == c["max_history"] and (ln.reshape(-1)[real] < c["min_history"]).all()
    assert np.isfinite(var).all() and (var.reshape(-1)[~real] == 0).all()
    assert (var.reshape(-1)[real] > 0).mean() > 0.2
    assert (_words(dst) != _words(acc)).any() and np.isfinite(dst).all()
    # the filter lowers the variance it carries on most of the surface pixels
    lower = dvar.reshape(-1)[real] <= var.reshape(-1)[real]
    assert lower.mean() > 0.9, lower.mean()
    p = S.chain_params(rtg)
    ref_var = S.restate_variance(h, c["W"], c["H"], (7, 3, None, c["min_history"]),
                                 G.plane_scale(c["name"], None), acc, m2, ln)
    assert (_words(var) == ref_var).all()
    st = (c["passes"], 7, 3, None, True, c["sigma"], c["eps"])
    ref = S.restate_svgf(h, c["W"], c["H"], st, G.plane_scale(c["name"], None), acc, var)
    assert (_words(dst) == ref[0]).all() and (_words(dvar) == ref[1]).all()
    assert int(p["svgf"]["flags"][0]) == 7 | rtg.SVGF_LUMA


# ---- 9. argument errors ----

def test_variance_argument_errors(rtg):
    R = rtg
    W, H = 8, 8
    n = W * H
    h = G.guides("reference", W, H)
    acc, m2 = S.state("reference", W, H, "gray")
    ln = S.len_field("reference", W, H, "seeded")
    ok = R.variance_params(R.FILTER_GRAY, ALL, 1.0, 3, 4)
    L = R.lib()
    out = np.zeros(n, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    okp = P(ok)
    cases = ((W, H, R.variance_params(R.FILTER_COUNT), "kind COUNT"),
             (W, H, R.variance_params(3), "kind 3"),
             (W, H, R.variance_params(1, 16), "unknown flags 0x10"),
             (W, H, R.variance_params(1, normal_log2=9), "normalLog2 9"),
             (W, H, R.variance_params(1, min_history=65536), "minHistory 65536"),
             (0, H, ok, "empty frame"), (W, 0, ok, "empty frame"),
             (1 << 16, 1 << 16, ok, "at most 2^32 - 1"))
    for w, hh, p, msg in cases:
        assert L.rtg_variance_host(P(h), w, hh, P(p), P(acc), P(m2), P(ln), P(out), 1) == -1
        text = L.rtg_last_error().decode()
        assert text.startswith("variance: ") and msg in text, text
    for args, msg in (((None, W, H, okp, P(acc), P(m2), P(ln), P(out), 1), "null hit buffer"),
                      ((P(h), W, H, okp, None, P(m2), P(ln), P(out), 1), "null acc"),
                      ((P(h), W, H, okp, P(acc), None, P(ln), P(out), 1), "null m2"),
                      ((P(h), W, H, okp, P(acc), P(m2), None, P(out), 1), "null len"),
                      ((P(h), W, H, okp, P(acc), P(m2), P(ln), None, 1), "null destination"),
                      ((P(h), W, H, None, P(acc), P(m2), P(ln), P(out), 1), "null params")):
        assert L.rtg_variance_host(*args) == -1
        assert L.rtg_last_error().decode() .startswith("variance: " + msg), L.rtg_last_error()
    # the destination's bytes may not touch an input's
    buf = np.zeros(2 * n, F)
    for args, msg in (((P(buf), P(m2), P(ln), P(buf[n - 1:])), "the destination overlaps the acc"),
                      ((P(acc), P(buf), P(ln), P(buf)), "the destination overlaps the m2"),
                      ((P(acc), P(m2), P(buf.view(np.uint16)[n - 1:]), P(buf)),
                       "the destination overlaps the len")):
        assert L.rtg_variance_host(P(h), W, H, okp, *args, 1) == -1
        assert L.rtg_last_error().decode() == "variance: " + msg
    assert L.rtg_variance_host(P(h), W, H, okp, P(buf), P(m2), P(ln), P(buf[n:]), 1) == 0  # adjacent
    assert L.rtg_variance_host(P(h), W, H, okp, P(acc), P(acc), P(ln), P(out), 1) == 0  # inputs may alias
    assert L.rtg_last_error() == b""
    with pytest.raises(ValueError):
        R.variance_host(h, W, H + 1, ok, acc, m2, ln)
    with pytest.raises(ValueError):
        R.variance_host(h, W, H, R.variance_params(R.FILTER_RGB), acc, m2, ln)


def test_svgf_argument_errors(rtg):
    R = rtg
    W, H = 8, 8
    n = W * H
    h, src = G.guides("reference", W, H), G.signal("reference", W, H, "gray")
    var = S.var_field("reference", W, H)
    ok = R.svgf_params(2, R.FILTER_GRAY, ALL | R.SVGF_LUMA, 1.0, 3)
    assert R.svgf_scratch(W, H, ok) == 2 * n * 4
    assert R.svgf_scratch(W, H, R.svgf_params(1)) == 0
    assert R.svgf_scratch(5, 1, R.svgf_params(8, R.FILTER_RGB)) == 64 + 32  # 60 and 20 bytes
    assert R.svgf_scratch(5, 1, R.svgf_params(3, R.FILTER_GRAY)) == 32 + 32
    cases = ((W, H, R.svgf_params(0, 1), "0 passes"),
             (W, H, R.svgf_params(9, 1), "9 passes"),
             (W, H, R.svgf_params(2, 1, normal_log2=9), "normalLog2 9"),
             (W, H, R.svgf_params(2, 3), "kind 3"),
             (W, H, R.svgf_params(2, R.FILTER_COUNT), "kind COUNT"),
             (W, H, R.svgf_params(2, 1, 32), "unknown flags 0x20"),
             (W, H, R.svgf_params(2, 1, 64 | 16), "unknown flags 0x40"),
             (0, H, ok, "empty frame"), (W, 0, ok, "empty frame"),
             (1 << 16, 1 << 16, ok, "at most 2\\^32 - 1"))
    for w, hh, p, msg in cases:
        with pytest.raises(R.RtgError, match="svgf_scratch: .*" + msg):
            R.svgf_scratch(w, hh, p)
    L = R.lib()
    out, vout = np.zeros(n, F), np.zeros(n, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    okp = P(ok)
    for w, hh, p, msg in cases:
        assert L.rtg_svgf_host(P(h), w, hh, P(p), P(src), P(var), P(out), P(vout), 1) == -1
        text = L.rtg_last_error().decode()
        assert text.startswith("svgf: ") and msg.replace("\\", "") in text, text
    full = (P(h), W, H, okp, P(src), P(var), P(out), P(vout), 1)
    for k, msg in ((0, "null hit buffer"), (3, "null params"), (4, "null source"),
                   (5, "null source variance"), (6, "null destination"),
                   (7, "null destination variance")):
        args = list(full)
        args[k] = None
        assert L.rtg_svgf_host(*args) == -1
        assert L.rtg_last_error().decode() == "svgf: " + msg, L.rtg_last_error()
    assert L.rtg_svgf_scratch(W, H, okp, None) == -1
    assert L.rtg_last_error().decode().startswith("svgf_scratch: null size")
    assert L.rtg_svgf_scratch(W, H, None, ctypes.byref(ctypes.c_size_t())) == -1
    assert L.rtg_last_error().decode().startswith("svgf_scratch: null params")
    # every pair with a written buffer in it
    buf = np.zeros(2 * n, F)
    a, b = P(buf), P(buf[n - 1:])
    for args, msg in (((a, P(var), b, P(vout)), "the destination overlaps the source"),
                      ((a, P(var), P(out), b), "the destination variance overlaps the source"),
                      ((P(src), a, b, P(vout)), "the destination overlaps the source variance"),
                      ((P(src), a, P(out), b), "the destination variance overlaps the source variance"),
                      ((P(src), P(var), a, b), "the destination variance overlaps the destination")):
        assert L.rtg_svgf_host(P(h), W, H, okp, *args, 1) == -1
        assert L.rtg_last_error().decode() == "svgf: " + msg
    assert L.rtg_svgf_host(P(h), W, H, okp, P(buf), P(var), P(buf[n:]), P(vout), 1) == 0  # adjacent
    assert L.rtg_svgf_host(P(h), W, H, okp, P(src), P(src), P(out), P(vout), 1) == 0  # inputs may alias
    assert L.rtg_last_error() == b""
    with pytest.raises(ValueError):
        R.svgf_host(h, W, H + 1, ok, src, var)
    with pytest.raises(ValueError):
        R.svgf_host(h, W, H, ok, src, var[:-1])
