"""CPU tests of the large-size tests' own arithmetic (largegen.py): which
elements test_gpu_large.py pulls back to the host, how it splits a batch, and
that each of its shapes crosses the thresholds it is there to cross.  Also a
numpy restatement of the kernels' divmod_u64 (rtg_trace_kernels.h), to show
both of its correction branches taken on the CPU.  No GPU calls.
"""
from __future__ import annotations

import numpy as np
import pytest

import largegen
from largegen import BYTE_LIMIT, WINDOW, WORD_LIMIT, cuts, windows
from test_camera_host import cam12, restate_rays


def test_windows_of_a_small_buffer():
    assert windows(100, 24) == [(0, 100)]
    assert windows(WINDOW, 4) == [(0, WINDOW)]
    assert windows(3 * WINDOW, 32) == [(0, WINDOW), (2 * WINDOW, 3 * WINDOW)]
    assert windows(2 * WINDOW - 1, 32) == [(0, 2 * WINDOW - 1)]  # overlapping ends merge


@pytest.mark.parametrize("stride", [1, 2, 4, 8, 12, 24, 32])
def test_windows_straddle_the_thresholds(stride):
    n = 3 * WORD_LIMIT // stride * 4 // 3 + 12345  # a little past word 2^31, ragged
    assert n * stride > 4 * WORD_LIMIT
    w = windows(n, stride)
    assert w[0] == (0, WINDOW) and w[-1] == (n - WINDOW, n)
    assert len(w) == 4 and all(hi - lo == WINDOW for lo, hi in w)
    assert all(a[1] <= b[0] for a, b in zip(w, w[1:]))
    for limit, (lo, hi) in ((BYTE_LIMIT, w[1]), (4 * WORD_LIMIT, w[2])):
        # the element that ends at or before the limit and the one that holds it
        assert lo * stride < limit <= (hi - 1) * stride
        assert (limit - 1) // stride in range(lo, hi) and limit // stride in range(lo, hi)
        assert limit // stride - lo == WINDOW // 2
    # a buffer that ends before a threshold has no window there
    short = BYTE_LIMIT // stride
    assert short * stride <= BYTE_LIMIT
    assert windows(short, stride) == [(0, WINDOW), (short - WINDOW, short)]
    # one element more: the threshold's window lies within the last one
    assert windows(short + 1, stride) == [(0, WINDOW), (short + 1 - WINDOW, short + 1)]


def test_windows_of_several_strides():
    n = largegen.N_RAYS
    w = largegen.windows_of(n, [24, 32, 12])
    assert w == sorted(w) and all(a[1] < b[0] for a, b in zip(w, w[1:]))
    for s in (24, 32, 12):
        for lo, hi in windows(n, s):
            assert any(a <= lo and hi <= b for a, b in w)
    assert sum(hi - lo for lo, hi in w) <= 9 * WINDOW


@pytest.mark.parametrize("name", sorted(largegen.SHAPES))
def test_shapes_cross_what_they_claim(name):
    n, stride, byte32, word31 = largegen.SHAPES[name]
    assert n <= 0xFFFFFFFF, "the documented limit of a device call"
    assert (n * stride > BYTE_LIMIT) == byte32
    assert (n * stride > 4 * WORD_LIMIT) == word31
    assert n * stride <= 12 * largegen.GIB
    w = windows(n, stride)
    held = lambda e: any(lo <= e < hi for lo, hi in w)  # noqa: E731
    assert held(0) and held(n - 1)
    for limit, crossed in ((BYTE_LIMIT, byte32), (4 * WORD_LIMIT, word31)):
        if crossed:  # the elements on both sides of it
            assert held((limit - 1) // stride) and held(limit // stride)


def test_shapes_are_the_smallest_that_cross():
    W = largegen.RENDER_W
    assert W % 2 == 1 and W & (W - 1) and (W * 12) % 64
    assert W * 21845 * 12 > 4 * WORD_LIMIT >= W * 21843 * 12  # within two rows of it
    assert W * 10923 * 12 > BYTE_LIMIT >= W * 10921 * 12
    assert W * 4097 * 32 > BYTE_LIMIT >= W * 4095 * 32
    assert largegen.N_RAYS * 24 > 4 * WORD_LIMIT >= largegen.RAYS_W * (largegen.RAYS_H - 1) * 24
    assert largegen.N_RAYS * 12 > BYTE_LIMIT
    assert largegen.N_POINTS * 32 > BYTE_LIMIT >= (largegen.N_POINTS - 64) * 32
    assert largegen.N_POINTS % 64 == 0 and largegen.N_POINTS < largegen.N_RAYS
    probes = largegen.N_PROBE_POINTS * largegen.PROBE_K
    assert probes * 24 > BYTE_LIMIT and probes <= 0xFFFFFFFF
    assert largegen.N_PROBE_POINTS * 32 < BYTE_LIMIT // 16  # crossed through n * K alone
    assert largegen.N_ORDER * 24 > BYTE_LIMIT >= (largegen.N_ORDER - 128) * 24
    F = largegen.FILTER_W
    assert F % 2 == 1 and F * 8192 * 32 > BYTE_LIMIT and F * 21846 * 12 > BYTE_LIMIT
    assert F * 21841 * 12 <= BYTE_LIMIT  # within five rows of it
    v = largegen.VIEW_W * largegen.VIEW_W * 12
    assert 5 * v < BYTE_LIMIT < 6 * v and largegen.VIEWS == 7  # view 5 straddles byte 2^32


@pytest.mark.parametrize("n,stride", [(largegen.N_RAYS, 32), (largegen.N_RAYS, 24),
                                      (largegen.N_POINTS, 32), (21845, largegen.RENDER_W * 12),
                                      (10923, largegen.RENDER_W * 12), (1000, 4),
                                      (largegen.N_PROBE_POINTS, 24 * largegen.PROBE_K)])
def test_cuts(n, stride):
    b = cuts(n, stride)
    assert b[0] == 0 and b[-1] == n and len(b) >= 3
    assert all(lo < hi and (hi - lo) * stride < BYTE_LIMIT for lo, hi in zip(b, b[1:]))
    assert b[1] % 64 == 37
    assert len(b) - 1 <= max(2, n * stride // (BYTE_LIMIT - 65 * stride) + 1)
    b3 = cuts(n, stride, least=3)
    assert len(b3) >= 4 and b3[-1] == n


def test_threshold_rows():
    W = largegen.RENDER_W
    rows = largegen.threshold_rows(W, 21845, 12)
    r32, r33 = BYTE_LIMIT // 12 // W, 4 * WORD_LIMIT // 12 // W
    assert list(rows) == [0, r32 - 1, r32, r32 + 1, r33, 21844]
    assert r32 * W * 12 <= BYTE_LIMIT < (r32 + 1) * W * 12
    assert r33 * W * 12 <= 4 * WORD_LIMIT < (r33 + 1) * W * 12
    assert list(largegen.threshold_rows(64, 48, 12)) == [0, 47]


@pytest.mark.parametrize("W,H,zoom", [(37, 29, -4.0), (64, 48, 2.5)])
def test_rays_at_equals_the_restatement(rtg, W, H, zoom):
    """largegen.rays_at at chosen pixels is test_camera_host.restate_rays of
    the frame at those pixels, and the library's host generator."""
    cam = cam12(rtg.camera_look_at([0.5, 0.25, 1.0], [0.0, 0.0, -20.0]))
    whole, nS = restate_rays(cam, W, H, 1.0, zoom)
    assert nS == 1
    pix = np.random.default_rng(5).permutation(W * H)[:300]
    got = largegen.rays_at(cam, W, H, zoom, pix)
    assert got.tobytes() == whole[pix].tobytes()
    rows = np.array([H - 1, 0, 7])
    some, _ = restate_rays(cam, W, H, 1.0, zoom, rows=rows)
    assert some.tobytes() == whole.reshape(H, W, 6)[rows].tobytes()
    lib = rtg.camera_rays_host(cam, W, H, zoom, 1.0)
    assert largegen.canon_words(lib).tobytes() == largegen.canon_words(whole).tobytes()


def _divmod_u64(a, d):
    """divmod_u64 of rtg_trace_kernels.h in numpy: (q, r, the estimate's error)."""
    a, d = np.asarray(a, np.uint64), np.asarray(d, np.uint64)
    invd = 1.0 / d.astype(np.float64)
    qq = (a.astype(np.float64) * invd).astype(np.uint64)
    rr = (a - qq * d).astype(np.int64)
    low, high = rr >= d.astype(np.int64), rr < 0
    qq = qq + low.astype(np.uint64) - high.astype(np.uint64)
    rr = rr - np.where(low, d, 0).astype(np.int64) + np.where(high, d, 0).astype(np.int64)
    return qq, rr.astype(np.uint64), low, high


def test_divmod_restatement_takes_both_corrections():
    """a = q d takes the upward correction (RN(1 / d) below 1 / d puts the
    estimate just under q), at a frame's width d and a large q and, less often,
    at the small q of the suite's other frames too; a = q d + d - 1 takes the
    downward one only once a is near 2^53, d large with it.  One correction is
    enough everywhere."""
    rng = np.random.default_rng(11)
    n = 1 << 18
    d = rng.integers(1, 1 << 17, n, dtype=np.uint64)
    q = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64)
    big = rng.integers(1 << 21, 1 << 32, n, dtype=np.uint64)
    top = ((1 << 53) - big) // big  # the largest q with q d + d - 1 < 2^53
    cases = ((d, q, np.zeros(n, np.uint64), True, False),
             (big, top - rng.integers(0, 1 << 10, n, dtype=np.uint64), big - 1, False, True))
    for dd, qq, r, up, down in cases:
        a = qq * dd + r
        assert int(a.max()) < 1 << 53 and int(qq.max()) < 1 << 32
        gq, gr, low, high = _divmod_u64(a, dd)
        assert (gq == a // dd).all() and (gr == a % dd).all()
        assert (low.sum() > n // 100) == up and (high.sum() > n // 100) == down
        assert low.sum() == 0 or up
        assert high.sum() == 0 or down
    q = rng.integers(0, 1 << 13, n, dtype=np.uint64)  # the suite's frame heights
    for r in (np.zeros(n, np.uint64), d - 1):
        gq, gr, low, high = _divmod_u64(q * d + r, d)
        assert (gq == q).all() and (gr == r).all()
        assert high.sum() == 0 and (low.sum() > 0) == (r[0] == 0)
