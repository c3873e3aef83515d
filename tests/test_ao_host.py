"""CPU tests of ambient occlusion (rtg_ao*, include/rtg.h): no GPU.

  1. the definition: the per-point sum of visible_host(walk 0) over
     ao_segments_host's segments is ao_host(walk 0), word for word;
  2. ao_segments_host equals a numpy float32 restatement of the segment
     arithmetic bit for bit, the jitter window and its wrap-around included;
  3. the kernel's own path (walk 1) equals the plain loops (walk 0) on every
     path the scene tables select (aogen.SCENES);
  4. every argument check, with its message;
  5. rtg_ao_directions: the upper hemisphere, unit length, the cosine weight.

Tables, records, parameter sets and the plain-loop answers are aogen.py's;
test_gpu_ao.py holds the device to the same answers.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import aogen
import hostile
from aogen import SCENES, SET_IDS, SETS
from test_raytrace_host import THREADS


def _first_bad(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return None if not len(bad) else f"{len(bad)} differ, first at {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


# ---- 1. the definition ----

@pytest.mark.parametrize("name", SCENES)
def test_counts_are_the_sum_of_visible_over_the_segments(rtg, name):
    aogen.assert_non_vacuous(name)
    sph = aogen.scene(name)
    for k, nd, flags in SETS:
        segs = aogen.want_segments(name, k, nd, flags)
        vis = rtg.visible_host(sph, segs, walk=0, threads=THREADS)
        folded = vis.reshape(aogen.N_POINTS, k).sum(1).astype(np.uint16)
        want = aogen.want(name, k, nd, flags)
        assert folded.tobytes() == want.tobytes(), (k, nd, flags, _first_bad(folded, want))
        assert (want[aogen.hits(name)["id"] < 0] == k).all()  # no point: K, no query
        assert want.max() <= k


def test_batches_hold_what_they_should():
    """Hits and misses in every wave, the hand-made records, the special
    directions, windows that wrap and a seed + i that wraps."""
    for name in SCENES:
        h = aogen.hits(name)
        for w0 in (0, 64, 128):
            ids = h["id"][w0:w0 + 64]
            assert (ids >= 0).any() and (ids < 0).any(), (name, w0)
        assert h[1]["id"] == -1 and np.isnan(h[1]["normal"]).all()
        assert tuple(h[2]["normal"]) == (0.0, 0.0, -1.0) and h[2]["id"] >= 0
    for nd in (7, 8, 97):
        d = aogen.dirs(nd)
        ln = np.linalg.norm(d.astype(np.float64), axis=1)
        assert (ln == 0).sum() == 1 and np.isnan(ln).sum() == 1 and (np.abs(ln - 1e3) < 1).sum() == 1
    i = np.arange(aogen.N_POINTS, dtype=np.uint64)
    assert ((np.uint64(aogen.SEED) + i) >> np.uint64(32)).any()
    s = aogen.mix32(np.uint64(aogen.SEED) + i) % np.uint64(8)
    assert (s + np.uint64(6) >= 8).any() and (s + np.uint64(6) < 8).any()


# ---- 2. the restatement ----

@pytest.mark.parametrize("k,nd,flags", SETS, ids=SET_IDS)
def test_segments_equal_the_numpy_restatement(rtg, k, nd, flags):
    for name in ("reference", "base150"):
        h = aogen.hits(name)
        got = aogen.want_segments(name, k, nd, flags)
        want = aogen.restate_segments(h, aogen.dirs(nd), k, aogen.radius(name), aogen.BIAS,
                                      aogen.SEED, flags)
        assert got.shape == want.shape
        bad = np.argwhere(got.view(np.uint32) != aogen.canon(want))
        assert not len(bad), (name, len(bad), bad[0], got[bad[0][0]], want[bad[0][0]])
        assert not got[np.repeat(h["id"] < 0, k)].view(np.uint32).any()  # no point: zeros
    if nd >= 7:
        assert np.isnan(got).any()  # (the NaN direction; its words are the canonical NaN)


def test_jitter_changes_the_windows(rtg):
    a = aogen.want_segments("reference", 7, 8, 0)
    b = aogen.want_segments("reference", 7, 8, 1)
    assert a.tobytes() != b.tobytes()
    assert aogen.want_segments("reference", 1, 1, 0).tobytes() == \
        aogen.want_segments("reference", 1, 1, 1).tobytes()  # one direction: one window


# ---- 3. walk 1 == walk 0 ----

@pytest.mark.parametrize("name", SCENES)
def test_kernel_path_equals_plain_loops(rtg, name):
    sph = aogen.scene(name)
    for k, nd, flags in SETS:
        got = rtg.ao_host(sph, aogen.hits(name), aogen.dirs(nd), aogen.params(rtg, name, k, flags),
                          walk=1, threads=THREADS)
        want = aogen.want(name, k, nd, flags)
        assert got.tobytes() == want.tobytes(), (k, nd, flags, _first_bad(got, want))


@pytest.mark.parametrize("n", hostile.SIZES)
def test_kernel_path_equals_plain_loops_on_hostile_scenes(rtg, n):
    """Every hostile.CASES mutation of size n, the batch test_gpu_ao.py runs."""
    radius = float(np.float32(2.5 * np.abs(hostile.base(n)[0]["radius"]).max()))
    for name in hostile.NAMES:
        sph, _ = hostile.mutated(n, name)
        h = aogen.hostile_hits(n, name)
        assert (h["id"] >= 0).any() and (h["id"] < 0).any()
        for flags in (0, 1):
            p = rtg.ao_params(7, radius, aogen.BIAS, aogen.SEED, flags)
            want = rtg.ao_host(sph, h, aogen.dirs(8), p, walk=0, threads=THREADS)
            got = rtg.ao_host(sph, h, aogen.dirs(8), p, walk=1, threads=THREADS)
            assert got.tobytes() == want.tobytes(), (name, flags, _first_bad(got, want))


def test_result_does_not_depend_on_threads(rtg):
    p = aogen.params(rtg, "base65", 7, 1)
    one = rtg.ao_host(aogen.scene("base65"), aogen.hits("base65"), aogen.dirs(8), p, walk=1, threads=1)
    assert one.tobytes() == aogen.want("base65", 7, 8, 1).tobytes()


# ---- 4. argument checks ----

def test_argument_errors(rtg):
    L = rtg.lib()
    sph = aogen.scene("reference")
    h = aogen.hits("reference").copy()
    d = aogen.dirs(8).copy()
    out = np.zeros(len(h), np.uint16)
    segs = np.zeros((len(h) * 7, 6), np.float32)
    P = rtg._ptr
    ok = rtg.ao_params(7, 1.0)

    def host(hits=h, n=len(h), p=ok, dirs=d, nd=8, dst=out, walk=0, spheres=sph):
        return L.rtg_ao_host(P(spheres) if spheres is not None else None, len(sph),
                             P(hits) if hits is not None else None, n,
                             P(p) if p is not None else None, P(dirs) if dirs is not None else None,
                             nd, P(dst) if dst is not None else None, walk, 1)

    def seg(hits=h, n=len(h), p=ok, dirs=d, nd=8, dst=segs):
        return L.rtg_ao_segments_host(P(hits) if hits is not None else None, n,
                                      P(p) if p is not None else None,
                                      P(dirs) if dirs is not None else None, nd,
                                      P(dst) if dst is not None else None, 1)

    def bad(rc, msg):
        assert rc == -1
        text = L.rtg_last_error().decode()
        assert text and msg in text, text

    assert host() == 0 and seg() == 0 and L.rtg_last_error() == b""
    assert out.any() and segs.any()
    out[:] = 0
    segs[:] = 0
    for call in (host, seg):
        bad(call(hits=None), "null hit buffer")
        bad(call(p=None), "null params")
        bad(call(dirs=None), "null direction table")
        bad(call(dst=None), "null output buffer")
        bad(call(p=rtg.ao_params(0, 1.0)), "0 samples")
        bad(call(p=rtg.ao_params(1025, 1.0), nd=2000), "1025 samples")
        bad(call(nd=6), "6 directions")
        bad(call(nd=65537), "65537 directions")
        bad(call(p=rtg.ao_params(7, 1.0, flags=2)), "unknown flags 0x2")
        bad(call(p=rtg.ao_params(7, 1.0, flags=0x80000001)), "unknown flags")
        bad(call(n=1 << 32), "points (at most 2^32 - 1)")
        assert call(n=0) == 0
    bad(seg(n=1 << 62, p=rtg.ao_params(1024, 1.0), nd=1024), "overflows size_t")
    bad(host(walk=2), "walk 2")
    bad(host(spheres=None), "null scene array")
    assert not out.any() and not segs.any()  # nothing was written by a refused call
    bad(L.rtg_ao_directions(8, None), "null table")
    bad(L.rtg_ao_directions(0, P(d)), "0 directions")
    bad(L.rtg_ao_directions(65537, P(d)), "65537 directions")
    with pytest.raises(rtg.RtgError, match="samples"):
        rtg.ao_host(sph, h, d, rtg.ao_params(9, 1.0))  # K above nDirs, through the binding


def test_empty_batch(rtg):
    sph = aogen.scene("reference")
    p = rtg.ao_params(7, 1.0)
    empty = np.zeros(0, rtg.HIT_DTYPE)
    assert rtg.ao_host(sph, empty, aogen.dirs(8), p).shape == (0,)
    assert rtg.ao_segments_host(empty, aogen.dirs(8), p).shape == (0, 6)


# ---- 5. the convenience table ----

@pytest.mark.parametrize("nd", [16, 64, 1024])
def test_directions(rtg, nd):
    d = rtg.ao_directions(nd).astype(np.float64)
    assert d.shape == (nd, 3)
    assert (d[:, 2] > 0).all()
    assert (np.abs(np.linalg.norm(d, axis=1) - 1.0) <= 1e-6).all()
    # the midpoint sum of the monotone sqrt(1 - u) on [0, 1] against its integral 2/3
    assert abs(d[:, 2].mean() - 2.0 / 3.0) <= 1.0 / (2 * nd) + 1e-6
    raw = np.zeros((nd + 4, 3), np.float32)
    assert rtg.lib().rtg_ao_directions(nd, ctypes.c_void_p(raw.ctypes.data)) == 0
    assert not raw[nd:].any() and raw[:nd].tobytes() == rtg.ao_directions(nd).tobytes()
