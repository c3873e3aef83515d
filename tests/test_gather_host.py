"""CPU tests of the gather (rtg_gather*, include/rtg.h): no GPU.

  1. gather_rays_host equals a numpy float32 restatement of the probe ray, one
     operation a line, bit for bit, the jitter window and its wrap included;
  2. the definition: gather_host(walk 0) is the numpy fold, in the defined
     order, of raytrace_host(walk 0) over gather_rays_host's rays, word for
     word, with and without the skip flag, the skip counts too;
  3. the kernel's own path (walk 1) equals the plain loops (walk 0) on every
     path the scene tables select (aogen.PATHS), and on the hostile scenes;
  4. the result does not depend on nthreads;
  5. every argument check, with its message.

Tables, records, parameter sets and the plain-loop answers are gathergen.py's;
test_gpu_gather.py holds the device to the same answers.
"""
from __future__ import annotations

import numpy as np
import pytest

import aogen
import gathergen
import hostile
from gathergen import JITTER, SCENES, SKIP
from test_raytrace_host import THREADS


# ---- 1. the restatement ----

@pytest.mark.parametrize("k,nd", gathergen.PROBES)
def test_rays_equal_the_numpy_restatement(rtg, k, nd):
    for name in ("reference", "base150", "c5"):
        h = gathergen.hits(name)
        for flags in (0, JITTER):
            got = gathergen.want_rays(name, k, nd, flags)
            want = gathergen.restate_rays(h, gathergen.dirs(nd), k, gathergen.bias(name),
                                          gathergen.SEED, flags)
            assert got.shape == want.shape
            bad = np.argwhere(got.view(np.uint32) != gathergen.canon(want))
            assert not len(bad), (name, flags, len(bad), bad[0], got[bad[0][0]], want[bad[0][0]])
            assert not got[np.repeat(h["id"] < 0, k)].view(np.uint32).any()  # no point: zeros
            real = got[np.repeat(h["id"] >= 0, k)]
            ln = np.linalg.norm(real[:, 3:].astype(np.float64), axis=1)
            ok = np.isfinite(ln)
            assert ok.any() and (np.abs(ln[ok] - 1.0) < 1e-6).all()  # unit rays
    if nd >= 7:
        assert np.isnan(got).any()  # (the zero and NaN directions; the canonical NaN)
        assert gathergen.want_rays("reference", k, nd, 0).tobytes() != \
            gathergen.want_rays("reference", k, nd, JITTER).tobytes()


def test_tables_hold_what_they_should():
    for nd in (8, 97):
        w = gathergen.weights(nd)
        assert (w == 0).sum() == 1 and (w < 0).sum() == 1 and np.isnan(w).sum() == 1 and \
            np.isposinf(w).sum() == 1
    assert np.isfinite(gathergen.weights(97)[:16]).all() and (gathergen.weights(97)[:16] > 0).all()
    j = gathergen.window(aogen.N_POINTS, 97, 16, gathergen.SEED, JITTER)
    assert (j[:, -1] < j[:, 0]).any() and (j[:, -1] > j[:, 0]).any()  # windows that wrap
    assert np.isin([97 // 4, 97 // 2, 3 * 97 // 4, 96], j).all()  # ... and reach the special weights


# ---- 2. the definition ----

@pytest.mark.parametrize("name", SCENES)
def test_sums_are_the_fold_of_raytrace_over_the_rays(rtg, name):
    gathergen.assert_non_vacuous(name)
    sph, lg, h = gathergen.scene(name), gathergen.lights(name), gathergen.hits(name)
    for k, nd, flags, S, sem in gathergen.cases(name):
        rays = gathergen.want_rays(name, k, nd, flags)
        col = rtg.raytrace_host(sph, lg, rays, stack_size=S, semantics=sem, walk=0,
                                threads=THREADS)
        acc, skp = gathergen.fold(h, col, gathergen.weights(nd), k, gathergen.SEED, flags)
        want, want_skp = gathergen.want(name, k, nd, flags, S, sem)
        case = gathergen.case_id((k, nd, flags, S, sem))
        assert gathergen.same_words(want, acc) is None, (case, gathergen.same_words(want, acc))
        assert want.view(np.uint32).tobytes() == gathergen.canon(want).tobytes(), case
        assert want_skp.tobytes() == skp.tobytes(), case
        none = h["id"] < 0
        assert not want[none].view(np.uint32).any() and not want_skp[none].any(), case
        if not flags & SKIP:
            assert not want_skp.any(), case
        assert want_skp.max() <= k


def test_skip_flag_changes_only_the_records_it_counts(rtg):
    for name in ("reference", "c5"):
        plain, _ = gathergen.want(name, 16, 97, 0)
        kept, skp = gathergen.want(name, 16, 97, SKIP)
        same = (gathergen.canon(plain) == gathergen.canon(kept)).all(1)
        assert same[skp == 0].all(), name
        assert np.isfinite(kept).all(), name  # ordinary weights: what is left is finite
    assert (~same).any()  # c5


# ---- 3. walk 1 == walk 0 ----

@pytest.mark.parametrize("name", SCENES)
def test_kernel_path_equals_plain_loops(rtg, name):
    sph, lg, h = gathergen.scene(name), gathergen.lights(name), gathergen.hits(name)
    for k, nd, flags, S, sem in gathergen.cases(name):
        got, skp = rtg.gather_host(sph, lg, h, gathergen.dirs(nd), gathergen.weights(nd),
                                   gathergen.params(rtg, name, k, flags), stack_size=S,
                                   semantics=sem, walk=1, threads=THREADS, skipped=True)
        want, want_skp = gathergen.want(name, k, nd, flags, S, sem)
        case = gathergen.case_id((k, nd, flags, S, sem))
        assert gathergen.same_words(got, want) is None, (case, gathergen.same_words(got, want))
        assert got.view(np.uint32).tobytes() == gathergen.canon(got).tobytes(), case
        assert skp.tobytes() == want_skp.tobytes(), case


@pytest.mark.parametrize("n", hostile.SIZES)
def test_kernel_path_equals_plain_loops_on_hostile_scenes(rtg, n):
    """Every hostile.CASES mutation of size n, the batch test_gpu_gather.py runs."""
    for name in hostile.NAMES:
        sph, lg = hostile.mutated(n, name)
        h = aogen.hostile_hits(n, name)
        assert (h["id"] >= 0).any() and (h["id"] < 0).any()
        for flags in (0, JITTER | SKIP):
            p = rtg.gather_params(7, aogen.BIAS, gathergen.SEED, flags)
            a = [rtg.gather_host(sph, lg, h, gathergen.dirs(8), gathergen.weights(8), p,
                                 stack_size=6, walk=w, threads=THREADS, skipped=True)
                 for w in (0, 1)]
            assert gathergen.same_words(a[1][0], a[0][0]) is None, \
                (name, flags, gathergen.same_words(a[1][0], a[0][0]))
            assert a[1][1].tobytes() == a[0][1].tobytes(), (name, flags)


# ---- 4. threads ----

def test_result_does_not_depend_on_threads(rtg):
    name = "base65"
    for walk in (0, 1):
        for nthreads in (1, 3):
            got, skp = rtg.gather_host(gathergen.scene(name), gathergen.lights(name),
                                       gathergen.hits(name), gathergen.dirs(8),
                                       gathergen.weights(8),
                                       gathergen.params(rtg, name, 7, JITTER | SKIP), walk=walk,
                                       threads=nthreads, skipped=True)
            want, want_skp = gathergen.want(name, 7, 8, JITTER | SKIP)
            assert gathergen.same_words(got, want) is None, (walk, nthreads)
            assert skp.tobytes() == want_skp.tobytes(), (walk, nthreads)
    one = rtg.gather_rays_host(gathergen.hits(name), gathergen.dirs(8),
                               gathergen.params(rtg, name, 7, JITTER), threads=1)
    assert one.tobytes() == gathergen.want_rays(name, 7, 8, JITTER).tobytes()


# ---- 5. argument checks ----

def test_argument_errors(rtg):
    L = rtg.lib()
    sph, lg = gathergen.scene("reference"), gathergen.lights("reference")
    h = gathergen.hits("reference").copy()
    d = gathergen.dirs(8).copy()
    w = gathergen.weights(8).copy()
    out = np.zeros((len(h), 3), np.float32)
    skp = np.zeros(len(h), np.uint16)
    rays = np.zeros((len(h) * 7, 6), np.float32)
    P = rtg._ptr
    ok = rtg.gather_params(7, 1e-3)

    def opt(a):
        return P(a) if a is not None else None

    def host(hits=h, n=len(h), p=ok, dirs=d, wt=w, nd=8, S=6, sem=0, dst=out, sk=skp, walk=0,
             spheres=sph):
        return L.rtg_gather_host(opt(spheres), len(sph), P(lg), len(lg), opt(hits), n, opt(p),
                                 opt(dirs), opt(wt), nd, S, sem, opt(dst), opt(sk), walk, 1)

    def gen(hits=h, n=len(h), p=ok, dirs=d, nd=8, dst=rays):
        return L.rtg_gather_rays_host(opt(hits), n, opt(p), opt(dirs), nd, opt(dst), 1)

    def bad(rc, msg):
        assert rc == -1
        text = L.rtg_last_error().decode()
        assert text and msg in text, text

    assert host() == 0 and gen() == 0 and L.rtg_last_error() == b""
    assert out.any() and rays.any()
    assert host(sk=None) == 0  # the counts are optional
    out[:] = 0
    rays[:] = 0
    for call in (host, gen):
        bad(call(hits=None), "null hit buffer")
        bad(call(p=None), "null params")
        bad(call(dirs=None), "null direction table")
        bad(call(dst=None), "null output buffer")
        bad(call(p=rtg.gather_params(0)), "0 samples")
        bad(call(p=rtg.gather_params(1025), nd=2000), "1025 samples")
        bad(call(nd=6), "6 directions")
        bad(call(nd=65537), "65537 directions")
        bad(call(p=rtg.gather_params(7, flags=4)), "unknown flags 0x4")
        bad(call(p=rtg.gather_params(7, flags=0x80000001)), "unknown flags")
        bad(call(n=1 << 32), "points (at most 2^32 - 1)")
        assert call(n=0) == 0
    bad(gen(n=1 << 62, p=rtg.gather_params(1024), nd=1024), "overflows size_t")
    bad(host(wt=None), "null weight table")
    bad(host(S=0), "stackSize 0")
    bad(host(S=17), "stackSize 17")
    bad(host(sem=2), "semantics 2")
    bad(host(walk=2), "walk 2")
    bad(host(spheres=None), "null scene array")
    assert not out.any() and not rays.any()  # nothing was written by a refused call
    with pytest.raises(rtg.RtgError, match="samples"):
        rtg.gather_host(sph, lg, h, d, w, rtg.gather_params(9))  # K above nDirs, through the binding
    with pytest.raises(rtg.RtgError, match="weights"):
        rtg.gather_host(sph, lg, h, d, w[:7], ok)


def test_empty_batch(rtg):
    sph, lg = gathergen.scene("reference"), gathergen.lights("reference")
    p = rtg.gather_params(7)
    empty = np.zeros(0, rtg.HIT_DTYPE)
    out, skp = rtg.gather_host(sph, lg, empty, gathergen.dirs(8), gathergen.weights(8), p,
                               skipped=True)
    assert out.shape == (0, 3) and skp.shape == (0,)
    assert rtg.gather_rays_host(empty, gathergen.dirs(8), p).shape == (0, 6)
