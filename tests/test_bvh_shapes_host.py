"""CPU tests over the structured scenes of tests/bvhgen.py: trees at the depth
limit, the finite scenes build_bvh refuses, exact ties across subtrees,
lattices and 256 lights.  No GPU:

  1. what the builders make of each scene (hostsim_bvh_stats): the
     precondition of everything below and of test_gpu_bvh_shapes.py;
  2. the kernel's traversal compiled for the host (tests/hostsim, the sample
     and the tile kernel's variants) equals the oracle's frame, and BvhStack
     never holds more than 3 * depth + 3 of its 64 entries;
  3. the batch and point queries' kernel path (walk 1) equals the plain loops
     (walk 0), byte for byte, the gather with its skip counts among them;
  4. the posed camera's walk 1 equals walk 0, from outside and from within,
     and so do the views folded into coefficients.

test_gpu_bvh_shapes.py holds the device to the same references.
"""
from __future__ import annotations

import numpy as np
import pytest

import aogen
import bvhgen as G
from conftest import bits_equal, first_mismatch
from raygen import diff_hits
from test_oracle import _hostsim_render, hostsim  # noqa: F401  (the fixture)

THREADS = G.THREADS


# ---- 1. the builders ----

def test_builder_facts(hostsim, rtg):  # noqa: F811
    """deep19 is 19 deep and deep20 exactly 20, the limit; one more shell and
    100 coincident records are refused (trees 23 and 50 deep) although every
    sphere is finite; C5 under 256 lights keeps its tree and loses its lists."""
    st = {name: G.bvh_stats(hostsim, name) for name in G.NAMES}
    for name, depth in G.DEPTH.items():
        if depth is None:
            assert not st[name]["built"] and st[name]["nodes"] == 0, (name, st[name])
            assert st[name]["depth"] > 20 and not st[name]["lists"], (name, st[name])
            assert len(G.scene(name)[0]) > 64 and np.isfinite(G.scene(name)[0]["radius"]).all()
        else:
            assert st[name]["built"] and st[name]["depth"] == depth, (name, st[name])
    for name in G.NAMES:
        if G.DEPTH.get(name, 0) is not None:
            assert st[name]["built"] and st[name]["nodes"] > 0, (name, st[name])
    assert len(G.scene("refused")[0]) == len(G.scene("deep20")[0]) + 1
    assert st["many_lights"]["built"] and not st["many_lights"]["lists"], st["many_lights"]
    own = G.bvh_stats(hostsim, G.c5())
    assert own["built"] and own["lists"] and own["nodes"] == st["many_lights"]["nodes"]
    for name in G.NAMES:
        if name != "many_lights" and st[name]["built"]:
            assert st[name]["lists"], (name, st[name])
    for name in G.LATTICES:
        assert len(G.scene(name)[0]) == 125
    for name in G.MIRRORS:
        assert len(G.scene(name)[0]) >= 2 * G.PAIRS


def test_mirror_scenes_are_mirrored(rtg):
    for name, axis in G.MIRRORS.items():
        sph = G.scene(name)[0]
        a, b = sph[:G.PAIRS], sph[G.PAIRS:2 * G.PAIRS]
        flip = a["pos"].copy()
        flip[:, axis] = -flip[:, axis]
        assert (flip == b["pos"]).all() and (a["radius"] == b["radius"]).all()
        assert (a["radius"] > np.abs(a["pos"][:, axis])).all()  # r > a: the two overlap
        low_side = np.sign(a["pos"][:, axis])
        assert (low_side == (-1 if name.endswith("swapped") else 1)).all()


# ---- 2. hostsim == oracle, and the stack bound ----

@pytest.mark.parametrize("name", G.NAMES)
def test_kernel_traversal_equals_oracle(hostsim, oracle, rtg, name):  # noqa: F811
    sph, lg = G.scene(name)
    st = G.bvh_stats(hostsim, name)
    w, h, runs = G.frame_args(name)
    G.stack_marks(hostsim)
    try:
        for variant in (0, 9):
            hostsim.hostsim_set_variant(variant)
            for aa, s in runs:
                want = G.oracle_frame(oracle, name, w, h, s, aa)
                got = _hostsim_render(hostsim, sph, lg, w, h, s, aa=aa)
                assert bits_equal(got, want), (variant, s, aa, first_mismatch(got, want))
    finally:
        hostsim.hostsim_set_variant(0)
    high, overflow = G.stack_marks(hostsim)
    assert not overflow, "a push with all 64 entries in use"
    # one sibling triple waits per level above the visited node, whose own
    # pushes come on top: at most 3 * depth + 3 entries, 63 at the depth limit
    if st["built"]:
        assert 0 < high <= 3 * st["depth"] + 3 <= 63, (high, st)
    else:
        assert high == 0, high  # the flat queries: no stack


def test_wide_deep_fills_the_stack_further_than_the_other_scenes(hostsim, oracle, rtg):  # noqa: F811
    """The high-water marks bvhgen.py's docstring quotes, at 32 x 24, aa 1, S 6
    (C5 and base150 at 48 x 27, aa 1, S 8 too, the frame the 13 was first seen on)."""
    import hostile

    def mark(scene, w=32, h=24, s=6):
        G.stack_marks(hostsim)
        _hostsim_render(hostsim, *scene, w, h, s, aa=1.0)
        high, overflow = G.stack_marks(hostsim)
        assert not overflow
        return high
    wide = mark(G.scene("wide_deep"))
    others = [mark(G.c5()), mark(G.c5(), 48, 27, 8), mark(hostile.base(150)),
              mark(hostile.base(150), 48, 27, 8)]
    assert wide == G.WIDE_HIGH_WATER and others == list(G.OTHER_HIGH_WATER), (wide, others)
    assert wide > max(others)
    assert wide <= 3 * G.bvh_stats(hostsim, "wide_deep")["depth"] + 3


# ---- 3. walk 1 == walk 0 ----

@pytest.mark.parametrize("name", G.NAMES)
def test_walk1_equals_walk0(rtg, name):
    """Seeded defects, each built into a scratch copy of rtg_trace.h and run
    against this module:

    take_closer without its tie clause (`t < minT` alone).  All 2000 in-plane
    rays of mirror_x, of mirror_y and of mirror_z differ from the plain loops
    (the lower index on the positive side: the octant copy of a ray with a
    zero component puts the negative side first, so the higher index is met
    first and kept), and not one in-plane ray of mirror_x_swapped does: one
    index order of the two sees it.  mirror_x_swapped still fails on one ray
    of the raygen mix, as do wide_deep, lattice_kiss, lattice_overlap and
    many_lights (other ties, 11 rays outside the plane in mirror_x).  Of the
    frames, those of mirror_x and mirror_y differ from the oracle, those of
    mirror_x_swapped and mirror_z do not.

    slab_pass with `tn < tf`: nothing here fails.  Entry equals exit only
    where a ray meets a box in one point, on an edge or with its reach ending
    on the entry plane; every box is grown past its spheres, so no root lies
    there, and no scene of this module aims a ray at a box edge exactly.

    beyond with the reach shortened to 0.99 of it: this test fails on
    wide_deep, the four mirror scenes, the three lattices and many_lights,
    the oracle frame of wide_deep and the posed camera of mirror_z and
    many_lights."""
    sph, lg = G.scene(name)
    rays, segs = G.batches(name)
    G.check_non_vacuous(name)
    hits, vis = G.walk0(name)
    got = rtg.intersect_host(sph, rays, walk=1, threads=THREADS)
    assert got.tobytes() == hits.tobytes(), diff_hits(got, hits)
    got = rtg.visible_host(sph, segs, walk=1, threads=THREADS)
    bad = np.flatnonzero(got != vis)
    assert not len(bad), f"{len(bad)} segments differ, first {bad[0]}: {segs[bad[0]]}"
    for sem in ((0, 1) if name in ("mirror_x", "deep19") else (0,)):
        want = G.colours0(name, sem)
        got = rtg.raytrace_host(sph, lg, G.trace_rays(name), stack_size=G.trace_stack(name),
                                semantics=sem, walk=1, threads=THREADS)
        assert got.tobytes() == want.tobytes(), (sem, first_mismatch(got, want))
        assert (want.view(np.uint32) << 1).any(), "black batch"


@pytest.mark.parametrize("name", G.NAMES)
def test_point_queries_walk1_equals_walk0(rtg, name):
    sph, lg = G.scene(name)
    h = G.hits(name)
    assert (h["id"] >= 0).sum() >= 200
    for flags in (0, rtg.AO_JITTER):
        want = G.ao0(name, flags)
        got = rtg.ao_host(sph, h, aogen.dirs(G.AO_DIRS), G.ao_params(rtg, name, flags), walk=1,
                          threads=THREADS)
        assert got.tobytes() == want.tobytes(), (flags, int((got != want).sum()))
    real = h["id"] >= 0
    assert 0 < int((G.ao0(name, 0)[real] < G.AO_K).sum()), "no probe is blocked"
    want, lit = G.matte0(name)
    got, got_lit = rtg.matte_host(sph, lg, h, walk=1, threads=THREADS, mask=True)
    assert aogen.canon(got).tobytes() == aogen.canon(want).tobytes(), first_mismatch(got, want)
    assert (got_lit == lit).all() and lit.any()
    want = G.contains0(name)
    got = rtg.contains_host(sph, G.points(name), walk=1, threads=THREADS)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{len(bad)} points differ, first {bad[0]}: {G.points(name)[bad[0]]}"
    assert (want >= 0).any() and (want < 0).any()


@pytest.mark.parametrize("name", G.NAMES)
def test_gather_walk1_equals_walk0(rtg, name):
    """The gather's kernel path over the packed tables against the plain
    loops, plain and with jitter and the skip flag, the skip counts included."""
    import gathergen
    sph, lg = G.scene(name)
    G.check_gather_fold_non_vacuous(name)
    for sem in ((0, 1) if name in ("mirror_x", "deep19") else (0,)):
        for flags in G.GATHER_FLAGS:
            want, want_skp = G.gather0(name, flags, sem)
            got, skp = rtg.gather_host(sph, lg, G.hits(name), gathergen.dirs(G.GATHER_DIRS),
                                       G.gather_weights(), G.gather_params(rtg, flags),
                                       stack_size=G.trace_stack(name), semantics=sem, walk=1,
                                       threads=THREADS, skipped=True)
            assert gathergen.same_words(got, want) is None, (sem, flags,
                                                             gathergen.same_words(got, want))
            assert skp.tobytes() == want_skp.tobytes(), (sem, flags)
            assert bool(want_skp.any()) <= bool(flags & G.GATHER_SKIP)


def test_gather_skips_on_most_scenes(rtg):
    """With the skip flag a probe is left out on at least ten of the thirteen
    scenes (measured: all but wide_deep), and the shares of points with a
    finite non-zero sum are at least 5 % plain and 15 % with the flag
    (measured minima: 11 % on lattice_overlap, 20 % on deep19)."""
    shares = {name: G.gather_shares(name) for name in G.NAMES}
    assert len(G.NAMES) == 13
    assert sum(s[2] > 0 for s in shares.values()) >= 10, shares
    assert min(s[0] for s in shares.values()) >= 0.05, shares
    assert min(s[1] for s in shares.values()) >= 0.15, shares
    folds = [int(G.fold0(name, G.FOLD_SKIP)[1].sum()) for name in G.NAMES]
    assert sum(c > 0 for c in folds) >= 10, folds


# ---- 4. the posed camera ----

@pytest.mark.parametrize("name", G.NAMES)
def test_posed_camera_walk1_equals_walk0(rtg, name):
    sph, lg = G.scene(name)
    s = G.trace_stack(name)
    for eye, target in G.poses(name):
        cam = rtg.camera_look_at(eye, target)
        want = rtg.render_camera_host(sph, lg, cam, G.VW, G.VH, alias_factor=2.0, stack_size=s,
                                      walk=0, threads=THREADS)
        got = rtg.render_camera_host(sph, lg, cam, G.VW, G.VH, alias_factor=2.0, stack_size=s,
                                     walk=1, threads=THREADS)
        assert got.tobytes() == want.tobytes(), (eye, first_mismatch(got, want))
        assert G.lit_fraction(want) >= 0.05, (eye, G.lit_fraction(want))
    # the same two poses, the identity and a NaN pose as one table of views
    want = G.views0(name)
    got = rtg.render_views_host(sph, lg, G.view_table(rtg, name), G.VW, G.VH, alias_factor=2.0,
                                stack_size=s, walk=1, threads=THREADS)
    assert bits_equal(got, want), first_mismatch(got, want)
    assert want[3].tobytes() != want[0].tobytes()  # the NaN pose: not the outside pose's frame


@pytest.mark.parametrize("name", G.NAMES)
def test_views_fold_walk1_equals_walk0(rtg, name):
    """render_views_fold_host over the kernel's path (walk 1) against the fold
    of the plain loops' frames, with and without the skip flag, counts included."""
    sph, lg = G.scene(name)
    G.check_gather_fold_non_vacuous(name)
    for sem in ((0, 1) if name in ("mirror_x", "deep19") else (0,)):
        for flags in (0, G.FOLD_SKIP):
            want, want_cnt = G.fold0(name, flags, sem)
            got, cnt = rtg.render_views_fold_host(
                sph, lg, G.view_table(rtg, name), G.VW, G.VH, G.fold_weights(),
                rtg.fold_params(G.FOLD_G, G.FOLD_K, flags), alias_factor=2.0,
                stack_size=G.trace_stack(name), semantics=sem, walk=1, threads=THREADS,
                skipped=True)
            assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (sem, flags)
            assert (cnt == want_cnt).all(), (sem, flags, cnt, want_cnt)
