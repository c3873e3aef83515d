"""GPU tests over the structured scenes of tests/bvhgen.py on an MI355X: trees
at the depth limit, the finite scenes build_bvh refuses, exact ties across
subtrees, lattices and 256 lights, through every device entry point that walks
the BVH, against the references test_bvh_shapes_host.py pins on the CPU (the
oracle's frames, the plain loops' hits, visibilities, colours, counts, sums and
indices, the host forms of the G-buffer and the posed views, the gather's sums
and the views' folded coefficients with their skip counts), bit for bit.

One context per scene, kept for the module.  Every destination is pre-filled
and PAD records longer than its result; the tail must stay.  The batches run
plain, in rtg_ray_order_device's order and in a seeded shuffle: the shuffle
gives a wave 64 unrelated rays (mixed octants, the union of their children on
the one LDS stack, lanes left over after the list-walk budget).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import aogen
import bvhgen as G
import gathergen
from conftest import bits_equal, first_mismatch
from raygen import diff_hits
from test_gpu_ao import _counts
from test_gpu_gather import FILL16, FILL32
from test_gpu_gather import _same as _same_gather
from test_gpu_hostile import _check_frame, _frame, _sharded, _words
from test_gpu_matte import _contains, _dev, _matte
from test_gpu_order import PAD, _run, _same_as_host, _stream
from test_gpu_views import _views
from test_gpu_views_fold import _fold, _fused
from test_gpu_views_fold import _same as _same_fold

pytestmark = pytest.mark.gpu

THREADS = G.THREADS
EXTRA_DEPTHS = ("deep19", "refused", "mirror_x")  # S = 1 and 16, and a 3-shard render
OPENCL = ("mirror_x", "deep19")


@pytest.fixture(scope="module")
def R(rtg):
    if rtg.device_count() < 1:
        pytest.fail("no GPU visible to librtg")
    return rtg


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def contexts(R):
    """One context per scene, made on first use and kept for the module."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = R.Context(0)
            made[name].set_scene(*G.scene(name))
            # which instantiation the kernels below run: the flat queries for
            # the two refused scenes, the BVH for every other
            nodes = made[name].scene_stats()["bvh_nodes"]
            assert (nodes == 0) == (name in G.DEPTH and G.DEPTH[name] is None), (name, nodes)
        return made[name]
    yield get
    for ctx in made.values():
        ctx.close()


# ---- frames and the G-buffer ----

@pytest.mark.parametrize("name", G.NAMES)
def test_frames(R, oracle, torch_cuda, contexts, name):
    torch = torch_cuda
    sph, lg = G.scene(name)
    ctx = contexts(name)
    w, h, runs = G.frame_args(name)
    if name in EXTRA_DEPTHS:
        runs = runs + [(1.0, 16), (2.0, 1)]
    for aa, s in runs:
        want = G.oracle_frame(oracle, name, w, h, s, aa)
        for variant in (0, 9):
            _check_frame(_frame(torch, ctx, w, h, s, aa, variant), want, (variant, aa, s))
    if name in EXTRA_DEPTHS:
        aa, s = runs[0]
        _check_frame(_sharded(torch, ctx, w, h, s, aa), G.oracle_frame(oracle, name, w, h, s, aa),
                     "3 shards")
    for aa in (2.0, 1.0):  # (the id channel shows a tie directly)
        got = _words(torch, lambda p: ctx.gbuffer_device(w, h, p, alias_factor=aa,
                                                         stream=_stream(torch)), w * h * 8)
        want = R.gbuffer_host(sph, w, h, -4.0, aa, threads=THREADS)
        assert got.tobytes() == want.tobytes(), ("G-buffer", aa)
        assert (want["hits"] > 0).any()


# ---- the batch queries: plain, ordered, shuffled ----

@pytest.mark.parametrize("name", G.NAMES)
def test_batches(R, torch_cuda, contexts, name):
    torch = torch_cuda
    sph, lg = G.scene(name)
    rays, segs = (a.copy() for a in G.batches(name))
    G.check_non_vacuous(name)
    hits, vis = G.walk0(name)
    ctx = contexts(name)
    d_rays, d_segs = torch.from_numpy(rays).cuda(), torch.from_numpy(segs).cuda()
    o_rays, _ = _same_as_host(R, torch, ctx, sph, rays)
    o_segs, _ = _same_as_host(R, torch, ctx, sph, segs, kind=R.ORDER_SEGMENTS)
    rng = np.random.default_rng(6400 + G.NAMES.index(name))
    nt = len(G.trace_rays(name))
    orders = {"plain": (None, None, None),
              "ordered": (o_rays, o_segs, R.ray_order_host(sph, rays[:nt], threads=THREADS)),
              "shuffled": tuple(rng.permutation(k).astype(np.uint32)
                                for k in (len(rays), len(segs), nt))}
    for label, (o_r, o_s, o_t) in orders.items():
        o_r, o_s, o_t = (None if o is None else torch.from_numpy(o.view(np.int32).copy()).cuda()
                         for o in (o_r, o_s, o_t))
        got = _run(torch, ctx.intersect_device, d_rays, len(rays), 8, o_r)
        assert got.tobytes() == hits.tobytes(), (label, diff_hits(got.view(R.HIT_DTYPE), hits))
        got = _run(torch, ctx.visible_device, d_segs, len(segs), 0, o_s)
        bad = np.flatnonzero(got != vis)
        assert not len(bad), (label, f"{len(bad)} segments differ, first {bad[0]}: {segs[bad[0]]}")
        for sem in ((0, 1) if name in OPENCL else (0,)):
            ctx.set_semantics(sem)
            try:
                got = _run(torch, functools.partial(ctx.raytrace_device,
                                                    stack_size=G.trace_stack(name)),
                           d_rays, nt, 3, o_t)
            finally:
                ctx.set_semantics(R.Context.SEMANTICS_CPU)
            want = G.colours0(name, sem)
            assert got.tobytes() == want.tobytes(), (
                label, sem, first_mismatch(got.view(np.float32).reshape(-1, 3), want))


# ---- the posed camera and the views ----

@pytest.mark.parametrize("name", G.NAMES)
def test_views(R, torch_cuda, contexts, name):
    torch = torch_cuda
    ctx = contexts(name)
    want = G.views0(name)
    table = G.view_table(R, name)
    s = G.trace_stack(name)
    assert G.lit_fraction(want[0]) >= 0.05 and G.lit_fraction(want[1]) >= 0.05
    assert want[3].tobytes() != want[0].tobytes()  # the NaN pose: not the outside pose's frame
    for v in (0, 1):
        cam = table[v].view(R.CAMERA_DTYPE)
        got = _words(torch, lambda p: ctx.render_camera(cam, G.VW, G.VH, p, alias_factor=2.0,
                                                        stack_size=s, stream=_stream(torch)),
                     G.VW * G.VH * 3).view(np.float32).reshape(G.VH, G.VW, 3)
        assert bits_equal(got, want[v]), ("camera", v, first_mismatch(got, want[v]))
    got = _views(torch, ctx, table, G.VW, G.VH, -4.0, 2.0, s)
    for v in range(4):
        assert bits_equal(got[v], want[v]), ("view", v, first_mismatch(got[v], want[v]))


# ---- ambient occlusion, direct light, containment ----

@pytest.mark.parametrize("name", G.NAMES)
def test_point_queries(R, torch_cuda, contexts, name):
    torch = torch_cuda
    ctx = contexts(name)
    h = G.hits(name)
    n = len(h)
    d_hits, d_dirs = _dev(torch, h), _dev(torch, aogen.dirs(G.AO_DIRS))
    for flags in (0, R.AO_JITTER):
        want = G.ao0(name, flags)
        got = _counts(torch, ctx, d_hits, n, G.ao_params(R, name, flags), d_dirs, G.AO_DIRS)
        assert got.tobytes() == want.tobytes(), (flags, int((got != want).sum()))
    want, lit = G.matte0(name)
    for mask in (True, False):
        got, got_lit = _matte(torch, ctx, d_hits, n, mask=mask)
        assert aogen.canon(got).tobytes() == aogen.canon(want).tobytes(), (
            mask, first_mismatch(got, want))
        if mask:  # (many_lights: the first 64 of its 256 lights)
            bad = np.flatnonzero(got_lit != lit)
            assert not len(bad), f"{len(bad)} masks differ, first {bad[0]}"
            assert lit.any()
    pts = G.points(name)
    got = _contains(torch, ctx, _dev(torch, pts), len(pts))
    want = G.contains0(name)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{len(bad)} points differ, first {bad[0]}: {pts[bad[0]]}"


# ---- the gather and the views folded into coefficients ----

def _with_semantics(R, ctx, name, body):
    """body(sem) under the scene's semantics in turn; the context is left with
    the CPU's."""
    for sem in ((0, 1) if name in OPENCL else (0,)):
        ctx.set_semantics(sem)
        try:
            body(sem)
        finally:
            ctx.set_semantics(R.Context.SEMANTICS_CPU)


def _gathers(torch, ctx, d_hits, n, params, d_dirs, d_w, nd, S):
    """One fused call per params record, each on a stream of its own and all in
    flight at once: [(sums, skipped), ...].  (A launch over many_lights takes
    0.7 s whether it holds 64 points or 600: a wave's 7 traces a lane under 256
    lights, one after the other.  Side by side the launches cost one.)"""
    out = [(torch.full(((n + PAD) * 3,), FILL32, dtype=torch.int32, device="cuda"),
            torch.full((n + PAD,), FILL16, dtype=torch.int16, device="cuda")) for _ in params]
    own = [torch.cuda.Stream() for _ in params]
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    for p, (dst, skp), st in zip(params, out, own):
        ctx.gather_device(d_hits.data_ptr(), n, p, d_dirs.data_ptr(), d_w.data_ptr(), nd,
                          dst.data_ptr(), skipped_ptr=skp.data_ptr(), stack_size=S,
                          stream=st.cuda_stream)
    torch.cuda.synchronize()
    res = []
    for dst, skp in out:
        sums, cnt = dst.cpu().numpy(), skp.cpu().numpy().view(np.uint16)
        assert (sums[n * 3:] == FILL32).all(), "sums past the batch were written"
        assert (cnt[n:] == FILL16).all(), "counts past the batch were written"
        res.append((sums[:n * 3].view(np.float32).reshape(n, 3), cnt[:n]))
    return res


@pytest.mark.parametrize("name", G.NAMES)
def test_gather(R, torch_cuda, contexts, name):
    """gather_kernel<S, kBvh, kCL> on the structured scenes: 64 unrelated
    points a wave, K = 7 traces each, lanes with id < 0 and past n stepping
    round the trace; sums and skip counts word for word."""
    torch = torch_cuda
    G.check_gather_fold_non_vacuous(name)
    ctx = contexts(name)
    h = G.hits(name)
    n = len(h)
    assert n % 64 and (h["id"] < 0).any() and (h["id"] >= 0).any()  # a ragged last wave
    d_hits, d_dirs = _dev(torch, h), _dev(torch, gathergen.dirs(G.GATHER_DIRS))
    d_w = _dev(torch, G.gather_weights())

    def body(sem):
        got = _gathers(torch, ctx, d_hits, n, [G.gather_params(R, f) for f in G.GATHER_FLAGS],
                       d_dirs, d_w, G.GATHER_DIRS, G.trace_stack(name))
        for flags, (sums, skp) in zip(G.GATHER_FLAGS, got):
            want, want_skp = G.gather0(name, flags, sem)
            _same_gather(sums, want, skp, want_skp, (sem, flags))
    _with_semantics(R, ctx, name, body)


@pytest.mark.parametrize("name", G.NAMES)
def test_views_fold(R, torch_cuda, contexts, name):
    """views_fold_kernel on the structured scenes: the fused call equals the
    fold of the plain loops' frames, and the device fold of the frames
    render_views writes (test_views holds those to the same frames)."""
    torch = torch_cuda
    G.check_gather_fold_non_vacuous(name)
    ctx = contexts(name)
    table, w, s = G.view_table(R, name), G.fold_weights(), G.trace_stack(name)

    def body(sem):
        frames = _views(torch, ctx, table, G.VW, G.VH, -4.0, 2.0, s)
        for flags in (0, G.FOLD_SKIP):
            want, want_cnt = G.fold0(name, flags, sem)
            want = (want.view(np.uint32), want_cnt)
            got = _fused(torch, R, ctx, table, G.VW, G.VH, -4.0, 2.0, s, w, G.FOLD_G, G.FOLD_K,
                         flags)
            _same_fold(got, want, ("fused", sem, flags))
            unfused = _fold(torch, R, ctx, frames, w, G.FOLD_G, G.FOLD_K, flags)
            _same_fold(unfused, want, ("render_views + views_fold", sem, flags))
    _with_semantics(R, ctx, name, body)
