"""GPU tests of the device calls on scenes, rays and signals scaled by powers
of two (scalegen.py) on an MI355X.  The hardware square root, reciprocal and
reciprocal square root with their refinements, their range tests and the
wave-uniform fallback branches (csrc/rtg_trace.h), and the frame passes' `/`
and sqrtf as the device compiler expands them, exist only in the device build:
the host forms of test_scale_host.py cannot see them.  Here every device call
writes into a pre-filled destination PAD records longer than needed and is
compared word for word with the host answers that file pins: the plain loops
(walk 0), the oracle's frames, and the host loops of the frame passes (equal
to their numpy restatements there).

The `laned` batches are the only inputs whose waves take the per-wave fallback
branches with a minority of their lanes (test_scale_host.py asserts what each
wave holds).
"""
from __future__ import annotations

import functools

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
from test_camera_host import pose
from test_gpu_accumulate import _accumulate, _dev_prev
from test_gpu_ao import _counts
from test_gpu_camera import _frame, _rays
from test_gpu_filter import _dev, _filter, _first_bad
from test_gpu_matte import _contains, _matte
from test_gpu_order import PAD, _order, _run, _stream
from test_gpu_svgf import _svgf, _variance
from test_gpu_views import _views
from test_gpu_views_fold import _fold
from test_raytrace_host import THREADS

pytestmark = pytest.mark.gpu

F = np.float32
FILL32, FILL16 = 0x5A5A5A5A, 0x5A5A
EVERY_BATCH = BATCHES + [(j, "laned") for j in J_LANED]
EVERY_ID = BATCH_IDS + [f"j{j}-laned" for j in J_LANED]
FLAT = {(65, -60), (200, -60), ("c5", -60), ("c5", -40)}  # more than 64 spheres and no BVH


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


def _words(a):
    return np.ascontiguousarray(a, F).view(np.uint32).reshape(-1)


def _index(torch, order):
    return torch.from_numpy(np.ascontiguousarray(order, np.uint32).view(np.int32)).cuda()


def _gather(torch, ctx, d_hits, n, p, d_dirs, d_w, nd, S_):
    dst = torch.full(((n + PAD) * 3,), FILL32, dtype=torch.int32, device="cuda")
    skp = torch.full((n + PAD,), FILL16, dtype=torch.int16, device="cuda")
    ctx.gather_device(d_hits.data_ptr(), n, p, d_dirs.data_ptr(), d_w.data_ptr(), nd, dst.data_ptr(),
                      skipped_ptr=skp.data_ptr(), stack_size=S_, stream=_stream(torch))
    torch.cuda.synchronize()
    out, cnt = dst.cpu().numpy().view(np.uint32), skp.cpu().numpy().view(np.uint16)
    assert (out[3 * n:] == FILL32).all() and (cnt[n:] == FILL16).all(), "written past the batch"
    return out[:3 * n], cnt[:n]


# ---- 1. the ray calls and the hit-point passes ----

@pytest.mark.parametrize("j,d", EVERY_BATCH, ids=EVERY_ID)
@pytest.mark.parametrize("name", SCENES)
def test_batch_calls_equal_plain_loops(R, torch_cuda, name, j, d):
    """rtg_intersect_device, rtg_visible_device and rtg_raytrace_device,
    un-indexed and through one _indexed launch with the device's own order;
    rtg_ao_device, rtg_matte_device with the mask, rtg_gather_device and
    rtg_contains_device on the batch's walk-0 records."""
    torch = torch_cuda
    sph, lg = X.scene(name, j)
    rays, segs = X._batch(name, j, d), X.segments(name, j, d)
    n = len(rays)
    want_h, want_v, want_c = X.want_hits(name, j, d), X.want_visible(name, j, d), X.want_colours(name, j, d)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        nodes = ctx.scene_stats()["bvh_nodes"]
        # 12, 64: the masked kernel; 65, 200, c5: the BVH with lists, but for the
        # scales at which the scene packer refuses a tree, where they take the
        # flat query above 64 spheres (so every path meets scaled rays)
        assert (nodes > 0) == (len(sph) > 64 and (name, j) not in FLAT), nodes
        d_rays, d_segs = torch.from_numpy(rays).cuda(), torch.from_numpy(segs).cuda()
        ray_order, _ = _order(R, torch, ctx, rays)
        seg_order, _ = _order(R, torch, ctx, segs, kind=R.ORDER_SEGMENTS)
        assert (np.sort(ray_order) == np.arange(n)).all() and (np.sort(seg_order) == np.arange(n)).all()
        trace = functools.partial(ctx.raytrace_device, stack_size=X.STACK)
        for o_r, o_s in ((None, None), (_index(torch, ray_order), _index(torch, seg_order))):
            got = _run(torch, ctx.intersect_device, d_rays, n, 8, o_r).view(R.HIT_DTYPE)
            assert diff_hits(got, want_h) is None, (o_r is not None, diff_hits(got, want_h))
            got = _run(torch, ctx.visible_device, d_segs, n, 0, o_s)
            assert got.tobytes() == want_v.tobytes(), (o_s is not None, np.flatnonzero(got != want_v)[:4])
            got = _run(torch, trace, d_rays, n, 3, o_r).view(np.uint32).reshape(n, 3)
            bad = np.flatnonzero((got != _words(want_c).reshape(n, 3)).any(1))
            assert not len(bad), (o_r is not None, len(bad), rays[bad[0]], got[bad[0]].view(F),
                                  want_c[bad[0]])
        h = X.hits(name, j, d)
        m = len(h)
        d_hits = _dev(torch, h)
        d_dirs = _dev(torch, aogen.dirs(X.AO_DIRS))
        got = _counts(torch, ctx, d_hits, m, X.ao_params(R, name, j), d_dirs, X.AO_DIRS)
        want = X.want_ao(name, j, d)
        assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:4]
        got, lit = _matte(torch, ctx, d_hits, m)
        want, want_lit = X.want_matte(name, j, d)
        assert (_words(got) == _words(want)).all() and (lit == want_lit).all()
        got, skp = _gather(torch, ctx, d_hits, m, X.gather_params(R, name, j), d_dirs,
                           _dev(torch, gathergen.weights(X.GATHER_DIRS)), X.GATHER_DIRS, X.STACK)
        want, want_skp = X.want_gather(name, j, d)
        assert (got == _words(want)).all() and (skp == want_skp).all()
        pts = X.points(name, j, d)
        got = _contains(torch, ctx, _dev(torch, pts), len(pts))
        assert got.tobytes() == X.want_contains(name, j, d).tobytes()
    finally:
        ctx.close()


# ---- 2. frames ----

def _device_frame(torch, call, W, H, words, **kw):
    dst = torch.full(((W * H + PAD) * words,), FILL32, dtype=torch.int32, device="cuda")
    call(W, H, dst.data_ptr(), stream=_stream(torch), **kw)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[W * H * words:] == FILL32).all(), "pixels past the frame were written"
    return out[:W * H * words]


@pytest.mark.parametrize("name,j", FRAMES)
def test_frames_equal_the_oracle(R, torch_cuda, name, j):
    """rtg_render_device and rtg_render_camera_device (identity pose) against
    the oracle in both semantics, rtg_gbuffer_device against rtg_gbuffer_host,
    and rtg_render_views_device with the six cube poses at the scaled centre
    of the scene, 8 x 8, against rtg_render_views_host(walk 0)."""
    torch = torch_cuda
    sph, lg = X.scene(name, j)
    W, H, aa, S_ = X.FRAME_W, X.FRAME_H, X.FRAME_AA, X.FRAME_S
    lo, hi = (sph["pos"].astype(np.float64).min(0), sph["pos"].astype(np.float64).max(0))
    cams = R.camera_cube(((lo + hi) * 0.5).astype(F))
    cams12 = np.ascontiguousarray(cams).view(F).reshape(6, 12)
    want_views = R.render_views_host(sph, lg, cams, 8, 8, -1.0, 1.0, S_, walk=0, threads=THREADS)
    assert (np.nan_to_num(want_views) != 0).any()
    want_g = R.gbuffer_host(sph, W, H, alias_factor=aa, threads=THREADS)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        for sem in (0, 1):
            ctx.set_semantics(sem)
            want = X.want_frame(name, j, sem)
            got = _device_frame(torch, ctx.render_device, W, H, 3, alias_factor=aa,
                                stack_size=S_).view(F).reshape(H, W, 3)
            assert bits_equal(got, want), (sem, "render", first_mismatch(got, want))
            got = _frame(torch, ctx, R.camera_identity(), W, H, -4.0, aa, S_)
            assert bits_equal(got, want), (sem, "camera", first_mismatch(got, want))
        ctx.set_semantics(0)
        got = _device_frame(torch, ctx.gbuffer_device, W, H, R.GBUF_DTYPE.itemsize // 4,
                            alias_factor=aa).view(R.GBUF_DTYPE).reshape(H, W)
        assert got.tobytes() == want_g.tobytes(), np.argwhere(
            got.view(np.uint32).reshape(H, W, -1) != want_g.view(np.uint32).reshape(H, W, -1))[:2]
        got = _views(torch, ctx, cams12, 8, 8, -1.0, 1.0, S_)
        for v in range(6):
            assert got[v].tobytes() == want_views[v].tobytes(), (v, first_mismatch(got[v], want_views[v]))
    finally:
        ctx.close()


# ---- 3. the generator and the projection ----

@pytest.mark.parametrize("j", J_POSE)
def test_camera_rays_and_project_equal_host(R, torch_cuda, j):
    torch = torch_cuda
    ctx = R.Context(0)  # no scene: neither call needs one
    try:
        for scene in (12, "c5"):
            for name in ("orbit", "raw"):
                cam, zoom = pose(name, scene)
                cam = X.scaled_pose(cam, j).reshape(-1)
                got = _rays(R, torch, ctx, cam, 9, 7, zoom, 2.0)
                want = R.camera_rays_host(cam, 9, 7, zoom, 2.0)
                assert bits_equal(got, want), (scene, name, first_mismatch(got, want))
        W, H = G.FULL
        for name in X.PASS_SCENES:
            pts = X.project_points(name, j)
            d_pts = _dev(torch, pts)
            for pk in ("same", "pan", "roll"):
                cam = X.scaled_pose(A.pose(name, pk), j)
                dst = torch.full(((len(pts) + PAD) * 3,), FILL32, dtype=torch.int32, device="cuda")
                ctx.camera_project_device(cam, W, H, d_pts.data_ptr(), len(pts), dst.data_ptr(),
                                          zoom=A.ZOOM, stream=_stream(torch))
                torch.cuda.synchronize()
                out = dst.cpu().numpy().view(np.uint32)
                assert (out[len(pts) * 3:] == FILL32).all(), "rows past the batch were written"
                want = _words(R.camera_project_host(cam, W, H, pts, zoom=A.ZOOM, threads=THREADS))
                assert (out[:len(pts) * 3] == want).all(), (name, pk, _first_bad(out[:len(pts) * 3], want))
    finally:
        ctx.close()


# ---- 4. the frame passes ----

@pytest.mark.parametrize("form", ["auto", "tiled", "direct"])
@pytest.mark.parametrize("k", K_SIGNAL)
@pytest.mark.parametrize("name", X.PASS_SCENES)
def test_frame_passes_equal_host(R, torch_cuda, name, k, form, monkeypatch):
    """rtg_filter_device, rtg_accumulate_device with M2, rtg_variance_device on
    the `seeded` and `zero` len fields and rtg_svgf_device with LUMA on signals
    x 2^k, at 33 x 17 and 67 x 35, with the pass kernels' form left to the
    library and forced either way (RTG_FILTER_FORM, RTG_SVGF_FORM)."""
    torch = torch_cuda
    if form != "auto":
        monkeypatch.setenv("RTG_FILTER_FORM", form)
        monkeypatch.setenv("RTG_SVGF_FORM", form)
    ctx = R.Context(0)  # no scene: the passes need none
    try:
        for W, H in X.PASS_FRAMES:
            d_hits = _dev(torch, G.guides(name, W, H))
            d_var = _dev(torch, X.var_field(name, W, H, k))
            d_len = {w: _dev(torch, S.len_field(name, W, H, w)) for w in X.VAR_FIELDS}
            for kind in X.PASS_SIGNALS:
                d_src = _dev(torch, X.signal(name, W, H, kind, k))
                for st in X.FILTER_SETS:
                    got = _filter(torch, R, ctx, d_hits, W, H, G.params(R, name, kind, st), d_src)
                    want = X.want_filter(name, W, H, kind, st, k)
                    assert got.tobytes() == want.tobytes(), ("filter", W, H, kind, st, _first_bad(got, want))
                for st in X.SVGF_SETS:
                    got = _svgf(torch, R, ctx, d_hits, W, H, S.svgf_params(R, name, kind, st), d_src, d_var)
                    want = X.want_svgf(name, W, H, kind, st, k)
                    for what, g, w in zip(("value", "variance"), got, want):
                        assert g.tobytes() == w.tobytes(), ("svgf", what, W, H, kind, st, _first_bad(g, w))
                if form != "auto":
                    continue  # the two calls below have one form
                acc, m2 = X.state(name, W, H, kind, k)
                d_acc, d_m2 = _dev(torch, acc), _dev(torch, m2)
                for which in X.VAR_FIELDS:
                    for st in X.VAR_SETS:
                        got = _variance(torch, R, ctx, d_hits, W, H, S.variance_params(R, name, kind, st),
                                        d_acc, d_m2, d_len[which])
                        want = X.want_variance(name, W, H, kind, which, st, k)
                        assert got.tobytes() == want.tobytes(), ("variance", W, H, kind, which, st,
                                                                 _first_bad(got, want))
                for pk, st in X.ACCUM_CASES:
                    pv, keep = _dev_prev(torch, X.prev(name, W, H, pk, kind, st, k))
                    got = _accumulate(torch, R, ctx, d_hits, W, H, A.params(R, name, kind, st), d_src,
                                      pv, True)
                    want = X.want_accumulate(name, W, H, kind, pk, st, k)
                    for what, g, w in zip(("acc", "len", "m2"), got, want):
                        assert (g == w).all(), ("accumulate", what, W, H, kind, pk, st,
                                                np.flatnonzero(g != w)[:4])
                    del keep
    finally:
        ctx.close()


@pytest.mark.parametrize("k", K_SIGNAL)
def test_views_fold_equals_host(R, torch_cuda, k):
    fr, w = X.fold_inputs(k)
    G_, _, _, K = X.FOLD_SHAPE
    ctx = R.Context(0)
    try:
        for flags in (0, 1):
            got, cnt = _fold(torch_cuda, R, ctx, fr, w, G_, K, flags)
            want, want_cnt = X.want_fold(k, flags)
            assert got.reshape(-1).tobytes() == want.tobytes(), flags
            assert (cnt == want_cnt).all()
    finally:
        ctx.close()
