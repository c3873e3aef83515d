"""Legal device calls whose buffers pass 4 GiB, and the kernels' division-free
index helpers, on an MI355X.

rtg.h promises n up to 2^32 - 1, W * H up to 2^32 - 1 and W * rows < 2^53;
the rest of the suite runs refusals past those limits and frames of at most
400 MB, so every size_t cast and every k * 24 of a kernel has otherwise only
met values that fit in 31 bits.  Here:

  0. divmod_u64, udiv_small and shard_global_row_fast (rtg_trace_kernels.h)
     against the device's 64-bit / and % (tests/fpcheck/fpcheck_index_gpu.hip),
     with counts that show both of divmod_u64's correction branches taken;
  1. the smallest shapes that cross byte offset 2^32 and word index 2^31
     (largegen.SHAPES; test_large_host.py checks what each crosses), each
     checked twice:
       all elements, on the device: the call over the whole batch gives the
         words of the same call over sub-batches, each below 2^32 bytes,
         reached by advancing the base pointers, one split away from a
         multiple of 64 elements (a frame: row ranges through
         render_rows_device, and row-cyclic shards);
       windows, against the plain reference: the elements at the buffer's
         start, around byte 2^32, around word 2^31 and at its end
         (largegen.windows) are copied to the host with their inputs and
         compared word for word, NaNs by position, with the walk-0 host loops,
         the oracle or the numpy restatements of the sibling tests.

Every destination is pre-filled with 0x5A bytes and PAD elements longer than
needed: the tail must survive.  Inputs are made on the device; nothing large
crosses to the host.  A test states its device memory up front (32 GiB at the
most) and skips, visibly, only where the device has less free.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import largegen
from conftest import load_scene, random_scene
from largegen import (BYTE_LIMIT, GIB, N_ORDER, N_POINTS, N_PROBE_POINTS, N_RAYS, PAD, PROBE_K,
                      RAYS_H, RAYS_W, RENDER_W, VIEW_W, VIEWS, Dest, canon_words, cuts,
                      device_memory, first_difference, threshold_rows, to_host, windows_of)
from test_camera_host import cam12
from test_gbuffer_host import restate as restate_gbuffer

pytestmark = pytest.mark.gpu

THREADS = 8
# At the reference's zoom of -4 the scenes cover the middle of a frame only and
# the rows and windows at byte 2^32, which lie at a frame's edge in most shapes,
# hold background alone; at -16 every window holds hits and misses.
ZOOM = -16.0
SLACK = 4 * GIB  # the comparisons' temporaries


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
def scenes():
    """(spheres, lights) of the suite's scenes: golden c3 (16 spheres, the
    masked render path), raygen's scene 200 (a BVH) and golden c5."""
    return {"c3": load_scene("c3", 16, 3), 200: random_scene(np.random.default_rng(1200), 200, 2),
            "c5": load_scene("c5", 1024, 4)}


@pytest.fixture(scope="module")
def pose(R):
    """A look-at pose in front of the scenes, a little off every axis."""
    return cam12(R.camera_look_at([0.5, 0.25, 1.0], [0.0, 0.0, -20.0]))


@pytest.fixture(autouse=True)
def stop_after_a_device_fault(torch_cuda):
    """A fault is sticky in the HIP runtime: where the device reports one after
    a test, the session ends there and nothing more is launched on it."""
    yield
    try:
        torch_cuda.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        pytest.exit(f"the device reports a fault, nothing more is run: {e}", returncode=3)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _context(R, sph, lg):
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    return ctx


# ===================================================================== 0. helpers
@pytest.fixture(scope="module")
def ixlib(R, torch_cuda):
    """After torch and librtg.so, so that the library binds to the HIP runtime
    the process already holds."""
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fpcheck",
                      "libfpcheck_index_gpu.so")
    return ctypes.CDLL(so)


DIVMOD_FLOOR = 100_000


def test_divmod_u64_draws(ixlib):
    """2^28 seeded (q, d, r), a = q d + r < 2^53: no mismatch with / and %, and
    each correction branch taken at least 100 000 times.  The floor is from the
    same draws evaluated on a CPU (IEEE f64, no contraction): 6 220 931 upward
    corrections, all at r = 0, and 2 406 165 downward ones, all at r = d - 1."""
    out = (ctypes.c_ulonglong * 8)()
    n = 1 << 28
    assert ixlib.fpcheck_divmod_run(ctypes.c_ulonglong(n), out) == 0
    total, bad, up, down, r_zero, r_max, small_d, _ = list(out)
    print(f"divmod_u64: {total} draws ({small_d} with d <= 2^17, {r_zero} with r = 0, {r_max} "
          f"with r = d - 1): {bad} mismatches, {up} upward corrections, {down} downward")
    assert total == n and small_d == n // 2
    assert r_zero > n // 4 and r_max > n // 4
    assert bad == 0
    assert up >= DIVMOD_FLOOR and down >= DIVMOD_FLOOR


def _divmod_edges():
    top, qtop = (1 << 53) - 1, (1 << 32) - 1
    a, d = [], []
    for dd in (1, 2, 3, 5, 64, 4096, 16387, 32771, 1 << 16, (1 << 17) - 1, 1 << 17,
               (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1,
               (1 << 32) - 2, (1 << 32) - 1):
        qmax = min(qtop, (top - (dd - 1)) // dd)  # the largest q with q d + d - 1 < 2^53
        for aa in (0, dd - 1, dd, dd + 1, qmax * dd, qmax * dd + dd - 1, qmax * dd - 1,
                   (qmax // 2) * dd, (qmax // 2) * dd + dd - 1, top, qtop * dd, qtop * dd + dd - 1):
            if 0 <= aa <= top and aa // dd <= qtop:
                a.append(aa)
                d.append(dd)
    return np.array(a, np.uint64), np.array(d, np.uint32)


def test_divmod_u64_edges(ixlib):
    """d = 1 and 2^32 - 1, a = 0 and 2^53 - 1 (where the quotient fits),
    q = 2^32 - 1, and the like around them."""
    a, d = _divmod_edges()
    q = a // d.astype(np.uint64)
    assert (d == 1).any() and (d == 0xFFFFFFFF).any() and (a == 0).any()
    assert (a == (1 << 53) - 1).sum() >= 5 and (q == 0xFFFFFFFF).sum() >= 10
    assert ((q == 0xFFFFFFFF) & (d == 1)).any() and ((a == (1 << 53) - 1) & (q == 0xFFFFFFFF)).any()
    inv = 1.0 / d.astype(np.float64)
    out = (ctypes.c_ulonglong * 8)()
    P = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    assert ixlib.fpcheck_divmod_edges_run(P(a), P(d), P(inv), len(a), out) == 0
    total, bad, up, down, _, _, _, inv_bad = list(out)
    print(f"divmod_u64 edges: {total} cases, {bad} mismatches, {up} upward and {down} downward "
          f"corrections, {inv_bad} reciprocals differ from the host's")
    assert total == len(a) and bad == 0 and inv_bad == 0


def test_udiv_small_exhaustive(ixlib):
    out = (ctypes.c_ulonglong * 2)()
    assert ixlib.fpcheck_udiv_small_run(out) == 0
    total, bad = list(out)
    print(f"udiv_small: {total} pairs, {bad} mismatches")
    assert total == 65 * 64 and bad == 0


def test_shard_global_row_fast(ixlib):
    out = (ctypes.c_ulonglong * 6)()
    n = 1 << 24
    assert ixlib.fpcheck_shard_row_run(ctypes.c_ulonglong(n), out) == 0
    total, bad, b_one, g_one, top, high = list(out)
    print(f"shard_global_row_fast: {total} tuples (B = 1: {b_one}, G = 1: {g_one}, the largest "
          f"local row: {top}, global row >= 2^31: {high}), {bad} mismatches")
    assert total == n and bad == 0
    # about a quarter of the draws each by construction
    assert min(b_one, g_one, top) >= n // 5 and high > n // 8


# ===================================================================== 1. harness
def _sub_batches(torch, n, widest, specs, full, launch):
    """The call over sub-batches [lo, hi) of the batch, each below 2^32 bytes in
    its widest buffer, into guarded destinations of their own: the words of
    the whole call's destinations `full` there, nothing after them."""
    b = cuts(n, widest)
    most = max(hi - lo for lo, hi in zip(b, b[1:]))
    assert most * widest < BYTE_LIMIT and any(x % 64 for x in b[1:-1])
    sub = [Dest(torch, most, *s) for s in specs]
    for lo, hi in zip(b, b[1:]):
        for d in sub:
            d.refill()
        launch(lo, hi - lo, [d.ptr() for d in sub])
        torch.cuda.synchronize()
        for k, (f, s) in enumerate(zip(full, sub)):
            assert s.tail_kept(hi - lo), f"output {k}: written past sub-batch [{lo}, {hi})"
            diff = first_difference(torch, f.values(lo, hi), s.values(0, hi - lo), f.canon)
            assert diff is None, (f"output {k}, sub-batch [{lo}, {hi}): value {diff[0]} of it is "
                                  f"{diff[1]:#x} in the whole call, {diff[2]:#x} alone")
    return b


def _batch(torch, n, widest, specs, launch):
    """launch(first, count, destination pointers) over the whole batch into
    guarded destinations (specs: (items, dtype, canon) each), then over
    sub-batches.  The whole call's destinations."""
    full = [Dest(torch, n, *s) for s in specs]
    launch(0, n, [d.ptr() for d in full])
    torch.cuda.synchronize()
    for k, d in enumerate(full):
        assert d.tail_kept(), f"output {k}: written past the batch"
    _sub_batches(torch, n, widest, specs, full, launch)
    return full


def _same_words(got, want, canon, what):
    g = np.ascontiguousarray(got).reshape(len(got), -1)
    w = np.ascontiguousarray(want).reshape(len(want), -1)
    assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (what, g.shape, w.shape)
    if canon:
        g, w = canon_words(g), canon_words(w)
    else:
        g, w = g.view(np.uint8), w.view(np.uint8)
    bad = np.flatnonzero((g != w).any(1))
    assert not len(bad), (f"{what}: {len(bad)} of {len(g)} window elements differ from the "
                          f"reference, first at window element {bad[0]}: {got[bad[0]]} vs "
                          f"{want[bad[0]]}")


def _windows(n, strides, ins, outs, reference, what):
    """The windows of every buffer of the call: reference(first, inputs on the
    host) of each window's inputs against the device's outputs there."""
    spans = windows_of(n, strides)
    seen = []
    for lo, hi in spans:
        host_in = [to_host(d.t, [(lo, hi)], d.items) for d in ins]
        want = reference(lo, *host_in)
        want = want if isinstance(want, (list, tuple)) else [want]
        assert len(want) == len(outs)
        for k, (d, w) in enumerate(zip(outs, want)):
            _same_words(d.host(lo, hi), np.asarray(w).reshape(hi - lo, -1), d.canon,
                        f"{what}, output {k}, elements [{lo}, {hi})")
        seen.append(want)
    return spans, seen


def _camera_rays(R, torch, ctx, pose):
    """The pose's aa 1 rays of the RAYS_W x RAYS_H frame on the device."""
    rays = Dest(torch, N_RAYS, 6, None, True)
    ctx.camera_rays(pose, RAYS_W, RAYS_H, rays.ptr(), ZOOM, 1.0, stream=_stream(torch))
    torch.cuda.synchronize()
    assert rays.tail_kept()
    return rays


def _f32(a):
    return np.ascontiguousarray(a).view(np.float32)


# ===================================================================== 2. ray batches
def test_camera_rays(R, torch_cuda, pose):
    """357 924 864 rays, 8.6 GB: past byte 2^32 and word 2^31.  A frame's
    generator has no sub-batch form, so all rays are compared on the device
    with the generator's formula evaluated by torch in float32, to 2^-22 per
    component: a direction is a unit vector, its components differ from the
    restatement's by at most the few roundings of 1 / sqrt and the product
    where torch's differ from the library's, while the next pixel's direction
    is about 2^-12 away.  The windows are the numpy restatement's, word for
    word."""
    torch = torch_cuda
    with device_memory(torch, N_RAYS * 24 + SLACK, "camera_rays"):
        _camera_rays_body(R, torch, pose)


def _camera_rays_body(R, torch, pose):
    ctx = R.Context(0)
    try:
        rays = _camera_rays(R, torch, ctx, pose)
    finally:
        ctx.close()
    W, H = RAYS_W, RAYS_H
    r = rays.t[:N_RAYS * 6].view(torch.float32).view(H, W, 6)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")  # noqa: E731
    xs, ys, asp = f(16.0) / f(W), f(12.0) / f(H), f(16.0) / f(12.0)
    eye, right, up, back = (torch.from_numpy(pose[k]).cuda() for k in range(4))
    rx = ((torch.arange(W, device="cuda").float() - f(W) * 0.5) * xs) * asp
    worst, exact, band = 0.0, 0, 512
    for y0 in range(0, H, band):
        y = torch.arange(y0, min(y0 + band, H), device="cuda").float()
        ry = (f(H) * 0.5 - y) * ys
        v = [(rx[None, :] * right[q] + ry[:, None] * up[q]) + f(ZOOM) * back[q] for q in range(3)]
        l = 1.0 / torch.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        got = r[y0:y0 + band]
        for q in range(3):
            want = l * v[q]
            worst = max(worst, float((got[..., 3 + q] - want).abs().max()))
            exact += int((got[..., 3 + q] == want).sum())
            assert bool((got[..., q] == eye[q]).all()), f"origins of rows {y0}.."
    print(f"camera_rays: all {N_RAYS} directions within {worst:.3g} of torch's float32 "
          f"restatement, {exact} of {3 * N_RAYS} components equal")
    assert worst <= 2.0 ** -22

    def reference(lo, _rays):
        return largegen.rays_at(pose, W, H, ZOOM, np.arange(lo, lo + len(_rays)))

    _windows(N_RAYS, [24], [rays], [rays], reference, "camera_rays")


@pytest.mark.parametrize("name", ["c3", 200])
def test_intersect(R, torch_cuda, scenes, pose, name):
    """Hits of the 357 924 864 rays: 11.5 GB of records."""
    torch = torch_cuda
    need = N_RAYS * (24 + 32) + (N_RAYS // 3 + 200) * 32 + SLACK
    with device_memory(torch, need, f"intersect[{name}]"):
        _intersect_body(R, torch, scenes[name], pose)


def _intersect_body(R, torch, scene, pose):
    sph, lg = scene
    ctx = _context(R, sph, lg)
    try:
        rays = _camera_rays(R, torch, ctx, pose)
        hits, = _batch(torch, N_RAYS, 32, [(8, None, False)],
                       lambda first, count, dst: ctx.intersect_device(
                           rays.ptr(first), count, dst[0], stream=_stream(torch)))
    finally:
        ctx.close()
    _, seen = _windows(N_RAYS, [24, 32], [rays], [hits],
                       lambda lo, r: R.intersect_host(sph, _f32(r), walk=0, threads=THREADS)
                       .view(np.uint32).reshape(-1, 8), "intersect")
    ids = np.concatenate([s[0][:, 0].view(np.int32) for s in seen])
    assert (ids < 0).any() and len(np.unique(ids[ids >= 0])) >= 2, "the windows hold no hits"


def _segments_in_place(torch, rays):
    """The rays as segments from the eye to the point 40 along the ray."""
    r = rays.t[:N_RAYS * 6].view(torch.float32).view(N_RAYS, 6)
    for lo in range(0, N_RAYS, 1 << 24):
        r[lo:lo + (1 << 24), 3:] = r[lo:lo + (1 << 24), :3] + r[lo:lo + (1 << 24), 3:] * 40.0


@pytest.mark.parametrize("name", ["c3", 200])
def test_visible(R, torch_cuda, scenes, pose, name):
    """Line of sight along the first 40 units of the same rays (the ray
    buffer rewritten as segments on the device)."""
    torch = torch_cuda
    with device_memory(torch, N_RAYS * (24 + 1) + N_RAYS + SLACK, f"visible[{name}]"):
        _visible_body(R, torch, scenes[name], pose)


def _visible_body(R, torch, scene, pose):
    sph, lg = scene
    ctx = _context(R, sph, lg)
    try:
        segs = _camera_rays(R, torch, ctx, pose)
        _segments_in_place(torch, segs)
        vis, = _batch(torch, N_RAYS, 24, [(1, torch.uint8, False)],
                      lambda first, count, dst: ctx.visible_device(
                          segs.ptr(first), count, dst[0], stream=_stream(torch)))
    finally:
        ctx.close()
    _, seen = _windows(N_RAYS, [24, 1], [segs], [vis],
                       lambda lo, s: R.visible_host(sph, _f32(s), walk=0, threads=THREADS),
                       "visible")
    v = np.concatenate([s[0].reshape(-1) for s in seen])
    assert (v == 0).any() and (v == 1).any(), "the windows hold one answer only"


@pytest.mark.parametrize("name", ["c3", 200])
def test_raytrace(R, torch_cuda, scenes, pose, name):
    """rayTrace's colours at stack size 3: 4.3 GB of them."""
    torch = torch_cuda
    need = N_RAYS * (24 + 12) + (N_RAYS // 2 + 200) * 12 + SLACK
    with device_memory(torch, need, f"raytrace[{name}]"):
        _raytrace_body(R, torch, scenes[name], pose)


def _raytrace_body(R, torch, scene, pose):
    sph, lg = scene
    ctx = _context(R, sph, lg)
    try:
        rays = _camera_rays(R, torch, ctx, pose)
        col, = _batch(torch, N_RAYS, 24, [(3, None, True)],
                      lambda first, count, dst: ctx.raytrace_device(
                          rays.ptr(first), count, dst[0], stack_size=3, stream=_stream(torch)))
    finally:
        ctx.close()
    _, seen = _windows(N_RAYS, [24, 12], [rays], [col],
                       lambda lo, r: R.raytrace_host(sph, lg, _f32(r), stack_size=3, walk=0,
                                                     threads=THREADS), "raytrace")
    c = np.concatenate([s[0] for s in seen])
    assert (np.nan_to_num(c) != 0).any() and (c == 0).all(1).any()


@pytest.mark.parametrize("call", ["intersect", "visible", "raytrace"])
def test_indexed_forms(R, torch_cuda, scenes, pose, call):
    """The _indexed forms with the reversed order over the whole batch: the
    plain call's output, word for word (the results stay in batch order)."""
    torch = torch_cuda
    out = {"intersect": 32, "visible": 1, "raytrace": 12}[call]
    # the rays and the order are freed before the outputs are compared
    with device_memory(torch, N_RAYS * (24 + 4 + 2 * out) + GIB // 2, f"indexed[{call}]"):
        _indexed_body(R, torch, scenes["c3"], pose, call)


def _indexed_body(R, torch, scene, pose, call):
    sph, lg = scene
    spec = {"intersect": (8, None, False), "visible": (1, torch.uint8, False),
            "raytrace": (3, None, True)}[call]
    ctx = _context(R, sph, lg)
    try:
        rays = _camera_rays(R, torch, ctx, pose)
        if call == "visible":
            _segments_in_place(torch, rays)
        order = torch.arange(N_RAYS - 1, -1, -1, dtype=torch.int32, device="cuda")  # < 2^31
        fn = {"intersect": ctx.intersect_device, "visible": ctx.visible_device,
              "raytrace": lambda *a, **k: ctx.raytrace_device(*a, stack_size=3, **k)}[call]
        plain, indexed = Dest(torch, N_RAYS, *spec), Dest(torch, N_RAYS, *spec)
        fn(rays.ptr(), N_RAYS, plain.ptr(), stream=_stream(torch))
        fn(rays.ptr(), N_RAYS, indexed.ptr(), stream=_stream(torch), order=order.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.close()
    del rays, order
    torch.cuda.empty_cache()
    assert plain.tail_kept() and indexed.tail_kept()
    diff = first_difference(torch, plain.values(0, N_RAYS), indexed.values(0, N_RAYS), spec[2])
    assert diff is None, f"{call}: value {diff[0]} is {diff[1]:#x} plain, {diff[2]:#x} indexed"
    # element i and element n - 1 - i differ somewhere, or the order would not matter
    m, items = 1 << 22, spec[0]
    head = plain.values(0, m).view(m, items)
    tail = plain.values(N_RAYS - m, N_RAYS).view(m, items).flip(0)
    assert bool((head != tail).any())


def test_camera_project(R, torch_cuda, scenes, pose):
    """The 357 924 864 hit points (12 B each, 4.3 GB) back into the frame."""
    torch = torch_cuda
    need = N_RAYS * (24 + 32 + 12) + SLACK
    with device_memory(torch, need, "camera_project"):
        _project_body(R, torch, scenes["c3"], pose)


def _hit_points(R, torch, scene, pose, n):
    """The first n hit records of the camera rays, and their points apart."""
    sph, lg = scene
    ctx = _context(R, sph, lg)
    try:
        rays = _camera_rays(R, torch, ctx, pose)
        hits = Dest(torch, n, 8)
        ctx.intersect_device(rays.ptr(), n, hits.ptr(), stream=_stream(torch))
        torch.cuda.synchronize()
        assert hits.tail_kept()
    finally:
        ctx.close()
    del rays
    pts = Dest(torch, n, 3, None, True)
    pts.t[:n * 3].view(n, 3).copy_(hits.t[:n * 8].view(n, 8)[:, 2:5])
    return hits, pts


def _project_body(R, torch, scene, pose):
    hits, pts = _hit_points(R, torch, scene, pose, N_RAYS)
    del hits
    torch.cuda.empty_cache()
    ctx = R.Context(0)
    try:
        out, = _batch(torch, N_RAYS, 12, [(3, None, True)],
                      lambda first, count, dst: ctx.camera_project_device(
                          pose.reshape(12).view(R.CAMERA_DTYPE), RAYS_W, RAYS_H, pts.ptr(first),
                          count, dst[0], zoom=ZOOM, stream=_stream(torch)))
    finally:
        ctx.close()
    _, seen = _windows(N_RAYS, [12], [pts], [out],
                       lambda lo, p: R.camera_project_host(
                           pose.reshape(12).view(R.CAMERA_DTYPE), RAYS_W, RAYS_H, _f32(p),
                           zoom=ZOOM, threads=THREADS), "camera_project")
    k = np.concatenate([s[0][:, 2] for s in seen])
    assert (k > 0).any()


# ===================================================================== 3. hit-point passes
def _points_need(out_bytes):
    # the rays and all hits while the records are made, then records, points, outputs
    return max(N_RAYS * 24 + N_POINTS * 32, N_POINTS * (32 + 12 + 2 * out_bytes)) + SLACK


def test_ao(R, torch_cuda, scenes, pose):
    """ao_device, K = 2 of a jittered table of 16, over 134 217 792 records
    (4.29 GB): a point's window depends on seed + its index, so a sub-batch
    starts with the seed advanced by its first index."""
    torch = torch_cuda
    with device_memory(torch, _points_need(2), "ao"):
        _ao_body(R, torch, scenes["c3"], pose)


def _ao_body(R, torch, scene, pose):
    sph, lg = scene
    hits, _ = _hit_points(R, torch, scene, pose, N_POINTS)
    dirs = R.ao_directions(16)
    params = lambda first: R.ao_params(2, 6.0, 1e-3, 77 + first, R.AO_JITTER)  # noqa: E731
    d = torch.from_numpy(dirs).cuda()
    ctx = _context(R, sph, lg)
    try:
        cnt, = _batch(torch, N_POINTS, 32, [(1, torch.int16, False)],
                      lambda first, count, dst: ctx.ao_device(
                          hits.ptr(first), count, params(first), d.data_ptr(), 16, dst[0],
                          stream=_stream(torch)))
    finally:
        ctx.close()
    _, seen = _windows(N_POINTS, [32, 2], [hits], [cnt],
                       lambda lo, h: R.ao_host(sph, h.view(R.HIT_DTYPE).reshape(-1), dirs,
                                               params(lo), walk=0, threads=THREADS), "ao")
    c = np.concatenate([s[0].reshape(-1) for s in seen])
    assert len(np.unique(c)) >= 2, "the windows hold one count only"


def test_matte(R, torch_cuda, scenes, pose):
    """matte_device with the lit mask."""
    torch = torch_cuda
    with device_memory(torch, _points_need(12 + 8), "matte"):
        _matte_body(R, torch, scenes["c3"], pose)


def _matte_body(R, torch, scene, pose):
    sph, lg = scene
    hits, _ = _hit_points(R, torch, scene, pose, N_POINTS)
    ctx = _context(R, sph, lg)
    try:
        col, lit = _batch(torch, N_POINTS, 32, [(3, None, True), (1, torch.int64, False)],
                          lambda first, count, dst: ctx.matte_device(
                              hits.ptr(first), count, dst[0], lit_ptr=dst[1],
                              stream=_stream(torch)))
    finally:
        ctx.close()

    def reference(lo, h):
        c, m = R.matte_host(sph, lg, h.view(R.HIT_DTYPE).reshape(-1), walk=0, threads=THREADS,
                            mask=True)
        return [c, m.reshape(-1, 1)]

    _, seen = _windows(N_POINTS, [32, 12, 8], [hits], [col, lit], reference, "matte")
    m = np.concatenate([s[1].reshape(-1) for s in seen])
    assert len(np.unique(m)) >= 2, "the windows hold one mask only"


def test_contains(R, torch_cuda, scenes, pose):
    """contains_device on the records' points."""
    torch = torch_cuda
    with device_memory(torch, _points_need(4), "contains"):
        _contains_body(R, torch, scenes["c3"], pose)


def _contains_body(R, torch, scene, pose):
    sph, lg = scene
    hits, pts = _hit_points(R, torch, scene, pose, N_POINTS)
    del hits
    ctx = _context(R, sph, lg)
    try:
        ids, = _batch(torch, N_POINTS, 12, [(1, None, False)],
                      lambda first, count, dst: ctx.contains_device(
                          pts.ptr(first), count, dst[0], stream=_stream(torch)))
    finally:
        ctx.close()
    _windows(N_POINTS, [12, 4, 32], [pts], [ids],
             lambda lo, p: R.contains_host(sph, _f32(p), walk=0, threads=THREADS), "contains")


def test_gather(R, torch_cuda, scenes, pose):
    """gather_device, K = 1 of a jittered table of 16, stack size 3, with the
    skipped counts."""
    torch = torch_cuda
    with device_memory(torch, _points_need(12 + 2), "gather"):
        _gather_body(R, torch, scenes["c3"], pose)


def _gather_body(R, torch, scene, pose):
    sph, lg = scene
    hits, _ = _hit_points(R, torch, scene, pose, N_POINTS)
    dirs = R.ao_directions(16)
    wts = (np.arange(16, dtype=np.float32) + 1) / 16
    flags = R.GATHER_JITTER | R.GATHER_SKIP_NONFINITE
    params = lambda first: R.gather_params(1, 1e-3, 5 + first, flags)  # noqa: E731
    d, w = torch.from_numpy(dirs).cuda(), torch.from_numpy(wts).cuda()
    ctx = _context(R, sph, lg)
    try:
        col, skp = _batch(torch, N_POINTS, 32, [(3, None, True), (1, torch.int16, False)],
                          lambda first, count, dst: ctx.gather_device(
                              hits.ptr(first), count, params(first), d.data_ptr(), w.data_ptr(),
                              16, dst[0], skipped_ptr=dst[1], stack_size=3,
                              stream=_stream(torch)))
    finally:
        ctx.close()

    def reference(lo, h):
        c, s = R.gather_host(sph, lg, h.view(R.HIT_DTYPE).reshape(-1), dirs, wts, params(lo),
                             stack_size=3, walk=0, threads=THREADS, skipped=True)
        return [c, s.reshape(-1, 1)]

    _, seen = _windows(N_POINTS, [32, 12, 2], [hits], [col, skp], reference, "gather")
    c = np.concatenate([s[0] for s in seen])
    assert (np.nan_to_num(c) != 0).any()


@pytest.mark.parametrize("call", ["ao_segments", "gather_rays"])
def test_probe_records(R, torch_cuda, scenes, pose, call):
    """4 194 368 points x K = 64: 268 M records, 6.4 GB, byte 2^32 crossed
    through n * K with a small n.  Sub-batches are taken over the points."""
    torch = torch_cuda
    n, k = N_PROBE_POINTS, PROBE_K
    need = max(N_RAYS * 24 + n * 32, n * 32 + (n + n // 2 + 2 * PAD) * k * 24) + SLACK
    with device_memory(torch, need, call):
        _probe_body(R, torch, scenes["c3"], pose, call)


def _probe_body(R, torch, scene, pose, call):
    n, k = N_PROBE_POINTS, PROBE_K
    # records of the frame's middle rows, where the scene is
    first_ray = (RAYS_H // 2) * RAYS_W - n // 2
    sph, lg = scene
    ctx = _context(R, sph, lg)
    try:
        rays = _camera_rays(R, torch, ctx, pose)
        hits = Dest(torch, n, 8)
        ctx.intersect_device(rays.ptr(first_ray), n, hits.ptr(), stream=_stream(torch))
        torch.cuda.synchronize()
        del rays
        torch.cuda.empty_cache()
        dirs = R.ao_directions(256)
        d = torch.from_numpy(dirs).cuda()
        if call == "ao_segments":
            params = lambda first: R.ao_params(k, 6.0, 1e-3, 9 + first, R.AO_JITTER)  # noqa: E731
            fn, host = ctx.ao_segments_device, R.ao_segments_host
        else:
            params = lambda first: R.gather_params(k, 1e-3, 9 + first,  # noqa: E731
                                                   R.GATHER_JITTER)
            fn, host = ctx.gather_rays_device, R.gather_rays_host
        rec, = _batch(torch, n, 24 * k, [(6 * k, None, True)],
                      lambda first, count, dst: fn(hits.ptr(first), count, params(first),
                                                   d.data_ptr(), 256, dst[0],
                                                   stream=_stream(torch)))
    finally:
        ctx.close()
    assert n * k * 24 > BYTE_LIMIT
    # windows of the records, as whole points
    spans = [(lo // k, -(-hi // k)) for lo, hi in largegen.windows(n * k, 24)]
    ids = []
    for lo, hi in spans:
        h = to_host(hits.t, [(lo, hi)], 8).view(R.HIT_DTYPE).reshape(-1)
        want = host(h, dirs, params(lo), threads=THREADS).reshape(hi - lo, 6 * k)
        _same_words(rec.host(lo, hi), want, True, f"{call}, points [{lo}, {hi})")
        ids.append(h["id"])
    assert (np.concatenate(ids) >= 0).any(), "the windows hold no hit"


# ===================================================================== 4. ordering
def test_ray_order(R, torch_cuda, scenes, pose):
    """ray_order over the first 178 957 056 rays (4.29 GB) on scene 200."""
    torch = torch_cuda
    n = N_ORDER
    need = N_RAYS * 24 + n * (4 + 8) + R.ray_order_scratch(n) + n * 40 + SLACK
    with device_memory(torch, need, "ray_order"):
        _order_body(R, torch, scenes[200], pose)


def _order_body(R, torch, scene, pose):
    n = N_ORDER
    sph, lg = scene
    nbytes = R.ray_order_scratch(n)
    ctx = _context(R, sph, lg)
    try:
        rays = _camera_rays(R, torch, ctx, pose)
        order, keys = Dest(torch, n, 1), Dest(torch, n, 1, torch.int64)
        scratch = Dest(torch, nbytes // 4, 1)
        ctx.ray_order(rays.ptr(), n, order.ptr(), scratch.ptr(), nbytes, keys_ptr=keys.ptr(),
                      stream=_stream(torch))
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert order.tail_kept() and keys.tail_kept() and scratch.tail_kept()
    del scratch
    torch.cuda.empty_cache()
    o, k = order.values(0, n), keys.values(0, n)  # indices below 2^31: int32 holds them
    assert torch.equal(torch.sort(o).values, torch.arange(n, dtype=torch.int32, device="cuda")), \
        "the order is no permutation"
    along = k[o.long()]
    assert bool((along[1:] >= along[:-1]).all()), "keys decrease along the order"
    tie = along[1:] == along[:-1]
    assert bool((o[1:][tie] > o[:-1][tie]).all()), "equal keys out of index order"
    assert int(tie.sum()) > 0 and int((~tie).sum()) > 1000
    del tie
    r = rays.t[:N_RAYS * 6].view(N_RAYS, 6)
    # the keys of rays i in the windows of the ray buffer, and of rays order[j]
    # for j in the windows of the order
    for what, spans, index in (("rays", largegen.windows(n, 24), None),
                               ("order", largegen.windows(n, 4), o)):
        for lo, hi in spans:
            idx = torch.arange(lo, hi, device="cuda") if index is None else index[lo:hi].long()
            got = (k[idx] if index is None else along[lo:hi]).cpu().numpy().view(np.uint64)
            some = r[idx].cpu().numpy().view(np.float32)
            _, want = R.ray_order_host(sph, some, threads=THREADS, keys=True)
            assert (got == want).all(), f"keys of {what} [{lo}, {hi}) differ from the host's"


# ===================================================================== 5. render family
def _rows_equal_frame(R, torch, ctx, frame, W, H, aa, S):
    """The frame against render_rows_device over three consecutive row ranges,
    each below 2^32 bytes."""
    b = cuts(H, W * 12, least=3)
    most = max(hi - lo for lo, hi in zip(b, b[1:]))
    rows = torch.arange(H, dtype=torch.int32, device="cuda")
    sub = Dest(torch, most * W, 3, None, True)
    for lo, hi in zip(b, b[1:]):
        sub.refill()
        ctx.render_rows_device(W, H, rows.data_ptr() + 4 * lo, hi - lo, sub.ptr(),
                               zoom=ZOOM, alias_factor=aa, stack_size=S,
                               stream=_stream(torch))
        torch.cuda.synchronize()
        assert sub.tail_kept((hi - lo) * W), f"written past rows [{lo}, {hi})"
        diff = first_difference(torch, frame.values(lo * W, hi * W),
                                sub.values(0, (hi - lo) * W), True)
        assert diff is None, (f"rows [{lo}, {hi}): word {diff[0]} is {diff[1]:#x} in the frame, "
                              f"{diff[2]:#x} in render_rows_device")


def _shards_equal_frame(R, torch, frame, W, H, items, render_shard, canon):
    """The frame against its row-cyclic shards (3 shards, blocks of 5 rows)
    put back in row order with torch."""
    G, B = 3, 5
    whole = Dest(torch, W * H, items, None, canon)
    for g in range(G):
        n_rows = R.shard_rows(H, B, g, G)
        shard = Dest(torch, n_rows * W, items, None, canon)
        assert n_rows * W * items * 4 < BYTE_LIMIT
        render_shard(shard.ptr(), B, g, G)
        torch.cuda.synchronize()
        assert shard.tail_kept(), f"written past shard {g}"
        idx = torch.from_numpy(R.shard_row_indices(H, B, g, G).astype(np.int64)).cuda()
        whole.t[:W * H * items].view(H, W * items).index_copy_(
            0, idx, shard.t[:n_rows * W * items].view(n_rows, W * items))
        del shard
    diff = first_difference(torch, frame.values(0, W * H), whole.values(0, W * H), canon)
    assert diff is None, f"word {diff[0]} is {diff[1]:#x} in the frame, {diff[2]:#x} in its shards"


RENDERS = {  # scene, H, aa, stack size, shards too
    "c3-aa1": ("c3", 21845, 1.0, 6, True),
    "c3-aa3": ("c3", 10923, 3.0, 6, False),
    "c5-aa1": ("c5", 10923, 1.0, 3, False),
}


@pytest.mark.parametrize("case", sorted(RENDERS))
def test_render_device(R, torch_cuda, oracle, scenes, case):
    """Frames 32771 wide (odd, no power of two, a row pitch that is no
    multiple of 64 bytes): 8.59 GB at aa 1 on c3 (byte 2^32 and word 2^31),
    4.30 GB at aa 3 (7 pixels per wave, ragged at every row end) and on c5."""
    torch = torch_cuda
    name, H, aa, S, shards = RENDERS[case]
    n = RENDER_W * H
    need = n * 12 * (2 if shards else 1) + (n // 3 + 2 * RENDER_W) * 12 + SLACK
    with device_memory(torch, need, f"render_device[{case}]"):
        _render_body(R, torch, oracle, scenes[name], H, aa, S, shards)


def _render_body(R, torch, oracle, scene, H, aa, S, shards):
    sph, lg = scene
    W = RENDER_W
    ctx = _context(R, sph, lg)
    try:
        frame = Dest(torch, W * H, 3, None, True)
        ctx.render_device(W, H, frame.ptr(), zoom=ZOOM, alias_factor=aa, stack_size=S,
                          stream=_stream(torch))
        torch.cuda.synchronize()
        assert frame.tail_kept(), "written past the frame"
        _rows_equal_frame(R, torch, ctx, frame, W, H, aa, S)
        if shards:
            _shards_equal_frame(
                R, torch, frame, W, H, 3,
                lambda ptr, B, g, G: ctx.render_device(
                    W, H, ptr, zoom=ZOOM, alias_factor=aa, stack_size=S, row_block=B,
                    shard=g, n_shards=G, stream=_stream(torch)), True)
    finally:
        ctx.close()
    rows = threshold_rows(W, H, 12)
    want = oracle.render(sph, lg, W, H, S, rows=rows, aa=aa, zoom=ZOOM)
    got = np.stack([frame.host(int(r) * W, (int(r) + 1) * W) for r in rows])
    _same_words(got.reshape(-1, 3), want.reshape(-1, 3), True, f"rows {list(rows)}")
    assert (np.nan_to_num(want) != 0).any(), "black rows"


def test_gbuffer_device(R, torch_cuda, scenes):
    """32771 x 4097 records of 32 bytes at aa 3: byte 2^32.  All pixels against
    the row-cyclic shards, the threshold rows against the numpy restatement
    of the record's definition (test_gbuffer_host.restate)."""
    torch = torch_cuda
    n = RENDER_W * 4097
    with device_memory(torch, n * 32 * 2 + (n // 3 + RENDER_W * 8) * 32 + SLACK, "gbuffer_device"):
        _gbuffer_body(R, torch, scenes["c3"])


def _gbuffer_body(R, torch, scene):
    sph, lg = scene
    W, H, aa = RENDER_W, 4097, 3.0
    ctx = _context(R, sph, lg)
    try:
        frame = Dest(torch, W * H, 8)
        ctx.gbuffer_device(W, H, frame.ptr(), zoom=ZOOM, alias_factor=aa,
                           stream=_stream(torch))
        torch.cuda.synchronize()
        assert frame.tail_kept(), "written past the frame"
        _shards_equal_frame(
            R, torch, frame, W, H, 8,
            lambda ptr, B, g, G: ctx.gbuffer_device(W, H, ptr, zoom=ZOOM, alias_factor=aa,
                                                    row_block=B, shard=g, n_shards=G,
                                                    stream=_stream(torch)), False)
    finally:
        ctx.close()
    rows = threshold_rows(W, H, 32)
    want = restate_gbuffer(R, sph, W, H, ZOOM, aa, rows=rows)
    got = np.stack([frame.host(int(r) * W, (int(r) + 1) * W) for r in rows])
    _same_words(got.reshape(-1, 8), want.view(np.uint32).reshape(-1, 8), False,
                f"rows {list(rows)}")
    assert (want["id"] >= 0).any() and (want["id"] < 0).any()


def test_render_camera(R, torch_cuda, scenes, pose):
    """render_camera of the look-at pose, 32771 x 10923 at aa 1: every pixel is
    0 + 1 * rayTrace's colour of its ray (main.cpp:442-445 with one sample), so
    all pixels are raytrace_device over camera_rays in sub-batches, and the
    threshold rows raytrace_host (walk 0) of those rows' device-made rays."""
    torch = torch_cuda
    n = RENDER_W * 10923
    with device_memory(torch, n * (12 + 24) + (n // 2 + 200) * 12 + SLACK, "render_camera"):
        _render_camera_body(R, torch, scenes["c3"], pose)


def _ray_route(R, torch, ctx, sph, lg, pose, W, H, S, frame, first_pixel, what):
    """A posed aa 1 frame of W x H at `frame` (a Dest, its pixels from
    first_pixel on) against raytrace_device over camera_rays in sub-batches,
    and its threshold windows against raytrace_host of the device's rays."""
    n = W * H
    rays = Dest(torch, n, 6, None, True)
    ctx.camera_rays(pose, W, H, rays.ptr(), ZOOM, 1.0, stream=_stream(torch))
    torch.cuda.synchronize()
    assert rays.tail_kept()
    b = cuts(n, 24)
    most = max(hi - lo for lo, hi in zip(b, b[1:]))
    sub = Dest(torch, most, 3, None, True)
    for lo, hi in zip(b, b[1:]):
        sub.refill()
        ctx.raytrace_device(rays.ptr(lo), hi - lo, sub.ptr(), stack_size=S, stream=_stream(torch))
        torch.cuda.synchronize()
        assert sub.tail_kept(hi - lo)
        v = sub.values(0, hi - lo)
        # 0 + 1 * colour: the colour, a -0 as +0
        v.masked_fill_(v == -(1 << 31), 0)
        diff = first_difference(torch, frame.values(first_pixel + lo, first_pixel + hi), v, True)
        assert diff is None, (f"{what}, pixels [{lo}, {hi}): word {diff[0]} is {diff[1]:#x} in "
                              f"the frame, {diff[2]:#x} from raytrace_device")
    return rays


def _ray_windows(R, sph, lg, S, rays, frame, first_pixel, spans, what):
    lit = False
    for lo, hi in spans:
        r = _f32(to_host(rays.t, [(lo, hi)], 6))
        col = R.raytrace_host(sph, lg, r, stack_size=S, walk=0, threads=THREADS)
        with np.errstate(invalid="ignore"):
            want = np.float32(0) + col * np.float32(1)
        _same_words(frame.host(first_pixel + lo, first_pixel + hi), want, True,
                    f"{what}, pixels [{lo}, {hi})")
        lit = lit or bool((np.nan_to_num(want) != 0).any())
    return lit


def _render_camera_body(R, torch, scene, pose):
    sph, lg = scene
    W, H, S = RENDER_W, 10923, 6
    ctx = _context(R, sph, lg)
    try:
        frame = Dest(torch, W * H, 3, None, True)
        ctx.render_camera(pose, W, H, frame.ptr(), zoom=ZOOM, alias_factor=1.0, stack_size=S,
                          stream=_stream(torch))
        torch.cuda.synchronize()
        assert frame.tail_kept(), "written past the frame"
        rays = _ray_route(R, torch, ctx, sph, lg, pose, W, H, S, frame, 0, "render_camera")
    finally:
        ctx.close()
    spans = [(int(r) * W, (int(r) + 1) * W) for r in threshold_rows(W, H, 12)]
    assert _ray_windows(R, sph, lg, S, rays, frame, 0, spans, "render_camera"), "black rows"


# ===================================================================== 6. views
def _view_poses(R, pose):
    """camera_cube's six poses about a point among the spheres and the look-at."""
    cube = np.asarray(R.camera_cube([0.0, 0.0, -12.0])).reshape(6).view(np.float32).reshape(6, 12)
    return np.concatenate([cube, pose.reshape(1, 12)]).astype(np.float32)


def test_render_views(R, torch_cuda, scenes, pose):
    """7 views of 8192 x 8192 at aa 1: 5.6 GB of frames, view 5 straddles byte
    2^32.  All pixels: the calls over views [0, 3) and [3, 7), the table and
    the destination advanced, and every view by the ray route; windows by
    raytrace_host of the device's rays."""
    torch = torch_cuda
    px = VIEW_W * VIEW_W
    need = VIEWS * px * 12 + 4 * px * 12 + px * (24 + 12) + SLACK
    with device_memory(torch, need, "render_views"):
        _views_body(R, torch, scenes["c3"], pose)


def _views_body(R, torch, scene, pose):
    sph, lg = scene
    W = H = VIEW_W
    px, S = W * H, 3
    poses = _view_poses(R, pose)
    cams = torch.from_numpy(poses).cuda()
    ctx = _context(R, sph, lg)
    try:
        frames = Dest(torch, VIEWS * px, 3, None, True)
        ctx.render_views(cams.data_ptr(), VIEWS, W, H, frames.ptr(), zoom=ZOOM, alias_factor=1.0,
                         stack_size=S, stream=_stream(torch))
        torch.cuda.synchronize()
        assert frames.tail_kept(), "written past the frames"
        sub = Dest(torch, 4 * px, 3, None, True)
        for lo, hi in ((0, 3), (3, 7)):
            sub.refill()
            ctx.render_views(cams.data_ptr() + 48 * lo, hi - lo, W, H, sub.ptr(), zoom=ZOOM,
                             alias_factor=1.0, stack_size=S, stream=_stream(torch))
            torch.cuda.synchronize()
            assert sub.tail_kept((hi - lo) * px)
            diff = first_difference(torch, frames.values(lo * px, hi * px),
                                    sub.values(0, (hi - lo) * px), True)
            assert diff is None, f"views [{lo}, {hi}): word {diff[0]}: {diff[1]:#x} / {diff[2]:#x}"
        del sub
        torch.cuda.empty_cache()
        spans = largegen.windows(VIEWS * px, 12)
        lit = False
        for v in range(VIEWS):
            rays = _ray_route(R, torch, ctx, sph, lg, poses[v].reshape(4, 3), W, H, S, frames,
                              v * px, f"view {v}")
            mine = [(max(lo, v * px) - v * px, min(hi, (v + 1) * px) - v * px)
                    for lo, hi in spans if lo < (v + 1) * px and hi > v * px]
            lit = _ray_windows(R, sph, lg, S, rays, frames, v * px, mine, f"view {v}") or lit
            del rays
    finally:
        ctx.close()
    assert lit, "black windows"


FOLDS = {"groups-of-1": (1, 2, 256), "one-group": (7, 3, 2048)}  # G, K, one pixel in `sparse` set


@pytest.mark.parametrize("case", sorted(FOLDS))
def test_views_fold(R, torch_cuda, case):
    """views_fold_device over 7 frames of 8192 x 8192 (5.6 GB) that hold small
    integers: every `sparse`-th pixel one of 0 .. 15 per channel, the rest 0,
    under weights 1, 2 and 4.  Every term is an integer and a group's terms
    sum to less than 2^24, so every partial sum is exact in float whatever the
    order, and the coefficients are torch's int64 sums.  Seven groups of one
    view (the frames pass byte 2^32) and one group of seven with K = 3 (the
    weight table, 5.6 GB, passes it too)."""
    torch = torch_cuda
    G, K, sparse = FOLDS[case]
    px = VIEW_W * VIEW_W
    need = VIEWS * px * 12 + G * px * K * 4 + R.views_fold_scratch(VIEWS, VIEW_W, VIEW_W, K) \
        + px * 8 * 16 + SLACK  # torch's int64 temporaries of one view
    with device_memory(torch, need, f"views_fold[{case}]"):
        _fold_body(R, torch, G, K, sparse)


def _fold_body(R, torch, G, K, sparse):
    W = H = VIEW_W
    px = W * H
    frames = Dest(torch, VIEWS * px, 3, None, True)
    wts = Dest(torch, G * px * K, 1, None, True)
    e = torch.arange(px, device="cuda")

    def mixed(x, salt):  # 32 scrambled bits of every element of an int64 tensor
        x = ((x ^ (x >> 13)) * 0x9E3779B1 + salt) & 0xFFFFFFFF
        x = ((x ^ (x >> 16)) * 0x85EBCA6B) & 0xFFFFFFFF
        return x ^ (x >> 15)

    want = torch.zeros((VIEWS // G, K, 3), dtype=torch.int64, device="cuda")
    most = [0] * (VIEWS // G)  # a bound of every partial sum of the group's terms
    for v in range(VIEWS):
        g, f = divmod(v, G)
        h = mixed(e + v * px, 1)
        val = torch.stack([(h >> (5 * c)) & 15 for c in range(3)], 1)
        val = val * ((e + v) % sparse == 0)[:, None]
        wt = torch.stack([2 ** (mixed(e + f * px, 77 + k) % 3) for k in range(K)], 1)
        frames.t[v * px * 3:(v + 1) * px * 3].view(torch.float32).copy_(val.reshape(-1))
        if g == 0:
            wts.t[f * px * K:(f + 1) * px * K].view(torch.float32).copy_(wt.reshape(-1))
        for k in range(K):
            want[g, k] += (val * wt[:, k:k + 1]).sum(0)
        most[g] += 4 * int(val.amax(1).sum())
        del h, val, wt
    del e
    assert max(most) < 1 << 24, most
    params = R.fold_params(G, K)
    nbytes = R.views_fold_scratch(VIEWS, W, H, K)
    scratch = Dest(torch, nbytes // 4, 1)
    out = Dest(torch, (VIEWS // G) * K, 3, None, True)
    ctx = R.Context(0)
    try:
        ctx.views_fold(frames.ptr(), VIEWS, W, H, params, wts.ptr(), out.ptr(), scratch.ptr(),
                       nbytes, stream=_stream(torch))
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert out.tail_kept() and scratch.tail_kept() and frames.tail_kept() and wts.tail_kept()
    got = out.values(0, (VIEWS // G) * K).view(torch.float32).view(VIEWS // G, K, 3)
    print(f"views_fold G {G} K {K}: coefficients {got.flatten().tolist()}")
    assert int(want.max()) < 1 << 24 and int(want.min()) > 0
    assert torch.equal(got.to(torch.int64), want) and torch.equal(got, want.float())


# ===================================================================== 7. frame filters
# A horizontal band of full-width rows is itself a contiguous frame, and a
# pixel's result depends on the rows within `halo` of it only: the call on a
# band (the base pointers advanced by whole rows) gives the full call's words
# on every row at least `halo` rows inside the band, or at the frame's own edge.
FILTER_W = largegen.FILTER_W
ALL_FLAGS = 1 | 2 | 4 | 8  # FILTER_SAME_ID | NORMAL | PLANE | SKIP_NONFINITE
PLANE_SCALE = 0.2  # 1 / c3's largest radius, as filtergen.plane_scale


def _guides(R, torch, scene, pose, W, H):
    """The hit records of the pose's aa 1 rays of a W x H frame."""
    sph, lg = scene
    ctx = _context(R, sph, lg)
    try:
        rays = Dest(torch, W * H, 6, None, True)
        ctx.camera_rays(pose, W, H, rays.ptr(), ZOOM, 1.0, stream=_stream(torch))
        hits = Dest(torch, W * H, 8)
        ctx.intersect_device(rays.ptr(), W * H, hits.ptr(), stream=_stream(torch))
        torch.cuda.synchronize()
        assert rays.tail_kept() and hits.tail_kept()
    finally:
        ctx.close()
    return hits


def _column(torch, hits, n, lo, hi):
    """Words [lo, hi) of every hit record as a buffer of its own."""
    out = Dest(torch, n, hi - lo, None, True)
    out.t[:n * (hi - lo)].view(n, hi - lo).copy_(hits.t[:n * 8].view(n, 8)[:, lo:hi])
    return out


def _scratch(torch, nbytes):
    return Dest(torch, nbytes // 4, 1) if nbytes else None


def _frame_check(R, torch, W, H, halo, ins, specs, call, host, what):
    """call(rows, input pointers, output pointers) on the whole frame, on three
    overlapping bands, and host(rows, inputs) on a band around every threshold
    row of every buffer, 16 rows of it compared."""
    n = W * H
    strides = [d.stride for d in ins] + [s[0] * 4 for s in specs]
    full = [Dest(torch, n, *s) for s in specs]
    call(H, [d.ptr() for d in ins], [d.ptr() for d in full])
    for k, d in enumerate(full):
        assert d.tail_kept(), f"{what}, output {k}: written past the frame"
    t = [0, H // 3 + 5, 2 * H // 3 + 11, H]  # no multiples of the 8-row tiles
    bands = [(max(0, a - halo), min(H, b + halo), a, b) for a, b in zip(t, t[1:])]
    most = max(hi - lo for lo, hi, _, _ in bands)
    assert most * W * max(strides) < BYTE_LIMIT
    sub = [Dest(torch, most * W, *s) for s in specs]
    for lo, hi, a, b in bands:
        for d in sub:
            d.refill()
        call(hi - lo, [d.ptr(lo * W) for d in ins], [d.ptr() for d in sub])
        for k, (f, s) in enumerate(zip(full, sub)):
            assert s.tail_kept((hi - lo) * W), f"{what}, output {k}: written past the band"
            diff = first_difference(torch, f.values(a * W, b * W),
                                    s.values((a - lo) * W, (b - lo) * W), f.canon)
            assert diff is None, (f"{what}, output {k}, rows [{a}, {b}) of band [{lo}, {hi}): "
                                  f"word {diff[0]} is {diff[1]:#x} in the frame, {diff[2]:#x} "
                                  f"in the band")
    del sub
    centres = {8, H - 8}
    for s in strides:
        for limit in (BYTE_LIMIT, 4 * largegen.WORD_LIMIT):
            if n * s > limit:
                centres.add(limit // s // W)
    for c in sorted(centres):
        a, b = max(0, c - 8), min(H, c + 8)
        lo, hi = max(0, a - halo), min(H, b + halo)
        host_in = [to_host(d.t, [(lo * W, hi * W)], d.items) for d in ins]
        want = host(hi - lo, *host_in)
        for k, (d, w) in enumerate(zip(full, want)):
            w = np.asarray(w).reshape(hi - lo, W, -1)[a - lo:b - lo].reshape((b - a) * W, -1)
            _same_words(d.host(a * W, b * W), w, d.canon, f"{what}, output {k}, rows [{a}, {b})")
        ids = host_in[0].reshape(hi - lo, W, 8)[a - lo:b - lo, :, 0]
        assert (ids < 0).any() and len(np.unique(ids[ids >= 0])) >= 2, \
            f"{what}: rows [{a}, {b}) hold {np.unique(ids)} only"
    return full


def _hit_records(R, h):
    return np.ascontiguousarray(h).view(R.HIT_DTYPE).reshape(-1)


FILTERS = {  # H, the signal, passes
    "count-p3": (8192, "count", 3),
    "gray-p5": (8192, "gray", 5),  # steps 8 and 16 take the direct form
    "rgb-p2": (21846, "rgb", 2),
}


@pytest.mark.parametrize("case", sorted(FILTERS))
def test_filter_device(R, torch_cuda, scenes, pose, case):
    """filter_device on frames 16387 wide: 8192 rows (the records pass byte
    2^32) with ao_device's counts (K = 7) and with the records' t, and 21846
    rows (the rgb planes pass byte 2^32, the records word 2^31) with the
    records' normals as colours."""
    torch = torch_cuda
    H, signal, passes = FILTERS[case]
    n, c = FILTER_W * H, {"count": 2, "gray": 4, "rgb": 12}[signal]
    out = 12 if signal == "rgb" else 4  # the result, and the ping-pong scratch as large
    need = max(n * (24 + 32), n * (32 + c + 2 * out) + (n // 3 + 20 * FILTER_W) * 2 * out) + SLACK
    with device_memory(torch, need, f"filter_device[{case}]"):
        _filter_body(R, torch, scenes["c3"], pose, H, signal, passes)


def _filter_body(R, torch, scene, pose, H, signal, passes):
    W, n = FILTER_W, FILTER_W * H
    sph, lg = scene
    hits = _guides(R, torch, scene, pose, W, H)
    ctx = _context(R, sph, lg)
    try:
        if signal == "count":
            src = Dest(torch, n, 1, torch.int16)
            d = torch.from_numpy(R.ao_directions(16)).cuda()
            ctx.ao_device(hits.ptr(), n, R.ao_params(7, 6.0), d.data_ptr(), 16, src.ptr(),
                          stream=_stream(torch))
            torch.cuda.synchronize()
            assert src.tail_kept()
        elif signal == "gray":
            src = _column(torch, hits, n, 1, 2)
        else:
            src = _column(torch, hits, n, 5, 8)
        kind = {"rgb": R.FILTER_RGB, "gray": R.FILTER_GRAY, "count": R.FILTER_COUNT}[signal]
        params = R.filter_params(passes, kind, ALL_FLAGS, PLANE_SCALE, 3)

        def call(rows, ins, outs):
            nb = R.filter_scratch(W, rows, params)
            scr = _scratch(torch, nb)
            ctx.filter_device(ins[0], W, rows, params, ins[1], outs[0], scr.ptr() if scr else 0,
                              nb, stream=_stream(torch))
            torch.cuda.synchronize()
            assert scr is None or scr.tail_kept(), "written past the scratch"

        def host(rows, h, s):
            s = s.view(np.uint16) if signal == "count" else _f32(s)
            return [R.filter_host(_hit_records(R, h), W, rows, params, s, threads=THREADS)]

        _frame_check(R, torch, W, H, 2 * (2 ** passes - 1), [hits, src],
                     [(3 if signal == "rgb" else 1, None, True)], call, host, f"filter {signal}")
    finally:
        ctx.close()


@pytest.mark.parametrize("lengths", ["seeded", "zero"])
def test_variance_device(R, torch_cuda, scenes, pose, lengths):
    """variance_device, gray, 16387 x 8192: moments made on the device as
    svgfgen.state makes them (acc in [0, 2), m2 = acc^2 + noise in [0, 0.5)),
    history lengths seeded in 0 .. 8 (some below minHistory 4: the spatial
    estimate) or all 0 (every tile with a hit stages its window)."""
    torch = torch_cuda
    n = FILTER_W * 8192
    with device_memory(torch, max(n * (24 + 32), n * (32 + 4 + 4 + 2 + 4 + 2)) + SLACK,
                       f"variance_device[{lengths}]"):
        _variance_body(R, torch, scenes["c3"], pose, lengths)


def _variance_body(R, torch, scene, pose, lengths):
    W, H = FILTER_W, 8192
    n = W * H
    hits = _guides(R, torch, scene, pose, W, H)
    gen = torch.Generator(device="cuda").manual_seed(8200)
    acc, m2 = Dest(torch, n, 1, None, True), Dest(torch, n, 1, None, True)
    ln = Dest(torch, n, 1, torch.int16)
    a = torch.rand(n, generator=gen, device="cuda") * 2
    acc.t[:n].view(torch.float32).copy_(a)
    m2.t[:n].view(torch.float32).copy_(a * a + torch.rand(n, generator=gen, device="cuda") * 0.5)
    del a
    if lengths == "seeded":
        ln.t[:n].copy_(torch.randint(0, 9, (n,), generator=gen, device="cuda", dtype=torch.int16))
    else:
        ln.t[:n].zero_()
    params = R.variance_params(R.FILTER_GRAY, ALL_FLAGS, PLANE_SCALE, 3, 4)
    ctx = R.Context(0)
    try:
        def call(rows, ins, outs):
            ctx.variance_device(ins[0], W, rows, params, ins[1], ins[2], ins[3], outs[0],
                                stream=_stream(torch))
            torch.cuda.synchronize()

        def host(rows, h, a, m, l):
            return [R.variance_host(_hit_records(R, h), W, rows, params, _f32(a), _f32(m),
                                    l.view(np.uint16), threads=THREADS)]

        var, = _frame_check(R, torch, W, H, 3, [hits, acc, m2, ln], [(1, None, True)], call, host,
                            f"variance {lengths}")
        v = var.values(0, n).view(torch.float32)
        assert float(v.max()) > 0
    finally:
        ctx.close()


def test_svgf_device(R, torch_cuda, scenes, pose):
    """svgf_device, gray, 3 passes, every flag and the luminance term, 16387 x
    8192: the records' t as the signal, a seeded variance in [0, 0.5)."""
    torch = torch_cuda
    n = FILTER_W * 8192
    with device_memory(torch, max(n * (24 + 32), n * (32 + 8 + 8 + 8) + n * 8) + SLACK,
                       "svgf_device"):
        _svgf_body(R, torch, scenes["c3"], pose)


def _svgf_body(R, torch, scene, pose):
    W, H, passes = FILTER_W, 8192, 3
    n = W * H
    hits = _guides(R, torch, scene, pose, W, H)
    src = _column(torch, hits, n, 1, 2)
    var = Dest(torch, n, 1, None, True)
    gen = torch.Generator(device="cuda").manual_seed(8100)
    var.t[:n].view(torch.float32).copy_(torch.rand(n, generator=gen, device="cuda") * 0.5)
    params = R.svgf_params(passes, R.FILTER_GRAY, ALL_FLAGS | R.SVGF_LUMA, PLANE_SCALE, 3)
    ctx = R.Context(0)
    try:
        def call(rows, ins, outs):
            nb = R.svgf_scratch(W, rows, params)
            scr = _scratch(torch, nb)
            ctx.svgf_device(ins[0], W, rows, params, ins[1], ins[2], outs[0], outs[1],
                            scr.ptr() if scr else 0, nb, stream=_stream(torch))
            torch.cuda.synchronize()
            assert scr is None or scr.tail_kept(), "written past the scratch"

        def host(rows, h, s, v):
            return list(R.svgf_host(_hit_records(R, h), W, rows, params, _f32(s), _f32(v),
                                    threads=THREADS))

        _frame_check(R, torch, W, H, 2 * (2 ** passes - 1) + 1, [hits, src, var],
                     [(1, None, True), (1, None, True)], call, host, "svgf")
    finally:
        ctx.close()
