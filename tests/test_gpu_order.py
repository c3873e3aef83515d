"""GPU tests of the ray order (rtg_ray_order_device, csrc/rtg_order.hip) and the
indexed launches (rtg_intersect_indexed_device, rtg_visible_indexed_device,
rtg_raytrace_indexed_device) on an MI355X: the device sort against the host
form (rtg_ray_order_host, pinned in test_order_host.py) word for word, keys
and order; the indexed launches against the un-indexed ones and the host's
plain loops, byte for byte.  Batches are small.
"""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import raygen
from conftest import GOLDEN, PKG, ROOT, bits_equal, first_mismatch, load_f32, load_scene
from raygen import scene
from test_order_host import check_order, host_mix, key_scenes, ladder_batch, restate_keys
from test_raytrace_host import THREADS, mixed_rays, scene_with_lights

pytestmark = pytest.mark.gpu

PAD = 64  # records the destinations are longer than the batch
FILL = 0x5A5A5A5A


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


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _order(R, torch, ctx, rays, kind=0):
    """(order, keys) of the device sort; both buffers are pre-filled and PAD
    entries longer, the tails must stay."""
    n = len(rays)
    src = torch.from_numpy(np.ascontiguousarray(rays, np.float32).reshape(-1, 6)).cuda()
    order = torch.full((n + PAD,), FILL, dtype=torch.int32, device="cuda")
    keys = torch.full((n + PAD,), FILL, dtype=torch.int64, device="cuda")
    nbytes = R.ray_order_scratch(n)
    scratch = torch.full((nbytes // 4 + PAD,), FILL, dtype=torch.int32, device="cuda")
    ctx.ray_order(src.data_ptr(), n, order.data_ptr(), scratch.data_ptr(), nbytes, kind=kind,
                  keys_ptr=keys.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    o, k, s = order.cpu().numpy(), keys.cpu().numpy(), scratch.cpu().numpy()
    assert (o[n:] == FILL).all() and (k[n:] == FILL).all(), "entries past the batch were written"
    assert (s[nbytes // 4:] == FILL).all(), "words past the scratch were written"
    return o[:n].view(np.uint32), k[:n].view(np.uint64)


def _same_as_host(R, torch, ctx, sph, rays, kind=0):
    got_o, got_k = _order(R, torch, ctx, rays, kind)
    want_o, want_k = R.ray_order_host(sph, rays, kind=kind, threads=THREADS, keys=True)
    bad = np.flatnonzero(got_k != want_k)
    assert not len(bad), f"{len(bad)} keys differ, first at {bad[0]}: ray {rays[bad[0]]}"
    bad = np.flatnonzero(got_o != want_o)
    assert not len(bad), f"{len(bad)} order words differ of {len(rays)}, first at {bad[0]}"
    return want_o, want_k


def _digits(keys):
    """Per 8-bit digit position of the used bits, whether the keys differ there."""
    import rtg_amd as R
    return [len(np.unique((keys >> np.uint64(8 * p)) & np.uint64(0xFF))) > 1
            for p in range(-(-R.ORDER_KEY_BITS // 8))]


def _one_digit_batch(n):
    """n rays from one origin into a 16 x 16 patch of octahedral bins aligned
    to 16 bins: only the lowest digit position of the key varies."""
    import rtg_amd as R
    rng = np.random.default_rng(21)
    half = 1 << (R.ORDER_DIR_BITS - 1)  # bins per unit of the octahedral map
    u, v = rng.integers(half, half + 16, n), rng.integers(half, half + 16, n)
    px, py = (u + 0.5) / half - 1.0, (v + 0.5) / half - 1.0
    out = np.zeros((n, 6))
    out[:, 3], out[:, 4], out[:, 5] = px, py, 1.0 - px - py
    return out.astype(np.float32)


# ---- 1. device == host ----

def _past_the_key_grid(R, torch, ctx, sph):
    """Two batches of ORDER_KEY_GRID + 2 tiles, the last ragged: the keys
    kernel's workgroups 0 and 1 take a second tile each and add both to one LDS
    histogram.  Random rays (every pass runs), then shuffled primary rays
    tiled to that length (one origin: the skipped-pass plan at that tile
    count)."""
    T, G = R.ORDER_TILE_RAYS, R.ORDER_KEY_GRID
    n = G * T + T + 1
    assert -(-n // T) == G + 2 and n % T == 1 and n < 1 << 32
    rays = raygen.inside(np.random.default_rng(42), sph, n)
    order, keys = _same_as_host(R, torch, ctx, sph, rays)
    check_order(order, keys, n)
    assert sum(_digits(keys)) >= 5
    prim = raygen.primary(64, 48)
    prim = prim[np.random.default_rng(8).permutation(len(prim))]
    prim = np.ascontiguousarray(np.tile(prim, (-(-n // len(prim)), 1))[:n])
    order, keys = _same_as_host(R, torch, ctx, sph, prim)
    check_order(order, keys, n)
    dpos = -(-2 * R.ORDER_DIR_BITS // 8)
    assert _digits(keys) == [True] * dpos + [False] * (len(_digits(keys)) - dpos)


@pytest.mark.parametrize("name", ["reference", 200, "c5"])
def test_device_order_equals_host(R, torch_cuda, name):
    """Ragged waves, one tile -1 / 0 / +1, and one batch with more tiles than
    one scan step handles (the carry between steps)."""
    T, ST = R.ORDER_TILE_RAYS, R.ORDER_SCAN_TILES
    big = min(ST * T + 1, 300000)
    assert big > ST * T  # ST + 1 tiles
    sph = scene(name)
    ctx = R.Context(0)
    ctx.set_scene(sph, np.zeros(0, R.LIGHT_DTYPE))
    try:
        for n in (1, 63, 64, 65, 4097, T - 1, T, T + 1):
            _, keys = _same_as_host(R, torch_cuda, ctx, sph, host_mix(sph, n, 10 + n))
        assert sum(_digits(keys)) >= 5  # the mix runs most digit passes
        # (the large batch: raygen.inside alone, which is vectorised)
        rays = raygen.inside(np.random.default_rng(40), sph, big)
        order, keys = _same_as_host(R, torch_cuda, ctx, sph, rays)
        check_order(order, keys, big)
        segs = raygen.segments(np.random.default_rng(41), sph, 4097)
        _same_as_host(R, torch_cuda, ctx, sph, segs, kind=R.ORDER_SEGMENTS)
        if name == 200:
            _past_the_key_grid(R, torch_cuda, ctx, sph)
    finally:
        ctx.close()


def test_device_order_special_batches(R, torch_cuda):
    """All keys equal (no pass runs: the identity), keys that differ in one
    digit position (the others are skipped), a batch in descending key order."""
    T = R.ORDER_TILE_RAYS
    sph = scene(200)
    ctx = R.Context(0)
    ctx.set_scene(sph, np.zeros(0, R.LIGHT_DTYPE))
    try:
        n = 2 * T + 5
        same = np.repeat(host_mix(sph, 4, 3)[2:3], n, axis=0)
        order, keys = _same_as_host(R, torch_cuda, ctx, sph, same)
        assert (order == np.arange(n)).all() and not any(_digits(keys))
        one = _one_digit_batch(n)
        order, keys = _same_as_host(R, torch_cuda, ctx, sph, one)
        assert _digits(keys) == [True] + [False] * (len(_digits(keys)) - 1)
        assert len(np.unique(keys)) == 256
        assert not (order == np.arange(n)).all()
        # primary rays, shuffled: one origin, only the direction's positions run
        prim = raygen.primary(64, 48)
        prim = prim[np.random.default_rng(7).permutation(len(prim))]
        order, keys = _same_as_host(R, torch_cuda, ctx, sph, prim)
        dpos = -(-2 * R.ORDER_DIR_BITS // 8)
        assert _digits(keys) == [True] * dpos + [False] * (len(_digits(keys)) - dpos)
        mix = host_mix(sph, n, 50)
        o, _ = R.ray_order_host(sph, mix, keys=True)
        desc = mix[o[::-1]]
        order, keys = _same_as_host(R, torch_cuda, ctx, sph, desc)
        assert (np.diff(keys.astype(np.int64)) <= 0).all() and keys[0] > keys[-1]
    finally:
        ctx.close()


# ---- 1b. the key against its restatement ----

@pytest.mark.parametrize("name", list(key_scenes()))
def test_device_keys_equal_the_restatement(R, torch_cuda, name):
    """The ladder-and-edges batch of test_order_host.py (origins and directions
    x 2^k for every k a float32 holds, zero, -0, 3e38, 1e-45, NaN and infinite
    components): the device's keys against the numpy restatement of rtg.h's
    text, not by way of the host form, and its order against the stable sort of
    those keys; rays and segments."""
    sph = key_scenes()[name]
    rays = ladder_batch(sph)
    ctx = R.Context(0)
    ctx.set_scene(sph, np.zeros(0, R.LIGHT_DTYPE))
    try:
        for kind in (R.ORDER_RAYS, R.ORDER_SEGMENTS):
            order, keys = _order(R, torch_cuda, ctx, rays, kind)
            want = restate_keys(sph, rays, kind)
            bad = np.flatnonzero(keys != want)
            assert not len(bad), (kind, len(bad), rays[bad[0]], hex(int(keys[bad[0]])),
                                  hex(int(want[bad[0]])))
            assert (order == np.argsort(want, kind="stable")).all(), kind
    finally:
        ctx.close()


# ---- 2. indexed == plain == host ----

def _run(torch, call, src, n, words, order):
    """One launch into a pre-filled destination of n records of `words` int32
    words (or bytes when words == 0) plus PAD; the tail must stay."""
    if words:
        dst = torch.full(((n + PAD) * words,), FILL, dtype=torch.int32, device="cuda")
    else:
        dst = torch.full((n + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
    call(src.data_ptr(), n, dst.data_ptr(), stream=_stream(torch),
         order=order.data_ptr() if order is not None else 0)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    k = n * (words or 1)
    assert (out[k:] == (FILL if words else 0x5A)).all(), "records past the batch were written"
    return out[:k]


@functools.lru_cache(maxsize=None)
def _batch(name):
    """The scene's rays and segments with the host's plain-loop results,
    computed once and left unchanged."""
    import rtg_amd as R
    sph, lg = scene_with_lights(name)
    rays = mixed_rays(sph, lg, 4097, 700 + len(sph))
    segs = raygen.segments(np.random.default_rng(60), sph, 4097)
    hits = R.intersect_host(sph, rays, walk=0, threads=THREADS)
    vis = R.visible_host(sph, segs, walk=0, threads=THREADS)
    return sph, lg, rays, segs, hits, vis


def _orders(R, torch, ctx, rays, n):
    dev, _ = _order(R, torch, ctx, rays[:n])
    assert (np.sort(dev) == np.arange(n)).all()
    rev = np.arange(n, dtype=np.uint32)[::-1].copy()
    rnd = np.random.default_rng(n).permutation(n).astype(np.uint32)
    return {"device": dev, "reversed": rev, "random": rnd}


@pytest.mark.parametrize("name", [12, 200, "c5"])
def test_indexed_equals_plain_equals_host(R, torch_cuda, name):
    torch = torch_cuda
    sph, lg, rays, segs, hits, vis = _batch(name)
    stacks = (6, 8) if name == "c5" else (6,)
    cols = {S: R.raytrace_host(sph, lg, rays, stack_size=S, walk=0, threads=THREADS)
            for S in stacks}
    assert (hits["id"] >= 0).any() and (np.nan_to_num(cols[6]) > 0).any()
    assert (vis == 0).any() and (vis == 1).any()
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        d_rays, d_segs = torch.from_numpy(rays).cuda(), torch.from_numpy(segs).cuda()
        for n in (65, 4097):
            plain_h = _run(torch, ctx.intersect_device, d_rays, n, 8, None)
            plain_v = _run(torch, ctx.visible_device, d_segs, n, 0, None)
            assert plain_h.tobytes() == hits[:n].tobytes()
            assert plain_v.tobytes() == vis[:n].tobytes()
            seg_order, _ = _order(R, torch, ctx, segs[:n], kind=R.ORDER_SEGMENTS)
            for label, o in _orders(R, torch, ctx, rays, n).items():
                d_o = torch.from_numpy(o.view(np.int32)).cuda()
                got = _run(torch, ctx.intersect_device, d_rays, n, 8, d_o)
                assert got.tobytes() == plain_h.tobytes(), (label, n)
                so = seg_order if label == "device" else o
                d_so = torch.from_numpy(so.view(np.int32)).cuda()
                got = _run(torch, ctx.visible_device, d_segs, n, 0, d_so)
                assert got.tobytes() == plain_v.tobytes(), (label, n)
                for S in stacks:
                    trace = functools.partial(ctx.raytrace_device, stack_size=S)
                    plain_c = _run(torch, trace, d_rays, n, 3, None)
                    assert plain_c.tobytes() == cols[S][:n].tobytes(), (S, n)
                    got = _run(torch, trace, d_rays, n, 3, d_o)
                    assert got.tobytes() == plain_c.tobytes(), (label, S, n)
        if name == 12:  # once with the OpenCL kernel's semantics
            n = 4097
            want = R.raytrace_host(sph, lg, rays, stack_size=6, semantics=1, walk=0,
                                   threads=THREADS)
            assert want.tobytes() != cols[6].tobytes()
            ctx.set_semantics(1)
            d_o = torch.from_numpy(_orders(R, torch, ctx, rays, n)["device"].view(np.int32)).cuda()
            got = _run(torch, ctx.raytrace_device, d_rays, n, 3, d_o)
            assert got.tobytes() == want.tobytes()
    finally:
        ctx.close()


# ---- 3. out-of-range and repeated entries ----

def test_out_of_range_and_repeated_entries(R, torch_cuda):
    """Entries >= n are skipped (never dereferenced), a repeated entry writes
    its record twice, a record no entry names keeps the fill."""
    torch = torch_cuda
    sph, lg, rays, segs, hits, vis = _batch(200)
    n = 65
    order = np.arange(n, dtype=np.uint32)[::-1].copy()
    order[3] = n            # the first index past the batch
    order[10] = 0xFFFFFFFF
    order[64] = n + 1000
    order[20] = order[21]   # a duplicate
    named = np.zeros(n, bool)
    named[order[order < n]] = True
    assert (~named).sum() == 4 and named.sum() == n - 4
    col = R.raytrace_host(sph, lg, rays[:n], stack_size=6, walk=0, threads=THREADS)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        d_rays, d_segs = torch.from_numpy(rays).cuda(), torch.from_numpy(segs).cuda()
        d_o = torch.from_numpy(order.view(np.int32)).cuda()
        got_h = _run(torch, ctx.intersect_device, d_rays, n, 8, d_o).reshape(n, 8)
        got_v = _run(torch, ctx.visible_device, d_segs, n, 0, d_o)
        got_c = _run(torch, ctx.raytrace_device, d_rays, n, 3, d_o).reshape(n, 3)
    finally:
        ctx.close()
    want_h = hits[:n].view(np.int32).reshape(n, 8)
    assert (got_h[named] == want_h[named]).all() and (got_h[~named] == FILL).all()
    assert (got_v[named] == vis[:n][named]).all() and (got_v[~named] == 0x5A).all()
    assert (got_c[named] == col.view(np.int32)[named]).all() and (got_c[~named] == FILL).all()


# ---- 4. no interference ----

def test_no_interference_with_renders(R, golden, torch_cuda):
    """render, ray_order, raytrace(order), render, intersect on one context and
    one stream: both frames the golden bits, both batches the host's."""
    torch = torch_cuda
    c = golden["configs"]["c3"]
    sph, lg = load_scene("c3", c["spheres"], c["lights"])
    W, H, S = c["small"]["W"], c["small"]["H"], c["stack_size"]
    want = load_f32(os.path.join(GOLDEN, "c3.small.f32"), (H, W, 3))
    rays = mixed_rays(sph, lg, 3000, 5)
    n = len(rays)
    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    try:
        stream = _stream(torch)
        fb1 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        fb2 = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        dr = torch.from_numpy(rays).cuda()
        col = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        hits = torch.zeros((n * 8,), dtype=torch.int32, device="cuda")
        order = torch.zeros((n,), dtype=torch.int32, device="cuda")
        nbytes = R.ray_order_scratch(n)
        scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
        ctx.render_device(W, H, fb1.data_ptr(), stack_size=S, stream=stream)
        ctx.ray_order(dr.data_ptr(), n, order.data_ptr(), scratch.data_ptr(), nbytes,
                      stream=stream)
        ctx.raytrace_device(dr.data_ptr(), n, col.data_ptr(), stack_size=S, stream=stream,
                            order=order.data_ptr())
        ctx.render_device(W, H, fb2.data_ptr(), stack_size=S, stream=stream)
        ctx.intersect_device(dr.data_ptr(), n, hits.data_ptr(), stream=stream,
                             order=order.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.close()
    for fb in (fb1.cpu().numpy(), fb2.cpu().numpy()):
        assert bits_equal(fb, want), first_mismatch(fb, want)
    assert (order.cpu().numpy().view(np.uint32) == R.ray_order_host(sph, rays)).all()
    w = R.raytrace_host(sph, lg, rays, stack_size=S, threads=THREADS)
    assert col.cpu().numpy().tobytes() == w.tobytes()
    assert hits.cpu().numpy().tobytes() == R.intersect_host(sph, rays, threads=THREADS).tobytes()


# ---- 5. the driver ----

def test_host_driver_sort_rays(R, tmp_path):
    sph, lg = R.reference_scene()
    rays = np.concatenate([raygen.primary(40, 30), host_mix(sph, 1000, 9)])
    rays = rays[np.random.default_rng(4).permutation(len(rays))]
    fin = str(tmp_path / "rays.bin")
    rays.tofile(fin)
    base = [os.path.join(PKG, "rtg_main"), "--scene",
            os.path.join(ROOT, "scenes", "reference.scene"), "--width", "32", "--height", "24",
            "--out", str(tmp_path / "o.ppm"), "--rays", fin]
    files = {}
    for tag, extra in (("plain", []), ("sorted", ["--sort-rays"])):
        fh, fr = str(tmp_path / f"hits.{tag}"), str(tmp_path / f"radiance.{tag}")
        r = subprocess.run(base + ["--hits", fh, "--radiance", fr] + extra, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("Ordered" in r.stdout) == bool(extra)
        files[tag] = (open(fh, "rb").read(), open(fr, "rb").read())
    assert files["plain"][0] == files["sorted"][0]
    assert files["plain"][1] == files["sorted"][1]
    assert files["plain"][0] == R.intersect_host(sph, rays, threads=THREADS).tobytes()
    assert files["plain"][1] == R.raytrace_host(sph, lg, rays, threads=THREADS).tobytes()
    r = subprocess.run(base[:-2] + ["--sort-rays"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "needs --rays" in r.stdout  # no GPU call


# ---- 6. entry-point errors ----

def test_entry_point_errors(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    ctx = R.Context(0)
    try:
        n = 64
        rays = torch.from_numpy(raygen.primary(8, 8)).cuda()
        order = torch.zeros((n,), dtype=torch.int32, device="cuda")
        nbytes = R.ray_order_scratch(n)
        scratch = torch.zeros((nbytes // 4 + 4,), dtype=torch.int32, device="cuda")
        hits = torch.zeros((n * 8,), dtype=torch.int32, device="cuda")
        vis = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        col = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        r, o, s = rays.data_ptr(), order.data_ptr(), scratch.data_ptr()
        with pytest.raises(R.RtgError, match="scene"):  # no scene yet
            ctx.ray_order(r, n, o, s, nbytes)
        ctx.set_scene(sph, lg)
        for args, kw, msg in (((0, n, o, s, nbytes), {}, "null ray"),
                              ((r, n, 0, s, nbytes), {}, "null order"),
                              ((r, n, o, 0, nbytes), {}, "null scratch"),
                              ((r, n, o, s, nbytes - 1), {}, "scratch of"),
                              ((r, n, o, s, 0), {}, "scratch of"),
                              ((r, n, o, s + 4, nbytes), {}, "aligned"),
                              ((r, 1 << 32, o, s, nbytes), {}, "2\\^32"),
                              ((r, n, o, s, nbytes), {"kind": 2}, "kind 2")):
            with pytest.raises(R.RtgError, match=msg):
                ctx.ray_order(*args, **kw)
        L, vp = R.lib(), __import__("ctypes").c_void_p
        for rc, msg in ((L.rtg_intersect_indexed_device(ctx._h, vp(r), None, n,
                                                        vp(hits.data_ptr()), None), "null order"),
                        (L.rtg_visible_indexed_device(ctx._h, vp(r), None, n,
                                                      vp(vis.data_ptr()), None), "null order"),
                        (L.rtg_raytrace_indexed_device(ctx._h, vp(r), None, n, 6,
                                                       vp(col.data_ptr()), None), "null order")):
            with pytest.raises(R.RtgError, match=msg):
                R._check(rc, "indexed")
        # the un-indexed calls' checks hold for the indexed forms
        with pytest.raises(R.RtgError, match="null ray"):
            ctx.intersect_device(0, n, hits.data_ptr(), order=o)
        with pytest.raises(R.RtgError, match="aligned"):
            ctx.intersect_device(r, n, hits.data_ptr() + 4, order=o)
        with pytest.raises(R.RtgError, match="stackSize 17"):
            ctx.raytrace_device(r, n, col.data_ptr(), stack_size=17, order=o)
        with pytest.raises(R.RtgError, match="too large"):
            ctx.visible_device(r, 1 << 37, vis.data_ptr(), order=o)
        # n == 0: RTG_OK, nothing launched
        ctx.ray_order(r, 0, o, s, nbytes)
        ctx.intersect_device(r, 0, hits.data_ptr(), order=o)
        ctx.visible_device(r, 0, vis.data_ptr(), order=o)
        ctx.raytrace_device(r, 0, col.data_ptr(), order=o)
        torch.cuda.synchronize()
        assert int(order.abs().sum()) == 0 and int(scratch.abs().sum()) == 0
        assert int(hits.abs().sum()) == 0 and int(vis.sum()) == 0 and int(col.abs().sum()) == 0
    finally:
        ctx.close()
