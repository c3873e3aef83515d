"""GPU tests of temporal accumulation by reprojection (rtg_accumulate*,
rtg_camera_project*; include/rtg.h) on an MI355X, against the host loops' words
test_accumulate_host.py pins on the CPU (accumgen.want), word for word.

Every output is pre-filled and PAD words longer than the call needs; the tail
must stay.

  1. accumulate_device == accumulate_host (outAcc, outLen, outM2) on every frame,
     previous pose, signal and parameter set of accumgen;
  2. camera_project_device == camera_project_host on the records' points, the
     planted NaN point and the eye itself among them;
  3. the one-shot forms;
  4. a launch on a stream of its own between two renders of the context;
  5. the device chain camera_rays -> intersect -> ao -> accumulate over four
     poses and seeds, then the filter, against the host chain;
  6. rtg_main --ao-history and --gather-history, with and without the filter;
  7. the device entry point's argument checks.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import accumgen as A
import aogen
import filtergen as G
from accumgen import FRAMES, FULL, SCENES, SIGNALS
from conftest import PKG, ROOT
from test_gpu_order import PAD, _stream
from test_raytrace_host import THREADS, scene_with_lights

pytestmark = pytest.mark.gpu

F = np.float32
FILL32, FILL16 = 0x5A5A5A5A, 0x5A5A


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
def ctx(R):
    c = R.Context(0)  # no scene: neither call needs one
    yield c
    c.close()


def _dev(torch, a):
    """A host array on the device as bytes, 16-byte aligned."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _dev_prev(torch, pv):
    """accumulate_host's `prev` with its arrays on the device: (what
    accumulate_device takes, the tensors to keep alive)."""
    if pv is None:
        return None, ()
    keep = tuple(None if a is None else _dev(torch, a) for a in pv[1:])
    return (pv[0],) + tuple(0 if t is None else t.data_ptr() for t in keep), keep


def _accumulate(torch, R, ctx, d_hits, W, H, p, d_src, prev, m2, stream=None):
    """Context.accumulate_device into pre-filled outputs, PAD words longer each:
    (acc words, len, m2 words or None)."""
    words = W * H * (3 if int(p["kind"][0]) == R.FILTER_RGB else 1)
    acc = torch.full((words + PAD,), FILL32, dtype=torch.int32, device="cuda")
    sq = torch.full((words + PAD,), FILL32, dtype=torch.int32, device="cuda")
    ln = torch.full((W * H + PAD,), FILL16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    ctx.accumulate_device(d_hits.data_ptr(), W, H, p, d_src.data_ptr(), acc.data_ptr(),
                          ln.data_ptr(), prev, zoom=A.ZOOM, out_m2_ptr=sq.data_ptr() if m2 else 0,
                          stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    acc, sq = (t.cpu().numpy().view(np.uint32) for t in (acc, sq))
    ln = ln.cpu().numpy().view(np.uint16)
    assert (acc[words:] == FILL32).all() and (ln[W * H:] == FILL16).all(), \
        "words past the frame were written"
    assert (sq[words if m2 else 0:] == FILL32).all(), "outM2 was written past the frame, or unasked"
    return acc[:words], ln[:W * H], sq[:words] if m2 else None


def _first_bad(got, want):
    for what, g, w in zip(("acc", "len", "m2"), got, want):
        if g is None:
            continue
        bad = np.flatnonzero(g != w)
        if len(bad):
            return f"{what}: {len(bad)} differ, first at {bad[0]}: {g[bad[0]]:#x} vs {w[bad[0]]:#x}"
    return None


def _check_cases(torch, R, ctx, name, kind, frames):
    for W, H in frames:
        d_hits = _dev(torch, G.guides(name, W, H))
        d_src = _dev(torch, G.signal(name, W, H, kind))
        on_device = {}
        for pk, st in A.cases():
            key = (pk, st[3], st[4], st[5])  # what the previous state depends on
            if key not in on_device:
                on_device[key] = _dev_prev(torch, A.prev(name, W, H, pk, kind, st))
            got = _accumulate(torch, R, ctx, d_hits, W, H, A.params(R, name, kind, st), d_src,
                              on_device[key][0], st[4])
            bad = _first_bad(got, A.want(name, W, H, kind, pk, st))
            assert bad is None, (W, H, pk, st, bad)


# ---- 1. every frame, previous pose, signal and parameter set ----

@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_host(R, torch_cuda, ctx, name, kind):
    _check_cases(torch_cuda, R, ctx, name, kind, FRAMES)


# ---- 2. the projection ----

@pytest.mark.parametrize("name", SCENES)
def test_project_device_equals_host(R, torch_cuda, ctx, name):
    torch = torch_cuda
    for (W, H), sizes in ((FULL, (None,)), ((33, 17), (1, 63, 64, 65))):
        pts = G.guides(name, W, H)["point"].astype(F).copy()
        pts[0] = A.pose_args(name, "same")[0]  # the eye itself: d = 0
        if (W, H) == FULL:
            assert np.isnan(pts).any()
        for n in sizes:
            p = pts[:n]
            d_pts = _dev(torch, p)
            for pk in A.PREV_KINDS:
                cam = A.pose(name, pk)
                out = torch.full((3 * len(p) + PAD,), FILL32, dtype=torch.int32, device="cuda")
                ctx.camera_project_device(cam, W, H, d_pts.data_ptr(), len(p), out.data_ptr(),
                                          zoom=A.ZOOM, stream=_stream(torch))
                torch.cuda.synchronize()
                got = out.cpu().numpy().view(np.uint32)
                want = R.camera_project_host(cam, W, H, p, zoom=A.ZOOM).view(np.uint32).reshape(-1)
                assert (got[3 * len(p):] == FILL32).all(), "words past the batch were written"
                assert got[:3 * len(p)].tobytes() == want.tobytes(), (W, H, n, pk)
    # no points: nothing is launched, null buffers are legal
    ctx.camera_project_device(A.pose(name, "pan"), 8, 8, 0, 0, 0)


# ---- 3. the one-shot forms ----

def test_one_shot(R, torch_cuda):
    for name, (W, H), kind, pk, st in (("reference", FULL, "count", "pan", A.SETS[0]),
                                       ("c5", FULL, "rgb", "roll", A.SETS[1]),
                                       (12, (33, 17), "gray", "dolly", A.SETS[6]),
                                       (12, (1, 1), "rgb", "same", A.SETS[2]),
                                       ("c5", (8, 8), "rgb", "same", A.SETS[13]),
                                       ("c5", (8, 8), "rgb", "same", A.SETS[14])):
        got = R.accumulate(G.guides(name, W, H), W, H, A.params(R, name, kind, st),
                           G.signal(name, W, H, kind), A.prev(name, W, H, pk, kind, st),
                           zoom=A.ZOOM, m2=st[4])
        assert got[0].shape == ((H, W, 3) if kind == "rgb" else (H, W)) and got[1].shape == (H, W)
        got = (got[0].view(np.uint32).reshape(-1), got[1].reshape(-1),
               got[2].view(np.uint32).reshape(-1) if st[4] else None)
        bad = _first_bad(got, A.want(name, W, H, kind, pk, st))
        assert bad is None, (name, W, H, kind, pk, st, bad)
    pts = G.guides("c5", *FULL)["point"]
    cam = A.pose("c5", "pan")
    got = R.camera_project(cam, *FULL, pts, zoom=A.ZOOM)
    want = R.camera_project_host(cam, *FULL, pts, zoom=A.ZOOM)
    assert got.shape == (len(pts), 3) and got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()


# ---- 4. a stream of its own, between two renders ----

def test_own_stream_between_renders(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    W, H = FULL
    name, kind, pk, st = "reference", "rgb", "pan", A.SETS[0]
    d_hits, d_src = _dev(torch, G.guides(name, W, H)), _dev(torch, G.signal(name, W, H, kind))
    prev, keep = _dev_prev(torch, A.prev(name, W, H, pk, kind, st))
    c = R.Context(0)
    try:
        c.set_scene(sph, lg)
        fb = [torch.zeros((48 * 36 * 3,), dtype=torch.float32, device="cuda") for _ in range(2)]
        own = torch.cuda.Stream()
        c.render_device(48, 36, fb[0].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        got = _accumulate(torch, R, c, d_hits, W, H, A.params(R, name, kind, st), d_src, prev,
                          st[4], stream=own.cuda_stream)
        c.render_device(48, 36, fb[1].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        torch.cuda.synchronize()
        assert _first_bad(got, A.want(name, W, H, kind, pk, st)) is None
        a, b = fb[0].cpu().numpy(), fb[1].cpu().numpy()
        assert (a != 0).any() and G.canon(a).tobytes() == G.canon(b).tobytes()
        want = R.render(sph, lg, 48, 36, alias_factor=2.0)
        assert G.canon(a).tobytes() == G.canon(want).tobytes()
    finally:
        c.close()


# ---- 5. the device chain ----

def _path(name, frames):
    eye, target = (np.array(v, np.float64) for v in G.POSES[name])
    return [(tuple(eye + k * np.array((0.3, 0.1, 0.0))), tuple(target + k * np.array((0.3, 0.1, 0.0))))
            for k in range(frames)]


def test_device_chain_equals_host_chain(R, torch_cuda):
    torch = torch_cuda
    W, H, K = 67, 35, 7
    name = "c5"
    n = W * H
    sph = aogen.scene(name)
    table = aogen.dirs(8)
    flags = R.ACCUM_SAME_ID | R.ACCUM_NORMAL | R.ACCUM_PLANE
    ap_ = R.accumulate_params(R.FILTER_COUNT, flags, G.plane_scale(name, None), 3, 3)
    fp = R.filter_params(3, R.FILTER_GRAY, flags, G.plane_scale(name, None), 3)
    cams = [R.camera_look_at(*p) for p in _path(name, 4)]
    aos = [R.ao_params(K, aogen.radius(name), aogen.BIAS, (aogen.SEED + k) & 0xFFFFFFFF, R.AO_JITTER)
           for k in range(4)]
    prev = None
    for cam, ap in zip(cams, aos):  # the host chain
        h = R.intersect_host(sph, R.camera_rays_host(cam, W, H, alias_factor=1.0), walk=0,
                             threads=THREADS)
        counts = R.ao_host(sph, h, table, ap, walk=0, threads=THREADS)
        acc, ln = R.accumulate_host(h, W, H, ap_, counts, prev, zoom=A.ZOOM, threads=THREADS)
        prev = (cam, h, acc, ln)
    want_acc, want_len = prev[2].view(np.uint32).reshape(-1), prev[3].reshape(-1)
    want = R.filter_host(prev[1], W, H, fp, prev[2], threads=THREADS).view(np.uint32).reshape(-1)
    assert want_len.max() == 3 and (want_len == 1).any() and (want != want_acc).any()
    c = R.Context(0)
    try:
        c.set_scene(sph, scene_with_lights(name)[1])
        d_rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        d_counts = torch.empty((n,), dtype=torch.int16, device="cuda")
        d_dirs = _dev(torch, table)
        d_hits = [torch.empty((n, 8), dtype=torch.int32, device="cuda") for _ in range(2)]
        d_acc = [torch.full((n + PAD,), FILL32, dtype=torch.int32, device="cuda") for _ in range(2)]
        d_len = [torch.full((n + PAD,), FILL16, dtype=torch.int16, device="cuda") for _ in range(2)]
        s = _stream(torch)
        for k, (cam, ap) in enumerate(zip(cams, aos)):
            a, b = k & 1, (k & 1) ^ 1
            c.camera_rays(cam, W, H, d_rays.data_ptr(), alias_factor=1.0, stream=s)
            c.intersect_device(d_rays.data_ptr(), n, d_hits[a].data_ptr(), stream=s)
            c.ao_device(d_hits[a].data_ptr(), n, ap, d_dirs.data_ptr(), 8, d_counts.data_ptr(), stream=s)
            pv = None if k == 0 else (cams[k - 1], d_hits[b].data_ptr(), d_acc[b].data_ptr(),
                                      d_len[b].data_ptr())
            c.accumulate_device(d_hits[a].data_ptr(), W, H, ap_, d_counts.data_ptr(),
                                d_acc[a].data_ptr(), d_len[a].data_ptr(), pv, zoom=A.ZOOM, stream=s)
        nbytes = R.filter_scratch(W, H, fp)
        dst = torch.full((n + PAD,), FILL32, dtype=torch.int32, device="cuda")
        scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
        c.filter_device(d_hits[1].data_ptr(), W, H, fp, d_acc[1].data_ptr(), dst.data_ptr(),
                        scratch.data_ptr(), nbytes, stream=s)
        torch.cuda.synchronize()
        acc, ln = d_acc[1].cpu().numpy().view(np.uint32), d_len[1].cpu().numpy().view(np.uint16)
        out = dst.cpu().numpy().view(np.uint32)
        assert (acc[n:] == FILL32).all() and (ln[n:] == FILL16).all() and (out[n:] == FILL32).all()
        assert _first_bad((acc[:n], ln[:n], out[:n]), (want_acc, want_len, want)) is None
    finally:
        c.close()


# ---- 6. the driver ----

def _pgm_of(v, K, W, H):
    x = F(255) * v.reshape(-1).astype(F) / F(K)
    x = np.where(x > 0, np.where(x < 255, x, F(255)), F(0))
    return b"P5\n%d %d\n255\n" % (W, H) + x.astype(np.uint8).tobytes()


def test_host_driver_history_options(R, torch_cuda, tmp_path):
    scene_file = os.path.join(ROOT, "scenes", "reference.scene")
    sph, lg = R.load_scene_file(scene_file)
    W, H, K = 48, 36, 16
    base = [os.path.join(PKG, "rtg_main"), "--scene", scene_file, "--width", str(W), "--height",
            str(H), "--out", str(tmp_path / "frame.ppm")]
    path = [((3.3, 2.1, -1), (0.2, 0, -10)), ((3.2, 2.0, -1), (0.1, 0, -10), (0.05, 1, 0)),
            ((3.1, 2.0, -1), (0, 0, -10))]
    poses_file = str(tmp_path / "path.txt")
    with open(poses_file, "w") as f:
        f.write("3.3,2.1,-1,0.2,0,-10\n\n3.2,2.0,-1,0.1,0,-10,0.05,1,0\n3.1,2.0,-1,0,0,-10\n")
    pose = ["--camera", "3,2,-1,0,0,-10"]
    cams = [R.camera_look_at(*p) for p in path] + [R.camera_look_at((3, 2, -1), (0, 0, -10))]
    hits = [R.intersect_host(sph, R.camera_rays_host(c, W, H, alias_factor=1.0), walk=0,
                             threads=THREADS) for c in cams]
    table = R.ao_directions(K)
    flags = R.ACCUM_SAME_ID | R.ACCUM_NORMAL | R.ACCUM_PLANE

    def run(extra):
        r = subprocess.run(base + pose + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr

    def chain(signal, p):
        prev = None
        for k, (c, h) in enumerate(zip(cams, hits)):
            acc, ln = R.accumulate_host(h, W, H, p, signal(k, h), prev, zoom=A.ZOOM, threads=THREADS)
            prev = (c, h, acc, ln)
        assert prev[3].max() == min(4, int(p["maxHistory"][0]))
        return prev[2]

    # --ao-history, with and without --ao-filter, and a maxHistory of its own
    ao = lambda k, h: R.ao_host(sph, h, table, R.ao_params(K, 12.5, 1e-3, 5 + k, R.AO_JITTER),  # noqa: E731
                                walk=0, threads=THREADS)
    out = str(tmp_path / "ao.pgm")
    seen = set()
    for spec, mh in ((poses_file, 65535), (poses_file + ",2", 2)):
        v = chain(ao, R.accumulate_params(R.FILTER_COUNT, flags, 1.0, 3, mh))
        run(["--ao", "16,12.5,0.001,5", "--ao-out", out, "--ao-history", spec])
        assert open(out, "rb").read() == _pgm_of(v, K, W, H), spec
        seen.add(_pgm_of(v, K, W, H))
        run(["--ao", "16,12.5,0.001,5", "--ao-out", out, "--ao-history", spec, "--ao-filter", "3,0.5"])
        sm = R.filter_host(hits[-1], W, H, R.filter_params(3, R.FILTER_GRAY, flags, 0.5, 3), v)
        assert open(out, "rb").read() == _pgm_of(sm, K, W, H), spec
        seen.add(_pgm_of(sm, K, W, H))
    run(["--ao", "16,12.5,0.001,8", "--ao-out", out])  # the last frame alone: seed 5 + 3
    seen.add(open(out, "rb").read())
    assert len(seen) == 5  # the history, its cap and the filter each change the picture
    # --gather-history, with --gather-skip and the filter
    wts = np.full(K, F(1) / F(K), F)

    def light(k, h):
        g = R.gather_host(sph, lg, h, table, wts, R.gather_params(K, 1e-3, 9 + k, R.GATHER_JITTER |
                                                                  R.GATHER_SKIP_NONFINITE),
                          stack_size=6, walk=0, threads=THREADS)
        return np.asarray(g if not isinstance(g, tuple) else g[0], F).reshape(W * H, 3)

    v = chain(light, R.accumulate_params(R.FILTER_RGB, flags | R.ACCUM_SKIP_NONFINITE, 1.0, 3, 65535))
    out = str(tmp_path / "g.ppm")
    run(["--gather", "16,0.001,9", "--gather-skip", "--gather-out", out, "--gather-history", poses_file])
    plain = open(out, "rb").read()
    assert plain == R.ppm_file_bytes(v)
    run(["--gather", "16,0.001,9", "--gather-skip", "--gather-out", out, "--gather-history",
         poses_file, "--gather-filter", "2"])
    sm = R.filter_host(hits[-1], W, H, R.filter_params(2, R.FILTER_RGB, flags | R.FILTER_SKIP_NONFINITE,
                                                       1.0, 3), v)
    assert open(out, "rb").read() == R.ppm_file_bytes(sm) != plain
    for bad in (["--ao-history", poses_file], ["--gather-history", poses_file],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-history", poses_file + ",0"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-history", poses_file + ",65536"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("Invalid history" in r.stdout or "needs --" in r.stdout), r.stdout
    r = subprocess.run(base[:1] + ["--help"], capture_output=True, text=True, timeout=120)
    assert "--ao-history" in r.stdout and "--gather-history" in r.stdout


# ---- 7. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda, ctx):
    torch = torch_cuda
    W, H = 33, 17
    n = W * H
    # one arena, 32 n bytes per buffer: a range laid over another buffer, or over
    # a buffer's end, meets that buffer and no other
    slot = 32 * n
    arena = torch.zeros((9 * slot,), dtype=torch.uint8, device="cuda")
    base = arena.data_ptr()
    hp, php, sp, pa, pl, p2, oa, ol, o2 = (base + k * slot for k in range(9))

    def part(k, nbytes):
        return arena[k * slot:k * slot + nbytes]

    part(0, 32 * n).copy_(_dev(torch, G.guides("reference", W, H)))
    part(1, 32 * n).copy_(_dev(torch, A.prev_hits("reference", W, H, "pan")))
    part(2, 4 * n).copy_(_dev(torch, G.signal("reference", W, H, "gray")))
    acc, ln, m2 = part(6, slot), part(7, slot), part(8, slot)
    cam = A.pose("reference", "pan")
    ok = R.accumulate_params(R.FILTER_GRAY, A.ALL, 1.0, 3, 3)
    assert hp % 16 == 0 and php % 16 == 0
    par = R.accumulate_params

    def call(hits=hp, w=W, h=H, p=ok, src=sp, prev=(cam, php, pa, pl, p2), out=(oa, ol, o2)):
        ctx.accumulate_device(hits, w, h, p, src, out[0], out[1], prev, zoom=A.ZOOM, out_m2_ptr=out[2])

    for kw, msg in ((dict(hits=0), "accumulate: null hit buffer"),
                    (dict(src=0), "accumulate: null source"),
                    (dict(out=(0, ol, o2)), "accumulate: null outAcc"),
                    (dict(out=(oa, 0, o2)), "accumulate: null outLen"),
                    (dict(prev=(cam, 0, pa, pl, p2)), "all null or all non-null"),
                    (dict(prev=(cam, php, 0, pl, p2)), "all null or all non-null"),
                    (dict(prev=(cam, php, pa, 0, p2)), "all null or all non-null"),
                    (dict(prev=(None, php, pa, pl, p2)), "accumulate: null previous pose"),
                    (dict(prev=(cam, php, pa, pl, 0)), "accumulate: outM2 without prevM2"),
                    (dict(out=(oa, ol, 0)), "accumulate: prevM2 without outM2"),
                    (dict(w=0), "accumulate: empty frame"),
                    (dict(h=0), "accumulate: empty frame"),
                    (dict(w=(1 << 24) + 1), "at most 2\\^24"),
                    (dict(h=(1 << 24) + 1), "at most 2\\^24"),
                    (dict(p=par(1, 0, 0.0, 9, 3)), "normalLog2 9"),
                    (dict(p=par(3, 0, 0.0, 0, 3)), "kind 3"),
                    (dict(p=par(1, 16, 0.0, 0, 3)), "unknown flags 0x10"),
                    (dict(p=par(1, 0, 0.0, 0, 0)), "maxHistory 0"),
                    (dict(p=par(1, 0, 0.0, 0, 65536)), "maxHistory 65536"),
                    (dict(hits=hp + 4), "accumulate: hit buffer not 16-byte aligned"),
                    (dict(prev=(cam, php + 8, pa, pl, p2)), "previous hit buffer not 16-byte aligned"),
                    (dict(out=(sp, ol, o2)), "outAcc overlaps src"),
                    (dict(out=(hp + 32 * n - 4, ol, o2)), "outAcc overlaps hits"),
                    (dict(out=(php, ol, o2)), "outAcc overlaps prevHits"),
                    (dict(out=(pa, ol, o2)), "outAcc overlaps prevAcc"),
                    (dict(out=(pa + 4 * n - 4, ol, o2)), "outAcc overlaps prevAcc"),
                    (dict(out=(pl, ol, o2)), "outAcc overlaps prevLen"),
                    (dict(out=(p2, ol, o2)), "outAcc overlaps prevM2"),
                    (dict(out=(oa, oa + 2, o2)), "outAcc overlaps outLen"),
                    (dict(out=(oa, ol, oa)), "outAcc overlaps outM2"),
                    (dict(out=(oa, sp, o2)), "outLen overlaps src"),
                    (dict(out=(oa, hp, o2)), "outLen overlaps hits"),
                    (dict(out=(oa, php, o2)), "outLen overlaps prevHits"),
                    (dict(out=(oa, pa, o2)), "outLen overlaps prevAcc"),
                    (dict(out=(oa, pl, o2)), "outLen overlaps prevLen"),
                    (dict(out=(oa, p2, o2)), "outLen overlaps prevM2"),
                    (dict(out=(oa, o2 + 4 * n - 2, o2)), "outLen overlaps outM2"),
                    (dict(out=(oa, ol, sp)), "outM2 overlaps src"),
                    (dict(out=(oa, ol, hp)), "outM2 overlaps hits"),
                    (dict(out=(oa, ol, php)), "outM2 overlaps prevHits"),
                    (dict(out=(oa, ol, pa)), "outM2 overlaps prevAcc"),
                    (dict(out=(oa, ol, pl)), "outM2 overlaps prevLen"),
                    (dict(out=(oa, ol, p2)), "outM2 overlaps prevM2")):
        with pytest.raises(R.RtgError, match=msg):
            call(**kw)
    L = R.lib()
    cam1 = np.ascontiguousarray(cam, R.CAMERA_DTYPE).reshape(1)
    assert L.rtg_accumulate_device(ctx._h, hp, W, H, None, sp, R._ptr(cam1), A.ZOOM, php, pa, pl, p2,
                                   oa, ol, o2, None) == -1
    assert b"accumulate: null params" in L.rtg_last_error()
    assert L.rtg_accumulate_device(None, hp, W, H, R._ptr(ok), sp, R._ptr(cam1), A.ZOOM, php, pa, pl,
                                   p2, oa, ol, o2, None) == -1
    assert b"accumulate: no context" in L.rtg_last_error()
    # a frame of 2^24 x 2^24 pixels has 2^43 workgroups; the address comparison takes its
    # ranges as numbers and nothing is dereferenced (the buffers lie far apart as numbers)
    big = 1 << 24
    with pytest.raises(R.RtgError, match="frame too large"):
        ctx.accumulate_device(16, big, big, par(R.FILTER_COUNT), 1 << 56, 1 << 58, 1 << 60)
    with pytest.raises(R.RtgError, match="camera_project: batch too large"):
        ctx.camera_project_device(cam, W, H, hp, 1 << 40, oa)
    assert L.rtg_camera_project_device(ctx._h, None, W, H, A.ZOOM, hp, 4, oa, None) == -1
    assert b"camera_project: null camera" in L.rtg_last_error()
    assert L.rtg_camera_project_device(None, R._ptr(cam1), W, H, A.ZOOM, hp, 4, oa, None) == -1
    assert b"camera_project: no context" in L.rtg_last_error()
    for a, msg in (((cam, 0, H, hp, 4, oa), "camera_project: empty frame"),
                   ((cam, W, big + 1, hp, 4, oa), "at most 2\\^24"),
                   ((cam, W, H, 0, 4, oa), "camera_project: null points"),
                   ((cam, W, H, hp, 4, 0), "camera_project: null destination")):
        with pytest.raises(R.RtgError, match=msg):
            ctx.camera_project_device(*a)
    torch.cuda.synchronize()
    for t in (acc, m2, ln):
        assert int(t.count_nonzero()) == 0  # nothing launched
    # ranges that touch do not overlap; a reset frame takes outM2 alone and no pose
    ctx.accumulate_device(hp, W, H, ok, sp, oa, ol, None, zoom=A.ZOOM, out_m2_ptr=oa + 4 * n)
    torch.cuda.synchronize()
    want = R.accumulate_host(G.guides("reference", W, H), W, H, ok, G.signal("reference", W, H, "gray"),
                             None, m2=True)
    assert (ln.cpu().numpy().view(np.uint16)[:n] == want[1].reshape(-1)).all() and want[1].any()
    assert int(ln[2 * n:].count_nonzero()) == 0 and int(acc[8 * n:].count_nonzero()) == 0
    assert int(m2.count_nonzero()) == 0
    got = acc.cpu().numpy().view(np.uint32)[:2 * n]
    assert got[:n].tobytes() == want[0].view(np.uint32).tobytes()
    assert got[n:].tobytes() == want[2].view(np.uint32).tobytes()
