"""GPU tests of the variance estimate and the variance-guided a-trous passes
(rtg_variance*, rtg_svgf*, include/rtg.h) on an MI355X, against the host loops'
words test_svgf_host.py pins on the CPU (svgfgen.want_*), word for word.

Every destination and scratch is pre-filled and PAD words longer than the
call needs; the tail must stay.

  1. both device calls == the host forms on every frame, signal and parameter
     set of svgfgen (passes 5 and 8 reach the steps the direct form takes);
  2. both pass-kernel forms, forced by RTG_SVGF_FORM, on the 67 x 35 frames;
  3. the four len fields: both sides of the variance kernel's vote;
  4. the one-shot forms;
  5. a launch on a stream of its own between two renders of the context;
  6. the device chain camera_rays -> intersect -> ao -> accumulate (M2) ->
     variance -> svgf over four frames, against the host chain;
  7. rtg_main --ao-variance and --gather-variance, and the same command lines
     without them;
  8. the device entry points' argument checks.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import aogen
import filtergen as G
import svgfgen as S
from conftest import PKG, ROOT
from filtergen import ALL, FRAMES, FULL, SCENES
from svgfgen import SIGNALS, SVGF_SETS
from test_gpu_order import PAD, _stream
from test_raytrace_host import THREADS, scene_with_lights

pytestmark = pytest.mark.gpu

F = np.float32
FILL32 = 0x5A5A5A5A
FILL16 = 0x5A5A


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


def _filled(torch, words):
    return torch.full((words + PAD,), FILL32, dtype=torch.int32, device="cuda")


def _tail_kept(t, words, what):
    out = t.cpu().numpy().view(np.uint32)
    assert (out[words:] == FILL32).all(), f"words past the {what} were written"
    return out[:words]


def _svgf(torch, R, ctx, d_hits, W, H, p, d_src, d_var, stream=None):
    """Context.svgf_device into pre-filled destinations and scratch, PAD words
    longer each: the result's (value words, variance words)."""
    n = W * H
    words = n * (3 if int(p["kind"][0]) == R.FILTER_RGB else 1)
    nbytes = R.svgf_scratch(W, H, p)
    assert nbytes % 16 == 0 and (nbytes >= (words + n) * 4 if int(p["passes"][0]) > 1 else nbytes == 0)
    dst, dvar, scratch = _filled(torch, words), _filled(torch, n), _filled(torch, nbytes // 4)
    torch.cuda.synchronize()  # the fills, before a launch on another stream
    ctx.svgf_device(d_hits.data_ptr(), W, H, p, d_src.data_ptr(), d_var.data_ptr(), dst.data_ptr(),
                    dvar.data_ptr(), scratch.data_ptr() if nbytes else 0, nbytes,
                    stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    _tail_kept(scratch, nbytes // 4, "scratch")
    return _tail_kept(dst, words, "frame"), _tail_kept(dvar, n, "variance")


def _variance(torch, R, ctx, d_hits, W, H, p, d_acc, d_m2, d_len, stream=None):
    """Context.variance_device into a pre-filled destination: its words."""
    out = _filled(torch, W * H)
    torch.cuda.synchronize()
    ctx.variance_device(d_hits.data_ptr(), W, H, p, d_acc.data_ptr(), d_m2.data_ptr(),
                        d_len.data_ptr(), out.data_ptr(),
                        stream=_stream(torch) if stream is None else stream)
    torch.cuda.synchronize()
    return _tail_kept(out, W * H, "frame")


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else \
        f"{len(bad)} differ, first at {bad[0]}: {got[bad[0]]:#x} vs {want[bad[0]]:#x}"


def _check_svgf(torch, R, ctx, name, kind, W, H, sets):
    d_hits = _dev(torch, G.guides(name, W, H))
    d_src, d_var = _dev(torch, G.signal(name, W, H, kind)), _dev(torch, S.var_field(name, W, H))
    for st in sets:
        got = _svgf(torch, R, ctx, d_hits, W, H, S.svgf_params(R, name, kind, st), d_src, d_var)
        want = S.want_svgf(name, W, H, kind, st)
        assert got[0].tobytes() == want[0].tobytes(), (name, kind, W, H, st, _first_bad(got[0], want[0]))
        assert got[1].tobytes() == want[1].tobytes(), (name, kind, W, H, st, "variance",
                                                       _first_bad(got[1], want[1]))


# ---- 1. every frame, signal and parameter set ----

@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_svgf_device_equals_host(R, torch_cuda, ctx, name, kind):
    for W, H in FRAMES:
        _check_svgf(torch_cuda, R, ctx, name, kind, W, H, SVGF_SETS)


def _check_variance(torch, R, ctx, name, kind, W, H, cases):
    d_hits = _dev(torch, G.guides(name, W, H))
    acc, m2 = S.state(name, W, H, kind)
    d_acc, d_m2 = _dev(torch, acc), _dev(torch, m2)
    d_len = {w: _dev(torch, S.len_field(name, W, H, w)) for w in S.LEN_FIELDS}
    for which, st in cases:
        got = _variance(torch, R, ctx, d_hits, W, H, S.variance_params(R, name, kind, st), d_acc, d_m2,
                        d_len[which])
        want = S.want_variance(name, W, H, kind, which, st)
        assert got.tobytes() == want.tobytes(), (name, kind, W, H, which, st, _first_bad(got, want))


@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("name", SCENES)
def test_variance_device_equals_host(R, torch_cuda, ctx, name, kind):
    for W, H in FRAMES:
        _check_variance(torch_cuda, R, ctx, name, kind, W, H, S.variance_cases())


# ---- 2. both forms of the pass kernel ----

@pytest.mark.parametrize("form", ["tiled", "direct"])
def test_forced_form_equals_host(R, torch_cuda, ctx, form, monkeypatch):
    """RTG_SVGF_FORM is read by every call: `tiled` stages steps 1 to 8 in LDS
    (step 8 needs more than 64 KiB of it), `direct` reads every tap from memory."""
    monkeypatch.setenv("RTG_SVGF_FORM", form)
    W, H = FULL
    for name in SCENES:
        for kind in SIGNALS:
            _check_svgf(torch_cuda, R, ctx, name, kind, W, H, SVGF_SETS)


# ---- 3. both sides of the variance kernel's vote ----

@pytest.mark.parametrize("name", SCENES)
def test_len_fields_on_both_sides_of_the_vote(R, torch_cuda, ctx, name):
    """`long`: no tile stages; `zero`: every tile with a hit does; `one`: one
    tile of the 67 x 35 frame stages for one pixel and its other lanes take the
    temporal estimate from the stage; `seeded`: a mixture."""
    W, H = FULL
    st = S.VAR_FEW[0]
    for kind in SIGNALS:
        _check_variance(torch_cuda, R, ctx, name, kind, W, H, [(w, st) for w in S.LEN_FIELDS])
        long_, one = (S.want_variance(name, W, H, kind, w, st) for w in ("long", "one"))
        assert (long_ != one).sum() == 1


# ---- 4. the one-shot forms ----

def test_one_shots(R, torch_cuda):
    for name, (W, H), kind, st in (("reference", FULL, "gray", SVGF_SETS[18 + 2]),
                                   ("c5", FULL, "rgb", SVGF_SETS[18 + 3]),
                                   (12, (33, 17), "gray", SVGF_SETS[4]),
                                   (12, (1, 1), "rgb", SVGF_SETS[18 + 1])):
        v, var = R.svgf(G.guides(name, W, H), W, H, S.svgf_params(R, name, kind, st),
                        G.signal(name, W, H, kind), S.var_field(name, W, H))
        assert v.shape == ((H, W, 3) if kind == "rgb" else (H, W)) and var.shape == (H, W)
        want = S.want_svgf(name, W, H, kind, st)
        assert v.view(np.uint32).reshape(-1).tobytes() == want[0].tobytes(), (name, W, H, kind, st)
        assert var.view(np.uint32).reshape(-1).tobytes() == want[1].tobytes(), (name, W, H, kind, st)
    for name, (W, H), kind, which, st in (("reference", FULL, "rgb", "seeded", S.VAR_SETS[6 + 5]),
                                          ("c5", (33, 17), "gray", "zero", S.VAR_FEW[1]),
                                          (12, (1, 1), "rgb", "one", S.VAR_FEW[0])):
        acc, m2 = S.state(name, W, H, kind)
        got = R.variance(G.guides(name, W, H), W, H, S.variance_params(R, name, kind, st), acc, m2,
                         S.len_field(name, W, H, which))
        assert got.shape == (H, W)
        want = S.want_variance(name, W, H, kind, which, st)
        assert got.view(np.uint32).reshape(-1).tobytes() == want.tobytes(), (name, W, H, kind, which)


# ---- 5. a stream of its own, between two renders ----

def test_own_stream_between_renders(R, torch_cuda):
    torch = torch_cuda
    sph, lg = R.reference_scene()
    W, H = FULL
    name, kind, st, vst = "reference", "rgb", SVGF_SETS[18 + 3], S.VAR_FEW[0]
    d_hits = _dev(torch, G.guides(name, W, H))
    d_src, d_var = _dev(torch, G.signal(name, W, H, kind)), _dev(torch, S.var_field(name, W, H))
    acc, m2 = S.state(name, W, H, kind)
    d_acc, d_m2, d_len = _dev(torch, acc), _dev(torch, m2), _dev(torch, S.len_field(name, W, H, "seeded"))
    c = R.Context(0)
    try:
        c.set_scene(sph, lg)
        fb = [torch.zeros((48 * 36 * 3,), dtype=torch.float32, device="cuda") for _ in range(2)]
        own = torch.cuda.Stream()
        c.render_device(48, 36, fb[0].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        got_var = _variance(torch, R, c, d_hits, W, H, S.variance_params(R, name, kind, vst), d_acc,
                            d_m2, d_len, stream=own.cuda_stream)
        got = _svgf(torch, R, c, d_hits, W, H, S.svgf_params(R, name, kind, st), d_src, d_var,
                    stream=own.cuda_stream)
        c.render_device(48, 36, fb[1].data_ptr(), alias_factor=2.0, stream=_stream(torch))
        torch.cuda.synchronize()
        want = S.want_svgf(name, W, H, kind, st)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert got_var.tobytes() == S.want_variance(name, W, H, kind, "seeded", vst).tobytes()
        a, b = fb[0].cpu().numpy(), fb[1].cpu().numpy()
        assert (a != 0).any() and G.canon(a).tobytes() == G.canon(b).tobytes()
        assert G.canon(a).tobytes() == G.canon(R.render(sph, lg, 48, 36, alias_factor=2.0)).tobytes()
    finally:
        c.close()


# ---- 6. the device chain ----

def test_device_chain_equals_host_chain(R, torch_cuda):
    torch = torch_cuda
    cfg, p = S.CHAIN, S.chain_params(R)
    W, H, name = cfg["W"], cfg["H"], cfg["name"]
    n = W * H
    h, acc, ln, m2, var, dst, dvar = S.chain_host()
    w32 = lambda a: np.ascontiguousarray(a).view(np.uint32).reshape(-1)  # noqa: E731
    table = aogen.dirs(8)
    c = R.Context(0)
    try:
        c.set_scene(aogen.scene(name), scene_with_lights(name)[1])
        d_rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        d_counts = torch.empty((n,), dtype=torch.int16, device="cuda")
        d_dirs = _dev(torch, table)
        d_hits = [torch.empty((n, 8), dtype=torch.int32, device="cuda") for _ in range(2)]
        d_acc = [_filled(torch, n) for _ in range(2)]
        d_m2 = [_filled(torch, n) for _ in range(2)]
        d_len = [torch.full((n + PAD,), FILL16, dtype=torch.int16, device="cuda") for _ in range(2)]
        s = _stream(torch)
        for k, (cam, ap) in enumerate(zip(p["cams"], p["aos"])):
            a, b = k & 1, (k & 1) ^ 1
            c.camera_rays(cam, W, H, d_rays.data_ptr(), alias_factor=1.0, stream=s)
            c.intersect_device(d_rays.data_ptr(), n, d_hits[a].data_ptr(), stream=s)
            c.ao_device(d_hits[a].data_ptr(), n, ap, d_dirs.data_ptr(), 8, d_counts.data_ptr(), stream=s)
            pv = None if k == 0 else (p["cams"][k - 1], d_hits[b].data_ptr(), d_acc[b].data_ptr(),
                                      d_len[b].data_ptr(), d_m2[b].data_ptr())
            c.accumulate_device(d_hits[a].data_ptr(), W, H, p["accum"], d_counts.data_ptr(),
                                d_acc[a].data_ptr(), d_len[a].data_ptr(), pv, zoom=-4.0,
                                out_m2_ptr=d_m2[a].data_ptr(), stream=s)
        last = (cfg["frames"] - 1) & 1
        got_var = _variance(torch, R, c, d_hits[last], W, H, p["variance"], d_acc[last], d_m2[last],
                            d_len[last])
        assert got_var.tobytes() == w32(var).tobytes(), _first_bad(got_var, w32(var))
        got = _svgf(torch, R, c, d_hits[last], W, H, p["svgf"], d_acc[last], _dev(torch, got_var))
        assert _tail_kept(d_acc[last], n, "acc").tobytes() == w32(acc).tobytes()
        assert _tail_kept(d_m2[last], n, "m2").tobytes() == w32(m2).tobytes()
        assert (d_len[last].cpu().numpy().view(np.uint16)[:n] == ln.reshape(-1)).all()
        assert got[0].tobytes() == w32(dst).tobytes(), _first_bad(got[0], w32(dst))
        assert got[1].tobytes() == w32(dvar).tobytes(), _first_bad(got[1], w32(dvar))
    finally:
        c.close()


# ---- 7. the driver ----

def _pgm_of(v, K, W, H):
    x = F(255) * v.reshape(-1).astype(F) / F(K)
    x = np.where(x > 0, np.where(x < 255, x, F(255)), F(0))
    return b"P5\n%d %d\n255\n" % (W, H) + x.astype(np.uint8).tobytes()


def test_host_driver_variance_options(R, torch_cuda, tmp_path):
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
    cams = [R.camera_look_at(*q) for q in path] + [R.camera_look_at((3, 2, -1), (0, 0, -10))]
    hits = [R.intersect_host(sph, R.camera_rays_host(c, W, H, alias_factor=1.0), walk=0,
                             threads=THREADS) for c in cams]
    table = R.ao_directions(K)
    flags = R.FILTER_SAME_ID | R.FILTER_NORMAL | R.FILTER_PLANE

    def run(extra):
        r = subprocess.run(base + pose + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr

    def chain(signal, ap, history):
        """The accumulated (acc, len, m2) of the path, or of the last frame alone."""
        prev = None
        for k in (range(len(cams)) if history else [len(cams) - 1]):
            out = R.accumulate_host(hits[k], W, H, ap, signal(k if history else 0, hits[k]), prev,
                                    zoom=-4.0, m2=True, threads=THREADS)
            prev = (cams[k], hits[k]) + tuple(out)
        return prev[2:]

    def guided(kind, kflags, state, passes, scale, sigma, min_history):
        acc, ln, m2 = state
        var = R.variance_host(hits[-1], W, H, R.variance_params(kind, kflags, scale, 3, min_history),
                              acc, m2, ln, threads=THREADS)
        return R.svgf_host(hits[-1], W, H, R.svgf_params(passes, kind, kflags | R.SVGF_LUMA, scale, 3,
                                                         sigma, 1e-6), acc, var, threads=THREADS)[0]

    # --ao: the counts of frame k have seed 5 + k; without a history the one frame has seed 5
    ao = lambda k, h: R.ao_host(sph, h, table, R.ao_params(K, 12.5, 1e-3, 5 + k, R.AO_JITTER),  # noqa: E731
                                walk=0, threads=THREADS)
    ap = R.accumulate_params(R.FILTER_COUNT, flags, 1.0, 3, 65535)
    out = str(tmp_path / "ao.pgm")
    seen = set()
    args = ["--ao", "16,12.5,0.001,5", "--ao-out", out, "--ao-filter", "3,0.5"]
    for history in (False, True):
        more = ["--ao-history", poses_file] if history else []
        state = chain(ao, ap, history)
        for spec, sigma, mh in (("4", 4.0, 4), ("1.5,2", 1.5, 2)):
            run(args + more + ["--ao-variance", spec])
            want = _pgm_of(guided(R.FILTER_GRAY, flags, state, 3, 0.5, sigma, mh), K, W, H)
            assert open(out, "rb").read() == want, (history, spec)
            seen.add(want)
        # the same command line without the option: today's chain
        run(args + more)
        src = state[0] if history else ao(0, hits[-1])
        kind = R.FILTER_GRAY if history else R.FILTER_COUNT
        want = _pgm_of(R.filter_host(hits[-1], W, H, R.filter_params(3, kind, flags, 0.5, 3), src),
                       K, W, H)
        assert open(out, "rb").read() == want, history
        seen.add(want)
    assert len(seen) >= 5  # the variance term, its sigma and the history change the picture
    # --gather, with --gather-skip
    wts = np.full(K, F(1) / F(K), F)

    def light(k, h):
        g = R.gather_host(sph, lg, h, table, wts, R.gather_params(K, 1e-3, 9 + k, R.GATHER_JITTER |
                                                                  R.GATHER_SKIP_NONFINITE),
                          stack_size=6, walk=0, threads=THREADS)
        return np.asarray(g if not isinstance(g, tuple) else g[0], F).reshape(W * H, 3)

    gp = R.accumulate_params(R.FILTER_RGB, flags | R.ACCUM_SKIP_NONFINITE, 1.0, 3, 65535)
    out = str(tmp_path / "g.ppm")
    args = ["--gather", "16,0.001,9", "--gather-skip", "--gather-out", out, "--gather-filter", "2"]
    kf = flags | R.FILTER_SKIP_NONFINITE
    pictures = set()
    for history in (False, True):
        more = ["--gather-history", poses_file] if history else []
        state = chain(light, gp, history)
        run(args + more + ["--gather-variance", "4"])
        want = R.ppm_file_bytes(guided(R.FILTER_RGB, kf, state, 2, 1.0, 4.0, 4))
        assert open(out, "rb").read() == want, history
        pictures.add(want)
        run(args + more)
        src = state[0] if history else light(0, hits[-1])
        want = R.ppm_file_bytes(R.filter_host(hits[-1], W, H, R.filter_params(2, R.FILTER_RGB, kf, 1.0, 3),
                                              src))
        assert open(out, "rb").read() == want, history
        pictures.add(want)
    assert len(pictures) == 4
    for bad in (["--ao", "16,1", "--ao-out", "x.pgm", "--ao-variance", "4"],
                ["--gather", "16", "--gather-out", "x.ppm", "--gather-variance", "4"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-filter", "3", "--ao-variance", "x"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-filter", "3", "--ao-variance", "4,65536"],
                ["--ao", "16,1", "--ao-out", "x.pgm", "--ao-filter", "3", "--ao-variance", "4,2,1"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("Invalid variance" in r.stdout or "needs --" in r.stdout), r.stdout
    r = subprocess.run(base[:1] + ["--help"], capture_output=True, text=True, timeout=120)
    assert "--ao-variance" in r.stdout and "--gather-variance" in r.stdout


# ---- 8. entry-point errors ----

def test_device_entry_point_errors(R, torch_cuda, ctx):
    torch = torch_cuda
    W, H = 33, 17
    n = W * H
    d_hits = _dev(torch, G.guides("reference", W, H))
    d_src = _dev(torch, G.signal("reference", W, H, "gray"))
    d_var = _dev(torch, S.var_field("reference", W, H))
    out = torch.zeros((4 * n + PAD,), dtype=torch.int32, device="cuda")
    scratch = torch.zeros((2 * n + 8 + PAD,), dtype=torch.int32, device="cuda")
    ok = R.svgf_params(3, R.FILTER_GRAY, ALL | R.SVGF_LUMA, 1.0, 3)
    need = R.svgf_scratch(W, H, ok)
    assert need == 2 * ((n * 4 + 15) // 16 * 16)
    hp, sp, vp, op, cp = (t.data_ptr() for t in (d_hits, d_src, d_var, out, scratch))
    ov = op + 4 * n  # the variance's destination
    assert hp % 16 == 0 and cp % 16 == 0
    good = (hp, W, H, ok, sp, vp, op, ov, cp, need)

    def but(**kw):
        a = dict(zip(("h", "W", "H", "p", "src", "var", "dst", "dvar", "scr", "need"), good))
        a.update(kw)
        return tuple(a.values())

    for a, msg in ((but(h=0), "svgf: null hit buffer"), (but(src=0), "svgf: null source"),
                   (but(var=0), "svgf: null source variance"), (but(dst=0), "svgf: null destination"),
                   (but(dvar=0), "svgf: null destination variance"),
                   (but(scr=0), "svgf: null scratch"),
                   (but(W=0), "svgf: empty frame"), (but(H=0), "svgf: empty frame"),
                   (but(W=1 << 16, H=1 << 16), "at most 2\\^32 - 1"),
                   (but(p=R.svgf_params(0, 1)), "0 passes"), (but(p=R.svgf_params(9, 1)), "9 passes"),
                   (but(p=R.svgf_params(2, 1, normal_log2=9)), "normalLog2 9"),
                   (but(p=R.svgf_params(2, 3)), "kind 3"),
                   (but(p=R.svgf_params(2, R.FILTER_COUNT)), "kind COUNT"),
                   (but(p=R.svgf_params(2, 1, 32)), "unknown flags 0x20"),
                   (but(h=hp + 4), "hit buffer not 16-byte aligned"),
                   (but(need=need - 1), "svgf: scratch of"), (but(scr=cp + 4), "svgf: scratch of"),
                   (but(dst=sp), "the destination overlaps the source"),
                   (but(dst=sp + 4 * n - 4), "the destination overlaps the source"),
                   (but(dvar=sp), "the destination variance overlaps the source"),
                   (but(dst=vp), "the destination overlaps the source variance"),
                   (but(dvar=vp), "the destination variance overlaps the source variance"),
                   (but(dvar=op + 4 * n - 4), "the destination variance overlaps the destination"),
                   (but(src=cp), "the scratch overlaps the source"),
                   (but(var=cp + need - 4 * n), "the scratch overlaps the source variance"),
                   (but(dst=cp), "the scratch overlaps the destination"),
                   (but(dvar=cp + need - 16), "the scratch overlaps the destination variance")):
        with pytest.raises(R.RtgError, match=msg):
            ctx.svgf_device(*a)
    L = R.lib()
    assert L.rtg_svgf_device(ctx._h, hp, W, H, None, sp, vp, op, ov, cp, need, None) == -1
    assert b"svgf: null params" in L.rtg_last_error()
    assert L.rtg_svgf_device(None, hp, W, H, R._ptr(ok), sp, vp, op, ov, cp, need, None) == -1
    assert b"svgf: no context" in L.rtg_last_error()
    # rtg_variance_device
    d_len = _dev(torch, S.len_field("reference", W, H, "seeded"))
    lp = d_len.data_ptr()
    vok = R.variance_params(R.FILTER_GRAY, ALL, 1.0, 3, 4)
    vgood = (hp, W, H, vok, sp, vp, lp, op)

    def vbut(**kw):
        a = dict(zip(("h", "W", "H", "p", "acc", "m2", "len", "out"), vgood))
        a.update(kw)
        return tuple(a.values())

    for a, msg in ((vbut(h=0), "variance: null hit buffer"), (vbut(acc=0), "variance: null acc"),
                   (vbut(m2=0), "variance: null m2"), (vbut(len=0), "variance: null len"),
                   (vbut(out=0), "variance: null destination"),
                   (vbut(W=0), "variance: empty frame"),
                   (vbut(W=1 << 16, H=1 << 16), "at most 2\\^32 - 1"),
                   (vbut(p=R.variance_params(R.FILTER_COUNT)), "kind COUNT"),
                   (vbut(p=R.variance_params(1, 16)), "unknown flags 0x10"),
                   (vbut(p=R.variance_params(1, normal_log2=9)), "normalLog2 9"),
                   (vbut(p=R.variance_params(1, min_history=65536)), "minHistory 65536"),
                   (vbut(h=hp + 4), "hit buffer not 16-byte aligned"),
                   (vbut(out=sp), "the destination overlaps the acc"),
                   (vbut(out=vp), "the destination overlaps the m2"),
                   (vbut(out=lp), "the destination overlaps the len")):
        with pytest.raises(R.RtgError, match=msg):
            ctx.variance_device(*a)
    assert L.rtg_variance_device(ctx._h, hp, W, H, None, sp, vp, lp, op, None) == -1
    assert b"variance: null params" in L.rtg_last_error()
    assert L.rtg_variance_device(None, hp, W, H, R._ptr(vok), sp, vp, lp, op, None) == -1
    assert b"variance: no context" in L.rtg_last_error()
    torch.cuda.synchronize()
    assert int(out.count_nonzero()) == 0 and int(scratch.count_nonzero()) == 0  # nothing launched
    # one pass needs no scratch: null is legal
    ctx.svgf_device(hp, W, H, R.svgf_params(1, R.FILTER_GRAY, ALL | R.SVGF_LUMA, 1.0, 3), sp, vp, op, ov)
    torch.cuda.synchronize()
    assert int(out[:2 * n].count_nonzero()) > 0 and int(out[2 * n:].count_nonzero()) == 0
