"""GPU tests of bench.py: the plain run with its output dump, and the N > 1
step (the driver's multi-GPU scaling run).

Two ranks share the box's one GPU and gather through host memory (gloo), so
the chunked pipeline the 8-GPU run uses — row-cyclic shards rendered in
chunks on two streams, each chunk gathered and put back in row order on rank
0's assembling stream — runs end to end on every GPU test pass, and its
fields are checked: the assembled frame is the golden frame, the per-rank
timings are non-negative and the rank-0 render + gather tail + assemble fit
in the step.
"""
from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits_equal, canon_md5, load_f32

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bench_lines(args, nproc, timeout=240):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return lines[0]


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_bench_plain_run_dumps_the_timed_frame(golden, tmp_path, name):
    """A plain bench.py run reports the timed steps only (none of --full's
    sections) and --dump-outputs writes the last timed frame: C1's whole,
    bit-equal to the golden frame; of C3's (99.5 MB) the documented seeded
    pixel sample, bit-equal to the golden rows where it meets them.  Two
    float32 arrays, no NaN in either, at most 64 MB together."""
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "2", "--warmup", "1", "--config", name, "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = lines[0]
    assert line["full"] is False and line["steps"] == 2 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["unit"] == "Mpixels/s" and line["dtype"] == "f32"
    for key in ("parity", "cpu_baseline", "roofline", "e2e"):
        assert key not in line
    assert sorted(os.listdir(out_dir)) == ["frame.npy", "frame_isnan.npy"]
    assert sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64e6
    vals, isnan = np.load(out_dir / "frame.npy"), np.load(out_dir / "frame_isnan.npy")
    assert vals.dtype == isnan.dtype == np.float32 and vals.shape == isnan.shape
    assert not np.isnan(vals).any() and set(np.unique(isnan)) <= {0.0, 1.0}
    got = np.where(isnan > 0, np.float32("nan"), vals)
    c = golden["configs"][name]
    W, H = c["W"], c["H"]
    if name == "c1":
        assert got.shape == (H, W, 3)
        assert canon_md5(got) == c["fb_md5"]
        return
    px = (48 << 20) // 24
    idx = np.sort(np.random.default_rng(7).choice(H * W, size=px, replace=False))
    assert got.shape == (px, 3)
    rows = np.asarray(c["rows"]["rows"])
    want = load_f32(os.path.join(GOLDEN, "c3.rows.f32"), (len(rows), W, 3))
    y, x = idx // W, idx % W
    k = np.searchsorted(rows, y).clip(max=len(rows) - 1)
    hit = rows[k] == y
    assert hit.sum() > 1000
    assert bits_equal(got[hit], want[k[hit], x[hit]])


@pytest.mark.parametrize("chunks", [0, 1])
def test_bench_two_rank_step(chunks):
    """bench.py --gpus 2 (gloo, both ranks on GPU 0) on C2: default chunking
    (4 chunks at two ranks) and a single gather."""
    out = _bench_lines(["--gpus", "2", "--steps", "4", "--warmup", "2", "--config", "c2", "--full",
                        "--dist-backend", "gloo", "--gather-chunks", str(chunks)], 2)
    assert out["n_gpus"] == 2
    assert out["parity"]["fb_md5_match"] is True
    assert out["parity"]["ppm_md5_match"] is True
    mg = out["multi_gpu"]
    assert mg["gather_chunks"] == (4 if chunks == 0 else 1)
    assert len(mg["render_ms_per_rank"]) == 2
    assert all(t > 0 for t in mg["render_ms_per_rank"])
    assert mg["gather_tail_ms_rank0"] >= 0.0
    assert mg["assemble_ms_rank0"] >= 0.0
    step = mg["step_ms"]
    assert mg["render_ms_per_rank"][0] + mg["gather_tail_ms_rank0"] + \
        mg["assemble_ms_rank0"] <= step * 1.05, mg
    assert out["value"] > 0 and abs(out["ms_per_step"] - step) < 1e-3 * step + 1e-3
