"""GPU tests of one context rendering on several streams with work in flight
(launch_trace in csrc/rtg_kernel.hip) on an MI355X: the three stream waits
that order a context's compacted-launch scratch between streams, and
rtg_context_set_scene / rtg_context_destroy called behind pending launches.

Scenes of at most 64 spheres render through a ring of four scratch slots
(rtg_context::kSlots) and up to eight launch-order cost entries.  A launch
waits (hipStreamWaitEvent, skipped on the same stream)

  1. for a slot's last launch before it reuses the slot; a larger frame then
     frees and reallocates the slot's list stream-ordered behind that wait;
  2. for the last launch of a cost entry it replaces (least recently used);
  3. for the last launch of a cost entry it shares with another stream.

The schedules below put a launch that needs one of these waits behind a
launch that is still running:

  1. slot reuse: the fifth launch takes the slot of the first, the heavy one;
  2. slot reuse with growth: the reused slot's list is too small;
  3. shared entry: one geometry on two streams at once;
  4. replacement: the ninth geometry replaces the heavy launch's entry;
  5. set_scene and close() right behind the heavy launch;
  6. every device entry point of the context on four streams at once.

One context on C3 (16 spheres, tests/golden).  Every launch writes its own
destination, pre-filled and PAD words longer than the result; the tail must
stay.  The full 3840 x 2160 frame is held to the golden md5 once per test and
its repeats are compared to that verified frame on the device, as int32 words;
every other size is held to the oracle.  Frames are verified after one
torch.cuda.synchronize() at the end of a round.  Launches that must not share
a cost entry get frame sizes of their own (the geometry key mixes W, H, zoom,
the alias factor, the stack size, the sharding and the scene generation).

Four streams and no more: a process opens four hardware queues here, and two
streams on one queue run in order whatever the library does, which would hide
a missing wait.

Evidence of overlap.  Ordering is only tested if the heavy launch is still
running when the contested one is enqueued, so schedules 1 to 5 record an event
behind the heavy launch and query it right after enqueuing the contested
launch (before the call, for the two blocking calls of schedule 5).  Each
schedule runs five rounds; every frame of every round must be right, and the
event must have been pending in at least one round, or the test FAILS saying
so.  A schedule that never sees C3's frame (about 1.35 ms) pending repeats with
C4's (32 spheres, about 9.5 ms) and says which in its report line.  This
condition stands in for a run with a wait removed: such a race could write
outside a frame, and no test provokes that.

Out of scope: hipStreamPerThread; stream handles destroyed and recreated with
work pending; rtg_render_multi on more than one device; scenes above 64
spheres (they do not take the compacted launch).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from conftest import bits_equal, canon, canon_md5, first_mismatch, load_scene

pytestmark = pytest.mark.gpu

PAD = 64  # words the destinations are longer than the result
FILL = 0x5A5A5A5A
ROUNDS = 5
# distinct sizes around 96 x 54: one cost entry each
SMALL = ((96, 54), (97, 55), (95, 53), (98, 54), (94, 55), (99, 53), (93, 54), (100, 55))
HEAVY = ("c3", "c4")  # the heavy launch: C3's golden frame, C4's where C3's is over too soon
MID = (2560, 1440)  # the launch in flight of schedule 2


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
def streams(torch_cuda):
    """The module's four streams."""
    return tuple(torch_cuda.cuda.Stream() for _ in range(4))


@functools.lru_cache(maxsize=None)
def _config(cfg):
    import json
    import os

    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        c = json.load(f)["configs"][cfg]
    sph, lg = load_scene(cfg, c["spheres"], c["lights"])
    return c, sph, lg


_oracle_frames = {}


def _want(oracle, cfg, W, H):
    """The oracle's W x H frame of a golden scene, computed once, read-only."""
    if (cfg, W, H) not in _oracle_frames:
        c, sph, lg = _config(cfg)
        fb = oracle.render(sph, lg, W, H, c["stack_size"])
        assert (fb != 0).any(), "black frame"
        fb.setflags(write=False)
        _oracle_frames[cfg, W, H] = fb
    return _oracle_frames[cfg, W, H]


class Frame:
    """One render's destination, W * H * 3 words plus PAD, and its check."""

    def __init__(self, torch, cfg, W, H):
        self.torch, self.cfg, self.W, self.H = torch, cfg, W, H
        self.S = _config(cfg)[0]["stack_size"]
        self.words = W * H * 3
        self.t = torch.full((self.words + PAD,), FILL, dtype=torch.int32, device="cuda")
        self.verified = None  # the words of a frame found right, on the device

    def refill(self):
        self.t.fill_(FILL)

    def launch(self, ctx, stream):
        ctx.render_device(self.W, self.H, self.t.data_ptr(), stack_size=self.S,
                          stream=stream.cuda_stream)

    def check(self, oracle, what):
        """After the synchronisation: the tail stayed; the frame is the golden
        md5's (a config's own size) or the oracle's, or, once one was, its words."""
        torch = self.torch
        assert bool((self.t[self.words:] == FILL).all()), (what, "words past the frame were written")
        if self.verified is not None:
            same = torch.equal(self.t[:self.words], self.verified)
            assert same, (what, int((self.t[:self.words] != self.verified).sum()), "words differ")
            return
        c = _config(self.cfg)[0]
        fb = self.t[:self.words].cpu().numpy().view(np.float32).reshape(self.H, self.W, 3)
        if (self.W, self.H) == (c["W"], c["H"]):
            assert canon_md5(fb) == c["fb_md5"], (what, self.cfg, "not the golden frame")
        else:
            want = _want(oracle, self.cfg, self.W, self.H)
            assert bits_equal(fb, want), (what, first_mismatch(fb, want))
        if self.words > 1 << 20:  # a large frame's repeats: compared on the device
            self.verified = self.t[:self.words].clone()


def _full(torch, cfg):
    c = _config(cfg)[0]
    return Frame(torch, cfg, c["W"], c["H"])


def _context(R, cfg):
    ctx = R.Context(0)
    ctx.set_scene(*_config(cfg)[1:])
    assert ctx.scene_stats()["bvh_nodes"] == 0 and len(_config(cfg)[1]) <= 64
    return ctx


def _begin(torch, frames):
    """Pre-fill every destination; the fills are done before any stream renders."""
    for f in frames:
        f.refill()
    torch.cuda.synchronize()


def _report(capsys, number, what, cfg, pending):
    line = ", ".join(f"{label}: {sum(p)} of {len(p)}" for label, p in pending.items())
    with capsys.disabled():
        print(f"\n[inflight] schedule {number} ({what}), heavy launch {cfg} "
              f"{_config(cfg)[0]['W']}x{_config(cfg)[0]['H']}: still pending in {line} rounds")


def _until_pending(capsys, number, what, schedule, heavy=HEAVY):
    """schedule(cfg) -> {label: [pending per round]} (it asserts its frames);
    every label needs a round with the heavy launch still pending, with C3 or,
    failing that, with C4."""
    for cfg in heavy:
        pending = schedule(cfg)
        _report(capsys, number, what, cfg, pending)
        if all(any(p) for p in pending.values()):
            return
    pytest.fail(f"schedule {number}: the heavy launch was never still pending when the contested "
                f"launch had been enqueued ({pending}): the schedule tested no ordering")


# ---- 1. slot reuse ----

def test_slot_reuse(R, oracle, torch_cuda, streams, capsys):
    """The heavy frame on stream 0, a small frame on each of streams 1 to 3,
    then a fourth small frame, the fifth compacted launch, which takes the
    heavy launch's slot: on each other stream in turn, five rounds each.  The
    fourth small frame's cull pass rewrites the slot's list, masks and
    counters, which the heavy launch's trace kernel is reading: wait 1."""
    torch = torch_cuda

    def schedule(cfg):
        heavy = _full(torch, cfg)
        small = [Frame(torch, cfg, W, H) for W, H in SMALL[:4]]
        pending = {}
        ctx = _context(R, cfg)
        try:
            for k in (1, 2, 3):
                seen = pending[f"fifth launch on stream {k}"] = []
                for r in range(ROUNDS):
                    _begin(torch, [heavy] + small)
                    ev = torch.cuda.Event()
                    heavy.launch(ctx, streams[0])
                    ev.record(streams[0])
                    for i in (1, 2, 3):
                        small[i - 1].launch(ctx, streams[i])
                    small[3].launch(ctx, streams[k])
                    seen.append(not ev.query())
                    torch.cuda.synchronize()
                    heavy.check(oracle, ("heavy", k, r))
                    for i, f in enumerate(small):
                        f.check(oracle, ("small", i, k, r))
        finally:
            ctx.close()
        return pending
    _until_pending(capsys, 1, "slot reuse", schedule)


# ---- 2. slot reuse with growth ----

def test_slot_reuse_with_growth(R, oracle, torch_cuda, streams, capsys):
    """C3 at 2560 x 1440 in flight on stream 0, three small frames on streams 1
    to 3 (they move the ring on), then the full frame on stream 1 in the slot
    of the launch in flight, whose list is too small for it: freed and
    reallocated on stream 1, behind wait 1.  A round is five launches, so round
    r starts on slot r % 4: the full frame finds a list it must grow in rounds
    0 to 3 (a slot that last held nothing or the 2560 x 1440 frame) and its own
    in round 4, and the launch in flight must have been pending in a round
    that grows."""
    torch = torch_cuda
    cfg = "c3"
    mid, full = Frame(torch, cfg, *MID), _full(torch, cfg)
    small = [Frame(torch, cfg, W, H) for W, H in SMALL[:3]]
    seen = []
    ctx = _context(R, cfg)
    try:
        for r in range(ROUNDS):
            _begin(torch, [mid, full] + small)
            ev = torch.cuda.Event()
            mid.launch(ctx, streams[0])
            ev.record(streams[0])
            for i in (1, 2, 3):
                small[i - 1].launch(ctx, streams[i])
            full.launch(ctx, streams[1])
            seen.append(not ev.query())
            torch.cuda.synchronize()
            mid.check(oracle, ("in flight", r))
            full.check(oracle, ("full", r))
            for i, f in enumerate(small):
                f.check(oracle, ("small", i, r))
    finally:
        ctx.close()
    with capsys.disabled():
        print(f"\n[inflight] schedule 2 (slot reuse with growth), launch in flight c3 "
              f"{MID[0]}x{MID[1]}: still pending in {sum(seen[:4])} of 4 rounds that grow the list, "
              f"{sum(seen[4:])} of 1 that does not")
    if not any(seen[:4]):
        pytest.fail(f"schedule 2: the 2560 x 1440 launch was never still pending when the full "
                    f"frame had been enqueued ({seen}): the schedule tested no ordering")


# ---- 3. shared entry ----

def test_shared_entry(R, oracle, torch_cuda, streams, capsys):
    """The heavy frame on stream 0, the same geometry into a second buffer on
    stream 1, a small frame on stream 2.  Both heavy launches add to and zero
    the sums of one cost entry: wait 3.  The entry's launches are counted
    across the rounds, so round 0 runs it with no costStat and then with
    costStat only, every later round ordered by costPrev."""
    torch = torch_cuda

    def schedule(cfg):
        a, b = _full(torch, cfg), _full(torch, cfg)
        small = Frame(torch, cfg, *SMALL[0])
        seen = []
        ctx = _context(R, cfg)
        try:
            for r in range(ROUNDS):
                _begin(torch, [a, b, small])
                ev = torch.cuda.Event()
                a.launch(ctx, streams[0])
                ev.record(streams[0])
                b.launch(ctx, streams[1])
                seen.append(not ev.query())
                small.launch(ctx, streams[2])
                torch.cuda.synchronize()
                a.check(oracle, ("first", r))
                b.verified = a.verified
                b.check(oracle, ("second", r))
                small.check(oracle, ("small", r))
        finally:
            ctx.close()
        return {"same geometry on stream 1": seen}
    _until_pending(capsys, 3, "shared entry", schedule)


# ---- 4. replacement ----

def test_entry_replaced_in_flight(R, oracle, torch_cuda, streams, capsys):
    """The heavy frame on stream 0 of a fresh context, then eight small frames
    of eight sizes dealt over streams 1 to 3: the eighth is the ninth geometry,
    so it replaces the heavy launch's cost entry, the least recently used,
    while that launch runs (wait 2).  A second pass over the same nine replaces
    every entry again, the heavy launch's first.

    What this shows: replacement in flight does no harm to any of the nine
    frames.  It does not claim more: a cost entry holds scheduling hints (the
    groups' measured times and their sums), so a missing wait 2 mostly
    disturbs the order in which groups are listed, and here the slot waits of
    the fifth and ninth launch already put the eighth small frame behind the
    heavy launch."""
    torch = torch_cuda

    def schedule(cfg):
        heavy = _full(torch, cfg)
        small = [Frame(torch, cfg, W, H) for W, H in SMALL]
        pending = {"pass 1": [], "pass 2": []}
        for r in range(ROUNDS):
            ctx = _context(R, cfg)
            try:
                for label in pending:
                    _begin(torch, [heavy] + small)
                    ev = torch.cuda.Event()
                    heavy.launch(ctx, streams[0])
                    ev.record(streams[0])
                    for i, f in enumerate(small):
                        f.launch(ctx, streams[1 + i % 3])
                    pending[label].append(not ev.query())
                    torch.cuda.synchronize()
                    heavy.check(oracle, ("heavy", label, r))
                    for i, f in enumerate(small):
                        f.check(oracle, ("small", i, label, r))
            finally:
                ctx.close()
        return pending
    _until_pending(capsys, 4, "replacement", schedule)


# ---- 5. set_scene and close() behind a launch ----

def test_set_scene_behind_a_launch(R, oracle, torch_cuda, streams, capsys):
    """The heavy frame on stream 0, at once set_scene of C2, then a small C2
    frame on stream 1.  rtg.h: set_scene waits for the context's pending work
    before it frees the old scene, so the heavy launch is over when it returns
    (pending is asked before the call, done after it)."""
    torch = torch_cuda
    c2 = _config("c2")

    def schedule(cfg):
        heavy, small = _full(torch, cfg), Frame(torch, "c2", *SMALL[0])
        seen = []
        ctx = R.Context(0)
        try:
            for r in range(ROUNDS):
                ctx.set_scene(*_config(cfg)[1:])
                _begin(torch, [heavy, small])
                ev = torch.cuda.Event()
                heavy.launch(ctx, streams[0])
                ev.record(streams[0])
                seen.append(not ev.query())
                ctx.set_scene(c2[1], c2[2])
                done = ev.query()
                small.launch(ctx, streams[1])
                torch.cuda.synchronize()
                assert done, (r, "set_scene returned with the heavy launch still running")
                heavy.check(oracle, ("heavy", r))
                small.check(oracle, ("small c2", r))
        finally:
            ctx.close()
        return {"set_scene": seen}
    _until_pending(capsys, "5a", "set_scene behind a launch", schedule)


def test_close_behind_a_launch(R, oracle, torch_cuda, streams, capsys):
    """The heavy frame on stream 0, at once close(): rtg_context_destroy waits
    for the context's pending work before it frees anything."""
    torch = torch_cuda

    def schedule(cfg):
        heavy = _full(torch, cfg)
        seen = []
        for r in range(ROUNDS):
            ctx = _context(R, cfg)
            try:
                _begin(torch, [heavy])
                ev = torch.cuda.Event()
                heavy.launch(ctx, streams[0])
                ev.record(streams[0])
                seen.append(not ev.query())
            finally:
                ctx.close()
            done = ev.query()
            torch.cuda.synchronize()
            assert done, (r, "close() returned with the heavy launch still running")
            heavy.check(oracle, ("heavy", r))
        return {"close": seen}
    _until_pending(capsys, "5b", "close() behind a launch", schedule)


# ---- 6. everything at once ----

class _Job:
    """One launch of schedule 6: pre-filled int32 destinations, the call and
    the words they must hold afterwards."""

    def __init__(self, torch, name, stream, call, wants):
        self.name, self.stream, self.call = name, stream, call
        self.wants = [_bytes(w) for w in wants]
        self.floats = [np.asarray(w).dtype == np.float32 for w in wants]
        # (bytes: the results are 1 to 32 bytes a record)
        self.dst = [torch.full((len(w) + 4 * PAD,), 0x5A, dtype=torch.uint8, device="cuda")
                    for w in self.wants]

    def launch(self, stream):
        self.call(stream.cuda_stream, *(d.data_ptr() for d in self.dst))

    def check(self):
        for k, (d, w, is_float) in enumerate(zip(self.dst, self.wants, self.floats)):
            got = d.cpu().numpy()
            assert (got[len(w):] == 0x5A).all(), (self.name, k, "bytes past the result were written")
            got = got[:len(w)]
            if is_float:  # NaN payloads are not part of the contract (conftest.canon)
                got, w = _bytes(canon(got.view(np.float32))), _bytes(canon(w.view(np.float32)))
            bad = np.flatnonzero(got != w)
            assert not len(bad), (self.name, k, f"{len(bad)} bytes differ, first at {bad[0]}")


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def test_everything_at_once(R, oracle, torch_cuda, streams):
    """Scene 12 of the shared generators (12 spheres, two lights).  With no
    synchronisation between them: on stream 0 two compacted renders of
    different sizes, the G-buffer, closest hits and lines of sight; on stream
    1 the batch ray tracer, the posed camera and the views; on stream 2
    ambient occlusion, direct light and the gather; on stream 3 the filter,
    the accumulation and two more compacted renders.  Inputs and references
    are the existing modules' own; every result is its stand-alone result."""
    torch = torch_cuda
    import accumgen
    import aogen
    import filtergen
    import gathergen
    import mattegen
    from test_gpu_accumulate import _dev_prev
    from test_gpu_order import _batch
    from test_raytrace_host import THREADS
    from test_views_host import VAA, VH, VS, VW, VZOOM, batch_poses, view_frames

    name = 12
    sph, lg, rays, segs, hits, vis = _batch(name)
    assert len(sph) <= 64 and (lg == mattegen.lights(name)).all()
    keep = []  # the inputs on the device

    def dev(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda())
        return keep[-1].data_ptr()

    ctx = R.Context(0)
    ctx.set_scene(sph, lg)
    jobs = []

    def job(stream, label, call, *wants):
        jobs.append(_Job(torch, label, stream, call, wants))

    def render(stream, W, H):
        want = oracle.render(sph, lg, W, H, 6)
        assert (want != 0).any()
        job(stream, f"render {W}x{H}",
            lambda s, p: ctx.render_device(W, H, p, stack_size=6, stream=s), want)

    try:
        # stream 0
        render(0, 96, 54)
        render(0, 80, 45)
        gb = R.gbuffer_host(sph, 32, 24, -4.0, 2.0, threads=THREADS)
        job(0, "gbuffer", lambda s, p: ctx.gbuffer_device(32, 24, p, alias_factor=2.0, stream=s), gb)
        n = len(rays)
        d_rays, d_segs = dev(rays), dev(segs)
        job(0, "intersect", lambda s, p: ctx.intersect_device(d_rays, n, p, stream=s), hits)
        job(0, "visible", lambda s, p: ctx.visible_device(d_segs, n, p, stream=s), vis)
        # stream 1
        cols = R.raytrace_host(sph, lg, rays, stack_size=6, walk=0, threads=THREADS)
        job(1, "raytrace", lambda s, p: ctx.raytrace_device(d_rays, n, p, stack_size=6, stream=s),
            cols)
        cams, frames = batch_poses(name), view_frames(name)
        job(1, "camera", lambda s, p: ctx.render_camera(cams[1].view(R.CAMERA_DTYPE), VW, VH, p,
                                                        VZOOM, VAA, VS, stream=s), frames[1])
        d_cams = dev(cams)
        job(1, "views", lambda s, p: ctx.render_views(d_cams, len(cams), VW, VH, p, VZOOM, VAA, VS,
                                                      stream=s), frames)
        # stream 2
        h, k, nd = aogen.hits(name), 7, 8
        d_hits, d_dirs, d_w = dev(h), dev(aogen.dirs(nd)), dev(gathergen.weights(nd))
        ap = aogen.params(R, name, k, 1)
        job(2, "ao", lambda s, p: ctx.ao_device(d_hits, len(h), ap, d_dirs, nd, p, stream=s),
            aogen.want(name, k, nd, 1))
        mh = mattegen.hits(name)
        d_mh = dev(mh)
        job(2, "matte", lambda s, p, q: ctx.matte_device(d_mh, len(mh), p, q, stream=s),
            *mattegen.want(name))
        gp = gathergen.params(R, name, k, gathergen.JITTER | gathergen.SKIP)
        sums, skipped = gathergen.want(name, k, nd, gathergen.JITTER | gathergen.SKIP)
        job(2, "gather", lambda s, p, q: ctx.gather_device(d_hits, len(h), gp, d_dirs, d_w, nd, p,
                                                           skipped_ptr=q, stack_size=6, stream=s),
            sums, skipped)
        # stream 3
        W, H, kind = 33, 17, "rgb"
        d_guides, d_src = dev(filtergen.guides(name, W, H)), dev(filtergen.signal(name, W, H, kind))
        fst = filtergen.SETS[2]
        fp = filtergen.params(R, name, kind, fst)
        nbytes = R.filter_scratch(W, H, fp)
        scratch = torch.full((nbytes // 4 + PAD,), FILL, dtype=torch.int32, device="cuda")
        job(3, "filter", lambda s, p: ctx.filter_device(d_guides, W, H, fp, d_src, p,
                                                        scratch.data_ptr(), nbytes, stream=s),
            filtergen.want(name, W, H, kind, fst))
        ast, pk = accumgen.SETS[0], "pan"
        assert ast[4] and not ast[5]  # with M2, not a reset frame
        prev, held = _dev_prev(torch, accumgen.prev(name, W, H, pk, kind, ast))
        keep.append(held)
        acp = accumgen.params(R, name, kind, ast)
        job(3, "accumulate",
            lambda s, p, q, m: ctx.accumulate_device(d_guides, W, H, acp, d_src, p, q, prev,
                                                     zoom=accumgen.ZOOM, out_m2_ptr=m, stream=s),
            *accumgen.want(name, W, H, kind, pk, ast))
        render(3, 64, 36)
        render(3, 48, 27)

        for rnd in range(2):  # the second round finds every slot and entry in use
            for j in jobs:
                for d in j.dst:
                    d.fill_(0x5A)
            torch.cuda.synchronize()
            for j in jobs:
                j.launch(streams[j.stream])
            torch.cuda.synchronize()
            for j in jobs:
                j.check()
            assert (scratch.cpu().numpy()[nbytes // 4:] == FILL).all(), "past the filter's scratch"
    finally:
        ctx.close()
