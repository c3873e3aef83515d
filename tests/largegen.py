"""Helpers of the large-size tests (test_gpu_large.py, test_large_host.py):
legal device calls whose buffers pass 4 GiB.

  windows     the element ranges of a large buffer that are pulled back to the
              host: its start, the elements around byte 2^32 and around word
              (4-byte) index 2^31, and its end
  cuts        sub-batches of a batch, every buffer of each below 2^32 bytes,
              one boundary away from a multiple of 64 elements
  SHAPES      the shapes test_gpu_large.py runs and the thresholds each is
              there to cross (test_large_host.py checks the claims)

and, for the GPU module only (torch is imported where it is used): guarded
destinations, comparisons of whole buffers on the device in slices, and copies
of windows to the host.
"""
from __future__ import annotations

import contextlib
import gc

import numpy as np

WINDOW = 4096
BYTE_LIMIT = 1 << 32  # the first byte offset 32 bits cannot hold
WORD_LIMIT = 1 << 31  # the first 4-byte word index a signed 32-bit int cannot hold
PAD = 64  # elements the destinations are longer than the batch
GUARD = 0x5A5A5A5A
GIB = 1 << 30


def windows(n, stride_bytes):
    """Sorted, disjoint [lo, hi) element ranges of a buffer of n elements of
    stride_bytes each: the first WINDOW elements, the WINDOW elements that
    straddle byte offset 2^32 and those that straddle word index 2^31 (byte
    2^33) where the buffer reaches them, and the last WINDOW elements."""
    assert n > 0 and stride_bytes > 0
    want = [(0, WINDOW), (n - WINDOW, n)]
    for limit in (BYTE_LIMIT, 4 * WORD_LIMIT):
        if n * stride_bytes > limit:
            e = limit // stride_bytes  # the element that holds that byte
            want.append((e - WINDOW // 2, e + WINDOW // 2))
    out = []
    for lo, hi in sorted((max(lo, 0), min(hi, n)) for lo, hi in want):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def windows_of(n, strides):
    """The union of windows(n, s) over the strides of every buffer of a call."""
    out = []
    for lo, hi in sorted(w for s in strides for w in windows(n, s)):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def cuts(n, stride_bytes, least=2):
    """Boundaries 0 = b0 < b1 < ... < bk = n of at least `least` sub-batches,
    each below 2^32 bytes at stride_bytes (the widest buffer of the call) per
    element; b1 is no multiple of 64."""
    most = (BYTE_LIMIT - 1) // stride_bytes  # elements a sub-batch may hold
    k = max(least, -(-n // (most - 64)))
    b = [i * n // k for i in range(k + 1)]
    b[1] = b[1] - b[1] % 64 + 37
    assert all(0 < hi - lo <= most for lo, hi in zip(b, b[1:])), (n, stride_bytes, b)
    return b


def threshold_rows(W, H, stride_bytes):
    """The rows of a W x H frame of stride_bytes per pixel that hold pixel 0,
    the pixel at byte 2^32 with the rows above and below it, the pixel at word
    2^31, and the last pixel."""
    rows = {0, H - 1}
    if W * H * stride_bytes > BYTE_LIMIT:
        r = BYTE_LIMIT // stride_bytes // W
        rows.update((r - 1, r, r + 1))
    if W * H * stride_bytes > 4 * WORD_LIMIT:
        rows.add(4 * WORD_LIMIT // stride_bytes // W)
    return np.array(sorted(r for r in rows if 0 <= r < H), np.uint32)


# ---- the shapes and what each crosses -------------------------------------
# name: (elements, bytes per element of the widest buffer, crosses byte 2^32,
#        crosses word 2^31)
RAYS_W, RAYS_H = 16384, 21846
N_RAYS = RAYS_W * RAYS_H  # 357 924 864
N_POINTS = 134_217_792  # hit records: 4.29 GB
N_PROBE_POINTS, PROBE_K = 4_194_368, 64
N_ORDER = 178_957_056
RENDER_W = 32771
FILTER_W = 16387
VIEWS, VIEW_W = 7, 8192

SHAPES = {
    "render_c3_aa1": (RENDER_W * 21845, 12, True, True),
    "render_c3_aa3": (RENDER_W * 10923, 12, True, False),
    "render_c5_aa1": (RENDER_W * 10923, 12, True, False),
    "gbuffer_c3": (RENDER_W * 4097, 32, True, False),
    "render_camera_c3": (RENDER_W * 10923, 12, True, False),
    "camera_rays": (N_RAYS, 24, True, True),
    "intersect": (N_RAYS, 32, True, True),
    "visible": (N_RAYS, 24, True, True),
    "raytrace": (N_RAYS, 24, True, True),
    "raytrace_colours": (N_RAYS, 12, True, False),
    "camera_project": (N_RAYS, 12, True, False),
    "hit_points": (N_POINTS, 32, True, False),
    "probes": (N_PROBE_POINTS * PROBE_K, 24, True, False),
    "ray_order": (N_ORDER, 24, True, False),
    "filter_hits": (FILTER_W * 8192, 32, True, False),
    "filter_rgb": (FILTER_W * 21846, 12, True, False),
    "views": (VIEWS * VIEW_W * VIEW_W, 12, True, False),
}


# ---- rays of a pose at chosen pixels (aa 1) --------------------------------
F = np.float32


def rays_at(cam, W, H, zoom, pix):
    """The aa = 1 sample rays of pixels `pix` (indices y * W + x) of a pose:
    test_camera_host.restate_rays' float32 arithmetic at those pixels only
    (test_large_host.py pins the two to each other).  (len(pix), 6) float32."""
    cam = np.asarray(cam, F).reshape(4, 3)
    pix = np.asarray(pix, np.int64)
    y, x = pix // W, pix % W
    zoom = F(zoom)
    xs, ys, asp = F(16) / F(W), F(12) / F(H), F(16) / F(12)
    st = xs / F(1)
    halfW, halfH = F(W) * F(0.5), F(H) * F(0.5)
    zero = np.zeros(len(pix), F)
    with np.errstate(all="ignore"):
        rx = ((x.astype(F) - halfW) * xs + zero * st) * asp
        ry = (halfH - y.astype(F)) * ys + zero * st
        eye, right, up, back = cam
        v = [(rx * right[q] + ry * up[q]) + zoom * back[q] for q in range(3)]
        l = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    out = np.zeros((len(pix), 6), F)
    out[:, :3] = eye
    for q in range(3):
        out[:, 3 + q] = l * v[q]
    return out


# ---- device side (torch) ----------------------------------------------------
def _guard_of(torch, dtype):
    return {torch.uint8: 0x5A, torch.int16: 0x5A5A, torch.int32: GUARD,
            torch.int64: 0x5A5A5A5A5A5A5A5A}[dtype]


class Dest:
    """A device destination of n elements of `items` values of `dtype` (int32
    for float and record outputs), pre-filled with 0x5A bytes and PAD elements
    longer than needed."""

    def __init__(self, torch, n, items, dtype=None, canon=False):
        self.torch, self.n, self.items = torch, n, items
        self.dtype = dtype or torch.int32
        self.canon = canon  # float words: NaNs compared by position
        self.guard = _guard_of(torch, self.dtype)
        self.t = torch.full(((n + PAD) * items,), self.guard, dtype=self.dtype, device="cuda")
        self.stride = items * self.t.element_size()

    def ptr(self, first=0):
        return self.t.data_ptr() + first * self.stride

    def refill(self):
        self.t.fill_(self.guard)

    def values(self, lo, hi):
        return self.t[lo * self.items:hi * self.items]

    def tail_kept(self, n=None):
        """Whether the PAD elements after element n (default: the whole
        destination's n) still hold the fill."""
        n = self.n if n is None else n
        return bool((self.values(n, n + PAD) == self.guard).all())

    def host(self, lo, hi):
        return self.values(lo, hi).cpu().numpy().reshape(hi - lo, self.items)


SLICE = 1 << 26  # values compared at a time


def _canon(x):
    """int32 float words with every NaN as 0xFFC00000 (conftest.canon)."""
    nan = (x & 0x7FFFFFFF) > 0x7F800000
    return x.masked_fill(nan, 0xFFC00000 - (1 << 32))


def first_difference(torch, a, b, canon=False):
    """None if the 1-D device tensors hold the same values (float words with
    NaNs by position when canon), else (index, a's value, b's value) of the
    first difference; compared SLICE values at a time."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape)
    for lo in range(0, a.numel(), SLICE):
        x, y = a[lo:lo + SLICE], b[lo:lo + SLICE]
        if torch.equal(x, y):
            continue
        if canon:
            x, y = _canon(x), _canon(y)
            if torch.equal(x, y):
                continue
        k = int((x != y).nonzero()[0])
        return lo + k, int(x[k]), int(y[k])
    return None


def to_host(t, ranges, items):
    """The element ranges of a 1-D device tensor, concatenated on the host as
    (elements, items)."""
    return np.concatenate([t[lo * items:hi * items].cpu().numpy().reshape(hi - lo, items)
                           for lo, hi in ranges])


def canon_words(a):
    """Host float data as uint32 words with every NaN as 0xFFC00000."""
    a = np.ascontiguousarray(a)
    f = a.view(np.float32)
    w = a.view(np.uint32).copy()
    w[np.isnan(f)] = 0xFFC00000
    return w


@contextlib.contextmanager
def device_memory(torch, need_bytes, what):
    """The module's one skip: less device memory free than the test's need plus
    2 GiB.  On the way out the cache is emptied and the peak printed."""
    import pytest
    assert need_bytes <= 32 * GIB, (what, need_bytes)
    free, _ = torch.cuda.mem_get_info()
    if free < need_bytes + 2 * GIB:
        pytest.skip(f"needs {need_bytes / GIB:.1f} GiB of device memory, {free / GIB:.1f} free")
    torch.cuda.reset_peak_memory_stats()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        gc.collect()
        torch.cuda.empty_cache()
        print(f"{what}: peak device memory {peak / GIB:.2f} GiB (declared need "
              f"{need_bytes / GIB:.2f} GiB)")
