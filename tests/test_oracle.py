"""CPU tests: the oracle (C restatement of raytracer.h) is pinned against the
reference's own output, and the kernel's restructured traversal (compiled for
the host, tests/hostsim) is checked bit for bit against the oracle.

Pinning sources, strongest first:
  * oracle/_ref/librtgref_S*.so — the reference compiled from /root/reference
    (present only in the build container; those tests skip elsewhere);
  * tests/golden/ — fixtures the reference produced (tests/golden/make_golden.py),
    including SURVEY.md §8c's known answers for the main.cpp scene.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import (ASAN, ASAN_BUILD, BUILD, GOLDEN, P, ROOT, bits_equal, canon_md5, first_mismatch,
                      load_f32, load_scene, md5, random_scene)

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
HAVE_REF = all(os.path.exists(os.path.join(REF_DIR, f"librtgref_S{s}.so")) for s in range(1, 10))

# SURVEY.md §8c known answers (recorded during the survey, before this build).
SURVEY_KNOWN = {
    "ref800": ("96b20332f1c1fdf97efec7da14a0d920", "77a498a83918ef392d1f080532d1f4dc"),
    "c1": ("de44ee1fbd894f8c734db17a8878ad08", "53f45653f638bf19d6d66c5775e85807"),
}


def test_survey_known_answers_in_golden(golden):
    for name, (fb, ppm) in SURVEY_KNOWN.items():
        assert golden["configs"][name]["fb_md5_raw"] == fb
        assert golden["configs"][name]["fb_md5"] == fb  # all NaNs already 0xFFC00000
        assert golden["configs"][name]["ppm_md5"] == ppm
    assert golden["configs"]["ref800"]["nan_values"] > 0  # TIR NaNs are exercised


@pytest.mark.parametrize("name", ["ref800", "c1", "c2", "c3", "c4", "c5"])
def test_oracle_small_frames(oracle, golden, name):
    c = golden["configs"][name]
    sph, lg = load_scene(name, c["spheres"], c["lights"])
    sw, sh = c["small"]["W"], c["small"]["H"]
    want = load_f32(os.path.join(GOLDEN, f"{name}.small.f32"), (sh, sw, 3))
    got = oracle.render(sph, lg, sw, sh, c["stack_size"])
    assert bits_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("name", ["ref800", "c1"])
def test_oracle_full_frame_md5(oracle, golden, rtg, name):
    c = golden["configs"][name]
    sph, lg = load_scene(name, c["spheres"], c["lights"])
    fb = oracle.render(sph, lg, c["W"], c["H"], c["stack_size"])
    assert canon_md5(fb) == c["fb_md5"]
    assert oracle.counters[0] == c["ray_sphere_tests"]
    mx = oracle.max_colour(fb)
    assert np.float32(mx).view(np.uint32) == c["max_colour_bits"]
    ppm = b"P6\n%d %d\n255\n" % (c["W"], c["H"]) + oracle.ppm_bytes(fb, mx).tobytes()
    assert md5(ppm) == c["ppm_md5"]


def test_oracle_sampled_rows(oracle, golden):
    c = golden["configs"]["c2"]
    sph, lg = load_scene("c2", c["spheres"], c["lights"])
    rows = c["rows"]["rows"]
    want = load_f32(os.path.join(GOLDEN, "c2.rows.f32"), (len(rows), c["W"], 3))
    got = oracle.render(sph, lg, c["W"], c["H"], c["stack_size"], rows=rows)
    assert bits_equal(got, want), first_mismatch(got, want)


def _cases(golden):
    return [(k, c) for k, c in enumerate(golden["cases"])]


def test_oracle_edge_cases(oracle, golden):
    for c in golden["cases"]:
        sph, lg = load_scene(c["name"], c["spheres"], c["lights"])
        want = load_f32(os.path.join(GOLDEN, c["name"] + ".f32"), (c["H"], c["W"], 3))
        got = oracle.render(sph, lg, c["W"], c["H"], c["stack_size"], aa=c["aliasFactor"],
                            zoom=c["zoom"])
        assert bits_equal(got, want), (c["name"], first_mismatch(got, want))
        assert oracle.counters[0] == c["ray_sphere_tests"]


@pytest.mark.skipif(not HAVE_REF, reason="reference build (oracle/_ref) not present")
def test_oracle_vs_reference_random_scenes(oracle, rtg):
    rng = np.random.default_rng(7)
    for trial in range(30):
        S = int(rng.integers(1, 10))
        n, m = int(rng.integers(0, 14)), int(rng.integers(0, 5))
        W, H = int(rng.integers(1, 48)), int(rng.integers(1, 36))
        aa = float(rng.choice([1.0, 2.0, 3.0, 2.5, 4.0]))
        zoom = float(rng.choice([-4.0, -2.0, -7.0]))
        sph, lg = random_scene(rng, n, m)
        ref = ctypes.CDLL(os.path.join(REF_DIR, f"librtgref_S{S}.so"))
        assert ref.ref_stack_size() == S
        rows = np.arange(H, dtype=np.uint32)
        want = np.zeros((H, W, 3), np.float32)
        ref.ref_render_rows(P(sph), n, P(lg), m, W, H, ctypes.c_float(zoom), ctypes.c_float(aa),
                            P(rows), H, P(want), 4)
        got = oracle.render(sph, lg, W, H, S, aa=aa, zoom=zoom)
        assert bits_equal(got, want), (trial, S, n, m, W, H, first_mismatch(got, want))


@pytest.mark.skipif(not HAVE_REF, reason="reference build (oracle/_ref) not present")
def test_reference_struct_layout(rtg):
    ref = ctypes.CDLL(os.path.join(REF_DIR, "librtgref_S6.so"))
    sizes = [ref.ref_sizeof(i) for i in range(6)]
    assert sizes == [12, 36, 32, 48, 24, 76]
    assert rtg.SPHERE_DTYPE.itemsize == sizes[3] and rtg.LIGHT_DTYPE.itemsize == sizes[4]
    assert rtg.MATERIAL_DTYPE.itemsize == sizes[2]


# ------------------------------------------------------------------ hostsim
@pytest.fixture(scope="session")
def hostsim():
    """Host build of the kernel's traversal (rtg_trace.h), test-only."""
    if ASAN:  # tests/asan/Makefile build (tests/test_sanitizers.py)
        return ctypes.CDLL(os.path.join(ASAN_BUILD, "libhostsim.so"))
    os.makedirs(BUILD, exist_ok=True)
    # RTG_HOSTSIM_DEFS="-DRTG_X=1 ...": an A/B knob's host build, for the
    # parity tests of a trial before it is adopted (DESIGN item 37)
    defs = os.environ.get("RTG_HOSTSIM_DEFS", "").split()
    tag = "".join(c for c in "_".join(defs) if c.isalnum() or c == "_")
    so = os.path.join(BUILD, "libhostsim%s.so" % (("_" + tag) if tag else ""))
    src = os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")
    deps = [src, os.path.abspath(__file__)] + [
        os.path.join(ROOT, "raytracer-gamma_amd", "csrc", f) for f in
        ("rtg_trace.h", "rtg_scene_pack.h", "rtg_internal.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # built under a private name and renamed into place: parallel test
        # workers (pytest -n) may rebuild at once, and none may load a
        # half-written library
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.run(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
                        "-fPIC", "-shared", *defs, "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "raytracer-gamma_amd", "csrc"), src, "-o", tmp],
                       check=True)
        os.replace(tmp, so)
    return ctypes.CDLL(so)


@pytest.fixture(params=[0, 1, 2, 3, 4, 5, 8, 9, 15, 23],
                ids=["v0", "v1", "v2", "v3", "v4", "v5", "v8", "v9", "v15", "v23"])
def variant(request, hostsim):
    hostsim.hostsim_set_variant(request.param)
    yield request.param
    hostsim.hostsim_set_variant(0)


def _hostsim_render(hs, sph, lg, W, H, S, aa=3.0, zoom=-4.0, rows=None):
    rows = np.arange(H, dtype=np.uint32) if rows is None else np.asarray(rows, np.uint32)
    out = np.zeros((len(rows), W, 3), np.float32)
    rc = hs.hostsim_render_rows(P(sph), len(sph), P(lg), len(lg), W, H, ctypes.c_float(zoom),
                                ctypes.c_float(aa), S, P(rows), len(rows), P(out))
    assert rc == 0
    return out


@pytest.mark.parametrize("name", ["ref800", "c1", "c2", "c3", "c4", "c5"])
def test_kernel_traversal_small_frames(hostsim, variant, golden, name):
    c = golden["configs"][name]
    sph, lg = load_scene(name, c["spheres"], c["lights"])
    sw, sh = c["small"]["W"], c["small"]["H"]
    want = load_f32(os.path.join(GOLDEN, f"{name}.small.f32"), (sh, sw, 3))
    got = _hostsim_render(hostsim, sph, lg, sw, sh, c["stack_size"])
    assert bits_equal(got, want), first_mismatch(got, want)


def test_kernel_traversal_edge_cases(hostsim, variant, golden):
    for c in golden["cases"]:
        if c["stack_size"] > 12:
            continue  # hostsim instantiates S <= 12
        sph, lg = load_scene(c["name"], c["spheres"], c["lights"])
        want = load_f32(os.path.join(GOLDEN, c["name"] + ".f32"), (c["H"], c["W"], 3))
        got = _hostsim_render(hostsim, sph, lg, c["W"], c["H"], c["stack_size"],
                              aa=c["aliasFactor"], zoom=c["zoom"])
        assert bits_equal(got, want), (c["name"], first_mismatch(got, want))


def test_kernel_traversal_random_scenes(hostsim, variant, oracle, rtg):
    rng = np.random.default_rng(11)
    for trial in range(40):
        S = int(rng.integers(1, 13))
        n, m = int(rng.integers(0, 14)), int(rng.integers(0, 5))
        W, H = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        aa = float(rng.choice([1.0, 2.0, 3.0, 2.5]))
        zoom = float(rng.choice([-4.0, -2.0, -7.0, 3.0, 0.5]))
        sph, lg = random_scene(rng, n, m)
        if zoom > 0:  # put some spheres behind the camera plane's other side
            sph["pos"][:, 2] *= -1.0
        want = oracle.render(sph, lg, W, H, S, aa=aa, zoom=zoom)
        got = _hostsim_render(hostsim, sph, lg, W, H, S, aa=aa, zoom=zoom)
        assert bits_equal(got, want), (trial, S, n, m, W, H, first_mismatch(got, want))


def test_kernel_traversal_c1_full_frame(hostsim, variant, golden):
    """A whole BASELINE config frame through the kernel's traversal (md5)."""
    c = golden["configs"]["c1"]
    sph, lg = load_scene("c1", c["spheres"], c["lights"])
    got = _hostsim_render(hostsim, sph, lg, c["W"], c["H"], c["stack_size"])
    assert canon_md5(got) == c["fb_md5"]


@pytest.mark.parametrize("name", ["ref800", "c1", "c2", "c3", "c4", "c5"])
def test_primary_cull_is_conservative(hostsim, golden, name):
    """The primary cull (primary_bundle + primary_possible) never drops a sphere that a sample of the
    bundle hits (exact root test), over whole small frames of every config,
    for the sample kernel's 7-pixel groups and the tile kernel's rows."""
    c = golden["configs"][name]
    sph, lg = load_scene(name, c["spheres"], c["lights"])
    f = hostsim.hostsim_cull_violations
    f.restype = ctypes.c_long
    for W, H, group in [(96, 54, 7), (160, 90, 8), (64, 48, 1)]:
        culled = ctypes.c_long(0)
        bad = f(P(sph), len(sph), W, H, ctypes.c_float(-4.0), ctypes.c_float(3.0), group,
                ctypes.byref(culled))
        assert bad == 0, (name, W, H, group, bad)
        if len(sph) > 3:
            assert culled.value > 0  # the cull does drop spheres


def test_primary_cull_random_scenes(hostsim):
    rng = np.random.default_rng(4242)
    f = hostsim.hostsim_cull_violations
    f.restype = ctypes.c_long
    total_culled = 0
    for trial in range(30):
        n = int(rng.integers(1, 40))
        sph, _ = random_scene(rng, n, 0)
        zoom = float(rng.choice([-4.0, -2.0, -7.0, 3.0, 0.5]))
        if zoom > 0:
            sph["pos"][:, 2] *= -1.0
        aa = float(rng.choice([1.0, 2.0, 3.0, 4.0]))
        culled = ctypes.c_long(0)
        bad = f(P(sph), n, 48, 36, ctypes.c_float(zoom), ctypes.c_float(aa), 7,
                ctypes.byref(culled))
        assert bad == 0, (trial, n, zoom, aa, bad)
        total_culled += culled.value
    assert total_culled > 0


def test_pass1_screen_is_a_superset(hostsim):
    """The fused pass-1 screen (pass1_rad) keeps every sphere the reference's
    radicand test accepts, over 4M adversarial near-tangent ray/sphere pairs
    at scales 1e-3..1e3.  (At K = 2^-22 this test finds misses: the 2^-16
    slack is 64x the smallest that holds.)  Extras come from the draws within
    ~1e-5 of tangency, which is most of this adversarial set's near misses."""
    f = hostsim.hostsim_pass1_check
    f.restype = ctypes.c_long
    acc, ext = ctypes.c_long(0), ctypes.c_long(0)
    n = 4_000_000
    bad = f(ctypes.c_long(n), ctypes.c_ulonglong(12345), ctypes.byref(acc), ctypes.byref(ext))
    assert bad == 0, bad
    assert acc.value > n // 5
    assert ext.value < 0.3 * n, ext.value


def test_shadow_masks_are_conservative(hostsim):
    """A sphere left out of a shadow mask (shadow_masks, rtg_scene_pack.h) never
    blocks a shadow ray from a hit point inside the guard ball to the light,
    by the reference's own test (raytracer.h:272-309), over random scenes at
    scales 1e-2..1e2 with half of the spheres placed just outside the capsule
    reach (relative gaps 1e-4..3e-2) and a quarter just behind the hit
    sphere's plane facing the light (which the masks drop: a shadow ray is
    cast only from points with incidence > 0); the hit points include
    grazing ones.  Moving that plane forward by 2^-5 g (past the margin mu)
    finds blockers."""
    f = hostsim.hostsim_shadow_mask_check
    f.restype = ctypes.c_long
    hostsim.hostsim_capsule_back_slack.argtypes = [ctypes.c_double]
    tested = ctypes.c_long(0)
    bad = f(ctypes.c_long(600), 12, ctypes.c_long(60), ctypes.c_ulonglong(99),
            ctypes.byref(tested))
    assert bad == 0, bad
    assert tested.value > 1_000_000, tested.value
    try:
        hostsim.hostsim_capsule_back_slack(2.0 ** -5)
        assert f(ctypes.c_long(300), 12, ctypes.c_long(60), ctypes.c_ulonglong(98),
                 ctypes.byref(tested)) > 0  # the check has teeth
    finally:
        hostsim.hostsim_capsule_back_slack(0.0)


def test_cell_lists_are_conservative(hostsim):
    """A sphere left out of the capsule list of a hit-point cell (cap_cell,
    cell_ball, cell_keep, cell_behind: rtg_scene_pack.h, the BVH scenes'
    shadow lists) never blocks a shadow ray from a point the kernel puts in
    that cell, by the reference's own test: random scenes at scales
    1e-2..1e2, half of the spheres just outside one cell's capsule, points
    near the surface, at the shell's inner radius, at the cells' edges and
    toward the left-out spheres, incidence > 0.  Shrinking the cell balls by
    1/8 finds blockers."""
    f = hostsim.hostsim_cell_list_check
    f.restype = ctypes.c_long
    hostsim.hostsim_cell_ball_slack.argtypes = [ctypes.c_double]
    tested = ctypes.c_long(0)
    bad = f(ctypes.c_long(300), 12, ctypes.c_long(40), ctypes.c_ulonglong(7),
            ctypes.byref(tested))
    assert bad == 0, bad
    assert tested.value > 300_000, tested.value
    try:
        hostsim.hostsim_cell_ball_slack(0.125)
        assert f(ctypes.c_long(300), 12, ctypes.c_long(40), ctypes.c_ulonglong(8),
                 ctypes.byref(tested)) > 0  # the check has teeth
    finally:
        hostsim.hostsim_cell_ball_slack(0.0)


@pytest.mark.parametrize("name", ["c2", "c3", "c4"])
def test_shadow_masks_cull(hostsim, golden, name):
    """The masks of the benchmark scenes are small (the point of them)."""
    c = golden["configs"][name]
    sph, lg = load_scene(name, c["spheres"], c["lights"])
    f = hostsim.hostsim_shadow_mask_bits
    f.restype = ctypes.c_long
    bits = f(P(sph), len(sph), P(lg), len(lg))
    assert 0 < bits <= 0.3 * len(sph) * len(sph) * len(lg), bits


# ------------------------------------------------------------ OpenCL semantics
REF_GPU_PPM = os.path.join(GOLDEN, "ref800.gpu_ppm.npz")


def test_opencl_semantics_approach_the_reference_gpu_image(oracle, rtg):
    """The reference's committed testPPM.ppm was made by its OpenCL kernel on
    the author's GPU (relaxed division/sqrt, FP contraction), so no IEEE
    restatement reproduces it bit for bit.  The OpenCL-semantics oracle at the
    .cl's stack size 5 comes within 3,978 px (max 18 levels) of it, against
    25,726 px for the CPU path as shipped (S = 6) and 10,102 px for the CPU
    path at S = 5.  The image's 800x600x3 bytes are the fixture
    tests/golden/ref800.gpu_ppm.npz (`pixels`, compressed)."""
    W, H = 800, 600
    ref = np.load(REF_GPU_PPM)["pixels"].astype(int)
    assert ref.shape == (H, W, 3)
    sph, lg = rtg.reference_scene()

    def diff(fb):
        b = np.frombuffer(rtg.ppm_file_bytes(fb)[-W * H * 3:], np.uint8).reshape(H, W, 3)
        d = np.abs(b.astype(int) - ref).max(axis=2)
        return int((d > 0).sum()), int(d.max())

    assert diff(oracle.render_cl(sph, lg, W, H, 5)) == (3978, 18)
    assert diff(oracle.render(sph, lg, W, H, 6))[0] == 25726
    assert diff(oracle.render(sph, lg, W, H, 5))[0] == 10102


def test_kernel_traversal_opencl_semantics(hostsim, oracle, rtg, golden):
    """The kernel's traversal with kCL (variant 50 in the host build) equals
    the OpenCL-semantics oracle bit for bit."""
    hostsim.hostsim_set_variant(50)
    try:
        rng = np.random.default_rng(505)
        for trial in range(30):
            S = int(rng.integers(1, 13))
            n, m = int(rng.integers(0, 14)), int(rng.integers(0, 5))
            W, H = int(rng.integers(1, 40)), int(rng.integers(1, 30))
            aa = float(rng.choice([1.0, 2.0, 3.0, 2.5]))
            zoom = float(rng.choice([-4.0, -2.0, 3.0]))
            sph, lg = random_scene(rng, n, m)
            if zoom > 0:
                sph["pos"][:, 2] *= -1.0
            want = oracle.render_cl(sph, lg, W, H, S, aa=aa, zoom=zoom)
            got = _hostsim_render(hostsim, sph, lg, W, H, S, aa=aa, zoom=zoom)
            assert bits_equal(got, want), (trial, S, n, m, W, H, first_mismatch(got, want))
        sph, lg = rtg.reference_scene()
        want = oracle.render_cl(sph, lg, 96, 72, 5)
        assert not bits_equal(want, oracle.render(sph, lg, 96, 72, 5))  # the modes differ
        got = _hostsim_render(hostsim, sph, lg, 96, 72, 5)
        assert bits_equal(got, want), first_mismatch(got, want)
    finally:
        hostsim.hostsim_set_variant(0)


def test_overlap_masks_bound_containment(hostsim):
    """A sphere left out of overlap mask h never contains the refraction test
    point P + 0.01f D of a hit point P in h's guard ball with |D| <= 3, by
    the reference's own containment test (raytracer.h:255-264), over random
    scenes at scales 0.03..30 with half of the spheres placed just outside the
    reach (relative gaps 1e-5..1e-2), negative radii included."""
    f = hostsim.hostsim_contain_mask_check
    f.restype = ctypes.c_long
    tested = ctypes.c_long(0)
    bad = f(ctypes.c_long(300), 12, ctypes.c_long(80), ctypes.c_ulonglong(7),
            ctypes.byref(tested))
    assert bad == 0, bad
    assert tested.value > 200_000, tested.value


def test_bvh_bounds_are_conservative(hostsim):
    """BVH boxes (bvh_grow: half-width r + 2^-8 (|p| + r) + rounding terms)
    pass the kernel's slab test for every sphere the reference's root test
    accepts, within a closest query's reach t* and within the shadow ray's
    reach sqrt(gap / a) for the smallest gap that makes t* block; and the
    sphere slots' distance prune (beyond) never drops an accepted root, over
    3M adversarial near-tangent / far / on-surface ray-sphere pairs at scales
    1e-3..1e3 (rtg_trace.h closest_bvh / blocked_bvh).  The tiny-far-sphere
    cases (lines the reference accepts although they miss by up to ~7e-4 |p|)
    need a margin >= ~2^-10.5: at 2^-12 the same check finds misses."""
    f = hostsim.hostsim_bvh_bound_check
    f.restype = ctypes.c_long
    hostsim.hostsim_bound_margin.argtypes = [ctypes.c_double]

    def run(trials, seed):
        acc, bad_screen = ctypes.c_long(0), ctypes.c_long(0)
        bad = f(ctypes.c_long(trials), ctypes.c_ulonglong(seed), ctypes.byref(acc),
                ctypes.byref(bad_screen))
        return bad, bad_screen.value, acc.value

    bad, bad_screen, acc = run(3_000_000, 2026)
    assert bad == 0 and bad_screen == 0, (bad, bad_screen)
    assert acc > 500_000, acc
    try:
        hostsim.hostsim_bound_margin(2.0 ** -12)
        assert run(1_000_000, 2027)[1] > 0  # the check has teeth
    finally:
        hostsim.hostsim_bound_margin(0.0)


def test_kernel_traversal_bvh_random_scenes(hostsim, oracle):
    """Scenes above 64 spheres take the BVH queries (closest, shadow,
    container); random scenes of 65..400 spheres, small and large radii,
    overlapping clusters, bit-exact against the oracle."""
    rng = np.random.default_rng(65)
    hostsim.hostsim_set_variant(0)
    for trial in range(12):
        S = int(rng.integers(1, 9))
        n, m = int(rng.integers(65, 400)), int(rng.integers(0, 5))
        W, H = int(rng.integers(1, 24)), int(rng.integers(1, 18))
        aa = float(rng.choice([1.0, 2.0, 3.0]))
        zoom = float(rng.choice([-4.0, -2.0, 3.0]))
        sph, lg = random_scene(rng, n, m)
        if trial % 3 == 0:  # dense overlapping clusters
            sph["pos"] *= 0.3
        if zoom > 0:
            sph["pos"][:, 2] *= -1.0
        want = oracle.render(sph, lg, W, H, S, aa=aa, zoom=zoom)
        got = _hostsim_render(hostsim, sph, lg, W, H, S, aa=aa, zoom=zoom)
        assert bits_equal(got, want), (trial, S, n, m, W, H, first_mismatch(got, want))


def test_sphere_list_limits(hostsim, golden, rtg):
    """Sphere lists (sphere_lists, rtg_scene_pack.h) stay within their record
    budget, whose 32-byte records the kernel addresses with 32-bit byte
    offsets: a scene over the budget gets no lists at all (its queries take
    the BVH), and so does a scene whose list build would cost more than the
    threshold of capsule + overlap tests, without doing that work."""
    import time
    f = hostsim.hostsim_list_records
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint,
                  ctypes.c_ulonglong, ctypes.c_void_p]
    out = (ctypes.c_ulonglong * 3)()
    c = golden["configs"]["c5"]
    sph, lg = load_scene("c5", c["spheres"], c["lights"])
    f(P(sph), len(sph), P(lg), len(lg), 1 << 23, out)
    cap, ov, nodes = list(out)
    assert cap > 0 and ov > 0 and nodes > 0, list(out)
    # padding records: capsule tables 3 (16-byte records, four per scalar
    # load), overlap tables 1 (32-byte records, two per load)
    cpad, opad = 3, 1
    assert (cap + cpad) * 16 < 2 ** 32 and (ov + opad) * 32 < 2 ** 32
    budget = max(cap + cpad, ov + opad) - 1  # the larger table just over the budget: no lists
    f(P(sph), len(sph), P(lg), len(lg), budget, out)
    assert out[0] == 0 and out[1] == 0 and out[2] == nodes
    f(P(sph), len(sph), P(lg), len(lg), budget + 1, out)
    assert (out[0], out[1]) == (cap, ov)
    # (m + 1) n^2 > 2^28 tests: no lists, and no quadratic build
    rng = np.random.default_rng(8)
    big, lg4 = random_scene(rng, 9000, 4)
    big["radius"] *= 0.05
    t0 = time.time()
    f(P(big), len(big), P(lg4), len(lg4), 1 << 23, out)
    assert out[0] == 0 and out[1] == 0 and out[2] > 0
    assert time.time() - t0 < 20


def test_bvh_large_coordinates(hostsim, oracle):
    """The slab test multiplies by 1/d (up to 2^64 for a near-axis direction):
    scenes with coordinates up to 2^56 keep the BVH and stay bit-exact with
    axis-aligned rays (the frame's centre column and row); beyond that the
    scene has no BVH (flat queries, same answers)."""
    f = hostsim.hostsim_list_records
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint,
                  ctypes.c_ulonglong, ctypes.c_void_p]
    out = (ctypes.c_ulonglong * 3)()
    rng = np.random.default_rng(56)
    hostsim.hostsim_set_variant(0)
    for scale, has_bvh in ((2.0 ** 40, True), (2.0 ** 52, True), (2.0 ** 60, False)):
        sph, lg = random_scene(rng, 80, 2)
        sph["pos"] *= scale / 40.0
        sph["radius"] *= scale / 40.0
        lg["pos"] *= scale / 40.0
        f(P(sph), len(sph), P(lg), len(lg), 1 << 23, out)
        assert (out[2] > 0) == has_bvh, (scale, list(out))
        W, H = 9, 7  # odd: the centre column and row have d.x = 0 / d.y = 0 samples
        want = oracle.render(sph, lg, W, H, 4)
        got = _hostsim_render(hostsim, sph, lg, W, H, 4)
        assert bits_equal(got, want), (scale, first_mismatch(got, want))


def test_behind_is_exact(hostsim):
    """`behind` (rtg_trace.h: the sphere lies wholly behind the ray's origin,
    proven from the pass-1 screen's fused terms) never drops a sphere the
    reference's own float root test accepts, over 4M adversarial rays from
    just outside a sphere (gaps 1e-9 r .. 3 r), pointing away from it or
    grazing it, at scales 1e-3 .. 1e3 with unit and unnormalised directions;
    and the margins matter: dropping them (x > 0, |p|^2 - r^2 > 0 only)
    would drop accepted roots."""
    f = hostsim.hostsim_behind_check
    f.restype = ctypes.c_long
    rej, loose = ctypes.c_long(0), ctypes.c_long(0)
    bad = f(ctypes.c_long(4_000_000), ctypes.c_ulonglong(2024), ctypes.byref(rej),
            ctypes.byref(loose))
    assert bad == 0, bad
    assert rej.value > 1_000_000, rej.value
    assert loose.value > 0, loose.value


def test_cap_screen_r2_is_conservative(hostsim):
    """The device's screen radius^2 of a 16-byte capsule record
    (cap_screen_r2: fma(r2, C, 2^-149), rtg_trace.h) is never below the host's
    screen_r2, the bound pass1_rad's screen is proven with: every 61st
    non-negative binary32 value, both sides of every binade boundary, every
    7th subnormal, inf and NaN (NaN stays NaN)."""
    f = hostsim.hostsim_cap_screen_check
    f.restype = ctypes.c_long
    checked = ctypes.c_long(0)
    bad = f(ctypes.c_uint(61), ctypes.byref(checked))
    assert bad == 0, bad
    assert checked.value > 30_000_000, checked.value


def test_no_root_is_exact(hostsim):
    """`no_root` (rtg_trace.h: the reference's own b and cc show that no root
    can be accepted) never skips a root the reference's float test accepts,
    over 4M rays from on / just inside / just outside a sphere's surface
    leaving it at angles down to grazing (the shadow ray of a hit point
    against its own sphere), scales 1e-3 .. 1e2, unit and unnormalised
    directions; the set includes accepted self-hits (grazing acne)."""
    f = hostsim.hostsim_no_root_check
    f.restype = ctypes.c_long
    sk, acc = ctypes.c_long(0), ctypes.c_long(0)
    bad = f(ctypes.c_long(4_000_000), ctypes.c_ulonglong(77), ctypes.byref(sk), ctypes.byref(acc))
    assert bad == 0, bad
    assert sk.value > 1_000_000 and acc.value > 1000, (sk.value, acc.value)


def test_cone_masks_are_conservative(hostsim):
    """Secondary-ray cone masks (cone_masks, rtg_scene_pack.h): a sphere left
    out of mask (h, cell(U)) is never hit, by the reference's own root test,
    by a ray from h's origin ball whose direction is within kConeHalf of U:
    grazing rays aimed at that sphere's silhouette from the ball's boundary,
    with U at the edge of the bundle, over random scenes at scales 0.03..30."""
    f = hostsim.hostsim_cone_mask_check
    f.restype = ctypes.c_long
    tested = ctypes.c_long(0)
    bad = f(ctypes.c_long(300), 16, ctypes.c_long(4000), ctypes.c_ulonglong(31),
            ctypes.byref(tested))
    assert bad == 0, bad
    assert tested.value > 200_000, tested.value


def test_kernel_traversal_c5_wide_rows(hostsim, golden):
    """The kernel's BVH traversal (host build) on C5 (1024 spheres, depth 7)
    against the widened reference fixture: two centre-band rows, where most
    rays enter the sphere cluster, and the random pixels that fall in them."""
    c = golden["configs"]["c5"]
    z = np.load(os.path.join(GOLDEN, c["wide"]["file"]))
    rows = list(z["rows"])
    sph, lg = load_scene("c5", c["spheres"], c["lights"])
    hostsim.hostsim_set_variant(0)
    pick = [1080, 1084]
    got = _hostsim_render(hostsim, sph, lg, c["W"], c["H"], c["stack_size"], rows=pick)
    for k, r in enumerate(pick):
        want = z["rows_fb"][rows.index(r)]
        assert bits_equal(got[k], want), (r, first_mismatch(got[k], want))
    gids = z["gids"].astype(np.int64)
    sel = np.isin(gids // c["W"], pick)
    assert sel.sum() > 50
    flat = {r: got[k] for k, r in enumerate(pick)}
    px = np.stack([flat[g // c["W"]][g % c["W"]] for g in gids[sel]])
    assert bits_equal(px, z["pixels"][sel])


def test_unit_counts_fixture_matches_hostsim(hostsim, golden):
    """tests/golden/unit_counts.json (the per-lane unit counts the GPU test
    holds the device counting build to) is the current traversal's."""
    import json
    import sys
    sys.path.insert(0, GOLDEN)
    import make_unit_counts as muc
    want = json.load(open(os.path.join(GOLDEN, "unit_counts.json")))
    assert want["units"] == muc.UNITS
    assert muc.hostsim_counts(hostsim, golden) == want["frames"]
