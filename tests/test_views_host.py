"""CPU tests of many posed views in one call (rtg_render_views_host,
rtg_camera_cube; csrc/rtg_camera.hip): a table of poses, one frame each.

  1. view v of a batch, walk 0 and walk 1, is rtg_render_camera_host(walk 0)'s
     frame of pose v, bit for bit: the five poses of test_camera_host.POSES as
     one batch on four scenes, in 9 x 9 frames (four 8 x 8 tiles on the device,
     three of them ragged) and once in the 48 x 36 frame;
  2. rtg_camera_cube equals a numpy float32 restatement of rtg.h's table and
     arithmetic word for word, every sample direction of a face points through
     that face, and the faces' directions are distinct wherever the geometry
     lets them be;
  3. no views, one view;
  4. the argument errors of the contract, host and one-shot form, with no GPU
     call (this tier has no GPU).

All comparisons are bit for bit.  test_gpu_views.py shares the batches of this
file.
"""
from __future__ import annotations

import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

from conftest import first_mismatch
from test_camera_host import POSES, PH, PW, cam12, pose, posed_frame, restate_look_at
from test_raytrace_host import THREADS, scene_with_lights

F = np.float32

VIEW_SCENES = ["reference", 12, 200, "c5"]
VZOOM = -4.0       # the zoom every view of a batch shares
VW = VH = 9        # four tiles, three of them ragged
VAA, VS = 2.5, 6


def shared_zoom_pose(name, scene, zoom=VZOOM):
    """pose(name, scene) for a batch whose views share `zoom`: the poses come
    with zooms of their own (-4, -12, -96), and only zoom * back enters the
    ray, so `back` takes the factor (rounded to float32 once; what a view must
    equal is the single-view call on this same pose, whatever it is)."""
    cam, z = pose(name, scene)
    cam = np.array(cam, F)
    cam[3] = cam[3] * F(z / zoom)
    return cam


def batch_poses(scene):
    """The five poses of POSES as one (5, 12) float32 table."""
    return np.stack([shared_zoom_pose(p, scene).reshape(12) for p in POSES])


@functools.lru_cache(maxsize=None)
def view_frames(scene, sem=0, W=VW, H=VH, aa=VAA, S=VS, extra=()):
    """render_camera_host(walk 0) of each pose of batch_poses(scene), then of
    each 12-tuple of `extra`, one call per view: (n, H, W, 3), computed once
    and left unchanged."""
    import rtg_amd as R
    sph, lg = scene_with_lights(scene)
    cams = list(batch_poses(scene)) + [np.array(e, F) for e in extra]
    out = np.stack([R.render_camera_host(sph, lg, c, W, H, VZOOM, aa, S, semantics=sem, walk=0,
                                         threads=THREADS) for c in cams])
    out.setflags(write=False)
    return out


def lit(fb):
    return float((fb != 0).any(-1).mean())


# ---- 1. view by view ----

@pytest.mark.parametrize("scene", VIEW_SCENES)
def test_views_equal_single_view_calls(rtg, scene):
    sph, lg = scene_with_lights(scene)
    cams = batch_poses(scene)
    for sem in (0, 1):
        want = view_frames(scene, sem)
        for walk in (0, 1):
            for threads in (1, THREADS):  # bands that cut views anywhere
                got = rtg.render_views_host(sph, lg, cams, VW, VH, VZOOM, VAA, VS, semantics=sem,
                                            walk=walk, threads=threads)
                assert got.shape == (5, VH, VW, 3) and got.dtype == F
                for v in range(5):
                    assert got[v].tobytes() == want[v].tobytes(), (
                        sem, walk, threads, POSES[v], first_mismatch(got[v], want[v]))
    # the conditions: the batch is lit, and its views are not one frame five times
    want = view_frames(scene)
    assert lit(want) >= 0.10, lit(want)
    assert len({want[v].tobytes() for v in range(5)}) == 5


def test_views_in_the_posed_frame(rtg):
    """48 x 36 on the reference's scene: the batch at the shared zoom, and each
    pose alone at its own zoom against test_camera_host's frame of it."""
    scene = "reference"
    sph, lg = scene_with_lights(scene)
    want = view_frames(scene, 0, PW, PH, 2.0, 6)
    for walk in (0, 1):
        got = rtg.render_views_host(sph, lg, batch_poses(scene), PW, PH, VZOOM, 2.0, 6, walk=walk,
                                    threads=THREADS)
        assert got.tobytes() == want.tobytes(), (walk, first_mismatch(got, want))
    assert lit(want) >= 0.10
    for name in POSES:
        cam, zoom = pose(name, scene)
        got = rtg.render_views_host(sph, lg, [cam.reshape(12)], PW, PH, zoom, 2.0, 6,
                                    threads=THREADS)
        assert got[0].tobytes() == posed_frame(scene, name).tobytes(), name


# ---- 2. the cube map's poses ----

# rtg.h's table: face, forward F, right R, up U
CUBE = [((1, 0, 0), (0, 0, 1), (0, 1, 0)),
        ((-1, 0, 0), (0, 0, -1), (0, 1, 0)),
        ((0, 1, 0), (-1, 0, 0), (0, 0, -1)),
        ((0, -1, 0), (-1, 0, 0), (0, 0, 1)),
        ((0, 0, 1), (-1, 0, 0), (0, 1, 0)),
        ((0, 0, -1), (1, 0, 0), (0, 1, 0))]


def restate_cube(eye):
    """{eye, R * (3/32), U * (float)(1/6), -F} per face in float32, a zero
    component +0: (6, 4, 3) float32."""
    out = np.zeros((6, 4, 3), F)
    for f, (fw, r, u) in enumerate(CUBE):
        out[f, 0] = np.asarray(eye, F)
        out[f, 1] = np.array(r, np.int32).astype(F) * (F(3) / F(32))
        out[f, 2] = np.array(u, np.int32).astype(F) * F(1.0 / 6.0)
        out[f, 3] = (-np.array(fw, np.int32)).astype(F)
    return out


@pytest.mark.parametrize("eye", [(0, 0, 0), (1.5, -2.25, 1e-3), (np.nan, np.inf, -0.0)])
def test_camera_cube_equals_the_restatement(rtg, eye):
    got = rtg.camera_cube(eye)
    assert got.dtype == rtg.CAMERA_DTYPE and got.shape == (6,)
    want = restate_cube(eye)
    g = got.view(F).reshape(6, 4, 3)
    assert g.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (g, want)
    for f, (fw, r, u) in enumerate(CUBE):  # right-handed: R x U = -F, as the identity pose's
        assert tuple(np.cross(r, u)) == tuple(-np.array(fw)), f
    # face 5 is the identity pose's basis, scaled; 3/32 is exact
    assert float(F(3) / F(32)) == 3 / 32
    assert g[5, 1:].tolist() == [[3 / 32, 0, 0], [0, float(F(1.0 / 6.0)), 0], [0, 0, 1]]


def test_camera_cube_faces_point_through_their_faces(rtg):
    """A 4 x 4 face at zoom -1, aa 1: sample (0, 0) of every pixel.  The
    face's own axis holds a largest-magnitude component of every direction,
    with the face's sign (a tie on the top and left edges, which the face
    holds: the sample grid starts at the pixel's corner).  Over the six faces
    the 96 directions are pairwise distinct except where two faces hold one
    edge of the cube: +Y's top row and left column (7 pixels) are directions
    that the side faces' top rows have too, by the exact geometry of rtg.h's
    table; nothing else may coincide."""
    cube = rtg.camera_cube((0.25, -1.0, 3.0))
    dirs = []
    for f, (fw, r, u) in enumerate(CUBE):
        rays = rtg.camera_rays_host(cube[f], 4, 4, -1.0, 1.0)
        assert rays.shape == (16, 6) and (rays[:, :3] == np.array([0.25, -1.0, 3.0], F)).all()
        axis = int(np.flatnonzero(fw)[0])
        d = rays[:, 3:]
        assert np.isfinite(d).all()
        assert (np.abs(d[:, axis]) == np.abs(d).max(axis=1)).all(), (f, d)
        assert (np.sign(d[:, axis]) == fw[axis]).all(), (f, d)
        dirs.append(d)
    # the same 96 points of the unit cube in exact arithmetic: pixel (x, y) of a
    # 4 x 4 face is at rx = -1 + x / 2 along R and ry = 1 - y / 2 along U
    exact = [tuple(Fraction(fw[q]) + Fraction(x - 2, 2) * r[q] + Fraction(2 - y, 2) * u[q]
                   for q in range(3))
             for fw, r, u in CUBE for y in range(4) for x in range(4)]
    got = [d.tobytes() for face in dirs for d in face]
    same_exact = {(a, b) for a in range(96) for b in range(a) if exact[a] == exact[b]}
    same_got = {(a, b) for a in range(96) for b in range(a) if got[a] == got[b]}
    # (1/6 is rounded and 3/32 is not, so one point of an edge reached through
    # two faces may differ in its last bits: float coincidences are some of
    # the exact ones, never others, and the exact ones agree to rounding)
    assert same_got <= same_exact and same_got
    flat = np.concatenate(dirs)
    for a, b in same_exact:
        assert np.allclose(flat[a], flat[b], rtol=0, atol=4 * 2.0 ** -24), (a, b)
        v = a if a // 16 == 2 else b  # +Y's pixel of the pair: its top row or left column
        assert v // 16 == 2 and (a // 16 == 2) != (b // 16 == 2)
        assert v % 16 < 4 or v % 4 == 0
    assert len(same_exact) == 7 and len(set(exact)) == 89


def test_camera_cube_errors(rtg):
    L = rtg.lib()
    eye = np.zeros(3, F)
    out = np.full((6, 12), 7.0, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for args in ((None, P(out)), (P(eye), None)):
        assert L.rtg_camera_cube(*args) == -1 and b"null pointer" in L.rtg_last_error()
    assert (out == 7.0).all()


# ---- 3. no views, one view ----

def test_no_views_and_one_view(rtg):
    L = rtg.lib()
    sph, lg = scene_with_lights("reference")
    out = np.full((2, VH, VW, 3), 7.0, F)
    f = ctypes.c_float
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    cams = batch_poses("reference")
    for table in (P(cams), None):  # no views need no table
        for walk in (0, 1):
            rc = L.rtg_render_views_host(P(sph), len(sph), P(lg), len(lg), table, 0, VW, VH,
                                         f(VZOOM), f(VAA), VS, 0, P(out), walk, 4)
            assert rc == 0 and L.rtg_last_error() == b""
    assert (out == 7.0).all()
    assert rtg.render_views_host(sph, lg, np.zeros((0, 12), F), VW, VH).shape == (0, VH, VW, 3)
    want = view_frames("reference")
    for v in (0, 4):
        got = rtg.render_views_host(sph, lg, cams[v:v + 1], VW, VH, VZOOM, VAA, VS,
                                    threads=THREADS)
        assert got.shape == (1, VH, VW, 3) and got[0].tobytes() == want[v].tobytes()
    # records and rows of 12 floats are the same table
    rec = cams.view(rtg.CAMERA_DTYPE).reshape(-1)
    assert rtg.render_views_host(sph, lg, rec, VW, VH, VZOOM, VAA, VS).tobytes() == want.tobytes()


def test_a_nan_view_spoils_its_own_frame_only(rtg):
    sph, lg = scene_with_lights(12)
    c = restate_look_at((1, 2, 3), (1, 2, 3))  # eye == target: a NaN basis
    assert np.isnan(c).any()
    cams = batch_poses(12)
    table = np.concatenate([cams[:2], c.reshape(1, 12), cams[2:]])
    got = rtg.render_views_host(sph, lg, table, VW, VH, VZOOM, VAA, VS, walk=1, threads=THREADS)
    want = view_frames(12, extra=(tuple(c.reshape(12).tolist()),))
    assert got[2].tobytes() == want[5].tobytes()
    assert np.concatenate([got[:2], got[3:]]).tobytes() == want[:5].tobytes()


# ---- 4. argument errors ----

def test_argument_errors(rtg):
    L = rtg.lib()
    sph, lg = scene_with_lights("reference")
    cams = batch_poses("reference")
    out = np.full((5, 4, 4, 3), 7.0, F)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    f = ctypes.c_float

    def host(spheres=P(sph), n_sph=len(sph), lights=P(lg), n_lg=len(lg), c=P(cams), n=5, W=4, H=4,
             zoom=-4.0, aa=3.0, S=6, sem=0, dst=P(out), walk=0, threads=1):
        rc = L.rtg_render_views_host(spheres, n_sph, lights, n_lg, c, n, W, H, f(zoom), f(aa), S,
                                     sem, dst, walk, threads)
        return rc, L.rtg_last_error().decode()

    def one_shot(spheres=P(sph), n_sph=len(sph), lights=P(lg), n_lg=len(lg), c=P(cams), n=5, W=4,
                 H=4, zoom=-4.0, aa=3.0, S=6, dst=P(out), **_):
        rc = L.rtg_render_views(0, spheres, n_sph, lights, n_lg, c, n, W, H, f(zoom), f(aa), S,
                                dst)
        return rc, L.rtg_last_error().decode()

    shared = ((dict(c=None), "null pose table"),
              (dict(dst=None), "null destination"),
              (dict(spheres=None), "null scene array"),
              (dict(lights=None), "null scene array"),
              (dict(W=0), "empty frame"),
              (dict(H=0), "empty frame"),
              (dict(aa=257.0), "aliasFactor"),
              (dict(aa=float("nan")), "aliasFactor"),
              (dict(S=0), "stackSize 0 outside"),
              (dict(S=17), "stackSize 17 outside"),
              (dict(n=0, S=0), "stackSize 0 outside"),   # no views, and still an argument
              (dict(n=0, W=0), "empty frame"),
              (dict(n=0, dst=None), "null destination"),
              # 2^20 views of 4096 x 4096: 2^38 tiles
              (dict(n=1 << 20, W=4096, H=4096), "2^31-1 workgroups"),
              (dict(n=(1 << 31) - 1, W=9, H=8), "2^31-1 workgroups"),
              (dict(n=1 << 31, W=1, H=1), "2^31-1 workgroups"))
    for call in (host, one_shot):
        for kw, msg in shared:
            rc, err = call(**kw)
            assert rc == -1 and msg in err, (call.__name__, kw, rc, err)  # RTG_ERR_INVALID
    for kw, msg in ((dict(sem=2), "semantics 2"), (dict(sem=-1), "semantics -1"),
                    (dict(walk=2), "walk 2"), (dict(walk=-1), "walk -1")):
        rc, err = host(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert (out == 7.0).all()  # nothing was written, on either form
    rc, err = one_shot(n=0, c=None)  # no views: nothing to upload, launch or download
    assert rc == 0 and err == "" and (out == 7.0).all()
    with pytest.raises(rtg.RtgError, match="walk 5"):
        rtg.render_views_host(sph, lg, cams, 4, 4, walk=5)
    rc, err = host(n_sph=0, spheres=None, n_lg=0, lights=None)  # an empty scene is a scene
    assert rc == 0 and err == "" and (out == 0).all()
