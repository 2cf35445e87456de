"""CPU: the thin lens (ky_lens).  The restatement of the disk map (tests/lens_restatement.py) against what defines Shirley's concentric map;
the geometry of section 12's ray on the CPU oracle alone -- a pinhole at the lens point, through the shifted film point, meets the pinhole ray on the focus plane --
with the wrong-sign shift rejected; what kyhip_lens_check refuses; the rectangle a lens launch reads.  tests/test_lens_gpu.py holds the device against all this."""
import ctypes as C
import math

import numpy as np
import pytest

import lens_restatement as L

f32, f64 = np.float32, np.float64


# ---- the disk map ----

def grid_centres(n):
    c = (np.arange(n, dtype=f64) + 0.5) / n
    return np.stack(np.meshgrid(c, c, indexing="ij"), axis=-1).reshape(-1, 2).astype(f32)


def test_the_centre_of_the_square_is_the_centre_of_the_disk():
    for dtype in (f32, f64):
        assert np.array_equal(L.disk(np.array([[0.5, 0.5]], f32), dtype), np.zeros((1, 2), dtype))


def test_every_point_lies_in_the_unit_disk():
    gen = np.random.default_rng(20261021)
    one = f32(1) - f32(2.0 ** -24)
    edge = np.array([[0, 0], [0, one], [one, 0], [one, one], [0, 0.5], [0.5, 0], [one, 0.5], [0.5, one], [0.25, 0.25], [0.75, 0.25]], f32)
    u = np.concatenate([edge, gen.random((1 << 16, 2), dtype=f32)])
    for dtype in (f32, f64):
        d = L.disk(u, dtype)
        assert d.dtype == dtype and np.isfinite(d).all()
        assert (np.hypot(d[:, 0].astype(f64), d[:, 1].astype(f64)) <= 1.0 + 2.0 ** -22).all()
    # the float32 restatement is the double one to a few units in the last place of 1
    assert np.abs(L.disk(u, f32).astype(f64) - L.disk(u, f64)).max() <= 4 * 2.0 ** -24


def test_a_grid_of_cell_centres_fills_rings_and_sectors_equally():
    """64 x 64 cell centres, (a, b) = 2 u - 1 odd multiples of 1 / 64.  The map sends the square |(a, b)|_inf = R to the circle of radius R and keeps areas.
    Rings: 16 of equal area, r^2 in sixteenths.  The disk of radius R holds the (2 n)^2 centres with n = the odd m < 64 R, which IS its share of the 4096,
    (64 R)^2, wherever 64 R is an even whole number: at R = 1/4, 1/2, 3/4, 1, the outer edges of rings 0, 3, 8 and 15, the counts are 256 k exactly.  Between
    those edges 16 sqrt(k) is no whole number and a ring cannot hold exactly 256 centres (ring 1 holds 228): there the count asserted is the one the
    concentric squares give, 4 (n_{k+1}^2 - n_k^2), exactly.  No centre lies on an edge (odd^2 / 256 is no whole number).
    Sectors: 8 of 45 degrees, centred on the axes and the diagonals -- 512 centres each, exactly: the angle from a wedge's axis is (pi / 4) (short / long), so the
    sector around an axis holds the centres with short < long / 2, which sum to 512 over long = 1, 3 .. 63; no centre has short = long / 2 (long is odd).
    (Sectors that END on the diagonals have the 128 centres with |a| = |b| on their edges.)"""
    d = L.disk(grid_centres(64), f64)
    r2 = d[:, 0] ** 2 + d[:, 1] ** 2
    rings = np.bincount(np.minimum((r2 * 16).astype(int), 15), minlength=16)
    inside = np.cumsum(rings)
    assert [int(inside[k - 1]) for k in (1, 4, 9, 16)] == [256, 1024, 2304, 4096], inside
    n_odd = [int((16 * math.sqrt(k) + 1) // 2) for k in range(17)]   # the odd m below 16 sqrt(k)
    assert np.array_equal(rings, [4 * (n_odd[k + 1] ** 2 - n_odd[k] ** 2) for k in range(16)]), rings
    assert np.abs(rings - 256).max() <= 2 * 129   # |(2 n)^2 - (64 R)^2| <= 128 R + 1 at either edge: what a grid of this size can miss equal counts by
    ang = np.mod(np.arctan2(d[:, 1], d[:, 0]) + math.pi / 8, 2 * math.pi)
    sectors = np.bincount((ang / (math.pi / 4)).astype(int), minlength=8)
    assert np.array_equal(sectors, np.full(8, 512)), sectors


def test_the_map_is_continuous_across_the_diagonals():
    """On |a| = |b| both forms give r (cos pi / 4, sin pi / 4); a step of 2^-12 across a diagonal moves the point by no more than a step of that size anywhere
    else does (the map's Lipschitz constant is below 2 sqrt(2) pi / 4 * 2 < 5 in u)."""
    t = np.linspace(0.03, 0.97, 400).astype(f32)
    eps = f32(2.0 ** -12)
    for other in (t, (f32(1) - t).astype(f32)):   # the two diagonals
        below = np.stack([t, other - eps], axis=1)
        above = np.stack([t, other + eps], axis=1)
        on = np.stack([t, other], axis=1)
        for dtype in (f32, f64):
            lo, mid, hi = L.disk(below, dtype).astype(f64), L.disk(on, dtype).astype(f64), L.disk(above, dtype).astype(f64)
            assert np.abs(hi - lo).max() <= 5 * 2 * float(eps)
            assert np.abs(mid - lo).max() <= 5 * float(eps) and np.abs(hi - mid).max() <= 5 * float(eps)


# ---- the geometry, on the oracle alone ----

def lens_points():
    """64 points of the unit disk: 32 on the rim, 32 inside (the disk map of a 4 x 8 grid)."""
    ang = (np.arange(32, dtype=f64) + 0.25) * (2 * math.pi / 32)
    rim = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(f32)
    c0, c1 = (np.arange(4, dtype=f64) + 0.5) / 4, (np.arange(8, dtype=f64) + 0.5) / 8
    inside = L.disk(np.stack(np.meshgrid(c0, c1, indexing="ij"), axis=-1).reshape(-1, 2).astype(f32))
    return np.concatenate([rim, inside])


def at_depth(rays6, cam, depth):
    """where each ray {o[3], d[3]} crosses the plane at `depth` along the camera's front from the camera's position"""
    o, d = rays6[:, :3].astype(f64), rays6[:, 3:].astype(f64)
    front = cam.front.astype(f64) / np.linalg.norm(cam.front.astype(f64))
    t = (depth - (o - cam.position.astype(f64)) @ front) / (d @ front)
    return o + d * t[:, None]


def lens_rays(O, A, scene, cam, lc, film2, d2, sign=1.0):
    """[n_film, n_lens, 6]: kyo_kat_camera with the camera moved to each lens point, at the film point shifted as section 12 says"""
    out = np.zeros((film2.shape[0], d2.shape[0], 6), f32)
    moved = A.Camera.from_buffer_copy(scene.c.camera)
    for i, (px, py) in enumerate(film2):
        px2, py2, o = L.lens_ray(cam, lc, np.full(d2.shape[0], px, f32), np.full(d2.shape[0], py, f32), d2, sign)
        for j in range(d2.shape[0]):
            moved.position[0], moved.position[1], moved.position[2] = float(o[j, 0]), float(o[j, 1]), float(o[j, 2])
            out[i, j] = O.kat_camera(moved, np.array([[px2[j], py2[j]]], f32))[0]
    return out


def test_lens_rays_meet_the_pinhole_ray_on_the_focus_plane(O, A, api):
    w, h = 64, 48
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    cam = L.Camera(scene.c.camera)
    sphere = O.world_bounding_sphere(scene)
    radius = 0.02 * 2 * float(sphere[3])
    focus = float((sphere[:3].astype(f64) - cam.position.astype(f64)) @ cam.front.astype(f64))
    assert radius > 0 and focus > 0
    gen = np.random.default_rng(7)
    film2 = (gen.random((16, 2)) * [w, h]).astype(f32)
    film2[0], film2[1], film2[2] = (0, 0), (w, h), (w / 2, h / 2)
    d2 = lens_points()
    pin = O.kat_camera(scene.c.camera, film2)
    assert np.array_equal(pin[:, :3], np.tile(cam.position, (16, 1)))

    def misses(focus_of_lens, depth, sign=1.0):
        """|lens ray - pinhole ray| on the plane at `depth`, [16, 64], for a lens focused at focus_of_lens"""
        rays = lens_rays(O, A, scene, cam, L.lens_const(cam, radius, focus_of_lens), film2, d2, sign)
        want = at_depth(pin, cam, depth)
        return np.stack([np.linalg.norm(at_depth(rays[i], cam, depth) - want[i], axis=1) for i in range(16)])

    m = misses(focus, focus)
    print("radius %.4g, focus %.4g: largest miss on the focus plane %.3g (bound %.3g)" % (radius, focus, m.max(), 1e-5 * focus))
    assert m.max() <= 1e-5 * focus
    # focused at twice the depth, the rays cross the plane at `focus` on circles of half the lens point's distance from the axis: radius / 2 for the rim
    m2 = misses(2 * focus, focus)
    ar, bu = L.lens_const(cam, radius, focus)[:2]
    off = np.linalg.norm(np.outer(ar * d2[:, 0], cam.right.astype(f64)) + np.outer(bu * d2[:, 1], cam.up.astype(f64)), axis=1)   # the lens points' offsets
    assert np.abs(off[:32] - radius).max() <= 1e-6 * radius
    print("focused at twice the depth: largest |miss - offset / 2| %.3g" % np.abs(m2 - off / 2).max())
    assert np.abs(m2 - off / 2).max() <= 1e-5 * focus
    assert np.abs(m2[:, :32] - radius / 2).max() <= 1e-5 * focus
    # the named defect: the film point shifted with the wrong sign sends the rays away from the pinhole ray's point -- by twice the offset on the focus plane
    wrong = misses(focus, focus, sign=-1.0)
    assert wrong.max() > 1e-5 * focus and np.abs(wrong - 2 * off).max() <= 1e-4 * focus


# ---- refusals, the pinhole, the rectangle ----

def test_what_the_check_refuses(A, api):
    lib = A.load_kyhip()
    nan, inf = float("nan"), float("inf")
    for r, f in ((0.0, 0.0), (0.0, -1.0), (0.0, nan), (0.02, 1.5), (1e-6, 1e-6), (5.0, 1e6)):   # a zero radius with any focus is the pinhole
        assert lib.kyhip_lens_check(C.byref(A.Lens(r, f, (0, 0)))) == A.KY_OK, (r, f)
    for r, f, word in ((-0.01, 1.0, b"radius"), (nan, 1.0, b"radius"), (inf, 1.0, b"radius"), (0.02, 0.0, b"focus"), (0.02, -1.0, b"focus"), (0.02, nan, b"focus"),
                       (0.02, inf, b"focus")):
        assert lib.kyhip_lens_check(C.byref(A.Lens(r, f, (0, 0)))) == A.KY_ERR_INVALID_VALUE, (r, f)
        assert word in lib.kyhip_last_error(), lib.kyhip_last_error()
    for res in ((1, 0), (0, 7)):
        assert lib.kyhip_lens_check(C.byref(A.Lens(0.02, 1.0, res))) == A.KY_ERR_INVALID_VALUE and b"reserved" in lib.kyhip_last_error()
        assert lib.kyhip_lens_check(C.byref(A.Lens(0.0, 1.0, res))) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_lens_check(None) == A.KY_ERR_INVALID_VALUE and b"NULL" in lib.kyhip_last_error()
    with pytest.raises(api.KyError):
        api.lens(-1.0, 1.0)
    got = api.lens(0.25, 3.0)
    assert (got.radius, got.focus_distance, tuple(got.reserved)) == (0.25, 3.0, (0, 0))
    assert C.sizeof(A.Lens) == 16


def test_a_lens_launch_reads_the_whole_pixel_range(A, api):
    w, h = 96, 72
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    p = api.make_params(w, h, 4)
    tent = api.pixel_filter(A.FILTER_TENT, 4.0)
    rect0, dead0, total0 = api.scene_screen_bound(scene, p)
    assert dead0 > 0
    for flt in (None, tent):
        want = api.scene_screen_bound(scene, p, filter=flt)
        assert api.scene_screen_bound(scene, p, filter=flt, lens=api.lens(0.0, 0.0)) == want     # radius 0: kyhip_scene_screen_bound_filtered's answer
        assert api.scene_screen_bound(scene, p, filter=flt, lens=api.lens(0.0, 2.5)) == want
        assert api.scene_screen_bound(scene, p, filter=flt, lens=api.lens(0.02, 2.5)) == ((0, 0, w, h), 0, total0)
    lib = A.load_kyhip()
    rect, counts = (C.c_int * 4)(), (C.c_longlong * 2)()
    assert lib.kyhip_scene_screen_bound_lens(api._scene_ptr(scene), C.byref(p), None, None, rect, counts) == A.KY_OK and tuple(rect) == rect0 and counts[0] == dead0
    bad = A.Lens(0.02, 0.0, (0, 0))
    assert lib.kyhip_scene_screen_bound_lens(api._scene_ptr(scene), C.byref(p), None, C.byref(bad), rect, counts) == A.KY_ERR_INVALID_VALUE
    assert b"focus" in lib.kyhip_last_error()


def test_the_device_entries_refuse_a_bad_lens_before_they_look_for_a_device(A, api):
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    p = api.make_params(16, 16, 4)
    film = np.zeros((16, 16, 3), np.float32)
    bad = A.Lens(0.02, -1.0, (0, 0))
    assert lib.kyhip_render_lens(0, api._scene_ptr(scene), C.byref(p), None, C.byref(bad), film.ctypes.data_as(C.c_void_p), 16) == A.KY_ERR_INVALID_VALUE
    assert b"focus" in lib.kyhip_last_error() and film.max() == 0
    out = np.zeros((4, 3), np.float32)
    assert lib.kyhip_kat_li_lens(0, api._scene_ptr(scene), C.byref(p), None, C.byref(bad), 3, 3, 0, 4, out.ctypes.data_as(C.c_void_p)) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_frame_set_lens(None, C.byref(bad)) == A.KY_ERR_INVALID_VALUE and b"focus" in lib.kyhip_last_error()
    assert lib.kyhip_frame_set_lens(None, C.byref(A.Lens(0.02, 1.0, (0, 0)))) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    flat = A.Scene.from_buffer_copy(scene.c)   # a camera whose `right` has no length carries no lens
    flat.camera.right[0] = flat.camera.right[1] = flat.camera.right[2] = 0.0
    ok = A.Lens(0.02, 1.0, (0, 0))
    assert lib.kyhip_kat_li_lens(0, C.byref(flat), C.byref(p), None, C.byref(ok), 3, 3, 0, 4, out.ctypes.data_as(C.c_void_p)) == A.KY_ERR_INVALID_VALUE
    assert b"camera" in lib.kyhip_last_error(), lib.kyhip_last_error()


def test_the_lens_in_a_frames_book(A):
    """kyhostcheck_lens (ky_hostcheck.cpp), host code only: the launch constants of a camera whose vectors are not unit length, the header fold beside the filter's,
    when a frame takes a lens, and the refusals that name it.  Returns the number of the case that went wrong."""
    import os
    import subprocess
    if A.SANITIZE:
        lib = A.load_kyhip()
    else:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        target = os.path.join("build", "san", "libkyhip_host_plain.so")
        r = subprocess.run(["make", "-s", "-C", root, target], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(os.path.join(root, target))
        lib.kyhostcheck_lens.restype, lib.kyhostcheck_lens.argtypes = A.KYHOSTCHECK_SYMBOLS["kyhostcheck_lens"]
    assert lib.kyhostcheck_lens() == 0
