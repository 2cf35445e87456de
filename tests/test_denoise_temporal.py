"""CPU: the temporal step of a frame's denoise filter (ky_amd/csrc/ky_denoise.hpp, temporal_pixel_t; DESIGN.md "Denoise", "Temporal") and what
kyhip_frame_denoise_temporal refuses before any device.  The header's function runs here as host code (kyhostcheck_temporal, ky_amd/csrc/ky_hostcheck.cpp: the
file the sanitizer builds hold too) against the NumPy restatement of tests/denoise_temporal_restatement.py; what the step means is checked on both, and each named
defect, injected into the restatement, fails the test that defines it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import denoise_chains_restatement as DC
import denoise_restatement as D
import denoise_temporal_restatement as DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIX = 2.0 * 0.55 / 40.0   # tests/test_denoise.py's: the order of the tests' Cornell camera at 40 pixels


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_temporal: the sanitizer build when the suite runs inside `make sanitize`, else the same sources built plainly."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    for name in ("kyhostcheck_temporal", "kyhostcheck_temporal_refusal", "kyhostcheck_denoise", "kyhostcheck_denoise_keyed"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = A.KYHOSTCHECK_SYMBOLS[name]
    return lib


def _camera(A, w, h, position=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0):
    """A ky_camera with a film `w PIX` wide and `h PIX` high at unit distance (generate_ray: front + right (px / w - 0.5) + up (0.5 - py / h)), turned by yaw
    about y and then by pitch about its right axis"""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    right = np.array([cy, 0.0, -sy])
    front = np.array([sy * cp, sp, cy * cp])
    up = np.cross(front, right)
    c = A.Camera()
    for i in range(3):
        c.position[i], c.front[i], c.right[i], c.up[i] = position[i], front[i], right[i] * w * PIX, up[i] * h * PIX
    c.resolution[0], c.resolution[1] = w, h
    return c


WALLS = ((np.array([0.0, 0.0, 5.0]), np.array([0.0, 0.0, -1.0])),     # a back wall, a floor and a left wall: three planes that meet at creases
         (np.array([0.0, -0.5, 0.0]), np.array([0.0, 1.0, 0.0])),
         (np.array([-0.8, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])))


def _film(A, camera, w, h, seed, walls=WALLS, classes=True, keys=True):
    """What a frame under `camera` sees of the walls: the guides of the nearest wall along each pixel centre's ray (normals with a little noise, as
    tests/test_denoise.py's), noisy colours around a picture that is a function of the WORLD position, a variance of the noise's order, all four classes and a
    patch of non-zero chain keys -> (cv, ga, gb, key)"""
    rng = np.random.default_rng(seed)
    o, f, r, u = DT.camera_vectors(camera)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d = f + r * ((xs[..., None] + 0.5) / w - 0.5) + u * (0.5 - (ys[..., None] + 0.5) / h)
    d = d / np.linalg.norm(d, axis=2, keepdims=True)
    t = np.full((h, w), np.inf)
    n = np.zeros((h, w, 3))
    for point, normal in walls:
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = ((point - o) @ normal) / (d @ normal)
        hit = (tt > 1e-6) & (tt < t)
        t = np.where(hit, tt, t)
        n = np.where(hit[..., None], normal, n)
    assert np.isfinite(t).all()
    P = o + t[..., None] * d
    ga = np.concatenate([n + rng.normal(0, 1e-4, (h, w, 3)), t[..., None]], axis=2).astype(np.float32)
    cls = np.zeros((h, w), np.float32)
    key = np.zeros((h, w), np.uint64)
    if classes:
        cls[:3, -4:] = D.MISS
        cls[h // 2:h // 2 + 2, w // 2:w // 2 + 3] = D.LIGHT
        cls[rng.random((h, w)) < 0.03] = D.FLAGGED
        cls[0, 5], cls[h - 1, 7], cls[4, 0], cls[9, w - 1] = D.MISS, D.LIGHT, D.FLAGGED, D.MISS
    if keys:
        key[h // 3:h // 3 + 5, w // 4:w // 4 + 7] = DC.digit(5, False)
        key[h // 3 + 2, w // 4 + 3] = DC.UNRESOLVED | DC.digit(6, True)
    gb = np.concatenate([P, cls[..., None]], axis=2).astype(np.float32)
    smooth = np.stack([0.4 + 0.3 * np.sin(3 * P[..., 0]), 0.5 + 0.2 * np.cos(2 * P[..., 1]), 0.3 + 0.05 * P[..., 2]], axis=2)
    rgb = np.abs(smooth + rng.normal(0, 0.05, (h, w, 3)))
    rgb[cls == D.LIGHT] = 17.0
    v = 0.05 ** 2 * rng.uniform(0.5, 1.5, (h, w))
    cv = np.concatenate([rgb, v[..., None]], axis=2).astype(np.float32)
    return cv, ga, gb, key


def _history(A, camera, w, h, seed, **kw):
    """A history side as an earlier call under `camera` would have left it: {P, m} with m = 0 on every pixel that is not class 0 or carries a key, on a
    scattered twentieth of the others too, and counts between 8 and 200 elsewhere"""
    cv, ga, gb, key = _film(A, camera, w, h, seed, **kw)
    rng = np.random.default_rng(seed + 1)
    m = np.floor(rng.uniform(8, 200, (h, w))).astype(np.float32)
    m[(gb[..., 3] != D.SURFACE) | (key != 0) | (rng.random((h, w)) < 0.05)] = 0
    hgb = gb.copy()
    hgb[..., 3] = m
    return cv, ga, hgb


def _host(check, A, cv, ga, gb, key, hist, w, h, n_p, then, pix, **over):
    t = A.TemporalParams(*(over.get(k, DT.DEFAULTS[k]) for k in ("max_history", "sigma_plane", "min_weight", "normal_squarings")))
    arrays = [np.ascontiguousarray(a, np.float32) for a in (cv, ga, gb)]
    keys = None if key is None else np.ascontiguousarray(key, np.uint64)
    hs = [None] * 3 if hist is None else [np.ascontiguousarray(a, np.float32) for a in hist]
    out_cv, out_gb = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    rc = check.kyhostcheck_temporal(*(a.ctypes.data for a in arrays), None if keys is None else keys.ctypes.data, *(None if a is None else a.ctypes.data for a in hs),
                                    w, h, float(n_p), C.byref(t), float(pix), C.byref(then), out_cv.ctypes.data, out_gb.ctypes.data)
    assert rc == A.KY_OK
    return out_cv, out_gb


def _within(got, want, ulps):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = float((err / np.maximum(np.abs(want.astype(np.float64)), 1e-300)).max())
    return bool((err <= ulps * 2.0 ** -23 * np.abs(want.astype(np.float64))).all()), rel


def _moved(A, w, h):
    """The two cameras of the first test: `now` at the origin looking along +z, `then` 1.9 ahead of it, 0.25 to the right and 0.05 down, turned by 0.12 about y
    and 0.05 upwards"""
    return _camera(A, w, h), _camera(A, w, h, position=(0.25, -0.05, 1.9), yaw=0.12, pitch=0.05)


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "keyed"])
@pytest.mark.parametrize("w,h", [(40, 24), (44, 21)])
def test_host_build_against_the_restatement(w, h, keyed, A, check):
    """The step stores float32 from double on both sides, blends of non-negative terms: rtol = 2 x 2^-23, atol = 0 for the step alone (one rounding, and one
    for a double that lands within its error of a float32 boundary), (levels + 2) x 2^-23 through the levels.  The history camera stands ahead of the current one
    and is turned, so the current film's points reproject off all four sides of the history's film, and the floor and the left wall near the current camera lie
    BEHIND the history camera.  Measured: the largest difference is 0 in every case (printed)."""
    now, then = _moved(A, w, h)
    cv, ga, gb, key = _film(A, now, w, h, 11 * w)
    hist = _history(A, then, w, h, 7 * w)
    key = key if keyed else None
    pix, n_p = D.pixel_width(now, w), 16
    sx, sy, z = DT.project(gb[..., :3], DT.camera_vectors(then), w, h)
    front = z > 0
    assert (z <= 0).sum() >= 10 and (front & (sx <= -1)).any() and (front & (sx >= w)).any() and (front & (sy <= -1)).any() and (front & (sy >= h)).any()
    assert {int(c) for c in np.unique(gb[..., 3])} == {0, 1, 2, 3} and (hist[2][..., 3] == 0).sum() > 40
    got_cv, got_gb = _host(check, A, cv, ga, gb, key, hist, w, h, n_p, then, pix)
    want_cv, want_gb, took = DT.temporal(cv, ga, gb, key, hist, n_p, pix, DT.camera_vectors(then))
    assert np.isfinite(got_cv).all() and np.isfinite(want_cv).all()
    assert took.mean() > 0.15 and (~took & (gb[..., 3] == D.SURFACE)).sum() > 100, took.mean()
    ok_c, rel_c = _within(got_cv, want_cv, 2)
    ok_m, rel_m = _within(got_gb, want_gb, 2)
    print("largest relative |host - restatement| (%d x %d, %s): colour / variance %.3e, count %.3e; %d of %d pixels took history" % (
        w, h, "keyed" if keyed else "plain", rel_c, rel_m, int(took.sum()), took.size))
    assert ok_c and ok_m, (rel_c, rel_m)
    assert np.array_equal(got_gb[..., :3], gb[..., :3])
    assert np.array_equal(got_cv[~took], cv[~took])                               # without history: the gather's bits
    eligible = (gb[..., 3] == D.SURFACE) & ((key == 0) if keyed else True)
    assert (got_gb[..., 3][eligible & ~took] == n_p).all() and (got_gb[..., 3][~eligible] == 0).all() and (got_gb[..., 3][took] > n_p).all()
    # ... and through the levels, on the host build's own levels
    for levels in (1, 3, 5):
        q = A.DenoiseParams(levels, *(D.DEFAULTS[k] for k in ("normal_squarings", "sigma_luminance", "sigma_plane")))
        out = np.zeros((h, w, 4), np.float32)
        if keyed:
            kk = np.ascontiguousarray(key, np.uint64)
            assert check.kyhostcheck_denoise_keyed(got_cv.ctypes.data, ga.ctypes.data, gb.ctypes.data, kk.ctypes.data, w, h, C.byref(q), pix, out.ctypes.data) == A.KY_OK
        else:
            assert check.kyhostcheck_denoise(got_cv.ctypes.data, ga.ctypes.data, gb.ctypes.data, w, h, C.byref(q), pix, out.ctypes.data) == A.KY_OK
        want = DT.levels(want_cv, ga, gb, key, None, pix, **dict(D.DEFAULTS, levels=levels))
        ok, rel = _within(out, want, levels + 2)
        print("    through %d levels: %.3e" % (levels, rel))
        assert ok, (levels, rel)
    # an empty history: the gather's bits and m = n_p
    got_cv, got_gb = _host(check, A, cv, ga, gb, key, None, w, h, n_p, then, pix)
    assert got_cv.tobytes() == cv.tobytes() and (got_gb[..., 3] == np.where(eligible, n_p, 0)).all()


# ---- what it means ----

def _both(check, A, cv, ga, gb, key, hist, w, h, n_p, then, pix, defect=None, **over):
    """(host build, restatement) of one step, or the restatement with a defect twice"""
    want = DT.temporal(cv, ga, gb, key, hist, n_p, pix, DT.camera_vectors(then), defect=defect, **dict(DT.DEFAULTS, **over))[:2]
    return [want, want] if defect else [_host(check, A, cv, ga, gb, key, hist, w, h, n_p, then, pix, **over), want]


def _same_camera(check, A, defect, n1, n2, max_history):
    """The same camera on both sides and the back wall's guides: the reprojection lands on pixel centres to float32 rounding, one tap carries all the weight, and
    the result is the sample-weighted mean (n1 c1 + n2 c2) / (n1 + n2) with v = (n2^2 v2 + n1^2 v1) / (n1 + n2)^2 -- 1e-4 relative: fx and fy are of order 1e-6"""
    w, h = 40, 24
    cam = _camera(A, w, h)
    back = WALLS[:1]
    cv2, ga, gb, _ = _film(A, cam, w, h, 3, walls=back, classes=False, keys=False)
    cv1, hga, hgb = _film(A, cam, w, h, 4, walls=back, classes=False, keys=False)[:3]
    hgb = hgb.copy()
    hgb[..., 3] = n1
    pix = D.pixel_width(cam, w)
    for out_cv, out_gb in _both(check, A, cv2, ga, gb, None, (cv1, hga, hgb), w, h, n2, cam, pix, defect=defect, max_history=max_history):
        mean = (n1 * cv1[..., :3].astype(np.float64) + n2 * cv2[..., :3].astype(np.float64)) / (n1 + n2)
        var = (n1 * n1 * cv1[..., 3].astype(np.float64) + n2 * n2 * cv2[..., 3].astype(np.float64)) / (n1 + n2) ** 2
        assert np.allclose(out_cv[..., :3], mean, rtol=1e-4, atol=0)
        assert np.allclose(out_cv[..., 3], var, rtol=1e-4, atol=0)
        assert np.allclose(out_gb[..., 3], n1 + n2, rtol=1e-4, atol=0)
        assert (out_cv[..., 3] < np.maximum(cv1[..., 3], cv2[..., 3])).all()        # v falls: a convex blend's variance lies below the larger of the two
    return out_cv


def test_the_same_camera_gives_the_sample_weighted_mean(A, check):
    _same_camera(check, A, None, 48.0, 16.0, 8.0)
    out = _same_camera(check, A, None, 16.0, 16.0, 1.0)    # max_history = 1 and equal counts: alpha is 1/2
    assert np.isfinite(out).all()


def _half_pixel(check, A, defect):
    """The camera moved by exactly half a pixel along its right axis at the back wall's depth: fx = 1/2, two taps of weight 1/2 each (fy is of order 1e-6),
    c_h their mean and v_h = (v_a + v_b) / 4 -- the w^2 rule; with equal counts n: c = (c_p + c_h) / 2, v = (v_p + v_h) / 4"""
    w, h = 40, 24
    then = _camera(A, w, h)
    now = _camera(A, w, h, position=(0.5 * PIX * 5.0, 0.0, 0.0))
    back = WALLS[:1]
    cv2, ga, gb, _ = _film(A, now, w, h, 3, walls=back, classes=False, keys=False)
    cv1, hga, hgb = _film(A, then, w, h, 4, walls=back, classes=False, keys=False)[:3]
    hgb = hgb.copy()
    hgb[..., 3] = 16.0
    ga[..., :3] = hga[..., :3] = np.float32([0.0, 0.0, -1.0])   # (exact normals: _film's noise of 1e-4 moves (n_p . n_q)^128 by 2 %, which one tap cancels and two do not)
    pix = D.pixel_width(now, w)
    inner =np.s_[:, :w - 1]          # the current pixel i lands between the history's i and i + 1: the last column has one tap only
    for out_cv, out_gb in _both(check, A, cv2, ga, gb, None, (cv1, hga, hgb), w, h, 16.0, then, pix, defect=defect, sigma_plane=4.0):
        a, b = cv1[:, :-1].astype(np.float64), cv1[:, 1:].astype(np.float64)
        c_h, v_h = (a[..., :3] + b[..., :3]) / 2, (a[..., 3] + b[..., 3]) / 4
        assert np.allclose(out_cv[inner][..., :3], (cv2[inner][..., :3] + c_h) / 2, rtol=1e-4, atol=0)
        assert np.allclose(out_cv[inner][..., 3], (cv2[inner][..., 3] + v_h) / 4, rtol=1e-4, atol=0)
        assert np.allclose(out_gb[inner][..., 3], 32.0, rtol=1e-4, atol=0)


def test_half_a_pixel_between_two_taps(A, check):
    _half_pixel(check, A, None)


def _capped(check, A, defect):
    """A history a hundred times the frame's samples is capped at max_history x n_p: m = 9 n_p and alpha = 1 / 9 at max_history 8"""
    w, h = 40, 24
    cam = _camera(A, w, h)
    back = WALLS[:1]
    cv2, ga, gb, _ = _film(A, cam, w, h, 3, walls=back, classes=False, keys=False)
    cv1, hga, hgb = _film(A, cam, w, h, 4, walls=back, classes=False, keys=False)[:3]
    hgb = hgb.copy()
    hgb[..., 3] = 1600.0
    for out_cv, out_gb in _both(check, A, cv2, ga, gb, None, (cv1, hga, hgb), w, h, 16.0, cam, D.pixel_width(cam, w), defect=defect):
        assert (out_gb[..., 3] == 9 * 16.0).all()
        assert np.allclose(out_cv[..., :3], (cv2[..., :3].astype(np.float64) + 8 * cv1[..., :3].astype(np.float64)) / 9, rtol=1e-4, atol=0)


def test_the_history_is_capped(A, check):
    _capped(check, A, None)


DEFINED_BY = {"sy_not_flipped": lambda check, A, d: _same_camera(check, A, d, 48.0, 16.0, 8.0),
              "no_half": lambda check, A, d: _same_camera(check, A, d, 48.0, 16.0, 8.0),
              "alpha_swapped": lambda check, A, d: _same_camera(check, A, d, 48.0, 16.0, 8.0),
              "v_by_w": lambda check, A, d: _half_pixel(check, A, d),
              "m_uncapped": lambda check, A, d: _capped(check, A, d)}


@pytest.mark.parametrize("defect", DT.DEFECTS)
def test_named_defects_fail_the_test_that_defines_them(defect, A, check):
    """sy not flipped, the -0.5 omitted, alpha and 1 - alpha swapped: the same-camera test; v_h weighted by w instead of w^2: the half-pixel test (one tap of
    weight 1 cannot tell w from w^2); M not capped: the cap's test.  Each runs on the restatement with the defect in place of the host build."""
    with pytest.raises(AssertionError):
        DEFINED_BY[defect](check, A, defect)


# ---- disocclusion, and who passes through ----

@pytest.mark.parametrize("what", ["depth", "normal"])
def test_disocclusion(what, A, check):
    """The current pixel's guides lie on a plane the history saw at another depth (the back wall 0.5 further away: xp is 0.5 / (0.25 x 5 x pix), far above 1 at
    every pixel ... 13: wp < 4e-5) or under another normal (0.8^128 < 4e-13): the weight stays below min_weight, m = n_p and the colour is the gather's bits"""
    w, h = 40, 24
    cam = _camera(A, w, h)
    cv2, ga, gb, _ = _film(A, cam, w, h, 3, walls=WALLS[:1], classes=False, keys=False)
    if what == "depth":
        other = ((np.array([0.0, 0.0, 5.5]), np.array([0.0, 0.0, -1.0])),)
        cv1, hga, hgb = _film(A, cam, w, h, 4, walls=other, classes=False, keys=False)[:3]
    else:
        cv1, hga, hgb = _film(A, cam, w, h, 4, walls=WALLS[:1], classes=False, keys=False)[:3]
        hga = hga.copy()
        hga[..., :3] = np.float32([0.6, 0.0, -0.8])
    hgb = hgb.copy()
    hgb[..., 3] = 64.0
    pix = D.pixel_width(cam, w)
    for out_cv, out_gb in _both(check, A, cv2, ga, gb, None, (cv1, hga, hgb), w, h, 16.0, cam, pix):
        assert out_cv.tobytes() == cv2.tobytes() and (out_gb[..., 3] == 16.0).all()


def test_pass_through(A, check):
    """Pixels of classes 1, 2 and 3 and pixels with a non-zero key pass through with m = 0, to the bit -- under the same camera, where every one of them would
    find a tap; their neighbours take history"""
    w, h = 44, 21
    cam = _camera(A, w, h)
    cv2, ga, gb, key = _film(A, cam, w, h, 3)
    cv1, hga, hgb = _film(A, cam, w, h, 4, classes=False, keys=False)[:3]
    hgb = hgb.copy()
    hgb[..., 3] = 64.0
    out = (gb[..., 3] != D.SURFACE) | (key != 0)
    assert {int(c) for c in np.unique(gb[..., 3])} == {0, 1, 2, 3} and (key != 0).sum() >= 30
    for out_cv, out_gb in _both(check, A, cv2, ga, gb, key, (cv1, hga, hgb), w, h, 16.0, cam, D.pixel_width(cam, w)):
        assert out_cv[out].tobytes() == cv2[out].tobytes() and (out_gb[..., 3][out] == 0).all()
        assert (out_gb[..., 3][~out] > 16.0).mean() > 0.9 and not np.array_equal(out_cv[~out], cv2[~out])


# ---- refusals, without a device ----

def test_defaults(A, api):
    lib = A.load_kyhip()
    t = A.TemporalParams(-1.0, -1.0, -1.0, -1)
    lib.kyhip_temporal_defaults(C.byref(t))
    d = api.temporal_defaults()
    for name in ("max_history", "sigma_plane", "min_weight", "normal_squarings"):
        assert getattr(t, name) == getattr(d, name) == np.float32(DT.DEFAULTS[name]), name
    lib.kyhip_temporal_defaults(None)          # nothing to write: fine


def test_arguments_are_refused_before_any_device(A, api):
    lib = A.load_kyhip()
    film = np.full((4, 4, 3), 7.0, np.float32)
    ptr = C.c_void_p(film.ctypes.data)
    call = lambda q, t: lib.kyhip_frame_denoise_temporal(None, None, None if q is None else C.byref(q), None if t is None else C.byref(t), ptr, 4)
    assert call(None, None) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    nan = float("nan")
    bad = [((0.0, 0.25, 0.05, 7), b"max_history"), ((-1.0, 0.25, 0.05, 7), b"max_history"), ((1024.5, 0.25, 0.05, 7), b"max_history"), ((nan, 0.25, 0.05, 7), b"max_history"),
           ((8.0, 0.0, 0.05, 7), b"sigma_plane"), ((8.0, -1e-30, 0.05, 7), b"sigma_plane"), ((8.0, nan, 0.05, 7), b"sigma_plane"),
           ((8.0, 0.25, -1e-30, 7), b"min_weight"), ((8.0, 0.25, 1.0, 7), b"min_weight"), ((8.0, 0.25, nan, 7), b"min_weight"),
           ((8.0, 0.25, 0.05, -1), b"normal_squarings"), ((8.0, 0.25, 0.05, 11), b"normal_squarings")]
    for fields, word in bad:
        assert call(None, A.TemporalParams(*fields)) == A.KY_ERR_INVALID_VALUE and word in lib.kyhip_last_error(), fields
    for fields in ((1e-30, 1e-30, 0.0, 0), (1024.0, 1e30, 0.999, 10)):   # the ends of the ranges pass the parameter check: the frame is what is missing
        assert call(None, A.TemporalParams(*fields)) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error(), fields
    for fields, word in (((7, 7, 4.0, 1.0), b"levels"), ((5, 11, 4.0, 1.0), b"normal_squarings"), ((5, 7, 0.0, 1.0), b"sigma_luminance"), ((5, 7, 4.0, nan), b"sigma_plane")):
        assert call(A.DenoiseParams(*fields), None) == A.KY_ERR_INVALID_VALUE and word in lib.kyhip_last_error(), fields   # (what kyhip_frame_denoise refuses of them)
    assert (film == 7).all()
    for fn in (lib.kyhip_history_destroy, lib.kyhip_history_reset, lib.kyhip_history_frames):
        assert fn(None) == A.KY_ERR_INVALID_VALUE and b"history is NULL" in lib.kyhip_last_error()
    ms = C.c_float(7)
    assert lib.kyhip_history_ms(None, C.byref(ms)) == A.KY_ERR_INVALID_VALUE and ms.value == 7
    assert lib.kyhip_history_read(None, ptr, None, 4) == A.KY_ERR_INVALID_VALUE and (film == 7).all()
    assert lib.kyhip_history_create(0, 4, 4, None) == A.KY_ERR_INVALID_VALUE and b"out is NULL" in lib.kyhip_last_error()
    out = C.c_void_p(7)
    for w, h in ((0, 4), (4, -1)):
        assert lib.kyhip_history_create(0, w, h, C.byref(out)) == A.KY_ERR_INVALID_VALUE and b"history of" in lib.kyhip_last_error() and not out.value


def test_what_is_refused_of_a_frame_and_a_history(A, api, check):
    """FrameBook::temporal_check, the question kyhip_frame_denoise_temporal asks its frame's book before any device work, on books without a device
    (kyhostcheck_temporal_refusal): what kyhip_frame_denoise refuses, a frame that tracks blocks, and a history of another device, size or albedo mode"""
    p = api.make_params(40, 24, 64)
    shard = api.make_params(40, 24, 64, tile_first=0, tile_step=2)
    last = check.kyhip_last_error
    last.restype = C.c_char_p
    #        params  noise blocks batches device grid | the history's device, width, height, albedo mode
    ok = (p, 1, 0, 2, 0, 0, 0, 40, 24, -1)
    assert check.kyhostcheck_temporal_refusal(C.byref(ok[0]), *ok[1:]) == A.KY_OK
    for fields in ((p, 1, 0, 5, 1, 4, 1, 40, 24, 1), (p, 1, 0, 2, 0, 0, 0, 40, 24, 0), (p, 1, 0, 2, 0, 4, 0, 40, 24, -1)):
        assert check.kyhostcheck_temporal_refusal(C.byref(fields[0]), *fields[1:]) == A.KY_OK, fields[1:]
    refused = [((p, 0, 0, 2, 0, 0, 0, 40, 24, -1), b"noise"), ((shard, 1, 0, 2, 0, 0, 0, 40, 24, -1), b"shard"), ((p, 1, 0, 1, 0, 0, 0, 40, 24, -1), b"noise batches"),
               ((p, 1, 1, 2, 0, 0, 0, 40, 24, -1), b"tracks blocks"), ((p, 1, 0, 2, 0, 0, 1, 40, 24, -1), b"device"), ((p, 1, 0, 2, 0, 0, 0, 44, 24, -1), b"the history is 44 x 24"),
               ((p, 1, 0, 2, 0, 0, 0, 40, 21, -1), b"the history is 40 x 21"), ((p, 1, 0, 2, 0, 4, 0, 40, 24, 0), b"plain colours"),
               ((p, 1, 0, 2, 0, 0, 0, 40, 24, 1), b"albedo-demodulated")]
    for fields, word in refused:
        assert check.kyhostcheck_temporal_refusal(C.byref(fields[0]), *fields[1:]) == A.KY_ERR_INVALID_VALUE and word in last(), (fields[1:], last())


def test_params_struct_layout(A, tmp_path):
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "kyhip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(ky_temporal_params), ' \
           'offsetof(ky_temporal_params, sigma_plane), offsetof(ky_temporal_params, min_weight), offsetof(ky_temporal_params, normal_squarings));return 0;}'
    (tmp_path / "sz.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "sz.c"), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    assert got == [C.sizeof(A.TemporalParams), A.TemporalParams.sigma_plane.offset, A.TemporalParams.min_weight.offset, A.TemporalParams.normal_squarings.offset]
