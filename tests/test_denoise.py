"""CPU: the arithmetic of a frame's denoise filter (ky_amd/csrc/ky_denoise.hpp; DESIGN.md "Denoise") and what its entry points refuse before any device.  The
header's level function runs here as host code (kyhostcheck_denoise, ky_amd/csrc/ky_hostcheck.cpp: the file the sanitizer builds hold too) on random guides and
colours, against the NumPy float64 restatement of tests/denoise_restatement.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_restatement as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIX = 2.0 * 0.55 / 40.0   # a pixel's width at unit distance: the order of the tests' Cornell camera at 40 pixels


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_denoise: the sanitizer build when the suite runs inside `make sanitize`, else the same sources built plainly."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    lib.kyhostcheck_denoise.restype, lib.kyhostcheck_denoise.argtypes = A.KYHOSTCHECK_SYMBOLS["kyhostcheck_denoise"]
    return lib


def _buffers(w, h, seed, zero_variance=False):
    """A film of three planes that meet at two creases (normals and positions that belong together), noisy colours around a smooth picture, a variance of the
    noise's order, and all four classes: a missed corner, a lamp, scattered flagged pixels, single pixels of every class on all four borders."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    plane = (xs > 0.45 * w).astype(int) + (ys > 0.6 * h).astype(int)
    normals = np.array([[0.0, 0.0, -1.0], [-0.6, 0.0, -0.8], [0.0, 0.8, -0.6]])
    depth = 3.0 + 0.02 * xs + 0.01 * ys + 0.3 * plane
    ga = np.concatenate([normals[plane] + rng.normal(0, 1e-4, (h, w, 3)), depth[..., None]], axis=2).astype(np.float32)
    pos = np.stack([(xs - w / 2) * PIX * depth, (h / 2 - ys) * PIX * depth, depth], axis=2)
    cls = np.zeros((h, w), np.float32)
    cls[:3, -4:] = D.MISS
    cls[h // 2:h // 2 + 2, w // 2:w // 2 + 3] = D.LIGHT
    cls[rng.random((h, w)) < 0.03] = D.FLAGGED
    cls[0, 5], cls[h - 1, 7], cls[4, 0], cls[9, w - 1] = D.MISS, D.LIGHT, D.FLAGGED, D.MISS
    gb = np.concatenate([pos, cls[..., None]], axis=2).astype(np.float32)
    smooth = np.stack([0.4 + 0.3 * np.sin(xs / 7), 0.5 + 0.2 * np.cos(ys / 5), 0.3 + 0.1 * plane], axis=2)
    sd = 0.0 if zero_variance else 0.05
    rgb = np.abs(smooth + rng.normal(0, sd, (h, w, 3)))
    rgb[cls == D.LIGHT] = 17.0
    v = np.zeros((h, w)) if zero_variance else (sd * sd) * rng.uniform(0.5, 1.5, (h, w))
    cv = np.concatenate([rgb, v[..., None]], axis=2).astype(np.float32)
    return cv, ga, gb


def _host(check, A, cv, ga, gb, levels, **over):
    h, w = cv.shape[:2]
    q = A.DenoiseParams(levels, *(over.get(k, D.DEFAULTS[k]) for k in ("normal_squarings", "sigma_luminance", "sigma_plane")))
    out = np.zeros((h, w, 4), np.float32)
    arrays = [np.ascontiguousarray(a, np.float32) for a in (cv, ga, gb)]
    assert check.kyhostcheck_denoise(*(a.ctypes.data for a in arrays), w, h, C.byref(q), PIX, out.ctypes.data) == A.KY_OK
    return out


worst = {}


@pytest.mark.parametrize("zero_variance", [False, True], ids=["noisy", "v_zero"])
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", [(40, 24), (44, 21)])
def test_host_build_against_the_restatement(w, h, levels, zero_variance, A, check):
    """Levels are float32 stored from double, on both sides: float32 outputs are equal except where a double lands within its rounding error of a float32
    boundary, and weights and colours are non-negative, so nothing cancels: rtol = levels x 2^-23, atol = 0.  At 40 x 24 and 44 x 21 every level from step 8 on
    has taps off the film for every pixel, and step 16 leaves it on both sides at once.  Measured: the largest difference is 0 in every case (printed)."""
    cv, ga, gb = _buffers(w, h, 11 * w + levels, zero_variance)
    got = _host(check, A, cv, ga, gb, levels)
    want = D.denoise(cv, ga, gb, PIX, levels=levels)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    surface = gb[..., 3] == D.SURFACE
    assert {int(c) for c in np.unique(gb[..., 3])} == {0, 1, 2, 3}
    assert np.array_equal(got[~surface], cv[~surface])            # pass-through: to the bit
    assert not np.array_equal(got[surface], cv[surface])
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = float((err / np.maximum(np.abs(want.astype(np.float64)), 1e-300)).max())
    worst[(w, h, levels, zero_variance)] = rel
    print("largest relative |host - restatement| (%d x %d, %d levels%s): %.3e" % (w, h, levels, ", v = 0" if zero_variance else "", rel))
    assert (err <= levels * 2.0 ** -23 * np.abs(want.astype(np.float64))).all(), rel
    if zero_variance:
        assert (got[..., 3] == 0).all()


def test_the_filter_smooths_inside_a_plane_and_keeps_the_creases(A, check):
    """What the weights are for, on the host build: inside a plane the noise falls; a pixel next to a crease takes nothing from the other plane (its normal
    weight is 0.8^128 or 0.6^128 there, below 4e-13), so a step in colour across the crease stays a step."""
    w, h = 40, 24
    cv, ga, gb = _buffers(w, h, 5)
    gb[..., 3] = 0
    plane_right = np.mgrid[0:h, 0:w][1] > 0.45 * w
    cv[..., :3] = np.where(plane_right[..., None], 0.9, 0.1) + np.random.default_rng(3).normal(0, 0.02, (h, w, 3))
    cv[..., 3] = 0.02 ** 2
    got = _host(check, A, cv, ga, gb, 5, sigma_luminance=4.0, sigma_plane=1.0)   # (wide sigmas: the synthetic planes' positions are not exactly planar)
    top = np.mgrid[0:h, 0:w][0] <= 0.6 * h - 1
    for side, level_ in ((plane_right, 0.9), (~plane_right, 0.1)):
        sel = side & top
        assert np.abs(got[sel][:, :3] - level_).max() < 0.02 and got[sel][:, :3].std() < 0.4 * cv[sel][:, :3].std()
    assert (got[..., 3] < cv[..., 3]).all()     # the carried variance falls with every level


def test_defaults(A):
    lib = A.load_kyhip()
    q = A.DenoiseParams(-1, -1, -1.0, -1.0)
    lib.kyhip_denoise_defaults(C.byref(q))
    assert (q.levels, q.normal_squarings) == (D.DEFAULTS["levels"], D.DEFAULTS["normal_squarings"]) == (5, 7)
    assert (q.sigma_luminance, q.sigma_plane) == (D.DEFAULTS["sigma_luminance"], D.DEFAULTS["sigma_plane"])
    lib.kyhip_denoise_defaults(None)           # nothing to write: fine


def test_arguments_are_refused_before_any_device(A, api):
    lib = A.load_kyhip()
    film = np.full((4, 4, 3), 7.0, np.float32)
    ptr = C.c_void_p(film.ctypes.data)
    assert lib.kyhip_frame_denoise(None, None, ptr, 4) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_guides(None, ptr, None, 4) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    ms = C.c_float(7)
    assert lib.kyhip_frame_denoise_ms(None, C.byref(ms), None) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error() and ms.value == 7
    nan = float("nan")
    bad = [((-1, 7, 4.0, 1.0), b"levels"), ((7, 7, 4.0, 1.0), b"levels"), ((5, -1, 4.0, 1.0), b"normal_squarings"), ((5, 11, 4.0, 1.0), b"normal_squarings"),
           ((5, 7, 0.0, 1.0), b"sigma_luminance"), ((5, 7, -2.0, 1.0), b"sigma_luminance"), ((5, 7, nan, 1.0), b"sigma_luminance"),
           ((5, 7, 4.0, 0.0), b"sigma_plane"), ((5, 7, 4.0, -1e-30), b"sigma_plane"), ((5, 7, 4.0, nan), b"sigma_plane")]
    for fields, word in bad:
        q = A.DenoiseParams(*fields)
        assert lib.kyhip_frame_denoise(None, C.byref(q), ptr, 4) == A.KY_ERR_INVALID_VALUE and word in lib.kyhip_last_error(), fields
    for fields in ((0, 0, 1e-30, 1e-30), (6, 10, 1e30, 1e30)):   # the ends of the ranges pass the parameter check: the frame is what is missing
        q = A.DenoiseParams(*fields)
        assert lib.kyhip_frame_denoise(None, C.byref(q), ptr, 4) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert (film == 7).all()


def test_params_struct_layout(A, tmp_path):
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "kyhip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(ky_denoise_params), ' \
           'offsetof(ky_denoise_params, normal_squarings), offsetof(ky_denoise_params, sigma_luminance), offsetof(ky_denoise_params, sigma_plane));return 0;}'
    (tmp_path / "sz.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "sz.c"), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    assert got == [C.sizeof(A.DenoiseParams), A.DenoiseParams.normal_squarings.offset, A.DenoiseParams.sigma_luminance.offset, A.DenoiseParams.sigma_plane.offset]
