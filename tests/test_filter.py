"""CPU: the pixel filters' host side (kyhip_filter_check / _defaults / _table, ky_pixel_filter) against the NumPy restatement
(tests/filter_restatement.py), and the restatement's own semantics -- centred on the pixel's CENTRE, distributed as the analytic filter -- on the CPU oracle alone.
The GPU tests (tests/test_filter_gpu.py) then hold the device against this restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_restatement as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every kind at the ends and in the middle of the radius range: (kind, radius, param)
CASES = ((F.BOX, None, 0.0), (F.TENT, 0.5, 0.0), (F.TENT, 1.0, 0.0), (F.TENT, 2.0, 0.0), (F.TENT, 4.0, 0.0), (F.GAUSSIAN, 0.5, 0.5), (F.GAUSSIAN, 1.5, 0.5),
         (F.GAUSSIAN, 4.0, 1.0), (F.GAUSSIAN, 4.0, 0.25), (F.BLACKMAN_HARRIS, 0.5, 0.0), (F.BLACKMAN_HARRIS, 1.0, 0.0), (F.BLACKMAN_HARRIS, 2.0, 0.0),
         (F.BLACKMAN_HARRIS, 4.0, 0.0))


def both(api, kind, radius, param):
    return api.pixel_filter(kind, radius, param or None), F.Filter(kind, radius, param)


def test_struct_layout(A, tmp_path):
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "kyhip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(ky_pixel_filter), ' \
           'offsetof(ky_pixel_filter, kind), offsetof(ky_pixel_filter, radius), offsetof(ky_pixel_filter, param), offsetof(ky_pixel_filter, reserved), ' \
           'KY_FILTER_BOX, KY_FILTER_TENT, KY_FILTER_GAUSSIAN, KY_FILTER_BLACKMAN_HARRIS, KYHIP_FILTER_MAX_RADIUS, KYHIP_FILTER_TABLE);return 0;}'
    (tmp_path / "sz.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "sz.c"), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    P = A.PixelFilter
    assert got == [C.sizeof(P), P.kind.offset, P.radius.offset, P.param.offset, P.reserved.offset, A.FILTER_BOX, A.FILTER_TENT, A.FILTER_GAUSSIAN,
                   A.FILTER_BLACKMAN_HARRIS, A.FILTER_MAX_RADIUS, A.FILTER_TABLE]
    assert got[0] == 16 and (F.BOX, F.TENT, F.GAUSSIAN, F.BLACKMAN_HARRIS, F.TABLE) == (A.FILTER_BOX, A.FILTER_TENT, A.FILTER_GAUSSIAN, A.FILTER_BLACKMAN_HARRIS, A.FILTER_TABLE)


def test_render_params_and_abi_version_stay(A):
    """The filter travels beside ky_render_params, never inside them."""
    assert C.sizeof(A.RenderParams) == 48 and A.load_kyhip().kyhip_abi_version() == 4


def test_defaults(A, api):
    for kind, radius, param in ((A.FILTER_TENT, 2.0, 0.0), (A.FILTER_GAUSSIAN, 1.5, 0.5), (A.FILTER_BLACKMAN_HARRIS, 2.0, 0.0)):
        f = api.pixel_filter(kind)
        assert (f.kind, f.radius, f.param, f.reserved) == (kind, radius, param, 0)
    assert api.pixel_filter(A.FILTER_BOX).kind == A.FILTER_BOX
    f = api.pixel_filter(A.FILTER_GAUSSIAN, radius=3, param=1.25)
    assert (f.radius, f.param) == (3.0, 1.25)
    lib = A.load_kyhip()
    out = A.PixelFilter()
    assert lib.kyhip_filter_defaults(4, C.byref(out)) == A.KY_ERR_INVALID_VALUE and lib.kyhip_filter_defaults(-1, C.byref(out)) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_filter_defaults(A.FILTER_TENT, None) == A.KY_ERR_INVALID_VALUE


def test_check_refuses_one_rule_at_a_time(A):
    lib = A.load_kyhip()
    nan, inf = float("nan"), float("inf")
    bad = [((-1, 2.0, 0.0, 0), b"kind"), ((4, 2.0, 0.0, 0), b"kind"),
           ((A.FILTER_TENT, 0.49, 0.0, 0), b"radius"), ((A.FILTER_TENT, 4.01, 0.0, 0), b"radius"), ((A.FILTER_TENT, nan, 0.0, 0), b"radius"),
           ((A.FILTER_BLACKMAN_HARRIS, inf, 0.0, 0), b"radius"), ((A.FILTER_GAUSSIAN, -1.0, 0.5, 0), b"radius"),
           ((A.FILTER_GAUSSIAN, 1.5, 0.0, 0), b"sigma"), ((A.FILTER_GAUSSIAN, 1.5, -0.5, 0), b"sigma"), ((A.FILTER_GAUSSIAN, 1.5, nan, 0), b"sigma"),
           ((A.FILTER_GAUSSIAN, 1.5, inf, 0), b"sigma"),
           ((A.FILTER_TENT, 2.0, 0.0, 1), b"reserved"), ((A.FILTER_BOX, 0.0, 0.0, -1), b"reserved")]
    for fields, word in bad:
        f = A.PixelFilter(*fields)
        assert lib.kyhip_filter_check(C.byref(f)) == A.KY_ERR_INVALID_VALUE and word in lib.kyhip_last_error(), fields
    assert lib.kyhip_filter_check(None) == A.KY_ERR_INVALID_VALUE
    good = [(A.FILTER_BOX, 0.0, 0.0, 0), (A.FILTER_BOX, 99.0, nan, 0), (A.FILTER_TENT, 0.5, nan, 0), (A.FILTER_TENT, 4.0, -3.0, 0), (A.FILTER_GAUSSIAN, 0.5, 1e-3, 0),
            (A.FILTER_GAUSSIAN, 4.0, 1e3, 0), (A.FILTER_BLACKMAN_HARRIS, 2.0, 0.0, 0)]
    for fields in good:   # a box's radius and a param the kind does not read are not looked at
        assert lib.kyhip_filter_check(C.byref(A.PixelFilter(*fields))) == A.KY_OK, fields
    # the entries that take a filter refuse a bad one before anything else
    f = A.PixelFilter(A.FILTER_TENT, 9.0, 0.0, 0)
    out = np.zeros(A.FILTER_TABLE + 1, np.float32)
    assert lib.kyhip_filter_table(C.byref(f), out.ctypes.data_as(C.c_void_p), out.size) == A.KY_ERR_INVALID_VALUE and (out == 0).all()
    assert lib.kyhip_frame_set_filter(None, C.byref(f)) == A.KY_ERR_INVALID_VALUE and b"radius" in lib.kyhip_last_error()
    ok = A.PixelFilter(A.FILTER_TENT, 2.0, 0.0, 0)
    assert lib.kyhip_frame_set_filter(None, C.byref(ok)) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_filter_table(C.byref(ok), out.ctypes.data_as(C.c_void_p), out.size - 1) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_filter_table(C.byref(ok), None, out.size) == A.KY_ERR_INVALID_VALUE


@pytest.mark.parametrize("kind,radius,param", CASES)
def test_table_is_the_restatements(api, kind, radius, param):
    """Both sides invert the analytic CDF in double and round once to float32: they agree to one float32 ulp of R (in fact they are equal but at the middle
    entry, which the library sets to exactly 0 and the bisection leaves within 1e-16 of it)."""
    f, flt = both(api, kind, radius, param)
    got, want = api.filter_table(f), F.table(flt)
    ulp = float(np.spacing(np.float32(flt.radius)))
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(flt, "largest difference %.3g, one ulp of R %.3g" % (worst, ulp))
    assert got.dtype == np.float32 and got.shape == (F.TABLE + 1,) and worst <= ulp


@pytest.mark.parametrize("kind,radius,param", CASES)
def test_table_shape_and_offsets(api, kind, radius, param):
    """Monotone, symmetric, the ends exactly -R and +R; and every offset the warp produces from it lies in [0.5 - R, 0.5 + R]."""
    f, flt = both(api, kind, radius, param)
    t = api.filter_table(f)
    R_ = np.float32(flt.radius)
    assert t[0] == -R_ and t[-1] == R_ and t[F.TABLE // 2] == 0
    assert (np.diff(t) >= 0).all() and np.array_equal(t, -t[::-1])
    gen = np.random.default_rng(7)
    u = np.concatenate([np.array([0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24], np.float32), np.arange(F.TABLE, dtype=np.float32) / F.TABLE,
                        np.nextafter(np.arange(1, F.TABLE + 1, dtype=np.float32) / F.TABLE, np.float32(0)), gen.random(1 << 14, dtype=np.float32)])
    o = F.warp(flt, u, tab=t)
    assert o.dtype == np.float32 and (o >= np.float32(0.5) - R_).all() and (o <= np.float32(0.5) + R_).all()
    order = np.argsort(u, kind="stable")
    assert (np.diff(o[order].astype(np.float64)) >= -float(np.spacing(R_))).all()   # monotone in u (the tent's two branches meet within an ulp at 0.5)
    assert F.warp(flt, np.float32(0.5), tab=t) == np.float32(0.5)                   # the debug sampler's number is the pixel's centre under every filter


# max |F(x(u)) - u| over 2^16 values of u for the library's 256-interval table, measured here on the CPU (this file, 2026-10): 1.225e-3, 1.777e-3, 1.800e-3.
# The deviation falls only linearly with the table's size -- these densities vanish at +-R -- and is what the issue that introduced the filters quotes as
# 1.2e-3, 1.8e-3, 1.8e-3; the bound is 1.5 x those: the margin is over the analytic reference and covers only the grid of u.
DEVIATION = (((F.GAUSSIAN, 1.5, 0.5), 1.2e-3), ((F.GAUSSIAN, 4.0, 1.0), 1.8e-3), ((F.BLACKMAN_HARRIS, 2.0, 0.0), 1.8e-3))


@pytest.mark.parametrize("case,measured", DEVIATION)
def test_table_strays_from_the_analytic_cdf_as_measured(api, case, measured):
    """Gaussian sigma 0.5 R 1.5: 1.225e-3; Gaussian sigma 1 R 4: 1.777e-3; Blackman-Harris R 2: 1.800e-3 (DESIGN.md section 11 has the same three)."""
    f, flt = both(api, *case)
    d = F.table_deviation(flt, api.filter_table(f))
    print(flt, "deviation %.4g, recorded %.4g" % (d, measured))
    assert d <= 1.5 * measured
    assert d >= 0.5 * measured   # (and it is no smaller table's figure: 64 intervals give 5.5e-3 .. 7.8e-3, 1024 a quarter of this)


def test_tent_table_is_the_closed_form(api):
    f, flt = both(api, F.TENT, 2.0, 0.0)
    u = np.arange(F.TABLE + 1, dtype=np.float64) / F.TABLE
    want = 2.0 * np.where(u < 0.5, np.sqrt(2 * u) - 1, 1 - np.sqrt(2 - 2 * u))
    assert np.abs(api.filter_table(f) - want).max() <= float(np.spacing(np.float32(2.0)))


def test_screen_bound_under_a_filter_is_the_plain_one_grown(A, api):
    w, h = 96, 72   # tests/test_screen_cull_gpu.py's frame: dead blocks on both sides of the box
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    p = api.make_params(w, h, 4)
    (x0, y0, x1, y1), dead, total = api.scene_screen_bound(scene, p)
    assert dead > 0 and x0 >= 8
    assert api.scene_screen_bound(scene, p, filter=api.pixel_filter(A.FILTER_BOX)) == ((x0, y0, x1, y1), dead, total)
    for radius, g in ((0.5, 0), (0.75, 1), (1.5, 1), (2.0, 2), (2.5, 2), (4.0, 4)):
        rect, d, t = api.scene_screen_bound(scene, p, filter=api.pixel_filter(A.FILTER_TENT, radius))
        assert rect == (max(x0 - g, 0), max(y0 - g, 0), min(x1 + g, w), min(y1 + g, h)) and t == total and d <= dead, (radius, rect)


# ---- centring and semantics, on the oracle alone ----
# KY_INTEGRATOR_BASECOLOR: a sample depends on its camera ray only.  Two quadratures of one integral, the 16 x 16 Cornell frame's pixel (x, y) under the filter f:
#   (a) kyo_li_tape fed a regular 16 x 16 grid of u through the restatement's warp -- midpoints in u, equal weights: what the filtered kernels estimate;
#   (b) the oracle's own 16x-supersampled box picture (and four pixels of margin, traced through pixel 0 with offsets outside [0, 1): the oracle adds the tape's
#       first two numbers to the pixel's corner whatever they are), weighted by the analytic density centred on the pixel's CENTRE.
# Measured here (tools/measure_tolerances.py filter): RMSE over the frame's 768 values 2.41e-3 for the tent of radius 2, 1.87e-3 for the default Gaussian; the
# bound is twice that.  A warp centred on the pixel's corner (shift -0.5) measures 2.39e-2 and 3.25e-2: ten times the bound, and the test rejects it below.
SUB = 16
CENTRING = ((F.TENT, 2.0, 0.0, 2.41e-3), (F.GAUSSIAN, 1.5, 0.5, 1.87e-3))


@pytest.fixture(scope="module")
def basecolor(O, A, api):
    w = h = 16
    margin = 4
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    params = api.make_params(w, h, 1, integrator=A.INTEGRATOR_BASECOLOR)
    n = (w + 2 * margin) * SUB
    X = (np.arange(n) + 0.5) / SUB - margin
    tape = np.zeros((n * n, 4), np.float32)
    tape[:, 0], tape[:, 1] = np.tile(X, n), np.repeat(X, n)
    fine = O.li_tape(scene, params, 0, 0, tape)[0].reshape(n, n, 3).astype(np.float64)
    fine.setflags(write=False)
    return scene, params, X, fine


def centring_reference(basecolor, flt):
    scene, params, X, fine = basecolor
    out = np.zeros((params.height, params.width, 3))
    for y in range(params.height):
        wy = F.density(flt, X - (y + 0.5))
        for x in range(params.width):
            wx = F.density(flt, X - (x + 0.5))
            out[y, x] = np.einsum("j,i,jic->c", wy, wx, fine) / (wy.sum() * wx.sum())
    return out


def centring_filtered(O, basecolor, flt, shift=0.0):
    scene, params, X, fine = basecolor
    o = F.warp(flt, ((np.arange(SUB) + 0.5) / SUB).astype(np.float32), shift=shift)
    tape = np.zeros((SUB * SUB, 4), np.float32)
    tape[:, 0], tape[:, 1] = np.tile(o, SUB), np.repeat(o, SUB)
    out = np.zeros((params.height, params.width, 3))
    for y in range(params.height):
        for x in range(params.width):
            out[y, x] = O.li_tape(scene, params, x, y, tape)[0].astype(np.float64).mean(axis=0)
    return out


def centring_rmse(O, basecolor, flt, shift=0.0):
    return float(np.sqrt(np.mean((centring_filtered(O, basecolor, flt, shift) - centring_reference(basecolor, flt)) ** 2)))


@pytest.mark.parametrize("kind,radius,param,measured", CENTRING)
def test_the_warp_renders_the_filter_centred_on_the_pixel(O, basecolor, kind, radius, param, measured):
    flt = F.Filter(kind, radius, param)
    e = centring_rmse(O, basecolor, flt)
    print(flt, "rmse %.4g, measured %.4g, allowed %.4g" % (e, measured, 2 * measured))
    assert basecolor[3].max() > 0.1 and e < 2 * measured


@pytest.mark.parametrize("kind,radius,param,measured", CENTRING)
def test_a_filter_centred_on_the_corner_is_rejected(O, basecolor, kind, radius, param, measured):
    """The named defect: offsets in [-R, R] around the pixel's corner instead of [0.5 - R, 0.5 + R] around its centre."""
    flt = F.Filter(kind, radius, param)
    e = centring_rmse(O, basecolor, flt, shift=-0.5)
    print(flt, "shifted: rmse %.4g against a bound of %.4g" % (e, 2 * measured))
    assert e > 4 * (2 * measured)
