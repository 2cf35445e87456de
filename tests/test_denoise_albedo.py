"""CPU: albedo demodulation in a frame's denoise filter (ky_amd/csrc/ky_denoise.hpp, demodulate_pixel / remodulate_pixel; DESIGN.md "Denoise", "Albedo").  The
header's functions run here as host code (kyhostcheck_denoise_albedo, ky_amd/csrc/ky_hostcheck.cpp) against the NumPy restatement of
tests/denoise_albedo_restatement.py, and the feature's claim -- on textured surfaces the demodulated filter beats today's filter and the unfiltered mean -- is
replayed on the CPU oracle alone, with the named defects each shown failing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_albedo_restatement as DA
import denoise_restatement as D
import noise_restatement as R
import texture_restatement as X
from test_denoise import PIX, _buffers
from test_denoise_chains import _keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_denoise_albedo: the sanitizer build when the suite runs inside `make sanitize`, else the same sources built plainly."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    for name in ("kyhostcheck_denoise", "kyhostcheck_denoise_albedo"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = A.KYHOSTCHECK_SYMBOLS[name]
    return lib


def _albedo(w, h, seed):
    """Albedos around a checker of two colours, with every special value on class-0 pixels and elsewhere: 0, values below 1/64 (negative ones too), exactly 1/64,
    values above 1"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    a = np.where((((xs // 3) + (ys // 2)) & 1)[..., None] == 0, [0.30, 0.28, 0.05], [0.04, 0.06, 0.25]) * rng.uniform(0.8, 1.2, (h, w, 3))
    special = rng.random((h, w, 3))
    a = np.where(special < 0.05, 0.0, a)
    a = np.where((special >= 0.05) & (special < 0.10), rng.uniform(-0.01, 1.0 / 64, (h, w, 3)), a)
    a = np.where((special >= 0.10) & (special < 0.15), rng.uniform(1.0, 3.0, (h, w, 3)), a)
    a = np.where((special >= 0.15) & (special < 0.17), 1.0 / 64, a)
    return np.concatenate([a, rng.integers(0, 17, (h, w, 1))], axis=2).astype(np.float32)


def _host(check, A, cv, ga, gb, key, albedo, levels):
    h, w = cv.shape[:2]
    q = A.DenoiseParams(levels, *(D.DEFAULTS[k] for k in ("normal_squarings", "sigma_luminance", "sigma_plane")))
    out = np.zeros((h, w, 4), np.float32)
    arrays = [np.ascontiguousarray(a, np.float32) for a in (cv, ga, gb)]
    keys = None if key is None else np.ascontiguousarray(key, np.uint64)
    al = np.ascontiguousarray(albedo, np.float32)
    rc = check.kyhostcheck_denoise_albedo(*(a.ctypes.data for a in arrays), None if keys is None else keys.ctypes.data, al.ctypes.data, w, h, C.byref(q), PIX,
                                          out.ctypes.data)
    assert rc == A.KY_OK
    return out


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "keyed"])
@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("w,h", [(40, 24), (44, 21)])
def test_host_build_against_the_restatement(w, h, levels, keyed, A, check):
    """tests/test_denoise.py's bound, levels x 2^-23, plus one float32 rounding each for demodulate and remodulate: rtol = (levels + 2) x 2^-23, atol = 0.  Both
    sides divide and multiply in double and round once, so the expectation is 0.  Measured: 0 in all twelve cases (printed)."""
    cv, ga, gb = _buffers(w, h, 11 * w + levels)
    key = _keys(w, h, 3 * w + levels)[0] if keyed else None
    albedo = _albedo(w, h, 7 * w + levels)
    surface = gb[..., 3] == D.SURFACE
    a3 = albedo[..., :3][surface]
    assert (a3 == 0).any() and ((a3 < 1.0 / 64) & (a3 != 0)).any() and (a3 > 1).any() and (a3 == np.float32(1.0 / 64)).any()
    assert {int(c) for c in np.unique(gb[..., 3])} == {0, 1, 2, 3}
    got = _host(check, A, cv, ga, gb, key, albedo, levels)
    want = DA.denoise(cv, ga, gb, albedo, PIX, key=key, levels=levels)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert np.array_equal(got[~surface], cv[~surface])
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = float((err / np.maximum(np.abs(want.astype(np.float64)), 1e-300)).max())
    print("largest relative |host - restatement| (%d x %d, %d levels, %s): %.3e" % (w, h, levels, "keyed" if keyed else "plain", rel))
    assert (err <= (levels + 2) * 2.0 ** -23 * np.abs(want.astype(np.float64))).all(), rel
    assert not np.array_equal(want, D.denoise(cv, ga, gb, PIX, levels=levels))   # (the albedo is seen)


@pytest.mark.parametrize("levels", [1, 5])
def test_an_albedo_of_ones_is_the_plain_filter(levels, A, check):
    """c / 1, v / Y(1)^2 and c x 1 are exact ... where Y(1) is 1: the three weights sum to 1.0 in double exactly as written (0.212671 + 0.715160 + 0.072169)."""
    w, h = 40, 24
    cv, ga, gb = _buffers(w, h, 3)
    assert 0.212671 + 0.715160 + 0.072169 == 1.0
    q = A.DenoiseParams(levels, *(D.DEFAULTS[k] for k in ("normal_squarings", "sigma_luminance", "sigma_plane")))
    plain = np.zeros((h, w, 4), np.float32)
    assert check.kyhostcheck_denoise(cv.ctypes.data, ga.ctypes.data, gb.ctypes.data, w, h, C.byref(q), PIX, plain.ctypes.data) == A.KY_OK
    ones = np.ones((h, w, 4), np.float32)
    assert _host(check, A, cv, ga, gb, None, ones, levels).tobytes() == plain.tobytes()


def test_pass_through_classes(A, check):
    """Classes 1, 2 and 3 come out bit for bit whatever their albedo says, NaN and infinity included"""
    w, h = 44, 21
    cv, ga, gb = _buffers(w, h, 9)
    albedo = _albedo(w, h, 5)
    other = gb[..., 3] != D.SURFACE
    albedo[other] = np.random.default_rng(1).choice(np.array([0.0, np.nan, np.inf, -1.0, 1e-30, 5.0], np.float32), (int(other.sum()), 4))
    for key in (None, _keys(w, h, 2)[0]):
        got = _host(check, A, cv, ga, gb, key, albedo, 3)
        assert got[other].tobytes() == cv[other].tobytes() and not np.array_equal(got[~other], cv[~other])


def test_arguments_are_refused_before_any_device(A):
    lib = A.load_kyhip()
    buf = np.full((4, 4, 4), 7.0, np.float32)
    for grid in (-1, A.ALBEDO_MAX_GRID + 1):
        assert lib.kyhip_frame_set_albedo_grid(None, grid) == A.KY_ERR_INVALID_VALUE and b"albedo grid" in lib.kyhip_last_error()
    assert lib.kyhip_frame_set_albedo_grid(None, 4) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_albedo_grid(None) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_frame_albedo(None, C.c_void_p(buf.ctypes.data), 4) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    ms = C.c_float(7)
    assert lib.kyhip_frame_albedo_ms(None, C.byref(ms)) == A.KY_ERR_INVALID_VALUE and ms.value == 7
    assert (buf == 7).all()
    header = open(os.path.join(ROOT, "include", "kyhip.h")).read()
    assert "#define KYHIP_ALBEDO_MAX_GRID %d\n" % A.ALBEDO_MAX_GRID in header


# ---- the claim, replayed on the oracle ----

W, H, SPP = 40, 24, 500
SEEDS = (1234, 101, 202)
AT = (112, 224)
TRUTH_SPP = 2048


@pytest.fixture(scope="module")
def replayed(A, api, O):
    """tests/texture_restatement.py's cornell_case cut into constant-colour tiles, the three seeds replayed up to 224 samples, the oracle's truth, guides and
    albedos (grid 4; grid 4 with u and v swapped) -- computed once"""
    scene, textures = X.cornell_case(A, api, W, H)
    tiled = X.tiled(A, scene.scene, textures)
    truth = O.render(tiled, api.make_params(W, H, TRUTH_SPP, seed=987654)).astype(np.float64)
    ga, gb = D.guides_from_hits(tiled.scene, O.kat_scene_intersect(tiled, D.centre_rays(O.kat_camera, tiled.scene.camera, W, H)), W, H)
    albedo, _, _ = DA.albedo(O, A, scene, textures, W, H, 4, check_clean=False)
    swapped, _, _ = DA.albedo(O, A, scene, textures, W, H, 4, swap=True, check_clean=False)
    first = DA.albedo(O, A, scene, textures, W, H, 1, check_clean=False)[2][..., 0]
    by_material = {t.material for t in textures}
    textured = np.isin(first, [s for s in range(scene.scene.surface_count) if scene.scene.surfaces[s].material in by_material])
    frames = {seed: DA.replay(O, api, R, tiled, W, H, SPP, seed, AT) for seed in SEEDS}
    return dict(truth=truth, ga=ga, gb=gb, albedo=albedo, swapped=swapped, textured=textured, frames=frames, pix=D.pixel_width(tiled.scene.camera, W))


def test_demodulation_beats_todays_filter_on_textured_surfaces(replayed):
    """On the oracle and the NumPy restatement ALONE: this test runs no line of ky_denoise.hpp -- the header's arithmetic is held to the restatement by
    test_host_build_against_the_restatement above and by the GPU tests -- and the named defects are injected into the restatement, not into the header.  What it
    protects is the claim the feature was built on and the restatement's own power to tell a right rule from a wrong one.
    RMSE over the pixels whose centre ray first hits a textured surface (320 of 960), against the oracle at 2048 samples -- the count at which the truth takes
    about two seconds on eight cores; its own noise (about 1 / sqrt(2048 / 224) = a third of the raw error at 224 samples) is added to all three errors alike, so
    the ratios printed here are nearer 1 than those against a 16 384-sample truth (tools/denoise_replay.py albedo; DESIGN.md "Albedo").  Measured:
    demodulated / today's 0.79 .. 0.89, demodulated / raw 0.60 .. 0.88 over the six (seed, count) cases (today's / raw is above 1 at 224 samples for seed 1234).
    Each named defect loses to the filter without it in every case: remodulating with a (on an albedo whose blue channel is black) 0.086 .. 0.098 against
    0.040 .. 0.065, no variance scale 0.4 .. 16 % worse, u and v swapped 32 .. 77 % worse."""
    r = replayed
    sel = r["textured"]
    assert int(sel.sum()) == 320
    for seed in SEEDS:
        for d in AT:
            cv = r["frames"][seed][d]
            e = lambda film: DA.rmse(film, r["truth"], sel)
            raw, today = e(cv), e(D.denoise(cv, r["ga"], r["gb"], r["pix"], **D.DEFAULTS))
            demod = e(DA.denoise(cv, r["ga"], r["gb"], r["albedo"], r["pix"], **D.DEFAULTS))
            print("seed %d at %d: raw %.5f today %.5f demodulated %.5f: / today %.3f, / raw %.3f" % (seed, d, raw, today, demod, demod / today, demod / raw))
            assert demod < today and demod < raw
            zeroed = r["albedo"].copy()
            zeroed[..., 2] = 0.0   # (a black channel: where a and a' differ)
            defects = {"remodulated with a": (e(DA.denoise(cv, r["ga"], r["gb"], zeroed, r["pix"], remodulate_floor=False, **D.DEFAULTS)),
                                              e(DA.denoise(cv, r["ga"], r["gb"], zeroed, r["pix"], **D.DEFAULTS))),
                       "no variance scale": (e(DA.denoise(cv, r["ga"], r["gb"], r["albedo"], r["pix"], variance="none", **D.DEFAULTS)), demod),
                       "u and v swapped": (e(DA.denoise(cv, r["ga"], r["gb"], r["swapped"], r["pix"], **D.DEFAULTS)), demod)}
            for name, (bad, good) in defects.items():
                print("    %s: %.5f against %.5f" % (name, bad, good))
                assert bad > good, name
