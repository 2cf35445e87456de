"""CPU: the denoiser's specular-chain guides (include/kyhip.h, kyhip_frame_set_guide_bounces; DESIGN.md "Denoise", "Guides beyond the first hit").  The keyed level of
ky_amd/csrc/ky_denoise.hpp (level_pixel_t<true>: taps share the pixel's chain key) runs here as host code (kyhostcheck_denoise_keyed, ky_amd/csrc/ky_hostcheck.cpp)
against the NumPy restatement of tests/denoise_chains_restatement.py; the chain walk runs on the CPU oracle's per-vertex traces and is pinned as a fixture the GPU
test reads (tests/golden/denoise_chains.npz); and the new entry points refuse what they must before any device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_chains_restatement as DC
import denoise_restatement as D
from test_denoise import PIX, _buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_denoise and kyhostcheck_denoise_keyed: tests/test_denoise.py's."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    for name in ("kyhostcheck_denoise", "kyhostcheck_denoise_keyed"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = A.KYHOSTCHECK_SYMBOLS[name]
    return lib


def _keys(w, h, seed, singletons=12):
    """Three key values in patches -- 0 around, a disc of one chain, a band of another that the disc cuts -- plus scattered pixels whose key nobody shares."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    key = np.zeros((h, w), np.uint64)
    key[(xs - 0.3 * w) ** 2 + (ys - 0.5 * h) ** 2 < (0.3 * h) ** 2] = 0xC
    key[(xs > 0.55 * w) & (ys > 0.2 * h) & (ys < 0.8 * h)] = 0x3C0F
    key[(xs - 0.6 * w) ** 2 + (ys - 0.5 * h) ** 2 < (0.12 * h) ** 2] = 0xC
    lone = rng.choice(w * h, singletons, replace=False)
    key.ravel()[lone] = DC.UNRESOLVED + 1 + np.arange(singletons, dtype=np.uint64)
    return key, np.unravel_index(lone, (h, w))


def _host(check, A, cv, ga, gb, key, levels):
    h, w = cv.shape[:2]
    q = A.DenoiseParams(levels, *(D.DEFAULTS[k] for k in ("normal_squarings", "sigma_luminance", "sigma_plane")))
    out = np.zeros((h, w, 4), np.float32)
    arrays = [np.ascontiguousarray(a, np.float32) for a in (cv, ga, gb)]
    if key is None:
        rc = check.kyhostcheck_denoise(*(a.ctypes.data for a in arrays), w, h, C.byref(q), PIX, out.ctypes.data)
    else:
        key = np.ascontiguousarray(key, np.uint64)
        rc = check.kyhostcheck_denoise_keyed(*(a.ctypes.data for a in arrays), key.ctypes.data, w, h, C.byref(q), PIX, out.ctypes.data)
    assert rc == A.KY_OK
    return out


@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("w,h", [(40, 24), (44, 21)])
def test_keyed_host_build_against_the_restatement(w, h, levels, A, check):
    """tests/test_denoise.py's buffers (all four classes) with keys in patches and scattered singletons, and its bound: float32 stored from double on both sides,
    non-negative weights and colours, so rtol = levels x 2^-23, atol = 0.  The keys change the result: the plain filter gives other bytes."""
    cv, ga, gb = _buffers(w, h, 11 * w + levels)
    key, _ = _keys(w, h, 7 * w + levels)
    got = _host(check, A, cv, ga, gb, key, levels)
    want = DC.denoise(cv, ga, gb, key, PIX, levels=levels)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    surface = gb[..., 3] == D.SURFACE
    assert {int(c) for c in np.unique(gb[..., 3])} == {0, 1, 2, 3} and len(np.unique(key)) >= 3 + 10
    assert np.array_equal(got[~surface], cv[~surface])            # pass-through: to the bit
    assert not np.array_equal(got, _host(check, A, cv, ga, gb, None, levels))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = float((err / np.maximum(np.abs(want.astype(np.float64)), 1e-300)).max())
    print("largest relative |keyed host - restatement| (%d x %d, %d levels): %.3e" % (w, h, levels, rel))
    assert (err <= levels * 2.0 ** -23 * np.abs(want.astype(np.float64))).all(), rel


@pytest.mark.parametrize("value", [0, 0xC, DC.UNRESOLVED | 0xF])
def test_all_keys_equal_is_the_plain_filter(value, A, check):
    """One key everywhere is no condition at all: kyhostcheck_denoise's bytes, and the keyed restatement is the plain one."""
    cv, ga, gb = _buffers(44, 21, 3)
    key = np.full((21, 44), value, np.uint64)
    assert np.array_equal(_host(check, A, cv, ga, gb, key, 5), _host(check, A, cv, ga, gb, None, 5))
    assert np.array_equal(DC.denoise(cv, ga, gb, key, PIX), D.denoise(cv, ga, gb, PIX))


def test_a_key_nobody_shares_passes_through(A, check):
    """Its only tap, and its prefilter's only neighbour, is itself: c' = w c / w and v' = w^2 v / w^2 in double, stored as the float32 they came from."""
    cv, ga, gb = _buffers(40, 24, 9)
    key, lone = _keys(40, 24, 9)
    gb[..., 3][lone] = D.SURFACE
    got = _host(check, A, cv, ga, gb, key, 5)
    assert np.array_equal(got[lone], cv[lone]) and len(lone[0]) == 12
    shared = (key == 0xC) & (gb[..., 3] == D.SURFACE)
    assert not np.array_equal(got[shared], cv[shared])


def test_the_oracles_chains(A, api, O):
    """The chains of the default Cornell 40 x 24 from the CPU oracle's trace_li (debug sampler, max_path_depth 8), regenerated and compared with the committed
    fixture: 76 pixels first hit a ball, 68 of their chains end on a surface and 8 leave the box, 5 distinct keys on the film (0 among them) at four bounces.  At
    one bounce the glass ball's refracted chains are unresolved: bit 62, the first digit, and the first hit's guides."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_denoise_chains as M
    finally:
        sys.path.remove(GOLDEN)
    scene, trace = M.oracle_trace()
    made = M.oracle_chains(scene, trace)
    stored = np.load(os.path.join(GOLDEN, "denoise_chains.npz"))
    assert sorted(stored.files) == sorted(made)
    for name in made:
        if name.startswith(("key", "cls")):
            assert np.array_equal(made[name], stored[name]), name
        else:
            assert np.allclose(made[name], stored[name], rtol=1e-6, atol=1e-6), name
    cls, key = stored["cls_4"], stored["key_4"]
    assert DC.counts(cls, key) == (76, 68, 8, 4) and len(np.unique(key)) == 5 and not (key >> np.uint64(62)).any()
    # the walk at 0 bounces is the first hit: every chain pixel there is "unresolved", a mirror or glass, and nothing else is
    plain_cls, plain_key, plain_ga, plain_gb = DC.chains(trace, scene.c, M.W, M.H, 0)
    assert np.array_equal(plain_key != 0, key != 0) and (plain_cls[key != 0] == D.SURFACE).all()
    one = stored["key_1"]
    unresolved = (one >> np.uint64(62)) != 0
    assert unresolved.any() and (one[unresolved] & np.uint64(0x3FF) == key[unresolved] & np.uint64(0x3FF)).all()
    assert np.array_equal(stored["ga_1"][unresolved], plain_ga[unresolved]) and np.array_equal(stored["gb_1"][unresolved], plain_gb[unresolved])
    assert (stored["cls_1"][unresolved] == D.SURFACE).all()


def test_arguments_are_refused_before_any_device(A):
    lib = A.load_kyhip()
    for bad in (-1, A.GUIDE_MAX_BOUNCES + 1):
        assert lib.kyhip_frame_set_guide_bounces(None, bad) == A.KY_ERR_INVALID_VALUE and b"guide bounces" in lib.kyhip_last_error()
    for fine in range(A.GUIDE_MAX_BOUNCES + 1):       # the value passes: the frame is what is missing
        assert lib.kyhip_frame_set_guide_bounces(None, fine) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_guide_bounces(None) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    keys = np.full((4, 4), 7, np.uint64)
    assert lib.kyhip_frame_guide_chains(None, C.c_void_p(keys.ctypes.data), 4) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert (keys == 7).all() and A.GUIDE_MAX_BOUNCES == 4


def test_the_header_and_the_bindings_agree(A):
    with open(os.path.join(ROOT, "include", "kyhip.h")) as f:
        text = f.read()
    assert "#define KYHIP_GUIDE_MAX_BOUNCES %d\n" % A.GUIDE_MAX_BOUNCES in text and "#define KYHIP_ABI_VERSION 4 " in text
    assert DC.MAX_BOUNCES == A.GUIDE_MAX_BOUNCES and DC.UNRESOLVED == A.GUIDE_KEY_UNRESOLVED
