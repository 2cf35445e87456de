"""SURVEY 8(f)4, pinned by the reference itself: smallpt2pbrt/smallpt_rewrite.cpp is the one program of the reference that this
image's toolchain builds unmodified (oracle/Makefile `ref` -> oracle/_ref/smallpt_rewrite).

Chain of evidence:
  reference binary  ==(every byte of its 1024 x 768 image)==  oracle/smallpt_rewrite_oracle.cpp with the reference's own
  std::mt19937_64 stream (rng_mode 1)                                  [CPU tests below; committed fixture for boxes without _ref]
  the same oracle code with per-sample splitmix64 streams (rng_mode 0)  ==(1e-9 per sample)==  the HIP fp64 path, variant 1
                                                                        [GPU tests below]
  and the HIP film against the reference's own 256-spp image, statistically.
"""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "smallpt_rewrite_16.npz")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "smallpt_rewrite")


def _params(A, w, h, spp, seed=1234, max_depth=10):
    return A.SmallptParams(w, h, spp, seed, max_depth, A.SP_VARIANT_REWRITE)


def _decode_bmp(raw):
    off = int.from_bytes(raw[10:14], "little")
    w = int.from_bytes(raw[18:22], "little", signed=True)
    h = int.from_bytes(raw[22:26], "little", signed=True)
    px = np.frombuffer(raw[off:off + w * h * 3], np.uint8).reshape(h, w, 3)
    return np.ascontiguousarray(px[::-1, :, ::-1])


@pytest.fixture(scope="module")
def oracle_image_16(A, O):
    """The oracle's restatement with the reference's generator at the reference's fixed size, argv[1] = 16 -> 4 spp."""
    film = O.sprw_render(O.sprw_scene(), _params(A, 1024, 768, 4), rng_mode=1)
    return O.sprw_gamma_bytes(film)


def test_scene_tables_agree(A, O):
    mine = (A.SmallptSphere * 9)()
    assert A.load_kyhip().kyhip_smallpt_scene_rewrite(mine) == 9
    ref = O.sprw_scene()
    assert bytes(mine) == bytes(ref)
    # smallpt_rewrite.cpp:1201-1211 is smallpt.cpp:42-52 mirrored in z
    sp = O.smallpt_scene()
    for a, b in zip(ref, sp):
        assert a.rad == b.rad and a.p[0] == b.p[0] and a.p[1] == b.p[1] and list(a.c) == list(b.c) and a.refl == b.refl
    assert [s.p[2] for s in ref] == [-81.6, -81.6, -1e5, 1e5 - 170, -81.6, -81.6, -47, -78, -81.6]


def test_oracle_matches_committed_reference_image(oracle_image_16):
    """Byte-exact against what the reference binary wrote (fixture made by tests/golden/make_smallpt_rewrite_fixture.py)."""
    g = np.load(GOLD)
    assert hashlib.sha256(oracle_image_16.tobytes()).digest() == g["sha256"].tobytes()
    assert np.array_equal(oracle_image_16[352:384], g["band"])


def test_oracle_matches_reference_binary_run_here(oracle_image_16, A, O):
    """Where oracle/_ref/smallpt_rewrite is not built (`make -C oracle ref` needs the reference tree), against what that binary wrote when
    the committed fixture was made: the SHA-256 of its image and the BMP layout (header, length) it recorded."""
    if not os.path.exists(REF_EXE):
        g = np.load(GOLD)
        assert hashlib.sha256(oracle_image_16.tobytes()).digest() == g["sha256"].tobytes()
        assert int.from_bytes(g["header"].tobytes()[18:22], "little") == 1024 and int.from_bytes(g["header"].tobytes()[22:26], "little") == 768
        assert int(g["file_bytes"]) == 54 + oracle_image_16.size
        return
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call([REF_EXE, "16"], cwd=d, stderr=subprocess.DEVNULL)
        raw = open(os.path.join(d, "image.bmp"), "rb").read()
    ref = _decode_bmp(raw)
    assert ref.shape == (768, 1024, 3)
    mism = int((ref != oracle_image_16).sum())
    assert mism == 0, f"{mism} of {ref.size} bytes differ from the reference binary's image"
    g = np.load(GOLD)
    assert bytes(raw[:54]) == g["header"].tobytes() and len(raw) == int(g["file_bytes"])


def test_oracle_rng_modes_converge(A, O):
    """The per-sample splitmix64 streams (what the HIP path uses) estimate the same image as the reference's own generator."""
    sp = O.sprw_scene()
    p = _params(A, 64, 48, 1024, seed=11)
    a, b = O.sprw_render(sp, p, 0), O.sprw_render(sp, p, 1)
    blocks = lambda im: im.reshape(6, 8, 8, 8, 3).mean(axis=(1, 3))
    d = np.abs(blocks(a) - blocks(b))
    # mode 1 replays ONE stream in every image row (Sampler::Clone, 1300): its noise is correlated down the columns of a block
    assert d.max() < 0.08 and d.mean() < 0.012, (d.max(), d.mean())
    # per-sample entry point = the film's own samples
    li = O.sprw_radiance(sp, p, 20, 30, 0, 1024)
    assert np.allclose(np.clip(li.mean(axis=0), 0, 1), a[30, 20], rtol=1e-12, atol=1e-15)


def test_abi_validation_host_side(A):
    lib = A.load_kyhip()
    sp = (A.SmallptSphere * 9)()
    lib.kyhip_smallpt_scene_rewrite(sp)
    img = np.zeros((8, 8, 3))
    bad = A.SmallptParams(8, 8, 1, 1, 10, 7)
    assert lib.kyhip_smallpt_render(0, sp, 9, C.byref(bad), img.ctypes.data_as(C.c_void_p)) == A.KY_ERR_INVALID_VALUE
    assert b"variant" in lib.kyhip_last_error()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_per_sample_radiance_matches_oracle(A, api, O):
    sp, spo = api.smallpt_scene_rewrite(), O.sprw_scene()
    p = api.smallpt_params(256, 192, 64, variant=A.SP_VARIANT_REWRITE)
    worst = 0.0
    for (x, y) in ((128, 96), (70, 150), (185, 140), (10, 10), (128, 4), (250, 100), (60, 130), (200, 160)):   # walls, mirror, glass, light
        g = api.smallpt_kat_radiance(sp, p, x, y, 0, 0, 0, 512)
        c = O.sprw_radiance(spo, p, x, y, 0, 512)
        assert np.isfinite(g).all()
        rel = np.abs(g - c) / np.maximum(1e-12, np.abs(c).max(axis=1, keepdims=True))
        # a path can differ only where libm and the device's cos/sin round differently AND a comparison flips on it
        assert (rel.max(axis=1) < 1e-9).mean() >= 0.998, (x, y, rel.max())
        worst = max(worst, float(np.median(rel.max(axis=1))))
    assert worst < 1e-12
    for md in (0, 1, 3):
        q = api.smallpt_params(64, 48, 4, seed=5, max_depth=md, variant=A.SP_VARIANT_REWRITE)
        g = api.smallpt_kat_radiance(sp, q, 46, 35, 0, 0, 0, 256)
        c = O.sprw_radiance(spo, q, 46, 35, 0, 256)
        assert np.allclose(g, c, rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_gpu_film_matches_oracle_film(A, api, O):
    sp, spo = api.smallpt_scene_rewrite(), O.sprw_scene()
    p = api.smallpt_params(128, 96, 64, seed=3, variant=A.SP_VARIANT_REWRITE)
    g = api.smallpt_render(sp, p)
    c = O.sprw_render(spo, p, 0)
    assert g.shape == c.shape == (96, 128, 3)
    rmse = float(np.sqrt(np.mean((g - c) ** 2)))
    assert rmse < 1e-9, rmse          # same streams, same arithmetic: only the summation order of a pixel's samples differs


@pytest.mark.gpu
def test_gpu_film_matches_reference_image_statistically(A, api, O):
    """The HIP path at the reference's own size against the reference binary's 256-spp image (other random numbers):
    16 x 16 block means of the 8-bit gamma-encoded pictures."""
    g = np.load(GOLD)
    sp = api.smallpt_scene_rewrite()
    p = api.smallpt_params(1024, 768, 256, seed=99, variant=A.SP_VARIANT_REWRITE)
    film = api.smallpt_render(sp, p)
    img = O.sprw_gamma_bytes(film).astype(np.float64)
    means = img.reshape(48, 16, 64, 16, 3).mean(axis=(1, 3))
    # The reference re-seeds its generator for every image row (Sampler::Clone, 1300): all rows of its picture replay ONE
    # random stream, so its noise does not average out down a block's rows -- a 16 x 16 block mean of its 256-spp picture
    # is as noisy as a 16-pixel row segment (about 2.5 of 255 levels).  Compare 192 x 256 regions instead (noise ~0.6 level);
    # a systematic difference (camera, a material, the roulette rule) shifts whole regions by several levels.
    big = lambda m: m.reshape(4, 12, 4, 16, 3).mean(axis=(1, 3))
    d = np.abs(big(means) - big(g["means64"].astype(np.float64)))
    assert d.mean() < 1.0 and d.max() < 3.0, (d.mean(), d.max())
    assert abs(means.mean() - g["means64"].mean()) < 0.6
    # and block by block the difference stays at the reference's own (row-correlated) noise level
    d16 = np.abs(means - g["means64"])
    assert d16.mean() < 4.0, d16.mean()
