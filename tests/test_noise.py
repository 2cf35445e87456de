"""CPU: the arithmetic of a frame's noise estimate (ky_amd/csrc/ky_noise.hpp; DESIGN.md "Noise") and what its entry points refuse before any device.  The
header's functions run here as host code (kyhostcheck_noise, ky_amd/csrc/ky_hostcheck.cpp: the file the sanitizer builds hold too) on hand-made accumulator
sequences, against closed forms and against the NumPy float64 restatement of tests/noise_restatement.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import noise_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_noise: the sanitizer build when the suite runs inside `make sanitize`, else the same sources built plainly."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    lib.kyhostcheck_noise.restype, lib.kyhostcheck_noise.argtypes = A.KYHOSTCHECK_SYMBOLS["kyhostcheck_noise"]
    return lib


def _host(check, accums, dones, total_spp, flags=None):
    """kyhostcheck_noise on per-pass [n_pix, 3] accumulators: (state [n_pass, n_pix, 2] float64, map [n_pass, n_pix] float32)."""
    acc = np.ascontiguousarray(np.stack([np.asarray(a, np.int64) for a in accums]))
    n_pass, n_pix = acc.shape[:2]
    done = np.ascontiguousarray(dones, np.int32)
    state = np.zeros((n_pass, n_pix, 2), np.float64)
    out = np.zeros((n_pass, n_pix), np.float32)
    fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
    rc = check.kyhostcheck_noise(acc.ctypes.data, done.ctypes.data, n_pass, n_pix, total_spp, None if fl is None else fl.ctypes.data, state.ctypes.data,
                                 out.ctypes.data, None, 0, 0, 0, 0)
    assert rc == 0
    return state, out


def test_constant_batches_have_no_variance(check):
    """Every batch has the same mean, and sample counts and sums are powers of two apart, so every quotient is exact: m2 == 0, the map 0 from the second batch."""
    per_sample = np.array([[3 << 20, 5 << 21, 7 << 19], [1 << 30, 0, 12345 << 8], [0, 0, 0]], np.int64)
    dones = [4, 8, 16, 32]
    state, out = _host(check, [per_sample * d for d in dones], dones, 32)
    assert (state[:, :, 1] == 0).all()
    assert np.isinf(out[0]).all() and (out[1:] == 0).all()
    assert np.array_equal(state[-1, :, 0], R.luminance(per_sample * 32, 32))


def test_two_batches_closed_form(check):
    """Batches of 4 and 3 samples with means a and b: m2 = 4 * 3 / 7 * (b - a)^2, the map sqrt(m2 / 1 / 7) / max(1, mean)."""
    first = np.array([[4 << 26, 4 << 27, 4 << 25], [9 << 28, 9 << 28, 9 << 28]], np.int64)
    second = first + np.array([[3 << 25, 9 << 27, 1 << 20], [1 << 33, 1 << 34, 1 << 33]], np.int64)
    total = 7
    state, out = _host(check, [first, second], [4, 7], total)
    y1, y2 = R.luminance(first, total), R.luminance(second, total)
    a, b = y1 / 4, (y2 - y1) / 3
    m2 = 12.0 / 7.0 * (b - a) ** 2
    assert (m2 > 0).all()
    assert np.allclose(state[1, :, 1], m2, rtol=1e-12, atol=0)
    assert np.array_equal(state[1, :, 0], y2) and (state[0, :, 1] == 0).all()
    mean = y2 / 7
    assert mean[0] < 1 < mean[1]   # the second pixel is over range: scaled down by its mean
    want = np.sqrt(m2 / 7) / np.maximum(1.0, mean)
    assert np.allclose(out[1], want, rtol=2e-7, atol=0)   # one rounding to float32 (6e-8) on a double value good to 1e-12


def test_unequal_batches_match_the_numpy_restatement(check):
    """The frame's own schedule of 500 samples (chunks of 24, 16, 8 and 4) in passes of one to five chunks, random accumulators that grow by random batch sums."""
    bounds = [24, 48, 64, 80, 112, 224, 308, 316, 436, 440, 496, 500]
    rng = np.random.default_rng(7)
    n_pix = 257
    per = rng.integers(0, 1 << 24, (n_pix, 3))   # a pixel's mean sample, about 0 .. 2 in units of 1 / 500 of the fixed-point scale x 500
    acc, accums, prev = np.zeros((n_pix, 3), np.int64), [], 0
    for d in bounds:
        acc = acc + (per * (d - prev) * rng.uniform(0.2, 1.8, (n_pix, 3))).astype(np.int64)
        accums.append(acc)
        prev = d
    flags = np.zeros(n_pix, np.uint32)
    flags[[3, 200]] = [1 << 4, 1 << 8]
    state, out = _host(check, accums, bounds, 500, flags)
    for k, (y_prev, m2, value) in enumerate(R.run(accums, bounds, 500, flags)):
        assert np.allclose(state[k, :, 0], y_prev, rtol=1e-12, atol=0)
        assert np.allclose(state[k, :, 1], m2, rtol=1e-12, atol=0)
        assert np.allclose(out[k], value, rtol=2e-7, atol=0) or k == 0
    assert np.isinf(out[0][flags == 0]).all() and (out[:, flags != 0] == 0).all()
    assert (state[-1, :, 1] > 0).all() and np.isfinite(out[-1]).all()


SHARD_1_3 = dict(tile_first=1, tile_step=3)
# film, tile: the square tiles the kernels were first tested at, the tiles that are not square, the tile that is one block, films that are no multiple of 8, and
# the frame of tests/test_frame_sizes_gpu.py (139 264 pixels: 544 partials of the statistics; as the shard 181 tiles, 181 partials)
XY_CASES = [(40, 24, 16, 16), (40, 24, 32, 32), (40, 24, 32, 8), (40, 24, 8, 24), (40, 24, 8, 8)]
XY_CASES += [(w, h, tw, th) for (w, h) in ((44, 21), (33, 17)) for (tw, th) in ((16, 16), (32, 8), (8, 24), (8, 8))] + [(264, 512, 16, 16)]


@pytest.mark.parametrize("shard", [{}, SHARD_1_3], ids=["whole", "shard_1_3"])
@pytest.mark.parametrize("w,h,tile_w,tile_h", XY_CASES, ids=["%dx%d_tile_%dx%d" % c for c in XY_CASES])
def test_pixel_map(w, h, tile_w, tile_h, shard, A, api, check):
    """noise_pixel_xy as the host runs it (through kyhostcheck_blocks: per block of 64 compact pixels, how many lie inside the film) against R.pixel_xy, and what
    the map must be whatever the tile: tile by tile a tile_w x tile_h rectangle of the film in row order, no two tiles at one place.  (That the blocks built on
    this map hold every pixel of the film once is tests/test_blocks.py::test_pixel_block_map's.)"""
    check.kyhostcheck_blocks.restype, check.kyhostcheck_blocks.argtypes = A.KYHOSTCHECK_SYMBOLS["kyhostcheck_blocks"]
    tile = dict(tile_w=tile_w, tile_h=tile_h)
    tiles_x, tiles_y = -(-w // tile_w), -(-h // tile_h)
    first, step = shard.get("tile_first", 0), shard.get("tile_step", 1)
    n_tiles = -(-(tiles_x * tiles_y - first) // step)
    n_pix = n_tiles * tile_w * tile_h
    if (w, h) == (264, 512):
        assert (n_tiles, -(-n_pix // 256)) == ((181, 181) if shard else (544, 544))
    x, y, inside = R.pixel_xy(n_pix, w, h, **tile, **shard)
    if tile_w == tile_h:   # `tile=` means a square tile
        assert all(np.array_equal(a, b) for a, b in zip((x, y, inside), R.pixel_xy(n_pix, w, h, tile=tile_w, **shard)))
    # the host's noise_pixel_xy: the in-film pixels of every block, the blocks' pixels located by the host too
    p = api.make_params(w, h, 500, **tile, **shard)
    pixel = np.full((n_pix // 64, 64), -1, np.int32)
    count = np.full(n_pix // 64, -1, np.int32)
    assert check.kyhostcheck_blocks(C.byref(p), None, pixel.ctypes.data, count.ctypes.data, None, 0, None, None, 0.0, 0.0, 2, 0, 0, None, 0, 0, 0, 0) == 0
    assert np.array_equal(count, inside[pixel].sum(axis=1))
    # a tile is a rectangle of the film in row order, at a tile's place of the grid, and no two tiles of a shard share a place
    tx, ty = x.reshape(n_tiles, tile_h, tile_w), y.reshape(n_tiles, tile_h, tile_w)
    assert (tx[:, 0, 0] % tile_w == 0).all() and (ty[:, 0, 0] % tile_h == 0).all()
    assert np.array_equal(tx - tx[:, :1, :1], np.broadcast_to(np.arange(tile_w)[None, None, :], tx.shape))
    assert np.array_equal(ty - ty[:, :1, :1], np.broadcast_to(np.arange(tile_h)[None, :, None], ty.shape))
    place = (ty[:, 0, 0] // tile_h) * tiles_x + tx[:, 0, 0] // tile_w
    assert len(set(place.tolist())) == n_tiles and place.max() < tiles_x * tiles_y
    if w % tile_w or h % tile_h:
        assert not inside.all() or shard                            # a ragged edge tile has padding
    assert ((x[~inside] >= w) | (y[~inside] >= h)).all() and (x[inside] < w).all() and (y[inside] < h).all()


def test_trailer_refusals(A, check):
    n_pix, base, done = 5, 200, 48
    def state(magic=R.NOISE_MAGIC, batches=2, n_prev=done, cut=0):
        s = bytes(base) + struct.pack("<Qii", magic, batches, n_prev) + bytes(16 * n_pix)
        return s[:len(s) - cut]
    def rc(s, samples_done=done):
        return check.kyhostcheck_noise(None, None, 0, 0, 500, None, None, None, s, len(s), base, n_pix, samples_done)
    assert rc(state()) == A.KY_OK
    assert rc(state() + b"xx") == A.KY_OK                      # longer is fine
    for bad in (state(cut=1), state(cut=16 * n_pix), state()[:base], state()[:base - 8], state(magic=R.NOISE_MAGIC ^ 1), state(magic=0),
                state(n_prev=done - 24), state(n_prev=0), state(batches=-1)):
        assert rc(bad) == A.KY_ERR_INVALID_VALUE
    assert rc(state(), samples_done=64) == A.KY_ERR_INVALID_VALUE   # the header's samples done is not the trailer's


def test_arguments_are_refused_before_any_device(A):
    lib = A.load_kyhip()
    st = A.NoiseStats()
    done = C.c_int(-7)
    buf = (C.c_float * 4)()
    assert lib.kyhip_frame_track_noise(None) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_noise(None, buf, 2) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_noise_stats(None, 0.01, C.byref(st)) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_render_until(None, 0.01, 0.0, 2, 1, C.byref(done), C.byref(st)) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    up = C.c_float(7)
    assert lib.kyhip_frame_noise_ms(None, C.byref(up), None) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error() and up.value == 7
    for min_batches in (1, 0, -3):
        assert lib.kyhip_frame_render_until(None, 0.01, 0.0, min_batches, 1, C.byref(done), C.byref(st)) == A.KY_ERR_INVALID_VALUE
        assert b"min_batches" in lib.kyhip_last_error()
    for threshold in (-1.0, -1e-30, float("nan")):
        assert lib.kyhip_frame_render_until(None, threshold, 0.0, 2, 1, C.byref(done), C.byref(st)) == A.KY_ERR_INVALID_VALUE
        assert b"threshold" in lib.kyhip_last_error()
        assert lib.kyhip_frame_noise_stats(None, threshold, C.byref(st)) == A.KY_ERR_INVALID_VALUE
        assert b"threshold" in lib.kyhip_last_error()
    assert lib.kyhip_frame_render_until(None, 0.01, 1.5, 2, 1, None, C.byref(st)) == A.KY_ERR_INVALID_VALUE and b"max_fraction_above" in lib.kyhip_last_error()
    assert lib.kyhip_frame_render_until(None, 0.01, 0.0, 2, 0, None, C.byref(st)) == A.KY_ERR_INVALID_VALUE and b"min_samples_per_pass" in lib.kyhip_last_error()
    assert done.value == -7


def test_stats_struct_layout(A, tmp_path):
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "kyhip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(ky_noise_stats), ' \
           'offsetof(ky_noise_stats, pixels), offsetof(ky_noise_stats, threshold), offsetof(ky_noise_stats, mean));return 0;}'
    (tmp_path / "sz.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "sz.c"), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    assert got == [C.sizeof(A.NoiseStats), A.NoiseStats.pixels.offset, A.NoiseStats.threshold.offset, A.NoiseStats.mean.offset]
