"""The noise estimate of a frame (ky_amd/csrc/ky_noise.hpp; DESIGN.md "Noise") restated in NumPy float64, operation by operation in the header's order, and
the layout of a tracking frame's checkpoint.  Shared by tests/test_noise.py (against the host build of the header) and tests/test_noise_gpu.py (against the
kernels)."""
import struct

import numpy as np

NOISE_MAGIC = 0x314553494F4E4B59   # "YKNOISE1"
HEADER_BYTES = 8 + 8 + 12 * 4 + 8 + 4 + 4   # FrameHeader (ky_checkpoint.hpp): magic, source hash, ky_render_params, scene hash, samples_done, n_pix
TRAILER_BYTES = 16                           # NoiseTrailer: magic, batches, n_prev


def luminance(accum, total_spp):
    """accum: [..., 3] int64 accumulators -> the sum of the samples' luminances (noise_luminance)."""
    a = np.asarray(accum, np.int64).astype(np.float64)
    y = 0.212671 * a[..., 0] + 0.715160 * a[..., 1] + 0.072169 * a[..., 2]
    return y / 4294967296.0 * float(total_spp)


def update(y_prev, m2, y_now, n_prev, n_now):
    """noise_update for arrays of pixels: -> (y_prev, m2) after the batch (n_prev, n_now]."""
    if n_prev > 0 and n_now > n_prev:
        n = float(n_now - n_prev)
        d = y_now - y_prev
        t = d / n - y_prev / float(n_prev)
        w = n * float(n_prev) / float(n_now)
        m2 = m2 + w * (t * t)
    return y_now.copy(), m2


def value(y_prev, m2, batches, n_done, flags=None):
    """noise_value: the map, float32."""
    if batches < 2 or n_done < 1:
        v = np.full(y_prev.shape, np.inf, np.float32)
    else:
        se = np.sqrt(m2 / float(batches - 1) / float(n_done))
        mean = y_prev / float(n_done)
        v = (se / np.where(mean > 1.0, mean, 1.0)).astype(np.float32)
    if flags is not None:
        v = np.where((np.asarray(flags) & 0x1FF) != 0, np.float32(0), v)
    return v


def run(accums, dones, total_spp, flags=None):
    """accums: per pass [n_pix, 3] int64; dones: the samples done after each pass -> per pass (y_prev, m2, map)."""
    out, n_prev = [], 0
    y_prev = np.zeros(np.asarray(accums[0]).shape[0], np.float64)
    m2 = np.zeros_like(y_prev)
    for k, (acc, done) in enumerate(zip(accums, dones)):
        y_prev, m2 = update(y_prev, m2, luminance(acc, total_spp), n_prev, done)
        n_prev = done
        out.append((y_prev, m2, value(y_prev, m2, k + 1, done, flags)))
    return out


def split_state(state, n_pix):
    """A checkpoint's bytes -> (samples_done, accum [n_pix, 3] int64, flags [n_pix] uint32, trailer or None); trailer = (batches, n_prev, y_prev, m2)."""
    samples_done, header_n_pix = struct.unpack_from("<ii", state, HEADER_BYTES - 8)
    assert header_n_pix == n_pix
    accum = np.frombuffer(state, np.int64, n_pix * 3, HEADER_BYTES).reshape(n_pix, 3)
    flags = np.frombuffer(state, np.uint32, n_pix, HEADER_BYTES + n_pix * 24)
    base = HEADER_BYTES + n_pix * 28
    if len(state) == base:
        return samples_done, accum, flags, None
    assert len(state) == base + TRAILER_BYTES + n_pix * 16
    magic, batches, n_prev = struct.unpack_from("<Qii", state, base)
    assert magic == NOISE_MAGIC
    pairs = np.frombuffer(state, np.float64, n_pix * 2, base + TRAILER_BYTES).reshape(n_pix, 2)
    return samples_done, accum, flags, (batches, n_prev, pairs[:, 0], pairs[:, 1])


def tile_size(tile=16, tile_w=None, tile_h=None):
    """(tile_w, tile_h): `tile` is a square tile; tile_w / tile_h name the sides apart (ShardConst::tile_w, tile_h)."""
    return (tile if tile_w is None else tile_w), (tile if tile_h is None else tile_h)


def pixel_xy(n_pix, width, height, tile=16, tile_first=0, tile_step=1, tile_w=None, tile_h=None):
    """Pixel i of a shard's compact tile buffer -> (x, y) in the film (noise_pixel_xy, film_add_kernel's de-interleave: tile rows rotated), and whether it
    lies inside."""
    tw, th = tile_size(tile, tile_w, tile_h)
    tiles_x = (width + tw - 1) // tw
    i = np.arange(n_pix)
    k, r = i // (tw * th), i % (tw * th)
    t = tile_first + k * tile_step
    trow = t // tiles_x
    tcol = (t % tiles_x + trow) % tiles_x
    x, y = tcol * tw + r % tw, trow * th + r // tw
    return x, y, (x < width) & (y < height)
