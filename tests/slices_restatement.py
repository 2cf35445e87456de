"""A merge of two frames' sample ranges (ky_amd/csrc/ky_noise.hpp: noise_merge, merge_pixel; DESIGN.md "Slices") restated in NumPy float64, operation by
operation in the header's order, the layout of a slice's checkpoint, a frame's resolve (ky_film_value.hpp) and the noise statistics' reduction order (ky_noise.hip) restated.  Shared by tests/test_slices.py (against
the host build of the headers) and tests/test_slices_gpu.py (against the kernel)."""
import struct

import numpy as np

import noise_restatement as R

SLICE_FRAME_MAGIC = 0x31434C5352464B59   # "YKFRSLC1": the header's
SLICE_MAGIC = 0x314543494C534B59         # "YKSLICE1": the trailer's
MAX_RANGES = 32
SLICE_TRAILER_BYTES = 8 + 4 * 4 + MAX_RANGES * 2 * 4   # magic; own_first, own_end, front, n_ranges; the ranges


def merge_pairs(y_a, m2_a, n_a, y_b, m2_b, n_b, y_merged):
    """noise_merge for arrays of pixels: -> (y_prev, m2) of a after it received b."""
    if n_a > 0 and n_b > 0:
        w = float(n_a) * float(n_b) / float(n_a + n_b)
        t = y_b / float(n_b) - y_a / float(n_a)
        m2 = m2_a + m2_b + w * (t * t)
    elif n_a <= 0:
        m2 = m2_b.copy()
    else:
        m2 = m2_a.copy()
    return y_merged.copy(), m2


def merge(words_a, flags_a, words_b, flags_b, total_spp, pairs_a=None, n_a=0, pairs_b=None, n_b=0):
    """merge_pixel for arrays: words [n, 3] int64 (two's complement sums), flags [n] uint32, pairs (y_prev [n], m2 [n]) or None -> (words, flags, pairs or None)."""
    words = (np.asarray(words_a, np.int64).view(np.uint64) + np.asarray(words_b, np.int64).view(np.uint64)).view(np.int64)
    flags = np.asarray(flags_a, np.uint32) | np.asarray(flags_b, np.uint32)
    if pairs_a is None:
        return words, flags, None
    return words, flags, merge_pairs(pairs_a[0], pairs_a[1], n_a, pairs_b[0], pairs_b[1], n_b, R.luminance(words, total_spp))


def split_slice_state(state, n_pix):
    """A slice's checkpoint -> (samples held, accum [n_pix, 3] int64, flags [n_pix] uint32, noise trailer or None, (own_first, own_end, front, ranges))."""
    magic, = struct.unpack_from("<Q", state, 0)
    assert magic == SLICE_FRAME_MAGIC
    plain = state[:len(state) - SLICE_TRAILER_BYTES]
    held, accum, flags, trailer = R.split_state(plain, n_pix)
    tmagic, first, end, front, n = struct.unpack_from("<Qiiii", state, len(plain))
    assert tmagic == SLICE_MAGIC and 0 <= n <= MAX_RANGES
    r = struct.unpack_from("<%di" % (2 * MAX_RANGES), state, len(plain) + 24)
    assert all(v == 0 for v in r[2 * n:])
    return held, accum, flags, trailer, (first, end, front, [(r[2 * i], r[2 * i + 1]) for i in range(n)])


def accum_part(state, n_pix):
    """The accumulator and flag words of any frame state, as bytes."""
    return state[R.HEADER_BYTES:R.HEADER_BYTES + n_pix * 28]


def film_values(accum, flags, scale):
    """film_value (ky_film_value.hpp) per pixel and channel: [n, 3] float32 = clamp01(word / 2^32 * scale), the products in double before the one rounding; the
    flag word's bits pin +inf to 1, -inf, NaN and both infinities to 0."""
    v = (np.asarray(accum, np.int64).astype(np.float64) * (1.0 / 4294967296.0) * float(scale)).astype(np.float32)
    fl = np.asarray(flags, np.uint32)[:, None]
    ch = np.arange(3, dtype=np.uint32)[None, :]
    nan, pinf, ninf = (fl >> ch) & 1, (fl >> (3 + ch)) & 1, (fl >> (6 + ch)) & 1
    v = np.where(pinf != 0, np.float32(1), v)
    v = np.where(ninf != 0, np.float32(0), v)
    v = np.where((nan != 0) | ((pinf != 0) & (ninf != 0)), np.float32(0), v)
    return np.clip(v, np.float32(0), np.float32(1))


def film_of(accum, flags, scale, width, height, **shard):
    """A zero film with film_values at the shard's pixels that lie inside it."""
    n_pix = len(flags)
    x, y, inside = R.pixel_xy(n_pix, width, height, **shard)
    film = np.zeros((height, width, 3), np.float32)
    film[y[inside], x[inside]] = film_values(accum, flags, scale)[inside]
    return film


def _tree256(v):
    """ky_noise.hip's block_reduce on 256 doubles: inside each wave of 64 lane l takes lane l + 32, + 16, ... + 1 (the lower lanes on the left), then the four waves'
    results are added in wave order."""
    w = np.asarray(v, np.float64).reshape(4, 64).copy()
    for delta in (32, 16, 8, 4, 2, 1):
        w[:, :64 - delta] = w[:, :64 - delta] + w[:, delta:]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def stats_sum(values):
    """noise_stats_kernel + noise_final_kernel's sum over the compact tile buffer's per-pixel contributions (float64; 0 for padding and flagged pixels): one partial
    per 256 pixels, then one workgroup whose thread t adds a contiguous run of partials to 0 in index order, through the same tree."""
    v = np.asarray(values, np.float64)
    blocks = (len(v) + 255) // 256
    v = np.concatenate([v, np.zeros(blocks * 256 - len(v))])
    partials = [_tree256(v[256 * b:256 * (b + 1)]) for b in range(blocks)]
    per = (blocks + 255) // 256
    mine = np.zeros(256)
    for t in range(256):
        for j in range(t * per, min(t * per + per, blocks)):
            mine[t] = mine[t] + partials[j]
    return _tree256(mine)
