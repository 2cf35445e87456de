"""The block arithmetic of a frame that retires pixel blocks (ky_amd/csrc/ky_blocks.hpp; DESIGN.md "Adaptive") restated in NumPy, and the layout of such a
frame's checkpoint.  Shared by tests/test_blocks.py (against the host build of the header) and tests/test_blocks_gpu.py (against the kernels)."""
import struct

import numpy as np

import noise_restatement as R

BLOCKS_MAGIC = 0x31534B434F4C4B59         # "YKLOCKS1"
FRAME_BLOCKS_MAGIC = 0x314B4C4252464B59   # "YKFRBLK1"
BLOCK_TRAILER_BYTES = 16                  # BlockTrailer: magic, n_blocks, padding; then n_blocks x {retired_at, batches} int32


def block_of_pixel(n_pix, tile=16):
    """Pixel i of a shard's compact tile buffer -> its 8 x 8 block, in the work decoder's order (tile, then block row, then block column)."""
    i = np.arange(n_pix)
    k, r = i // (tile * tile), i % (tile * tile)
    px, py = r % tile, r // tile
    bw = tile // 8
    return k * bw * bw + (py // 8) * bw + px // 8


def pixel_of_block(n_blocks, tile=16):
    """[n_blocks, 64]: pixel `lane` (row-major inside the block) of block b."""
    bw = tile // 8
    b = np.arange(n_blocks)[:, None]
    lane = np.arange(64)[None, :]
    k, inner = b // (bw * bw), b % (bw * bw)
    bx, by = inner % bw, inner // bw
    return (k * tile + by * 8 + lane // 8) * tile + bx * 8 + lane % 8


def inside_count(n_pix, width, height, tile=16, **shard):
    """Per block, its pixels inside the film."""
    _, _, inside = R.pixel_xy(n_pix, width, height, tile=tile, **shard)
    return np.bincount(block_of_pixel(n_pix, tile), weights=inside, minlength=n_pix // 64).astype(np.int64)


def initial_state(inside):
    """[n_blocks, 2] int32 {retired_at, batches}: blocks without a pixel inside the film are retired at 0, the others live (-1)."""
    st = np.zeros((len(inside), 2), np.int32)
    st[inside > 0, 0] = -1
    return st


def retire(state, values, counted, threshold, max_fraction_above, min_batches, front, batches, tile=16):
    """One application of the retire rule.  values: [n_pix] float32 in compact tile order; counted: [n_pix] bool, inside the film and unflagged."""
    state = state.copy()
    pix = pixel_of_block(len(state), tile)
    n_counted = counted[pix].sum(axis=1)
    n_above = (counted[pix] & (values[pix] > np.float32(threshold))).sum(axis=1)
    ok = (batches >= min_batches) & (n_above.astype(np.float64) <= np.float64(np.float32(max_fraction_above)) * n_counted.astype(np.float64))
    go = ok & (state[:, 0] < 0)
    state[go] = (front, batches)
    return state


def samples_per_pixel(state, front, n_pix, tile=16):
    """[n_pix]: the samples each compact pixel's block has received."""
    per_block = np.where(state[:, 0] >= 0, state[:, 0], front)
    return per_block[block_of_pixel(n_pix, tile)]


def split_blocks(state, n_pix, n_blocks, noise):
    """A block-tracking frame's checkpoint -> (the bytes before the block trailer, [n_blocks, 2] int32)."""
    at = R.HEADER_BYTES + n_pix * 28 + ((R.TRAILER_BYTES + n_pix * 16) if noise else 0)
    assert len(state) == at + BLOCK_TRAILER_BYTES + n_blocks * 8
    magic, n, _ = struct.unpack_from("<Qii", state, at)
    assert magic == BLOCKS_MAGIC and n == n_blocks
    return state[:at], np.frombuffer(state, np.int32, n_blocks * 2, at + BLOCK_TRAILER_BYTES).reshape(n_blocks, 2)
