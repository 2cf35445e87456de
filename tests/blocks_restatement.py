"""The block arithmetic of a frame that retires pixel blocks (ky_amd/csrc/ky_blocks.hpp; DESIGN.md "Adaptive") restated in NumPy, and the layout of such a
frame's checkpoint, and the chunk schedule that cuts a frame into passes (ky_amd/csrc/ky_shard.hpp).  Shared by tests/test_blocks.py (against the host build of
the header) and tests/test_blocks_gpu.py, tests/test_frame_sizes_gpu.py (against the kernels)."""
import struct

import numpy as np

import noise_restatement as R

BLOCKS_MAGIC = 0x31534B434F4C4B59         # "YKLOCKS1"
FRAME_BLOCKS_MAGIC = 0x314B4C4252464B59   # "YKFRBLK1"
BLOCK_TRAILER_BYTES = 16                  # BlockTrailer: magic, n_blocks, padding; then n_blocks x {retired_at, batches} int32


def block_of_pixel(n_pix, tile=16, tile_w=None, tile_h=None):
    """Pixel i of a shard's compact tile buffer -> its 8 x 8 block, in the work decoder's order (tile, then block row, then block column)."""
    tw, th = R.tile_size(tile, tile_w, tile_h)
    i = np.arange(n_pix)
    k, r = i // (tw * th), i % (tw * th)
    px, py = r % tw, r // tw
    bw = tw // 8
    return k * (bw * (th // 8)) + (py // 8) * bw + px // 8


def pixel_of_block(n_blocks, tile=16, tile_w=None, tile_h=None):
    """[n_blocks, 64]: pixel `lane` (row-major inside the block) of block b."""
    tw, th = R.tile_size(tile, tile_w, tile_h)
    bw = tw // 8
    per_tile = bw * (th // 8)
    b = np.arange(n_blocks)[:, None]
    lane = np.arange(64)[None, :]
    k, inner = b // per_tile, b % per_tile
    bx, by = inner % bw, inner // bw
    return (k * th + by * 8 + lane // 8) * tw + bx * 8 + lane % 8


def inside_count(n_pix, width, height, tile=16, tile_w=None, tile_h=None, **shard):
    """Per block, its pixels inside the film."""
    _, _, inside = R.pixel_xy(n_pix, width, height, tile=tile, tile_w=tile_w, tile_h=tile_h, **shard)
    return np.bincount(block_of_pixel(n_pix, tile, tile_w, tile_h), weights=inside, minlength=n_pix // 64).astype(np.int64)


def keep_mask(blocks, n_pix, width, height, tile=16, tile_w=None, tile_h=None, **shard):
    """(height, width) uint8 for Frame.keep: the in-film pixels of the blocks whose indices (the work decoder's order) are given are set, nothing else."""
    x, y, inside = R.pixel_xy(n_pix, width, height, tile=tile, tile_w=tile_w, tile_h=tile_h, **shard)
    pix = pixel_of_block(n_pix // 64, tile, tile_w, tile_h)[np.asarray(sorted(blocks), np.int64)].ravel()
    pix = pix[inside[pix]]
    mask = np.zeros((height, width), np.uint8)
    mask[y[pix], x[pix]] = 1
    return mask


def initial_state(inside):
    """[n_blocks, 2] int32 {retired_at, batches}: blocks without a pixel inside the film are retired at 0, the others live (-1)."""
    st = np.zeros((len(inside), 2), np.int32)
    st[inside > 0, 0] = -1
    return st


def retire(state, values, counted, threshold, max_fraction_above, min_batches, front, batches, tile=16, tile_w=None, tile_h=None):
    """One application of the retire rule.  values: [n_pix] float32 in compact tile order; counted: [n_pix] bool, inside the film and unflagged."""
    state = state.copy()
    pix = pixel_of_block(len(state), tile, tile_w, tile_h)
    n_counted = counted[pix].sum(axis=1)
    n_above = (counted[pix] & (values[pix] > np.float32(threshold))).sum(axis=1)
    ok = (batches >= min_batches) & (n_above.astype(np.float64) <= np.float64(np.float32(max_fraction_above)) * n_counted.astype(np.float64))
    go = ok & (state[:, 0] < 0)
    state[go] = (front, batches)
    return state


def samples_per_pixel(state, front, n_pix, tile=16, tile_w=None, tile_h=None):
    """[n_pix]: the samples each compact pixel's block has received."""
    per_block = np.where(state[:, 0] >= 0, state[:, 0], front)
    return per_block[block_of_pixel(n_pix, tile, tile_w, tile_h)]


def split_blocks(state, n_pix, n_blocks, noise):
    """A block-tracking frame's checkpoint -> (the bytes before the block trailer, [n_blocks, 2] int32)."""
    at = R.HEADER_BYTES + n_pix * 28 + ((R.TRAILER_BYTES + n_pix * 16) if noise else 0)
    assert len(state) == at + BLOCK_TRAILER_BYTES + n_blocks * 8
    magic, n, _ = struct.unpack_from("<Qii", state, at)
    assert magic == BLOCKS_MAGIC and n == n_blocks
    return state[:at], np.frombuffer(state, np.int32, n_blocks * 2, at + BLOCK_TRAILER_BYTES).reshape(n_blocks, 2)


def chunk_ends(spp):
    """chunk_plan (ky_shard.hpp) restated: the sample counts at which the chunks of an spp-sample frame end.  Chunks of 24 samples, then the taper: the last 64
    samples in chunks of 4, the 128 before them in 8s, the 256 before those in 16s, which also take what is left of the bulk's last chunk."""
    b3 = spp
    b2 = max(b3 - 64, 0)
    b1 = max(b2 - 128, 0)
    b0 = max(b1 - 256, 0)
    head = b0 // 24 * 24
    ends = list(range(24, head + 1, 24))
    for first, limit, size in ((head, b1, 16), (b1, b2, 8), (b2, b3, 4)):
        s = first
        while s < limit:
            s = min(s + size, limit)
            ends.append(s)
    return ends


def pass_plan(spp, min_samples):
    """[(first chunk, chunks, samples done behind the pass)] of render(min_samples) until the frame is complete (pass_chunk_end, ky_shard.hpp)."""
    ends, plan, c = chunk_ends(spp), [], 0
    while c < len(ends):
        want = (ends[c - 1] if c else 0) + min_samples
        e = c
        while e < len(ends) - 1 and ends[e] < want:
            e += 1
        plan.append((c, e + 1 - c, ends[e]))
        c = e + 1
    return plan
