/*
 * ky_blocks.hpp -- adaptive sampling: a frame that retires clean pixel blocks between its passes (kyhip_frame_track_blocks ...; DESIGN.md "Adaptive").  The unit
 * is the work decoder's item, a block of 8 x 8 pixels (ShardConst::blocks_per_tile, n_blocks): a block is live, or retired at the sample count it had when it was
 * last rendered.  Live blocks all stand at the frame's front; a pass renders the live ones only, through the ascending list of their indices (ky_render.hpp,
 * LISTED).  The arithmetic is written ONCE here, as KY_HD functions: the pixel <-> block index in compact tile order, the retire rule and the check of a
 * checkpoint's block trailer.  The device kernels (ky_blocks.hip), the host (ky_frame_book.cpp) and the host-only builds (kyhostcheck_blocks, ky_hostcheck.cpp)
 * share it.  Plain C++: part of `make sanitize`.
 */
#pragma once
#include <cstddef>
#include <cstdint>

#include "ky_noise.hpp"   // ky_shard.hpp, the pixels' classes

namespace kyb {
struct BlockState {
    int32_t retired_at;   // the samples per pixel the block had received when it retired; -1: live
    int32_t batches;      // ... and the noise batches it had then (0 for a frame that does not track noise)
};
// what a block-tracking frame's checkpoint appends behind the state (and behind the noise trailer, when both are tracked): this, then n_blocks BlockState
struct BlockTrailer {
    uint64_t magic;       // KY_BLOCKS_MAGIC
    int32_t n_blocks, passes;   // ... and the passes rendered so far (ky_block_stats::passes)
};
constexpr uint64_t KY_BLOCKS_MAGIC = 0x31534b434f4c4b59ull;   // "YKLOCKS1"
constexpr int KY_BLOCK_PIXELS = 64;

// Pixel i of a shard's compact tile buffer -> its block (the work decoder's b, ky_render.hpp) and its place in the block (lane = py * 8 + px)
KY_HD inline int block_of_pixel(const ShardConst& sh, int i, int* lane = nullptr) {
    const int per_tile = sh.tile_w * sh.tile_h;
    const int k = i / per_tile, r = i % per_tile;
    const int px = r % sh.tile_w, py = r / sh.tile_w;
    if (lane) *lane = (py & 7) * 8 + (px & 7);
    return k * sh.blocks_per_tile + (py >> 3) * sh.blocks_w + (px >> 3);
}
// ... and back: pixel `lane` of block b (the decoder's pix0 + py * tile_w + px)
KY_HD inline int pixel_of_block(const ShardConst& sh, int b, int lane) {
    const int k = b / sh.blocks_per_tile, inner = b % sh.blocks_per_tile;
    const int bx = inner % sh.blocks_w, by = inner / sh.blocks_w;
    return (k * sh.tile_h + by * 8 + (lane >> 3)) * sh.tile_w + bx * 8 + (lane & 7);
}
// whether compact pixel i lies inside the film (a ragged edge tile's padding does not)
KY_HD inline bool pixel_inside(const ShardConst& sh, int i, int width, int height, int* x_out = nullptr, int* y_out = nullptr) {
    int x, y;
    kyn::noise_pixel_xy(sh, i, x, y);
    if (x_out) *x_out = x;
    if (y_out) *y_out = y;
    return x < width && y < height;
}
// The retire rule, kyhip_frame_render_until's comparison per block: `above` of the block's `counted` pixels (inside the film and unflagged) lie above the threshold.
// A flagged pixel reads 0 and is not counted: it holds nothing back.  Before the second batch every counted pixel reads +inf.
KY_HD inline bool block_retires(int batches, int min_batches, int above, int counted, float max_fraction_above) {
    return batches >= min_batches && (double)above <= (double)max_fraction_above * (double)counted;
}
// the samples a block has received with the frame's front at `front`
KY_HD inline int block_samples(const BlockState& s, int front) { return s.retired_at >= 0 ? s.retired_at : front; }

// where the live list lies in a frame's accumulator block: behind the accumulators and the flag words (ky_render.hpp reads flags + n_pix)
inline size_t blocks_list_offset(const ShardConst& sh) { return (size_t)sh.n_pix * (3 * sizeof(unsigned long long) + sizeof(unsigned)); }
inline size_t blocks_list_bytes(const ShardConst& sh) { return (size_t)sh.n_blocks * sizeof(int); }

// ---- the block trailer of a checkpoint (ky_frame_book.cpp) ----
inline size_t block_trailer_bytes(int n_blocks) { return sizeof(BlockTrailer) + (size_t)n_blocks * sizeof(BlockState); }
// KY_OK, or KY_ERR_INVALID_VALUE with the message: `bytes` after `offset` hold no whole trailer, another magic, another block count, a retirement count that is
// neither -1 nor a sample count at which a pass of a total_spp-sample frame can end (0 included), or one beyond samples_done; a pass count below 0; a batch count
// that is not 0 on a live block or on one retired at 0 samples, or lies outside 0 .. noise_batches (the noise trailer's batch count; 0 for a frame without one)
int block_trailer_check(const void* buf, size_t bytes, size_t offset, int n_blocks, int total_spp, int samples_done, int noise_batches, BlockTrailer* out = nullptr);

// ---- the kernels (ky_blocks.hip); every pointer is device memory, `stream` a hipStream_t ----
constexpr int KY_BLOCKS_GROUP = 256;   // blocks per workgroup of the compaction
inline int blocks_groups(int n_blocks) { return (n_blocks + KY_BLOCKS_GROUP - 1) / KY_BLOCKS_GROUP; }
inline size_t blocks_scratch_bytes(int n_blocks) { return ((size_t)blocks_groups(n_blocks) + 1) * sizeof(int); }   // the groups' counts, then n_live
// every block with a pixel inside the film live, every other one retired at 0
int blocks_init_device(void* state, const ShardConst& sh, int width, int height, void* stream);
// retires (at `front`, with `batches`) every live block none of whose in-film pixels is set in `mask` (width x height bytes, y down)
int blocks_keep_device(void* state, const unsigned char* mask, const ShardConst& sh, int width, int height, int front, int batches, void* stream);
// one application of the retire rule to the live blocks: `map` and `cls` are noise_map_device's
int blocks_retire_device(void* state, const float* map, const unsigned char* cls, const ShardConst& sh, float threshold, float max_fraction_above, int min_batches,
                         int front, int batches, void* stream);
// the ascending list of the live blocks -> list, their count -> the last word of scratch
int blocks_compact_device(const void* state, int n_blocks, int* list, void* scratch, void* stream);
// resolve_frame_kernel with a per-block scale total_spp / (the block's samples); blocks at 0 samples resolve to 0
int blocks_resolve_device(const void* ws, const void* state, float* d_tiles, const ShardConst& sh, int total_spp, int front, void* stream);
}  // namespace kyb
