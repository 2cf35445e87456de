/*
 * ky_checkpoint.hpp -- what kyhip_frame_save writes and kyhip_frame_load reads, described ONCE (DESIGN.md "Checkpoint").  A checkpoint is the header, the
 * accumulators and flag words, then for a frame that tracks noise a NoiseTrailer and n_pix NoisePixel (ky_noise.hpp), then for one that tracks blocks a
 * BlockTrailer and n_blocks BlockState (ky_blocks.hpp).  CheckpointLayout says where each part lies, checkpoint_write_host writes the parts the host holds,
 * checkpoint_check decides what a frame loads; ky_frame.cpp adds the copies of the device parts and nothing else.  Host only, no HIP call: defined in
 * ky_pack.cpp, part of `make sanitize` (kyhostcheck_checkpoint, ky_hostcheck.cpp).
 */
#pragma once
#include "ky_blocks.hpp"   // ky_noise.hpp, ky_shard.hpp
#include "ky_host.hpp"

namespace kyh {
// Everything in the header but samples_done names what the frame IS: a state is loaded only into a frame whose own header agrees in all of that.
struct FrameHeader {
    uint64_t magic;            // KY_FRAME_MAGIC, or KY_FRAME_BLOCKS_MAGIC in the checkpoint of a frame that tracks blocks
    uint64_t source_hash;      // kyhip_kernel_source_hash(): another kernel source's chunk sums differ in the last bit
    ky_render_params params;
    uint64_t scene_hash;       // scene_hash of the packed scene
    int32_t samples_done, n_pix;
};
constexpr uint64_t KY_FRAME_MAGIC = 0x31454d4152464b59ull;   // "YKFRAME1"
constexpr uint64_t KY_FRAME_BLOCKS_MAGIC = 0x314b4c4252464b59ull;   // "YKFRBLK1": a frame that retires pixel blocks (ky_blocks.hpp): its accumulators stand at per-block
                                                                    // sample counts, which a frame that does not track blocks would resolve wrongly
FrameHeader frame_header(const ky_render_params* p, uint64_t scene_hash, int samples_done);   // (with KY_FRAME_MAGIC: a checkpoint's magic is its layout's)

// Where each part begins.  The parts lie back to back in this order, so a part ends where the next one begins and the last at `total`; a part the frame does not
// track is empty.  The header begins at 0.
struct CheckpointLayout {
    size_t accum = 0;          // 3 x 64-bit sums per pixel, then the pixels' flag words: the frame's accumulator block as it lies on the device
    size_t noise = 0;          // NoiseTrailer
    size_t noise_pixels = 0;   // n_pix NoisePixel (device)
    size_t blocks = 0;         // BlockTrailer
    size_t block_states = 0;   // n_blocks BlockState
    size_t total = 0;
    int n_pix = 0, n_blocks = 0;
    bool tracks_noise = false, tracks_blocks = false;
    size_t accum_bytes() const { return noise - accum; }
    size_t noise_pixels_bytes() const { return blocks - noise_pixels; }
    size_t block_states_bytes() const { return total - block_states; }
};
CheckpointLayout checkpoint_layout(const ky_render_params* p, bool noise, bool blocks);

// what a checkpoint says beside the device parts (a part the layout does not have: its counts are not written, and read as 0)
struct CheckpointCounts {
    int samples_done = 0, chunks_done = 0;   // the header's, and the chunk count it stands for (checkpoint_check's result; not written)
    int batches = 0, n_prev = 0;             // NoiseTrailer
    int passes = 0;                          // BlockTrailer
};
// the header (own, with the layout's magic and n.samples_done), both trailers and the block states (`states`: L.n_blocks of them, the host's copy) into buf
void checkpoint_write_host(const FrameHeader& own, const CheckpointLayout& L, const CheckpointCounts& n, const kyb::BlockState* states, void* buf);
// KY_OK and the counts, or KY_ERR_INVALID_VALUE with the message of the first part that refuses: the header (frame_state_check), then the noise trailer
// (kyn::noise_trailer_check, its n_prev against the header's samples), then the block trailer (kyb::block_trailer_check, its blocks against the header's samples
// and the noise trailer's batches).  A buffer longer than L.total is accepted.
int checkpoint_check(const FrameHeader& own, const CheckpointLayout& L, const void* buf, size_t bytes, CheckpointCounts* out);
// the header's part of it: KY_OK and the chunk count the state's samples_done stands for, or KY_ERR_INVALID_VALUE with the message: a short buffer, another
// frame's state, a samples_done at which no chunk of the frame ends.  state_end: where the accumulators and flag words end (CheckpointLayout::noise)
int frame_state_check(const FrameHeader& own, const void* buf, size_t bytes, size_t state_end, int* chunks_done);
}  // namespace kyh
