/*
 * ky_checkpoint.hpp -- what kyhip_frame_save writes and kyhip_frame_load reads, described ONCE (DESIGN.md "Checkpoint").  A checkpoint is the header, the
 * accumulators and flag words, then for a frame that tracks noise a NoiseTrailer and n_pix NoisePixel (ky_noise.hpp), then for one that tracks blocks a
 * BlockTrailer and n_blocks BlockState (ky_blocks.hpp), then for a frame that owns a sample range other than all of them (a slice, DESIGN.md "Slices") a
 * SliceTrailer.  CheckpointLayout says where each part lies, checkpoint_write_host writes the parts the host holds,
 * checkpoint_check decides what a frame loads; ky_frame.cpp adds the copies of the device parts and nothing else.  Host only, no HIP call: defined in
 * ky_frame_book.cpp next to the frame's book, which asks and writes through it (ky_frame_book.hpp); part of `make sanitize` (kyhostcheck_checkpoint, kyhostcheck_book,
 * ky_hostcheck.cpp).
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
constexpr uint64_t KY_FRAME_SLICE_MAGIC = 0x31434c5352464b59ull;   // "YKFRSLC1": a frame that owns the sample range [first, end) of its pixels, not all of them: its
                                                                   // samples_done is the count it HOLDS, which need be no pass boundary, and a SliceTrailer says which
FrameHeader frame_header(const ky_render_params* p, uint64_t scene_hash, int samples_done);   // (with KY_FRAME_MAGIC: a checkpoint's magic is its layout's)

// ---- slices: the sample ranges a frame's accumulators contain (DESIGN.md "Slices") ----
constexpr int KY_SLICE_MAX_RANGES = KYHIP_SLICE_MAX_RANGES;
// disjoint, ascending, non-empty [first, end) pairs, adjacent ones joined
struct Coverage {
    int n = 0;
    int r[2 * KY_SLICE_MAX_RANGES] = {};
    int held() const { int s = 0; for (int i = 0; i < n; ++i) s += r[2 * i + 1] - r[2 * i]; return s; }
};
// *out = a U b (out may be a or b): KY_OK; KY_ERR_INVALID_VALUE where they intersect; KY_ERR_LIMIT for more than KY_SLICE_MAX_RANGES ranges.  *out is written on KY_OK only.
int coverage_union(const Coverage& a, const Coverage& b, Coverage* out);
// kyhip_slice_bounds
int slice_bounds(int spp, int n_slices, int* bounds);
// what kyhip_frame_begin_slice asks of its range: both 0 or a pass boundary of the spp-sample frame, first <= end; KY_OK, or KY_ERR_INVALID_VALUE with the message
int slice_range_check(int spp, int first_sample, int end_sample);
// what a slice's checkpoint ends with; of fixed size, so that all slices of a frame have states of one size (one gather of equal-length buffers)
struct SliceTrailer {
    uint64_t magic;                      // KY_SLICE_MAGIC
    int32_t own_first, own_end, front;   // the owned range and how far it is rendered: own_first <= front <= own_end
    int32_t n_ranges;
    int32_t ranges[2 * KY_SLICE_MAX_RANGES];   // the coverage; zeros behind n_ranges pairs
};
constexpr uint64_t KY_SLICE_MAGIC = 0x314543494c534b59ull;   // "YKSLICE1"

// Where each part begins.  The parts lie back to back in this order, so a part ends where the next one begins and the last at `total`; a part the frame does not
// track is empty.  The header begins at 0.
struct CheckpointLayout {
    size_t accum = 0;          // 3 x 64-bit sums per pixel, then the pixels' flag words: the frame's accumulator block as it lies on the device
    size_t noise = 0;          // NoiseTrailer
    size_t noise_pixels = 0;   // n_pix NoisePixel (device)
    size_t blocks = 0;         // BlockTrailer
    size_t block_states = 0;   // n_blocks BlockState
    size_t slice = 0;          // SliceTrailer
    size_t total = 0;
    int n_pix = 0, n_blocks = 0;
    bool tracks_noise = false, tracks_blocks = false;
    bool sliced = false;       // the owned range is not (0, samples_per_pixel): the slice magic and trailer
    int own_first = 0, own_end = 0;
    size_t accum_bytes() const { return noise - accum; }
    size_t noise_pixels_bytes() const { return blocks - noise_pixels; }
    size_t block_states_bytes() const { return slice - block_states; }
};
// (own_end < 0: the frame owns all of its samples, as every frame of kyhip_frame_begin does)
CheckpointLayout checkpoint_layout(const ky_render_params* p, bool noise, bool blocks, int own_first = 0, int own_end = -1);

// what a checkpoint says beside the device parts (a part the layout does not have: its counts are not written, and read as 0)
struct CheckpointCounts {
    int samples_done = 0, chunks_done = 0;   // the header's, and the chunk count it stands for (checkpoint_check's result; not written)
    int batches = 0, n_prev = 0;             // NoiseTrailer
    int passes = 0;                          // BlockTrailer
    // SliceTrailer: the absolute sample the owned range is rendered to (chunks_done is ITS chunk count; samples_done the held count) and the coverage.  Of a frame
    // that is no slice: checkpoint_check gives front = samples_done and the coverage [0, samples_done); checkpoint_write_host reads neither.
    int front = 0;
    Coverage cov;
};
// the header (own, with the layout's magic and n.samples_done), both trailers and the block states (`states`: L.n_blocks of them, the host's copy) into buf
void checkpoint_write_host(const FrameHeader& own, const CheckpointLayout& L, const CheckpointCounts& n, const kyb::BlockState* states, void* buf);
// KY_OK and the counts, or KY_ERR_INVALID_VALUE with the message of the first part that refuses: the header (frame_state_check), then the noise trailer
// (kyn::noise_trailer_check, its n_prev against the header's samples), then the block trailer (kyb::block_trailer_check, its blocks against the header's samples
// and the noise trailer's batches).  A buffer longer than L.total is accepted.
int checkpoint_check(const FrameHeader& own, const CheckpointLayout& L, const void* buf, size_t bytes, CheckpointCounts* out);
// (a slice: the header with samples_done as the held count, the noise trailer against it, then the slice trailer -- slice_trailer_check with the layout's owned range)
// The slice trailer at `offset`: KY_OK and the trailer, or KY_ERR_INVALID_VALUE with the message: no whole trailer, another magic, an owned range that is not
// (own_first, own_end) (own_end < 0: any valid one), a front outside the owned range or on no boundary, ranges that are not ascending, disjoint, joined and on
// boundaries or whose part inside the owned range is not exactly [first, front), a held count that is not samples_done
int slice_trailer_check(const void* buf, size_t bytes, size_t offset, int total_spp, int samples_done, int own_first, int own_end, SliceTrailer* out);
// What kyhip_frame_merge accepts: `buf` is the saved state of another frame of own's identity (a plain one: its coverage is [0, samples_done); a slice; not one that
// tracks blocks).  KY_OK and what the state holds -- its coverage, where its accumulator block lies, where its noise pairs lie (0: it has no valid noise trailer) and
// their batch count --, or KY_ERR_INVALID_VALUE with the message.  Looks at nothing of the receiving frame but its header.
struct MergeSource {
    Coverage cov;
    size_t accum = 0, noise_pixels = 0;
    int batches = 0;
};
int merge_source_check(const FrameHeader& own, const void* buf, size_t bytes, MergeSource* out);
// ... and whether a frame that owns [own_first, own_end), holds `mine` and tracks noise or not may receive it: KY_OK and the union, KY_ERR_INVALID_VALUE, KY_ERR_LIMIT
int merge_accept(const Coverage& mine, int own_first, int own_end, int total_spp, bool tracks_noise, bool tracks_blocks, const Coverage& theirs, bool has_noise, Coverage* merged);
// the header's part of it: KY_OK and the chunk count the state's samples_done stands for, or KY_ERR_INVALID_VALUE with the message: a short buffer, another
// frame's state, a samples_done at which no chunk of the frame ends.  state_end: where the accumulators and flag words end (CheckpointLayout::noise)
int frame_state_check(const FrameHeader& own, const void* buf, size_t bytes, size_t state_end, int* chunks_done);
}  // namespace kyh
