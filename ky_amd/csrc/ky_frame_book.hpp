/*
 * ky_frame_book.hpp -- everything a frame in passes (kyhip_frame_*; DESIGN.md "Passes") IS apart from its device memory: what it describes, which samples it owns, how
 * far it is rendered, what its accumulators hold, what it tracks -- and the state machine over those small integers.  Every operation is a QUESTION, answered from the
 * book alone (KY_OK, or the status and message the entry point gives), or a COMMIT, which the caller applies only behind the wait for the device work it stands for.
 * ky_frame.cpp asks, does the HIP work, waits and commits; kyhostcheck_book (ky_hostcheck.cpp) asks and commits, so that whole life cycles run without a GPU.  A frame
 * has two sample counts since slices: its FRONT, the absolute sample its owned range is rendered to, and what it HOLDS, the samples per pixel in its accumulators; the
 * operations hand out the one that is meant.  Plain C++17, no HIP header: ky_frame_book.cpp also defines what ky_checkpoint.hpp declares; part of `make sanitize`.
 */
#pragma once
#include <vector>

#include "ky_checkpoint.hpp"

namespace kyh {
// a pass: chunks [chunk_first, chunk_first + chunk_count) of the owned range; chunk_count 0: nothing to do (the owned range is rendered, or no block is live)
struct PassStep {
    int chunk_first = 0, chunk_count = 0;
    int n_prev = 0, n_now = 0;   // the noise estimate's batch: it stands at n_prev samples, the frame holds n_now behind the pass
    Coverage held_then;
    bool launch = false;         // the shard has pixels: a shard without commits the step without a launch
};
// a resolve: nothing to do, or clamp01(sum * scale), with blocks_resolve_kernel's per-block scale where `per_block` (held: the samples it divides by)
struct ResolveStep {
    bool nothing = true, per_block = false;
    double scale = 1.0;
    int held = 0;
};
// a merge: where the source's parts lie in its saved state (0, 0 for another frame's device memory), what the source and the receiver hold, the union
struct MergeStep {
    size_t accum = 0, noise_pixels = 0;
    int n_mine = 0, n_src = 0, src_batches = 0;
    Coverage merged;
};

struct FrameBook {
    ky_render_params params{};
    ShardConst sh{};
    ChunkPlan plan{};
    FrameHeader header{};         // with samples_done = 0
    CheckpointLayout layout;      // of what the frame tracks now
    int own_first = 0, own_end = 0;   // the samples the frame owns and renders, and ...
    int own_c0 = 0, own_c1 = 0;       // ... the chunks they are
    int chunks_done = 0;          // the chunks before the frame's front: own_c0 .. own_c1
    Coverage cov;                 // the samples the accumulators hold: [own_first, front) and what was merged
    bool loaded = false;
    struct { bool on = false; int batches = 0, n_prev = 0; } noise;   // updates so far and the samples held at the last one
    struct {
        bool on = false;
        int n_live = 0, passes = 0;
        std::vector<kyb::BlockState> host;   // the host's copy of the device's block states: current behind every call
        std::vector<int> inside;             // per block, its pixels inside the film
    } blocks;

    // The frame's pixel filter, the box until set_filter: part of what the frame IS.  header.scene_hash is filter_fold(base_hash, &filter):
    // the packed scene's hash itself under the box, so every state of an unfiltered frame is what it was.
    ky_pixel_filter filter{};
    uint64_t base_hash = 0;
    // ... and its lens (section 12), the pinhole {0, 0} until set_lens: header.scene_hash is lens_fold(filter_fold(base_hash, &filter), &lens)
    ky_lens lens{};
    int set_lens(const ky_lens* l);   // kyhip_frame_set_lens behind its NULL frame, as set_filter
    // ... and the digest of its texture set (section 13; texture_digest, ky_pack.cpp), 0 while it has none: folded in last, texture_fold(lens_fold(...), digest)
    uint64_t tex_digest = 0;
    int set_textures(uint64_t digest);   // kyhip_frame_set_textures behind its checks; refused once the frame holds a sample

    // the book of the frame of p that owns [first_sample, end_sample): behind begin_check
    void begin(const ky_render_params* p, uint64_t scene_hash, int first_sample, int end_sample);
    // kyhip_frame_set_filter behind its NULL frame: refuses an invalid filter, and any filter once the frame holds or has loaded a sample; then a commit of its own
    // (no device work stands behind it)
    int set_filter(const ky_pixel_filter* f);

    // ---- questions ----
    int front() const { return chunk_end(plan, chunks_done - 1); }
    int held() const { return cov.held(); }
    bool untouched() const { return chunks_done == own_c0 && cov.n == 0 && !loaded; }
    bool owned_rendered() const { return chunks_done >= own_c1; }
    // a block-tracking frame all of whose blocks are retired: no pass renders anything any more and the front stays (a shard without blocks is none)
    bool nothing_live() const { return blocks.on && sh.n_blocks > 0 && blocks.n_live == 0; }
    int tracks(bool want_blocks, bool want_noise) const;   // what the entries of a frame that tracks something refuse
    int coverage(int* ranges2, int n, int own[2]) const;   // kyhip_frame_coverage behind its NULL frame
    int next_pass(int min_samples, PassStep* out) const;
    int can_track_noise() const;
    int can_track_blocks() const;
    int resolve(int normalise, const float* film_rgb, size_t stride_px, ResolveStep* out) const;
    int denoise_check(bool needs_variance) const;
    // kyhip_frame_denoise_temporal behind its NULL arguments and parameters: denoise_check(true), then a frame that tracks blocks, then a history of another
    // device, size or albedo mode than this frame's (hist_albedo: -1 while the history holds no picture, else 0 / 1)
    int temporal_check(int device, int albedo_grid, int hist_device, int hist_width, int hist_height, int hist_albedo) const;
    int save_host(void* buf, size_t bytes) const;          // refuses a short buffer, then writes the parts of the checkpoint the host holds
    int load_check(const void* buf, size_t bytes, CheckpointCounts* out) const;
    int filter_refusal(const void* buf, size_t bytes) const;   // a saved state that differs from this frame in its pixel filter: the refusal that names it
    int merge_state(const void* state, size_t bytes, MergeStep* out) const;
    int merge_book(const FrameBook& src, MergeStep* out) const;
    void block_stats(ky_block_stats* out) const;
    int sample_map(int32_t* map, size_t stride_px) const;
    // the two stop verdicts behind a pass: kyhip_frame_render_until's on its statistics, kyhip_frame_render_adaptive's
    bool until_stops(const ky_noise_stats& s, float max_fraction_above, int min_batches) const;
    bool adaptive_stops() const { return nothing_live() || front() >= params.samples_per_pixel; }

    // ---- commits ----
    void commit_pass(const PassStep& s);
    void track_noise();
    void size_blocks();                  // the host's block states and `inside`, before the device's states come home into them
    void track_blocks();
    int blocks_home(int n_live);         // behind the copy of the device's states into blocks.host: their live count
    void commit_load(const CheckpointCounts& n);
    void commit_merge(const MergeStep& s);

private:
    void retrack() { layout = checkpoint_layout(&params, noise.on, blocks.on, own_first, own_end); }
};

// What kyhip_frame_begin and kyhip_frame_begin_slice refuse before they look for a device, in this order: the params, the shard's and the film's range, `out` (set to
// NULL behind it), the slice's range.  The host-only builds' stand-ins (ky_hostcheck.cpp) call it too.
int begin_check(const ky_scene* scene, const ky_render_params* p, int first_sample, int end_sample, kyhip_frame** out);
}  // namespace kyh
