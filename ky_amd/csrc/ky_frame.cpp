/*
 * ky_frame.cpp -- a frame rendered in passes: kyhip_frame_* (include/kyhip.h; DESIGN.md "Passes").  The reference's render() (ky.cpp:3689-3729) reports
 * its progress per row (3703) and has the picture only at the end; here a frame keeps its own accumulator block on the device, each pass adds whole chunks
 * of every pixel's samples to it (render_tiles_device with a FramePass, ky_launch.hip), and the picture so far can be resolved, saved and loaded between
 * passes.  Which chunks a pass renders is host arithmetic (ky_shard.hpp); where a checkpoint's parts lie, its host-side parts and what a frame loads are
 * described once in ky_checkpoint.hpp (defined in ky_pack.cpp), and so are the stop rule's argument checks (ky_host.hpp).  HIP runtime calls only: no
 * kernel is defined here.  A frame that tracks noise (kyhip_frame_track_noise; DESIGN.md "Noise") also owns a per-pixel estimate that every pass advances behind its
 * render kernel: the arithmetic is ky_noise.hpp's, the kernels ky_noise.hip's.  A frame that tracks blocks (kyhip_frame_track_blocks; DESIGN.md "Adaptive") retires
 * pixel blocks between its passes and renders the live ones only: the arithmetic is ky_blocks.hpp's, the kernels ky_blocks.hip's, the render kernels' listed form
 * ky_render.hpp's.  A frame may own a range of its samples only (kyhip_frame_begin_slice; DESIGN.md "Slices") and receive what other frames of its scene and params
 * hold (kyhip_frame_merge, _merge_from): what a frame holds is its coverage, the arithmetic of ranges and of a state's acceptance ky_checkpoint.hpp's, the kernel
 * ky_merge.hip's.
 */
#include <cstring>
#include <string>
#include <vector>

#include "ky_checkpoint.hpp"
#include "ky_ctx.hpp"
#include "ky_denoise.hpp"

using namespace kyh;
using namespace kyn;
using namespace kyb;
using namespace kydn;

// An event pair around the last kernel of a kind, for the _ms entries: -1 until `valid` is set, behind the wait for a span that was enqueued whole
struct TimedSpan {
    hipEvent_t ev[2] = {};
    bool valid = false;
    ~TimedSpan() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int create() {
        for (hipEvent_t& e : ev) if (!e) HIP_TRY(hipEventCreate(&e));
        return KY_OK;
    }
    void begin(hipStream_t s) { (void)hipEventRecord(ev[0], s); }
    void end(hipStream_t s) { (void)hipEventRecord(ev[1], s); }
    float ms() const { float v; return valid && hipEventElapsedTime(&v, ev[0], ev[1]) == hipSuccess ? v : -1.f; }
};
// the noise estimate of a frame that tracks it (`on`)
struct NoiseTrack {
    bool on = false;
    int batches = 0, n_prev = 0;       // updates so far and the samples done at the last one (the per-pixel state stands at n_prev)
    DevBuf state, map, cls, sums;      // n_pix NoisePixel; the map (compact tile order) and the pixels' classes; the statistics' partials and their result
    std::vector<float> hmap;           // host copies of the map and the classes
    std::vector<unsigned char> hcls;
    TimedSpan update, stats;           // the last update kernel; the last map + statistics (kyhip_frame_noise_ms)
};
// the blocks of a frame that retires them (`on`): every pass is a listed one (FramePass::n_live), the live list lies in `ws` behind the flag words
struct BlockTrack {
    bool on = false;
    int n_live = 0, passes = 0;
    DevBuf state, scratch, mask;       // n_blocks BlockState; the compaction's counts and n_live; kyhip_frame_keep's mask
    std::vector<BlockState> host;      // the host's copy of `state`: current behind every call
    std::vector<int> inside;           // per block, its pixels inside the film
    TimedSpan rule, list;              // the last retire / keep kernel; the last compaction (kyhip_frame_blocks_ms)
};
// what kyhip_frame_denoise keeps between calls (no part of a checkpoint): the guides, traced once per frame, and the filter's film-order buffers
struct DenoiseTrack {
    bool guides_done = false;
    DevBuf ga, gb_traced, gb, cv[2];   // width x height Px4 each: {n, t}; {P, class} as traced and as the frame's state classes it now; the levels' ping-pong
    std::vector<float> hga, hgb;       // host copies of the guides (kyhip_frame_guides)
    TimedSpan guides, filter;          // the guide trace; the last call's gather, levels and add (kyhip_frame_denoise_ms)
};
struct kyhip_frame {
    int device = 0;
    ky_render_params params{};
    // the caller's scene, copied: `scene` points into these
    std::vector<ky_shape> shapes;
    std::vector<ky_material> materials;
    std::vector<ky_light> lights;
    std::vector<ky_surface> surfaces;
    ky_scene scene{};
    ShardConst sh{};
    ChunkPlan plan{};
    FrameHeader header{};         // with samples_done = 0
    CheckpointLayout layout;      // of what the frame tracks now (retrack)
    int own_first = 0, own_end = 0;   // the samples the frame owns and renders, and ...
    int own_c0 = 0, own_c1 = 0;       // ... the chunks they are
    int chunks_done = 0;          // the chunks before the frame's front: own_c0 .. own_c1
    Coverage cov;                 // the samples the accumulators hold: [own_first, front) and what was merged
    bool loaded = false;
    FramePass pass;               // the frame's accumulator block and the kernel its first pass took
    DevBuf ws, tiles, film;       // accumulators + flag words; resolve's compact tile buffer; resolve's device film (pageable host films)
    std::vector<float> stage;     // ... and its host copy
    NoiseTrack noise;
    BlockTrack blocks;
    DenoiseTrack denoise;
    DevBuf merge_ws, merge_state; // what a merge from a saved state or from another device reads: the other frame's accumulator block and noise pairs
    TimedSpan merge;              // the last merge kernel (kyhip_frame_merge_ms)
};

// the frame's front: the absolute sample its owned range is rendered to; and the samples per pixel it holds -- the same for a frame that owns all and merged nothing
static int samples_done(const kyhip_frame* f) { return chunk_end(f->plan, f->chunks_done - 1); }
static int samples_held(const kyhip_frame* f) { return f->cov.held(); }
static bool owned_rendered(const kyhip_frame* f) { return f->chunks_done >= f->own_c1; }
static bool untouched(const kyhip_frame* f) { return f->chunks_done == f->own_c0 && f->cov.n == 0 && !f->loaded; }
static void retrack(kyhip_frame* f) { f->layout = checkpoint_layout(&f->params, f->noise.on, f->blocks.on, f->own_first, f->own_end); }
static const void* block_state_or_null(const kyhip_frame* f) { return f->blocks.on ? f->blocks.state.p : nullptr; }

// Waits for what was enqueued on `stream`, also after a failed enqueue, whose status `rcode` comes first; then the device's, as "<what> failed: <error><tail>"
static int finish(hipStream_t stream, int rcode, const char* what, const char* tail = "") {
    const hipError_t e = hipStreamSynchronize(stream);
    if (rcode != KY_OK) return rcode;
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "%s failed: %s%s", what, hipGetErrorString(e), tail);
    return KY_OK;
}

// The live list (into the frame's accumulator block, behind the flag words) and its length from the device's block state, which comes home too: enqueued and
// waited for.  Behind every call that changes the state.
static int blocks_refresh(kyhip_frame* f) {
    BlockTrack& b = f->blocks;
    if (f->sh.n_blocks <= 0) { b.n_live = 0; return KY_OK; }
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    int* list = (int*)((char*)f->ws.p + blocks_list_offset(f->sh));
    b.list.begin(c->stream);
    const int rcode = blocks_compact_device(b.state.p, f->sh.n_blocks, list, b.scratch.p, c->stream);
    b.list.end(c->stream);
    KY_TRY(finish(c->stream, rcode, "block list"));
    int n_live = -1;
    HIP_TRY(hipMemcpy(&n_live, b.scratch.as<int>() + blocks_groups(f->sh.n_blocks), sizeof n_live, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b.host.data(), b.state.p, b.host.size() * sizeof(BlockState), hipMemcpyDeviceToHost));
    if (n_live < 0 || n_live > f->sh.n_blocks) return fail(KY_ERR_DEVICE, "internal: %d live blocks of %d", n_live, f->sh.n_blocks);
    b.n_live = n_live;
    b.list.valid = true;
    return KY_OK;
}
// behind a retire / keep kernel enqueued inside blocks.rule's span (rcode: the enqueue's status): the state it changed comes home
static int blocks_changed(kyhip_frame* f, hipStream_t stream, int rcode) {
    if (rcode != KY_OK) { (void)hipStreamSynchronize(stream); return rcode; }
    f->blocks.rule.valid = true;
    return blocks_refresh(f);
}

// a block-tracking frame all of whose blocks are retired: no pass renders anything any more and the front stays (a shard without blocks is none: its bookkeeping
// advances like a plain frame's)
static bool nothing_live(const kyhip_frame* f) { return f->blocks.on && f->sh.n_blocks > 0 && f->blocks.n_live == 0; }

static void block_stats_of(const kyhip_frame* f, ky_block_stats* out) {
    const BlockTrack& b = f->blocks;
    std::memset(out, 0, sizeof *out);
    const int front = samples_done(f);
    out->blocks = f->sh.n_blocks;
    out->live = b.n_live;
    out->passes = b.passes;
    out->samples_done = front;
    bool any = false;
    for (size_t i = 0; i < b.host.size(); ++i) {
        if (b.inside[i] == 0) continue;
        const int n = block_samples(b.host[i], front);
        out->pixels += b.inside[i];
        out->pixel_samples += (int64_t)b.inside[i] * n;
        if (!any || n < out->min_samples) out->min_samples = n;
        if (!any || n > out->max_samples) out->max_samples = n;
        any = true;
    }
}
// what the entries of a frame that tracks something refuse first: KY_OK, or KY_ERR_INVALID_VALUE with the message
static int frame_tracks(const kyhip_frame* f, bool blocks, bool noise) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (blocks && !f->blocks.on) return fail(KY_ERR_INVALID_VALUE, "the frame does not track blocks (kyhip_frame_track_blocks)");
    if (noise && !f->noise.on) return fail(KY_ERR_INVALID_VALUE, "the frame does not track noise (kyhip_frame_track_noise)");
    return KY_OK;
}

// kyhip_frame_begin and kyhip_frame_begin_slice: the frame that owns samples [first_sample, end_sample)
static int frame_begin(int device, const ky_scene* scene, const ky_render_params* p, int first_sample, int end_sample, kyhip_frame** out) {
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params (integrator %d, direct_sample %d)", p ? p->integrator : -1, p ? p->direct_sample : -1);
    if (!shard_in_range(p)) return fail(KY_ERR_LIMIT, "frame too large for the device's 32-bit work-item and pixel indices (%d x %d, %d spp)", p->width, p->height, p->samples_per_pixel);
    if (film_range_check(p, scene) != KY_OK) return KY_ERR_LIMIT;
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    *out = nullptr;
    KY_TRY(slice_range_check(p->samples_per_pixel, first_sample, end_sample));
    DeviceCtx* c;
    KY_TRY(get_ctx(device, &c));
    static thread_local DScene packed;
    KY_TRY(pack_scene(scene, &packed));   // (refuses a missing or malformed scene with the statuses kyhip_render gives)
    std::unique_ptr<kyhip_frame> f(new kyhip_frame);
    f->device = device;
    f->params = *p;
    f->scene = *scene;
    f->shapes.assign(scene->shapes, scene->shapes + scene->shape_count);
    f->materials.assign(scene->materials, scene->materials + scene->material_count);
    f->lights.assign(scene->lights, scene->lights + scene->light_count);
    f->surfaces.assign(scene->surfaces, scene->surfaces + scene->surface_count);
    f->scene.shapes = f->shapes.data(); f->scene.materials = f->materials.data(); f->scene.lights = f->lights.data(); f->scene.surfaces = f->surfaces.data();
    f->sh = make_shard(p);
    f->plan = chunk_plan(p->samples_per_pixel);
    f->own_first = first_sample; f->own_end = end_sample;
    f->own_c0 = chunks_at_sample(f->plan, first_sample); f->own_c1 = chunks_at_sample(f->plan, end_sample);
    f->chunks_done = f->own_c0;
    f->header = frame_header(p, scene_hash(packed), 0);
    if (f->sh.n_pix > 0) {
        const size_t bytes = workspace_bytes_for(f->sh) + blocks_list_bytes(f->sh);   // (the live list of a frame that tracks blocks: behind the flag words)
        HIP_TRY(f->ws.alloc(bytes));
        HIP_TRY(f->tiles.alloc((size_t)f->sh.n_pix * 3 * sizeof(float)));
        HIP_TRY(hipMemsetAsync(f->ws.p, 0, bytes, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    f->pass.ws = f->ws.p;
    retrack(f.get());
    *out = f.release();
    return KY_OK;
}

extern "C" {

int kyhip_frame_begin(int device, const ky_scene* scene, const ky_render_params* p, kyhip_frame** out) {
    return frame_begin(device, scene, p, 0, p ? p->samples_per_pixel : 0, out);   // (invalid params are refused before the range is looked at)
}
int kyhip_frame_begin_slice(int device, const ky_scene* scene, const ky_render_params* p, int first_sample, int end_sample, kyhip_frame** out) {
    return frame_begin(device, scene, p, first_sample, end_sample, out);
}

int kyhip_frame_coverage(const kyhip_frame* f, int* ranges2, int n, int own[2]) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (n > 0 && !ranges2) return fail(KY_ERR_INVALID_VALUE, "ranges2 is NULL");
    for (int i = 0; i < f->cov.n && i < n; ++i) { ranges2[2 * i] = f->cov.r[2 * i]; ranges2[2 * i + 1] = f->cov.r[2 * i + 1]; }
    if (own) { own[0] = f->own_first; own[1] = f->own_end; }
    return f->cov.n;
}

int kyhip_frame_samples(const kyhip_frame* f, int* done, int* total) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (done) *done = samples_held(f);
    if (total) *total = f->params.samples_per_pixel;
    return KY_OK;
}

int kyhip_frame_render(kyhip_frame* f, int min_samples, int* done) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (min_samples < 1) return fail(KY_ERR_INVALID_VALUE, "min_samples %d: a pass renders at least one sample per pixel", min_samples);
    int c1 = pass_chunk_end(f->plan, f->chunks_done, min_samples);
    if (c1 > f->own_c1) c1 = f->own_c1;   // (a slice ends where its owned range does)
    if (nothing_live(f)) {   // every block is retired: nothing is launched and the front stays
        if (done) *done = samples_held(f);
        return KY_OK;
    }
    if (c1 > f->chunks_done) {
        // what the frame holds behind the pass: its front moves, and the estimate's batch is the samples the pass adds to the held ones
        Coverage pass_range, held_then;
        pass_range.n = 1; pass_range.r[0] = samples_done(f); pass_range.r[1] = chunk_end(f->plan, c1 - 1);
        KY_TRY(coverage_union(f->cov, pass_range, &held_then));
        const int n_now = held_then.held();
        if (f->sh.n_pix > 0) {
            DeviceCtx* c;
            KY_TRY(get_ctx(f->device, &c));
            if (f->blocks.on) f->pass.n_live = f->blocks.n_live;
            f->pass.chunk_first = f->chunks_done;
            f->pass.chunk_count = c1 - f->chunks_done;
            int rcode = render_tiles_device(f->device, &f->scene, &f->params, nullptr, nullptr, 0, c->stream, 0, nullptr, &f->pass);
            if (rcode == KY_OK && f->noise.on) {   // the batch this pass adds, behind its render kernel
                f->noise.update.begin(c->stream);
                rcode = noise_update_device(f->ws.p, f->noise.state.p, f->sh, f->params.samples_per_pixel, f->noise.n_prev, n_now, block_state_or_null(f), c->stream);
                f->noise.update.end(c->stream);
            }
            KY_TRY(finish(c->stream, rcode, "pass", " (the frame's accumulators may hold a part of it)"));   // (blocking)
            if (f->noise.on) f->noise.update.valid = true;
        }
        // the bookkeeping, behind the pass's synchronisation (a failed pass is not counted) and alone for a shard without pixels
        if (f->noise.on) { f->noise.batches += 1; f->noise.n_prev = n_now; }
        if (f->blocks.on) f->blocks.passes += 1;
        f->cov = held_then;
    }
    f->chunks_done = c1;
    if (done) *done = samples_held(f);
    return KY_OK;
}

int kyhip_frame_resolve(kyhip_frame* f, int normalise, float* film_rgb, size_t stride_px) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (normalise != 0 && normalise != 1) return fail(KY_ERR_INVALID_VALUE, "normalise %d: 0 (sum / total) or 1 (sum / done)", normalise);
    const ky_render_params* p = &f->params;
    if (!film_rgb || stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    const int done = samples_held(f);
    const BlockTrack& bl = f->blocks;
    if (bl.on && !normalise)
        for (size_t b = 0; b < bl.host.size(); ++b)
            if (bl.inside[b] > 0 && bl.host[b].retired_at >= 0 && bl.host[b].retired_at < p->samples_per_pixel)
                return fail(KY_ERR_INVALID_VALUE, "normalise 0 on a frame with blocks retired short of its %d samples (block %zu at %d): sum / total would darken them; normalise 1",
                            p->samples_per_pixel, b, bl.host[b].retired_at);
    if (f->sh.n_pix == 0 || (normalise && done == 0)) return KY_OK;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    const double scale = normalise ? (double)p->samples_per_pixel / (double)done : 1.0;
    int rcode;
    if (bl.on && normalise) rcode = blocks_resolve_device(f->ws.p, bl.state.p, f->tiles.as<float>(), f->sh, p->samples_per_pixel, done, c->stream);
    else rcode = resolve_frame_device(f->ws.p, f->tiles.as<float>(), f->sh.n_pix, scale, c->stream);
    if (rcode != KY_OK) return rcode;
    const size_t span = ((size_t)(p->height - 1) * stride_px + (size_t)p->width) * 3 * sizeof(float);
    if (float* alias = film_in_place_alias(film_rgb, span)) {   // a pinned film: film_t::add_color by the GPU, where the film lies
        rcode = kyhip_film_add_tiles_device(f->device, p, f->tiles.as<float>(), alias, stride_px, c->stream);
        return finish(c->stream, rcode, "resolve");
    }
    // any other film: de-interleaved into a device film, brought home, added by the host (film_t::add_color, 1586-1590)
    const size_t film_floats = (size_t)p->width * p->height * 3;
    if (!f->film.p) HIP_TRY(f->film.alloc(film_floats * sizeof(float)));
    f->stage.resize(film_floats);
    HIP_TRY(hipMemsetAsync(f->film.p, 0, film_floats * sizeof(float), c->stream));
    rcode = kyhip_film_add_tiles_device(f->device, p, f->tiles.as<float>(), f->film.as<float>(), (size_t)p->width, c->stream);
    KY_TRY(finish(c->stream, rcode, "resolve"));
    const hipError_t e = hipMemcpy(f->stage.data(), f->film.p, film_floats * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "resolve failed: %s", hipGetErrorString(e));
    host_add_rows(film_rgb, stride_px, f->stage.data(), p->width, 0, p->height);
    return KY_OK;
}

int64_t kyhip_frame_state_bytes(const kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return (int64_t)f->layout.total;
}

// (a checkpoint's parts and what a frame loads: ky_checkpoint.hpp; here only the copies of the parts that live on the device, at the layout's offsets)
int kyhip_frame_save(kyhip_frame* f, void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const CheckpointLayout& L = f->layout;
    if (!buf || bytes < L.total) return fail(KY_ERR_INVALID_VALUE, "frame state: a buffer of %zu bytes, the state has %zu", bytes, L.total);
    CheckpointCounts n;
    n.samples_done = samples_held(f);
    n.front = samples_done(f); n.cov = f->cov;
    n.batches = f->noise.batches; n.n_prev = f->noise.n_prev; n.passes = f->blocks.passes;
    checkpoint_write_host(f->header, L, n, f->blocks.host.data(), buf);   // (the host's block states are current: every call that changes the device's brings them home)
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        HIP_TRY(hipMemcpy((char*)buf + L.accum, f->ws.p, L.accum_bytes(), hipMemcpyDeviceToHost));   // (passes are blocking: nothing of the frame is in flight)
        if (f->noise.on) HIP_TRY(hipMemcpy((char*)buf + L.noise_pixels, f->noise.state.p, L.noise_pixels_bytes(), hipMemcpyDeviceToHost));
    }
    return KY_OK;
}

int kyhip_frame_load(kyhip_frame* f, const void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const CheckpointLayout& L = f->layout;
    CheckpointCounts n;
    KY_TRY(checkpoint_check(f->header, L, buf, bytes, &n));
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        HIP_TRY(hipMemcpy(f->ws.p, (const char*)buf + L.accum, L.accum_bytes(), hipMemcpyHostToDevice));
        if (f->noise.on) HIP_TRY(hipMemcpy(f->noise.state.p, (const char*)buf + L.noise_pixels, L.noise_pixels_bytes(), hipMemcpyHostToDevice));
    }
    // (the frame is left untouched by every REFUSAL above; a copy that fails half way is a device error, KY_ERR_DEVICE, behind which the frame's accumulators and
    // pairs may disagree with its counts, which are advanced only here, behind both copies: such a frame is to be ended or loaded again)
    if (f->noise.on) { f->noise.batches = n.batches; f->noise.n_prev = n.n_prev; }
    if (f->blocks.on) f->blocks.passes = n.passes;
    if (f->blocks.on && f->sh.n_blocks > 0) {
        HIP_TRY(hipMemcpy(f->blocks.state.p, (const char*)buf + L.block_states, L.block_states_bytes(), hipMemcpyHostToDevice));
        KY_TRY(blocks_refresh(f));
    }
    f->chunks_done = n.chunks_done;
    f->cov = n.cov;
    f->loaded = true;
    return KY_OK;
}

// ---- the noise estimate (DESIGN.md "Noise") ----
int kyhip_frame_track_noise(kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    NoiseTrack& t = f->noise;
    if (t.on) return KY_OK;
    if (!untouched(f)) return fail(KY_ERR_INVALID_VALUE, "noise is tracked from a frame's first pass: this one has rendered, loaded or merged something");
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        const size_t n = (size_t)f->sh.n_pix;
        HIP_TRY(t.state.alloc(n * sizeof(NoisePixel)));
        HIP_TRY(t.map.alloc(n * sizeof(float)));
        HIP_TRY(t.cls.alloc(n));
        HIP_TRY(t.sums.alloc(((size_t)noise_blocks(f->sh.n_pix) + 1) * sizeof(NoiseSums)));
        KY_TRY(t.update.create());
        KY_TRY(t.stats.create());
        HIP_TRY(hipMemsetAsync(t.state.p, 0, n * sizeof(NoisePixel), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    t.on = true;
    retrack(f);
    return KY_OK;
}

// the map and the classes (device), and with `sums` the statistics against `threshold`: enqueued and waited for
static int noise_map_and_stats(kyhip_frame* f, float threshold, NoiseSums* sums) {
    NoiseTrack& t = f->noise;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    t.stats.begin(c->stream);
    int rcode = noise_map_device(f->ws.p, t.state.p, t.map.as<float>(), t.cls.as<unsigned char>(), f->sh, f->params.width, f->params.height, t.batches, t.n_prev,
                             block_state_or_null(f), c->stream);
    if (rcode == KY_OK && sums) rcode = noise_stats_device(t.map.as<float>(), t.cls.as<unsigned char>(), f->sh.n_pix, threshold, t.sums.p, c->stream);
    t.stats.end(c->stream);
    KY_TRY(finish(c->stream, rcode, "noise map"));
    t.stats.valid = true;
    if (sums) HIP_TRY(hipMemcpy(sums, t.sums.as<NoiseSums>() + noise_blocks(f->sh.n_pix), sizeof *sums, hipMemcpyDeviceToHost));
    return KY_OK;
}

int kyhip_frame_noise(kyhip_frame* f, float* map, size_t stride_px) {
    KY_TRY(frame_tracks(f, false, true));
    if (!map || stride_px < (size_t)f->params.width) return fail(KY_ERR_INVALID_VALUE, "bad map arguments");
    if (f->sh.n_pix == 0) return KY_OK;
    KY_TRY(noise_map_and_stats(f, 0.f, nullptr));
    NoiseTrack& t = f->noise;
    const size_t n = (size_t)f->sh.n_pix;
    t.hmap.resize(n);
    t.hcls.resize(n);
    HIP_TRY(hipMemcpy(t.hmap.data(), t.map.p, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t.hcls.data(), t.cls.p, n, hipMemcpyDeviceToHost));
    for (int i = 0; i < f->sh.n_pix; ++i) {
        if (t.hcls[(size_t)i] == KY_NOISE_PADDING) continue;
        int x, y;
        noise_pixel_xy(f->sh, i, x, y);
        map[(size_t)y * stride_px + (size_t)x] = t.hmap[(size_t)i];
    }
    return KY_OK;
}

int kyhip_frame_noise_stats(kyhip_frame* f, float threshold, ky_noise_stats* out) {
    KY_TRY(threshold_check(threshold));
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    KY_TRY(frame_tracks(f, false, true));
    NoiseSums s = {};
    if (f->sh.n_pix > 0) {
        KY_TRY(noise_map_and_stats(f, threshold, &s));
    }
    std::memset(out, 0, sizeof *out);
    out->batches = f->noise.batches;
    out->samples_done = samples_held(f);
    out->pixels = s.pixels; out->flagged = s.flagged; out->above = s.above;
    out->threshold = threshold;
    out->max = s.max;
    out->mean = s.pixels - s.flagged > 0 ? s.sum / (double)(s.pixels - s.flagged) : 0.0;
    return KY_OK;
}

int kyhip_frame_render_until(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int* done, ky_noise_stats* out) {
    KY_TRY(stop_rule_check(threshold, max_fraction_above, min_batches));
    KY_TRY(pass_samples_check(min_samples_per_pass));
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    KY_TRY(frame_tracks(f, false, true));
    for (;;) {
        KY_TRY(kyhip_frame_render(f, min_samples_per_pass, done));
        KY_TRY(kyhip_frame_noise_stats(f, threshold, out));
        const bool clean = out->batches >= min_batches && (double)out->above <= (double)max_fraction_above * (double)(out->pixels - out->flagged);
        // (a block-tracking frame without a live block renders no further: its front and its map stay what they are, and so would this verdict)
        if (clean || owned_rendered(f) || nothing_live(f)) return KY_OK;
    }
}

// ---- blocks that retire between passes (DESIGN.md "Adaptive") ----
int kyhip_frame_track_blocks(kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    BlockTrack& b = f->blocks;
    if (b.on) return KY_OK;
    if (f->layout.sliced)
        return fail(KY_ERR_INVALID_VALUE, "the frame owns samples %d..%d of %d: blocks retire on a frame that owns them all (per-block sample counts across slices are not kept)",
                    f->own_first, f->own_end, f->params.samples_per_pixel);
    if (!untouched(f)) return fail(KY_ERR_INVALID_VALUE, "blocks are tracked from a frame's first pass: this one has rendered or loaded something");
    const int nb = f->sh.n_blocks;
    b.host.assign((size_t)nb, BlockState{-1, 0});
    b.inside.assign((size_t)nb, 0);
    for (int i = 0; i < f->sh.n_pix; ++i)
        if (pixel_inside(f->sh, i, f->params.width, f->params.height)) b.inside[(size_t)block_of_pixel(f->sh, i)] += 1;
    if (nb > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        if (!b.state.p) HIP_TRY(b.state.alloc((size_t)nb * sizeof(BlockState)));
        if (!b.scratch.p) HIP_TRY(b.scratch.alloc(blocks_scratch_bytes(nb)));
        if (!b.mask.p) HIP_TRY(b.mask.alloc((size_t)f->params.width * (size_t)f->params.height));
        KY_TRY(b.rule.create());
        KY_TRY(b.list.create());
        KY_TRY(blocks_init_device(b.state.p, f->sh, f->params.width, f->params.height, c->stream));
        KY_TRY(blocks_refresh(f));
    }
    b.on = true;
    retrack(f);   // (the checkpoints' magic changes with the layout: plain frames refuse this one's states and it theirs)
    return KY_OK;
}

int kyhip_frame_keep(kyhip_frame* f, const unsigned char* mask, size_t row_stride) {
    if (!mask) return fail(KY_ERR_INVALID_VALUE, "mask is NULL");
    KY_TRY(frame_tracks(f, true, false));
    const size_t w = (size_t)f->params.width, h = (size_t)f->params.height;
    if (row_stride < w) return fail(KY_ERR_INVALID_VALUE, "row_stride %zu: the mask's rows are %zu bytes", row_stride, w);
    if (f->sh.n_blocks == 0) return KY_OK;
    BlockTrack& b = f->blocks;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    HIP_TRY(hipMemcpy2D(b.mask.p, w, mask, row_stride, w, h, hipMemcpyHostToDevice));
    b.rule.begin(c->stream);
    const int rcode = blocks_keep_device(b.state.p, b.mask.as<unsigned char>(), f->sh, f->params.width, f->params.height, samples_done(f), f->noise.batches, c->stream);
    b.rule.end(c->stream);
    return blocks_changed(f, c->stream, rcode);
}

// what both adaptive entries refuse after their arguments
static int adaptive_frame(const kyhip_frame* f, const ky_block_stats* out) {
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    return frame_tracks(f, true, true);
}

int kyhip_frame_retire_noisy(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, ky_block_stats* out) {
    KY_TRY(stop_rule_check(threshold, max_fraction_above, min_batches));
    KY_TRY(adaptive_frame(f, out));
    BlockTrack& b = f->blocks;
    if (b.n_live > 0) {
        KY_TRY(noise_map_and_stats(f, threshold, nullptr));   // the map at the current state (retired blocks: frozen)
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        b.rule.begin(c->stream);
        const int rcode = blocks_retire_device(b.state.p, f->noise.map.as<float>(), f->noise.cls.as<unsigned char>(), f->sh, threshold, max_fraction_above, min_batches, samples_done(f),
                                     f->noise.batches, c->stream);
        b.rule.end(c->stream);
        KY_TRY(blocks_changed(f, c->stream, rcode));
    }
    block_stats_of(f, out);
    return KY_OK;
}

int kyhip_frame_render_adaptive(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int* done, ky_block_stats* out) {
    KY_TRY(stop_rule_check(threshold, max_fraction_above, min_batches));
    KY_TRY(pass_samples_check(min_samples_per_pass));
    KY_TRY(adaptive_frame(f, out));
    for (;;) {
        KY_TRY(kyhip_frame_render(f, min_samples_per_pass, done));
        KY_TRY(kyhip_frame_retire_noisy(f, threshold, max_fraction_above, min_batches, out));
        if (nothing_live(f) || samples_done(f) >= f->params.samples_per_pixel) return KY_OK;
    }
}

int kyhip_frame_sample_map(kyhip_frame* f, int32_t* map, size_t stride_px) {
    KY_TRY(frame_tracks(f, true, false));
    if (!map || stride_px < (size_t)f->params.width) return fail(KY_ERR_INVALID_VALUE, "bad map arguments");
    const int front = samples_done(f);
    for (int i = 0; i < f->sh.n_pix; ++i) {
        int x, y;
        if (!pixel_inside(f->sh, i, f->params.width, f->params.height, &x, &y)) continue;
        map[(size_t)y * stride_px + (size_t)x] = block_samples(f->blocks.host[(size_t)block_of_pixel(f->sh, i)], front);
    }
    return KY_OK;
}

int kyhip_frame_block_stats(kyhip_frame* f, ky_block_stats* out) {
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    KY_TRY(frame_tracks(f, true, false));
    block_stats_of(f, out);
    return KY_OK;
}

// (-1: no such kernel has run and been waited for yet)
int kyhip_frame_blocks_ms(const kyhip_frame* f, float* retire_ms, float* list_ms) {
    KY_TRY(frame_tracks(f, true, false));
    if (retire_ms) *retire_ms = f->blocks.rule.ms();
    if (list_ms) *list_ms = f->blocks.list.ms();
    return KY_OK;
}

int kyhip_frame_noise_ms(const kyhip_frame* f, float* update_ms, float* stats_ms) {
    KY_TRY(frame_tracks(f, false, true));
    if (update_ms) *update_ms = f->noise.update.ms();
    if (stats_ms) *stats_ms = f->noise.stats.ms();
    return KY_OK;
}

// ---- the denoised picture (DESIGN.md "Denoise") ----
// what the denoise entries refuse of a frame, after their other arguments: KY_OK, or KY_ERR_INVALID_VALUE with the message
static int denoise_frame_check(const kyhip_frame* f, bool needs_variance) {
    KY_TRY(frame_tracks(f, false, true));
    if (f->params.tile_first != 0 || f->params.tile_step != 1)
        return fail(KY_ERR_INVALID_VALUE, "the frame's shard (tile_first %d, tile_step %d) is not the whole film: a shard's neighbours live elsewhere", f->params.tile_first, f->params.tile_step);
    if (needs_variance && f->noise.batches < 2) return fail(KY_ERR_INVALID_VALUE, "%d noise batches: the filter needs a variance, two passes or more", f->noise.batches);
    return KY_OK;
}
// the filter's buffers, the guides (traced on the first call) and the gather of the frame's state as it stands: enqueued, the trace also waited for
static int denoise_prepare(kyhip_frame* f, DeviceCtx* c, bool timed) {
    DenoiseTrack& d = f->denoise;
    const ky_render_params* p = &f->params;
    const size_t bytes = (size_t)p->width * (size_t)p->height * sizeof(Px4);
    for (DevBuf* b : {&d.ga, &d.gb_traced, &d.gb, &d.cv[0], &d.cv[1]})
        if (!b->p) HIP_TRY(b->alloc(bytes));
    KY_TRY(d.guides.create());
    KY_TRY(d.filter.create());
    if (!d.guides_done) {
        d.guides.begin(c->stream);
        const int rcode = denoise_guides_device(f->device, &f->scene, p->width, p->height, d.ga.p, d.gb_traced.p, c->stream);
        d.guides.end(c->stream);
        KY_TRY(finish(c->stream, rcode, "denoise guides"));
        d.guides.valid = d.guides_done = true;
    }
    if (timed) {   // (kyhip_frame_denoise: its span begins with the gather)
        d.filter.valid = false;
        d.filter.begin(c->stream);
    }
    return denoise_gather_device(f->ws.p, f->noise.state.p, block_state_or_null(f), f->sh, p->width, p->height, p->samples_per_pixel, samples_held(f), f->noise.batches,
                                 d.gb_traced.p, d.cv[0].p, d.gb.p, c->stream);
}

int kyhip_frame_denoise(kyhip_frame* f, const ky_denoise_params* params, float* film_rgb, size_t stride_px) {
    ky_denoise_params q;
    kyhip_denoise_defaults(&q);
    if (params) q = *params;
    KY_TRY(denoise_params_check(&q));
    KY_TRY(denoise_frame_check(f, true));
    const ky_render_params* p = &f->params;
    if (!film_rgb || stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    if (q.levels == 0) return kyhip_frame_resolve(f, 1, film_rgb, stride_px);
    if (f->sh.n_pix == 0) return KY_OK;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    DenoiseTrack& d = f->denoise;
    int rcode = denoise_prepare(f, c, true);
    if (rcode != KY_OK) return finish(c->stream, rcode, "denoise");   // (nothing of the filter is enqueued; its span stays invalid)
    LevelConst k{};
    k.width = p->width; k.height = p->height;
    k.normal_squarings = q.normal_squarings;
    k.sigma_l2 = (double)q.sigma_luminance * (double)q.sigma_luminance;
    k.sigma_plane = (double)q.sigma_plane;
    k.pix = denoise_pixel_width(f->scene.camera, p->width);
    for (int l = 0; l < q.levels && rcode == KY_OK; ++l) rcode = denoise_level_device(d.cv[l & 1].p, d.cv[(l + 1) & 1].p, d.ga.p, d.gb.p, 1 << l, k, c->stream);
    const void* result = d.cv[q.levels & 1].p;
    const size_t span = ((size_t)(p->height - 1) * stride_px + (size_t)p->width) * 3 * sizeof(float);
    if (float* alias = film_in_place_alias(film_rgb, span)) {   // a pinned film: added to where it lies
        if (rcode == KY_OK) rcode = denoise_add_device(result, alias, stride_px, p->width, p->height, c->stream);
        d.filter.end(c->stream);
        KY_TRY(finish(c->stream, rcode, "denoise"));
        d.filter.valid = true;
        return KY_OK;
    }
    // any other film: added into the frame's device film, brought home, added by the host (kyhip_frame_resolve's path)
    const size_t film_floats = (size_t)p->width * p->height * 3;
    if (!f->film.p && rcode == KY_OK) {
        const hipError_t e = f->film.alloc(film_floats * sizeof(float));
        if (e != hipSuccess) rcode = fail(KY_ERR_DEVICE, "denoise failed: %s", hipGetErrorString(e));
    }
    if (rcode == KY_OK) {
        f->stage.resize(film_floats);
        const hipError_t e = hipMemsetAsync(f->film.p, 0, film_floats * sizeof(float), c->stream);
        if (e != hipSuccess) rcode = fail(KY_ERR_DEVICE, "denoise failed: %s", hipGetErrorString(e));
    }
    if (rcode == KY_OK) rcode = denoise_add_device(result, f->film.as<float>(), (size_t)p->width, p->width, p->height, c->stream);
    d.filter.end(c->stream);
    KY_TRY(finish(c->stream, rcode, "denoise"));
    d.filter.valid = true;
    const hipError_t e = hipMemcpy(f->stage.data(), f->film.p, film_floats * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "denoise failed: %s", hipGetErrorString(e));
    host_add_rows(film_rgb, stride_px, f->stage.data(), p->width, 0, p->height);
    return KY_OK;
}

int kyhip_frame_guides(kyhip_frame* f, float* normal_t4, float* position_class4, size_t stride_px) {
    KY_TRY(denoise_frame_check(f, false));
    const ky_render_params* p = &f->params;
    if (stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "row_stride_px %zu: the guides' rows are %d pixels", stride_px, p->width);
    if (f->sh.n_pix == 0) return KY_OK;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    DenoiseTrack& d = f->denoise;
    const int rcode = denoise_prepare(f, c, false);
    KY_TRY(finish(c->stream, rcode, "denoise guides"));
    const size_t n = (size_t)p->width * (size_t)p->height * 4;
    d.hga.resize(n);
    d.hgb.resize(n);
    HIP_TRY(hipMemcpy(d.hga.data(), d.ga.p, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(d.hgb.data(), d.gb.p, n * sizeof(float), hipMemcpyDeviceToHost));
    for (int y = 0; y < p->height; ++y) {
        const size_t row = (size_t)p->width * 4 * sizeof(float);
        if (normal_t4) std::memcpy(normal_t4 + (size_t)y * stride_px * 4, d.hga.data() + (size_t)y * p->width * 4, row);
        if (position_class4) std::memcpy(position_class4 + (size_t)y * stride_px * 4, d.hgb.data() + (size_t)y * p->width * 4, row);
    }
    return KY_OK;
}

int kyhip_frame_denoise_ms(const kyhip_frame* f, float* guides_ms, float* filter_ms) {
    KY_TRY(frame_tracks(f, false, true));
    if (guides_ms) *guides_ms = f->denoise.guides.ms();
    if (filter_ms) *filter_ms = f->denoise.filter.ms();
    return KY_OK;
}

}  // extern "C"

// ---- merging what other frames hold (DESIGN.md "Slices") ----
// The kernel and, behind it, the bookkeeping: src_ws / src_state are device memory of f's device (src_state is read where f tracks noise), the other frame held
// n_src samples in src_batches noise batches, `merged` is merge_accept's union.  Blocking; a failed merge is not counted.
static int merge_apply(kyhip_frame* f, const void* src_ws, const void* src_state, int n_src, int src_batches, const Coverage& merged) {
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        f->merge.valid = false;
        f->merge.begin(c->stream);
        const int rcode = merge_device(f->ws.p, src_ws, f->noise.on ? f->noise.state.p : nullptr, src_state, f->sh.n_pix, f->params.samples_per_pixel, samples_held(f), n_src, c->stream);
        f->merge.end(c->stream);
        KY_TRY(finish(c->stream, rcode, "merge", " (the frame's accumulators may hold a part of it)"));
        f->merge.valid = true;
    }
    if (f->noise.on) { f->noise.batches += src_batches; f->noise.n_prev = merged.held(); }
    f->cov = merged;
    return KY_OK;
}
// the buffers a merge stages the other frame's parts in, allocated on the first merge that needs them (the device is current)
static int merge_staging(kyhip_frame* f) {
    if (!f->merge_ws.p) HIP_TRY(f->merge_ws.alloc(workspace_bytes_for(f->sh)));
    if (f->noise.on && !f->merge_state.p) HIP_TRY(f->merge_state.alloc((size_t)f->sh.n_pix * sizeof(NoisePixel)));
    return KY_OK;
}
extern "C" {

int kyhip_frame_merge(kyhip_frame* f, const void* state, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    MergeSource m;
    KY_TRY(merge_source_check(f->header, state, bytes, &m));
    Coverage merged;
    KY_TRY(merge_accept(f->cov, f->own_first, f->own_end, f->params.samples_per_pixel, f->noise.on, f->blocks.on, m.cov, m.noise_pixels != 0, &merged));
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        KY_TRY(f->merge.create());
        KY_TRY(merge_staging(f));
        HIP_TRY(hipMemcpy(f->merge_ws.p, (const char*)state + m.accum, workspace_bytes_for(f->sh), hipMemcpyHostToDevice));
        if (f->noise.on) HIP_TRY(hipMemcpy(f->merge_state.p, (const char*)state + m.noise_pixels, (size_t)f->sh.n_pix * sizeof(NoisePixel), hipMemcpyHostToDevice));
    }
    return merge_apply(f, f->merge_ws.p, f->merge_state.p, m.cov.held(), m.batches, merged);
}

int kyhip_frame_merge_from(kyhip_frame* f, kyhip_frame* src) {
    if (!f || !src) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (f == src) return fail(KY_ERR_INVALID_VALUE, "merge: a frame holds its own samples already");
    if (std::memcmp(&f->header, &src->header, sizeof f->header) != 0)
        return fail(KY_ERR_INVALID_VALUE, "merge: the frames differ in their render params, scene or film size");
    if (src->blocks.on) return fail(KY_ERR_INVALID_VALUE, "merge: the other frame retires pixel blocks: its pixels stand at sample counts of their own and merge with nothing");
    Coverage merged;
    KY_TRY(merge_accept(f->cov, f->own_first, f->own_end, f->params.samples_per_pixel, f->noise.on, f->blocks.on, src->cov, src->noise.on, &merged));
    const void* src_ws = src->ws.p;
    const void* src_state = src->noise.state.p;
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        KY_TRY(f->merge.create());
        if (src->device != f->device) {   // (the other frame's calls are blocking: nothing of it is in flight on its device)
            KY_TRY(merge_staging(f));
            HIP_TRY(hipMemcpyPeerAsync(f->merge_ws.p, f->device, src->ws.p, src->device, workspace_bytes_for(f->sh), c->stream));
            if (f->noise.on) HIP_TRY(hipMemcpyPeerAsync(f->merge_state.p, f->device, src->noise.state.p, src->device, (size_t)f->sh.n_pix * sizeof(NoisePixel), c->stream));
            src_ws = f->merge_ws.p; src_state = f->merge_state.p;
        }
    }
    return merge_apply(f, src_ws, src_state, samples_held(src), src->noise.batches, merged);
}

int kyhip_frame_merge_ms(const kyhip_frame* f, float* ms) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (ms) *ms = f->merge.ms();
    return KY_OK;
}

void kyhip_frame_end(kyhip_frame* f) {
    if (!f) return;
    DeviceCtx* c;
    if (get_ctx(f->device, &c) == KY_OK) (void)hipStreamSynchronize(c->stream);   // (the device is current for the buffers' release)
    delete f;
}

}  // extern "C"
