/*
 * ky_frame.cpp -- a frame rendered in passes: kyhip_frame_* (include/kyhip.h; DESIGN.md "Passes").  The reference's render() (ky.cpp:3689-3729) reports
 * its progress per row (3703) and has the picture only at the end; here a frame keeps its own accumulator block on the device, each pass adds whole chunks
 * of every pixel's samples to it (render_tiles_device with a FramePass, ky_launch.hip), and the picture so far can be resolved, saved and loaded between
 * passes.  Which chunks a pass renders and what a checkpoint must agree in is host arithmetic (ky_shard.hpp, ky_pack.cpp); HIP runtime calls only: no
 * kernel is defined here.  A frame that tracks noise (kyhip_frame_track_noise; DESIGN.md "Noise") also owns a per-pixel estimate that every pass advances behind its
 * render kernel: the arithmetic is ky_noise.hpp's, the kernels ky_noise.hip's.  A frame that tracks blocks (kyhip_frame_track_blocks; DESIGN.md "Adaptive") retires
 * pixel blocks between its passes and renders the live ones only: the arithmetic is ky_blocks.hpp's, the kernels ky_blocks.hip's, the render kernels' listed form
 * ky_render.hpp's.
 */
#include <cstring>
#include <string>
#include <vector>

#include "ky_blocks.hpp"
#include "ky_ctx.hpp"
#include "ky_noise.hpp"

using namespace kyh;
using namespace kyn;
using namespace kyb;

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
    int chunks_done = 0;
    FramePass pass;               // the frame's accumulator block and the kernel its first pass took
    DevBuf ws, tiles, film;       // accumulators + flag words; resolve's compact tile buffer; resolve's device film (pageable host films)
    std::vector<float> stage;     // ... and its host copy
    // the noise estimate of a frame that tracks it
    bool track = false, loaded = false;
    int batches = 0, n_prev = 0;  // updates so far and the samples done at the last one (the per-pixel state stands at n_prev)
    DevBuf noise, nmap, ncls, nsums;   // n_pix NoisePixel; the map (compact tile order) and the pixels' classes; the statistics' partials and their result
    std::vector<float> hmap;      // host copies of the map and the classes
    std::vector<unsigned char> hcls;
    // the blocks of a frame that retires them: every pass is a listed one (FramePass::n_live), the live list lies in `ws` behind the flag words
    bool blocks = false;
    int n_live = 0, passes = 0;
    DevBuf bstate, bscratch, bmask;    // n_blocks BlockState; the compaction's counts and n_live; kyhip_frame_keep's mask
    std::vector<BlockState> hblocks;   // the host's copy of bstate: current behind every call
    std::vector<int> hinside;          // per block, its pixels inside the film
    hipEvent_t bev[4] = {};            // around the last retire / keep kernel and the last compaction (kyhip_frame_blocks_ms)
    bool btimed[2] = {false, false};
    hipEvent_t ev[4] = {};        // around the last update kernel / the last map + statistics (kyhip_frame_noise_ms)
    bool timed[2] = {false, false};
    ~kyhip_frame() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : bev) if (e) (void)hipEventDestroy(e);
    }
};

static int samples_done(const kyhip_frame* f) { return chunk_end(f->plan, f->chunks_done - 1); }
// a checkpoint: the state, then the noise trailer of a frame that tracks noise, then the block trailer of one that tracks blocks
static size_t blocks_at(const kyhip_frame* f) { return frame_state_bytes(&f->params) + (f->track ? noise_trailer_bytes(f->sh.n_pix) : 0); }
static size_t state_bytes(const kyhip_frame* f) { return blocks_at(f) + (f->blocks ? block_trailer_bytes(f->sh.n_blocks) : 0); }

// The live list (into the frame's accumulator block, behind the flag words) and its length from the device's block state, which comes home too: enqueued and
// waited for.  Behind every call that changes the state.
static int blocks_refresh(kyhip_frame* f) {
    if (f->sh.n_blocks <= 0) { f->n_live = 0; return KY_OK; }
    DeviceCtx* c;
    int rcode = get_ctx(f->device, &c);
    if (rcode != KY_OK) return rcode;
    int* list = (int*)((char*)f->ws.p + blocks_list_offset(f->sh));
    (void)hipEventRecord(f->bev[2], c->stream);
    rcode = blocks_compact_device(f->bstate.p, f->sh.n_blocks, list, f->bscratch.p, c->stream);
    (void)hipEventRecord(f->bev[3], c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rcode != KY_OK) return rcode;
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "block list failed: %s", hipGetErrorString(e));
    int n_live = -1;
    HIP_TRY(hipMemcpy(&n_live, f->bscratch.as<int>() + blocks_groups(f->sh.n_blocks), sizeof n_live, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(f->hblocks.data(), f->bstate.p, f->hblocks.size() * sizeof(BlockState), hipMemcpyDeviceToHost));
    if (n_live < 0 || n_live > f->sh.n_blocks) return fail(KY_ERR_DEVICE, "internal: %d live blocks of %d", n_live, f->sh.n_blocks);
    f->n_live = n_live;
    f->btimed[1] = true;
    return KY_OK;
}

// a block-tracking frame all of whose blocks are retired: no pass renders anything any more and the front stays (a shard without blocks is none: its bookkeeping
// advances like a plain frame's)
static bool nothing_live(const kyhip_frame* f) { return f->blocks && f->sh.n_blocks > 0 && f->n_live == 0; }

static void block_stats_of(const kyhip_frame* f, ky_block_stats* out) {
    std::memset(out, 0, sizeof *out);
    const int front = samples_done(f);
    out->blocks = f->sh.n_blocks;
    out->live = f->n_live;
    out->passes = f->passes;
    out->samples_done = front;
    bool any = false;
    for (size_t b = 0; b < f->hblocks.size(); ++b) {
        if (f->hinside[b] == 0) continue;
        const int n = block_samples(f->hblocks[b], front);
        out->pixels += f->hinside[b];
        out->pixel_samples += (int64_t)f->hinside[b] * n;
        if (!any || n < out->min_samples) out->min_samples = n;
        if (!any || n > out->max_samples) out->max_samples = n;
        any = true;
    }
}

extern "C" {

int kyhip_frame_begin(int device, const ky_scene* scene, const ky_render_params* p, kyhip_frame** out) {
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params (integrator %d, direct_sample %d)", p ? p->integrator : -1, p ? p->direct_sample : -1);
    if (!shard_in_range(p)) return fail(KY_ERR_LIMIT, "frame too large for the device's 32-bit work-item and pixel indices (%d x %d, %d spp)", p->width, p->height, p->samples_per_pixel);
    if (film_range_check(p, scene) != KY_OK) return KY_ERR_LIMIT;
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    *out = nullptr;
    DeviceCtx* c;
    int rcode = get_ctx(device, &c);
    if (rcode != KY_OK) return rcode;
    static thread_local DScene packed;
    rcode = pack_scene(scene, &packed);   // (refuses a missing or malformed scene with the statuses kyhip_render gives)
    if (rcode != KY_OK) return rcode;
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
    f->header = frame_header(p, scene_hash(packed), 0);
    if (f->sh.n_pix > 0) {
        const size_t bytes = workspace_bytes_for(f->sh) + blocks_list_bytes(f->sh);   // (the live list of a frame that tracks blocks: behind the flag words)
        HIP_TRY(f->ws.alloc(bytes));
        HIP_TRY(f->tiles.alloc((size_t)f->sh.n_pix * 3 * sizeof(float)));
        HIP_TRY(hipMemsetAsync(f->ws.p, 0, bytes, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    f->pass.ws = f->ws.p;
    *out = f.release();
    return KY_OK;
}

int kyhip_frame_samples(const kyhip_frame* f, int* done, int* total) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (done) *done = samples_done(f);
    if (total) *total = f->params.samples_per_pixel;
    return KY_OK;
}

int kyhip_frame_render(kyhip_frame* f, int min_samples, int* done) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (min_samples < 1) return fail(KY_ERR_INVALID_VALUE, "min_samples %d: a pass renders at least one sample per pixel", min_samples);
    const int c1 = pass_chunk_end(f->plan, f->chunks_done, min_samples);
    if (nothing_live(f)) {   // every block is retired: nothing is launched and the front stays
        if (done) *done = samples_done(f);
        return KY_OK;
    }
    if (f->blocks) f->pass.n_live = f->n_live;
    if (c1 > f->chunks_done && f->sh.n_pix > 0) {
        DeviceCtx* c;
        int rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        f->pass.chunk_first = f->chunks_done;
        f->pass.chunk_count = c1 - f->chunks_done;
        rcode = render_tiles_device(f->device, &f->scene, &f->params, nullptr, nullptr, 0, c->stream, 0, nullptr, &f->pass);
        const int n_now = chunk_end(f->plan, c1 - 1);
        if (rcode == KY_OK && f->track) {   // the batch this pass adds, behind its render kernel
            (void)hipEventRecord(f->ev[0], c->stream);
            rcode = noise_update_device(f->ws.p, f->noise.p, f->sh, f->params.samples_per_pixel, f->n_prev, n_now, f->blocks ? f->bstate.p : nullptr, c->stream);
            (void)hipEventRecord(f->ev[1], c->stream);
        }
        const hipError_t e = hipStreamSynchronize(c->stream);   // blocking, and also after a failed enqueue
        if (rcode != KY_OK) return rcode;
        if (e != hipSuccess) return fail(KY_ERR_DEVICE, "pass failed: %s (the frame's accumulators may hold a part of it)", hipGetErrorString(e));
        if (f->track) { f->batches += 1; f->n_prev = n_now; f->timed[0] = true; }
    } else if (c1 > f->chunks_done && f->track) {   // a shard without pixels: the bookkeeping alone
        f->batches += 1;
        f->n_prev = chunk_end(f->plan, c1 - 1);
    }
    if (f->blocks && c1 > f->chunks_done) f->passes += 1;   // (behind the pass's synchronisation: a failed pass is not counted)
    f->chunks_done = c1;
    if (done) *done = samples_done(f);
    return KY_OK;
}

int kyhip_frame_resolve(kyhip_frame* f, int normalise, float* film_rgb, size_t stride_px) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (normalise != 0 && normalise != 1) return fail(KY_ERR_INVALID_VALUE, "normalise %d: 0 (sum / total) or 1 (sum / done)", normalise);
    const ky_render_params* p = &f->params;
    if (!film_rgb || stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    const int done = samples_done(f);
    if (f->blocks && !normalise)
        for (size_t b = 0; b < f->hblocks.size(); ++b)
            if (f->hinside[b] > 0 && f->hblocks[b].retired_at >= 0 && f->hblocks[b].retired_at < p->samples_per_pixel)
                return fail(KY_ERR_INVALID_VALUE, "normalise 0 on a frame with blocks retired short of its %d samples (block %zu at %d): sum / total would darken them; normalise 1",
                            p->samples_per_pixel, b, f->hblocks[b].retired_at);
    if (f->sh.n_pix == 0 || (normalise && done == 0)) return KY_OK;
    DeviceCtx* c;
    int rcode = get_ctx(f->device, &c);
    if (rcode != KY_OK) return rcode;
    const double scale = normalise ? (double)p->samples_per_pixel / (double)done : 1.0;
    if (f->blocks && normalise) rcode = blocks_resolve_device(f->ws.p, f->bstate.p, f->tiles.as<float>(), f->sh, p->samples_per_pixel, done, c->stream);
    else rcode = resolve_frame_device(f->ws.p, f->tiles.as<float>(), f->sh.n_pix, scale, c->stream);
    if (rcode != KY_OK) return rcode;
    const size_t span = ((size_t)(p->height - 1) * stride_px + (size_t)p->width) * 3 * sizeof(float);
    if (float* alias = film_in_place_alias(film_rgb, span)) {   // a pinned film: film_t::add_color by the GPU, where the film lies
        rcode = kyhip_film_add_tiles_device(f->device, p, f->tiles.as<float>(), alias, stride_px, c->stream);
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (rcode != KY_OK) return rcode;
        if (e != hipSuccess) return fail(KY_ERR_DEVICE, "resolve failed: %s", hipGetErrorString(e));
        return KY_OK;
    }
    // any other film: de-interleaved into a device film, brought home, added by the host (film_t::add_color, 1586-1590)
    const size_t film_floats = (size_t)p->width * p->height * 3;
    if (!f->film.p) HIP_TRY(f->film.alloc(film_floats * sizeof(float)));
    f->stage.resize(film_floats);
    HIP_TRY(hipMemsetAsync(f->film.p, 0, film_floats * sizeof(float), c->stream));
    rcode = kyhip_film_add_tiles_device(f->device, p, f->tiles.as<float>(), f->film.as<float>(), (size_t)p->width, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (rcode != KY_OK) return rcode;
    if (e == hipSuccess) e = hipMemcpy(f->stage.data(), f->film.p, film_floats * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "resolve failed: %s", hipGetErrorString(e));
    host_add_rows(film_rgb, stride_px, f->stage.data(), p->width, 0, p->height);
    return KY_OK;
}

int64_t kyhip_frame_state_bytes(const kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return (int64_t)state_bytes(f);
}

int kyhip_frame_save(kyhip_frame* f, void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const size_t base = frame_state_bytes(&f->params), need = state_bytes(f);
    if (!buf || bytes < need) return fail(KY_ERR_INVALID_VALUE, "frame state: a buffer of %zu bytes, the state has %zu", bytes, need);
    FrameHeader h = f->header;
    h.samples_done = samples_done(f);
    std::memcpy(buf, &h, sizeof h);
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        const int rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        HIP_TRY(hipMemcpy((char*)buf + sizeof h, f->ws.p, base - sizeof h, hipMemcpyDeviceToHost));   // (passes are blocking: nothing of the frame is in flight)
        if (f->track) HIP_TRY(hipMemcpy((char*)buf + base + sizeof(NoiseTrailer), f->noise.p, (size_t)f->sh.n_pix * sizeof(NoisePixel), hipMemcpyDeviceToHost));
    }
    if (f->track) {
        const NoiseTrailer t = {KY_NOISE_MAGIC, f->batches, f->n_prev};
        std::memcpy((char*)buf + base, &t, sizeof t);
    }
    if (f->blocks) {   // (the host's copy is current: every call that changes the device's brings it home)
        const BlockTrailer t = {KY_BLOCKS_MAGIC, f->sh.n_blocks, f->passes};
        std::memcpy((char*)buf + blocks_at(f), &t, sizeof t);
        if (!f->hblocks.empty()) std::memcpy((char*)buf + blocks_at(f) + sizeof t, f->hblocks.data(), f->hblocks.size() * sizeof(BlockState));
    }
    return KY_OK;
}

int kyhip_frame_load(kyhip_frame* f, const void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    int chunks = 0;
    int rcode = frame_state_check(f->header, buf, bytes, &chunks);
    if (rcode != KY_OK) return rcode;
    const size_t base = frame_state_bytes(&f->params);
    NoiseTrailer t = {};
    BlockTrailer bt = {};
    if (f->track) {   // (a frame that does not track accepts a longer buffer and ignores the trailer)
        rcode = noise_trailer_check(buf, bytes, base, f->sh.n_pix, chunk_end(f->plan, chunks - 1), &t);
        if (rcode != KY_OK) return rcode;
    }
    if (f->blocks) {
        rcode = block_trailer_check(buf, bytes, blocks_at(f), f->sh.n_blocks, f->params.samples_per_pixel, chunk_end(f->plan, chunks - 1), f->track ? t.batches : 0, &bt);
        if (rcode != KY_OK) return rcode;
    }
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        HIP_TRY(hipMemcpy(f->ws.p, (const char*)buf + sizeof(FrameHeader), base - sizeof(FrameHeader), hipMemcpyHostToDevice));
        if (f->track) HIP_TRY(hipMemcpy(f->noise.p, (const char*)buf + base + sizeof(NoiseTrailer), (size_t)f->sh.n_pix * sizeof(NoisePixel), hipMemcpyHostToDevice));
    }
    // (the frame is left untouched by every REFUSAL above; a copy that fails half way is a device error, KY_ERR_DEVICE, behind which the frame's accumulators and
    // pairs may disagree with its counts, which are advanced only here, behind both copies: such a frame is to be ended or loaded again)
    if (f->track) { f->batches = t.batches; f->n_prev = t.n_prev; }
    if (f->blocks) f->passes = bt.passes;
    if (f->blocks && f->sh.n_blocks > 0) {
        HIP_TRY(hipMemcpy(f->bstate.p, (const char*)buf + blocks_at(f) + sizeof(BlockTrailer), (size_t)f->sh.n_blocks * sizeof(BlockState), hipMemcpyHostToDevice));
        rcode = blocks_refresh(f);
        if (rcode != KY_OK) return rcode;
    }
    f->chunks_done = chunks;
    f->loaded = true;
    return KY_OK;
}

// ---- the noise estimate (DESIGN.md "Noise") ----
int kyhip_frame_track_noise(kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (f->track) return KY_OK;
    if (f->chunks_done != 0 || f->loaded) return fail(KY_ERR_INVALID_VALUE, "noise is tracked from a frame's first pass: this one has rendered or loaded something");
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        const int rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        const size_t n = (size_t)f->sh.n_pix;
        HIP_TRY(f->noise.alloc(n * sizeof(NoisePixel)));
        HIP_TRY(f->nmap.alloc(n * sizeof(float)));
        HIP_TRY(f->ncls.alloc(n));
        HIP_TRY(f->nsums.alloc(((size_t)noise_blocks(f->sh.n_pix) + 1) * sizeof(NoiseSums)));
        for (hipEvent_t& e : f->ev) if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipMemsetAsync(f->noise.p, 0, n * sizeof(NoisePixel), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    f->track = true;
    return KY_OK;
}

static bool good_threshold(float t) { return t >= 0.f; }   // (false for a NaN)

// the map and the classes (device), and with `sums` the statistics against `threshold`: enqueued and waited for
static int noise_map_and_stats(kyhip_frame* f, float threshold, NoiseSums* sums) {
    DeviceCtx* c;
    int rcode = get_ctx(f->device, &c);
    if (rcode != KY_OK) return rcode;
    (void)hipEventRecord(f->ev[2], c->stream);
    rcode = noise_map_device(f->ws.p, f->noise.p, f->nmap.as<float>(), f->ncls.as<unsigned char>(), f->sh, f->params.width, f->params.height, f->batches, f->n_prev,
                             f->blocks ? f->bstate.p : nullptr, c->stream);
    if (rcode == KY_OK && sums) rcode = noise_stats_device(f->nmap.as<float>(), f->ncls.as<unsigned char>(), f->sh.n_pix, threshold, f->nsums.p, c->stream);
    (void)hipEventRecord(f->ev[3], c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rcode != KY_OK) return rcode;
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "noise map failed: %s", hipGetErrorString(e));
    f->timed[1] = true;
    if (sums) HIP_TRY(hipMemcpy(sums, f->nsums.as<NoiseSums>() + noise_blocks(f->sh.n_pix), sizeof *sums, hipMemcpyDeviceToHost));
    return KY_OK;
}

int kyhip_frame_noise(kyhip_frame* f, float* map, size_t stride_px) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->track) return fail(KY_ERR_INVALID_VALUE, "the frame does not track noise (kyhip_frame_track_noise)");
    if (!map || stride_px < (size_t)f->params.width) return fail(KY_ERR_INVALID_VALUE, "bad map arguments");
    if (f->sh.n_pix == 0) return KY_OK;
    const int rcode = noise_map_and_stats(f, 0.f, nullptr);
    if (rcode != KY_OK) return rcode;
    const size_t n = (size_t)f->sh.n_pix;
    f->hmap.resize(n);
    f->hcls.resize(n);
    HIP_TRY(hipMemcpy(f->hmap.data(), f->nmap.p, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(f->hcls.data(), f->ncls.p, n, hipMemcpyDeviceToHost));
    for (int i = 0; i < f->sh.n_pix; ++i) {
        if (f->hcls[(size_t)i] == KY_NOISE_PADDING) continue;
        int x, y;
        noise_pixel_xy(f->sh, i, x, y);
        map[(size_t)y * stride_px + (size_t)x] = f->hmap[(size_t)i];
    }
    return KY_OK;
}

int kyhip_frame_noise_stats(kyhip_frame* f, float threshold, ky_noise_stats* out) {
    if (!good_threshold(threshold)) return fail(KY_ERR_INVALID_VALUE, "threshold %g: a noise level is >= 0", (double)threshold);
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->track) return fail(KY_ERR_INVALID_VALUE, "the frame does not track noise (kyhip_frame_track_noise)");
    NoiseSums s = {};
    if (f->sh.n_pix > 0) {
        const int rcode = noise_map_and_stats(f, threshold, &s);
        if (rcode != KY_OK) return rcode;
    }
    std::memset(out, 0, sizeof *out);
    out->batches = f->batches;
    out->samples_done = samples_done(f);
    out->pixels = s.pixels; out->flagged = s.flagged; out->above = s.above;
    out->threshold = threshold;
    out->max = s.max;
    out->mean = s.pixels - s.flagged > 0 ? s.sum / (double)(s.pixels - s.flagged) : 0.0;
    return KY_OK;
}

int kyhip_frame_render_until(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int* done, ky_noise_stats* out) {
    if (!good_threshold(threshold)) return fail(KY_ERR_INVALID_VALUE, "threshold %g: a noise level is >= 0", (double)threshold);
    if (!(max_fraction_above >= 0.f && max_fraction_above <= 1.f)) return fail(KY_ERR_INVALID_VALUE, "max_fraction_above %g: a fraction of the pixels, 0 .. 1", (double)max_fraction_above);
    if (min_batches < 2) return fail(KY_ERR_INVALID_VALUE, "min_batches %d: the estimate needs two batches", min_batches);
    if (min_samples_per_pass < 1) return fail(KY_ERR_INVALID_VALUE, "min_samples_per_pass %d: a pass renders at least one sample per pixel", min_samples_per_pass);
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->track) return fail(KY_ERR_INVALID_VALUE, "the frame does not track noise (kyhip_frame_track_noise)");
    for (;;) {
        int rcode = kyhip_frame_render(f, min_samples_per_pass, done);
        if (rcode != KY_OK) return rcode;
        rcode = kyhip_frame_noise_stats(f, threshold, out);
        if (rcode != KY_OK) return rcode;
        const bool clean = out->batches >= min_batches && (double)out->above <= (double)max_fraction_above * (double)(out->pixels - out->flagged);
        // (a block-tracking frame without a live block renders no further: its front and its map stay what they are, and so would this verdict)
        if (clean || samples_done(f) >= f->params.samples_per_pixel || nothing_live(f)) return KY_OK;
    }
}

// ---- blocks that retire between passes (DESIGN.md "Adaptive") ----
int kyhip_frame_track_blocks(kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (f->blocks) return KY_OK;
    if (f->chunks_done != 0 || f->loaded) return fail(KY_ERR_INVALID_VALUE, "blocks are tracked from a frame's first pass: this one has rendered or loaded something");
    const int nb = f->sh.n_blocks;
    f->hblocks.assign((size_t)nb, BlockState{-1, 0});
    f->hinside.assign((size_t)nb, 0);
    for (int i = 0; i < f->sh.n_pix; ++i)
        if (pixel_inside(f->sh, i, f->params.width, f->params.height)) f->hinside[(size_t)block_of_pixel(f->sh, i)] += 1;
    if (nb > 0) {
        DeviceCtx* c;
        int rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        if (!f->bstate.p) HIP_TRY(f->bstate.alloc((size_t)nb * sizeof(BlockState)));
        if (!f->bscratch.p) HIP_TRY(f->bscratch.alloc(blocks_scratch_bytes(nb)));
        if (!f->bmask.p) HIP_TRY(f->bmask.alloc((size_t)f->params.width * (size_t)f->params.height));
        for (hipEvent_t& e : f->bev) if (!e) HIP_TRY(hipEventCreate(&e));
        rcode = blocks_init_device(f->bstate.p, f->sh, f->params.width, f->params.height, c->stream);
        if (rcode != KY_OK) return rcode;
        rcode = blocks_refresh(f);
        if (rcode != KY_OK) return rcode;
    }
    f->header.magic = KY_FRAME_BLOCKS_MAGIC;
    f->blocks = true;
    return KY_OK;
}

int kyhip_frame_keep(kyhip_frame* f, const unsigned char* mask, size_t row_stride) {
    if (!mask) return fail(KY_ERR_INVALID_VALUE, "mask is NULL");
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->blocks) return fail(KY_ERR_INVALID_VALUE, "the frame does not track blocks (kyhip_frame_track_blocks)");
    const size_t w = (size_t)f->params.width, h = (size_t)f->params.height;
    if (row_stride < w) return fail(KY_ERR_INVALID_VALUE, "row_stride %zu: the mask's rows are %zu bytes", row_stride, w);
    if (f->sh.n_blocks == 0) return KY_OK;
    DeviceCtx* c;
    int rcode = get_ctx(f->device, &c);
    if (rcode != KY_OK) return rcode;
    HIP_TRY(hipMemcpy2D(f->bmask.p, w, mask, row_stride, w, h, hipMemcpyHostToDevice));
    (void)hipEventRecord(f->bev[0], c->stream);
    rcode = blocks_keep_device(f->bstate.p, f->bmask.as<unsigned char>(), f->sh, f->params.width, f->params.height, samples_done(f), f->batches, c->stream);
    (void)hipEventRecord(f->bev[1], c->stream);
    if (rcode != KY_OK) { (void)hipStreamSynchronize(c->stream); return rcode; }
    f->btimed[0] = true;
    return blocks_refresh(f);
}

static int adaptive_args(float threshold, float max_fraction_above, int min_batches) {
    if (!good_threshold(threshold)) return fail(KY_ERR_INVALID_VALUE, "threshold %g: a noise level is >= 0", (double)threshold);
    if (!(max_fraction_above >= 0.f && max_fraction_above <= 1.f)) return fail(KY_ERR_INVALID_VALUE, "max_fraction_above %g: a fraction of the pixels, 0 .. 1", (double)max_fraction_above);
    if (min_batches < 2) return fail(KY_ERR_INVALID_VALUE, "min_batches %d: the estimate needs two batches", min_batches);
    return KY_OK;
}
static int adaptive_frame(const kyhip_frame* f, const ky_block_stats* out) {
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->blocks) return fail(KY_ERR_INVALID_VALUE, "the frame does not track blocks (kyhip_frame_track_blocks)");
    if (!f->track) return fail(KY_ERR_INVALID_VALUE, "the frame does not track noise (kyhip_frame_track_noise)");
    return KY_OK;
}

int kyhip_frame_retire_noisy(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, ky_block_stats* out) {
    int rcode = adaptive_args(threshold, max_fraction_above, min_batches);
    if (rcode == KY_OK) rcode = adaptive_frame(f, out);
    if (rcode != KY_OK) return rcode;
    if (f->n_live > 0) {
        rcode = noise_map_and_stats(f, threshold, nullptr);   // the map at the current state (retired blocks: frozen)
        if (rcode != KY_OK) return rcode;
        DeviceCtx* c;
        rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        (void)hipEventRecord(f->bev[0], c->stream);
        rcode = blocks_retire_device(f->bstate.p, f->nmap.as<float>(), f->ncls.as<unsigned char>(), f->sh, threshold, max_fraction_above, min_batches, samples_done(f),
                                     f->batches, c->stream);
        (void)hipEventRecord(f->bev[1], c->stream);
        if (rcode != KY_OK) { (void)hipStreamSynchronize(c->stream); return rcode; }
        f->btimed[0] = true;
        rcode = blocks_refresh(f);
        if (rcode != KY_OK) return rcode;
    }
    block_stats_of(f, out);
    return KY_OK;
}

int kyhip_frame_render_adaptive(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int* done, ky_block_stats* out) {
    int rcode = adaptive_args(threshold, max_fraction_above, min_batches);
    if (rcode != KY_OK) return rcode;
    if (min_samples_per_pass < 1) return fail(KY_ERR_INVALID_VALUE, "min_samples_per_pass %d: a pass renders at least one sample per pixel", min_samples_per_pass);
    rcode = adaptive_frame(f, out);
    if (rcode != KY_OK) return rcode;
    for (;;) {
        rcode = kyhip_frame_render(f, min_samples_per_pass, done);
        if (rcode != KY_OK) return rcode;
        rcode = kyhip_frame_retire_noisy(f, threshold, max_fraction_above, min_batches, out);
        if (rcode != KY_OK) return rcode;
        if (nothing_live(f) || samples_done(f) >= f->params.samples_per_pixel) return KY_OK;
    }
}

int kyhip_frame_sample_map(kyhip_frame* f, int32_t* map, size_t stride_px) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->blocks) return fail(KY_ERR_INVALID_VALUE, "the frame does not track blocks (kyhip_frame_track_blocks)");
    if (!map || stride_px < (size_t)f->params.width) return fail(KY_ERR_INVALID_VALUE, "bad map arguments");
    const int front = samples_done(f);
    for (int i = 0; i < f->sh.n_pix; ++i) {
        int x, y;
        if (!pixel_inside(f->sh, i, f->params.width, f->params.height, &x, &y)) continue;
        map[(size_t)y * stride_px + (size_t)x] = block_samples(f->hblocks[(size_t)block_of_pixel(f->sh, i)], front);
    }
    return KY_OK;
}

int kyhip_frame_block_stats(kyhip_frame* f, ky_block_stats* out) {
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->blocks) return fail(KY_ERR_INVALID_VALUE, "the frame does not track blocks (kyhip_frame_track_blocks)");
    block_stats_of(f, out);
    return KY_OK;
}

int kyhip_frame_blocks_ms(const kyhip_frame* f, float* retire_ms, float* list_ms) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->blocks) return fail(KY_ERR_INVALID_VALUE, "the frame does not track blocks (kyhip_frame_track_blocks)");
    float ms[2] = {-1.f, -1.f};
    for (int k = 0; k < 2; ++k)
        if (f->btimed[k] && hipEventElapsedTime(&ms[k], f->bev[2 * k], f->bev[2 * k + 1]) != hipSuccess) ms[k] = -1.f;
    if (retire_ms) *retire_ms = ms[0];
    if (list_ms) *list_ms = ms[1];
    return KY_OK;
}

int kyhip_frame_noise_ms(const kyhip_frame* f, float* update_ms, float* stats_ms) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->track) return fail(KY_ERR_INVALID_VALUE, "the frame does not track noise (kyhip_frame_track_noise)");
    float ms[2] = {-1.f, -1.f};
    for (int k = 0; k < 2; ++k)
        if (f->timed[k] && hipEventElapsedTime(&ms[k], f->ev[2 * k], f->ev[2 * k + 1]) != hipSuccess) ms[k] = -1.f;
    if (update_ms) *update_ms = ms[0];
    if (stats_ms) *stats_ms = ms[1];
    return KY_OK;
}

void kyhip_frame_end(kyhip_frame* f) {
    if (!f) return;
    DeviceCtx* c;
    if (get_ctx(f->device, &c) == KY_OK) (void)hipStreamSynchronize(c->stream);   // (the device is current for the buffers' release)
    delete f;
}

}  // extern "C"
