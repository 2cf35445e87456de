/*
 * ky_frame.cpp -- the device work of a frame rendered in passes: kyhip_frame_* (include/kyhip.h; DESIGN.md "Passes").  The reference's render() (ky.cpp:3689-3729)
 * reports its progress per row (3703) and has the picture only at the end; here a frame keeps its own accumulator block on the device, each pass adds whole chunks
 * of every pixel's samples to it (render_tiles_device with a FramePass, ky_launch.hip), and the picture so far can be resolved, saved and loaded between passes.
 * A kyhip_frame is a FrameBook (ky_frame_book.hpp) plus device buffers, event spans and staging vectors, and every entry reads: ask the book, do the HIP work,
 * wait, commit to the book.  Which chunks a pass takes, what the frame holds afterwards, what a load or a merge accepts, which of the frame's two sample counts
 * (its front, what it holds) a kernel is given: all of that is the book's, host code that runs without a GPU (ky_frame_book.cpp, with what a checkpoint is,
 * ky_checkpoint.hpp); the stop rule's argument checks are ky_host.hpp's.  HIP runtime calls only: no kernel is defined here.  The noise estimate's kernels are
 * ky_noise.hip's (DESIGN.md "Noise"), the block kernels ky_blocks.hip's ("Adaptive"), the denoiser's ky_denoise.hip's ("Denoise"), the merge kernel ky_merge.hip's
 * ("Slices").
 */
#include <cstring>
#include <string>
#include <vector>

#include "ky_ctx.hpp"
#include "ky_denoise.hpp"
#include "ky_frame_book.hpp"

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
    void begin(hipStream_t s) { valid = false; (void)hipEventRecord(ev[0], s); }
    void end(hipStream_t s) { (void)hipEventRecord(ev[1], s); }
    float ms() const { float v; return valid && hipEventElapsedTime(&v, ev[0], ev[1]) == hipSuccess ? v : -1.f; }
};
// the device side of the noise estimate of a frame that tracks it (the book's noise.on)
struct NoiseTrack {
    DevBuf state, map, cls, sums;      // n_pix NoisePixel; the map (compact tile order) and the pixels' classes; the statistics' partials and their result
    std::vector<float> hmap;           // host copies of the map and the classes
    std::vector<unsigned char> hcls;
    TimedSpan update, stats;           // the last update kernel; the last map + statistics (kyhip_frame_noise_ms)
};
// ... of the blocks of a frame that retires them (the book's blocks.on): every pass is a listed one (FramePass::n_live), the live list lies in `ws` behind the flag words
struct BlockTrack {
    DevBuf state, scratch, mask;       // n_blocks BlockState; the compaction's counts and n_live; kyhip_frame_keep's mask
    TimedSpan rule, list;              // the last retire / keep kernel; the last compaction (kyhip_frame_blocks_ms)
};
// what kyhip_frame_denoise keeps between calls (no part of a checkpoint): the guides, traced once per frame, and the filter's film-order buffers
struct DenoiseTrack {
    bool guides_done = false;
    int guide_bounces = 0;             // kyhip_frame_set_guide_bounces: fixed once the guides are traced
    DevBuf ga, gb_traced, gb, cv[2];   // width x height Px4 each: {n, t}; {P, class} as traced and as the frame's state classes it now; the levels' ping-pong
    DevBuf key;                        // width x height uint64_t, the chain keys of a frame with guide bounces (none at 0 bounces: every key is 0)
    std::vector<float> hga, hgb;       // host copies of the guides (kyhip_frame_guides)
    std::vector<uint64_t> hkey;        // ... and of the keys (kyhip_frame_guide_chains)
    TimedSpan guides, filter;          // the guide trace; the last call's gather, levels and add (kyhip_frame_denoise_ms)
    int albedo_grid = 0;               // kyhip_frame_set_albedo_grid: 0 is off; fixed once the guides are traced
    DevBuf albedo;                     // width x height Px4 {r, g, b, count} of a frame with an albedo grid, traced when the guides are
    std::vector<float> halbedo;        // ... and its host copy (kyhip_frame_albedo)
    TimedSpan albedo_span;             // the albedo trace (kyhip_frame_albedo_ms)
};
struct kyhip_frame {
    int device = 0;
    FrameBook book;               // everything the frame is apart from what follows
    // the caller's scene, copied: `scene` points into these
    std::vector<ky_shape> shapes;
    std::vector<ky_material> materials;
    std::vector<ky_light> lights;
    std::vector<ky_surface> surfaces;
    ky_scene scene{};
    FramePass pass;               // the frame's accumulator block and the kernel its first pass took
    DevBuf ws, tiles, film;       // accumulators + flag words; resolve's compact tile buffer; the device film of a delivery into a pageable host film
    std::vector<float> stage;     // ... and its host copy
    NoiseTrack noise;
    BlockTrack blocks;
    DenoiseTrack denoise;
    DevBuf filter_table;          // the inverse-CDF table of the frame's pixel filter (kyhip_frame_set_filter), which pass.filter points to
    DevBuf tex_set, tex_texels;   // the frame's texture set (kyhip_frame_set_textures): the DTexSet block and the float4 texels pass.tex points to
    DevBuf merge_ws, merge_state; // what a merge from a saved state or from another device reads: the other frame's accumulator block and noise pairs
    TimedSpan merge;              // the last merge kernel (kyhip_frame_merge_ms)
};

// What frames of one scene under a moving camera hand to each other (kyhip_history_*; DESIGN.md "Denoise", "Temporal"): no part of a frame and of no checkpoint.
// Film order, double-buffered: a temporal call reads side `side`, writes the other and swaps behind its wait.
struct kyhip_history {
    int device = 0, width = 0, height = 0;
    int frames = 0;                    // temporal calls since create / reset; 0: the history holds no picture
    int side = 0;
    int albedo = -1;                   // whether its colours are albedo-demodulated (0 / 1); -1 while it holds no picture
    ky_camera camera{};                // of the frame that wrote side `side`
    DevBuf cv[2], ga[2], gb[2];        // width x height Px4 each: {r, g, b, v} accumulated; {n, t}; {P, m} (the accumulated sample count in the class slot)
    std::vector<float> hcv, hgb;       // host copies (kyhip_history_read)
    TimedSpan span;                    // the last temporal kernel (kyhip_history_ms)
};

static const void* block_state_or_null(const kyhip_frame* f) { return f->book.blocks.on ? f->blocks.state.p : nullptr; }

// Waits for what was enqueued on `stream`, also after a failed enqueue, whose status `rcode` comes first; then the device's, as "<what> failed: <error><tail>"
static int finish(hipStream_t stream, int rcode, const char* what, const char* tail = "") {
    const hipError_t e = hipStreamSynchronize(stream);
    if (rcode != KY_OK) return rcode;
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "%s failed: %s%s", what, hipGetErrorString(e), tail);
    return KY_OK;
}
// The timed span around an enqueue: `enqueue` (-> a KY_* status) between the span's events, then the wait.  A span is valid only once what it brackets was
// enqueued whole and waited for.
template <class Enqueue>
static int timed(TimedSpan& span, hipStream_t stream, const char* what, const char* tail, Enqueue enqueue) {
    span.begin(stream);
    const int rcode = enqueue();
    span.end(stream);
    KY_TRY(finish(stream, rcode, what, tail));
    span.valid = true;
    return KY_OK;
}

// The delivery of a finished device picture into the caller's film (film_t::add_color, 1586-1590).  add(dst, dst_stride_px) enqueues the add of the picture to a
// device film.  A pinned film is added to where it lies; for any other the picture is added into the frame's zeroed device film, brought home and added by the
// host.  rcode: the status of what the caller enqueued before (a failed enqueue is still waited for before its status returns); `span`, when given, ends behind the
// add and becomes valid only after the wait.
template <class Add>
static int deliver(kyhip_frame* f, hipStream_t stream, int rcode, const char* what, TimedSpan* span, float* film_rgb, size_t stride_px, Add add) {
    const ky_render_params* p = &f->book.params;
    const size_t span_bytes = ((size_t)(p->height - 1) * stride_px + (size_t)p->width) * 3 * sizeof(float);
    const size_t film_floats = (size_t)p->width * p->height * 3;
    float* dst = film_in_place_alias(film_rgb, span_bytes);
    size_t dst_stride = stride_px;
    const bool in_place = dst != nullptr;
    if (!in_place) {
        hipError_t e = hipSuccess;
        if (rcode == KY_OK && !f->film.p) e = f->film.alloc(film_floats * sizeof(float));
        if (rcode == KY_OK && e == hipSuccess) {
            f->stage.resize(film_floats);
            e = hipMemsetAsync(f->film.p, 0, film_floats * sizeof(float), stream);
        }
        if (e != hipSuccess) rcode = fail(KY_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e));
        dst = f->film.as<float>();
        dst_stride = (size_t)p->width;
    }
    if (rcode == KY_OK) rcode = add(dst, dst_stride);
    if (span) span->end(stream);
    KY_TRY(finish(stream, rcode, what));
    if (span) span->valid = true;
    if (in_place) return KY_OK;
    const hipError_t e = hipMemcpy(f->stage.data(), f->film.p, film_floats * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(KY_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e));
    host_add_rows(film_rgb, stride_px, f->stage.data(), p->width, 0, p->height);
    return KY_OK;
}

// The live list (into the frame's accumulator block, behind the flag words) and its length from the device's block state, which comes home too: enqueued and
// waited for.  Behind every call that changes the state.
static int blocks_refresh(kyhip_frame* f) {
    BlockTrack& b = f->blocks;
    FrameBook& book = f->book;
    if (book.sh.n_blocks <= 0) return book.blocks_home(0);
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    int* list = (int*)((char*)f->ws.p + blocks_list_offset(book.sh));
    KY_TRY(timed(b.list, c->stream, "block list", "", [&] { return blocks_compact_device(b.state.p, book.sh.n_blocks, list, b.scratch.p, c->stream); }));
    int n_live = -1;
    HIP_TRY(hipMemcpy(&n_live, b.scratch.as<int>() + blocks_groups(book.sh.n_blocks), sizeof n_live, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(book.blocks.host.data(), b.state.p, book.blocks.host.size() * sizeof(BlockState), hipMemcpyDeviceToHost));
    return book.blocks_home(n_live);
}

// what the entries of a frame that tracks something refuse first: KY_OK, or KY_ERR_INVALID_VALUE with the message
static int frame_tracks(const kyhip_frame* f, bool blocks, bool noise) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return f->book.tracks(blocks, noise);
}

// kyhip_frame_begin and kyhip_frame_begin_slice: the frame that owns samples [first_sample, end_sample)
static int frame_begin(int device, const ky_scene* scene, const ky_render_params* p, int first_sample, int end_sample, kyhip_frame** out) {
    KY_TRY(begin_check(scene, p, first_sample, end_sample, out));
    DeviceCtx* c;
    KY_TRY(get_ctx(device, &c));
    static thread_local DScene packed;
    KY_TRY(pack_scene(scene, &packed));   // (refuses a missing or malformed scene with the statuses kyhip_render gives)
    std::unique_ptr<kyhip_frame> f(new kyhip_frame);
    f->device = device;
    f->scene = *scene;
    f->shapes.assign(scene->shapes, scene->shapes + scene->shape_count);
    f->materials.assign(scene->materials, scene->materials + scene->material_count);
    f->lights.assign(scene->lights, scene->lights + scene->light_count);
    f->surfaces.assign(scene->surfaces, scene->surfaces + scene->surface_count);
    f->scene.shapes = f->shapes.data(); f->scene.materials = f->materials.data(); f->scene.lights = f->lights.data(); f->scene.surfaces = f->surfaces.data();
    f->book.begin(p, scene_hash(packed), first_sample, end_sample);
    const ShardConst& sh = f->book.sh;
    if (sh.n_pix > 0) {
        const size_t bytes = workspace_bytes_for(sh) + blocks_list_bytes(sh);   // (the live list of a frame that tracks blocks: behind the flag words)
        HIP_TRY(f->ws.alloc(bytes));
        HIP_TRY(f->tiles.alloc((size_t)sh.n_pix * 3 * sizeof(float)));
        HIP_TRY(hipMemsetAsync(f->ws.p, 0, bytes, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    f->pass.ws = f->ws.p;
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

// ---- the frame's pixel filter ----
int kyhip_frame_set_filter(kyhip_frame* f, const ky_pixel_filter* filter) {
    KY_TRY(filter_check(filter));   // (the filter first, then the frame: the host-only builds' stand-in refuses in the same order)
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!f->book.untouched()) return f->book.set_filter(filter);   // (the book's refusal)
    FramePass& pass = f->pass;
    if (filter->kind != KY_FILTER_BOX) {   // the table first: a failed copy leaves the frame's filter what it was
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        float table[KYHIP_FILTER_TABLE + 1];
        filter_table(filter, table);
        if (!f->filter_table.p) HIP_TRY(f->filter_table.alloc(sizeof table));
        HIP_TRY(hipMemcpy(f->filter_table.p, table, sizeof table, hipMemcpyHostToDevice));
    }
    KY_TRY(f->book.set_filter(filter));
    pass.filtered = filter->kind != KY_FILTER_BOX;
    pass.filter = FilterConst{filter->kind, filter->radius, filter_grow(filter), pass.filtered ? f->filter_table.as<const float>() : nullptr};
    pass.filter_note = filter_describe(filter);
    return KY_OK;
}
int kyhip_frame_filter(const kyhip_frame* f, ky_pixel_filter* out) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    *out = f->book.filter;
    return KY_OK;
}
// kyhip_render under a pixel filter: a frame of its own, rendered in one pass and resolved -- the accumulators of a frame in any number of passes or slices are the
// same words (DESIGN.md "Passes"), and resolve_frame_kernel at scale 1 is resolve_kernel bit for bit.  A box filter is kyhip_render itself.
int kyhip_render_filtered(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, float* film_rgb, size_t stride_px) {
    if (filter_is_box(filter)) {
        if (filter) KY_TRY(filter_check(filter));
        return kyhip_render(device, scene, p, film_rgb, stride_px);
    }
    KY_TRY(filter_check(filter));
    if (p && valid_params(p) && p->sampler == KY_SAMPLER_DEBUG) return kyhip_render(device, scene, p, film_rgb, stride_px);   // (0.5 is the centre under every filter)
    if (!film_rgb || (p && valid_params(p) && stride_px < (size_t)p->width)) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    kyhip_frame* f = nullptr;
    KY_TRY(kyhip_frame_begin(device, scene, p, &f));
    int rcode = kyhip_frame_set_filter(f, filter);
    if (rcode == KY_OK) rcode = kyhip_frame_render(f, p->samples_per_pixel, nullptr);
    if (rcode == KY_OK) rcode = kyhip_frame_resolve(f, 1, film_rgb, stride_px);
    kyhip_frame_end(f);
    return rcode;
}

// ---- the frame's lens ----
int kyhip_frame_set_lens(kyhip_frame* f, const ky_lens* lens) {
    KY_TRY(lens_check(lens));   // (the lens first, then the frame, as for the filter)
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    LensConst lc{};
    if (!lens_is_pinhole(lens) && f->book.untouched()) KY_TRY(lens_const_checked(&f->scene.camera, lens, &lc));   // (first: a refusal leaves the frame's lens what it was)
    KY_TRY(f->book.set_lens(lens));   // (refused once the frame holds a sample; no device work stands behind a lens)
    FramePass& pass = f->pass;
    pass.lensed = !lens_is_pinhole(lens);
    pass.lens = lc;
    pass.lens_note = lens_describe(lens);
    return KY_OK;
}
int kyhip_frame_lens(const kyhip_frame* f, ky_lens* out) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    *out = f->book.lens;
    return KY_OK;
}
// kyhip_render_filtered under a lens: once more a frame of its own, rendered in one pass and resolved.  The pinhole is kyhip_render_filtered itself.
int kyhip_render_lens(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, const ky_lens* lens, float* film_rgb, size_t stride_px) {
    if (lens) KY_TRY(lens_check(lens));
    if (lens_is_pinhole(lens)) return kyhip_render_filtered(device, scene, p, filter, film_rgb, stride_px);
    if (filter) KY_TRY(filter_check(filter));
    if (p && valid_params(p) && p->sampler == KY_SAMPLER_DEBUG) return kyhip_render(device, scene, p, film_rgb, stride_px);   // ((0.5, 0.5) is the centre of every lens)
    if (!film_rgb || (p && valid_params(p) && stride_px < (size_t)p->width)) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    kyhip_frame* f = nullptr;
    KY_TRY(kyhip_frame_begin(device, scene, p, &f));
    int rcode = filter_is_box(filter) ? (int)KY_OK : kyhip_frame_set_filter(f, filter);
    if (rcode == KY_OK) rcode = kyhip_frame_set_lens(f, lens);
    if (rcode == KY_OK) rcode = kyhip_frame_render(f, p->samples_per_pixel, nullptr);
    if (rcode == KY_OK) rcode = kyhip_frame_resolve(f, 1, film_rgb, stride_px);
    kyhip_frame_end(f);
    return rcode;
}

// ---- the frame's textures ----
int kyhip_frame_set_textures(kyhip_frame* f, const ky_texture* textures, int n) {
    if (!f) {   // (the set first, as far as it can be checked without a scene, then the frame -- as for the filter and the lens)
        if (n < 0 || (n > 0 && !textures)) return fail(KY_ERR_INVALID_VALUE, "bad texture arguments");
        if (n > KYHIP_MAX_TEXTURES) return fail(KY_ERR_LIMIT, "textures: %d, at most %d", n, KYHIP_MAX_TEXTURES);
        return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    }
    KY_TRY(texture_check(&f->scene, textures, n));
    FramePass& pass = f->pass;
    if (!f->book.untouched()) return f->book.set_textures(0);   // (the book's refusal)
    DevBuf new_set, new_texels;   // the upload first, into buffers of its own: a failed allocation or copy leaves the frame's textures what they were
    if (n > 0) {
        static thread_local DScene packed;
        KY_TRY(pack_scene(&f->scene, &packed));
        std::unique_ptr<DTexSet> set(new DTexSet);
        std::vector<float> texels4;
        texture_pack(&f->scene, &packed, textures, n, set.get(), &texels4);
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        HIP_TRY(new_set.alloc(sizeof(DTexSet)));
        HIP_TRY(new_texels.alloc(texels4.size() * sizeof(float)));
        HIP_TRY(hipMemcpy(new_set.p, set.get(), sizeof(DTexSet), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(new_texels.p, texels4.data(), texels4.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    KY_TRY(f->book.set_textures(texture_digest(textures, n)));
    std::swap(f->tex_set.p, new_set.p);         // (what the frame held before -- a set replaced before the first pass -- is released with new_set / new_texels)
    std::swap(f->tex_texels.p, new_texels.p);
    pass.textured = n > 0;
    pass.tex = TexConst{n > 0 ? f->tex_set.as<const DTexSet>() : nullptr, n > 0 ? f->tex_texels.as<const float4>() : nullptr};
    pass.tex_note = n > 0 ? texture_describe(textures, n) : std::string();
    return KY_OK;
}
// kyhip_render_lens under a texture set: a frame of its own again.  No textures: kyhip_render_lens itself.
int kyhip_render_textured(int device, const ky_scene* scene, const ky_texture* textures, int n, const ky_render_params* p, const ky_pixel_filter* filter, const ky_lens* lens,
                          float* film_rgb, size_t stride_px) {
    KY_TRY(texture_check(scene, textures, n));
    if (n == 0) return kyhip_render_lens(device, scene, p, filter, lens, film_rgb, stride_px);
    if (lens) KY_TRY(lens_check(lens));
    if (filter) KY_TRY(filter_check(filter));
    if (p && valid_params(p) && p->sampler == KY_SAMPLER_DEBUG) return fail(KY_ERR_INVALID_VALUE, "a render under a texture set has no row for the debug sampler");
    if (!film_rgb || (p && valid_params(p) && stride_px < (size_t)p->width)) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    kyhip_frame* f = nullptr;
    KY_TRY(kyhip_frame_begin(device, scene, p, &f));
    int rcode = filter_is_box(filter) ? (int)KY_OK : kyhip_frame_set_filter(f, filter);
    if (rcode == KY_OK && !lens_is_pinhole(lens)) rcode = kyhip_frame_set_lens(f, lens);
    if (rcode == KY_OK) rcode = kyhip_frame_set_textures(f, textures, n);
    if (rcode == KY_OK) rcode = kyhip_frame_render(f, p->samples_per_pixel, nullptr);
    if (rcode == KY_OK) rcode = kyhip_frame_resolve(f, 1, film_rgb, stride_px);
    kyhip_frame_end(f);
    return rcode;
}

int kyhip_frame_coverage(const kyhip_frame* f, int* ranges2, int n, int own[2]) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return f->book.coverage(ranges2, n, own);
}

int kyhip_frame_samples(const kyhip_frame* f, int* done, int* total) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (done) *done = f->book.held();
    if (total) *total = f->book.params.samples_per_pixel;
    return KY_OK;
}

int kyhip_frame_render(kyhip_frame* f, int min_samples, int* done) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    FrameBook& book = f->book;
    PassStep step;
    KY_TRY(book.next_pass(min_samples, &step));
    if (step.launch) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        if (book.blocks.on) f->pass.n_live = book.blocks.n_live;
        f->pass.chunk_first = step.chunk_first;
        f->pass.chunk_count = step.chunk_count;
        const char* tail = " (the frame's accumulators may hold a part of it)";
        const int rcode = render_tiles_device(f->device, &f->scene, &book.params, nullptr, nullptr, 0, c->stream, 0, nullptr, &f->pass);
        if (rcode == KY_OK && book.noise.on)   // the batch this pass adds, behind its render kernel
            KY_TRY(timed(f->noise.update, c->stream, "pass", tail, [&] {
                return noise_update_device(f->ws.p, f->noise.state.p, book.sh, book.params.samples_per_pixel, step.n_prev, step.n_now, block_state_or_null(f), c->stream);
            }));
        else
            KY_TRY(finish(c->stream, rcode, "pass", tail));   // (blocking)
    }
    book.commit_pass(step);   // (behind the pass's synchronisation, and alone for a shard without pixels)
    if (done) *done = book.held();
    return KY_OK;
}

int kyhip_frame_resolve(kyhip_frame* f, int normalise, float* film_rgb, size_t stride_px) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const FrameBook& book = f->book;
    ResolveStep step;
    KY_TRY(book.resolve(normalise, film_rgb, stride_px, &step));
    if (step.nothing) return KY_OK;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    const ky_render_params* p = &book.params;
    int rcode;
    if (step.per_block) rcode = blocks_resolve_device(f->ws.p, f->blocks.state.p, f->tiles.as<float>(), book.sh, p->samples_per_pixel, step.held, c->stream);
    else rcode = resolve_frame_device(f->ws.p, f->tiles.as<float>(), book.sh.n_pix, step.scale, c->stream);
    return deliver(f, c->stream, rcode, "resolve", nullptr, film_rgb, stride_px, [&](float* dst, size_t dst_stride) {
        return kyhip_film_add_tiles_device(f->device, p, f->tiles.as<float>(), dst, dst_stride, c->stream);   // de-interleaved: compact tiles -> film order
    });
}

int64_t kyhip_frame_state_bytes(const kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return (int64_t)f->book.layout.total;
}

// (a checkpoint's parts and what a frame loads: ky_checkpoint.hpp; here only the copies of the parts that live on the device, at the layout's offsets)
int kyhip_frame_save(kyhip_frame* f, void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const FrameBook& book = f->book;
    const CheckpointLayout& L = book.layout;
    KY_TRY(book.save_host(buf, bytes));
    if (book.sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        HIP_TRY(hipMemcpy((char*)buf + L.accum, f->ws.p, L.accum_bytes(), hipMemcpyDeviceToHost));   // (passes are blocking: nothing of the frame is in flight)
        if (book.noise.on) HIP_TRY(hipMemcpy((char*)buf + L.noise_pixels, f->noise.state.p, L.noise_pixels_bytes(), hipMemcpyDeviceToHost));
    }
    return KY_OK;
}

int kyhip_frame_load(kyhip_frame* f, const void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    FrameBook& book = f->book;
    const CheckpointLayout& L = book.layout;
    CheckpointCounts n;
    KY_TRY(book.load_check(buf, bytes, &n));
    // (the frame is left untouched by every REFUSAL above; a copy that fails half way is a device error, KY_ERR_DEVICE, behind which the frame's accumulators and
    // pairs may disagree with its counts, which are advanced only at the end, behind every copy: such a frame is to be ended or loaded again)
    if (book.sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        HIP_TRY(hipMemcpy(f->ws.p, (const char*)buf + L.accum, L.accum_bytes(), hipMemcpyHostToDevice));
        if (book.noise.on) HIP_TRY(hipMemcpy(f->noise.state.p, (const char*)buf + L.noise_pixels, L.noise_pixels_bytes(), hipMemcpyHostToDevice));
    }
    if (book.blocks.on && book.sh.n_blocks > 0) {
        HIP_TRY(hipMemcpy(f->blocks.state.p, (const char*)buf + L.block_states, L.block_states_bytes(), hipMemcpyHostToDevice));
        KY_TRY(blocks_refresh(f));
    }
    book.commit_load(n);
    return KY_OK;
}

// ---- the noise estimate (DESIGN.md "Noise") ----
int kyhip_frame_track_noise(kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    NoiseTrack& t = f->noise;
    FrameBook& book = f->book;
    if (book.noise.on) return KY_OK;
    KY_TRY(book.can_track_noise());
    if (book.sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        const size_t n = (size_t)book.sh.n_pix;
        HIP_TRY(t.state.alloc(n * sizeof(NoisePixel)));
        HIP_TRY(t.map.alloc(n * sizeof(float)));
        HIP_TRY(t.cls.alloc(n));
        HIP_TRY(t.sums.alloc(((size_t)noise_blocks(book.sh.n_pix) + 1) * sizeof(NoiseSums)));
        KY_TRY(t.update.create());
        KY_TRY(t.stats.create());
        HIP_TRY(hipMemsetAsync(t.state.p, 0, n * sizeof(NoisePixel), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    book.track_noise();
    return KY_OK;
}

// the map and the classes (device), and with `sums` the statistics against `threshold`: enqueued and waited for
static int noise_map_and_stats(kyhip_frame* f, float threshold, NoiseSums* sums) {
    NoiseTrack& t = f->noise;
    const FrameBook& book = f->book;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    KY_TRY(timed(t.stats, c->stream, "noise map", "", [&] {
        const int rcode = noise_map_device(f->ws.p, t.state.p, t.map.as<float>(), t.cls.as<unsigned char>(), book.sh, book.params.width, book.params.height, book.noise.batches,
                                           book.noise.n_prev, block_state_or_null(f), c->stream);
        if (rcode != KY_OK || !sums) return rcode;
        return noise_stats_device(t.map.as<float>(), t.cls.as<unsigned char>(), book.sh.n_pix, threshold, t.sums.p, c->stream);
    }));
    if (sums) HIP_TRY(hipMemcpy(sums, t.sums.as<NoiseSums>() + noise_blocks(book.sh.n_pix), sizeof *sums, hipMemcpyDeviceToHost));
    return KY_OK;
}

int kyhip_frame_noise(kyhip_frame* f, float* map, size_t stride_px) {
    KY_TRY(frame_tracks(f, false, true));
    const ShardConst& sh = f->book.sh;
    if (!map || stride_px < (size_t)f->book.params.width) return fail(KY_ERR_INVALID_VALUE, "bad map arguments");
    if (sh.n_pix == 0) return KY_OK;
    KY_TRY(noise_map_and_stats(f, 0.f, nullptr));
    NoiseTrack& t = f->noise;
    const size_t n = (size_t)sh.n_pix;
    t.hmap.resize(n);
    t.hcls.resize(n);
    HIP_TRY(hipMemcpy(t.hmap.data(), t.map.p, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t.hcls.data(), t.cls.p, n, hipMemcpyDeviceToHost));
    for (int i = 0; i < sh.n_pix; ++i) {
        if (t.hcls[(size_t)i] == KY_NOISE_PADDING) continue;
        int x, y;
        noise_pixel_xy(sh, i, x, y);
        map[(size_t)y * stride_px + (size_t)x] = t.hmap[(size_t)i];
    }
    return KY_OK;
}

int kyhip_frame_noise_stats(kyhip_frame* f, float threshold, ky_noise_stats* out) {
    KY_TRY(threshold_check(threshold));
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    KY_TRY(frame_tracks(f, false, true));
    NoiseSums s = {};
    if (f->book.sh.n_pix > 0) {
        KY_TRY(noise_map_and_stats(f, threshold, &s));
    }
    std::memset(out, 0, sizeof *out);
    out->batches = f->book.noise.batches;
    out->samples_done = f->book.held();
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
        if (f->book.until_stops(*out, max_fraction_above, min_batches)) return KY_OK;
    }
}

// ---- blocks that retire between passes (DESIGN.md "Adaptive") ----
int kyhip_frame_track_blocks(kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    BlockTrack& b = f->blocks;
    FrameBook& book = f->book;
    if (book.blocks.on) return KY_OK;
    KY_TRY(book.can_track_blocks());
    book.size_blocks();
    const int nb = book.sh.n_blocks;
    if (nb > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        if (!b.state.p) HIP_TRY(b.state.alloc((size_t)nb * sizeof(BlockState)));
        if (!b.scratch.p) HIP_TRY(b.scratch.alloc(blocks_scratch_bytes(nb)));
        if (!b.mask.p) HIP_TRY(b.mask.alloc((size_t)book.params.width * (size_t)book.params.height));
        KY_TRY(b.rule.create());
        KY_TRY(b.list.create());
        KY_TRY(blocks_init_device(b.state.p, book.sh, book.params.width, book.params.height, c->stream));
        KY_TRY(blocks_refresh(f));
    }
    book.track_blocks();
    return KY_OK;
}

int kyhip_frame_keep(kyhip_frame* f, const unsigned char* mask, size_t row_stride) {
    if (!mask) return fail(KY_ERR_INVALID_VALUE, "mask is NULL");
    KY_TRY(frame_tracks(f, true, false));
    const FrameBook& book = f->book;
    const size_t w = (size_t)book.params.width, h = (size_t)book.params.height;
    if (row_stride < w) return fail(KY_ERR_INVALID_VALUE, "row_stride %zu: the mask's rows are %zu bytes", row_stride, w);
    if (book.sh.n_blocks == 0) return KY_OK;
    BlockTrack& b = f->blocks;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    HIP_TRY(hipMemcpy2D(b.mask.p, w, mask, row_stride, w, h, hipMemcpyHostToDevice));
    KY_TRY(timed(b.rule, c->stream, "block rule", "", [&] {
        return blocks_keep_device(b.state.p, b.mask.as<unsigned char>(), book.sh, book.params.width, book.params.height, book.front(), book.noise.batches, c->stream);
    }));
    return blocks_refresh(f);   // the state the kernel changed comes home
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
    const FrameBook& book = f->book;
    if (book.blocks.n_live > 0) {
        KY_TRY(noise_map_and_stats(f, threshold, nullptr));   // the map at the current state (retired blocks: frozen)
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        KY_TRY(timed(b.rule, c->stream, "block rule", "", [&] {
            return blocks_retire_device(b.state.p, f->noise.map.as<float>(), f->noise.cls.as<unsigned char>(), book.sh, threshold, max_fraction_above, min_batches, book.front(),
                                        book.noise.batches, c->stream);
        }));
        KY_TRY(blocks_refresh(f));
    }
    book.block_stats(out);
    return KY_OK;
}

int kyhip_frame_render_adaptive(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int* done, ky_block_stats* out) {
    KY_TRY(stop_rule_check(threshold, max_fraction_above, min_batches));
    KY_TRY(pass_samples_check(min_samples_per_pass));
    KY_TRY(adaptive_frame(f, out));
    for (;;) {
        KY_TRY(kyhip_frame_render(f, min_samples_per_pass, done));
        KY_TRY(kyhip_frame_retire_noisy(f, threshold, max_fraction_above, min_batches, out));
        if (f->book.adaptive_stops()) return KY_OK;
    }
}

int kyhip_frame_sample_map(kyhip_frame* f, int32_t* map, size_t stride_px) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return f->book.sample_map(map, stride_px);
}

int kyhip_frame_block_stats(kyhip_frame* f, ky_block_stats* out) {
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    KY_TRY(frame_tracks(f, true, false));
    f->book.block_stats(out);
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
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return f->book.denoise_check(needs_variance);
}
// the filter's buffers, the guides (traced on the first call) and the gather of the frame's state as it stands: enqueued, the trace also waited for
static int denoise_prepare(kyhip_frame* f, DeviceCtx* c, bool timed_filter) {
    DenoiseTrack& d = f->denoise;
    const FrameBook& book = f->book;
    const ky_render_params* p = &book.params;
    const size_t bytes = (size_t)p->width * (size_t)p->height * sizeof(Px4);
    for (DevBuf* b : {&d.ga, &d.gb_traced, &d.gb, &d.cv[0], &d.cv[1]})
        if (!b->p) HIP_TRY(b->alloc(bytes));
    if (d.guide_bounces > 0 && !d.key.p) HIP_TRY(d.key.alloc((size_t)p->width * (size_t)p->height * sizeof(uint64_t)));
    if (d.albedo_grid > 0 && !d.albedo.p) HIP_TRY(d.albedo.alloc(bytes));
    KY_TRY(d.guides.create());
    KY_TRY(d.filter.create());
    if (d.albedo_grid > 0) KY_TRY(d.albedo_span.create());
    if (!d.guides_done) {
        KY_TRY(timed(d.guides, c->stream, "denoise guides", "", [&] {
            if (d.guide_bounces > 0) return denoise_chain_guides_device(f->device, &f->scene, p->width, p->height, d.guide_bounces, d.ga.p, d.gb_traced.p, d.key.p, c->stream);
            return denoise_guides_device(f->device, &f->scene, p->width, p->height, d.ga.p, d.gb_traced.p, c->stream);
        }));
        if (d.albedo_grid > 0) {   // the albedo with the guides: through the camera form, the textures and the guide bounces the frame holds now
            const FramePass& pass = f->pass;
            LensCam cam;
            static_cast<FilterConst&>(cam) = pass.filter;
            cam.lens = pass.lensed ? pass.lens : LensConst{0.f, 0.f, 0.f, 0.f};
            const TexConst tex = pass.textured ? pass.tex : TexConst{nullptr, nullptr};
            KY_TRY(timed(d.albedo_span, c->stream, "denoise albedo", "", [&] {
                return denoise_albedo_device(f->device, &f->scene, p->width, p->height, d.guide_bounces, d.albedo_grid, cam, tex, d.albedo.p, c->stream);
            }));
        }
        d.guides_done = true;
    }
    if (timed_filter) d.filter.begin(c->stream);   // (kyhip_frame_denoise: its span begins with the gather and ends behind the delivery's add)
    if (d.albedo_grid > 0)
        return denoise_gather_albedo_device(f->ws.p, f->noise.state.p, block_state_or_null(f), book.sh, p->width, p->height, p->samples_per_pixel, book.held(),
                                            book.noise.batches, d.gb_traced.p, d.albedo.p, d.cv[0].p, d.gb.p, c->stream);
    return denoise_gather_device(f->ws.p, f->noise.state.p, block_state_or_null(f), book.sh, p->width, p->height, p->samples_per_pixel, book.held(), book.noise.batches,
                                 d.gb_traced.p, d.cv[0].p, d.gb.p, c->stream);
}

int kyhip_frame_denoise(kyhip_frame* f, const ky_denoise_params* params, float* film_rgb, size_t stride_px) {
    ky_denoise_params q;
    kyhip_denoise_defaults(&q);
    if (params) q = *params;
    KY_TRY(denoise_params_check(&q));
    KY_TRY(denoise_frame_check(f, true));
    const ky_render_params* p = &f->book.params;
    if (!film_rgb || stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    if (q.levels == 0) return kyhip_frame_resolve(f, 1, film_rgb, stride_px);
    if (f->book.sh.n_pix == 0) return KY_OK;
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
    for (int l = 0; l < q.levels && rcode == KY_OK; ++l)
        rcode = d.guide_bounces > 0 ? denoise_level_keyed_device(d.cv[l & 1].p, d.cv[(l + 1) & 1].p, d.ga.p, d.gb.p, d.key.p, 1 << l, k, c->stream)
                                    : denoise_level_device(d.cv[l & 1].p, d.cv[(l + 1) & 1].p, d.ga.p, d.gb.p, 1 << l, k, c->stream);
    const void* result = d.cv[q.levels & 1].p;
    return deliver(f, c->stream, rcode, "denoise", &d.filter, film_rgb, stride_px, [&](float* dst, size_t dst_stride) {
        if (d.albedo_grid > 0) return denoise_add_albedo_device(result, d.gb.p, d.albedo.p, dst, dst_stride, p->width, p->height, c->stream);
        return denoise_add_device(result, dst, dst_stride, p->width, p->height, c->stream);   // film order already
    });
}

// ---- temporal reuse (DESIGN.md "Denoise", "Temporal"; kyhip_temporal_defaults is host code: ky_pack.cpp) ----
// Every refusal comes before any device work; the history is committed (side, camera, mode, count) only behind the wait for a call that was enqueued whole.

int kyhip_history_create(int device, int width, int height, kyhip_history** out) {
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    *out = nullptr;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return fail(KY_ERR_INVALID_VALUE, "a history of %d x %d pixels", width, height);
    DeviceCtx* c;
    KY_TRY(get_ctx(device, &c));
    std::unique_ptr<kyhip_history> h(new kyhip_history);
    h->device = device; h->width = width; h->height = height;
    const size_t bytes = (size_t)width * (size_t)height * sizeof(Px4);
    for (int s = 0; s < 2; ++s)
        for (DevBuf* b : {&h->cv[s], &h->ga[s], &h->gb[s]}) HIP_TRY(b->alloc(bytes));
    KY_TRY(h->span.create());
    *out = h.release();
    return KY_OK;
}

int kyhip_history_destroy(kyhip_history* h) {
    if (!h) return fail(KY_ERR_INVALID_VALUE, "history is NULL");
    DeviceCtx* c;
    if (get_ctx(h->device, &c) == KY_OK) (void)hipStreamSynchronize(c->stream);   // (the device is current for the buffers' release)
    delete h;
    return KY_OK;
}

int kyhip_history_reset(kyhip_history* h) {
    if (!h) return fail(KY_ERR_INVALID_VALUE, "history is NULL");
    h->frames = 0;
    h->albedo = -1;
    return KY_OK;
}

int kyhip_history_frames(const kyhip_history* h) {
    if (!h) return fail(KY_ERR_INVALID_VALUE, "history is NULL");
    return h->frames;
}

int kyhip_history_read(kyhip_history* h, float* colour_variance4, float* count, size_t stride_px) {
    if (!h) return fail(KY_ERR_INVALID_VALUE, "history is NULL");
    if (stride_px < (size_t)h->width) return fail(KY_ERR_INVALID_VALUE, "row_stride_px %zu: the history's rows are %d pixels", stride_px, h->width);
    const size_t n = (size_t)h->width * (size_t)h->height * 4;
    h->hcv.assign(n, 0.f);
    h->hgb.assign(n, 0.f);
    if (h->frames > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(h->device, &c));
        HIP_TRY(hipMemcpy(h->hcv.data(), h->cv[h->side].p, n * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h->hgb.data(), h->gb[h->side].p, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (int y = 0; y < h->height; ++y) {
        if (colour_variance4) std::memcpy(colour_variance4 + (size_t)y * stride_px * 4, h->hcv.data() + (size_t)y * h->width * 4, (size_t)h->width * 4 * sizeof(float));
        if (count)
            for (int x = 0; x < h->width; ++x) count[(size_t)y * stride_px + (size_t)x] = h->hgb[((size_t)y * h->width + (size_t)x) * 4 + 3];
    }
    return KY_OK;
}

int kyhip_history_ms(const kyhip_history* h, float* ms) {
    if (!h) return fail(KY_ERR_INVALID_VALUE, "history is NULL");
    if (ms) *ms = h->span.ms();
    return KY_OK;
}

int kyhip_frame_denoise_temporal(kyhip_frame* f, kyhip_history* h, const ky_denoise_params* params, const ky_temporal_params* temporal, float* film_rgb, size_t stride_px) {
    ky_denoise_params q;
    kyhip_denoise_defaults(&q);
    if (params) q = *params;
    ky_temporal_params t;
    kyhip_temporal_defaults(&t);
    if (temporal) t = *temporal;
    KY_TRY(denoise_params_check(&q));
    KY_TRY(temporal_params_check(&t));
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (!h) return fail(KY_ERR_INVALID_VALUE, "history is NULL");
    DenoiseTrack& d = f->denoise;
    KY_TRY(f->book.temporal_check(f->device, d.albedo_grid, h->device, h->width, h->height, h->frames > 0 ? h->albedo : -1));
    const ky_render_params* p = &f->book.params;
    if (!film_rgb || stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    if (f->book.sh.n_pix == 0) return KY_OK;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    int rcode = denoise_prepare(f, c, true);
    if (rcode != KY_OK) return finish(c->stream, rcode, "denoise");   // (nothing of the filter is enqueued; its span stays invalid)
    TemporalConst tk{};
    tk.width = p->width; tk.height = p->height;
    tk.normal_squarings = t.normal_squarings;
    tk.has_history = h->frames > 0 ? 1 : 0;
    tk.n_p = (double)f->book.held();
    tk.max_history = (double)t.max_history; tk.sigma_plane = (double)t.sigma_plane; tk.min_weight = (double)t.min_weight;
    tk.pix = denoise_pixel_width(f->scene.camera, p->width);
    tk.then = h->camera;
    const int from = h->side, to = h->side ^ 1;
    h->span.begin(c->stream);
    rcode = denoise_temporal_device(d.cv[0].p, d.ga.p, d.gb.p, d.guide_bounces > 0 ? d.key.p : nullptr, h->cv[from].p, h->ga[from].p, h->gb[from].p, h->cv[to].p, h->ga[to].p,
                                    h->gb[to].p, tk, c->stream);
    h->span.end(c->stream);
    LevelConst k{};
    k.width = p->width; k.height = p->height;
    k.normal_squarings = q.normal_squarings;
    k.sigma_l2 = (double)q.sigma_luminance * (double)q.sigma_luminance;
    k.sigma_plane = (double)q.sigma_plane;
    k.pix = tk.pix;
    // the levels read the history's new side first and ping-pong between the frame's own buffers from then on: nothing filtered is fed back into the history
    for (int l = 0; l < q.levels && rcode == KY_OK; ++l) {
        const void* in = l == 0 ? h->cv[to].p : d.cv[l & 1].p;
        rcode = d.guide_bounces > 0 ? denoise_level_keyed_device(in, d.cv[(l + 1) & 1].p, d.ga.p, d.gb.p, d.key.p, 1 << l, k, c->stream)
                                    : denoise_level_device(in, d.cv[(l + 1) & 1].p, d.ga.p, d.gb.p, 1 << l, k, c->stream);
    }
    const void* result = q.levels == 0 ? h->cv[to].p : d.cv[q.levels & 1].p;
    const bool enqueued = rcode == KY_OK;
    rcode = deliver(f, c->stream, rcode, "denoise", &d.filter, film_rgb, stride_px, [&](float* dst, size_t dst_stride) {
        if (d.albedo_grid > 0) return denoise_add_albedo_device(result, d.gb.p, d.albedo.p, dst, dst_stride, p->width, p->height, c->stream);
        return denoise_add_device(result, dst, dst_stride, p->width, p->height, c->stream);
    });
    if (!enqueued || rcode != KY_OK) {   // the history keeps its old side: a failed call is not counted
        h->span.valid = false;
        return rcode;
    }
    h->span.valid = true;
    h->side = to;
    h->camera = f->scene.camera;
    h->albedo = d.albedo_grid > 0 ? 1 : 0;
    ++h->frames;
    return KY_OK;
}

int kyhip_frame_guides(kyhip_frame* f, float* normal_t4, float* position_class4, size_t stride_px) {
    KY_TRY(denoise_frame_check(f, false));
    const ky_render_params* p = &f->book.params;
    if (stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "row_stride_px %zu: the guides' rows are %d pixels", stride_px, p->width);
    if (f->book.sh.n_pix == 0) return KY_OK;
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

int kyhip_frame_set_guide_bounces(kyhip_frame* f, int bounces) {
    if (bounces < 0 || bounces > KYHIP_GUIDE_MAX_BOUNCES) return fail(KY_ERR_INVALID_VALUE, "guide bounces %d: 0 .. %d", bounces, KYHIP_GUIDE_MAX_BOUNCES);
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    DenoiseTrack& d = f->denoise;
    if (bounces == d.guide_bounces) return KY_OK;
    if (d.guides_done) return fail(KY_ERR_INVALID_VALUE, "guide bounces %d: the frame's guides are traced, with %d", bounces, d.guide_bounces);
    d.guide_bounces = bounces;
    return KY_OK;
}

int kyhip_frame_guide_bounces(const kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return f->denoise.guide_bounces;
}

int kyhip_frame_guide_chains(kyhip_frame* f, uint64_t* keys, size_t stride_px) {
    KY_TRY(denoise_frame_check(f, false));
    const ky_render_params* p = &f->book.params;
    if (!keys) return fail(KY_ERR_INVALID_VALUE, "keys is NULL");
    if (stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "row_stride_px %zu: the keys' rows are %d pixels", stride_px, p->width);
    if (f->book.sh.n_pix == 0) return KY_OK;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    DenoiseTrack& d = f->denoise;
    const int rcode = denoise_prepare(f, c, false);
    KY_TRY(finish(c->stream, rcode, "denoise guides"));
    const size_t n = (size_t)p->width * (size_t)p->height;
    d.hkey.assign(n, 0);
    if (d.guide_bounces > 0) HIP_TRY(hipMemcpy(d.hkey.data(), d.key.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int y = 0; y < p->height; ++y) std::memcpy(keys + (size_t)y * stride_px, d.hkey.data() + (size_t)y * p->width, (size_t)p->width * sizeof(uint64_t));
    return KY_OK;
}

// ---- the albedo of a frame that demodulates (DESIGN.md "Denoise", "Albedo") ----
int kyhip_frame_set_albedo_grid(kyhip_frame* f, int grid) {
    if (grid < 0 || grid > KY_DN_ALBEDO_MAX_GRID) return fail(KY_ERR_INVALID_VALUE, "albedo grid %d: 0 .. %d", grid, KY_DN_ALBEDO_MAX_GRID);
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    DenoiseTrack& d = f->denoise;
    if (grid == d.albedo_grid) return KY_OK;
    if (d.guides_done) return fail(KY_ERR_INVALID_VALUE, "albedo grid %d: the frame's guides are traced, with %d", grid, d.albedo_grid);
    d.albedo_grid = grid;
    return KY_OK;
}

int kyhip_frame_albedo_grid(const kyhip_frame* f) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    return f->denoise.albedo_grid;
}

int kyhip_frame_albedo(kyhip_frame* f, float* albedo4, size_t stride_px) {
    KY_TRY(denoise_frame_check(f, false));
    const ky_render_params* p = &f->book.params;
    if (!albedo4) return fail(KY_ERR_INVALID_VALUE, "albedo4 is NULL");
    if (stride_px < (size_t)p->width) return fail(KY_ERR_INVALID_VALUE, "row_stride_px %zu: the albedo's rows are %d pixels", stride_px, p->width);
    DenoiseTrack& d = f->denoise;
    if (d.albedo_grid == 0) return fail(KY_ERR_INVALID_VALUE, "the frame has no albedo: its albedo grid is 0");
    if (f->book.sh.n_pix == 0) return KY_OK;
    DeviceCtx* c;
    KY_TRY(get_ctx(f->device, &c));
    const int rcode = denoise_prepare(f, c, false);
    KY_TRY(finish(c->stream, rcode, "denoise albedo"));
    const size_t n = (size_t)p->width * (size_t)p->height * 4;
    d.halbedo.resize(n);
    HIP_TRY(hipMemcpy(d.halbedo.data(), d.albedo.p, n * sizeof(float), hipMemcpyDeviceToHost));
    for (int y = 0; y < p->height; ++y) std::memcpy(albedo4 + (size_t)y * stride_px * 4, d.halbedo.data() + (size_t)y * p->width * 4, (size_t)p->width * 4 * sizeof(float));
    return KY_OK;
}

int kyhip_frame_albedo_ms(const kyhip_frame* f, float* ms) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    if (ms) *ms = f->denoise.albedo_span.ms();
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
// The kernel and, behind it, the book's commit: src_ws / src_state are device memory of f's device (src_state is read where f tracks noise), `step` the book's
// answer to the merge.  Blocking; a failed merge is not counted.
static int merge_apply(kyhip_frame* f, const void* src_ws, const void* src_state, const MergeStep& step) {
    FrameBook& book = f->book;
    if (book.sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        KY_TRY(timed(f->merge, c->stream, "merge", " (the frame's accumulators may hold a part of it)", [&] {
            return merge_device(f->ws.p, src_ws, book.noise.on ? f->noise.state.p : nullptr, src_state, book.sh.n_pix, book.params.samples_per_pixel, step.n_mine, step.n_src, c->stream);
        }));
    }
    book.commit_merge(step);
    return KY_OK;
}
// the buffers a merge stages the other frame's parts in, allocated on the first merge that needs them (the device is current)
static int merge_staging(kyhip_frame* f) {
    if (!f->merge_ws.p) HIP_TRY(f->merge_ws.alloc(workspace_bytes_for(f->book.sh)));
    if (f->book.noise.on && !f->merge_state.p) HIP_TRY(f->merge_state.alloc((size_t)f->book.sh.n_pix * sizeof(NoisePixel)));
    return KY_OK;
}
extern "C" {

int kyhip_frame_merge(kyhip_frame* f, const void* state, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const FrameBook& book = f->book;
    MergeStep step;
    KY_TRY(book.merge_state(state, bytes, &step));
    if (book.sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        KY_TRY(f->merge.create());
        KY_TRY(merge_staging(f));
        HIP_TRY(hipMemcpy(f->merge_ws.p, (const char*)state + step.accum, workspace_bytes_for(book.sh), hipMemcpyHostToDevice));
        if (book.noise.on) HIP_TRY(hipMemcpy(f->merge_state.p, (const char*)state + step.noise_pixels, (size_t)book.sh.n_pix * sizeof(NoisePixel), hipMemcpyHostToDevice));
    }
    return merge_apply(f, f->merge_ws.p, f->merge_state.p, step);
}

int kyhip_frame_merge_from(kyhip_frame* f, kyhip_frame* src) {
    if (!f || !src) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const FrameBook& book = f->book;
    MergeStep step;
    KY_TRY(book.merge_book(src->book, &step));
    const void* src_ws = src->ws.p;
    const void* src_state = src->noise.state.p;
    if (book.sh.n_pix > 0) {
        DeviceCtx* c;
        KY_TRY(get_ctx(f->device, &c));
        KY_TRY(f->merge.create());
        if (src->device != f->device) {   // (the other frame's calls are blocking: nothing of it is in flight on its device)
            KY_TRY(merge_staging(f));
            HIP_TRY(hipMemcpyPeerAsync(f->merge_ws.p, f->device, src->ws.p, src->device, workspace_bytes_for(book.sh), c->stream));
            if (book.noise.on) HIP_TRY(hipMemcpyPeerAsync(f->merge_state.p, f->device, src->noise.state.p, src->device, (size_t)book.sh.n_pix * sizeof(NoisePixel), c->stream));
            src_ws = f->merge_ws.p; src_state = f->merge_state.p;
        }
    }
    return merge_apply(f, src_ws, src_state, step);
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
