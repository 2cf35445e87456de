/*
 * ky_frame.cpp -- a frame rendered in passes: kyhip_frame_* (include/kyhip.h; DESIGN.md "Passes").  The reference's render() (ky.cpp:3689-3729) reports
 * its progress per row (3703) and has the picture only at the end; here a frame keeps its own accumulator block on the device, each pass adds whole chunks
 * of every pixel's samples to it (render_tiles_device with a FramePass, ky_launch.hip), and the picture so far can be resolved, saved and loaded between
 * passes.  Which chunks a pass renders and what a checkpoint must agree in is host arithmetic (ky_shard.hpp, ky_pack.cpp); HIP runtime calls only: no
 * kernel is defined here.
 */
#include <cstring>
#include <string>
#include <vector>

#include "ky_ctx.hpp"

using namespace kyh;

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
};

static int samples_done(const kyhip_frame* f) { return chunk_end(f->plan, f->chunks_done - 1); }

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
        const size_t bytes = workspace_bytes_for(f->sh);
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
    if (c1 > f->chunks_done && f->sh.n_pix > 0) {
        DeviceCtx* c;
        int rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        f->pass.chunk_first = f->chunks_done;
        f->pass.chunk_count = c1 - f->chunks_done;
        rcode = render_tiles_device(f->device, &f->scene, &f->params, nullptr, nullptr, 0, c->stream, 0, nullptr, &f->pass);
        const hipError_t e = hipStreamSynchronize(c->stream);   // blocking, and also after a failed enqueue
        if (rcode != KY_OK) return rcode;
        if (e != hipSuccess) return fail(KY_ERR_DEVICE, "pass failed: %s (the frame's accumulators may hold a part of it)", hipGetErrorString(e));
    }
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
    if (f->sh.n_pix == 0 || (normalise && done == 0)) return KY_OK;
    DeviceCtx* c;
    int rcode = get_ctx(f->device, &c);
    if (rcode != KY_OK) return rcode;
    const double scale = normalise ? (double)p->samples_per_pixel / (double)done : 1.0;
    rcode = resolve_frame_device(f->ws.p, f->tiles.as<float>(), f->sh.n_pix, scale, c->stream);
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
    return (int64_t)frame_state_bytes(&f->params);
}

int kyhip_frame_save(kyhip_frame* f, void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    const size_t need = frame_state_bytes(&f->params);
    if (!buf || bytes < need) return fail(KY_ERR_INVALID_VALUE, "frame state: a buffer of %zu bytes, the state has %zu", bytes, need);
    FrameHeader h = f->header;
    h.samples_done = samples_done(f);
    std::memcpy(buf, &h, sizeof h);
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        const int rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        HIP_TRY(hipMemcpy((char*)buf + sizeof h, f->ws.p, need - sizeof h, hipMemcpyDeviceToHost));   // (passes are blocking: nothing of the frame is in flight)
    }
    return KY_OK;
}

int kyhip_frame_load(kyhip_frame* f, const void* buf, size_t bytes) {
    if (!f) return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
    int chunks = 0;
    int rcode = frame_state_check(f->header, buf, bytes, &chunks);
    if (rcode != KY_OK) return rcode;
    if (f->sh.n_pix > 0) {
        DeviceCtx* c;
        rcode = get_ctx(f->device, &c);
        if (rcode != KY_OK) return rcode;
        HIP_TRY(hipMemcpy(f->ws.p, (const char*)buf + sizeof(FrameHeader), frame_state_bytes(&f->params) - sizeof(FrameHeader), hipMemcpyHostToDevice));
    }
    f->chunks_done = chunks;
    return KY_OK;
}

void kyhip_frame_end(kyhip_frame* f) {
    if (!f) return;
    DeviceCtx* c;
    if (get_ctx(f->device, &c) == KY_OK) (void)hipStreamSynchronize(c->stream);   // (the device is current for the buffers' release)
    delete f;
}

}  // extern "C"
