/*
 * ky_denoise.hip -- the kernels of a frame's denoised picture (ky_denoise.hpp; DESIGN.md "Denoise"), film-sized and apart from the render kernels, which they read
 * a frame between the passes of like noise_map_kernel and blocks_retire_kernel do:
 *   denoise_guides_kernel   once per frame, one thread per film pixel: the camera ray through the pixel centre (generate_ray) and its nearest hit WITHOUT the box
 *                           traversal (trace_nearest; the slab test moves t by a few ulp, and the guides do not depend on kyhip_set_boxes) -> {n, t}, {P, class}; the
 *                           scene's tables staged in LDS as the KAT kernels stage them (the product's device functions, ky_device.hpp, called directly);
 *   denoise_chain_guides_kernel   the same for a frame with guide bounces (kyhip_frame_set_guide_bounces): the ray followed through mirrors and glass, every sampler
 *                           number 0.5, to the first vertex that is neither -> its {n, t summed}, {P, class} and the chain's key, one uint64_t per pixel;
 *   denoise_gather_kernel   one thread per pixel of the compact tile buffer: film_add_kernel's de-interleave (noise_pixel_xy) -> {r, g, b, v} in film order and
 *                           the pixel's class as the frame's state gives it (flagged: 3; a block at 0 samples: 1); a ragged tile's padding writes nothing;
 *   denoise_level_kernel    one thread per film pixel, 256-thread workgroups: level_pixel (ky_denoise.hpp) from one film-order buffer into the other; every tap is
 *                           three 16-byte loads from global memory;
 *   denoise_level_keyed_kernel   ... with the taps that share the pixel's chain key only (level_pixel_t<true>): 8 more bytes per tap;
 *   denoise_add_kernel     clamp01 per channel, then film_t::add_color into a device film or a pinned host film;
 *   denoise_albedo_kernel   once per frame with an albedo grid (kyhip_frame_set_albedo_grid), one thread per film pixel: grid x grid camera rays per pixel through
 *                           the frame's camera form, each walked like the chain guides' ray -> the mean colour of what they end on, {r, g, b, count};
 *   denoise_gather_albedo_kernel / denoise_add_albedo_kernel   the gather and the add of such a frame: a class-0 pixel is divided by its albedo before the
 *                           levels and multiplied by it behind them (demodulate_pixel / remodulate_pixel, ky_denoise.hpp); the level kernels are the same;
 *   denoise_temporal_kernel one thread per film pixel between the gather and the first level of kyhip_frame_denoise_temporal: temporal_pixel_t (ky_denoise.hpp) from the
 *                           frame's buffers and a history's old side into its new side; at most four taps of three 16-byte loads.
 * No floating-point atomics and no order that depends on scheduling: two calls return identical bytes.  gfx950 only.
 */
#include <hip/hip_runtime.h>

#include "ky_device.hpp"

#include "ky_blocks.hpp"
#include "ky_ctx.hpp"
#include "ky_denoise.hpp"

using namespace kyd;
using namespace kyh;
using namespace kydn;
using kyb::BlockState;
using kyn::NoisePixel;

static_assert(sizeof(Px4) == 16 && alignof(Px4) == 16, "a pixel of the filter's buffers is one 16-byte load");

__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_guides_kernel(const DScene* __restrict__ S_, int width, int height, Px4* __restrict__ ga, Px4* __restrict__ gb) {
    const SceneRef S{S_, true, 0, true};
    const LdsScene Lds = stage_scene<true>(S);   // the scene-sized dynamic block, as the KAT kernels take it; ends with a barrier
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= width * height) return;
    const int x = i % width, y = i / width;
    f3 o, d;
    generate_ray(S, (float)x + 0.5f, (float)y + 0.5f, o, d);
    float t = K_INF;
    const int hs = trace_nearest(S, o, d, t);
    Px4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, (float)KY_DN_MISS};
    if (hs >= 0) {
        const f3 p = o + t * d;
        const f3 n = hit_normal(Lds.hit[hs], p, d);
        a = Px4{n.x, n.y, n.z, t};
        b = Px4{p.x, p.y, p.z, Lds.hit[hs].area_light >= 0 ? (float)KY_DN_LIGHT : (float)KY_DN_SURFACE};
    }
    ga[i] = a;
    gb[i] = b;
}

// The guides of a frame with guide bounces (DESIGN.md "Denoise", "Guides beyond the first hit"): the camera ray through the pixel centre followed through mirrors
// and glass as the debug sampler walks it -- every number 0.5, so glass takes its likelier branch (bsdf_sample_delta) -- to the first vertex that is neither, a
// lamp, or nothing.  Every vertex is the one the render kernels build at that hit (path_intersect / path_shade: position, hit_normal, the material's lobe, the
// offset origin of the next ray).  At most bounces + 1 traversals per lane (bounces <= KYHIP_GUIDE_MAX_BOUNCES): the loop's last turn has k == bounces and leaves.
__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_chain_guides_kernel(const DScene* __restrict__ S_, int width, int height, int bounces, Px4* __restrict__ ga,
                                                                            Px4* __restrict__ gb, uint64_t* __restrict__ key) {
    const SceneRef S{S_, true, 0, true};
    const LdsScene Lds = stage_scene<true>(S);   // the scene-sized dynamic block, as denoise_guides_kernel takes it; ends with a barrier
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= width * height) return;
    const int x = i % width, y = i / width;
    f3 o, d;
    generate_ray(S, (float)x + 0.5f, (float)y + 0.5f, o, d);
    float t_sum = 0.f;
    uint64_t kk = 0;
    Px4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, (float)KY_DN_MISS};
    Px4 a0 = a, b0 = b;   // the first hit's guides: what an unresolved chain keeps
    for (int k = 0; k <= bounces; ++k) {
        float t = K_INF;
        const int hs = trace_nearest(S, o, d, t);
        if (hs < 0) {   // the chain leaves the scene: class 1, nobody's tap
            a = Px4{0.f, 0.f, 0.f, 0.f};
            b = Px4{0.f, 0.f, 0.f, (float)KY_DN_MISS};
            break;
        }
        t_sum += t;
        const DHit& H = Lds.hit[hs];
        Vertex v;
        v.t = t;
        v.position = o + t * d;
        v.normal = hit_normal(H, v.position, d);
        v.surface = hs;
        v.bsdf = make_bsdf(Lds.mat[H.material], 0.5f);   // (a plastic surface's draw: either of its lobes ends the chain)
        const bool lamp = H.area_light >= 0;
        a = Px4{v.normal.x, v.normal.y, v.normal.z, t_sum};
        b = Px4{v.position.x, v.position.y, v.position.z, lamp ? (float)KY_DN_LIGHT : (float)KY_DN_SURFACE};
        if (k == 0) { a0 = a; b0 = b; }
        if (lamp || !bsdf_is_delta(v.bsdf)) break;
        if (k == bounces) {   // unresolved: the first hit's guides (a mirror or glass that carries no lamp: class 0) and the first digit
            a = a0;
            b = b0;
            kk = chain_unresolved(kk);
            break;
        }
        const DeltaSample s = bsdf_sample_delta(v, -d, 0.5f);
        kk |= chain_digit(S->orig[hs], s.reflected) << (KY_DN_KEY_DIGIT_BITS * k);
        o = offset_ray_origin(v.position, v.normal, s.wi);
        d = s.wi;
    }
    ga[i] = a;
    gb[i] = b;
    key[i] = kk;
}

// c0 of the material of (sorted) surface `hs` at the point p as a vertex there takes it (vertex_material): the look-up's colour where the staged record links a
// texture (bits 8-15 of exp_flags, stage_textures), the record's own elsewhere
KY_DEV f3 albedo_c0(const LdsScene& Lds, const TexLds& tx, const DMat& M, int hs, f3 p) {
    const int ti = (M.exp_flags >> 8) & 0xff;
    if (ti == 0) return ld3(M.c0);
    float us, vs;
    return tex_at(tx, ti - 1, hs, p, us, vs);
}

// The albedo of a frame with an albedo grid (DESIGN.md "Denoise", "Albedo"): per pixel grid x grid camera rays through the frame's own camera form
// (camera_ray_any: what path_begin<..., KY_CAM_ANY> does with a sample), laid over the pixel -- sub-sample (i, j) has the film pair ((i + 0.5) / G, (j + 0.5) / G)
// and the lens pair ((j + 0.5) / G, (G - 1 - i + 0.5) / G), j-major -- each walked as denoise_chain_guides_kernel walks the centre ray.  A sub-sample's colour
// starts at (1, 1, 1), takes what each delta branch it walks through carries (a mirror's c0; glass: c0 reflected, c1 transmitted) and the c0 of the matte, plastic
// or mirror surface it ends on; glass it ends on, a lamp and a miss multiply by nothing.  The pixel: the sum in visit order times the float 1 / G^2, and in w the
// sub-samples that ended on a surface without a lamp.  At most grid^2 (bounces + 1) traversals per lane.
__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_albedo_kernel(const DScene* __restrict__ S_, int width, int height, int bounces, int grid, float inv_grid,
                                                                      float inv_count, LensCam fc, TexConst tc, Px4* __restrict__ albedo) {
    KY_NOFMA_BODY
    const SceneRef S{S_, true, 0, true};
    const LdsScene Lds = stage_scene<true>(S);   // the scene-sized dynamic block, as denoise_guides_kernel takes it; ends with a barrier
    TexLds tx{nullptr, nullptr, nullptr};
    if (tc.set) tx = stage_textures(tc, Lds);    // (uniform over the launch: every thread reaches its barrier)
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= width * height) return;
    const int x = i % width, y = i / width;
    f3 sum = mk3(0, 0, 0);
    int ended = 0;
    for (int sj = 0; sj < grid; ++sj)
        for (int si = 0; si < grid; ++si) {
            const float fu = ((float)si + 0.5f) * inv_grid, fv = ((float)sj + 0.5f) * inv_grid;   // (inv_grid, inv_count: the host's 1 / G and 1 / G^2, rounded once)
            f3 o, d;
            camera_ray_any(S, fc, x, y, fu, fv, fv, ((float)(grid - 1 - si) + 0.5f) * inv_grid, o, d);
            f3 col = mk3(1, 1, 1);
            for (int k = 0; k <= bounces; ++k) {
                float t = K_INF;
                const int hs = trace_nearest(S, o, d, t);
                if (hs < 0) break;
                const DHit& H = Lds.hit[hs];
                if (H.area_light >= 0) break;
                const DMat& M = Lds.mat[H.material];
                Vertex v;
                v.t = t;
                v.position = o + t * d;
                v.normal = hit_normal(H, v.position, d);
                v.surface = hs;
                v.bsdf = make_bsdf(M, 0.5f);
                if (!bsdf_is_delta(v.bsdf) || k == bounces) {   // the vertex the walk ends on; a chain that is not followed further: a mirror shows its own colour, glass nothing
                    if (v.bsdf.lobe != LOBE_GLASS) col = col * albedo_c0(Lds, tx, M, hs, v.position);
                    ++ended;
                    break;
                }
                const DeltaSample s = bsdf_sample_delta(v, -d, 0.5f);
                col = col * (s.reflected ? albedo_c0(Lds, tx, M, hs, v.position) : ld3(M.c1));
                o = offset_ray_origin(v.position, v.normal, s.wi);
                d = s.wi;
            }
            sum = sum + col;
        }
    albedo[i] = Px4{sum.x * inv_count, sum.y * inv_count, sum.z * inv_count, (float)ended};
}

// (denoise_gather_albedo_kernel below repeats this body and adds one line: a change here belongs there too)
__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_gather_kernel(const unsigned long long* __restrict__ accum, const unsigned* __restrict__ flags,
                                                                      const NoisePixel* __restrict__ state, const BlockState* __restrict__ blocks, ShardConst sh, int width,
                                                                      int height, int total_spp, int n_done, int batches, const Px4* __restrict__ gb_traced,
                                                                      Px4* __restrict__ cv, Px4* __restrict__ gb) {
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= sh.n_pix) return;
    int x, y;
    kyn::noise_pixel_xy(sh, i, x, y);
    if (x >= width || y >= height) return;
    if (blocks) {   // a retired block's pixels stand at the counts it retired with
        const BlockState b = blocks[kyb::block_of_pixel(sh, i)];
        if (b.retired_at >= 0) { batches = b.batches; n_done = b.retired_at; }
    }
    const unsigned fl = flags[i];
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    Px4 g = gb_traced[at];
    if (n_done <= 0) g.w = (float)KY_DN_MISS;
    else if (fl & 0x1ffu) g.w = (float)KY_DN_FLAGGED;
    cv[at] = gather_pixel((long long)accum[3 * (size_t)i], (long long)accum[3 * (size_t)i + 1], (long long)accum[3 * (size_t)i + 2], fl, state[i].m2, total_spp, n_done, batches);
    gb[at] = g;
}

// ... of a frame with an albedo grid: the same gather (kept apart so that denoise_gather_kernel's listing stays what it was), and a class-0 pixel demodulated by
// its albedo (demodulate_pixel)
__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_gather_albedo_kernel(const unsigned long long* __restrict__ accum, const unsigned* __restrict__ flags,
                                                                             const NoisePixel* __restrict__ state, const BlockState* __restrict__ blocks, ShardConst sh,
                                                                             int width, int height, int total_spp, int n_done, int batches,
                                                                             const Px4* __restrict__ gb_traced, const Px4* __restrict__ albedo, Px4* __restrict__ cv,
                                                                             Px4* __restrict__ gb) {
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= sh.n_pix) return;
    int x, y;
    kyn::noise_pixel_xy(sh, i, x, y);
    if (x >= width || y >= height) return;
    if (blocks) {
        const BlockState b = blocks[kyb::block_of_pixel(sh, i)];
        if (b.retired_at >= 0) { batches = b.batches; n_done = b.retired_at; }
    }
    const unsigned fl = flags[i];
    const size_t at = (size_t)y * (size_t)width + (size_t)x;
    Px4 g = gb_traced[at];
    if (n_done <= 0) g.w = (float)KY_DN_MISS;
    else if (fl & 0x1ffu) g.w = (float)KY_DN_FLAGGED;
    Px4 c = gather_pixel((long long)accum[3 * (size_t)i], (long long)accum[3 * (size_t)i + 1], (long long)accum[3 * (size_t)i + 2], fl, state[i].m2, total_spp, n_done, batches);
    if (is_surface(g)) c = demodulate_pixel(c, albedo[at]);
    cv[at] = c;
    gb[at] = g;
}

__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_level_kernel(const Px4* __restrict__ cv_in, Px4* __restrict__ cv_out, const Px4* __restrict__ ga,
                                                                     const Px4* __restrict__ gb, int step, LevelConst k) {
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= k.width * k.height) return;
    cv_out[i] = level_pixel(cv_in, ga, gb, i % k.width, i / k.width, step, k);
}

// ... of a frame with guide bounces: taps share the pixel's chain key (level_pixel_t<true>; 8 more bytes per tap)
__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_level_keyed_kernel(const Px4* __restrict__ cv_in, Px4* __restrict__ cv_out, const Px4* __restrict__ ga,
                                                                           const Px4* __restrict__ gb, const uint64_t* __restrict__ key, int step, LevelConst k) {
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= k.width * k.height) return;
    cv_out[i] = level_pixel_t<true>(cv_in, ga, gb, key, i % k.width, i / k.width, step, k);
}

__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_add_kernel(const Px4* __restrict__ cv, float* __restrict__ film, size_t stride_px, int width, int height) {
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= width * height) return;
    const int x = i % width, y = i / width;
    const Px4 c = cv[i];
    float* px = film + ((size_t)y * stride_px + (size_t)x) * 3;
    px[0] += fminf(fmaxf(c.x, 0.f), 1.f); px[1] += fminf(fmaxf(c.y, 0.f), 1.f); px[2] += fminf(fmaxf(c.z, 0.f), 1.f);
}

// ... of a frame with an albedo grid: the class-0 pixels (gb: the classes the gather wrote) remodulated before the clamp
__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_add_albedo_kernel(const Px4* __restrict__ cv, const Px4* __restrict__ gb, const Px4* __restrict__ albedo,
                                                                          float* __restrict__ film, size_t stride_px, int width, int height) {
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= width * height) return;
    const int x = i % width, y = i / width;
    Px4 c = cv[i];
    if (is_surface(gb[i])) c = remodulate_pixel(c, albedo[i]);
    float* px = film + ((size_t)y * stride_px + (size_t)x) * 3;
    px[0] += fminf(fmaxf(c.x, 0.f), 1.f); px[1] += fminf(fmaxf(c.y, 0.f), 1.f); px[2] += fminf(fmaxf(c.z, 0.f), 1.f);
}

// Temporal reuse (kyhip_frame_denoise_temporal; DESIGN.md "Denoise", "Temporal"): one thread per film pixel between the gather and the first level.  It reads the
// frame's three Px4 at the pixel (and its key when KEYED) and at most four taps of three Px4 from the history's old side -- bounds-checked inside temporal_pixel_t,
// and not at all while the history holds no picture -- and writes the history's new side whole.  No LDS, no atomics, the taps in one order.
template <bool KEYED>
__global__ __launch_bounds__(KY_DN_BLOCK) void denoise_temporal_kernel(const Px4* __restrict__ cv, const Px4* __restrict__ ga, const Px4* __restrict__ gb,
                                                                        const uint64_t* __restrict__ key, const Px4* __restrict__ hcv, const Px4* __restrict__ hga,
                                                                        const Px4* __restrict__ hgb, Px4* __restrict__ ncv, Px4* __restrict__ nga, Px4* __restrict__ ngb,
                                                                        TemporalConst k) {
    const int i = blockIdx.x * KY_DN_BLOCK + threadIdx.x;
    if (i >= k.width * k.height) return;
    const TemporalPixel o = temporal_pixel_t<KEYED>(cv, ga, gb, key, hcv, hga, hgb, i % k.width, i / k.width, k);
    ncv[i] = o.cv;
    nga[i] = ga[i];
    ngb[i] = o.gb;
}

namespace kydn {
static dim3 film_grid(int width, int height) { return dim3((unsigned)((width * height + KY_DN_BLOCK - 1) / KY_DN_BLOCK)); }

// The scene on the device, `launch(scene, lds_bytes)` on the stream, and the WAIT: the scene cache's slot is the kernel's until it is done, so all under the context's lock
template <class Launch>
static int trace_guides(int device, const ky_scene* scene, void* stream_, Launch launch) {
    DeviceCtx* c;
    KY_TRY(get_ctx(device, &c));
    std::lock_guard<std::mutex> lock(c->m);
    hipStream_t stream = (hipStream_t)stream_;
    SceneSlot* sc;
    KY_TRY(upload_scene(c, scene, stream, &sc));
    launch((const DScene*)sc->d, (size_t)lds_scene_bytes(scene->surface_count, scene->material_count, scene->light_count), stream);
    const hipError_t launched = hipGetLastError();
    const hipError_t done = hipStreamSynchronize(stream);
    HIP_TRY(launched);
    HIP_TRY(done);
    return KY_OK;
}

int denoise_guides_device(int device, const ky_scene* scene, int width, int height, void* ga, void* gb, void* stream) {
    if (width <= 0 || height <= 0) return KY_OK;
    return trace_guides(device, scene, stream, [&](const DScene* S, size_t lds, hipStream_t s) {
        hipLaunchKernelGGL(denoise_guides_kernel, film_grid(width, height), dim3(KY_DN_BLOCK), lds, s, S, width, height, (Px4*)ga, (Px4*)gb);
    });
}

static_assert(((KYHIP_MAX_SURFACES + 1) << 1 | 1) < (1 << KY_DN_KEY_DIGIT_BITS) && KY_DN_KEY_DIGIT_BITS * KYHIP_GUIDE_MAX_BOUNCES <= 62, "a chain's digits fit its key");

int denoise_chain_guides_device(int device, const ky_scene* scene, int width, int height, int bounces, void* ga, void* gb, void* key, void* stream) {
    if (bounces < 1 || bounces > KYHIP_GUIDE_MAX_BOUNCES) return fail(KY_ERR_INVALID_VALUE, "guide bounces %d: 1 .. %d", bounces, KYHIP_GUIDE_MAX_BOUNCES);
    if (width <= 0 || height <= 0) return KY_OK;
    return trace_guides(device, scene, stream, [&](const DScene* S, size_t lds, hipStream_t s) {
        hipLaunchKernelGGL(denoise_chain_guides_kernel, film_grid(width, height), dim3(KY_DN_BLOCK), lds, s, S, width, height, bounces, (Px4*)ga, (Px4*)gb, (uint64_t*)key);
    });
}

int denoise_albedo_device(int device, const ky_scene* scene, int width, int height, int bounces, int grid, const LensCam& cam, const TexConst& tex, void* albedo, void* stream) {
    if (bounces < 0 || bounces > KYHIP_GUIDE_MAX_BOUNCES) return fail(KY_ERR_INVALID_VALUE, "guide bounces %d: 0 .. %d", bounces, KYHIP_GUIDE_MAX_BOUNCES);
    if (grid < 1 || grid > KY_DN_ALBEDO_MAX_GRID) return fail(KY_ERR_INVALID_VALUE, "albedo grid %d: 1 .. %d", grid, KY_DN_ALBEDO_MAX_GRID);
    if (width <= 0 || height <= 0) return KY_OK;
    const float inv_grid = 1.f / (float)grid, inv_count = 1.f / (float)(grid * grid);   // (host divisions: correctly rounded)
    return trace_guides(device, scene, stream, [&](const DScene* S, size_t lds, hipStream_t s) {
        hipLaunchKernelGGL(denoise_albedo_kernel, film_grid(width, height), dim3(KY_DN_BLOCK), lds, s, S, width, height, bounces, grid, inv_grid, inv_count, cam, tex, (Px4*)albedo);
    });
}

int denoise_gather_device(const void* ws, const void* noise_state, const void* blocks, const ShardConst& sh, int width, int height, int total_spp, int n_done, int batches,
                          const void* gb_traced, void* cv, void* gb, void* stream) {
    if (sh.n_pix <= 0) return KY_OK;
    const unsigned long long* accum = (const unsigned long long*)ws;
    const unsigned* flags = (const unsigned*)(accum + (size_t)sh.n_pix * 3);
    hipLaunchKernelGGL(denoise_gather_kernel, dim3((unsigned)((sh.n_pix + KY_DN_BLOCK - 1) / KY_DN_BLOCK)), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, accum, flags,
                       (const NoisePixel*)noise_state, (const BlockState*)blocks, sh, width, height, total_spp, n_done, batches, (const Px4*)gb_traced, (Px4*)cv, (Px4*)gb);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int denoise_gather_albedo_device(const void* ws, const void* noise_state, const void* blocks, const ShardConst& sh, int width, int height, int total_spp, int n_done,
                                 int batches, const void* gb_traced, const void* albedo, void* cv, void* gb, void* stream) {
    if (sh.n_pix <= 0) return KY_OK;
    const unsigned long long* accum = (const unsigned long long*)ws;
    const unsigned* flags = (const unsigned*)(accum + (size_t)sh.n_pix * 3);
    hipLaunchKernelGGL(denoise_gather_albedo_kernel, dim3((unsigned)((sh.n_pix + KY_DN_BLOCK - 1) / KY_DN_BLOCK)), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, accum, flags,
                       (const NoisePixel*)noise_state, (const BlockState*)blocks, sh, width, height, total_spp, n_done, batches, (const Px4*)gb_traced, (const Px4*)albedo,
                       (Px4*)cv, (Px4*)gb);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int denoise_level_device(const void* cv_in, void* cv_out, const void* ga, const void* gb, int step, const LevelConst& k, void* stream) {
    if (k.width <= 0 || k.height <= 0) return KY_OK;
    hipLaunchKernelGGL(denoise_level_kernel, film_grid(k.width, k.height), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, (const Px4*)cv_in, (Px4*)cv_out, (const Px4*)ga,
                       (const Px4*)gb, step, k);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int denoise_level_keyed_device(const void* cv_in, void* cv_out, const void* ga, const void* gb, const void* key, int step, const LevelConst& k, void* stream) {
    if (k.width <= 0 || k.height <= 0) return KY_OK;
    hipLaunchKernelGGL(denoise_level_keyed_kernel, film_grid(k.width, k.height), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, (const Px4*)cv_in, (Px4*)cv_out,
                       (const Px4*)ga, (const Px4*)gb, (const uint64_t*)key, step, k);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int denoise_temporal_device(const void* cv, const void* ga, const void* gb, const void* key, const void* hcv, const void* hga, const void* hgb, void* ncv, void* nga,
                            void* ngb, const TemporalConst& k, void* stream) {
    if (k.width <= 0 || k.height <= 0) return KY_OK;
    if (key)
        hipLaunchKernelGGL(denoise_temporal_kernel<true>, film_grid(k.width, k.height), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, (const Px4*)cv, (const Px4*)ga,
                           (const Px4*)gb, (const uint64_t*)key, (const Px4*)hcv, (const Px4*)hga, (const Px4*)hgb, (Px4*)ncv, (Px4*)nga, (Px4*)ngb, k);
    else
        hipLaunchKernelGGL(denoise_temporal_kernel<false>, film_grid(k.width, k.height), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, (const Px4*)cv, (const Px4*)ga,
                           (const Px4*)gb, (const uint64_t*)nullptr, (const Px4*)hcv, (const Px4*)hga, (const Px4*)hgb, (Px4*)ncv, (Px4*)nga, (Px4*)ngb, k);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int denoise_add_device(const void* cv, float* film, size_t stride_px, int width, int height, void* stream) {
    if (width <= 0 || height <= 0) return KY_OK;
    hipLaunchKernelGGL(denoise_add_kernel, film_grid(width, height), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, (const Px4*)cv, film, stride_px, width, height);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int denoise_add_albedo_device(const void* cv, const void* gb, const void* albedo, float* film, size_t stride_px, int width, int height, void* stream) {
    if (width <= 0 || height <= 0) return KY_OK;
    hipLaunchKernelGGL(denoise_add_albedo_kernel, film_grid(width, height), dim3(KY_DN_BLOCK), 0, (hipStream_t)stream, (const Px4*)cv, (const Px4*)gb, (const Px4*)albedo, film,
                       stride_px, width, height);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}
}  // namespace kydn
