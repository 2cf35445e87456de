/*
 * ky_capi.cpp -- a thin C API over the C++ host layer (ky.hpp) so that Python (ctypes) can build the
 * reference's scenes, drive integrator_t::render() exactly as a C++ caller would, and use the film
 * writers.  Plumbing only: no rendering arithmetic lives here.
 */
#include <cstring>
#include <memory>
#include <string>

#include "ky.hpp"

static thread_local std::string g_host_error;

namespace {
struct scene_box {
    ky::scene_t scene;
};
template <typename F>
int guarded(F f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        g_host_error = e.what();
        return -1;
    }
}
}  // namespace

extern "C" {

const char* kyhost_last_error(void) { return g_host_error.c_str(); }

// scene_t::create_cornell_box_scene(flags, resolution), ky.cpp:3240.  NULL on error (both large balls: 3268-3271).
void* kyhost_scene_create_cornell_box(int flags, float width, float height) {
    scene_box* box = nullptr;
    guarded([&] { box = new scene_box{ky::scene_t::create_cornell_box_scene((ky::cornell_box_enum_t)flags, {width, height})}; });
    return box;
}

// scene_t::create_mis_scene(resolution), ky.cpp:3434
void* kyhost_scene_create_mis(float width, float height) {
    scene_box* box = nullptr;
    guarded([&] { box = new scene_box{ky::scene_t::create_mis_scene({width, height})}; });
    return box;
}

void kyhost_scene_destroy(void* scene) { delete (scene_box*)scene; }

// flat view (valid until the scene is destroyed)
const ky_scene* kyhost_scene_flatten(void* scene) {
    const ky_scene* flat = nullptr;
    guarded([&] { flat = &((scene_box*)scene)->scene.flatten(); });
    return flat;
}

// Material `material` of the scene rebuilt from a texture (ky.hpp: the texture_sptr_t overloads of matte_material_t, mirror_material_t and plastic_material_t): the
// material keeps its kind and, for plastic, its specular colour and exponent; glass takes no texture.  Every render entry below then renders the scene textured.
static void retexture(ky::scene_t& scene, int material, ky::texture_sptr_t texture) {
    if (material < 0 || material >= scene.material_count()) throw std::runtime_error("texture: material index out of range");
    const ky_material m = scene.material(material)->flatten();
    ky::material_sptr_t made;
    if (m.kind == KY_MATERIAL_MATTE) made = std::make_shared<ky::matte_material_t>(texture);
    else if (m.kind == KY_MATERIAL_MIRROR) made = std::make_shared<ky::mirror_material_t>(texture);
    else if (m.kind == KY_MATERIAL_PLASTIC) made = std::make_shared<ky::plastic_material_t>(texture, ky::color_t{m.color1[0], m.color1[1], m.color1[2]}, m.exponent);
    else throw std::runtime_error("texture: a glass material takes no texture");
    scene.replace_material(material, made);
}
// checker_texture_t(a, b, scale, offset) on material `material`
int kyhost_scene_texture_checker(void* scene, int material, const float* a3, const float* b3, const float* scale2, const float* offset2) {
    return guarded([&] {
        retexture(((scene_box*)scene)->scene, material, std::make_shared<ky::checker_texture_t>(ky::color_t{a3[0], a3[1], a3[2]}, ky::color_t{b3[0], b3[1], b3[2]},
                                                                                                 ky::vec2_t{scale2[0], scale2[1]}, ky::vec2_t{offset2[0], offset2[1]}));
    });
}
// image_texture_t(width, height, texels, bilinear, clamp, scale, offset) on material `material`; the texels are copied
int kyhost_scene_texture_image(void* scene, int material, int width, int height, const float* texels, int bilinear, int clamp, const float* scale2, const float* offset2) {
    return guarded([&] {
        if (width < 1 || height < 1 || !texels) throw std::runtime_error("texture: an image of width x height RGB triples");
        std::vector<float> copy(texels, texels + (size_t)width * (size_t)height * 3);
        retexture(((scene_box*)scene)->scene, material, std::make_shared<ky::image_texture_t>(width, height, std::move(copy), bilinear != 0, clamp != 0,
                                                                                               ky::vec2_t{scale2[0], scale2[1]}, ky::vec2_t{offset2[0], offset2[1]}));
    });
}
// scene_t::flatten_textures(): writes min(count, max) ky_texture to `out` (may be NULL with max 0) and returns the count, or -1 on error.  Pointers inside are valid
// until the scene is destroyed or retextured.
int kyhost_scene_textures(void* scene, ky_texture* out, int max) {
    int n = -1;
    guarded([&] {
        const std::vector<ky_texture>& set = ((scene_box*)scene)->scene.flatten_textures();
        for (int i = 0; i < (int)set.size() && i < max; ++i) out[i] = set[(size_t)i];
        n = (int)set.size();
    });
    return n;
}

// the sampler_t of a ky_sampler_kind (every other value: the random sampler, as before the stratified one existed)
static std::unique_ptr<ky::sampler_t> make_sampler(int kind, int spp, unsigned seed) {
    std::unique_ptr<ky::sampler_t> sampler;
    if (kind == KY_SAMPLER_DEBUG) sampler = std::make_unique<ky::debug_sampler_t>(spp);
    else if (kind == KY_SAMPLER_STRATIFIED) sampler = std::make_unique<ky::stratified_sampler_t>(spp);
    else sampler = std::make_unique<ky::random_sampler_t>(spp);
    sampler->set_seed(seed);
    return sampler;
}

// create_integrator(enum, depth, direct_sample)->render(&scene, sampler, &film) on a film_t (grid_rows = 0)
// or on cell `cell` of a film_grid_t(grid_rows, grid_cols, width, height): the call shape of every
// reference driver (ky.cpp:4697, 4732, 4770, 4810, 4851, 4899).  film points at the WHOLE film
// (grid_cols*width x grid_rows*height when a grid is used) and is accumulated into.
// Returns 0, -1 on error, -2 when create_integrator returns nullptr.
static int render_impl(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed,
                       int width, int height, int grid_rows, int grid_cols, int cell, float* film, int device, int lighting) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, device < 0 ? 0 : device);                          // 4730-4731
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, device < 0 ? 0 : device);  // 4621
        if (!integrator) { status = -2; return; }
        if (lighting >= 0) {   // kyhost_render_lighting: set_lighting of the integrators that have one; every other integrator renders all or throws
            if (auto* pi = dynamic_cast<ky::path_integrator_t*>(integrator.get())) pi->set_lighting((ky::lighting_enum_t)lighting);
            else if (auto* dl = dynamic_cast<ky::direct_lighting_t*>(integrator.get())) dl->set_lighting((ky::lighting_enum_t)lighting);
            else if ((lighting & 7) != 7 || lighting > 31 || ((lighting >> 3) & 1) != ((lighting >> 4) & 1)) throw std::runtime_error("lighting_enum_t: the debug integrators render all only");
        }
        // device < 0 selects a device LIST: -1 = every visible GPU; -n (n >= 2) = device 0 listed n times, which drives the
        // multi-device path (shards, gather, one add) on a single GPU
        if (device == -1) integrator->set_devices(ky::integrator_t::all_devices());
        else if (device < -1) integrator->set_devices(std::vector<int>((size_t)-device, 0));
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        std::unique_ptr<ky::film_t> f;
        if (grid_rows > 0) {
            auto grid = std::make_unique<ky::film_grid_t>(grid_rows, grid_cols, width, height);
            for (int i = 0; i < cell; ++i) grid->next_subfilm();
            f = std::move(grid);
        } else {
            f = std::make_unique<ky::film_t>(width, height);
        }
        const size_t n = (size_t)f->get_pixel_num() * 3;
        std::memcpy(f->data(), film, n * sizeof(float));
        integrator->render(&((scene_box*)scene)->scene, sampler.get(), f.get());
        std::memcpy(film, f->data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

int kyhost_render(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed,
                  int width, int height, int grid_rows, int grid_cols, int cell, float* film, int device) {
    return render_impl(scene, integrator_enum, depth, direct_sample_enum, sampler_kind, spp, seed, width, height, grid_rows, grid_cols, cell, film, device, -1);
}
// kyhost_render after integrator->set_lighting(lighting) (lighting_enum_t, ky.cpp:3591-3603): the light classes of the mask only
int kyhost_render_lighting(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed,
                           int width, int height, int grid_rows, int grid_cols, int cell, float* film, int device, int lighting) {
    if (lighting < 0) { g_host_error = "lighting_enum_t: negative mask"; return -1; }
    return render_impl(scene, integrator_enum, depth, direct_sample_enum, sampler_kind, spp, seed, width, height, grid_rows, grid_cols, cell, film, device, lighting);
}

// film_t::set_filter then one of the integrator's render entries on a film_t of width x height: the film's pixel filter (ky.hpp, filter_t) through the host mirror.
// filter_kind: ky_filter_kind, with `radius` and `param` (the Gaussian's sigma).  mode 0: render(); 1: render_passes(min_samples_per_pass) to the end; 2:
// render_sliced over {device, device}; 3: render_until with a threshold nothing reaches (it renders to the end and adds the mean of all samples).
// `film` is read, added to and written back.  Returns 0, -1 on error, -2 when create_integrator returns nullptr.
int kyhost_render_filtered(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                           float* film, int device, int filter_kind, float radius, float param, int mode, int min_samples_per_pass) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, device);
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, device);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        if (filter_kind == KY_FILTER_BOX) f.set_filter(std::make_unique<ky::box_filter_t>());
        else if (filter_kind == KY_FILTER_TENT) f.set_filter(std::make_unique<ky::triangle_filter_t>(radius));
        else if (filter_kind == KY_FILTER_GAUSSIAN) f.set_filter(std::make_unique<ky::gaussian_filter_t>(radius, param));
        else if (filter_kind == KY_FILTER_BLACKMAN_HARRIS) f.set_filter(std::make_unique<ky::blackman_harris_filter_t>(radius));
        else throw std::runtime_error("kyhost_render_filtered: unknown filter kind");
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        ky::scene_t* sc = &((scene_box*)scene)->scene;
        if (mode == 0) integrator->render(sc, sampler.get(), &f);
        else if (mode == 1) integrator->render_passes(sc, sampler.get(), &f, min_samples_per_pass, {});
        else if (mode == 2) integrator->render_sliced(sc, sampler.get(), &f, std::vector<int>{device, device}, min_samples_per_pass);
        else if (mode == 3) integrator->render_until(sc, sampler.get(), &f, 0.f, 0.f, 2, min_samples_per_pass);
        else throw std::runtime_error("kyhost_render_filtered: mode 0 .. 3");
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// camera_t::set_lens(radius, focus_distance) on a copy of the scene's camera (scene_t::set_camera), then one of the integrator's render entries on a film_t of
// width x height: the camera's lens through the host mirror.  mode 0: render(); 1: render_passes(min_samples_per_pass) to the end; 2: render_sliced over
// {device, device}.  The scene gets its own camera back whatever happens.  `film` is read, added to and written back.  Returns 0, -1 on error, -2 when
// create_integrator returns nullptr.
int kyhost_render_lens(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                       float* film, int device, float radius, float focus_distance, int mode, int min_samples_per_pass) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator = ky::create_integrator((ky::integrator_enum_t)integrator_enum, depth, (ky::direct_sample_enum_t)direct_sample_enum, device);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        ky::scene_t* sc = &((scene_box*)scene)->scene;
        struct restore_camera {
            ky::scene_t* sc;
            ky::const_camera_sptr_t pinhole;
            ~restore_camera() { sc->set_camera(pinhole); }
        } restore{sc, std::make_shared<ky::camera_t>(*sc->get_camera())};
        auto with_lens = std::make_shared<ky::camera_t>(*sc->get_camera());
        with_lens->set_lens(radius, focus_distance);
        sc->set_camera(with_lens);
        if (mode == 0) integrator->render(sc, sampler.get(), &f);
        else if (mode == 1) integrator->render_passes(sc, sampler.get(), &f, min_samples_per_pass, {});
        else if (mode == 2) integrator->render_sliced(sc, sampler.get(), &f, std::vector<int>{device, device}, min_samples_per_pass);
        else throw std::runtime_error("kyhost_render_lens: mode 0 .. 2");
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// create_integrator(...)->render_passes(&scene, sampler, &film, min_samples_per_pass, on_pass) on a film_t of width x height; on_pass(done, total, user) returns
// nonzero to go on (NULL: render to the end).  `film` is read, added to and written back.  Returns 0, -1 on error, -2 when create_integrator returns nullptr.
int kyhost_render_passes(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                         float* film, int device, int min_samples_per_pass, int (*on_pass)(int done, int total, void* user), void* user) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, device);
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, device);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        std::function<bool(int, int)> cb;
        if (on_pass) cb = [&](int done, int total) { return on_pass(done, total, user) != 0; };
        integrator->render_passes(&((scene_box*)scene)->scene, sampler.get(), &f, min_samples_per_pass, cb);
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// create_integrator(...)->render_sliced(&scene, sampler, &film, {devices[0 .. n_devices)}, min_samples_per_pass, {}) on a film_t of width x height: the frame by
// sample range, rendered to the end.  `film` is read, added to and written back.  Returns 0, -1 on error, -2 when create_integrator returns nullptr.
int kyhost_render_sliced(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                         float* film, const int* devices, int n_devices, int min_samples_per_pass) {
    int status = 0;
    int rc = guarded([&] {
        if (!devices || n_devices < 1) throw std::runtime_error("kyhost_render_sliced: an empty device list");
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, devices[0]);
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, devices[0]);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        integrator->render_sliced(&((scene_box*)scene)->scene, sampler.get(), &f, std::vector<int>(devices, devices + n_devices), min_samples_per_pass);
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// create_integrator(...)->render_until(&scene, sampler, &film, threshold, max_fraction_above, min_batches, min_samples_per_pass) on a film_t of width x height.
// `film` is read, added to and written back.  Returns the samples done per pixel (>= 1), -1 on error, -2 when create_integrator returns nullptr.
int kyhost_render_until(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                        float* film, int device, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, device);
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, device);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        status = integrator->render_until(&((scene_box*)scene)->scene, sampler.get(), &f, threshold, max_fraction_above, min_batches, min_samples_per_pass);
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// create_integrator(...)->render_denoised(&scene, sampler, &film, min_samples_per_pass, stop_after_samples, params) on a film_t of width x height; params may be
// NULL (the library's defaults).  `film` is read, added to and written back.  Returns the samples done per pixel (>= 1), -1 on error, -2 when create_integrator
// returns nullptr.  kyhost_render_denoised_chains: ... with render_denoised's guide_bounces (kyhip_frame_set_guide_bounces); the other is its 0.
// kyhost_render_denoised_albedo: ... and its albedo_grid (kyhip_frame_set_albedo_grid); the other two are its 0.
int kyhost_render_denoised_albedo(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                                  float* film, int device, int min_samples_per_pass, int stop_after_samples, const ky_denoise_params* params, int guide_bounces,
                                  int albedo_grid);
int kyhost_render_denoised_chains(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                                  float* film, int device, int min_samples_per_pass, int stop_after_samples, const ky_denoise_params* params, int guide_bounces) {
    return kyhost_render_denoised_albedo(scene, integrator_enum, depth, direct_sample_enum, sampler_kind, spp, seed, width, height, film, device, min_samples_per_pass,
                                         stop_after_samples, params, guide_bounces, 0);
}
int kyhost_render_denoised(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                           float* film, int device, int min_samples_per_pass, int stop_after_samples, const ky_denoise_params* params) {
    return kyhost_render_denoised_chains(scene, integrator_enum, depth, direct_sample_enum, sampler_kind, spp, seed, width, height, film, device, min_samples_per_pass,
                                         stop_after_samples, params, 0);
}
int kyhost_render_denoised_albedo(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                                  float* film, int device, int min_samples_per_pass, int stop_after_samples, const ky_denoise_params* params, int guide_bounces,
                                  int albedo_grid) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, device);
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, device);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        status = integrator->render_denoised(&((scene_box*)scene)->scene, sampler.get(), &f, min_samples_per_pass, stop_after_samples, params, guide_bounces, albedo_grid);
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// create_integrator(...)->render_adaptive(&scene, sampler, &film, threshold, max_fraction_above, min_batches, min_samples_per_pass, &counts) on a film_t of width x
// height.  `film` is read, added to and written back; sample_counts (may be NULL) receives width x height int32; *stats (may be NULL) the block statistics.
// Returns 0, -1 on error, -2 when create_integrator returns nullptr.
int kyhost_render_adaptive(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed, int width, int height,
                           float* film, int device, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int32_t* sample_counts,
                           ky_block_stats* stats) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, device);
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, device);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        std::vector<int32_t> counts;
        const ky_block_stats st = integrator->render_adaptive(&((scene_box*)scene)->scene, sampler.get(), &f, threshold, max_fraction_above, min_batches,
                                                              min_samples_per_pass, sample_counts ? &counts : nullptr);
        if (stats) *stats = st;
        if (sample_counts) std::memcpy(sample_counts, counts.data(), counts.size() * sizeof(int32_t));
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// create_integrator(...)->debug_area(&scene, sampler, &film, {bx, by}, {ex, ey}) on a film_t of width x height (ky.cpp:3733-3777);
// `film` is read, modified and written back.  Returns 0, -1 on error, -2 when create_integrator returns nullptr.
int kyhost_debug_area(void* scene, int integrator_enum, int depth, int direct_sample_enum, int sampler_kind, int spp, unsigned seed,
                      int width, int height, float* film, int bx, int by, int ex, int ey, int device) {
    int status = 0;
    int rc = guarded([&] {
        std::unique_ptr<ky::integrator_t> integrator;
        const auto ie = (ky::integrator_enum_t)integrator_enum;
        if (ie == ky::integrator_enum_t::position || ie == ky::integrator_enum_t::normal || ie == ky::integrator_enum_t::basecolor)
            integrator = std::make_unique<ky::debug_integrator_t>(ie, device);
        else
            integrator = ky::create_integrator(ie, depth, (ky::direct_sample_enum_t)direct_sample_enum, device);
        if (!integrator) { status = -2; return; }
        std::unique_ptr<ky::sampler_t> sampler = make_sampler(sampler_kind, spp, seed);
        ky::film_t f(width, height);
        const size_t n = (size_t)f.get_pixel_num() * 3;
        std::memcpy(f.data(), film, n * sizeof(float));
        if (ex == bx + 1 && ey == by + 1) integrator->debug_pixel(&((scene_box*)scene)->scene, sampler.get(), &f, ky::point2_t((float)bx, (float)by));
        else integrator->debug_area(&((scene_box*)scene)->scene, sampler.get(), &f, ky::point2_t((float)bx, (float)by), ky::point2_t((float)ex, (float)ey));
        std::memcpy(film, f.data(), n * sizeof(float));
    });
    return rc != 0 ? rc : status;
}

// film writers, ky.cpp:1646-1782.  kind: 0 ppm, 1 bmp, 2 hdr (image_enum_t, 1531-1536)
int kyhost_store_image(const char* filename, int kind, int width, int height, const float* rgb) {
    bool ok = false;
    guarded([&] {
        switch (kind) {
        case 0: ok = ky::film_t::store_ppm_impl(filename, width, height, 3, rgb); break;
        case 1: ok = ky::film_t::store_bmp_impl(filename, width, height, 3, rgb); break;
        case 2: ok = ky::film_t::store_hdr_impl(filename, width, height, 3, rgb); break;
        default: g_host_error = "unknown image kind"; break;
        }
    });
    return ok ? 0 : -1;
}

int kyhost_gamma_encoding(float x) { return ky::gamma_encoding(x); }

}  // extern "C"
