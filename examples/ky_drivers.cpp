/*
 * ky_drivers.cpp -- the reference's experiment drivers (ky.cpp:4675-4949) written against ky_amd/host/ky.hpp,
 * i.e. the same call shape `use_devices(*integrator); integrator->render(&scene, sampler.get(), &film); film.next_subfilm();` with the
 * rendering done by the MI355X library.  Workload definitions only: spp, grids and scene flags are the reference's.
 *
 *   ky_drivers single [spp4]     render_single_scene       (4675): 1024x1024 Cornell + environment light
 *   ky_drivers debug             render_debug              (4715): Veach position / normal / basecolor, 1x3 grid
 *   ky_drivers multiple_integrator render_multiple_integrator (4740): 4 Cornell lights x 5 integrators, 4x5 grid
 *   ky_drivers direct_sample     render_direct_sample_enum (4779): 4 Cornell lights x 5 strategies, 4x5 grid
 *   ky_drivers multiple_scene    render_multiple_scene     (4819): 3 strategies x 4 Cornell lights, 3x4 grid
 *   ky_drivers mis               render_mis_scene          (4878): Veach x 6 strategies, 2x3 grid
 *   ky_drivers lighting_enum [spp] [w] [h]  BASELINE.json configs[1]: the scene of the reference's (commented-out) render_lighting_enum
 *                                (4907-4935: Cornell, both small spheres, area light) at 1024 x 768, 1024 spp, path_tracing_iteration d5
 *                                both_mis; writes lighting_enum.bmp
 *   ky_drivers lighting_cells [spp] [cell]  render_lighting_enum (4907-4935) made to work: the scene above as emitted, direct, indirect and all light,
 *                                path_tracing_recursion_defered_t(10, both_mis, e) into a film_grid_t(1, 4, cell, cell) (256); writes lighting_cells.bmp
 *   ky_drivers batch [spp] [res] BASELINE.json configs[3]: render_multiple_scene scaled up -- the four Cornell light variants
 *                                (both_mis), Veach (both_mis) and a first-hit AOV pass, each res x res (1024) at spp (2048),
 *                                into a film_grid_t(2, 3, res, res); writes batch.bmp
 *   ky_drivers stress [spp] [res] BASELINE.json configs[4]: Cornell res x res (4096), spp (16384), max depth 16; writes stress.bmp
 *   ky_drivers progressive [spp] [w] [h]  the frame of lighting_enum (512 spp, 1024 x 768) rendered in passes of at least 64 samples (kyhip_frame_*): prints the
 *                                reference's progress line (3703) per pass, writes progressive_preview.bmp after the first pass and progressive.bmp at the end
 *   ky_drivers converge [threshold] [spp_cap] [w] [h]  the same frame until it is clean (0.01, at most 4096 spp, 1024 x 768): per pass the progress line and the noise
 *                                statistics (kyhip_frame_noise_stats); writes converge.bmp and converge_noise.bmp, the map scaled by 1 / threshold and clamped
 *   ky_drivers adaptive [threshold] [spp] [w] [h]  the same frame rendered adaptively (0.008, 1024 spp, 1024 x 768): passes of 64, and after each the 8 x 8 pixel
 *                                blocks at most a tenth of whose pixels are noisier than the threshold retire (integrator_t::render_adaptive); writes adaptive.bmp:
 *                                the picture and, next to it, the sample-count map (white: the frame's total)
 *   ky_drivers denoise [low_spp] [spp] [w] [h]  the same frame after its first low_spp samples (64 of 1024, 1024 x 768), in two passes, as the plain mean and through
 *                                the edge-avoiding filter (integrator_t::render_denoised), next to the complete frame; writes denoise.bmp: raw | denoised | full
 *                                (a fifth argument, guide_bounces 1 .. 4, adds the filter with specular-chain guides: raw | first-hit | chains | full;
 *                                a sixth, albedo_grid 1 .. 8, one more cell before the full frame: the filter with those guide bounces and albedo demodulation)
 *   ky_drivers flythrough [frames] [spp] [size]  the Cornell box with both balls along a fixed camera path (8 frames of 16 spp, 512 x 384: a dolly, a move to the right and a
 *                                pan), guide bounces 1, every frame denoised across the frames before it (history_t; kyhip_frame_denoise_temporal); writes fly_NNN.bmp
 *   ky_drivers sliced [n] [spp] [w] [h]  the same frame by sample range (3 slices, 512 spp, 1024 x 768; kyhip_frame_begin_slice, kyhip_frame_merge_from): the n slices
 *                                render on device 0 one after the other, slice 0 merges the rest; prints per slice its samples and kernel time, the merge times, and
 *                                whether the film is render()'s bit for bit (it must be: exit status 1 otherwise); writes sliced.bmp
 *   ky_drivers stratified [scene] [spp] [cell]  one scene (cornell, the default, or veach) under the random and the stratified sampler side by side at equal spp
 *                                (16; cells of 256, the Veach scene 256 x 144), path_tracing_iteration d5 both_mis into a film_grid_t(1, 2, ...); prints both
 *                                kernel times and writes stratified.bmp: random | stratified
 *   ky_drivers filtered [spp] [cell]  the Cornell box at a preview's sample count (16; cells of 256) under the box, the tent (radius 2) and the default Gaussian pixel
 *                                filter side by side (film_t::set_filter, kyhip_render_filtered), path_tracing_iteration d5 both_mis into a film_grid_t(1, 3, ...);
 *                                prints the three kernel times and writes filtered.bmp: box | tent | gaussian
 *   ky_drivers lens [spp] [cell]      the Cornell box at a preview's sample count (16; cells of 256) through the pinhole and through a thin lens (camera_t::set_lens,
 *                                kyhip_render_lens) of radius 2 % and 4 % of the scene's diagonal focused on the front ball -- the nearest sphere a coarse grid of pinhole
 *                                rays finds (kyhip_kat_camera, kyhip_kat_scene_intersect) --, path_tracing_iteration d5 both_mis into a film_grid_t(1, 3, ...); prints
 *                                the focus distance and the three kernel times and writes lens.bmp: pinhole | lens | wider lens
 *   ky_drivers textured [spp] [size] the Cornell box (16 spp; 256 x 256) with a 4 x 4 checker on its floor and a small image, generated here, on the wall the camera
 *                                faces (checker_texture_t, image_texture_t on plastic_material_t / matte_material_t; kyhip_render_textured), path_tracing_iteration d5
 *                                both_mis; prints the kernel's name and time and writes textured.bmp
 *   ky_drivers pick [spp] [w] [h]    the Veach frame under sample_single_light with its light picked uniformly (49), by power (113) and by position at the vertex
 *                                (177) side by side at equal spp (16; cells of 512 x 288), path_tracing_iteration d5 into a film_grid_t(1, 3, ...); writes pick.bmp:
 *                                uniform | power | spatial
 * An optional last argument multiplies every spp (the reference's values are tiny because its CPU path is slow).
 * KY_DEVICES=all (or a count n: devices 0 .. n-1) makes every integrator spread its tiles over that many GPUs of the node
 * (integrator_t::set_devices); the images do not depend on it.
 */
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../ky_amd/host/ky.hpp"

using namespace ky;

static int g_spp_scale = 1;

// KY_DEVICES: the GPUs every integrator of this process renders on
static void use_devices(integrator_t& integrator) {
    const char* e = std::getenv("KY_DEVICES");
    if (!e || !*e) return;
    std::vector<int> all = integrator_t::all_devices();
    if (std::strcmp(e, "all") != 0) {
        const int n = std::atoi(e);
        if (n < 1) return;
        all.resize((size_t)n);
        for (int i = 0; i < n; ++i) all[(size_t)i] = i;
    }
    integrator.set_devices(all);
}

template <typename F>
static double timing_seconds(F f) {  // wall clock (the reference's clock() counts CPU time on Linux, ky.cpp:156-163)
    const auto t0 = std::chrono::steady_clock::now();
    f();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

static void render_single_scene(int spp4) {
    const int width = 1024, height = 1024;
    film_t film(width, height);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_environment, film.get_resolution());
    const int samples_per_pixel = (spp4 > 0 ? spp4 / 4 : 16) * g_spp_scale;
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(samples_per_pixel);
    auto integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
    use_devices(*integrator);
    const double seconds = timing_seconds([&] { integrator->render(&scene, sampler.get(), &film); });
    std::printf("%d spp, %.3f seconds (kernel %.3f ms), %.1f Msamples/s\n", samples_per_pixel, seconds, integrator->last_kernel_ms(),
                (double)width * height * samples_per_pixel / seconds / 1e6);
    film.store_image("single");
}

static void render_debug() {
    film_grid_t film(1, 3, 512, 308);
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(10 * g_spp_scale);
    scene_t scene = scene_t::create_mis_scene(film.get_resolution());
    for (auto e : {integrator_enum_t::position, integrator_enum_t::normal, integrator_enum_t::basecolor}) {
        std::unique_ptr<integrator_t> integrator = std::make_unique<debug_integrator_t>(e);
        use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
        film.next_subfilm();
    }
    film.store_image("render_debug");
}

static const std::vector<std::pair<cornell_box_enum_t, int>>& scene_params(bool multiple_scene) {
    static const std::vector<std::pair<cornell_box_enum_t, int>> a{{cornell_box_enum_t::light_point, 1}, {cornell_box_enum_t::light_direction, 10},
                                                                   {cornell_box_enum_t::light_area, 1}, {cornell_box_enum_t::light_environment, 10}};
    static const std::vector<std::pair<cornell_box_enum_t, int>> b{{cornell_box_enum_t::light_point, 10}, {cornell_box_enum_t::light_direction, 40},
                                                                   {cornell_box_enum_t::light_area, 40}, {cornell_box_enum_t::light_environment, 10}};
    return multiple_scene ? b : a;
}

static void render_multiple_integrator() {
    const std::vector<integrator_enum_t> integrator_enums{integrator_enum_t::direct_lighting, integrator_enum_t::simple_path_tracing_recursion,
                                                          integrator_enum_t::path_tracing_recursion, integrator_enum_t::path_tracing_recursion_defered,
                                                          integrator_enum_t::path_tracing_iteration};
    film_grid_t film(4, 5, 256, 256);
    for (auto [scene_enum, spp] : scene_params(false)) {
        scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | scene_enum, film.get_resolution());
        std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp * g_spp_scale);
        for (auto integrator_enum : integrator_enums) {
            auto integrator = create_integrator(integrator_enum, 5, direct_sample_enum_t::both_mis);
            use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
            film.next_subfilm();
        }
    }
    film.store_image("direct_sample");   // (sic) the reference writes this driver's mosaic under the same name, 4776
}

static void render_direct_sample_enum() {
    const std::vector<direct_sample_enum_t> sample_enums{direct_sample_enum_t::bsdf, direct_sample_enum_t::light, direct_sample_enum_t::bsdf_mis,
                                                        direct_sample_enum_t::light_mis, direct_sample_enum_t::both_mis};
    film_grid_t film(4, 5, 256, 256);
    for (auto [scene_enum, spp] : scene_params(false)) {
        std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp * g_spp_scale);
        scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | scene_enum, film.get_resolution());
        for (auto sample_enum : sample_enums) {
            std::unique_ptr<integrator_t> integrator = std::make_unique<path_tracing_iteration_t>(5, sample_enum);
            use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
            film.next_subfilm();
        }
    }
    film.store_image("direct_sample");
}

static void render_multiple_scene() {
    const std::vector<direct_sample_enum_t> sample_enums{direct_sample_enum_t::bsdf, direct_sample_enum_t::light, direct_sample_enum_t::both_mis};
    film_grid_t film(3, 4, 256, 256);
    for (auto sample_enum : sample_enums) {
        std::unique_ptr<integrator_t> integrator = std::make_unique<path_tracing_iteration_t>(5, sample_enum);
        for (auto [scene_enum, spp] : scene_params(true)) {
            std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp * g_spp_scale);
            scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | scene_enum, film.get_resolution());
            use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
            film.next_subfilm();
        }
    }
    film.store_image("light_mis");
}

static void render_mis_scene() {
    film_grid_t film(2, 3, 512, 308);
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(10 * g_spp_scale);
    scene_t scene = scene_t::create_mis_scene(film.get_resolution());
    for (auto sample_enum : {direct_sample_enum_t::bsdf, direct_sample_enum_t::light, direct_sample_enum_t::idle, direct_sample_enum_t::bsdf_mis,
                             direct_sample_enum_t::light_mis, direct_sample_enum_t::both_mis}) {
        std::unique_ptr<integrator_t> integrator = std::make_unique<path_tracing_iteration_t>(5, sample_enum);
        use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
        film.next_subfilm();
    }
    film.store_image("veach_mis");
}

// sample_single_light's three picks on the scene that tells them apart: one lamp holds 95 % of the power and lights a pixel about as much as each of the row's
static void render_pick(int spp, int width, int height) {
    film_grid_t film(1, 3, width, height);
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp);
    scene_t scene = scene_t::create_mis_scene(film.get_resolution());
    const direct_sample_enum_t single = direct_sample_enum_t::sample_single_light | direct_sample_enum_t::both_mis;
    for (auto sample_enum : {single, single | direct_sample_enum_t::pick_power, single | direct_sample_enum_t::pick_spatial}) {
        std::unique_ptr<integrator_t> integrator = std::make_unique<path_tracing_iteration_t>(5, sample_enum);
        use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
        film.next_subfilm();
    }
    film.store_image("pick");
}

// BASELINE.json configs[3]: the batch of render_multiple_scene (4819-4876) at production size -- one film_grid_t, one
// integrator->render() per cell, every frame's tiles interleaved over the GPUs of KY_DEVICES
static void render_batch(int spp, int res) {
    film_grid_t film(2, 3, res, res);
    double samples = 0;
    const double seconds = timing_seconds([&] {
        std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp);
        for (auto light : {cornell_box_enum_t::light_point, cornell_box_enum_t::light_direction, cornell_box_enum_t::light_area, cornell_box_enum_t::light_environment}) {
            scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | light, film.get_resolution());
            std::unique_ptr<integrator_t> integrator = std::make_unique<path_tracing_iteration_t>(5, direct_sample_enum_t::both_mis);
            use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
            film.next_subfilm();
            samples += (double)res * res * spp;
        }
        {
            scene_t scene = scene_t::create_mis_scene(film.get_resolution());
            std::unique_ptr<integrator_t> integrator = std::make_unique<path_tracing_iteration_t>(5, direct_sample_enum_t::both_mis);
            use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
            film.next_subfilm();
            samples += (double)res * res * spp;
            std::unique_ptr<integrator_t> aov = std::make_unique<debug_integrator_t>(integrator_enum_t::normal);   // the "debug" member of the batch
            std::unique_ptr<sampler_t> one = std::make_unique<debug_sampler_t>(1);
            use_devices(*aov); aov->render(&scene, one.get(), &film);
            samples += (double)res * res;
        }
    });
    std::printf("batch: 6 frames %dx%d, %d spp: %.3f seconds, %.1f Msamples/s\n", res, res, spp, seconds, samples / seconds / 1e6);
    film.store_image("batch");
}

// BASELINE.json configs[1]: the headline frame
static void render_lighting_enum(int spp, int width, int height) {
    film_t film(width, height);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, film.get_resolution());
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp);
    auto integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
    use_devices(*integrator);
    const double seconds = timing_seconds([&] { integrator->render(&scene, sampler.get(), &film); });
    std::printf("lighting_enum: %dx%d, %d spp: %.3f seconds (kernel %.3f ms), %.1f Msamples/s\n", width, height, spp, seconds, integrator->last_kernel_ms(),
                (double)width * height * spp / seconds / 1e6);
    film.store_image("lighting_enum");
}

// render_lighting_enum as the reference wrote it (4907-4935) -- it is commented out there: lighting_enum_t is never read (4423) and film_grid_t has no next_cell().
// One Cornell box four times: what it emits, its direct light, its indirect light, all of it.
static void render_lighting_cells(int spp, int cell) {
    film_grid_t film(1, 4, cell, cell);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, film.get_resolution());
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp);
    double kernel_ms = 0;
    for (auto e : {lighting_enum_t::emit, lighting_enum_t::direct, lighting_enum_t::indirect, lighting_enum_t::all}) {
        std::unique_ptr<integrator_t> integrator = std::make_unique<path_tracing_recursion_defered_t>(10, direct_sample_enum_t::both_mis, e);
        use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
        kernel_ms += integrator->last_kernel_ms();
        film.next_subfilm();
    }
    std::printf("lighting_cells: 4 cells %dx%d, %d spp: kernels %.3f ms\n", cell, cell, spp, kernel_ms);
    film.store_image("lighting_cells");
}

// One scene under random_sampler_t and stratified_sampler_t (ky.cpp:977, a stub there) at equal spp: what the strata buy at a preview's sample count.
static void render_stratified(bool veach, int spp, int cell) {
    const int width = cell, height = veach ? cell * 9 / 16 : cell;
    film_grid_t film(1, 2, width, height);
    scene_t scene = veach ? scene_t::create_mis_scene(film.get_resolution())
                          : scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, film.get_resolution());
    double ms[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        std::unique_ptr<sampler_t> sampler;
        if (k == 0) sampler = std::make_unique<random_sampler_t>(spp);
        else sampler = std::make_unique<stratified_sampler_t>(spp);
        auto integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
        use_devices(*integrator); integrator->render(&scene, sampler.get(), &film);
        ms[k] = integrator->last_kernel_ms();
        film.next_subfilm();
    }
    std::printf("stratified: %s %dx%d, %d spp: kernel %.3f ms random, %.3f ms stratified\n", veach ? "veach" : "cornell", width, height, spp, ms[0], ms[1]);
    film.store_image("stratified");
}

// The Cornell box under three pixel filters (the reference's empty `#pragma region filter`, ky.cpp:1525-1527): what a reconstruction filter does to the edges of a
// preview.  The film owns the filter; a filtered render runs on one device (the default list), so the cells do not take KY_DEVICES.
static void render_filtered(int spp, int cell) {
    film_grid_t film(1, 3, cell, cell);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::default_scene, film.get_resolution());
    const char* names[3] = {"box", "tent", "gaussian"};
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        if (k == 0) film.set_filter(std::make_unique<box_filter_t>());
        else if (k == 1) film.set_filter(std::make_unique<triangle_filter_t>(2.f));
        else film.set_filter(std::make_unique<gaussian_filter_t>());
        random_sampler_t sampler(spp);
        auto integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
        integrator->render(&scene, &sampler, &film);
        ms[k] = integrator->last_kernel_ms();
        film.next_subfilm();
    }
    std::printf("filtered: cornell %dx%d, %d spp: kernel", cell, cell, spp);
    for (int k = 0; k < 3; ++k) std::printf(" %.3f ms %s%s", ms[k], names[k], k < 2 ? "," : "\n");
    film.store_image("filtered");
}

// The Cornell box with textures (the reference's `// TODO class texture_t`, ky.cpp:2559-2564): a 4 x 4 checker on the floor -- the plane the balls stand on, whose material
// is the plastic one -- and an 8 x 8 image on the wall the camera faces, nearest and repeating twice each way.  The image is made here: red rises with x, green with
// y, in sixteenths.  The materials own their textures; the scene's flattening collects the set and the integrator hands it to kyhip_render_textured.
static void render_textured(int spp, int size) {
    film_t film(size, size);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::default_scene, film.get_resolution());
    const ky_scene& flat = scene.flatten();
    const int floor = flat.surfaces[3].material, wall = flat.surfaces[4].material;   // (surface_list_ order: 3 is the plane z = -1.28, 4 the plane y = -1.305)
    const ky_material fm = flat.materials[floor];
    std::vector<float> texels((size_t)8 * 8 * 3);
    for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) {
            float* t = &texels[((size_t)y * 8 + x) * 3];
            t[0] = (2 * x + 1) / 16.f; t[1] = (2 * y + 1) / 16.f; t[2] = 0.25f;
        }
    scene.replace_material(floor, std::make_shared<plastic_material_t>(std::make_shared<checker_texture_t>(color_t{0.25f, 0.25f, 0.0625f}, color_t{0.03125f, 0.0625f, 0.25f}, vec2_t{4, 4}),
                                                                       color_t{fm.color1[0], fm.color1[1], fm.color1[2]}, fm.exponent));
    scene.replace_material(wall, std::make_shared<matte_material_t>(std::make_shared<image_texture_t>(8, 8, texels, false, false, vec2_t{2, 2})));
    random_sampler_t sampler(spp);
    auto integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
    integrator->render(&scene, &sampler, &film);
    std::string kernel = kyhip_last_kernel(0);
    std::printf("textured: cornell %dx%d, %d spp: kernel %.3f ms  %s\n", size, size, spp, integrator->last_kernel_ms(), kernel.substr(0, kernel.find(" [")).c_str());
    film.store_image("textured");
}

// The Cornell box through a thin lens (the reference's commented-out `p_lens`, ky.cpp:870-874, and `// sample_ray(...)`, 1894): depth of field.  The camera owns
// the lens; a scene holds its camera const, so each cell renders with a copy of the camera that has the cell's lens.  One device, like a filtered render.
static void render_lens(int spp, int cell) {
    film_grid_t film(1, 3, cell, cell);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::default_scene, film.get_resolution());
    // focus: the depth along front of the nearest sphere hit among the pinhole rays through a 32 x 32 grid of the cell's pixels
    const ky_scene& flat = scene.flatten();
    const int g = 32, n = g * g;
    std::vector<float> film2((size_t)n * 2), rays6((size_t)n * 6), rays7((size_t)n * 7), hits9((size_t)n * 9);
    for (int i = 0; i < n; ++i) { film2[2 * (size_t)i] = ((i % g) + 0.5f) * cell / g; film2[2 * (size_t)i + 1] = ((i / g) + 0.5f) * cell / g; }
    if (kyhip_kat_camera(0, &flat.camera, film2.data(), n, rays6.data()) != KY_OK) throw std::runtime_error(std::string("kyhip_kat_camera: ") + kyhip_last_error());
    for (int i = 0; i < n; ++i) { std::copy(&rays6[6 * (size_t)i], &rays6[6 * (size_t)i] + 6, &rays7[7 * (size_t)i]); rays7[7 * (size_t)i + 6] = INFINITY; }
    if (kyhip_kat_scene_intersect(0, &flat, rays7.data(), n, hits9.data()) != KY_OK) throw std::runtime_error(std::string("kyhip_kat_scene_intersect: ") + kyhip_last_error());
    float focus = 0.f, nearest = INFINITY;
    for (int i = 0; i < n; ++i) {
        const float* hit = &hits9[9 * (size_t)i];
        if (hit[0] == 0.f || flat.shapes[flat.surfaces[(int)hit[8]].shape].kind != KY_SHAPE_SPHERE || !(hit[1] < nearest)) continue;
        nearest = hit[1];
        focus = 0.f;
        for (int k = 0; k < 3; ++k) focus += (hit[2 + k] - flat.camera.position[k]) * flat.camera.front[k];
    }
    if (!(focus > 0.f)) throw std::runtime_error("lens: no pinhole ray of the grid meets a ball");
    const bounds3_t bound = scene.world_bound();
    const float diagonal = (bound.max_ - bound.min_).magnitude();
    const float radii[3] = {0.f, 0.02f * diagonal, 0.04f * diagonal};
    float ms[3] = {0, 0, 0};
    const const_camera_sptr_t pinhole = std::make_shared<camera_t>(*scene.get_camera());
    for (int k = 0; k < 3; ++k) {
        auto camera = std::make_shared<camera_t>(*pinhole);
        camera->set_lens(radii[k], focus);
        scene.set_camera(camera);
        random_sampler_t sampler(spp);
        auto integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
        integrator->render(&scene, &sampler, &film);
        ms[k] = integrator->last_kernel_ms();
        film.next_subfilm();
    }
    std::printf("lens: cornell %dx%d, %d spp, focus %.4g: kernel %.3f ms pinhole, %.3f ms radius %.4g, %.3f ms radius %.4g\n", cell, cell, spp, focus, ms[0], ms[1], radii[1], ms[2], radii[2]);
    film.store_image("lens");
}

// The headline frame in passes: a picture after the first 64 samples, the reference's progress line (3703) after every pass, and a final image that is
// render()'s bit for bit (include/kyhip.h, kyhip_frame_*).
static void render_progressive(int spp, int width, int height) {
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, {(float)width, (float)height});
    ky_render_params p{};
    p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS;
    p.samples_per_pixel = spp; p.sampler = KY_SAMPLER_RANDOM; p.seed = random_sampler_t(spp).seed();
    p.width = width; p.height = height; p.tile_w = 16; p.tile_h = 16; p.tile_first = 0; p.tile_step = 1;
    kyhip_frame* frame = nullptr;
    if (kyhip_frame_begin(0, &scene.flatten(), &p, &frame) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_begin: ") + kyhip_last_error());
    struct frame_end_t { kyhip_frame* f; ~frame_end_t() { kyhip_frame_end(f); } } frame_end{frame};
    int done = 0, passes = 0;
    double kernel_ms = 0;
    const double seconds = timing_seconds([&] {
        while (done < spp) {
            if (kyhip_frame_render(frame, 64, &done) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_render: ") + kyhip_last_error());
            kernel_ms += kyhip_kernel_ms(0);
            std::printf("rendering... %d spp, %.2f%%\n", spp, 100. * done / spp);
            if (passes++ == 0) {   // the picture so far: the mean of the samples done
                film_t preview(width, height);
                if (kyhip_frame_resolve(frame, 1, preview.target_origin(), preview.row_stride_px()) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_resolve: ") + kyhip_last_error());
                preview.store_image("progressive_preview");
            }
        }
    });
    film_t film(width, height);
    if (kyhip_frame_resolve(frame, 0, film.target_origin(), film.row_stride_px()) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_resolve: ") + kyhip_last_error());
    std::printf("progressive: %dx%d, %d spp in %d passes: %.3f seconds (kernels %.3f ms)\n", width, height, spp, passes, seconds, kernel_ms);
    film.store_image("progressive");
}

// The headline frame by sample range: n slices of its samples, each over the whole film, merged into slice 0 (include/kyhip.h "Slices").  On one device the slices
// run one after the other; integrator_t::render_sliced gives each device of a list a thread.  Returns whether the film equals render()'s.
static bool render_sliced(int n, int spp, int width, int height) {
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, {(float)width, (float)height});
    ky_render_params p{};
    p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS;
    p.samples_per_pixel = spp; p.sampler = KY_SAMPLER_RANDOM; p.seed = random_sampler_t(spp).seed();
    p.width = width; p.height = height; p.tile_w = 16; p.tile_h = 16; p.tile_first = 0; p.tile_step = 1;
    std::vector<int> bounds((size_t)(n > 0 ? n : 0) + 1);
    if (kyhip_slice_bounds(spp, n, bounds.data()) != KY_OK) throw std::runtime_error(std::string("kyhip_slice_bounds: ") + kyhip_last_error());
    std::vector<kyhip_frame*> frames((size_t)n, nullptr);
    struct frames_end_t { std::vector<kyhip_frame*>& f; ~frames_end_t() { for (kyhip_frame* x : f) kyhip_frame_end(x); } } frames_end{frames};
    film_t film(width, height);
    const double seconds = timing_seconds([&] {
        for (int k = 0; k < n; ++k) {
            if (kyhip_frame_begin_slice(0, &scene.flatten(), &p, bounds[(size_t)k], bounds[(size_t)k + 1], &frames[(size_t)k]) != KY_OK)
                throw std::runtime_error(std::string("kyhip_frame_begin_slice: ") + kyhip_last_error());
            const int size = bounds[(size_t)k + 1] - bounds[(size_t)k];
            int done = 0, passes = 0;
            double kernel_ms = 0;
            while (done < size) {
                if (kyhip_frame_render(frames[(size_t)k], 64, &done) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_render: ") + kyhip_last_error());
                kernel_ms += kyhip_kernel_ms(0);
                ++passes;
            }
            std::printf("slice %d: samples %d..%d (%d) in %d passes, kernels %.3f ms\n", k, bounds[(size_t)k], bounds[(size_t)k + 1], size, passes, kernel_ms);
        }
        for (int k = 1; k < n; ++k) {
            float ms = -1.f;
            if (kyhip_frame_merge_from(frames[0], frames[(size_t)k]) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_merge_from: ") + kyhip_last_error());
            kyhip_frame_merge_ms(frames[0], &ms);
            std::printf("merge of slice %d: %.3f ms\n", k, (double)ms);
        }
        if (kyhip_frame_resolve(frames[0], 0, film.target_origin(), film.row_stride_px()) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_resolve: ") + kyhip_last_error());
    });
    film_t whole(width, height);
    if (kyhip_render(0, &scene.flatten(), &p, whole.target_origin(), whole.row_stride_px()) != KY_OK) throw std::runtime_error(std::string("kyhip_render: ") + kyhip_last_error());
    const bool same = std::memcmp(film.data(), whole.data(), (size_t)film.get_pixel_num() * 3 * sizeof(float)) == 0;
    std::printf("sliced: %dx%d, %d spp in %d slices: %.3f seconds; the film %s render()'s\n", width, height, spp, n, seconds, same ? "IS" : "IS NOT");
    film.store_image("sliced");
    return same;
}

// The same frame until it is clean: passes of at least 64 samples until at most 2 % of the pixels have a noise estimate (kyhip_frame_noise: the standard error
// of the pixel's mean luminance, in units of the film's white) above `threshold`, or the cap is reached.  Writes the mean of the samples done and the noise
// map scaled by 1 / threshold (white: at or above the threshold).
static void render_converge(float threshold, int spp_cap, int width, int height) {
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, {(float)width, (float)height});
    ky_render_params p{};
    p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS;
    p.samples_per_pixel = spp_cap; p.sampler = KY_SAMPLER_RANDOM; p.seed = random_sampler_t(spp_cap).seed();
    p.width = width; p.height = height; p.tile_w = 16; p.tile_h = 16; p.tile_first = 0; p.tile_step = 1;
    kyhip_frame* frame = nullptr;
    if (kyhip_frame_begin(0, &scene.flatten(), &p, &frame) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_begin: ") + kyhip_last_error());
    struct frame_end_t { kyhip_frame* f; ~frame_end_t() { kyhip_frame_end(f); } } frame_end{frame};
    if (kyhip_frame_track_noise(frame) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_track_noise: ") + kyhip_last_error());
    const float fraction = 0.02f;
    int done = 0, passes = 0;
    ky_noise_stats st{};
    bool clean = false;
    const double seconds = timing_seconds([&] {
        while (done < spp_cap && !clean) {
            if (kyhip_frame_render(frame, 64, &done) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_render: ") + kyhip_last_error());
            if (kyhip_frame_noise_stats(frame, threshold, &st) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_noise_stats: ") + kyhip_last_error());
            ++passes;
            std::printf("rendering... %d spp, %.2f%%\n", spp_cap, 100. * done / spp_cap);
            std::printf("  noise after %d batches: %lld of %lld pixels above %g (%lld flagged), max %g, mean %g\n", st.batches, (long long)st.above,
                        (long long)st.pixels, (double)threshold, (long long)st.flagged, (double)st.max, st.mean);
            clean = st.batches >= 2 && (double)st.above <= (double)fraction * (double)(st.pixels - st.flagged);
        }
    });
    std::printf("converge: %dx%d, %s at %d of %d spp in %d passes: %.3f seconds\n", width, height, clean ? "clean" : "NOT clean", done, spp_cap, passes, seconds);
    film_t film(width, height);
    if (kyhip_frame_resolve(frame, 1, film.target_origin(), film.row_stride_px()) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_resolve: ") + kyhip_last_error());
    film.store_image("converge");
    std::vector<float> map((size_t)width * height, 0.f);
    if (kyhip_frame_noise(frame, map.data(), (size_t)width) != KY_OK) throw std::runtime_error(std::string("kyhip_frame_noise: ") + kyhip_last_error());
    film_t noise(width, height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const float v = std::min(map[(size_t)y * width + x] / threshold, 1.f);
            noise.add_color(x, y, color_t{v, v, v});
        }
    noise.store_image("converge_noise");
}

// The headline frame rendered adaptively (integrator_t::render_adaptive; include/kyhip.h, kyhip_frame_track_blocks ...): the picture and the samples each pixel's
// block received, side by side.
static void render_adaptive(float threshold, int spp, int width, int height) {
    film_grid_t film(1, 2, width, height);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, film.get_resolution());
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp);
    std::unique_ptr<integrator_t> integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
    std::vector<int32_t> counts;
    ky_block_stats st{};
    const double seconds = timing_seconds([&] { st = integrator->render_adaptive(&scene, sampler.get(), &film, threshold, 0.10f, 3, 64, &counts); });
    std::printf("adaptive: %dx%d, threshold %g: %d passes, the front at %d of %d spp, %d of %d blocks still live; %.1f samples per pixel (%d .. %d): %.3f seconds\n", width,
                height, (double)threshold, st.passes, st.samples_done, spp, st.live, st.blocks, (double)st.pixel_samples / (double)st.pixels, st.min_samples, st.max_samples,
                seconds);
    film.next_subfilm();
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const float v = (float)counts[(size_t)y * width + x] / (float)spp;
            film.add_color(x, y, color_t{v, v, v});
        }
    film.store_image("adaptive");
}

// The headline frame early on, raw and denoised (integrator_t::render_denoised; include/kyhip.h, kyhip_frame_denoise), and complete: three cells side by side.  The
// first two are the same samples: the frame's first passes, two of at least low_spp / 2 samples.  guide_bounces 1 .. 4 adds a cell, the same samples once more
// denoised with guides that follow the balls' mirror and glass that far (kyhip_frame_set_guide_bounces): raw | first-hit | chains | full.  albedo_grid 1 .. 8 adds
// another before the full frame: those guide bounces and albedo demodulation (kyhip_frame_set_albedo_grid).
static void render_denoise(int low_spp, int spp, int width, int height, int guide_bounces, int albedo_grid) {
    film_grid_t film(1, 3 + (guide_bounces > 0 ? 1 : 0) + (albedo_grid > 0 ? 1 : 0), width, height);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, film.get_resolution());
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp);
    std::unique_ptr<integrator_t> integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
    const int per_pass = std::max(1, (low_spp + 1) / 2);
    int raw_done = 0, passes = 0;
    integrator->render_passes(&scene, sampler.get(), &film, per_pass, [&](int done, int) { raw_done = done; return ++passes < 2 || done < low_spp; });
    film.next_subfilm();
    int done = 0;
    const double seconds = timing_seconds([&] { done = integrator->render_denoised(&scene, sampler.get(), &film, per_pass, low_spp); });
    film.next_subfilm();
    if (guide_bounces > 0) {
        integrator->render_denoised(&scene, sampler.get(), &film, per_pass, low_spp, nullptr, guide_bounces);
        film.next_subfilm();
    }
    if (albedo_grid > 0) {
        integrator->render_denoised(&scene, sampler.get(), &film, per_pass, low_spp, nullptr, guide_bounces, albedo_grid);
        film.next_subfilm();
    }
    integrator->render(&scene, sampler.get(), &film);
    std::printf("denoise: %dx%d, raw at %d and denoised at %d of %d spp (%.3f seconds with its passes)%s%s, then the complete frame\n", width, height, raw_done, done, spp, seconds,
                guide_bounces > 0 ? ", denoised once more with specular-chain guides" : "", albedo_grid > 0 ? ", and once more with albedo demodulation" : "");
    film.store_image("denoise");
}

// A fly-through denoised across its frames (history_t, integrator_t::render_denoised(..., history_t*); include/kyhip.h, kyhip_frame_denoise_temporal): the Cornell
// box with both balls, guide bounces 1, the camera dollying forwards, moving to its right and panning along a fixed path; every frame has `spp` samples in two
// passes and a seed of its own, and takes what the frames before it saw of the surfaces it sees.  Writes fly_NNN.bmp per frame.
static void render_flythrough(int frames, int spp, int size) {
    const int width = size, height = size * 3 / 4;
    film_t film(width, height);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, film.get_resolution());
    const ky_camera start = scene.flatten().camera;
    const vec3_t p0{start.position[0], start.position[1], start.position[2]}, f0{start.front[0], start.front[1], start.front[2]};
    const vec3_t r0 = vec3_t{start.right[0], start.right[1], start.right[2]}.normalize(), up{start.up[0], start.up[1], start.up[2]};
    const float fov_degree = 2.f * std::atan(up.magnitude()) * 180.f / 3.14159265358979f;
    history_t history(width, height);
    std::unique_ptr<integrator_t> integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 5, direct_sample_enum_t::both_mis);
    float kernel_ms = 0.f;
    for (int k = 0; k < frames; ++k) {
        const float s = frames > 1 ? (float)k / (float)(frames - 1) : 0.f;
        scene.set_camera(std::make_shared<camera_t>(p0 + f0 * (0.6f * s) + r0 * (0.3f * s), f0 + r0 * (0.12f * s), up, fov_degree, film.get_resolution()));
        film_t frame_film(width, height);
        random_sampler_t sampler(spp);
        sampler.set_seed(1234u + (unsigned)k);
        integrator->render_denoised(&scene, &sampler, &frame_film, std::max(1, (spp + 1) / 2), spp, nullptr, 1, 0, &history);
        kernel_ms += history.ms();
        char name[32];
        std::snprintf(name, sizeof name, "fly_%03d", k);
        frame_film.store_image(name);
    }
    std::printf("flythrough: %d frames of %dx%d at %d spp, guide bounces 1; the temporal kernel took %.3f ms per frame\n", frames, width, height, spp, kernel_ms / (float)frames);
}

// BASELINE.json configs[4]: the stress frame
static void render_stress(int spp, int res) {
    film_t film(res, res);
    scene_t scene = scene_t::create_cornell_box_scene(cornell_box_enum_t::both_small_spheres | cornell_box_enum_t::light_area, film.get_resolution());
    std::unique_ptr<sampler_t> sampler = std::make_unique<random_sampler_t>(spp);
    auto integrator = create_integrator(integrator_enum_t::path_tracing_iteration, 16, direct_sample_enum_t::both_mis);
    use_devices(*integrator);
    const double seconds = timing_seconds([&] { integrator->render(&scene, sampler.get(), &film); });
    std::printf("stress: %dx%d, %d spp, depth 16: %.3f seconds, %.1f Msamples/s\n", res, res, spp, seconds, (double)res * res * spp / seconds / 1e6);
    film.store_image("stress");
}

int main(int argc, char* argv[]) {
    const char* which = argc > 1 ? argv[1] : "single";
    try {
        if (!std::strcmp(which, "single")) {
            if (argc > 3) g_spp_scale = std::atoi(argv[3]);
            render_single_scene(argc > 2 ? std::atoi(argv[2]) : 0);
        } else if (!std::strcmp(which, "lighting_enum")) {
            render_lighting_enum(argc > 2 ? std::atoi(argv[2]) : 1024, argc > 3 ? std::atoi(argv[3]) : 1024, argc > 4 ? std::atoi(argv[4]) : 768);
        } else if (!std::strcmp(which, "progressive")) {
            render_progressive(argc > 2 ? std::atoi(argv[2]) : 512, argc > 3 ? std::atoi(argv[3]) : 1024, argc > 4 ? std::atoi(argv[4]) : 768);
        } else if (!std::strcmp(which, "sliced")) {
            if (!render_sliced(argc > 2 ? std::atoi(argv[2]) : 3, argc > 3 ? std::atoi(argv[3]) : 512, argc > 4 ? std::atoi(argv[4]) : 1024, argc > 5 ? std::atoi(argv[5]) : 768)) return 1;
        } else if (!std::strcmp(which, "converge")) {
            const float threshold = argc > 2 ? (float)std::atof(argv[2]) : 0.01f;
            if (!(threshold > 0.f)) { std::fprintf(stderr, "converge: a threshold above 0\n"); return 2; }
            render_converge(threshold, argc > 3 ? std::atoi(argv[3]) : 4096, argc > 4 ? std::atoi(argv[4]) : 1024, argc > 5 ? std::atoi(argv[5]) : 768);
        } else if (!std::strcmp(which, "adaptive")) {
            const float threshold = argc > 2 ? (float)std::atof(argv[2]) : 0.008f;
            if (!(threshold > 0.f)) { std::fprintf(stderr, "adaptive: a threshold above 0\n"); return 2; }
            render_adaptive(threshold, argc > 3 ? std::atoi(argv[3]) : 1024, argc > 4 ? std::atoi(argv[4]) : 1024, argc > 5 ? std::atoi(argv[5]) : 768);
        } else if (!std::strcmp(which, "denoise")) {
            render_denoise(argc > 2 ? std::atoi(argv[2]) : 64, argc > 3 ? std::atoi(argv[3]) : 1024, argc > 4 ? std::atoi(argv[4]) : 1024, argc > 5 ? std::atoi(argv[5]) : 768,
                           argc > 6 ? std::atoi(argv[6]) : 0, argc > 7 ? std::atoi(argv[7]) : 0);
        } else if (!std::strcmp(which, "flythrough")) {
            const int frames = argc > 2 ? std::atoi(argv[2]) : 8, spp = argc > 3 ? std::atoi(argv[3]) : 16, size = argc > 4 ? std::atoi(argv[4]) : 512;
            if (frames < 1 || frames > 999 || spp < 2 || size < 16) { std::fprintf(stderr, "flythrough: 1 .. 999 frames, two samples per pixel or more, a film of 16 or more\n"); return 2; }
            render_flythrough(frames, spp, size);
        } else if (!std::strcmp(which, "stratified")) {
            const bool veach = argc > 2 && !std::strcmp(argv[2], "veach");
            if (argc > 2 && !veach && std::strcmp(argv[2], "cornell")) { std::fprintf(stderr, "stratified: cornell or veach\n"); return 2; }
            const int spp = argc > 3 ? std::atoi(argv[3]) : 16, cell = argc > 4 ? std::atoi(argv[4]) : 256;
            if (spp < 1 || spp > (1 << 24) || cell < 16) { std::fprintf(stderr, "stratified: 1 .. 2^24 samples per pixel, cells of 16 or more\n"); return 2; }
            render_stratified(veach, spp, cell);
        } else if (!std::strcmp(which, "filtered")) {
            const int spp = argc > 2 ? std::atoi(argv[2]) : 16, cell = argc > 3 ? std::atoi(argv[3]) : 256;
            if (spp < 1 || cell < 16) { std::fprintf(stderr, "filtered: at least one sample per pixel, cells of 16 or more\n"); return 2; }
            render_filtered(spp, cell);
        } else if (!std::strcmp(which, "lens")) {
            const int spp = argc > 2 ? std::atoi(argv[2]) : 16, cell = argc > 3 ? std::atoi(argv[3]) : 256;
            if (spp < 1 || cell < 16) { std::fprintf(stderr, "lens: at least one sample per pixel, cells of 16 or more\n"); return 2; }
            render_lens(spp, cell);
        } else if (!std::strcmp(which, "textured")) {
            const int spp = argc > 2 ? std::atoi(argv[2]) : 16, size = argc > 3 ? std::atoi(argv[3]) : 256;
            if (spp < 1 || size < 16) { std::fprintf(stderr, "textured: at least one sample per pixel, a film of 16 or more\n"); return 2; }
            render_textured(spp, size);
        } else if (!std::strcmp(which, "pick")) {
            const int spp = argc > 2 ? std::atoi(argv[2]) : 16, w = argc > 3 ? std::atoi(argv[3]) : 512, h = argc > 4 ? std::atoi(argv[4]) : 288;
            if (spp < 1 || w < 16 || h < 16) { std::fprintf(stderr, "pick: at least one sample per pixel, cells of 16 x 16 or more\n"); return 2; }
            render_pick(spp, w, h);
        } else if (!std::strcmp(which, "lighting_cells")) {
            render_lighting_cells(argc > 2 ? std::atoi(argv[2]) : 10, argc > 3 ? std::atoi(argv[3]) : 256);
        } else if (!std::strcmp(which, "batch")) {
            render_batch(argc > 2 ? std::atoi(argv[2]) : 2048, argc > 3 ? std::atoi(argv[3]) : 1024);
        } else if (!std::strcmp(which, "stress")) {
            render_stress(argc > 2 ? std::atoi(argv[2]) : 16384, argc > 3 ? std::atoi(argv[3]) : 4096);
        } else {
            if (argc > 2) g_spp_scale = std::atoi(argv[2]);
            if (g_spp_scale < 1) g_spp_scale = 1;
            if (!std::strcmp(which, "debug")) render_debug();
            else if (!std::strcmp(which, "multiple_integrator")) render_multiple_integrator();
            else if (!std::strcmp(which, "direct_sample")) render_direct_sample_enum();
            else if (!std::strcmp(which, "multiple_scene")) render_multiple_scene();
            else if (!std::strcmp(which, "mis")) render_mis_scene();
            else { std::fprintf(stderr, "unknown driver '%s'\n", which); return 2; }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
