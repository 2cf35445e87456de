/*
 * ky_host.hpp -- what the host-side translation units of libkyhip.so share that needs NO HIP runtime: error reporting, parameter checks and shard
 * geometry, scene packing and the occluder classification, the launch policies (specialisation, deferred shadow rays, engine), the run-time
 * instantiations' code cache, and the small thread pool of the host-film seam.  Implemented in ky_pack.cpp, ky_frame_book.cpp (pass_boundaries) and ky_jit.cpp, which are plain C++:
 * `make sanitize` builds them with g++ -fsanitize=address,undefined / thread next to the oracle and runs them through tests/test_sanitize.py.
 * (The HIP side -- device contexts, streams, the scene cache -- is ky_ctx.hpp.)
 */
#pragma once
#include <cstddef>
#include <cstdint>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include <sys/types.h>

#include "ky_shard.hpp"   // ky_scene.hpp (DScene ...), ShardConst, the chunk schedule

namespace kyh {
using namespace kyd;

// ---- errors: kyhip_last_error() returns the calling thread's last message ----
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const std::string& last_error();
// a call that returns a KY_* status (and has set the message): any other than KY_OK is the caller's
#define KY_TRY(expr)                            \
    do {                                        \
        const int rc_ = (expr);                 \
        if (rc_ != KY_OK) return rc_;           \
    } while (0)

// ---- parameters and shard geometry ----
bool valid_params(const ky_render_params* p);
bool shard_in_range(const ky_render_params* p);
ShardConst make_shard(const ky_render_params* p);
RenderConstS make_rc(const ky_render_params* p);   // the launch constants with the stratified sampler's strata; every other kernel takes its RenderConst (ky_scene.hpp)
// The stratified sampler has strata for the frame's own samples only: what the KAT entries refuse before any device work.
// strat_samples_check: samples s0 .. s0 + n - 1 of a launch of p (every other sampler: any index).  kat_sampler_kind_check: kyhip_kat_sampler_kind's arguments.
int strat_samples_check(const ky_render_params* p, int s0, int n);
int kat_sampler_kind_check(int kind, int spp, const uint32_t* keys2, int n, int k, const uint32_t* out);
// The film's range rule (DESIGN.md "Film"): N = the most terms one accumulator word can receive in a launch of p (n_lights lights, on the queue engine or
// the lane engine with or without deferred shadow rays), and the term limit T = min(2e9, 2^31 / N) as a float rounded down (0 when it is below 1:
// such a launch is refused with KY_ERR_LIMIT).  n_lights: 0 .. KYHIP_MAX_LIGHTS.
long long film_term_count(const ky_render_params* p, int n_lights, bool queue_engine, bool deferred);
float film_term_limit(long long n_terms);
// Whether every kernel a launch of p on a scene of n_lights lights may run on has a term limit T >= 1: the count with deferred shadow rays (where the strategy
// has them) bounds every other one.  film_range_check: KY_OK, or KY_ERR_LIMIT with the message -- the render entry points call it next to shard_in_range,
// before any device work.
bool film_in_range(const ky_render_params* p, int n_lights);
int film_range_check(const ky_render_params* p, const ky_scene* scene);
// Light classes (lighting_enum_t, ky.cpp:3591-3603): how a render of p that keeps only the classes of `lighting` (bit 1 emit, 2 direct, 4
// indirect; 8 and 16 both or neither) is run.  Most of a mask is a shorter path: without the indirect class the launch's depth is min(depth, 1), with emit alone 0,
// and what is left for the kernels are two drop bits (path_intersect, ky_device.hpp): 1 no emission at the first vertex, 2 no k = 1 term.  `nothing`: the mask
// selects no class this launch can produce -- no launch at all.  `plain`: the launch is the unmasked one (every class it can produce is selected).
struct LightingPlan {
    int mask = 7, effective_depth = 0, dropped = 0;
    bool nothing = false, plain = true;
};
int lighting_check(int integrator, int lighting);   // KY_OK, or KY_ERR_INVALID_VALUE with the message: the mask's own validity and whether the integrator renders it
int lighting_plan(const ky_render_params* p, int lighting, LightingPlan* out);   // KY_OK, or KY_ERR_INVALID_VALUE with the message
std::string lighting_note(const ky_render_params* p, int lighting, const LightingPlan& plan);   // what kyhip_last_kernel says of the launch's form ("" for a plain one)
inline size_t workspace_bytes_for(const ShardConst& s) { return (size_t)s.n_pix * (3 * sizeof(unsigned long long) + sizeof(unsigned)); }   // per pixel: 3 x 64-bit fixed-point sums + one flag word

// ---- passes of a frame (kyhip_frame_*; the chunk arithmetic is ky_shard.hpp's) ----
int pass_boundaries(int spp, int* bounds, int n);   // kyhip_pass_boundaries
// (a frame's checkpoint: ky_checkpoint.hpp; its bookkeeping: ky_frame_book.hpp)
// The stop rule's arguments, refused before a frame or a device is looked at, in this order by every entry that takes them (ky_frame.cpp and the host-only
// builds' stand-ins, ky_hostcheck.cpp): KY_OK, or KY_ERR_INVALID_VALUE with the message
int threshold_check(float threshold);                                                  // a noise level is >= 0 (a NaN is not)
int stop_rule_check(float threshold, float max_fraction_above, int min_batches);      // threshold_check, then the fraction in 0 .. 1, then min_batches >= 2
int pass_samples_check(int min_samples_per_pass);                                      // >= 1
int denoise_params_check(const ky_denoise_params* p);                                  // levels 0 .. 6, normal_squarings 0 .. 10, both sigmas > 0 (a NaN is not)
int temporal_params_check(const ky_temporal_params* t);                                // max_history in (0, 1024], sigma_plane > 0, min_weight in [0, 1), normal_squarings 0 .. 10
double denoise_pixel_width(const ky_camera& camera, int width);                        // the width of a pixel at unit distance: 2 |camera.right| / width

// ---- scene packing (ky_pack.cpp) ----
void cp3(float* d, const float* s);
void pack_shape(const ky_shape& sh, int full_index, DSurf* surf, DShapeFull* full);
void pack_material(const ky_material& m, DMat* d);
bool shape_normal_ok(const ky_shape& sh);
struct NonOccluders {
    std::vector<char> wall;                  // [surface]
    std::vector<char> light_ok;              // [light]
    bool deferred_ok = false;                // all lights ok (the deferred shadow rays share one stack)
    int ts_light = -1;                       // two-stage scan (DScene::occ_front / occ_behind): the light, its plane n.x = k, and
    double ts_plane[4] = {0, 0, 0, 0};       // the surfaces that lie entirely in n.x <= k (not the light's own)
    std::vector<char> ts_behind;             // [surface]
};
void find_non_occluders(const ky_scene* in, NonOccluders& R);
// Axis-aligned boxes whose faces are surfaces of the scene (DBox, ky_scene.hpp): which, and which surface is which face.
struct Boxes {
    struct Box { float lo[3], hi[3]; int face[6]; };   // face[2 axis + side] = the caller's surface index, -1: an open side
    std::vector<Box> box;
    std::vector<int> box_of;                            // [surface] -> box, -1: none
};
void find_boxes(const ky_scene* in, Boxes& B);
// The live rectangle of a scene (DScene::live; ky_pack.cpp states the proof): live[0..3] = x0, y0, x1, y1, the whole range when the proof does not hold
void screen_bound(const ky_scene* in, int32_t live[4]);
// ... and for a launch's tiling: the 8 x 8 blocks of the shard that lie outside it (the work items a render kernel skips per chunk), and all of them
void screen_bound_counts(const int32_t live[4], const ky_render_params* p, long long* dead, long long* total);
// ---- pixel filters (ky_pixel_filter; ky_pack.cpp) ----
int filter_check(const ky_pixel_filter* f);                    // kyhip_filter_check
inline bool filter_is_box(const ky_pixel_filter* f) { return !f || f->kind == KY_FILTER_BOX; }
int filter_grow(const ky_pixel_filter* f);                     // the pixels a valid filter's offsets reach beyond the pixel, ceil(radius - 0.5); 0 for a box
void filter_table(const ky_pixel_filter* f, float* out);       // kyhip_filter_table's KYHIP_FILTER_TABLE + 1 floats, of a valid filter
std::string filter_describe(const ky_pixel_filter* f);         // "tent filter, radius 2", "Gaussian filter, radius 1.5, sigma 0.5", "box filter"
// the scene hash a frame's header carries under `f`: `hash` itself for a box, else `hash` with the filter's kind, radius bits and param bits folded in
uint64_t filter_fold(uint64_t hash, const ky_pixel_filter* f);
// the live rectangle as a launch under `f` reads it: grown by filter_grow on every side (the kernels' work decoder does the same, ky_render.hpp)
void screen_bound_widen(const int32_t live[4], const ky_pixel_filter* f, int32_t out[4]);
// ---- the thin lens (ky_lens; ky_pack.cpp) ----
int lens_check(const ky_lens* l);                              // kyhip_lens_check
inline bool lens_is_pinhole(const ky_lens* l) { return !l || !(l->radius > 0.f); }
std::string lens_describe(const ky_lens* l);                   // "lens radius 0.02, focus 1.45", "pinhole"
// the scene hash a frame's header carries under `l`: `hash` itself for the pinhole, else `hash` with the bits of radius and focus_distance folded in
uint64_t lens_fold(uint64_t hash, const ky_lens* l);
// a valid lens of radius > 0 in the units of `cam`'s generate_ray, computed in double and rounded once (LensConst, ky_scene.hpp)
kyd::LensConst lens_const(const ky_camera* cam, const ky_lens* l);
// ... refused (KY_ERR_INVALID_VALUE) where they are not finite: a camera whose front, right or up has no length or is not finite
int lens_const_checked(const ky_camera* cam, const ky_lens* l, kyd::LensConst* out);
// ---- textures (ky_texture; ky_pack.cpp) ----
int texture_check(const ky_scene* scene, const ky_texture* textures, int n);   // kyhip_texture_check
// a valid set as the device reads it: the block (descriptors, links, the uv record of every surface by `packed`'s sorted order) and the texels as float4, a plastic
// material's divided by its diffuse_probability
void texture_pack(const ky_scene* scene, const DScene* packed, const ky_texture* textures, int n, DTexSet* set, std::vector<float>* texels4);
uint64_t texture_digest(const ky_texture* textures, int n);   // 64 bits over every descriptor field and every texel; never 0 for n > 0, 0 for n == 0
uint64_t texture_fold(uint64_t hash, uint64_t digest);        // the scene hash a frame's header carries under a set of that digest: `hash` itself for 0
std::string texture_describe(const ky_texture* textures, int n);   // "2 textures (checker on material 3, 4 x 4 nearest image on material 1)"
int pack_scene(const ky_scene* in, DScene* out);
void pack_light_pick(const ky_scene* in, DLightPick* out);   // sample_single_light's power and spatial picks: the emitter proxies and the power rule's probabilities (a scene pack_scene accepts)
uint64_t scene_hash(const DScene& s);
bool scene_input(const ky_scene* in, std::vector<unsigned char>& out, uint64_t& hash);

// ---- the fp64 smallpt kernels' host side ----
constexpr int KY_SP_MAX_SPHERES = 32;   // == kysp::SP_MAX_SPHERES (ky_launch.hip asserts it)
int smallpt_check(const ky_smallpt_sphere* spheres, int n, const ky_smallpt_params* p);

// ---- launch policies (each has an environment variable and a kyhip_set_* entry) ----
bool specialisation_enabled();
bool boxes_enabled();
bool screen_cull_enabled();
int shadow_queue_mode();
bool shadow_queue_wanted(const ky_scene* scene);
int blocks_per_cu_cap();
enum { KY_ENGINE_LANE = 0, KY_ENGINE_QUEUE = 1 };
int current_engine();

// ---- the host-film seam's CPU side ----
int cpus_granted();
int seam_threads();   // host threads of the banded add (kyhip_seam_threads)
void host_add_rows(float* __restrict__ film, size_t stride_px, const float* __restrict__ src, int width, int y0, int y1);
// A few parked host threads for the banded add (creating and joining threads per call cost 50-100 us of a 4 ms frame).  run(n, fn) calls
// fn(0) ... fn(n - 1), fn(0) on the caller; one job at a time (the callers hold a seam mutex anyway, this one serialises across devices).
class HostPool {
public:
    void run(int n, const std::function<void(int)>& fn);
private:
    void loop(int id);
    std::mutex job_m_, m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    int n_ = 0, pending_ = 0, n_threads_ = 0;
    pid_t pid_ = 0;
    unsigned long long generation_ = 0;
};
HostPool& host_pool();
// The seam mutexes of a call's device list, taken in ascending device order whatever order the list names them in (and once per device): two calls with
// overlapping lists cannot deadlock.  Never called while a context's enqueue mutex is held.
std::vector<std::unique_lock<std::mutex>> lock_seams(std::vector<std::pair<int, std::mutex*>> by_device);
}  // namespace kyh

// ---- run-time instantiations: the code cache (ky_jit.cpp) ----
namespace kyjit {
struct Code {   // one compiled instantiation
    std::vector<char> object;
    bool failed = false;
};
extern const char k_entry[];                       // the extern "C" name of every run-time instantiation's kernel
int mode();                                        // 0 off, 1 on (blocking: the first launch of a kind waits for its compile), 2 on, asynchronous
// the code object of render_kernel_body<args> from memory or disk, compiling it when neither has it.  wait = false: a missing object is
// compiled by a background thread and nullptr is returned until it is there (`*pending` says so); nullptr with !*pending: it cannot be had
// (kyhip_jit_status() says why)
const Code* get_code(const std::string& args, bool wait = true, bool* pending = nullptr);
uint64_t source_hash();
int set_mode(int m);                               // -> the previous mode
bool mode_by_default();                            // nobody chose the mode: it is default_mode()'s (the launch code then instantiates for fact-free / run-time-dispatched picks only)
std::string status();
int failures();                                    // compiles that failed so far in this process
// A frame that is rendered by several launches (kyhip_render_multi's shards) must not switch kernels in the middle: between frame_begin() and
// frame_end() the calling thread's non-blocking get_code() treats objects that were finished after frame_begin() as still pending.
void frame_begin();
void frame_end();
}  // namespace kyjit
