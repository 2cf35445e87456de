/*
 * kyhip.h -- C ABI of the MI355X (gfx950) path-tracing integrator that replaces the body of
 *            ky's `integrator_t::render()` for `path_tracing_iteration_t`.
 *
 * The reference (infancy/ky, one C++ translation unit) has no FFI layer; its seam for this hot
 * path is the C++ call
 *
 *     void integrator_t::render(scene_t* scene, sampler_t* sampler, film_t* film)   ky.cpp:3689
 *     virtual color_t integrator_t::Li(ray_t, scene_t*, sampler_t*)                 ky.cpp:3792
 *     std::unique_ptr<integrator_t> create_integrator(enum, depth, direct_sample)   ky.cpp:4621
 *
 * This header is what a binding for that seam would declare: plain structs, pointers and sizes,
 * no C++ / torch types.  Every entry point cites the reference interface it stands in for.
 * The library (libkyhip.so) owns all device memory it allocates; caller-owned buffers are only
 * read or accumulated into.  No entry point throws; all return 0 on success or a negative
 * ky_status, and kyhip_last_error() returns a thread-local message for the last failure.
 *
 * All arithmetic on the path is fp32 (ky.cpp:171-172).
 */
#ifndef KYHIP_H
#define KYHIP_H

#ifndef __HIPCC_RTC__   /* the library compiles this header at run time too (hiprtc: no system headers, the types are built in) */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define KYHIP_ABI_VERSION 4   /* 4 (round 5): + kyhip_jit_failures, kyhip_multi_status, kyhip_seam_threads, kyhip_film_alloc / _free; kyhip_set_jit mode 2 */

/* ------------------------------------------------------------------------------------------
 * Scene description: a flat restatement of what scene_t holds (ky.cpp:3535-3546) and what the
 * path reads from it (SURVEY.md 8(b) "Inputs read by the path").
 * ---------------------------------------------------------------------------------------- */

/* shape_t subclasses, ky.cpp:1100 (disk), 1165 (triangle), 1245 (rectangle), 1326 (sphere) */
typedef enum ky_shape_kind {
    KY_SHAPE_DISK      = 0,
    KY_SHAPE_TRIANGLE  = 1,
    KY_SHAPE_RECTANGLE = 2,
    KY_SHAPE_SPHERE    = 3
} ky_shape_kind;

typedef struct ky_shape {
    int32_t kind;      /* ky_shape_kind */
    float   p[4][3];   /* rectangle: p0..p3 (1318-1321); triangle: p0..p2 (1238-1240);
                          disk: p[0] = position_ (1159); sphere: p[0] = center_ (1516) */
    float   normal[3]; /* stored normal_ after flip_normal (1174-1176, 1256-1258), disk: normalize(normal) (1105); MUST be unit
                          length (the reference's constructors normalise it); KY_ERR_INVALID_VALUE otherwise */
    float   radius;    /* disk radius_ (1161), sphere radius_ (1517) */
} ky_shape;

/* material_t subclasses, ky.cpp:2579 (matte), 2596 (mirror), 2613 (glass), 2639 (plastic) */
typedef enum ky_material_kind {
    KY_MATERIAL_MATTE   = 0,
    KY_MATERIAL_MIRROR  = 1,
    KY_MATERIAL_GLASS   = 2,
    KY_MATERIAL_PLASTIC = 3
} ky_material_kind;

typedef struct ky_material {
    int32_t kind;                 /* ky_material_kind */
    float   color0[3];            /* matte diffuse_color_ / mirror specular_color_ / glass reflection_color_ / plastic diffuse_color_ */
    float   color1[3];            /* glass transmission_color_ / plastic specular_color_ */
    float   eta;                  /* glass eta_ (2634); the outside index is 1 (2630) */
    float   exponent;             /* plastic exponent_ (2677) */
    float   diffuse_probability;  /* plastic diffuse_probility_  = lum(Kd)/(lum(Kd)+lum(Ks))   (2653-2657) */
    float   specular_probability; /* plastic specular_probility_ = lum(Ks)/(lum(Kd)+lum(Ks))   (2658) */
} ky_material;

/* light_t subclasses, ky.cpp:2810 (point), 2868 (direction), 2923 (area), 2999 (environment) */
typedef enum ky_light_kind {
    KY_LIGHT_POINT       = 0,
    KY_LIGHT_DIRECTION   = 1,
    KY_LIGHT_AREA        = 2,
    KY_LIGHT_ENVIRONMENT = 3
} ky_light_kind;

typedef struct ky_light {
    int32_t kind;          /* ky_light_kind */
    int32_t shape;         /* area: index into ky_scene.shapes of the shape it SAMPLES (area_light_t::shape_, 2993).
                              May differ from the shape of the surface that carries the light (Veach lights 1/2, 3498-3499 vs 3525-3526) */
    float   color[3];      /* point intensity_ / direction irradiance_ / area radiance_ / environment radiance_ */
    float   position[3];   /* point: world_position_ (2802) */
    float   direction[3];  /* direction: normalized world_direction_ (2874) */
    float   world_radius;  /* direction / environment: world_radius_ set by preprocess (3555-3574) */
} ky_light;

/* surface_t, ky.cpp:3071-3075 */
typedef struct ky_surface {
    int32_t shape;       /* index into shapes */
    int32_t material;    /* index into materials */
    int32_t area_light;  /* index into lights, or -1 (nullptr) */
} ky_surface;

/* camera_t members after its constructor ran, ky.cpp:1900-1905 */
typedef struct ky_camera {
    float position[3];
    float front[3];       /* normalized */
    float right[3];       /* scaled by tan(fov/2) * aspect (1878) */
    float up[3];          /* scaled by tan(fov/2)          (1879) */
    float resolution[2];
} ky_camera;

typedef struct ky_scene {
    const ky_shape*    shapes;    int32_t shape_count;
    const ky_material* materials; int32_t material_count;
    const ky_light*    lights;    int32_t light_count;     /* light_list_, in order (3541) */
    const ky_surface*  surfaces;  int32_t surface_count;   /* surface_list_, in order: order decides ties (3177) */
    int32_t            environment_light;                  /* index into lights of environment_light_ (3542), or -1 */
    ky_camera          camera;
} ky_scene;

/* Hard limits of the device path (the scene lives in on-chip memory). */
#define KYHIP_MAX_SHAPES    256
#define KYHIP_MAX_SURFACES  256
#define KYHIP_MAX_MATERIALS 64
#define KYHIP_MAX_LIGHTS    16

/* ------------------------------------------------------------------------------------------
 * Render parameters.
 * ---------------------------------------------------------------------------------------- */

/* integrator_enum_t values that have a device path (ky.cpp:3625-3654). */
typedef enum ky_integrator_kind {
    KY_INTEGRATOR_POSITION               = 0,  /* debug_integrator_t, 4112 */
    KY_INTEGRATOR_NORMAL                 = 1,  /* debug_integrator_t, 4114 */
    KY_INTEGRATOR_BASECOLOR              = 2,  /* debug_integrator_t, 4116 */
    KY_INTEGRATOR_DIRECT_LIGHTING        = 6,  /* direct_lighting_t, 4125 */
    KY_INTEGRATOR_SIMPLE_PATH_TRACING_RECURSION   = 8,   /* simple_path_tracing_recursion_t, 4191 (BSDF sampling only) */
    KY_INTEGRATOR_PATH_TRACING_RECURSION          = 9,   /* path_tracing_recursion_t, 4305 */
    KY_INTEGRATOR_PATH_TRACING_RECURSION_DEFERED  = 10,  /* path_tracing_recursion_defered_t, 4409 */
    KY_INTEGRATOR_PATH_TRACING_ITERATION = 11  /* path_tracing_iteration_t, 4523 -- the hot path */
} ky_integrator_kind;

/* direct_sample_enum_t (ky.cpp:3608-3623).  Matched by exact value (3840-3862). */
typedef enum ky_direct_sample {
    KY_DIRECT_IDLE      = 0,
    KY_DIRECT_SINGLE_LIGHT = 1,      /* flag (sample_single_light, 3612): ONE light per vertex, picked uniformly, its estimate divided by the pick
                                        probability (3813-3832).  Accepted only as KY_DIRECT_SINGLE_BOTH_MIS: the reference's function is fixed to both_mis */
    KY_DIRECT_BSDF      = 4,
    KY_DIRECT_LIGHT     = 8,
    KY_DIRECT_BSDF_MIS  = 16,
    KY_DIRECT_LIGHT_MIS = 32,
    KY_DIRECT_BOTH_MIS  = 48,
    KY_DIRECT_SINGLE_BOTH_MIS = 49,  /* KY_DIRECT_SINGLE_LIGHT | KY_DIRECT_BOTH_MIS */
    /* How sample_single_light picks its light: two flags on free bits of the reference's enum, which marks the spot `// TODO: power based, spatial based` (3805,
       3821).  Accepted only on KY_DIRECT_SINGLE_BOTH_MIS, one at a time; every other value that carries one is refused with KY_ERR_INVALID_VALUE.
       The picked light's estimate is divided by its probability p[li] = a / n + (1 - a) w[li] / W, a = 1/4 the share of the uniform pick (so the estimate stays
       unbiased whatever the weights, and p = 1 / n when they are all zero), n the light count, W the sum of the weights w:
         power    w = the light's power: pi e A for an area light (e the luminance of its colour, A the sampled shape's area), 4 pi e for a point light,
                  pi R^2 e for a directional one and pi^2 R^2 e for the environment (R = world_radius);
         spatial  w = the sum over the light's emitter proxies of clamp(e Om m, 0, 1e30) at the vertex (NaN counts as 0): Om the solid angle of the proxy seen
                  from the vertex -- a sphere's cone, a planar shape's A cos_l / max(d^2, r^2) on its emitting side, 1 / d^2 for a point light, 1 for a directional
                  one --, m the material's response towards it: a cosine that a lamp straddling the horizon keeps, c = clamp(N.om + sin_t, 1/64, 1) (the floor keeps the weights of a vertex with every lamp below its horizon off the rounding of that sum), times, for a
                  plastic material, Kd_lum / pi + Ks_lum min(Nn t^exponent, 1 / Om) with the Phong lobe evaluated at the point of the lamp nearest the mirror
                  direction.  The environment's w = e (Kd_lum + Ks_lum).  DESIGN.md section 3, "One light per vertex", has the definition operation by operation.
       A proxy is the shape a light samples, and one more per carrier surface of another shape (kyhip_scene_light_pick lists them).
       A scene with one light renders the film of 49 bit for bit under either rule. */
    KY_DIRECT_PICK_POWER      = 64,
    KY_DIRECT_PICK_SPATIAL    = 128,
    KY_DIRECT_SINGLE_POWER    = 113, /* KY_DIRECT_SINGLE_BOTH_MIS | KY_DIRECT_PICK_POWER */
    KY_DIRECT_SINGLE_SPATIAL  = 177  /* KY_DIRECT_SINGLE_BOTH_MIS | KY_DIRECT_PICK_SPATIAL */
} ky_direct_sample;

/* sampler_t subclasses that can be instantiated (ky.cpp:922, 949). */
typedef enum ky_sampler_kind {
    KY_SAMPLER_DEBUG  = 0,  /* debug_sampler_t: every number 0.5, camera sample = pixel centre (933-946) */
    KY_SAMPLER_RANDOM = 1,  /* random_sampler_t semantics (uniform [0,1) fp32) on a counter-based generator
                               keyed (seed, pixel, sample, dimension); see DESIGN.md "Random numbers" */
    KY_SAMPLER_STRATIFIED = 2   /* stratified_sampler_t, which ky.cpp:977 declares and leaves a stub: the camera sample multi-jittered, the next
                               KYHIP_STRATIFIED_DIMS - 2 draws of a sample Latin-hypercube strata over the pixel's samples_per_pixel samples, every later
                               draw the random sampler's; samples_per_pixel <= 2^24.  DESIGN.md "Random numbers" has the definition */
} ky_sampler_kind;
#define KYHIP_STRATIFIED_DIMS 16   /* the draws of a camera sample that KY_SAMPLER_STRATIFIED stratifies (the camera's two among them) */

/* Pixel reconstruction filters (the reference's empty `#pragma region filter`, ky.cpp:1525-1527), by filter importance sampling: the camera
   sample's offset from its pixel's corner is drawn from the filter's density, 0.5 + F^-1(u) per axis, and the sample still lands in its own pixel with weight 1.  All
   kinds are separable, one 1-D law for x and y, with support [-radius, radius] in pixels around the pixel's centre.  The filter that is rendered is the TABLE's
   (kyhip_filter_table): a piecewise-linear inverse CDF over KYHIP_FILTER_TABLE intervals of u, which strays from the analytic CDF by at most 1.8e-3 for the kinds
   below (DESIGN.md section 11 has the figures); the tent's inverse is closed and reads no table.  A filter travels beside ky_render_params, never inside them. */
typedef enum ky_filter_kind {
    KY_FILTER_BOX             = 0,  /* today's camera sample: uniform over the pixel.  The radius is ignored */
    KY_FILTER_TENT            = 1,  /* density proportional to radius - |x| */
    KY_FILTER_GAUSSIAN        = 2,  /* param = sigma in pixels; density exp(-x^2 / 2 sigma^2) - exp(-radius^2 / 2 sigma^2) on |x| < radius, as in pbrt */
    KY_FILTER_BLACKMAN_HARRIS = 3   /* the four-term window 0.35875 + 0.48829 cos(pi x / R) + 0.14128 cos(2 pi x / R) + 0.01168 cos(3 pi x / R) over [-R, R] */
} ky_filter_kind;
#define KYHIP_FILTER_MAX_RADIUS 4   /* 0.5 <= radius <= 4 */
#define KYHIP_FILTER_TABLE 256      /* intervals of the inverse-CDF table: KYHIP_FILTER_TABLE + 1 floats */
typedef struct ky_pixel_filter {
    int32_t kind;       /* ky_filter_kind */
    float   radius;     /* pixels */
    float   param;      /* KY_FILTER_GAUSSIAN: sigma; ignored by the other kinds */
    int32_t reserved;   /* 0 */
} ky_pixel_filter;

/* A thin lens in front of the camera (the reference's commented-out `point2_t p_lens` of camera_sample_t, ky.cpp:870-874, and `// sample_ray(...)`, 1894; DESIGN.md
   section 12): a camera sample leaves from a point of a disk of `radius` around the camera's position, in the plane of `right` and `up`, towards the point its
   pinhole ray meets on the plane at depth `focus_distance` along `front`.  What lies on that plane is sharp; everything else is blurred by a disk that grows with
   radius * |1 / focus_distance - 1 / depth|.  radius 0 is the pinhole camera.  A lens travels beside ky_render_params, like a pixel filter: never inside
   ky_camera, ky_scene or the params. */
typedef struct ky_lens {
    float   radius;           /* aperture radius, world units; 0: the pinhole */
    float   focus_distance;   /* depth of the focus plane along `front`, world units; looked at only when radius > 0 */
    int32_t reserved[2];      /* 0 */
} ky_lens;

/* Textures (the reference's empty `#pragma region texture` / `// TODO class texture_t`, ky.cpp:2559-2564): a texture replaces the colour
   color0 of one material of the scene -- a matte material's diffuse_color_, a mirror's specular_color_, a plastic material's diffuse_color_ (its lobe probabilities
   stay the struct's) -- by a function of the hit point's surface coordinates (u, v).  Glass is refused.  A texture set travels beside ky_scene, as a filter and a
   lens travel beside the params: never inside ky_material or ky_scene.
   (u, v) of a hit point p: rectangle u = (p - p0).(p1 - p0) / |p1 - p0|^2, v = (p - p0).(p3 - p0) / |p3 - p0|^2 (for a quad that is no parallelogram simply the
   definition); triangle: the barycentric pair of p = p0 + u (p1 - p0) + v (p2 - p0); disk u = 0.5 + (p - c).s / 2r, v = 0.5 + (p - c).t / 2r with (s, t) of
   frame_t(normal); sphere d = (p - c) / r, u = 0.5 + atan2(d.z, d.x) / 2 pi, v = acos(clamp(d.y, -1, 1)) / pi.
   Checker: colour a where floor(u') + floor(v') is even, b where it is odd.  Image: u', v' are wrapped first -- repeat x - floor(x), clamp to [0, 1) --; nearest
   reads texel (min(int(u' W), W - 1), min(int(v' H), H - 1)); bilinear is pbrt's, sampled at u' W - 0.5, its four neighbours wrapped or clamped by the same rule. */
#define KYHIP_MAX_TEXTURES 16
#define KYHIP_MAX_TEXTURE_SIZE 4096          /* an image dimension */
#define KYHIP_MAX_TEXELS (1 << 24)           /* over the set's images */
#define KYHIP_MAX_TEXTURE_SCALE (1 << 20)    /* |scale| and |offset|, each component */
typedef enum ky_texture_kind { KY_TEXTURE_CHECKER = 0, KY_TEXTURE_IMAGE = 1 } ky_texture_kind;
typedef enum ky_texture_flags { KY_TEXTURE_BILINEAR = 1 /* else nearest */, KY_TEXTURE_CLAMP = 2 /* else repeat */ } ky_texture_flags;
typedef struct ky_texture {
    int32_t kind, material;      /* the ky_scene material whose color0 this texture replaces; at most one texture per material */
    int32_t flags, reserved;     /* image only; reserved 0 */
    float   scale[2], offset[2]; /* (u', v') = (scale[0] u + offset[0], scale[1] v + offset[1]) */
    float   a[3], b[3];          /* checker: colour where floor(u') + floor(v') is even / odd */
    int32_t width, height;       /* image: 1 .. 4096 each */
    const float* texels;         /* image: height rows of width RGB triples, row 0 at v' = 0; finite, >= 0 */
} ky_texture;

typedef struct ky_render_params {
    int32_t  integrator;         /* ky_integrator_kind */
    int32_t  max_path_depth;     /* path_integrator_t::max_path_depth_ (4182) */
    int32_t  direct_sample;      /* ky_direct_sample, path_integrator_t::direct_sample_enum_ (4183) */
    int32_t  samples_per_pixel;  /* sampler_t::samples_per_pixel_ (918) */
    int32_t  sampler;            /* ky_sampler_kind */
    uint32_t seed;               /* rng_t seed, default 1234 (833) */
    int32_t  width, height;      /* film->get_resolution() (3692): the pixel loop bounds */
    /* Image-tile sharding.  The film is cut into tile_w x tile_h tiles; with
       tiles_x = ceil(width / tile_w), tile number t lies in tile row t / tiles_x at tile column
       (t % tiles_x + t / tiles_x) % tiles_x -- row-major with every row rotated by its index, so that
       an interleaved shard is a comb of diagonals even when tiles_x is a multiple of tile_step.
       This call renders tiles tile_first, tile_first+tile_step, ...  A single-GPU render uses
       tile_first = 0, tile_step = 1.  tile_w and tile_h must be multiples of 8. */
    int32_t  tile_w, tile_h;
    int32_t  tile_first, tile_step;
} ky_render_params;

typedef enum ky_status {
    KY_OK                = 0,
    KY_ERR_INVALID_VALUE = -1,  /* bad argument, unknown enum (create_integrator returns nullptr, 4638;
                                   sample_all_light leaves the std::function empty, 3860) */
    KY_ERR_LIMIT         = -2,  /* scene larger than the KYHIP_MAX_* limits, or a frame whose work items / pixels do not fit
                                   the device code's 32-bit indices (e.g. 4096 x 4096 at more than ~1.8e6 spp) */
    KY_ERR_DEVICE        = -3,  /* HIP runtime error (message has the hipError string) */
    KY_ERR_NO_DEVICE     = -4   /* no gfx950 device visible: the product has no CPU fallback */
} ky_status;

const char* kyhip_last_error(void);
/* Selects the render kernel for path_tracing_iteration_t: 0 = lane engine (default: one lane walks one path, state in
   registers), 1 = queue engine (experimental: path state in LDS, one queue per path state, wavefronts take full batches
   from the fullest queue -- ky_amd/csrc/ky_queue.hpp).  Both run the same per-sample arithmetic and random streams; the
   images differ by float summation order only.  The default is read from the environment variable KYHIP_ENGINE
   ("lane" / "queue").  Returns the previous engine.  Not part of the reference's interface: a tuning knob. */
int         kyhip_set_engine(int engine);
/* Specialised kernel instantiations -- a scene lit by exactly one rectangle area light runs a both_mis kernel compiled without the
   other light kinds, the environment term, the lights loop and the other light shapes' sampling; each of the other five
   direct-lighting strategies of the iterative integrator has its own kernel instead of the run-time-dispatched one -- on = 1 (default;
   environment variable KYHIP_SPECIALISE=0 turns them off) / off = 0.  The image does not depend on it (to the last bit of a pixel: the
   compiler contracts a few multiply-adds differently once code around them is gone).  Returns the previous setting.
   A tuning knob, like kyhip_set_engine. */
int         kyhip_set_specialisation(int on);
/* Boxes: axis-aligned rectangles that are whole faces of a common axis-aligned box -- the five walls of a Cornell box, its lamp housing -- are tested by the
   nearest-hit traversal with ONE slab test per box instead of face by face (kernels with the fact KY_FEAT_BOXES; kyhip_scene_boxes says which surfaces).  The slab
   test's hit distance differs from the rectangle test's by up to 15 units in the last place, so unlike the switch above this one moves an image beyond its last bit
   (tests/test_boxes.py: by how much).  on = 1 (default; environment variable KYHIP_BOXES=0 turns it off) / off = 0; needs kyhip_set_specialisation(1).  Returns the
   previous setting.  A tuning knob. */
int         kyhip_set_boxes(int on);
/* The screen cull: when a scene is packed the library projects the world bound of its surfaces through the scene's camera and keeps the pixel
   rectangle around it (kyhip_scene_screen_bound); the lane engine's render kernels take no work for an 8 x 8 pixel block outside it -- every camera ray of such a
   block misses every surface, and without an environment light a miss adds nothing.  The image does not depend on it, to the bit.  on = 1 (default; environment
   variable KYHIP_SCREEN_CULL=0 turns it off) / off = 0: the rectangle is the whole frame; -1 (any other value) only queries.  Returns the previous setting.  A tuning knob. */
int         kyhip_set_screen_cull(int on);
/* Deferred shadow rays (the render kernels' QUEUE instantiations: light samples wait on a per-wavefront stack until 64 of them fill a traversal).
   mode -1 (default): by the scene -- when its sphere area lights outnumber its point / directional lights by five or more (create_mis_scene's five
   lamps; measured crossing, tools/queue_policy.py); 0: never; 1: for every scene with lights.  The environment variable KYHIP_SHADOW_QUEUE = 0 / 1 sets the
   initial mode.  The image does not depend on it beyond float summation order (contributions enter the film in fixed point either way).  Returns the
   previous mode.  A tuning knob, like kyhip_set_engine. */
int         kyhip_set_shadow_queue(int mode);
/* Run-time instantiations.  The render kernel is a template over (sampler, strategy, integrator, deferred shadow rays, general shapes, scene
   facts, table size); the library ships a fixed table of instantiations and picks the nearest one per launch.  mode 1: a launch whose exact
   combination -- with ALL of its scene's facts -- is not in the table gets its own kernel, compiled from the library's embedded source by the
   ROCm compiler (a child process: $KYHIP_HIPCC, default /opt/rocm/bin/hipcc) on first use (a few seconds, blocking that launch; afterwards a
   code object in memory and under $KYHIP_CACHE_DIR, default ~/.cache/kyhip).
   mode 2 (round 5): the same without the wait -- a missing instantiation is compiled by a background thread while the table's kernel renders, and
   launches switch to it once it is there; all shards of one kyhip_render_multi call use one kernel.  WHEN a process switches is a matter of timing,
   and table and own kernel differ in the last bit of a pixel: use mode 1 where frames must be reproducible bit for bit (the ranks of a multi-process
   job: ky_amd/dist.py refuses mode 2 there).
   mode 0: the table only.  The image does not depend on the mode beyond the last bit of a pixel (like kyhip_set_specialisation).
   The mode a process STARTS in (round 6; rounds 4-5: 0): the environment variable KYHIP_JIT = 0 / 1 / 2 if set; otherwise 2 when this process can run instantiations
   without surprising anyone -- a compiler at a known path, no profiler attached, a single-process job (WORLD_SIZE unset or 1) -- and 0 when not; kyhip_jit_status()
   says which and why.  kyhip_last_kernel() names the kernel a launch ran on and adds "[its own instantiation ... is being compiled ...]" / "[... is unavailable: ...]"
   when that was the table's kernel for the time being.  kyhip_set_jit(-1) returns the mode without changing it.  If no compiler is found or a compile fails, the table's kernel runs and kyhip_jit_status() says why
   (kyhip_jit_failures() counts such compiles: a multi-rank job checks it, because a rank that fell back renders its shards on another kernel).
   The compiler is started with posix_spawn (argv array, no shell) and an environment without LD_PRELOAD / profiler variables; in a process that
   is itself being profiled nothing is compiled ("stands down under a profiler").  Processes share the cache directory safely (flock, write-once).
   Returns the previous mode.  A tuning knob, not part of the reference's interface. */
int         kyhip_set_jit(int mode);
const char* kyhip_jit_status(void);
int         kyhip_jit_failures(void);
/* Host only (no GPU needed): compiles -- or fetches from the cache -- the instantiation named by a C++ expression such as
   "render_kernel<false, 48, false, false, 135, 11, false>" and returns the size of its gfx950 code object, or a negative ky_status. */
int64_t     kyhip_jit_compile(const char* name_expression);
/* 64 bits over the text of the device headers the render kernels are compiled from (ky_device.hpp, ky_render.hpp, this file) and their compile flags:
   what identifies the KERNELS of a build (host-side changes do not move it).  profiles/valu.json carries the hash of the build its counters were
   measured on, and bench.py withholds those counters when it runs another. */
uint64_t    kyhip_kernel_source_hash(void);
int         kyhip_abi_version(void);
int         kyhip_device_count(void);

/* Number of tiles this (first, step) shard owns, and the float count of its compact tile buffer
   (tiles * tile_w * tile_h * 3).  Pure host arithmetic. */
int64_t kyhip_shard_tile_count(const ky_render_params* params);
int64_t kyhip_shard_float_count(const ky_render_params* params);
/* The film's range rule (DESIGN.md "Film").  A launch adds each pixel's radiance to a signed 32.32 fixed-point word in terms (chunk sums, samples,
   deferred shadow rays); N is the most terms one word can receive in a launch of `params` on a scene of n_lights lights, on engine 0 (lane) or 1
   (queue; path_tracing_iteration only, other integrators run on the lane engine), with deferred shadow rays (deferred = 1) or without; n_lights
   0 .. KYHIP_MAX_LIGHTS.  Every term at or beyond +-T, T = min(2e9, 2^31 / N) as a float rounded down, sets the pixel's +inf / -inf flag instead of
   being added, so the word never wraps; *limit (may be NULL) receives T.  Returns N, or KY_ERR_LIMIT when T would be below 1.  kyhip_render and its
   device variants refuse with KY_ERR_LIMIT, before any device work, a launch whose count with deferred shadow rays (the largest of its counts) is
   such.  A single-light strategy (49, 113, 177) counts both_mis's terms -- it adds fewer --, but one of its terms is up to n / a times one light's estimate
   (n the light count, a = 1/4 the uniform share of the power and spatial picks; n times under 49): the counts are the same for all three, the terms that reach
   T are not.  Pure host arithmetic. */
int64_t kyhip_film_term_limit(const ky_render_params* params, int n_lights, int engine, int deferred, float* limit);

/*
 * kyhip_render -- drop-in for integrator_t::render(scene, sampler, film) (ky.cpp:3689-3729).
 *   film_rgb           caller-owned HOST buffer of film_t::pixels_ layout (AoS RGB fp32, row-major,
 *                      y down, ky.cpp:1574); the library ADDS clamp01(mean radiance) per pixel,
 *                      exactly like film_t::add_color (1586-1590, 3726).
 *   film_row_stride_px row stride in pixels (>= params->width), and film_rgb may point at the
 *                      first pixel of a sub-film, so a film_grid_t cell can be the target (1817-1822).
 * Renders the shard named by params (all tiles when tile_first = 0, tile_step = 1) on `device`.
 * Blocking.
 */
int kyhip_render(int device, const ky_scene* scene, const ky_render_params* params,
                 float* film_rgb, size_t film_row_stride_px);

/*
 * Light classes -- lighting_enum_t (ky.cpp:3591-3603), the argument of path_tracing_recursion_defered_t (4415) behind render_lighting_enum (4907-4935).
 * A contribution to a sample's radiance belongs to the class given by k, the number of scattering vertices between the camera and the emitter (the
 * expansion at 3582-3589): emit k = 0, direct k = 1, indirect k >= 2.  For path_tracing_iteration_t (11) and path_tracing_recursion_defered_t (10):
 * emission or environment radiance added at a vertex with bounces == b has k = b (b >= 1 only after a delta bounce), the light estimate at that vertex
 * k = b + 1 -- so a lamp seen in one mirror is direct light, in two indirect.  direct_lighting_t (6): emission k = 0, its estimate k = 1, nothing else.
 * A masked render adds to the film only the contributions whose class bit is set; the sample is otherwise the unmasked one -- its random numbers,
 * their order, every path decision, the roulette -- and clamp01 applies to the masked mean.  So per camera sample the three classes add up to
 * the unmasked radiance, and lighting 1 / 3 are what the unmasked render gives at max_path_depth 0 / 1.
 * The scattering bits diffuse = 8 and specular = 16 have no meaning in the reference: accepted both set or both clear (31 = lighting_enum_t::all = 7).
 *
 * kyhip_render_lighting: kyhip_render in every respect (it adds, the shard named by params, pinned films) for the classes of `lighting`.  With 7 / 31
 *   it IS kyhip_render: the same kernel, the same film.  A mask that selects nothing the launch can produce (indirect alone at depth <= 1 or on
 *   integrator 6) adds nothing and returns KY_OK.  KY_ERR_INVALID_VALUE, before any device work and with the film untouched: lighting 0, a bit above
 *   31, exactly one of 8 / 16; any mask but all on integrators 0, 1, 2, 8, 9, whose terms are not one class each.
 *   kyhip_last_kernel names the form of a masked launch behind the kernel: ", lighting 3: depth 1", ", lighting 4: emission at the first vertex and
 *   its direct light dropped".  The queue engine has no masked form: such a launch runs on the lane engine, and the name says so.
 * kyhip_lighting_plan: how that launch is run (host arithmetic, no device).  *effective_depth: the max_path_depth it renders at -- min(depth, 1)
 *   without the indirect class, 0 with emit alone: paths end where what they could still add is masked out --, -1: nothing is launched.  *dropped:
 *   what is left for the kernel, bit 1 no emission at the first vertex (bounces == 0), bit 2 no k = 1 term (the first vertex's light estimate,
 *   whose random numbers are still drawn, and emission at bounces == 1).  Either pointer may be NULL.
 * kyhip_kat_li_lighting: kyhip_kat_li for the samples of that launch.
 */
typedef enum ky_lighting {
    KY_LIGHTING_EMIT     = 1,
    KY_LIGHTING_DIRECT   = 2,
    KY_LIGHTING_INDIRECT = 4,
    KY_LIGHTING_ALL      = 7
} ky_lighting;
int kyhip_render_lighting(int device, const ky_scene* scene, const ky_render_params* params, int lighting,
                          float* film_rgb, size_t film_row_stride_px);
int kyhip_lighting_plan(const ky_render_params* params, int lighting, int* effective_depth, int* dropped);
/* The refusals alone, without render params (host arithmetic): KY_OK when `integrator` (ky_integrator_kind) renders the classes of `lighting`. */
int kyhip_lighting_check(int integrator, int lighting);
int kyhip_kat_li_lighting(int device, const ky_scene* scene, const ky_render_params* params, int lighting,
                          int x, int y, int s0, int n, float* out3);

/*
 * Device-resident variants used by the multi-GPU path and by bench.py (inputs and outputs stay in
 * HBM; nothing crosses PCIe inside the timed region).
 *
 * kyhip_render_tiles_device: renders this shard's tiles into `d_tiles`, a DEVICE buffer of
 *   kyhip_shard_float_count() floats laid out [local_tile][ty][tx][rgb]; every pixel is written
 *   with clamp01(mean radiance) (pixels of edge tiles outside the film are written as 0).
 *   `stream` is a hipStream_t (0 = default stream).  Asynchronous w.r.t. the host.
 *   `d_workspace`/`workspace_bytes`: device scratch of at least kyhip_workspace_bytes(); may be
 *   NULL, in which case the library allocates and caches one per device.
 *
 * kyhip_film_add_tiles_device: the de-interleave step after the gather: adds the compact tiles of
 *   shard (tile_first, tile_step) into a DEVICE film (same layout as kyhip_render's film_rgb).
 *
 * Streams: what a launch writes (work counter, accumulator workspace, timing events, shadow-ray stacks) belongs to the STREAM it is
 *   enqueued on -- the library keeps one such state per (device, stream), up to eight per device -- so calls on one stream execute in
 *   stream order and calls on different streams share nothing and may overlap on the device: a frame's kernel starts on the compute
 *   units the previous frame's persistent kernel is draining from (ky_amd/dist.py alternates two streams).  The packed scene is cached
 *   per device by content (eight slots): alternating between a few scenes uploads each once.  Calls for different devices are
 *   independent (one lock per device).
 *
 * kyhip_film_add_gathered_device: the same de-interleave for ALL shards of a frame in one kernel.  The frame described
 *   by params (tile_first, tile_step) was rendered as `world` shards -- shard r = (tile_first + r * tile_step,
 *   tile_step * world) -- whose compact tile buffers lie at d_gathered + r * rank_stride_floats (the layout a gather
 *   collective leaves on the root); rank_stride_floats >= kyhip_shard_float_count() of shard 0.
 */
size_t kyhip_workspace_bytes(const ky_render_params* params);
int kyhip_render_tiles_device(int device, const ky_scene* scene, const ky_render_params* params,
                              float* d_tiles, void* d_workspace, size_t workspace_bytes, void* stream);
int kyhip_film_add_tiles_device(int device, const ky_render_params* params, const float* d_tiles,
                                float* d_film_rgb, size_t film_row_stride_px, void* stream);
int kyhip_film_add_gathered_device(int device, const ky_render_params* params, int world, const float* d_gathered,
                                   size_t rank_stride_floats, float* d_film_rgb, size_t film_row_stride_px, void* stream);

/*
 * kyhip_render_multi -- integrator_t::render(scene, sampler, film) on a LIST of devices of one node.  The reference
 * spreads render()'s pixel loop over all cores itself (`#pragma omp parallel for schedule(dynamic, 1)`, ky.cpp:3696-3699);
 * here the frame's tiles are interleaved over the listed GPUs: shard i = (tile_first + i * tile_step, tile_step * n_devices)
 * renders on devices[i] on that device's own stream, all shards concurrently and without communication; the tile buffers
 * are then gathered on devices[0] (one peer copy per remote shard over xGMI), de-interleaved by one kernel and ADDED into
 * the caller's host film exactly like kyhip_render.  A device may be listed more than once (its shards then run one after
 * the other).  The image does not depend on the device list: it is bit-identical to kyhip_render's.  Blocking.
 * kyhip_render(device, ...) is kyhip_render_multi(&device, 1, ...).
 * kyhip_multi_status(root): how the last kyhip_render_multi call whose devices[0] was `root` gathered its shards, one clause per shard -- "local" (rendered on
 *   the root), "peer" (hipMemcpyPeerAsync over a peer mapping that hipDeviceEnablePeerAccess set up: a direct xGMI copy; the mapping is made ONCE per
 *   (root, device) pair and remembered) or "staged" (the runtime reports no peer access: the same call, which the runtime then stages through the host) --
 *   and how many host threads added the film.  Valid until the next call on this thread.
 * kyhip_film_alloc(bytes) / kyhip_film_free: film memory the GPU can add to IN PLACE -- pinned, mapped host memory (hipHostMalloc).  kyhip_render /
 *   kyhip_render_multi recognise such a film (or one the caller registered with hipHostRegister) and let the root GPU's add kernel read and write it over
 *   PCIe: no staging copy, no host pass, no dependence on the CPUs the process is granted.  Any other film (malloc, new[], numpy) takes the banded
 *   download + host add.  The images are bit-identical.  NULL without a device: callers fall back to ordinary memory (ky.hpp's film_t does).
 * kyhip_seam_threads(): host threads the banded add of the next kyhip_render / kyhip_render_multi call will use (the caller's plus parked ones): the CPUs
 *   the process is granted (affinity mask and cgroup quota), at most four (environment variable KYHIP_SEAM_THREADS overrides).  A pinned film uses none.
 */
void*       kyhip_film_alloc(size_t bytes);
void        kyhip_film_free(void* film);
const char* kyhip_multi_status(int root_device);
int kyhip_seam_threads(void);
int kyhip_render_multi(const int* devices, int n_devices, const ky_scene* scene, const ky_render_params* params,
                       float* film_rgb, size_t film_row_stride_px);

/*
 * A frame rendered in passes -- integrator_t::render (ky.cpp:3689-3729) with the picture available, and the right to stop, after every pass; the
 * reference only reports how far it is, "rendering... N spp, x%" per row (3703).
 * A pixel's samples are cut into chunks by a schedule that depends on samples_per_pixel only, work items are queued chunk by chunk, samples are keyed by
 * their absolute index and a chunk's sum enters an integer accumulator: so the frame's chunks may be rendered by any number of launches, in order, and a
 * complete frame IS kyhip_render's film, bit for bit, however its passes were cut (DESIGN.md "Passes").  A frame owns its accumulators (on `device`);
 * kyhip_render* calls and other frames between its passes neither disturb it nor are disturbed.  All passes of a frame run the kernel its first pass
 * took.  The queue engine renders no passes: a frame runs on the lane engine, and kyhip_last_kernel says so.  Calls on one frame must not overlap.
 *
 * kyhip_pass_boundaries: the sample counts at which a pass of an `spp`-sample frame can end -- the ends of the chunks of its schedule, ascending, the
 *   last is spp.  Writes min(n, count) values to `bounds` (may be NULL with n = 0); returns count, or KY_ERR_INVALID_VALUE for spp < 1 (or above 2^24,
 *   which no render accepts).  Pure host arithmetic.
 * kyhip_frame_begin: validates exactly as kyhip_render does (the same statuses, before any device work); params->samples_per_pixel is the frame's
 *   TOTAL, the shard named by params is the frame's.  The scene is copied: the caller's arrays need not outlive the call.  *out: the frame, with
 *   nothing rendered.
 * kyhip_frame_render: renders whole chunks until at least min_samples more samples per pixel are done or the frame is complete.  Blocking.
 *   *samples_done (may be NULL) receives the total done so far, always a value of kyhip_pass_boundaries (or 0).  On a complete frame: KY_OK, nothing
 *   is launched.  min_samples < 1: KY_ERR_INVALID_VALUE.  kyhip_last_kernel names the pass behind the kernel: ", pass: chunks 2..18 of 51, samples
 *   48..308 of 500".
 * kyhip_frame_samples: samples per pixel done so far and the frame's total (either pointer may be NULL).
 * kyhip_frame_resolve: ADDS clamp01(value) per pixel to a host film exactly like kyhip_render (a sub-film's first pixel and its row stride; a pinned
 *   film is added to in place by the GPU, any other film by the host).  normalise 0: value = sum / total -- for a complete frame this IS kyhip_render's
 *   film; normalise 1: value = sum / done, the picture so far (nothing is added while done == 0).  Pixels whose sums met NaN or +-inf or saturated
 *   resolve as they do in kyhip_render.  Does not change the frame: it may be resolved any number of times and rendered further.
 * kyhip_frame_state_bytes / _save / _load: a checkpoint -- a header (a magic number, kyhip_kernel_source_hash, the params, a hash of the packed scene,
 *   the samples done, the shard's pixel count), then the accumulators and the flag words.  kyhip_frame_load refuses with KY_ERR_INVALID_VALUE, the frame
 *   untouched, a buffer shorter than the state and a state whose header differs in any field but the samples done from what `f` was begun with (another
 *   seed, sample count, scene, film size, shard, or a library built from other kernel sources); otherwise `f` continues from the saved pass.
 * kyhip_frame_end: releases the frame (NULL is fine).
 */
typedef struct kyhip_frame kyhip_frame;   /* opaque */
int     kyhip_pass_boundaries(int spp, int* bounds, int n);
int     kyhip_frame_begin(int device, const ky_scene* scene, const ky_render_params* params, kyhip_frame** out);
int     kyhip_frame_render(kyhip_frame* f, int min_samples, int* samples_done);
int     kyhip_frame_samples(const kyhip_frame* f, int* done, int* total);
int     kyhip_frame_resolve(kyhip_frame* f, int normalise, float* film_rgb, size_t film_row_stride_px);
int64_t kyhip_frame_state_bytes(const kyhip_frame* f);
int     kyhip_frame_save(kyhip_frame* f, void* buf, size_t bytes);
int     kyhip_frame_load(kyhip_frame* f, const void* buf, size_t bytes);
void    kyhip_frame_end(kyhip_frame* f);

/*
 * A frame's noise estimate: when to stop (DESIGN.md "Noise").  A frame's accumulators change by whole chunks only, so the difference between them after two passes
 * is an exact batch sum of the pixel's samples; a frame that tracks noise keeps per pixel the luminance sum (color_t::luminance's weights, ky.cpp:249-255) at
 * its last pass and West's weighted sum of squares of the passes' batch means, 16 bytes, advanced by one film-sized kernel behind every pass.  The render
 * kernels know nothing of it and a tracking frame's film is the film of any other frame, bit for bit.  The estimate is weak where batch means are: the batches
 * are few and unequal (2 to 24 samples each), and a heavy-tailed pixel is under-estimated until a firefly lands in it.
 *
 * kyhip_frame_track_noise: only while nothing is rendered or loaded, else KY_ERR_INVALID_VALUE.  Tracking twice is fine.
 * kyhip_frame_noise: WRITES (does not add) width x height floats, y down, row_stride_px floats apart: per pixel of the frame's shard the standard error of its
 *   mean luminance so far in units of the film's white, sqrt(m2 / (batches - 1) / samples) / max(1, mean luminance) -- over-range pixels are scaled down because
 *   clamp01 hides their error.  +inf while the frame has fewer than two batches (passes); 0 for a pixel that met NaN or +-inf or saturated, whose resolved
 *   value the flag rules pin.  Pixels of other shards are left untouched.
 * kyhip_frame_noise_stats: over the shard's pixels inside the film -- their count, how many are flagged, how many of the others lie above `threshold`, the
 *   others' largest value and mean.  Deterministic: two calls return identical bytes.  threshold < 0 or NaN: KY_ERR_INVALID_VALUE.
 * kyhip_frame_render_until: passes of at least min_samples_per_pass until batches >= min_batches (a value >= 2, else KY_ERR_INVALID_VALUE) and
 *   above <= max_fraction_above * (pixels - flagged), or until the frame is complete; KY_OK either way, *out (the statistics behind the last pass) says which.
 *   At least one pass is rendered unless the frame is complete.  *samples_done may be NULL.
 * kyhip_frame_noise_ms: hipEvent durations of the last pass's update kernel and of the last map (+ statistics) kernels, negative where there was none.
 * Every argument is checked before any device work; the four calls on a frame that does not track return KY_ERR_INVALID_VALUE.
 * A tracking frame's checkpoint (kyhip_frame_state_bytes / _save / _load) carries a trailer behind the state described above: a magic number, the batch count
 *   and the samples done at the last update, then the per-pixel pairs.  kyhip_frame_load into a tracking frame refuses, the frame untouched, a state without
 *   a valid trailer or whose trailer stands at another sample count than its header; a frame that does not track saves today's bytes, accepts a longer buffer
 *   and ignores the trailer.
 */
typedef struct ky_noise_stats { int32_t batches, samples_done; int64_t pixels, flagged, above; float threshold, max; double mean; } ky_noise_stats;
int     kyhip_frame_track_noise(kyhip_frame* f);
int     kyhip_frame_noise(kyhip_frame* f, float* map, size_t row_stride_px);
int     kyhip_frame_noise_stats(kyhip_frame* f, float threshold, ky_noise_stats* out);
int     kyhip_frame_render_until(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass,
                                 int* samples_done, ky_noise_stats* out);
int     kyhip_frame_noise_ms(const kyhip_frame* f, float* update_ms, float* stats_ms);

/*
 * Adaptive sampling: a frame that retires clean pixel blocks between its passes (DESIGN.md "Adaptive").  The unit is the render kernels' work item, a block of
 * 8 x 8 pixels.  A block is live, or retired at the samples it had when it retired; a retired block is never rendered again, all live blocks stand at the same
 * sample count (the frame's front, what kyhip_frame_samples reports as done), and retirement happens only between passes and is final.  Blocks of a ragged edge
 * tile that have no pixel inside the film are retired at 0 samples from the start.  Every pass of such a frame runs a render kernel that reads its blocks from
 * the frame's list of live ones (kyhip_last_kernel: "... listed blocks ..., blocks: 9 of 24 live"); with nothing retired the film is kyhip_render's.
 * Caveat: a block that stops on the estimate of its own samples is biased towards the value it had when it looked clean.
 *
 * kyhip_frame_track_blocks: only while nothing is rendered or loaded, else KY_ERR_INVALID_VALUE; independent of kyhip_frame_track_noise (either order).  Twice is fine.
 * kyhip_frame_keep: `mask` is width x height bytes, y down, row_stride bytes apart; every live block none of whose pixels inside the film has a non-zero byte is
 *   retired (the reference's debug_area: go on rendering a part of the film only).  Needs no noise tracking.  NULL mask, row_stride < width: KY_ERR_INVALID_VALUE.
 * kyhip_frame_retire_noisy: one application of the retire rule to the live blocks as the frame stands: a block retires when batches >= min_batches and
 *   above <= max_fraction_above * counted, over its pixels inside the film that are not flagged (kyhip_frame_render_until's comparison, per block).  Needs noise
 *   tracking; threshold, max_fraction_above and min_batches are checked as kyhip_frame_render_until checks them.  *out: the statistics behind it.
 * kyhip_frame_render_adaptive: kyhip_frame_render(min_samples_per_pass) then kyhip_frame_retire_noisy, until no block is live or the front has reached the
 *   total; KY_OK either way, *out says which.  *samples_done (may be NULL): the front.
 * kyhip_frame_sample_map: WRITES width x height int32, y down, row_stride_px apart: per pixel of the frame's shard the samples its block has received.  Pixels
 *   of other shards are left untouched.
 * kyhip_frame_block_stats: blocks (padding included) and how many are live, passes rendered (saved and loaded with the frame's state), the front, the smallest and largest per-pixel sample count, the
 *   shard's pixels inside the film and the pixel-samples rendered so far (the sum of the sample map).
 * kyhip_frame_blocks_ms: hipEvent durations of the last retire (or keep) kernel and of the last compaction of the live list, negative where there was none.
 * On a block-tracking frame kyhip_frame_render renders the live blocks only (none live: KY_OK, nothing is launched, the front stays -- a caller's loop
 *   `while (done < total)` must also end on kyhip_frame_block_stats' live == 0; a shard without tiles has no blocks and advances its front like any other
 *   frame's empty shard); kyhip_frame_render_until applies its whole-frame rule as on any frame and also returns, KY_OK, as soon as no block is live: the front
 *   and the map would not change any more. kyhip_frame_resolve with
 *   normalise 1 scales each pixel by total / (its block's samples) in double before the one rounding (blocks at 0 samples add nothing), and with normalise 0
 *   returns KY_ERR_INVALID_VALUE, the film untouched, while a block inside the film is retired short of the total (it would be darkened silently).
 * Checkpoints: a block-tracking frame's header has a magic number of its own -- frames that do not track blocks refuse its states and it refuses theirs -- and
 *   its state ends with a block trailer (behind the noise trailer when both are tracked): a magic number, the block count, then per block the retirement count
 *   (-1: live) and its batch count; the trailer also holds the passes rendered.  kyhip_frame_load refuses, the frame untouched, a missing or short trailer, another
 *   block count, a retirement count that is no value of kyhip_pass_boundaries (or 0) or lies beyond the header's samples done, and a block's batch count that is
 *   not 0 on a live block or one retired at 0 samples or exceeds the noise trailer's (0 on a frame that tracks no noise).
 * The calls on a frame that does not track blocks return KY_ERR_INVALID_VALUE; arguments are checked before any device work.
 */
typedef struct ky_block_stats { int32_t blocks, live, passes, samples_done, min_samples, max_samples; int64_t pixels, pixel_samples; } ky_block_stats;
int     kyhip_frame_track_blocks(kyhip_frame* f);
int     kyhip_frame_keep(kyhip_frame* f, const unsigned char* mask, size_t row_stride);
int     kyhip_frame_retire_noisy(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, ky_block_stats* out);
int     kyhip_frame_render_adaptive(kyhip_frame* f, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass,
                                    int* samples_done, ky_block_stats* out);
int     kyhip_frame_sample_map(kyhip_frame* f, int32_t* map, size_t row_stride_px);
int     kyhip_frame_block_stats(kyhip_frame* f, ky_block_stats* out);
int     kyhip_frame_blocks_ms(const kyhip_frame* f, float* retire_ms, float* list_ms);

/*
 * The denoised picture so far (DESIGN.md section 3 "Denoise"): an edge-avoiding a-trous wavelet filter over the frame's normalised picture
 * (kyhip_frame_resolve with normalise 1, before its clamp), guided by the per-pixel variance a tracking frame keeps and by the geometry at each pixel's first
 * hit, which one kernel traces once per frame (the camera ray through the pixel centre; independent of kyhip_set_boxes).  Level k = 0 .. levels - 1 is a
 * 5 x 5 B3-spline kernel with its taps 2^k pixels apart; a tap's weight is the spline's times max(0, n_p . n_q)^(2^normal_squarings), a plane distance term with
 * sigma_plane and a luminance term with sigma_luminance against the locally averaged variance, which the filter carries through its levels.  The arithmetic is
 * double precision without transcendentals (ky_amd/csrc/ky_denoise.hpp); two calls return identical bytes.
 *
 * kyhip_denoise_defaults: host only; the parameters a NULL `p` stands for.
 * kyhip_frame_denoise: ADDS clamp01(filtered value) per pixel to the film exactly as kyhip_frame_resolve does (a sub-film's first pixel and its row stride; a
 *   pinned film is added to in place).  levels == 0 IS kyhip_frame_resolve(f, 1, ...).  Pixels whose camera ray misses the scene (1), whose first hit carries an
 *   area light (2) or whose flag word pins their value (3) pass through unfiltered and are no other pixel's tap; every other pixel is class 0.  On a
 *   block-tracking frame each pixel is scaled and evaluated at its block's counts; blocks at 0 samples are class 1 and add nothing.
 *   KY_ERR_INVALID_VALUE, before any device work and with the film untouched: levels outside 0 .. 6, normal_squarings outside 0 .. 10, a sigma that is not > 0;
 *   a frame that does not track noise; a frame whose shard is not the whole film (tile_first 0, tile_step 1: a shard's neighbours live elsewhere); fewer than
 *   two noise batches (no variance yet).  Nothing a checkpoint holds changes: a frame may be denoised any number of times, rendered further, or be complete.
 * kyhip_frame_guides: WRITES width x height float4, y down, row_stride_px float4 apart: normal_t4 = {n.x, n.y, n.z, t} (the normal as the integrator sees it
 *   and the hit distance), position_class4 = {P.x, P.y, P.z, class}; zeros beside the class where there is no hit.  Either pointer may be NULL.  The frame as
 *   for kyhip_frame_denoise, but any number of batches.
 * kyhip_frame_denoise_ms: hipEvent spans of the guide trace (set once per frame) and of the last call's gather, levels and add; negative where there was none.
 *
 * Guides beyond the first hit (opt-in; the default, 0 bounces, is everything above).  With guide bounces B = 1 .. KYHIP_GUIDE_MAX_BOUNCES the guide kernel
 * follows the camera ray through mirrors and glass the way the debug sampler walks it (every number 0.5: glass takes the likelier of reflection and
 * refraction, total internal reflection reflects) for up to B specular vertices, and a pixel takes the guides of the first vertex that is neither -- its normal
 * and position, t summed along the chain, class 2 if it carries an area light, class 1 with zeros if the chain leaves the scene.  Each pixel also gets a KEY:
 * 10 bits per specular vertex k at bit 10 k, ((surface + 1) << 1) | (1 if transmitted), the caller's surface index; 0 where the first hit is not specular.  A
 * chain with more than B specular vertices is unresolved: bit 62 plus its first digit, the first hit's guides, class 0.  The filter then takes a class-0
 * pixel's taps, and its variance prefilter's neighbours, from the class-0 pixels with the SAME key only: what a mirror shows is filtered by the geometry it
 * shows, and neither ball is a tap of the walls around it.  Where it helps and where it does not: DESIGN.md "Denoise".
 * kyhip_frame_set_guide_bounces: 0 .. KYHIP_GUIDE_MAX_BOUNCES, else KY_ERR_INVALID_VALUE; KY_ERR_INVALID_VALUE with the frame untouched once its guides have been
 *   traced (the first kyhip_frame_denoise / _guides / _guide_chains call that reaches the device), unless the value is the one it has.  No part of a checkpoint.
 * kyhip_frame_guide_bounces: the value, or KY_ERR_INVALID_VALUE for a NULL frame.
 * kyhip_frame_guide_chains: WRITES width x height keys, y down, row_stride_px keys apart (all 0 at 0 bounces); the frame as for kyhip_frame_guides, which
 *   returns the chain-end guides.
 *
 * Albedo demodulation (opt-in per frame; the default, grid 0, is everything above to the byte and to the kernel).  With an albedo grid G = 1 .. KYHIP_ALBEDO_MAX_GRID
 * one more kernel, traced once per frame when the guides are, gives every pixel an ALBEDO {r, g, b, w}: G x G camera rays per pixel through the frame's own camera
 * form (its pixel filter's warp and its lens) -- sub-sample (i, j), j-major, has the film pair ((i + 0.5) g, (j + 0.5) g) and the lens pair ((j + 0.5) g,
 * (G - 1 - i + 0.5) g) with g the float 1 / G -- each walked through mirrors and glass for up to the frame's guide bounces as the guide kernel walks the centre ray.
 * A sub-sample's colour starts at (1, 1, 1); each specular vertex walked through multiplies by what its branch carries (a mirror's colour; glass: its reflection
 * colour reflected, its transmission colour transmitted); the vertex the walk ends on multiplies by its colour0 as the integrator takes it -- the frame's texture
 * there where the material has one, and for plastic colour0 / diffuse_probability -- if it is matte, plastic or a mirror, and by nothing if it is glass; a miss and
 * a surface that carries an area light multiply by nothing.  The pixel's albedo is the float32 sum of the G^2 colours in visit order times the float 1 / G^2, and w
 * the number of sub-samples that ended on a surface without a lamp.  kyhip_frame_denoise then DEMODULATES: with a' = max(albedo, 1/64) per channel, a class-0
 * pixel's colour is divided by a' and its variance by luminance(a')^2 before the levels, and the filtered colour is multiplied by a' before the clamp (double
 * arithmetic, one float32 rounding each; ky_amd/csrc/ky_denoise.hpp).  The levels filter what the light did, not what a checker or a texel edge did.  Pixels of
 * class 1, 2 and 3 take neither step; levels == 0 stays kyhip_frame_resolve(f, 1, ...).
 * kyhip_frame_set_albedo_grid: 0 .. KYHIP_ALBEDO_MAX_GRID (0: off), else KY_ERR_INVALID_VALUE; KY_ERR_INVALID_VALUE with the frame untouched once its guides have
 *   been traced (the first kyhip_frame_denoise / _guides / _guide_chains / _albedo call that reaches the device), unless the value is the one it has.  The albedo is
 *   traced with the guide bounces, filter, lens and textures the frame holds at that call.  No part of a checkpoint.
 * kyhip_frame_albedo_grid: the value, or KY_ERR_INVALID_VALUE for a NULL frame.
 * kyhip_frame_albedo: WRITES width x height float4 {r, g, b, w}, y down, row_stride_px float4 apart; the frame as for kyhip_frame_guides; KY_ERR_INVALID_VALUE
 *   at grid 0.
 * kyhip_frame_albedo_ms: the hipEvent span of the albedo trace (set once per frame), negative where there was none.
 */
#define KYHIP_GUIDE_MAX_BOUNCES 4
#define KYHIP_ALBEDO_MAX_GRID 8
typedef struct ky_denoise_params { int32_t levels, normal_squarings; float sigma_luminance, sigma_plane; } ky_denoise_params;
void    kyhip_denoise_defaults(ky_denoise_params* out);
int     kyhip_frame_denoise(kyhip_frame* f, const ky_denoise_params* p, float* film_rgb, size_t film_row_stride_px);
int     kyhip_frame_guides(kyhip_frame* f, float* normal_t4, float* position_class4, size_t row_stride_px);
int     kyhip_frame_denoise_ms(const kyhip_frame* f, float* guides_ms, float* filter_ms);
int     kyhip_frame_set_guide_bounces(kyhip_frame* f, int bounces);
int     kyhip_frame_guide_bounces(const kyhip_frame* f);
int     kyhip_frame_guide_chains(kyhip_frame* f, uint64_t* keys, size_t row_stride_px);
int     kyhip_frame_set_albedo_grid(kyhip_frame* f, int grid);
int     kyhip_frame_albedo_grid(const kyhip_frame* f);
int     kyhip_frame_albedo(kyhip_frame* f, float* albedo4, size_t row_stride_px);
int     kyhip_frame_albedo_ms(const kyhip_frame* f, float* ms);

/*
 * Temporal reuse: denoise across frames under a moving camera (DESIGN.md section 3 "Denoise", "Temporal").  A kyhip_history is a device-resident object of its
 * own, independent of any frame's lifetime: per pixel, in film order and double-buffered, the accumulated colour and variance {r, g, b, v}, the accumulated sample
 * count m (float32; 0: the pixel is nobody's tap), the guides {n, t} and {P} as they stood at the call that wrote them, the camera of that frame, and whether its
 * colours are albedo-demodulated.  It is no part of any checkpoint: kyhip_frame_state_bytes and saved states do not know of it.
 * THE CALLER'S CONTRACT: every frame that uses one history renders the SAME scene -- shapes, materials, lights, textures -- and differs in its camera (and seed,
 * sample counts, filter, lens) only.  Nothing checks this: there are no motion vectors, and moved geometry or lights show as ghosts.
 *
 * kyhip_frame_denoise_temporal is kyhip_frame_denoise with one kernel between the gather and the first level.  A class-0 pixel whose chain key is 0 projects its
 * guide position through the history's camera, takes the up to four history pixels around the landing point (bilinear weights times the level's own normal and
 * plane-distance weights, with t->normal_squarings and t->sigma_plane: they are the disocclusion test), and where their weight reaches t->min_weight blends their
 * mean with its own by sample counts: alpha = n / (n + M), M = min(the taps' mean m, t->max_history x n), n the samples the frame holds; the variance follows as
 * alpha^2 v + (1 - alpha)^2 v_h and the new count is n + M (ky_amd/csrc/ky_denoise.hpp, temporal_pixel_t: double arithmetic, two calls on equal inputs return
 * identical bytes).  Elsewhere the pixel keeps its own bits with m = n.  Pixels of class 1, 2, 3 and pixels with a non-zero chain key pass through with m = 0: a
 * virtual image behind a mirror does not reproject by this formula.  The result becomes the history's new side, the levels run on it (the history is not written
 * by them), then remodulate, clamp and ADD as kyhip_frame_denoise does.  levels == 0 delivers the accumulated picture unfiltered.  With a history that holds no
 * picture (fresh, or reset) the film is kyhip_frame_denoise's bit for bit at levels >= 1.
 * A frame with 0 guide bounces is accepted: its mirror and glass pixels then reuse history like any surface, and what they show LAGS the camera.  Use guide
 * bounces >= 1 where the scene has either.
 * KY_ERR_INVALID_VALUE, before any device work and with film and history untouched: a NULL frame, history or film; everything kyhip_frame_denoise refuses (its
 * parameters, a frame that tracks no noise, a shard, fewer than two noise batches); a frame that tracks blocks; a history of another device or size than the
 * frame's; a frame whose albedo mode (grid 0, or grid > 0) differs from what the history holds; max_history outside (0, 1024], sigma_plane <= 0, min_weight
 * outside [0, 1), normal_squarings outside 0 .. 10.  p and t may be NULL: the defaults.
 * kyhip_temporal_defaults: host only.  kyhip_history_create: width, height >= 1.  kyhip_history_reset: the history holds no picture afterwards, and its frame count
 * is 0.  kyhip_history_frames: the temporal calls since create / reset, or KY_ERR_INVALID_VALUE for a NULL history.  kyhip_history_read: WRITES width x height
 * float4 {r, g, b, v} (row_stride_px float4 apart) and width x height float counts (row_stride_px floats apart), either pointer may be NULL; zeros while the
 * history holds no picture.  kyhip_history_ms: the hipEvent span of the last temporal kernel, negative where there was none.
 */
typedef struct kyhip_history kyhip_history;
typedef struct ky_temporal_params { float max_history, sigma_plane, min_weight; int32_t normal_squarings; } ky_temporal_params;
void    kyhip_temporal_defaults(ky_temporal_params* out);
int     kyhip_history_create(int device, int width, int height, kyhip_history** out);
int     kyhip_history_destroy(kyhip_history* h);
int     kyhip_history_reset(kyhip_history* h);
int     kyhip_history_frames(const kyhip_history* h);
int     kyhip_history_read(kyhip_history* h, float* colour_variance4, float* count, size_t row_stride_px);
int     kyhip_history_ms(const kyhip_history* h, float* ms);
int     kyhip_frame_denoise_temporal(kyhip_frame* f, kyhip_history* h, const ky_denoise_params* p, const ky_temporal_params* t, float* film_rgb,
                                     size_t film_row_stride_px);

/*
 * Slices: a frame's sample ranges rendered apart and merged, bit for bit (DESIGN.md section 3 "Slices").  A pixel's samples are keyed by their absolute index,
 * cut into chunks by a schedule of samples_per_pixel alone, and every chunk sum enters a 64-bit integer word scaled by 1 / total under the WHOLE frame's term
 * limit: frames of one (scene, params) that rendered disjoint sets of chunks hold words whose integer sum is the word of one frame that rendered them all, in
 * any order, and flag words only gain bits.  A slice is a frame that owns the samples [first_sample, end_sample) of every pixel of its shard; a merge adds
 * another frame's words, ORs its flag words and pools its noise pairs.  Slices may live on any device, in any process, on any machine.
 *
 * kyhip_slice_bounds: host arithmetic.  Writes n_slices + 1 strictly ascending values, bounds[0] = 0 and bounds[n_slices] = spp; inner value k is the value of
 *   kyhip_pass_boundaries(spp) nearest to k * spp / n_slices (a tie goes to the lower one; moved by as few chunks as it takes to leave every slice one).  Returns KY_OK, or KY_ERR_INVALID_VALUE for an spp that
 *   kyhip_pass_boundaries refuses, n_slices < 1, a NULL bounds, or a frame of fewer chunks than n_slices.
 * kyhip_frame_begin_slice: kyhip_frame_begin in every check and status; the frame owns samples [first_sample, end_sample) of the samples_per_pixel-sample frame.
 *   Both are 0 or a value of kyhip_pass_boundaries and first <= end, else KY_ERR_INVALID_VALUE.  first == end is a collector: it owns and renders nothing and
 *   exists to receive merges (a preview of all slices as they stand).  (0, samples_per_pixel) IS kyhip_frame_begin: the same frame, the same checkpoint bytes.
 * A frame holds a coverage: the sample ranges its accumulators contain -- disjoint, ascending, adjacent ones joined, at most KYHIP_SLICE_MAX_RANGES.
 * kyhip_frame_coverage: returns the number of ranges; writes min(n, count) {first, end} pairs to ranges2 and the owned range to own (either may be NULL).
 * kyhip_frame_samples' done is the number of samples per pixel HELD, the sum of the coverage (on a frame that never merged: what it always was), and that is
 *   what kyhip_frame_resolve with normalise 1, the noise estimate and kyhip_frame_denoise divide by.
 * kyhip_frame_render on a slice renders whole chunks of the owned range from its front; the frame is complete when the owned range is rendered.  The pass note
 *   of kyhip_last_kernel names absolute chunk and sample indices.  kyhip_frame_render_until works on a slice as on any frame.
 * kyhip_frame_merge: `state` is what kyhip_frame_save wrote for another frame of the same scene and params.  KY_ERR_INVALID_VALUE, before any device work and
 *   with dst untouched (its next save returns the bytes it returned before): a short buffer; a header that is no frame state or differs in source hash, params,
 *   scene hash or pixel count; a coverage that intersects dst's coverage, or dst's owned range whether rendered or not (later passes would count those samples
 *   twice -- so a kyhip_frame_begin frame, which owns everything, never receives a merge); a dst that tracks noise and a state without a valid noise trailer; a
 *   block-tracking frame on either side.  KY_ERR_LIMIT: a union of more than KYHIP_SLICE_MAX_RANGES ranges.  A dst that does not track noise ignores the state's
 *   noise trailer.  Otherwise one kernel merges and the coverage becomes the union.  Blocking.
 *   Noise pairs: m2 = a.m2 + b.m2 + n_a n_b / (n_a + n_b) (mean_b - mean_a)^2, the batch counts add, and the luminance sum is recomputed from the merged words;
 *   the last bits of m2 depend on which side is dst and on the order of the merges.  The words and flags do not.
 * kyhip_frame_merge_from: the same for a frame of this process without a host round trip: on dst's device the kernel reads src's buffers, from another device
 *   they are copied peer to peer into a buffer dst owns first.  src is unchanged.  src == dst: KY_ERR_INVALID_VALUE.
 * kyhip_frame_merge_ms: the hipEvent span of the last merge kernel, negative when there was none.
 * kyhip_frame_track_blocks on a frame whose owned range is not (0, samples_per_pixel) returns KY_ERR_INVALID_VALUE.
 * Checkpoints: every frame not begun as (0, samples_per_pixel) has a header magic of its own -- plain and block frames refuse its states and it theirs on load --
 *   whose samples done is the held count, and its state ends, behind the noise trailer, with a slice trailer of fixed size: a magic number, the owned range, the
 *   front, the range count and KYHIP_SLICE_MAX_RANGES pairs.  All slices of one frame that agree in tracking noise have states of one size.  kyhip_frame_load
 *   refuses, the frame untouched: another owned range; a front outside the owned range or on no pass boundary; ranges that are not ascending, disjoint and on
 *   boundaries, or whose part inside the owned range is not exactly [first, front); a held count that disagrees with the header or the noise trailer.
 */
#define KYHIP_SLICE_MAX_RANGES 32
int     kyhip_slice_bounds(int spp, int n_slices, int* bounds);
int     kyhip_frame_begin_slice(int device, const ky_scene* scene, const ky_render_params* params, int first_sample, int end_sample, kyhip_frame** out);
int     kyhip_frame_coverage(const kyhip_frame* f, int* ranges2, int n, int own[2]);
int     kyhip_frame_merge(kyhip_frame* dst, const void* state, size_t bytes);
int     kyhip_frame_merge_from(kyhip_frame* dst, kyhip_frame* src);
int     kyhip_frame_merge_ms(const kyhip_frame* f, float* ms);

/*
 * Pixel filters (ky_pixel_filter above).
 * Host only, no device needed:
 *   kyhip_filter_check     KY_OK, or KY_ERR_INVALID_VALUE with the message: NULL, an unknown kind, a radius outside 0.5 .. KYHIP_FILTER_MAX_RADIUS or not finite
 *                          (a box's radius is not looked at), a Gaussian sigma that is not > 0 and finite, reserved != 0.
 *   kyhip_filter_defaults  box; tent radius 2; Gaussian radius 1.5, sigma 0.5; Blackman-Harris radius 2.
 *   kyhip_filter_table     the inverse-CDF table the device reads: n must be KYHIP_FILTER_TABLE + 1; out[i] = F^-1(i / KYHIP_FILTER_TABLE) in pixels from the pixel's
 *                          centre, computed in double and rounded once; out[0] = -radius and out[n - 1] = +radius exactly, out[i] = -out[n - 1 - i].  Every kind gets
 *                          one (the box's is the uniform law over [-0.5, 0.5]), though the device reads it for the Gaussian and Blackman-Harris only.
 *   kyhip_scene_screen_bound_filtered  kyhip_scene_screen_bound for a launch under `filter`: the scene's live rectangle grown by ceil(radius - 0.5) pixels on every
 *                          side before it is cut to the frame -- a filter's offsets lie in [0.5 - radius, 0.5 + radius], not in [0, 1) -- and the blocks of the shard
 *                          outside THAT rectangle, which are the ones a filtered launch skips.  A box filter (or NULL) gives kyhip_scene_screen_bound's answer.
 * On the device:
 *   kyhip_render_filtered  kyhip_render under a pixel filter.  A box filter (or NULL) IS kyhip_render: the same film bit for bit, the same kernel.  Any other filter
 *                          runs a filtered run-time-dispatched kernel (kyhip_last_kernel names it and the filter): there are no specialised, masked or queue-engine
 *                          filtered kernels and no run-time instantiation of one.  The debug sampler's 0.5 is the pixel's centre under every filter: it ignores the
 *                          filter and runs kyhip_render's kernels.  The film equals that of a filtered frame rendered in any number of passes or slices.
 *   kyhip_frame_set_filter the frame's filter, before its first sample is rendered, loaded or merged (KY_ERR_INVALID_VALUE afterwards).  The filter is part of what the
 *                          frame IS: for any filter but the box its kind, radius and param are folded into the scene hash of the frame's header, so a state loads and
 *                          merges only into a frame with the same filter; the checkpoint's layout and size do not change.  Denoise guides stay traced through pixel centres.
 *   kyhip_frame_filter     reads it back (box until one is set).
 *   kyhip_kat_filter       the warp alone: out[i] = the offset from the pixel's corner for u[i] in [0, 1).
 *   kyhip_kat_li_filtered  kyhip_kat_li's samples under a filter: what the filtered kernels add per camera sample.
 */
int     kyhip_filter_check(const ky_pixel_filter* filter);
int     kyhip_filter_defaults(int kind, ky_pixel_filter* out);
int     kyhip_filter_table(const ky_pixel_filter* filter, float* out, int n);
int     kyhip_scene_screen_bound_filtered(const ky_scene* scene, const ky_render_params* params, const ky_pixel_filter* filter, int rect[4], long long counts[2]);
int     kyhip_render_filtered(int device, const ky_scene* scene, const ky_render_params* params, const ky_pixel_filter* filter,
                              float* film_rgb, size_t film_row_stride_px);
int     kyhip_frame_set_filter(kyhip_frame* f, const ky_pixel_filter* filter);
int     kyhip_frame_filter(const kyhip_frame* f, ky_pixel_filter* out);
int     kyhip_kat_filter(int device, const ky_pixel_filter* filter, const float* u, int n, float* out);
int     kyhip_kat_li_filtered(int device, const ky_scene* scene, const ky_render_params* params, const ky_pixel_filter* filter,
                              int x, int y, int s0, int n, float* out3);

/*
 * The thin lens (ky_lens above).
 * Host only, no device needed:
 *   kyhip_lens_check       KY_OK, or KY_ERR_INVALID_VALUE with the message: NULL, a radius that is negative or not finite, a focus distance that is not finite
 *                          and > 0 when the radius is > 0 (a pinhole's focus distance is not looked at), reserved words != 0.
 *   kyhip_scene_screen_bound_lens  kyhip_scene_screen_bound_filtered for a launch under `lens` as well: with radius > 0 the whole pixel range -- the live
 *                          rectangle's proof is a projection from ONE point and does not hold from a disk, so a lens launch culls nothing (counts[0] = 0).
 *                          radius 0 (or NULL) gives kyhip_scene_screen_bound_filtered's answer.
 * On the device:
 *   kyhip_render_lens      kyhip_render_filtered under a lens.  radius 0 (or NULL) IS kyhip_render_filtered: the same film bit for bit, the same kernel.  Any
 *                          other lens runs a lens row of the run-time-dispatched kernels (kyhip_last_kernel names it, the lens and the filter): the lens point
 *                          is Shirley's concentric map of the sample's third and fourth numbers.  No specialised, masked or queue-engine lens kernels, no
 *                          run-time instantiation.  The debug sampler's (0.5, 0.5) is the centre of the lens: it ignores the lens and runs kyhip_render's kernels.
 *   kyhip_frame_set_lens   the frame's lens, before its first sample is rendered, loaded or merged (KY_ERR_INVALID_VALUE afterwards).  For radius > 0 the bits of
 *                          radius and focus_distance are folded into the scene hash of the frame's header: a state loads and merges only into a frame with the
 *                          same lens; the checkpoint's layout and size do not change.  Denoise guides stay traced from the lens centre through pixel centres.
 *   kyhip_frame_lens       reads it back (the pinhole, {0, 0}, until one is set).
 *   kyhip_kat_lens         the disk map alone: out[2 i], out[2 i + 1] = the point of the unit disk for u[2 i], u[2 i + 1] in [0, 1).
 *   kyhip_kat_li_lens      kyhip_kat_li_filtered's samples under a lens: what the lens rows add per camera sample.
 */
int     kyhip_lens_check(const ky_lens* lens);
int     kyhip_scene_screen_bound_lens(const ky_scene* scene, const ky_render_params* params, const ky_pixel_filter* filter, const ky_lens* lens,
                                      int rect[4], long long counts[2]);
int     kyhip_render_lens(int device, const ky_scene* scene, const ky_render_params* params, const ky_pixel_filter* filter, const ky_lens* lens,
                          float* film_rgb, size_t film_row_stride_px);
int     kyhip_frame_set_lens(kyhip_frame* f, const ky_lens* lens);
int     kyhip_frame_lens(const kyhip_frame* f, ky_lens* out);
int     kyhip_kat_lens(int device, const float* u2, int n, float* out2);
int     kyhip_kat_li_lens(int device, const ky_scene* scene, const ky_render_params* params, const ky_pixel_filter* filter, const ky_lens* lens,
                          int x, int y, int s0, int n, float* out3);

/*
 * Textures (ky_texture above).
 * Host only, no device needed:
 *   kyhip_texture_check    KY_OK, or the refusal every entry below makes first.  KY_ERR_INVALID_VALUE: a NULL set with n_textures > 0, n_textures < 0, an unknown
 *                          kind, a material index out of range, a glass material, a second texture on one material, a non-finite or negative a / b / texel, a scale
 *                          that is 0, not finite or beyond KYHIP_MAX_TEXTURE_SCALE in size, an offset that is not finite or beyond it, flags beyond KY_TEXTURE_BILINEAR | KY_TEXTURE_CLAMP, reserved != 0, an image
 *                          without texels or with a dimension < 1.  KY_ERR_LIMIT: more than KYHIP_MAX_TEXTURES textures, an image dimension over
 *                          KYHIP_MAX_TEXTURE_SIZE, more than KYHIP_MAX_TEXELS texels over the set.
 * On the device:
 *   kyhip_render_textured  kyhip_render_lens under a texture set; filter and lens may be NULL.  n_textures == 0 IS kyhip_render_lens: the same film bit for bit, the
 *                          same kernels.  Otherwise a textured row of the run-time-dispatched kernels runs (kyhip_last_kernel: "..., textured>" and a note that
 *                          names the camera form): ONE camera form serves plain, filtered and lens launches -- it warps unless the filter is the box, and moves
 *                          the ray onto the lens unless that is the pinhole -- and reads the live rectangle as the filtered kernels do (grown by the filter's
 *                          reach; with a lens of radius > 0 the whole pixel range).  No specialised, masked or queue-engine textured kernels, no run-time
 *                          instantiation, and no textured row for the debug sampler (KY_ERR_INVALID_VALUE).  A texture draws no random number and does not
 *                          touch the film: a textured frame in any number of passes, slices or merges is the one-shot film bit for bit.
 *                          sample_single_light's spatial pick (177) weighs a plastic vertex by the colour the vertex has, the textured one (it reads the
 *                          vertex's material record, which is the lane's textured copy); the estimate is unbiased under any positive weights.
 *   kyhip_frame_set_textures  the frame's texture set, before its first sample is rendered, loaded or merged (KY_ERR_INVALID_VALUE afterwards).  Descriptors and texels
 *                          are copied and uploaded once; a digest of both is folded into the scene hash of the frame's header, so a state loads and merges only into
 *                          a frame with the same textures.  n_textures == 0 removes the set.  The denoise guides hold geometry only; a frame's albedo (kyhip_frame_set_albedo_grid) reads the set.
 *   kyhip_kat_li_textured  kyhip_kat_li_lens's samples under a texture set: what the textured rows add per camera sample.
 *   kyhip_kat_texture      a known-answer probe through the device functions the render kernels call: for n_points world points on surface `surface` (the caller's
 *                          index; its material must carry a texture of the set) out5 = (u', v', r, g, b), the colour as the vertex's material takes it (on a
 *                          plastic material: texel / diffuse_probability).
 */
int     kyhip_texture_check(const ky_scene* scene, const ky_texture* textures, int n_textures);
int     kyhip_render_textured(int device, const ky_scene* scene, const ky_texture* textures, int n_textures, const ky_render_params* params,
                              const ky_pixel_filter* filter, const ky_lens* lens, float* film_rgb, size_t film_row_stride_px);
int     kyhip_frame_set_textures(kyhip_frame* f, const ky_texture* textures, int n_textures);
int     kyhip_kat_li_textured(int device, const ky_scene* scene, const ky_texture* textures, int n_textures, const ky_render_params* params,
                              const ky_pixel_filter* filter, const ky_lens* lens, int x, int y, int s0, int n, float* out3);
int     kyhip_kat_texture(int device, const ky_scene* scene, const ky_texture* textures, int n_textures, int surface, const float* points3, int n_points, float* out5);

/*
 * Duration in milliseconds of the integrator kernel (render_kernel) of the most recent
 * kyhip_render* call on `device`, from hipEvents recorded on the launch stream around that one
 * kernel.  The stream must have been synchronised.  Negative if no timing is available.
 */
float kyhip_kernel_ms(int device);
/* Which render-kernel instantiation that call launched, e.g. "render_kernel<strategy 48, feat 7, integrator 11>" (the library holds one
   per direct-lighting strategy, integrator and set of scene facts; ky_launch.hip, g_variants).  The string stays valid until the next call
   of this function from the same thread.  "" if nothing was launched. */
const char* kyhip_last_kernel(int device);

/* ------------------------------------------------------------------------------------------
 * Function-level entry points (known-answer tests).  Each runs the DEVICE implementation of one
 * reference function over n host-side inputs and copies the results back.  Blocking.
 * ---------------------------------------------------------------------------------------- */

/* shape_t::intersect (1111, 1179, 1261, 1336).  rays: n x {o[3], d[3], tmax}.
   out: n x {hit(0/1), t, p[3], n[3]}. */
int kyhip_kat_intersect(int device, const ky_shape* shape, const float* rays7, int n, float* out8);

/* camera_t::generate_ray (1884-1892).  p_film: n x {x, y}.  out: n x {o[3], d[3]}. */
int kyhip_kat_camera(int device, const ky_camera* camera, const float* p_film2, int n, float* out6);

/* surface_t::intersect + material_t::scattering + bsdf_t::{sample, eval, pdf} (3077, 2587-2671, 2162-2179).
   in: n x {normal[3], wo[3], u[2], wi_eval[3], lobe_u}.  out: n x {f[3], wi[3], pdf, flags, eval[3], pdf_eval, is_delta}. */
int kyhip_kat_bsdf(int device, const ky_material* material, const float* in12, int n, float* out13);
/* The same rows through the lobe code the render kernels execute: what path_tracing_iteration_t makes of its BSDF sample (4586-4597: the direction, the
   factor f |n.wi| / pdf its throughput is multiplied by, whether the path goes on, whether the lobe is specular) and the light-sampling estimators' evaluation
   of wi_eval as colour x scale.  flat_phong != 0: the variant of scenes whose plastic surfaces are all rectangles (no flip behind a Phong lobe); the same
   result wherever n.wo >= 0.  Rows are taken 256 per workgroup in order, so 64 consecutive rows share a wavefront.
   out: n x {wi[3], weight[3], ok(0/1), specular(0/1), eval[3], pdf_eval}. */
int kyhip_kat_bsdf_continue(int device, const ky_material* material, const float* in12, int n, int flat_phong, float* out12);

/* light_t::sample_Li / pdf_Li (2825, 2891, 2964, 3026).
   in: n x {p[3], normal[3], u[2], wi[3]}.  out: n x {position[3], wi[3], pdf, Li[3], pdf_Li}. */
int kyhip_kat_light(int device, const ky_scene* scene, int light, const float* in11, int n, float* out11);

/* scene_t::intersect (3172) and scene_t::occluded (3187-3201).
   rays7 as above.  out: n x {hit, t, p[3], n[3], surface}.
   occluded: in n x {p[3], normal[3], target[3]}, out n x {0/1}. */
int kyhip_kat_scene_intersect(int device, const ky_scene* scene, const float* rays7, int n, float* out9);
int kyhip_kat_occluded(int device, const ky_scene* scene, const float* in9, int n, float* out1);
/* The any-hit pair scan of the environment light's both_mis estimate (round 6: trace_any_pair, ky_device.hpp): per row two rays through ONE scan of every surface --
   ray A without an end ("does it leave the scene": scene_t::intersect finds nothing, 4000), ray B ending at tmax_b (scene_t::occluded's scan, 3193-3195) -- with the box
   traversal when the scene has boxes.  in: n x {o_a[3], d_a[3], o_b[3], d_b[3], tmax_b}.  out: n x {A meets a surface 0/1, B meets one before tmax_b 0/1}. */
int kyhip_kat_any_pair(int device, const ky_scene* scene, const float* in13, int n, float* out2);
/* The same query against the occluder tables the render kernels use for shadow rays ("occluder tables").
   light = -1: p and target are promised to lie on surfaces, area lights' shapes or point lights of the scene; rectangles that have the
   whole scene in one closed half-space of their plane (the walls of a room) are not tested.
   light >= 0: additionally target is a point of the shape area light `light` samples and p lies in front of it (where light_t::sample_Li
   returns a non-black Li, 2957-2960); for a planar sampled shape the surfaces on or behind its plane are not tested either.
   For segments that keep the promise the answer equals kyhip_kat_occluded's. */
int kyhip_kat_occluded_between(int device, const ky_scene* scene, int light, const float* in9, int n, float* out1);
/* Host only (no GPU needed): left_out[i] = 1 when surface i (the caller's index) is not in the occluder table for `light` (-1: the table
   for rays that end on a scene point), 2 when it is scanned only for rays with an end behind that light's plane (the two-stage scan:
   what is mounted behind a lamp), 0 when it is always tested.  n = entries in left_out, at least scene->surface_count.  Returns the
   number of 1s, or a negative ky_status. */
int kyhip_scene_non_occluders(const ky_scene* scene, int light, int* left_out, int n);
/* Host only (no GPU needed): the axis-aligned boxes whose faces are surfaces of the scene, which a nearest-hit traversal (scene_t::intersect, ky.cpp:3172-3184) tests
   with one slab test each instead of face by face ("boxes"): box_face[i] = 8 * box + 2 * axis + side (side 0: the box's low plane on that axis, 1: its high
   plane) when surface i (the caller's index) is such a face, -1 otherwise.  n = entries in box_face, at least scene->surface_count.  Returns the number of boxes
   (0 with kyhip_set_specialisation(0)), or a negative ky_status. */
int kyhip_scene_boxes(const ky_scene* scene, int* box_face, int n);
/* Host only (no GPU needed): the scene's live rectangle for the frame of `params` -- rect = {x0, y0, x1, y1}: no camera sample of a pixel outside
   [x0, x1) x [y0, y1) reaches a surface, so the film is exactly 0 there.  The whole frame {0, 0, width, height} when that cannot be proved (an environment light, a
   camera inside or beside the scene's bound, coordinates that are not finite, no surfaces) and with kyhip_set_screen_cull(0).  counts (may be NULL): counts[0] = the
   8 x 8 pixel blocks of the shard `params` names that lie outside the rectangle (the work the render kernels skip), counts[1] = all of the shard's blocks.
   Returns KY_OK or a negative ky_status. */
int kyhip_scene_screen_bound(const ky_scene* scene, const ky_render_params* params, int rect[4], long long counts[2]);
/* Host only: the facts the library finds for a scene when it packs it -- a mask of the KY_FEAT_* values of ky_amd/csrc/ky_scene.hpp (1 exactly one area light, 2 every
   area light samples a rectangle, 4 few carrier surfaces per light, 8 exactly one point / directional light, 16 exactly one environment light, 32 sphere lamps only,
   64 no mirror or glass, 128 at most 16 surfaces and 8 materials, 256 every lamp is its own one carrier, 512 boxes, 1024 every planar surface is a rectangle in an axis
   plane, 2048 every plastic surface is a rectangle, 4096 every tilted rectangle is a plank about the x axis) -- which decide the render-kernel instantiation a launch takes (kyhip_last_kernel names it).  0 with kyhip_set_specialisation(0); negative: a ky_status. */
int kyhip_scene_facts(const ky_scene* scene);
/* Host only: what sample_single_light's power and spatial picks (KY_DIRECT_SINGLE_POWER / _SPATIAL) know of the scene's lights.  power_p16 (may be NULL): the 16
   probabilities of the power rule, defensive share included, zeros behind the light count.  proxies (may be NULL with max_proxies 0): up to max_proxies emitter
   proxies of 11 floats {light (the caller's index), kind (0 sphere, 1 planar, 2 point, 3 direction, 4 environment), c[3], r, n[3], A, e}; a light's proxies are
   contiguous: the shape it samples, then its carrier surfaces of other shapes; the table holds at most 32, carrier proxies dropped from the last light backwards.
   `rule`: 1 or 2 (both tables are the same for either; anything else is refused).  Returns the proxy count, or a negative ky_status. */
int kyhip_scene_light_pick(const ky_scene* scene, int rule, float* power_p16, float* proxies, int max_proxies);

/* integrator_t::Li per camera sample (3714-3717): for pixel (x, y) and samples [s0, s0+n) writes the
   unclamped radiance Li (3 floats per sample) -- the quantity `dL` is built from. */
int kyhip_kat_li(int device, const ky_scene* scene, const ky_render_params* params,
                 int x, int y, int s0, int n, float* out3);

/* estimate_direct_lighting_{by_bsdf, by_emitter, by_bsdf_mis, by_emitter_mis} (3889-4074) for ONE light at given vertices with given
   random numbers.  in15: n x {position[3], normal[3], wo[3], surface (index into scene->surfaces), lobe_u (the plastic material's lobe
   number, 2663), random_bsdf[2], random_light[2]}; out6: n x {the BSDF-sampling half [3], the light-sampling half [3]}.
   direct_sample 4 / 8: the plain estimators (by_bsdf uses random_bsdf as the float2 it draws itself, 3900); 16 / 32: the MIS halves;
   48: both MIS halves (not yet weighted by the 0.5 of 4083).  Vertices on delta surfaces return zeros (4571). */
int kyhip_kat_nee(int device, const ky_scene* scene, int direct_sample, int light, const float* in15, int n, float* out6);
/* integrator_t::sample_single_light (3813-3832) at given vertices with given numbers.  in16: a kyhip_kat_nee row, then pick_u; the light is
 * min((int)(pick_u * light_count), light_count - 1) in fp32.  out6: the picked light's two both_mis halves (BSDF half, light half), each already
 * divided by the pick probability 1 / light_count, and -- like kyhip_kat_nee's -- not weighted by the 0.5 of 4083.  A scene without lights is refused. */
int kyhip_kat_single_light(int device, const ky_scene* scene, const float* in16, int n, float* out6);
/* sample_single_light's pick under `rule` (0 uniform, 1 power, 2 spatial) at kyhip_kat_single_light's rows, through the device function the render kernels
 * call.  out18: n x {the picked light's index, its probability, p[0 .. 15] -- every light's probability at the row's vertex, from the same weight function one
 * light at a time; zeros behind the light count}.  Vertices on mirror or glass surfaces take no estimate in a render; their rows are computed all the same. */
int kyhip_kat_light_pick(int device, const ky_scene* scene, int rule, const float* in16, int n, float* out18);
/* kyhip_kat_single_light with the light picked under `rule` and the two halves divided by that light's probability; rule 0 is kyhip_kat_single_light. */
int kyhip_kat_single_light_rule(int device, const ky_scene* scene, int rule, const float* in16, int n, float* out6);

/* The same sample of path_tracing_iteration_t vertex by vertex (the reference's LOG_VAST at ky.cpp:4578 prints the same facts):
   one row of 26 floats per vertex that reaches the continuation sample (4586):
   {bounces, surface (caller's index), lobe (0 lambert, 1 mirror, 2 glass, 3 phong), position[3], normal[3], wo[3],
    beta[3] before the bounce, Lo[3] after this vertex's direct lighting, bs.f[3], bs.pdf, |dot(bs.wi, normal)|, bsdf flags,
    bits of the lights whose BSDF-sampling estimate was non-black, bits of the lights whose light-sampling estimate was}.
   Returns the number of rows written (<= max_rows) or a negative ky_status; li3 (optional) receives the sample's radiance. */
int kyhip_kat_li_trace(int device, const ky_scene* scene, const ky_render_params* params, int x, int y, int s,
                       float* rows26, int max_rows, float* li3);

/* The random-number streams of the render kernels by key.  keys2: n x {pixel_index (y * width + x), sample_index} as uint32;
   out: n x k uint32, the BIT PATTERNS of the first k floats the stream of (seed, pixel_index, sample_index) hands out, in order.  1 <= k <= 256.
   debug != 0: the debug sampler's stream (0.5 everywhere). */
int kyhip_kat_sampler(int device, uint32_t seed, const uint32_t* keys2, int n, int k, int debug, uint32_t* out);
/* The same for any ky_sampler_kind, through the device functions the render kernels draw with.  spp: the frame's samples_per_pixel, which the stratified
   sampler's strata depend on (the other kinds ignore it); under KY_SAMPLER_STRATIFIED 1 <= spp <= 2^24 and a key whose sample_index is >= spp is refused. */
int kyhip_kat_sampler_kind(int device, int kind, uint32_t seed, int spp, const uint32_t* keys2, int n, int k, uint32_t* out);

/* ---- the smallpt lineage's own scene, in double precision -----------------------------------------
   smallpt2pbrt/smallpt.cpp is the 99-line path tracer ky grew out of (smallpt_milo.cpp is its 256 x 256 build):
   9 spheres -- the walls are spheres of radius 1e5, which is why ky's fp32 sphere test cannot render this scene
    -- recursive radiance() with Russian roulette after 5 bounces and a two-way split at the glass
   sphere for the first two bounces (smallpt.cpp:56-89), 2 x 2 subpixels with a tent filter, per-subpixel clamp
   (91-118).  Random numbers: smallpt seeds erand48 per image ROW and walks the row sequentially (98); this library
   gives every (pixel, subpixel, sample) its own stream keyed by (seed, pixel, subpixel, sample) and consumes numbers in
   radiance()'s order, reflection subtree before transmission subtree. */
enum ky_smallpt_refl { KY_SP_DIFF = 0, KY_SP_SPEC = 1, KY_SP_REFR = 2 };   /* Refl_t, smallpt.cpp:24 */

typedef struct ky_smallpt_sphere {   /* struct Sphere, smallpt.cpp:26-39 */
    double rad;
    double p[3], e[3], c[3];         /* position, emission, colour */
    int refl;
    int pad_;
} ky_smallpt_sphere;

/* Which program of the smallpt lineage the fp64 path restates.
   KY_SP_VARIANT_SMALLPT  smallpt2pbrt/smallpt.cpp as described above.
   KY_SP_VARIANT_REWRITE  smallpt2pbrt/smallpt_rewrite.cpp ("structured smallpt", the pbrt-style step towards ky.cpp; the one
                          reference program that builds in this image and therefore pins this path, oracle/_ref): the nine
                          spheres mirrored in z (1199-1244), PerspectiveCamera fov 53 (1391), RandomSampler (uniform jitter,
                          `samps` samples per PIXEL, 369-392), RecursionPathIntegrater(max_depth 10) (1335-1372), one clamp per
                          pixel (1316).  Streams are keyed (seed, pixel, sample). */
enum ky_smallpt_variant { KY_SP_VARIANT_SMALLPT = 0, KY_SP_VARIANT_REWRITE = 1 };

typedef struct ky_smallpt_params {
    int width, height;
    int samps;                       /* variant 0: samples per SUBPIXEL (smallpt.cpp:92: argv[1] / 4), spp = 4 * samps;
                                        variant 1: samples per pixel (smallpt_rewrite.cpp:1388: argv[1] / 4) */
    uint32_t seed;
    int max_depth;                   /* `if (depth > 10) return obj.e` (smallpt.cpp:63) / RecursionPathIntegrater(10) (1396): 10 */
    int variant;                     /* ky_smallpt_variant */
} ky_smallpt_params;

/* The scene of smallpt.cpp:42-52; `out` has room for 9 spheres.  Returns 9.  Pure host code. */
int kyhip_smallpt_scene(ky_smallpt_sphere* out);
/* Scene::CreateSmallptScene of smallpt_rewrite.cpp:1199-1244 (the same spheres at -z).  Returns 9.  Pure host code. */
int kyhip_smallpt_scene_rewrite(ky_smallpt_sphere* out);

/* main()'s loop nest (smallpt.cpp:91-118) with the fixed camera of 93-94.  image_rgb: width * height * 3 doubles in
   smallpt's own order, c[(height - y - 1) * width + x], i.e. row 0 is the TOP of the picture; the image is overwritten.
   Variant 1: Integrater::Render (smallpt_rewrite.cpp:1287-1318) into a cleared Film, pixels_[y * width + x] with y = 0 the
   top row (517-520).  For variant 1 the kat entry ignores (sx, sy), which must be 0. */
int kyhip_smallpt_render(int device, const ky_smallpt_sphere* spheres, int n_spheres, const ky_smallpt_params* params,
                         double* image_rgb);

/* radiance(Ray(cam.o + d * 140, d.norm()), 0, Xi) (smallpt.cpp:109) for samples [s0, s0 + n) of subpixel (sx, sy) of
   pixel (x, y): 3 doubles per sample, unclamped. */
int kyhip_smallpt_kat_radiance(int device, const ky_smallpt_sphere* spheres, int n_spheres, const ky_smallpt_params* params,
                               int x, int y, int sx, int sy, int s0, int n, double* out3);

/* The fp64 path's random-number streams by key.  keys2: n x {subpixel_index ((y * width + x) * 4 + sy * 2 + sx; variant 1: y * width + x), sample}
   as uint32; out: n x k uint64, the bit patterns of the first k doubles of the stream of (seed, subpixel_index, sample).  1 <= k <= 256. */
int kyhip_smallpt_kat_rng(int device, uint32_t seed, const uint32_t* keys2, int n, int k, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* KYHIP_H */
