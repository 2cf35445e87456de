/*
 * ky_kat.hip -- function-level known-answer-test kernels and their C-ABI entry points (include/kyhip.h, "KAT entry points"): each runs ONE function
 * of the path -- a shape test, the camera, a BSDF lobe, a light, the scene traversal, an occlusion query, one estimator, one camera sample's
 * radiance with or without a vertex trace, the random-number streams by key -- on caller-supplied inputs, for tests/test_parity_gpu.py to compare with the
 * oracle (the streams: tests/test_sampler_gpu.py, with a restatement that shares no code with either).  Test surface
 * of the library, not part of a render; the kernels are the product's device functions (ky_device.hpp) called directly.
 * The kernels come first and the entry points after them, both in the same order, by subject.
 */
#include <cstring>
#include <vector>

#include "ky_ctx.hpp"
#include "ky_render.hpp"

using namespace kyh;

// ---- KAT kernels ----
struct KatShape { DSurf surf; DShapeFull full; DHit hit; };

__global__ void kat_intersect_kernel(KatShape sh, const float* __restrict__ rays7, int n, float* __restrict__ out8) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rays7 + 7 * (size_t)i;
    const f3 o = ld3(r), d = ld3(r + 3);
    float t;
    const bool hit = surf_hit(sh.surf, &sh.full, o, d, r[6], t);
    float* o8 = out8 + 8 * (size_t)i;
    f3 p = mk3(0, 0, 0), nn = mk3(0, 0, 0);
    if (hit) { p = o + t * d; nn = hit_normal(sh.hit, p, d); }
    o8[0] = hit ? 1.f : 0.f; o8[1] = hit ? t : 0.f;
    o8[2] = p.x; o8[3] = p.y; o8[4] = p.z; o8[5] = nn.x; o8[6] = nn.y; o8[7] = nn.z;
}

__global__ void kat_camera_kernel(const DScene* __restrict__ S, const float* __restrict__ pf, int n, float* __restrict__ out6) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f3 o, d;
    generate_ray(S, pf[2 * (size_t)i], pf[2 * (size_t)i + 1], o, d);
    float* q = out6 + 6 * (size_t)i;
    q[0] = o.x; q[1] = o.y; q[2] = o.z; q[3] = d.x; q[4] = d.y; q[5] = d.z;
}

__global__ void kat_bsdf_kernel(DMat M, const float* __restrict__ in12, int n, float* __restrict__ out13) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = in12 + 12 * (size_t)i;
    const f3 normal = ld3(r), wo = ld3(r + 3), wi_eval = ld3(r + 8);
    Vertex v;
    v.normal = normal;
    v.bsdf = make_bsdf(M, r[11]);
    const Bsdf& B = v.bsdf;
    vertex_prepare(v, wo);
    const BsdfSample bs = bsdf_sample(v, wo, r[6], r[7]);
    f3 ev; float pd, abs_cos_i;
    bsdf_eval_pdf(v, wo, wi_eval, ev, pd, abs_cos_i);
    float* q = out13 + 13 * (size_t)i;
    q[0] = bs.f.x; q[1] = bs.f.y; q[2] = bs.f.z; q[3] = bs.wi.x; q[4] = bs.wi.y; q[5] = bs.wi.z; q[6] = bs.pdf;
    q[7] = (float)bs.flags; q[8] = ev.x; q[9] = ev.y; q[10] = ev.z; q[11] = pd; q[12] = bsdf_is_delta(B) ? 1.f : 0.f;
}

// the same rows and the same vertex through what the render kernels execute: bsdf_continue (the iterative integrator's sample: direction, value |cos| / pdf in one
// factor, whether the path goes on) and bsdf_eval_parts (the light-sampling estimators' evaluation as two factors).  256 rows per workgroup in order: a wave is 64
// consecutive rows, which is what phong_pow_lobe's vote sees.  FLAT_PHONG: a compile-time fact here as in the render kernels (KY_FEAT_FLAT_PHONG).
template <bool FLAT_PHONG>
__global__ void kat_bsdf_continue_kernel(DMat M, const float* __restrict__ in12, int n, float* __restrict__ out12) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = in12 + 12 * (size_t)i;
    const f3 normal = ld3(r), wo = ld3(r + 3), wi_eval = ld3(r + 8);
    Vertex v;
    v.normal = normal;
    v.bsdf = make_bsdf(M, r[11]);
    vertex_prepare(v, wo);
    const BsdfContinue c = bsdf_continue(v, wo, r[6], r[7], FLAT_PHONG);
    f3 col; float scale, pd, abs_cos_i;
    bsdf_eval_parts(v, wo, wi_eval, col, scale, pd, abs_cos_i);
    const f3 ev = col * scale;
    float* q = out12 + 12 * (size_t)i;
    q[0] = c.wi.x; q[1] = c.wi.y; q[2] = c.wi.z; q[3] = c.weight.x; q[4] = c.weight.y; q[5] = c.weight.z;
    q[6] = c.ok ? 1.f : 0.f; q[7] = c.specular ? 1.f : 0.f; q[8] = ev.x; q[9] = ev.y; q[10] = ev.z; q[11] = pd;
}

__global__ void kat_light_kernel(const DScene* __restrict__ S, int li, const float* __restrict__ in11, int n, float* __restrict__ out11) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = in11 + 11 * (size_t)i;
    const f3 p = ld3(r), pn = ld3(r + 3), wi = ld3(r + 8);
    const LightSample ls = light_sample_Li(S->light[li], p, pn, r[6], r[7]);
    const float pdf = light_pdf_Li(S->light[li], S->full, p, pn, wi);
    float* q = out11 + 11 * (size_t)i;
    q[0] = ls.position.x; q[1] = ls.position.y; q[2] = ls.position.z; q[3] = ls.wi.x; q[4] = ls.wi.y; q[5] = ls.wi.z;
    q[6] = ls.pdf; q[7] = ls.Li.x; q[8] = ls.Li.y; q[9] = ls.Li.z; q[10] = pdf;
}

template <bool BOXES>   // the scene has boxes (KY_FEAT_BOXES): the traversal the box kernels run
__global__ void kat_scene_intersect_kernel(const DScene* __restrict__ S_, const float* __restrict__ rays7, int n, float* __restrict__ out9) {
    const SceneRef S{S_, true, BOXES ? KY_FEAT_BOXES : 0, true};
    const LdsScene Lds = stage_scene<true>(S);   // KAT kernels: always the scene-sized dynamic block
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rays7 + 7 * (size_t)i;
    const f3 o = ld3(r), d = ld3(r + 3);
    float t = r[6];
    const int hs = trace_nearest(S, o, d, t);
    f3 p = mk3(0, 0, 0), nn = mk3(0, 0, 0);
    if (hs >= 0) { p = o + t * d; nn = hit_normal(Lds.hit[hs], p, d); }
    float* q = out9 + 9 * (size_t)i;
    q[0] = hs >= 0 ? 1.f : 0.f; q[1] = hs >= 0 ? t : 0.f;
    q[2] = p.x; q[3] = p.y; q[4] = p.z; q[5] = nn.x; q[6] = nn.y; q[7] = nn.z; q[8] = hs >= 0 ? (float)S->orig[hs] : -1.f;
}

// table: -2 every surface, -1 DScene::occ, l >= 0 what by_emitter uses for light l
__global__ void kat_occluded_kernel(const DScene* __restrict__ S, const float* __restrict__ in9, int n, float* __restrict__ out1, int table) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = in9 + 9 * (size_t)i;
    const f3 p = ld3(r), pn = ld3(r + 3), target = ld3(r + 6);
    const f3 dir = normalize(target - p);
    const float dist = sqrtf(length_sq(p - target));
    const f3 o = offset_ray_origin(p, pn, dir);
    bool occ;
    if (table >= 0) occ = light_sample_occluded(S, table, o, dir, dist - 2e-3f);
    else occ = trace_any(S, table == -1 ? S->occ : S->trav, o, dir, dist - 2e-3f);
    out1[i] = occ ? 1.f : 0.f;
}

// the environment estimate's pair scan (trace_any_pair): ray A unbounded, ray B up to tmax
template <bool BOXES>
__global__ void kat_any_pair_kernel(const DScene* __restrict__ S_, const float* __restrict__ in13, int n, float* __restrict__ out2) {
    const SceneRef S{S_, true, BOXES ? KY_FEAT_BOXES : 0, true};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = in13 + 13 * (size_t)i;
    const AnyRay A{ld3(r), ld3(r + 3), K_INF}, B{ld3(r + 6), ld3(r + 9), r[12]};
    bool occ_a, occ_b;
    trace_any_pair(S, A, B, occ_a, occ_b);
    out2[2 * (size_t)i] = occ_a ? 1.f : 0.f;
    out2[2 * (size_t)i + 1] = occ_b ? 1.f : 0.f;
}

// one light's direct-lighting estimate at given vertices with given random numbers (estimate_direct_lighting_*, 3889-4088)
__global__ void kat_nee_kernel(const DScene* __restrict__ S, int strategy, int li, const float* __restrict__ in15, int n, float* __restrict__ out6) {
    const LdsScene Lds = stage_scene<true>(S);   // KAT kernels: always the scene-sized dynamic block
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const float* r = in15 + 15 * (size_t)(active ? i : 0);
    Vertex v;
    v.position = ld3(r); v.normal = ld3(r + 3);
    v.t = 0.f;
    v.surface = 0;
    for (int j = 0; j < S->n_surfaces; ++j)
        if (S->orig[j] == (int)r[9]) v.surface = j;          // the caller's surface index -> the device's sorted index
    v.bsdf = make_bsdf(Lds.mat[Lds.hit[v.surface].material], r[10]);
    const f3 wo = ld3(r + 6);
    vertex_prepare(v, wo);
    f3 Lb = mk3(0, 0, 0), Ll = mk3(0, 0, 0);
    const bool nee = active && !bsdf_is_delta(v.bsdf);        // sample_all_light runs for non-delta vertices only (4571)
    // (wave-uniform calls: every lane makes them, `nee` says whether it takes part)
    const f3 one = mk3(1, 1, 1);   // the estimators ADD w x their estimate to an accumulator
    if (strategy == KY_DIRECT_BSDF) estimate_by_bsdf<false>(S, Lds, v, wo, li, r[11], r[12], nee, Lb, one);
    else if (strategy == KY_DIRECT_BSDF_MIS || strategy == KY_DIRECT_BOTH_MIS) estimate_by_bsdf<true>(S, Lds, v, wo, li, r[11], r[12], nee, Lb, one);
    if (nee) {
        if (strategy == KY_DIRECT_LIGHT) estimate_by_emitter<false>(S, Lds, v, wo, li, r[13], r[14], Ll, one);
        else if (strategy == KY_DIRECT_LIGHT_MIS || strategy == KY_DIRECT_BOTH_MIS) estimate_by_emitter<true>(S, Lds, v, wo, li, r[13], r[14], Ll, one);
    }
    if (active) {
        float* o = out6 + 6 * (size_t)i;
        o[0] = Lb.x; o[1] = Lb.y; o[2] = Lb.z; o[3] = Ll.x; o[4] = Ll.y; o[5] = Ll.z;
    }
}

// sample_single_light's pick and the picked light's two both_mis halves times the light count (3813-3832), the lights read per lane as the render kernels read them
__global__ void kat_single_light_kernel(const DScene* __restrict__ S, const float* __restrict__ in16, int n, float* __restrict__ out6) {
    const LdsScene Lds = stage_lights(S, stage_scene<true>(S), true);   // KAT kernels: always the scene-sized dynamic block
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const float* r = in16 + 16 * (size_t)(active ? i : 0);
    Vertex v;
    v.position = ld3(r); v.normal = ld3(r + 3);
    v.t = 0.f;
    v.surface = 0;
    for (int j = 0; j < S->n_surfaces; ++j)
        if (S->orig[j] == (int)r[9]) v.surface = j;          // the caller's surface index -> the device's sorted index
    v.bsdf = make_bsdf(Lds.mat[Lds.hit[v.surface].material], r[10]);
    const f3 wo = ld3(r + 6);
    vertex_prepare(v, wo);
    const int nl = S->n_lights;
    const int li = active ? min((int)(r[15] * (float)nl), nl - 1) : 0;   // 3821
    const DLight* Lp = Lds.light + li;
    f3 Lb = mk3(0, 0, 0), Ll = mk3(0, 0, 0);
    const bool nee = active && !bsdf_is_delta(v.bsdf);
    const float fn = (float)nl;
    const f3 w = mk3(fn, fn, fn);   // 1 / pick probability, 3830
    estimate_by_bsdf<true, true>(S, Lds, v, wo, li, r[11], r[12], nee, Lb, w, nullptr, f3{0, 0, 0}, 0.f, 0, nullptr, Lp);   // (wave-uniform call)
    if (nee) estimate_by_emitter<true, true>(S, Lds, v, wo, li, r[13], r[14], Ll, w, Lp);
    if (active) {
        float* o = out6 + 6 * (size_t)i;
        o[0] = Lb.x; o[1] = Lb.y; o[2] = Lb.z; o[3] = Ll.x; o[4] = Ll.y; o[5] = Ll.z;
    }
}

// sample_single_light's pick by power and by position: kat_single_light_kernel's rows, the light picked by pick_light as the render kernels call it.  `out18` (may
// be null): {li, p[li], every light's p from the same weight function one light at a time}; `out6` (may be null): the picked light's two both_mis halves over p[li].
static __device__ Vertex kat_pick_vertex(const DScene* __restrict__ S, const LdsScene& Lds, const float* r) {
    Vertex v;
    v.position = ld3(r); v.normal = ld3(r + 3);
    v.t = 0.f;
    v.surface = 0;
    for (int j = 0; j < S->n_surfaces; ++j)
        if (S->orig[j] == (int)r[9]) v.surface = j;          // the caller's surface index -> the device's sorted index
    v.bsdf = make_bsdf(Lds.mat[Lds.hit[v.surface].material], r[10]);
    vertex_prepare(v, ld3(r + 6));
    return v;
}
__global__ void kat_light_pick_kernel(const DScene* __restrict__ S, int rule, const float* __restrict__ in16, int n, float* __restrict__ out18, float* __restrict__ out6) {
    const LdsScene Lds = stage_lights(S, stage_scene<true>(S), true);   // KAT kernels: always the scene-sized dynamic block
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const float* r = in16 + 16 * (size_t)(active ? i : 0);
    const Vertex v = kat_pick_vertex(S, Lds, r);
    const f3 wo = ld3(r + 6);
    const int nl = S->n_lights;
    const float u = r[15];
    int li = min((int)(u * (float)nl), nl - 1);   // 3821
    float p = rcp((float)nl);
    if (rule == KY_PICK_POWER) pick_light<KY_PICK_POWER>(S, v, wo, u, nl, li, p);
    else if (rule == KY_PICK_SPATIAL) pick_light<KY_PICK_SPATIAL>(S, v, wo, u, nl, li, p);
    if (out18 && active) {
        float* o = out18 + 18 * (size_t)i;
        o[0] = (float)li; o[1] = p;
        for (int k = 0; k < KYHIP_MAX_LIGHTS; ++k) o[2 + k] = 0.f;
        if (rule == KY_PICK_SPATIAL && nl > 1) {
            const PickVertex pv = pick_vertex(v, wo);
            float W = 0.f;
            for (int k = 0; k < nl; ++k) W += pick_light_weight(S, pv, k);
            for (int k = 0; k < nl; ++k)
                o[2 + k] = W > 0.f ? KY_PICK_UNIFORM_SHARE * rcp((float)nl) + (1.f - KY_PICK_UNIFORM_SHARE) * (pick_light_weight(S, pv, k) * rcp(W)) : rcp((float)nl);
        } else {
            for (int k = 0; k < nl; ++k) o[2 + k] = nl == 1 ? 1.f : (rule == KY_PICK_POWER ? S->pick.power_p[k] : rcp((float)nl));
        }
    }
    if (out6) {
        const DLight* Lp = Lds.light + (active ? li : 0);
        f3 Lb = mk3(0, 0, 0), Ll = mk3(0, 0, 0);
        const bool nee = active && !bsdf_is_delta(v.bsdf);
        const float fn = rcp(p);   // 1 / pick probability, 3830
        const f3 w = mk3(fn, fn, fn);
        estimate_by_bsdf<true, true>(S, Lds, v, wo, li, r[11], r[12], nee, Lb, w, nullptr, f3{0, 0, 0}, 0.f, 0, nullptr, Lp);   // (wave-uniform call)
        if (nee) estimate_by_emitter<true, true>(S, Lds, v, wo, li, r[13], r[14], Ll, w, Lp);
        if (active) {
            float* o = out6 + 6 * (size_t)i;
            o[0] = Lb.x; o[1] = Lb.y; o[2] = Lb.z; o[3] = Ll.x; o[4] = Ll.y; o[5] = Ll.z;
        }
    }
}

// the bit patterns of the first k numbers of the stream the render kernels give the key (seed, pixel_index, sample_index): sampler_pixel_key, sampler_start
// and sampler_next as path_begin calls them.  One thread per key; its k words lie together.
template <bool DEBUG_SAMPLER>
__global__ void kat_sampler_kernel(uint32_t seed, const uint32_t* __restrict__ keys2, int n, int k, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Sampler smp;
    sampler_start(smp, sampler_pixel_key(seed, keys2[2 * (size_t)i]), keys2[2 * (size_t)i + 1]);
    uint32_t* q = out + (size_t)i * (size_t)k;
    for (int j = 0; j < k; ++j) q[j] = __float_as_uint(sampler_next<DEBUG_SAMPLER>(smp));
}
// ... of the stratified sampler: sampler_start_kind and sampler_next as the render kernels' later draws call them, or -- camera != 0 -- the first two through
// sampler_camera, which is how path_begin draws them
__global__ void kat_sampler_stratified_kernel(uint32_t seed, RenderConstS rc, int camera, const uint32_t* __restrict__ keys2, int n, int k, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    StratSampler smp;
    sampler_bind(smp, rc);
    sampler_start_kind<KY_SMP_STRATIFIED>(smp, sampler_pixel_key(seed, keys2[2 * (size_t)i]), keys2[2 * (size_t)i + 1]);
    uint32_t* q = out + (size_t)i * (size_t)k;
    int j = 0;
    if (camera && k >= 2) {
        float u0, u1;
        sampler_camera<KY_SMP_STRATIFIED>(smp, u0, u1);
        q[0] = __float_as_uint(u0); q[1] = __float_as_uint(u1);
        j = 2;
    }
    for (; j < k; ++j) q[j] = __float_as_uint(sampler_next<KY_SMP_STRATIFIED>(smp));
}

// the lens's disk map alone, as path_begin applies it to a camera sample's third and fourth numbers
__global__ void kat_lens_kernel(const float* __restrict__ u2, int n, float* __restrict__ out2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lens_disk(u2[2 * (size_t)i], u2[2 * (size_t)i + 1], out2[2 * (size_t)i], out2[2 * (size_t)i + 1]);
}
// a pixel filter's warp alone, as path_begin applies it to each of a camera sample's two numbers; `table`: KYHIP_FILTER_TABLE + 1 floats
__global__ void kat_filter_kernel(FilterConst fc, const float* __restrict__ u, int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = filter_offset(fc, u[i]);
}

// ---- the per-sample replay: one camera sample's radiance by the walk of the render kernel that rendered it, written once ----
// What a launch decides and its replay has to decide alike are the five template arguments:
//   SAMPLER  the sampler kind; its launch constants are RenderConstFor<SAMPLER>, wider by the strata for KY_SMP_STRATIFIED.
//   BOXES    the launch runs a kernel with the box traversal (render_uses_boxes): the replay takes the same one, to the last decision (a ray along a box's edge may
//            take the other face in the other traversal).  single_env, a run-time flag since these kernels are not timed, likewise: the launch's both_mis estimate
//            is estimate_env_both (KY_FEAT_SINGLE_ENV).
//   DROP     0, or -1 for a masked launch (kyhip_render_lighting), whose drop bits `drop` are read at run time (path_intersect, ky_device.hpp); the stratified
//            sampler's forms always read them.  Which products contract to an fma differs between the two, so an unmasked replay keeps the compile-time 0.
//   CAM      KY_CAM_FILTER: the launch runs under a pixel filter (rc_.filter): the filtered render kernels assume no scene facts (no box traversal, no pair scan),
//            and so does this.  KY_CAM_LENS: ... and under a lens (rc_.lens; the filter may then be the box).  KY_CAM_PLAIN otherwise.
//   TRACE    one sample, s0, traced vertex by vertex into out[4..] (`n` rows at most) behind {rows, Lo}: lane 0 walks the path, the other lanes only keep the
//            wave-uniform calls company.  Otherwise lane i < n walks sample s0 + i and writes out[3 i ..].
template <int SAMPLER, int CAM> struct ReplayConstFor { typedef typename RenderConstFor<SAMPLER>::type type; };
template <int SAMPLER> struct ReplayConstFor<SAMPLER, KY_CAM_FILTER> { typedef RenderConstF type; };
template <int SAMPLER> struct ReplayConstFor<SAMPLER, KY_CAM_LENS> { typedef RenderConstL type; };

template <int SAMPLER, bool BOXES, int DROP, int CAM, bool TRACE>
__global__ void kat_li_kernel(const DScene* __restrict__ S_, typename ReplayConstFor<SAMPLER, CAM>::type rc_, int x, int y, int s0, int n, float* __restrict__ out, int single_env, int drop) {
    const SceneRef S{S_, true, CAM != KY_CAM_PLAIN ? 0 : (BOXES ? KY_FEAT_BOXES : 0) | (single_env ? KY_FEAT_SINGLE_ENV : 0), true};
    const typename RenderConstFor<SAMPLER>::type& rc = rc_;
    const LdsScene Lds = stage_lights(S, stage_scene<true>(S), ky_direct_is_single(rc.strategy));   // KAT kernels: always the scene-sized dynamic block
    const int i = TRACE ? 0 : blockIdx.x * blockDim.x + threadIdx.x;
    PathStateFor<SAMPLER> ps;
    sampler_bind(ps.smp, rc);
    const bool mine = TRACE ? threadIdx.x == 0 : i < n;
    bool alive = mine;
    VertexTrace tr{out + 4, n, 0};
    if (alive) {
        const uint32_t key = sampler_pixel_key(rc.seed, (uint32_t)(y * rc.width + x));
        if constexpr (CAM == KY_CAM_LENS) path_begin<SAMPLER, false, KY_CAM_LENS>(ps, S, key, x, y, s0 + i, lens_cam(rc_));
        else if constexpr (CAM == KY_CAM_FILTER) path_begin<SAMPLER, false, KY_CAM_FILTER>(ps, S, key, x, y, s0 + i, rc_.filter);
        else path_begin<SAMPLER>(ps, S, key, x, y, s0 + i);
    }
    while (__any(alive)) {  // path_shade is a wave-uniform call
        Vertex v;
        bool have_vertex = false;
        if (alive) have_vertex = path_intersect<SAMPLER, DROP>(ps, v, S, Lds, rc, drop);
        const bool cont = path_shade<SAMPLER, DROP>(ps, v, S, Lds, rc, have_vertex, -1, TRACE ? &tr : nullptr, nullptr, 0, false, false, drop);
        alive = have_vertex && cont;
    }
    if (!mine) return;
    if (TRACE) { out[0] = (float)tr.n; out[1] = ps.Lo.x; out[2] = ps.Lo.y; out[3] = ps.Lo.z; }
    else { out[3 * (size_t)i] = ps.Lo.x; out[3 * (size_t)i + 1] = ps.Lo.y; out[3 * (size_t)i + 2] = ps.Lo.z; }
}

// ... and under a texture set: the walk of the textured render kernels -- no scene facts, the one camera form KY_CAM_ANY, the vertex's
// material through vertex_material<true>.  A kernel of its own, so that every form of kat_li_kernel keeps its name and its code.
template <int SAMPLER>
__global__ void kat_li_textured_kernel(const DScene* __restrict__ S_, RenderConstT rc_, int x, int y, int s0, int n, float* __restrict__ out) {
    const SceneRef S{S_, true, 0, true};
    const typename RenderConstFor<SAMPLER>::type& rc = rc_;
    const LdsScene Lds = stage_lights(S, stage_scene<true>(S), ky_direct_is_single(rc.strategy));
    const TexLds tx = stage_textures(rc_.tex, Lds);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    PathStateFor<SAMPLER> ps;
    sampler_bind(ps.smp, rc);
    const bool mine = i < n;
    bool alive = mine;
    if (alive) path_begin<SAMPLER, false, KY_CAM_ANY>(ps, S, sampler_pixel_key(rc.seed, (uint32_t)(y * rc.width + x)), x, y, s0 + i, lens_cam(rc_));
    while (__any(alive)) {  // path_shade is a wave-uniform call
        Vertex v;
        bool have_vertex = false;
        if (alive) have_vertex = path_intersect<SAMPLER, 0>(ps, v, S, Lds, rc, 0);
        const bool cont = path_shade<SAMPLER, 0, true>(ps, v, S, Lds, rc, have_vertex, -1, nullptr, nullptr, 0, false, false, 0, &tx);
        alive = have_vertex && cont;
    }
    if (!mine) return;
    out[3 * (size_t)i] = ps.Lo.x; out[3 * (size_t)i + 1] = ps.Lo.y; out[3 * (size_t)i + 2] = ps.Lo.z;
}
// the known-answer probe of the texture code: (u', v', r, g, b) at world points of (sorted) surface `surface` under texture `ti`, through tex_at
__global__ void kat_texture_kernel(TexConst tc, int ti, int surface, const float* __restrict__ points3, int n, float* __restrict__ out5) {
    __shared__ __attribute__((aligned(16))) DTex tex[KYHIP_MAX_TEXTURES];
    if (threadIdx.x < KYHIP_MAX_TEXTURES) tex[threadIdx.x] = tc.set->tex[threadIdx.x];
    __syncthreads();
    const TexLds tx{tex, tc.set->uv, tc.texels};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float us, vs;
    const f3 col = tex_at(tx, ti, surface, mk3(points3[3 * (size_t)i], points3[3 * (size_t)i + 1], points3[3 * (size_t)i + 2]), us, vs);
    float* q = out5 + 5 * (size_t)i;
    q[0] = us; q[1] = vs; q[2] = col.x; q[3] = col.y; q[4] = col.z;
}

// ---- shared drivers of the KAT entry points ----
template <typename F>
static int kat_run(int device, const void* in, size_t in_bytes, void* out, size_t out_bytes, F launch) {
    DeviceCtx* c;
    int rcode = get_ctx(device, &c);
    if (rcode != KY_OK) return rcode;
    std::lock_guard<std::mutex> lock(c->m);
    DevBuf d_in, d_out;
    HIP_TRY(d_in.alloc(in_bytes));
    HIP_TRY(d_out.alloc(out_bytes));
    HIP_TRY(hipDeviceSynchronize());   // KAT entries use the default stream and may replace the device's scene copy
    HIP_TRY(hipMemcpy(d_in.p, in, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_out.p, 0, out_bytes));
    rcode = launch(c, d_in.as<const float>(), d_out.as<float>());
    if (rcode != KY_OK) return rcode;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return KY_OK;
}

// kat_run for the kernels that read a scene: uploads it and hands `launch` the device's copy, the packed host copy (what it holds) and the bytes of the scene-sized
// dynamic LDS block
template <typename F>
static int kat_run_scene(int device, const ky_scene* scene, const void* in, size_t in_bytes, void* out, size_t out_bytes, F launch) {
    return kat_run(device, in, in_bytes, out, out_bytes, [&](DeviceCtx* c, const float* d_in, float* d_out) {
        SceneSlot* sc; int r = upload_scene(c, scene, 0, &sc);
        if (r != KY_OK) return r;
        launch((const DScene*)sc->d, (const DScene*)sc->h, (size_t)lds_scene_bytes(scene->surface_count, scene->material_count, scene->light_count), d_in, d_out);
        return (int)KY_OK;
    });
}

// ---- the replay's host side: one shared refusal, one launch ----
// what the four replay entries refuse alike, each after its own checks: samples s0 .. s0 + n - 1 of pixel (x, y) of a launch of p (valid: the caller has checked)
static int replay_check(const ky_scene* scene, const ky_render_params* p, int x, int y, int s0, int n, const float* out) {
    if (!scene || !out || n <= 0 || x < 0 || y < 0 || x >= p->width || y >= p->height) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    return strat_samples_check(p, s0, n);
}

struct ReplayLaunch {   // kat_li_kernel's grid and arguments
    dim3 grid, block;
    size_t lds;
    const DScene* S;
    RenderConstL rc;   // (a kernel without a lens, a filter or strata takes the base it declares)
    int x, y, s0, n;
    float* out;
    int boxes, single_env, drop;
};
template <int SAMPLER, int DROP, bool TRACE, int CAM = KY_CAM_PLAIN>
static void replay_launch(const ReplayLaunch& a) {   // (under a filter or a lens both lines name the one form without boxes)
    constexpr bool FILTER = CAM != KY_CAM_PLAIN;
    if (!FILTER && a.boxes) hipLaunchKernelGGL((kat_li_kernel<SAMPLER, !FILTER, DROP, CAM, TRACE>), a.grid, a.block, a.lds, 0, a.S, a.rc, a.x, a.y, a.s0, a.n, a.out, a.single_env, a.drop);
    else hipLaunchKernelGGL((kat_li_kernel<SAMPLER, false, DROP, CAM, TRACE>), a.grid, a.block, a.lds, 0, a.S, a.rc, a.x, a.y, a.s0, a.n, a.out, a.single_env, a.drop);
}

// Replays samples s0 .. s0 + n - 1 of pixel (x, y) of a launch of `p` into out[3 n] -- trace: sample s0 alone into out[4 + 26 n], n rows at most -- with the form of
// kat_li_kernel that launch's kernel corresponds to; these are all the forms there are.  masked: the launch has a lighting plan with drop bits `drop` (0 otherwise);
// filter: its pixel filter, null for none (the callers hand a box filter and the debug sampler on without one); lens: its lens, null for the pinhole (likewise).
static int replay_run(int device, const ky_scene* scene, const ky_render_params* p, bool masked, int drop, const ky_pixel_filter* filter, bool trace,
                      int x, int y, int s0, int n, float* out, size_t out_bytes, const ky_lens* lens = nullptr) {
    float table[KYHIP_FILTER_TABLE + 1] = {0.f};
    if (filter) filter_table(filter, table);
    const bool dbg = p->sampler == KY_SAMPLER_DEBUG, strat = p->sampler == KY_SAMPLER_STRATIFIED;
    return kat_run_scene(device, scene, table, filter ? sizeof table : 4, out, out_bytes, [&](const DScene* S, const DScene* packed, size_t lds, const float* d_in, float* d_out) {
        ReplayLaunch a{dim3(trace ? 1 : (n + 255) / 256), dim3(trace ? 64 : 256), lds, S, RenderConstL{}, x, y, s0, n, d_out, 0, 0, drop};
        static_cast<RenderConstS&>(a.rc) = make_rc(p);
        if (lens) {   // (the filter's constants beside the lens's, the box's where there is no filter)
            if (filter) a.rc.filter = FilterConst{filter->kind, filter->radius, filter_grow(filter), d_in};
            a.rc.lens = lens_const(&scene->camera, lens);
            return strat ? replay_launch<KY_SMP_STRATIFIED, 0, false, KY_CAM_LENS>(a) : replay_launch<KY_SMP_RANDOM, 0, false, KY_CAM_LENS>(a);
        }
        if (filter) {
            a.rc.filter = FilterConst{filter->kind, filter->radius, filter_grow(filter), d_in};
            return strat ? replay_launch<KY_SMP_STRATIFIED, 0, false, KY_CAM_FILTER>(a) : replay_launch<KY_SMP_RANDOM, 0, false, KY_CAM_FILTER>(a);
        }
        const int rf = render_replay_feat(scene, p, packed, drop);
        a.boxes = (rf & KY_FEAT_BOXES) != 0;
        a.single_env = (rf & KY_FEAT_SINGLE_ENV) ? 1 : 0;
        if (trace) return strat ? replay_launch<KY_SMP_STRATIFIED, 0, true>(a) : dbg ? replay_launch<KY_SMP_DEBUG, 0, true>(a) : replay_launch<KY_SMP_RANDOM, 0, true>(a);
        if (strat) return replay_launch<KY_SMP_STRATIFIED, -1, false>(a);
        if (masked) return dbg ? replay_launch<KY_SMP_DEBUG, -1, false>(a) : replay_launch<KY_SMP_RANDOM, -1, false>(a);
        return dbg ? replay_launch<KY_SMP_DEBUG, 0, false>(a) : replay_launch<KY_SMP_RANDOM, 0, false>(a);
    });
}

extern "C" {

// ---- KAT entry points ----
int kyhip_kat_intersect(int device, const ky_shape* shape, const float* rays7, int n, float* out8) {
    if (!shape || !rays7 || !out8 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (shape->kind < KY_SHAPE_DISK || shape->kind > KY_SHAPE_SPHERE) return fail(KY_ERR_INVALID_VALUE, "unknown shape kind");
    if (!shape_normal_ok(*shape)) return fail(KY_ERR_INVALID_VALUE, "the stored normal must be unit length");
    KatShape ks{};
    pack_shape(*shape, 0, &ks.surf, &ks.full);
    cp3(ks.hit.n, shape->kind == KY_SHAPE_SPHERE ? shape->p[0] : shape->normal);
    ks.hit.kind = shape->kind;
    return kat_run(device, rays7, (size_t)n * 7 * 4, out8, (size_t)n * 8 * 4, [&](DeviceCtx*, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_intersect_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, ks, d_in, n, d_out);
        return (int)KY_OK;
    });
}

int kyhip_kat_camera(int device, const ky_camera* camera, const float* p_film2, int n, float* out6) {
    if (!camera || !p_film2 || !out6 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    ky_scene sc{};
    sc.environment_light = -1;
    sc.camera = *camera;
    if (!(camera->resolution[0] > 0) || !(camera->resolution[1] > 0)) return fail(KY_ERR_INVALID_VALUE, "bad camera resolution");
    return kat_run_scene(device, &sc, p_film2, (size_t)n * 2 * 4, out6, (size_t)n * 6 * 4, [&](const DScene* S, const DScene*, size_t, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_camera_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, S, d_in, n, d_out);
    });
}

int kyhip_kat_bsdf(int device, const ky_material* m, const float* in12, int n, float* out13) {
    if (!m || !in12 || !out13 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (m->kind < KY_MATERIAL_MATTE || m->kind > KY_MATERIAL_PLASTIC) return fail(KY_ERR_INVALID_VALUE, "unknown material kind");
    DMat d{};
    pack_material(*m, &d);
    return kat_run(device, in12, (size_t)n * 12 * 4, out13, (size_t)n * 13 * 4, [&](DeviceCtx*, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_bsdf_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d, d_in, n, d_out);
        return (int)KY_OK;
    });
}

// kyhip_kat_bsdf's rows through bsdf_continue and bsdf_eval_parts
int kyhip_kat_bsdf_continue(int device, const ky_material* m, const float* in12, int n, int flat_phong, float* out12) {
    if (!m || !in12 || !out12 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (m->kind < KY_MATERIAL_MATTE || m->kind > KY_MATERIAL_PLASTIC) return fail(KY_ERR_INVALID_VALUE, "unknown material kind");
    DMat d{};
    pack_material(*m, &d);
    return kat_run(device, in12, (size_t)n * 12 * 4, out12, (size_t)n * 12 * 4, [&](DeviceCtx*, const float* d_in, float* d_out) {
        if (flat_phong) hipLaunchKernelGGL(kat_bsdf_continue_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, 0, d, d_in, n, d_out);
        else hipLaunchKernelGGL(kat_bsdf_continue_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, 0, d, d_in, n, d_out);
        return (int)KY_OK;
    });
}

int kyhip_kat_light(int device, const ky_scene* scene, int light, const float* in11, int n, float* out11) {
    if (!scene || !in11 || !out11 || n <= 0 || light < 0 || light >= scene->light_count) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    return kat_run_scene(device, scene, in11, (size_t)n * 11 * 4, out11, (size_t)n * 11 * 4, [&](const DScene* S, const DScene*, size_t, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_light_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, S, light, d_in, n, d_out);
    });
}

int kyhip_kat_scene_intersect(int device, const ky_scene* scene, const float* rays7, int n, float* out9) {
    if (!scene || !rays7 || !out9 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    return kat_run_scene(device, scene, rays7, (size_t)n * 7 * 4, out9, (size_t)n * 9 * 4, [&](const DScene* S, const DScene* packed, size_t lds, const float* d_in, float* d_out) {
        if (packed->feat & KY_FEAT_BOXES) hipLaunchKernelGGL(kat_scene_intersect_kernel<true>, dim3((n + 255) / 256), dim3(256), lds, 0, S, d_in, n, d_out);
        else hipLaunchKernelGGL(kat_scene_intersect_kernel<false>, dim3((n + 255) / 256), dim3(256), lds, 0, S, d_in, n, d_out);
    });
}

static int kat_occluded_impl(int device, const ky_scene* scene, const float* in9, int n, float* out1, int table) {
    if (!scene || !in9 || !out1 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (table >= scene->light_count) return fail(KY_ERR_INVALID_VALUE, "light %d out of range", table);
    return kat_run_scene(device, scene, in9, (size_t)n * 9 * 4, out1, (size_t)n * 4, [&](const DScene* S, const DScene*, size_t, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_occluded_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, S, d_in, n, d_out, table);
    });
}
int kyhip_kat_occluded(int device, const ky_scene* scene, const float* in9, int n, float* out1) { return kat_occluded_impl(device, scene, in9, n, out1, -2); }
int kyhip_kat_occluded_between(int device, const ky_scene* scene, int light, const float* in9, int n, float* out1) {
    if (light < -1) return fail(KY_ERR_INVALID_VALUE, "light %d out of range", light);
    return kat_occluded_impl(device, scene, in9, n, out1, light);
}
int kyhip_kat_any_pair(int device, const ky_scene* scene, const float* in13, int n, float* out2) {
    if (!scene || !in13 || !out2 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    return kat_run_scene(device, scene, in13, (size_t)n * 13 * 4, out2, (size_t)n * 2 * 4, [&](const DScene* S, const DScene* packed, size_t, const float* d_in, float* d_out) {
        if (packed->feat & KY_FEAT_BOXES) hipLaunchKernelGGL(kat_any_pair_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, 0, S, d_in, n, d_out);
        else hipLaunchKernelGGL(kat_any_pair_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, 0, S, d_in, n, d_out);
    });
}

int kyhip_kat_nee(int device, const ky_scene* scene, int direct_sample, int light, const float* in15, int n, float* out6) {
    if (!scene || !in15 || !out6 || n <= 0 || light < 0 || light >= scene->light_count) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (direct_sample != KY_DIRECT_BSDF && direct_sample != KY_DIRECT_LIGHT && direct_sample != KY_DIRECT_BSDF_MIS && direct_sample != KY_DIRECT_LIGHT_MIS &&
        direct_sample != KY_DIRECT_BOTH_MIS)
        return fail(KY_ERR_INVALID_VALUE, "direct_sample %d has no estimator to test", direct_sample);
    for (int i = 0; i < n; ++i) {
        const float sf = in15[15 * (size_t)i + 9];
        if (!(sf >= 0 && sf < scene->surface_count)) return fail(KY_ERR_INVALID_VALUE, "row %d: surface out of range", i);
    }
    return kat_run_scene(device, scene, in15, (size_t)n * 15 * 4, out6, (size_t)n * 6 * 4, [&](const DScene* S, const DScene*, size_t lds, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_nee_kernel, dim3((n + 255) / 256), dim3(256), lds, 0, S, direct_sample, light, d_in, n, d_out);
    });
}

static int kat_light_pick_check(const ky_scene* scene, int rule, const float* in16, int n, const float* out) {
    if (!scene || !in16 || !out || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (rule < KY_PICK_UNIFORM || rule > KY_PICK_SPATIAL) return fail(KY_ERR_INVALID_VALUE, "rule %d: 0 picks uniformly, 1 by power, 2 by position", rule);
    if (scene->light_count <= 0) return fail(KY_ERR_INVALID_VALUE, "sample_single_light picks among the scene's lights: the scene has none");
    for (int i = 0; i < n; ++i) {
        const float sf = in16[16 * (size_t)i + 9], u = in16[16 * (size_t)i + 15];
        if (!(sf >= 0 && sf < scene->surface_count)) return fail(KY_ERR_INVALID_VALUE, "row %d: surface out of range", i);
        if (!(u >= 0.f && u < 1.f)) return fail(KY_ERR_INVALID_VALUE, "row %d: pick_u outside [0, 1)", i);
    }
    return KY_OK;
}

int kyhip_kat_single_light(int device, const ky_scene* scene, const float* in16, int n, float* out6) {
    if (!scene || !in16 || !out6 || n <= 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (scene->light_count <= 0) return fail(KY_ERR_INVALID_VALUE, "sample_single_light picks among the scene's lights: the scene has none");
    for (int i = 0; i < n; ++i) {
        const float sf = in16[16 * (size_t)i + 9], u = in16[16 * (size_t)i + 15];
        if (!(sf >= 0 && sf < scene->surface_count)) return fail(KY_ERR_INVALID_VALUE, "row %d: surface out of range", i);
        if (!(u >= 0.f && u < 1.f)) return fail(KY_ERR_INVALID_VALUE, "row %d: pick_u outside [0, 1)", i);
    }
    return kat_run_scene(device, scene, in16, (size_t)n * 16 * 4, out6, (size_t)n * 6 * 4, [&](const DScene* S, const DScene*, size_t lds, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_single_light_kernel, dim3((n + 255) / 256), dim3(256), lds, 0, S, d_in, n, d_out);
    });
}

int kyhip_kat_light_pick(int device, const ky_scene* scene, int rule, const float* in16, int n, float* out18) {
    KY_TRY(kat_light_pick_check(scene, rule, in16, n, out18));
    return kat_run_scene(device, scene, in16, (size_t)n * 16 * 4, out18, (size_t)n * 18 * 4, [&](const DScene* S, const DScene*, size_t lds, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_light_pick_kernel, dim3((n + 255) / 256), dim3(256), lds, 0, S, rule, d_in, n, d_out, (float*)nullptr);
    });
}

int kyhip_kat_single_light_rule(int device, const ky_scene* scene, int rule, const float* in16, int n, float* out6) {
    KY_TRY(kat_light_pick_check(scene, rule, in16, n, out6));
    if (rule == KY_PICK_UNIFORM) return kyhip_kat_single_light(device, scene, in16, n, out6);
    return kat_run_scene(device, scene, in16, (size_t)n * 16 * 4, out6, (size_t)n * 6 * 4, [&](const DScene* S, const DScene*, size_t lds, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_light_pick_kernel, dim3((n + 255) / 256), dim3(256), lds, 0, S, rule, d_in, n, (float*)nullptr, d_out);
    });
}

// the render kernels' random-number streams by key
int kyhip_kat_sampler(int device, uint32_t seed, const uint32_t* keys2, int n, int k, int debug, uint32_t* out) {
    if (!keys2 || !out || n <= 0 || k < 1 || k > 256 || (size_t)n * (size_t)k > ((size_t)1 << 28)) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    return kat_run(device, keys2, (size_t)n * 2 * 4, out, (size_t)n * (size_t)k * 4, [&](DeviceCtx*, const float* d_in, float* d_out) {
        const dim3 grid((n + 255) / 256), block(256);
        if (debug) hipLaunchKernelGGL(kat_sampler_kernel<true>, grid, block, 0, 0, seed, (const uint32_t*)d_in, n, k, (uint32_t*)d_out);
        else hipLaunchKernelGGL(kat_sampler_kernel<false>, grid, block, 0, 0, seed, (const uint32_t*)d_in, n, k, (uint32_t*)d_out);
        return (int)KY_OK;
    });
}

// ... for any ky_sampler_kind.  The stratified sampler's first two numbers are drawn twice, draw by draw and as path_begin draws them (sampler_camera), and the entry
// fails with KY_ERR_DEVICE if the two disagree: there is one stream per key, however it is read.
int kyhip_kat_sampler_kind(int device, int kind, uint32_t seed, int spp, const uint32_t* keys2, int n, int k, uint32_t* out) {
    KY_TRY(kat_sampler_kind_check(kind, spp, keys2, n, k, out));
    if (kind != KY_SAMPLER_STRATIFIED) return kyhip_kat_sampler(device, seed, keys2, n, k, kind == KY_SAMPLER_DEBUG, out);
    ky_render_params q{};
    q.samples_per_pixel = spp;
    const RenderConstS rc = make_rc(&q);
    std::vector<uint32_t> first(k >= 2 ? (size_t)n * (size_t)k : 0);
    for (int camera = k >= 2 ? 1 : 0; camera >= 0; --camera) {
        const int rcode = kat_run(device, keys2, (size_t)n * 2 * 4, out, (size_t)n * (size_t)k * 4, [&](DeviceCtx*, const float* d_in, float* d_out) {
            hipLaunchKernelGGL(kat_sampler_stratified_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, seed, rc, camera, (const uint32_t*)d_in, n, k, (uint32_t*)d_out);
            return (int)KY_OK;
        });
        if (rcode != KY_OK) return rcode;
        if (camera) std::memcpy(first.data(), out, first.size() * sizeof(uint32_t));
    }
    if (!first.empty() && std::memcmp(first.data(), out, first.size() * sizeof(uint32_t)) != 0) return fail(KY_ERR_DEVICE, "the stratified camera sample differs between sampler_camera and sampler_next");
    return KY_OK;
}

int kyhip_kat_filter(int device, const ky_pixel_filter* filter, const float* u, int n, float* out) {
    KY_TRY(filter_check(filter));
    if (!u || !out || n <= 0 || n > (1 << 26)) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    for (int i = 0; i < n; ++i)
        if (!(u[i] >= 0.f && u[i] < 1.f)) return fail(KY_ERR_INVALID_VALUE, "u[%d] = %g outside [0, 1)", i, (double)u[i]);
    constexpr int T = KYHIP_FILTER_TABLE + 1;
    std::vector<float> in((size_t)T + (size_t)n);   // the table, then the numbers
    filter_table(filter, in.data());
    std::memcpy(in.data() + T, u, (size_t)n * sizeof(float));
    return kat_run(device, in.data(), in.size() * 4, out, (size_t)n * 4, [&](DeviceCtx*, const float* d_in, float* d_out) {
        const FilterConst fc{filter->kind, filter->kind == KY_FILTER_BOX ? 0.5f : filter->radius, filter_grow(filter), d_in};
        hipLaunchKernelGGL(kat_filter_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, fc, d_in + T, n, d_out);
        return (int)KY_OK;
    });
}

// ---- the per-sample replay (replay_run) ----
int kyhip_kat_li(int device, const ky_scene* scene, const ky_render_params* p, int x, int y, int s0, int n, float* out3) {
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params");
    KY_TRY(replay_check(scene, p, x, y, s0, n, out3));
    return replay_run(device, scene, p, false, 0, nullptr, false, x, y, s0, n, out3, (size_t)n * 3 * 4);
}

// kyhip_kat_li for the samples of a masked render: what kyhip_render_lighting(lighting) adds per camera sample, before the mean and its clamp
int kyhip_kat_li_lighting(int device, const ky_scene* scene, const ky_render_params* p, int lighting, int x, int y, int s0, int n, float* out3) {
    LightingPlan plan;
    KY_TRY(lighting_plan(p, lighting, &plan));
    if (plan.plain) return kyhip_kat_li(device, scene, p, x, y, s0, n, out3);
    KY_TRY(replay_check(scene, p, x, y, s0, n, out3));
    if (plan.nothing) { std::memset(out3, 0, (size_t)n * 3 * sizeof(float)); return KY_OK; }
    ky_render_params q = *p;
    q.max_path_depth = plan.effective_depth;
    return replay_run(device, scene, &q, true, plan.dropped, nullptr, false, x, y, s0, n, out3, (size_t)n * 3 * 4);
}

// kyhip_kat_li for the samples of a render under a pixel filter: the walk of the filtered render kernels
int kyhip_kat_li_filtered(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, int x, int y, int s0, int n, float* out3) {
    if (filter_is_box(filter)) {
        if (filter) KY_TRY(filter_check(filter));
        return kyhip_kat_li(device, scene, p, x, y, s0, n, out3);
    }
    KY_TRY(filter_check(filter));
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params");
    if (p->sampler == KY_SAMPLER_DEBUG) return kyhip_kat_li(device, scene, p, x, y, s0, n, out3);   // (0.5 is the pixel's centre under every filter)
    KY_TRY(replay_check(scene, p, x, y, s0, n, out3));
    return replay_run(device, scene, p, false, 0, filter, false, x, y, s0, n, out3, (size_t)n * 3 * 4);
}

// ... under a lens (and a pixel filter): the walk of the lens render kernels
int kyhip_kat_li_lens(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, const ky_lens* lens, int x, int y, int s0, int n, float* out3) {
    if (lens) KY_TRY(lens_check(lens));
    if (lens_is_pinhole(lens)) return kyhip_kat_li_filtered(device, scene, p, filter, x, y, s0, n, out3);
    if (filter) KY_TRY(filter_check(filter));
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params");
    if (p->sampler == KY_SAMPLER_DEBUG) return kyhip_kat_li(device, scene, p, x, y, s0, n, out3);   // ((0.5, 0.5) is the centre of every lens)
    KY_TRY(replay_check(scene, p, x, y, s0, n, out3));
    LensConst lc;
    KY_TRY(lens_const_checked(&scene->camera, lens, &lc));
    return replay_run(device, scene, p, false, 0, filter_is_box(filter) ? nullptr : filter, false, x, y, s0, n, out3, (size_t)n * 3 * 4, lens);
}

int kyhip_kat_lens(int device, const float* u2, int n, float* out2) {
    if (!u2 || !out2 || n <= 0 || n > (1 << 25)) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    for (int i = 0; i < 2 * n; ++i)
        if (!(u2[i] >= 0.f && u2[i] < 1.f)) return fail(KY_ERR_INVALID_VALUE, "u[%d] = %g outside [0, 1)", i, (double)u2[i]);
    return kat_run(device, u2, (size_t)n * 8, out2, (size_t)n * 8, [&](DeviceCtx*, const float* d_in, float* d_out) {
        hipLaunchKernelGGL(kat_lens_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, n, d_out);
        return (int)KY_OK;
    });
}

// ... under a texture set (and a pixel filter and a lens): the walk of the textured render kernels
// the set on the device for the span of one KAT call
struct KatTextures {
    DevBuf set, texels;
    TexConst tc{};
    int upload(const ky_scene* scene, const DScene* packed, const ky_texture* textures, int n) {
        std::unique_ptr<DTexSet> h(new DTexSet);
        std::vector<float> texels4;
        texture_pack(scene, packed, textures, n, h.get(), &texels4);
        HIP_TRY(set.alloc(sizeof(DTexSet)));
        HIP_TRY(texels.alloc(texels4.size() * sizeof(float)));
        HIP_TRY(hipMemcpy(set.p, h.get(), sizeof(DTexSet), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(texels.p, texels4.data(), texels4.size() * sizeof(float), hipMemcpyHostToDevice));
        tc = TexConst{set.as<const DTexSet>(), texels.as<const float4>()};
        return KY_OK;
    }
};
int kyhip_kat_li_textured(int device, const ky_scene* scene, const ky_texture* textures, int n_textures, const ky_render_params* p, const ky_pixel_filter* filter,
                          const ky_lens* lens, int x, int y, int s0, int n, float* out3) {
    KY_TRY(texture_check(scene, textures, n_textures));
    if (n_textures == 0) return kyhip_kat_li_lens(device, scene, p, filter, lens, x, y, s0, n, out3);
    if (lens) KY_TRY(lens_check(lens));
    if (filter) KY_TRY(filter_check(filter));
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params");
    if (p->sampler == KY_SAMPLER_DEBUG) return fail(KY_ERR_INVALID_VALUE, "a render under a texture set has no row for the debug sampler");
    KY_TRY(replay_check(scene, p, x, y, s0, n, out3));
    LensConst lc{0.f, 0.f, 0.f, 0.f};
    if (!lens_is_pinhole(lens)) KY_TRY(lens_const_checked(&scene->camera, lens, &lc));
    const bool filt = !filter_is_box(filter);
    float table[KYHIP_FILTER_TABLE + 1] = {0.f};
    if (filt) filter_table(filter, table);
    KatTextures kt;
    int up = KY_OK;
    const int rcode = kat_run_scene(device, scene, table, filt ? sizeof table : 4, out3, (size_t)n * 3 * 4, [&](const DScene* S, const DScene* packed, size_t lds, const float* d_in, float* d_out) {
        up = kt.upload(scene, packed, textures, n_textures);
        if (up != KY_OK) return;
        RenderConstT rc{};
        static_cast<RenderConstS&>(rc) = make_rc(p);
        if (filt) rc.filter = FilterConst{filter->kind, filter->radius, filter_grow(filter), d_in};
        rc.lens = lc;
        rc.tex = kt.tc;
        const dim3 grid((n + 255) / 256), block(256);
        if (p->sampler == KY_SAMPLER_STRATIFIED) hipLaunchKernelGGL((kat_li_textured_kernel<KY_SMP_STRATIFIED>), grid, block, lds, 0, S, rc, x, y, s0, n, d_out);
        else hipLaunchKernelGGL((kat_li_textured_kernel<KY_SMP_RANDOM>), grid, block, lds, 0, S, rc, x, y, s0, n, d_out);
    });
    return up != KY_OK ? up : rcode;
}

int kyhip_kat_texture(int device, const ky_scene* scene, const ky_texture* textures, int n_textures, int surface, const float* points3, int n_points, float* out5) {
    KY_TRY(texture_check(scene, textures, n_textures));
    if (!scene || !points3 || !out5 || n_points <= 0 || n_points > (1 << 24) || n_textures < 1) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (surface < 0 || surface >= scene->surface_count) return fail(KY_ERR_INVALID_VALUE, "surface %d out of range", surface);
    int ti = -1;
    for (int i = 0; i < n_textures; ++i)
        if (textures[i].material == scene->surfaces[surface].material) ti = i;
    if (ti < 0) return fail(KY_ERR_INVALID_VALUE, "surface %d: its material %d carries no texture of the set", surface, scene->surfaces[surface].material);
    KatTextures kt;
    int up = KY_OK;
    const int rcode = kat_run_scene(device, scene, points3, (size_t)n_points * 12, out5, (size_t)n_points * 20, [&](const DScene*, const DScene* packed, size_t, const float* d_in, float* d_out) {
        up = kt.upload(scene, packed, textures, n_textures);
        if (up != KY_OK) return;
        int sorted = -1;
        for (int j = 0; j < packed->n_surfaces; ++j)
            if (packed->orig[j] == surface) sorted = j;
        if (sorted < 0) { up = fail(KY_ERR_DEVICE, "internal: surface %d is not in the packed scene", surface); return; }
        hipLaunchKernelGGL(kat_texture_kernel, dim3((n_points + 255) / 256), dim3(256), 0, 0, kt.tc, ti, sorted, d_in, n_points, d_out);
    });
    return up != KY_OK ? up : rcode;
}

// one camera sample, traced vertex by vertex
int kyhip_kat_li_trace(int device, const ky_scene* scene, const ky_render_params* p, int x, int y, int s, float* rows26, int max_rows, float* li3) {
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params");
    if (p->integrator != KY_INTEGRATOR_PATH_TRACING_ITERATION) return fail(KY_ERR_INVALID_VALUE, "the vertex trace follows path_tracing_iteration_t");
    if (max_rows <= 0 || max_rows > 4096 || s < 0) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    KY_TRY(replay_check(scene, p, x, y, s, 1, rows26));
    std::vector<float> host((size_t)4 + (size_t)max_rows * 26, 0.f);
    const int rcode = replay_run(device, scene, p, false, 0, nullptr, true, x, y, s, max_rows, host.data(), host.size() * 4);
    if (rcode != KY_OK) return rcode;
    const int n = (int)host[0];
    std::memcpy(rows26, host.data() + 4, (size_t)n * 26 * sizeof(float));
    if (li3) { li3[0] = host[1]; li3[1] = host[2]; li3[2] = host[3]; }
    return n;
}

}  // extern "C"
