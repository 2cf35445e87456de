/*
 * ky_denoise.hpp -- the denoised picture of a frame rendered in passes (kyhip_frame_denoise ...; DESIGN.md "Denoise"): an edge-avoiding a-trous wavelet filter
 * over the frame's normalised picture, guided by the variance of each pixel's mean luminance (the quantity ky_noise.hpp's noise_value takes its square root of)
 * and by the geometry at the pixel's first hit -- or, with guide bounces, at the vertex its specular chain ends on, taps sharing the chain's key.  The arithmetic is written ONCE here, as KY_HD functions with floating-point contraction off: the device kernels
 * (ky_denoise.hip), the host-only builds (kyhostcheck_denoise, ky_hostcheck.cpp) and a NumPy restatement (tests/denoise_restatement.py) round alike.  All of it is
 * DOUBLE arithmetic on float32 inputs -- + - x /, max and comparisons, nothing transcendental: the library's fp32 division is not correctly rounded and could not
 * be restated, double division is -- and what one level hands to the next is stored as float32.  Plain C++: part of `make sanitize`.
 */
#pragma once
#include <cmath>
#include <cstdint>

#include "ky_noise.hpp"   // ky_shard.hpp, KY_NOFMA_*, noise_pixel_xy

namespace kydn {
// 16 bytes, 16-byte aligned: every buffer of the filter is read and written a whole pixel at a time
struct alignas(16) Px4 {
    float x, y, z, w;
};
// the three film-order buffers a level reads per tap:
//   colour / variance  {r, g, b, v}       the normalised picture (unclamped) and the variance of the pixel's mean luminance
//   guide A            {n.x, n.y, n.z, t} the normal as the integrator sees it and the hit distance
//   guide B            {P.x, P.y, P.z, class}
enum { KY_DN_SURFACE = 0, KY_DN_MISS = 1, KY_DN_LIGHT = 2, KY_DN_FLAGGED = 3 };   // a pixel's class; every class but 0 passes through and is nobody's tap
constexpr int KY_DN_MAX_LEVELS = 6, KY_DN_MAX_SQUARINGS = 10;
// what a level needs beside its buffers and its step
struct LevelConst {
    int width, height;
    int normal_squarings, pad_;
    double sigma_l2;        // sigma_luminance^2
    double sigma_plane;
    double pix;             // the width of a pixel at unit distance: 2 |camera.right| / width
};

// the B3 spline's taps (1 4 6 4 1) / 16 and the variance prefilter's (1 2 1) / 4, by distance from the centre (no table: nothing of a level lives in scratch)
KY_HD inline double tap5(int i) { const int k = i < 0 ? -i : i; return k == 0 ? 0.375 : k == 1 ? 0.25 : 0.0625; }
KY_HD inline double tap3(int i) { return i == 0 ? 0.5 : 0.25; }
// color_t::luminance()'s weights (ky.cpp:249-255)
KY_NOFMA_FN KY_HD inline double luminance(const Px4& c) {
    KY_NOFMA_BODY
    return 0.212671 * (double)c.x + 0.715160 * (double)c.y + 0.072169 * (double)c.z;
}

// One pixel's {r, g, b, v} from its three accumulator words, its flag word and its noise pair: the accumulator x total / n / 2^32 (what resolve_frame_kernel and
// blocks_resolve_kernel compute before their clamp; n the samples of the pixel's block), v = m2 / (batches - 1) / n with the block's own counts, 0 before the
// second batch.  A flagged pixel (class 3) holds what the flag rules pin it to (film_value, ky_film_value.hpp): it passes through.
KY_NOFMA_FN KY_HD inline Px4 gather_pixel(long long r, long long g, long long b, unsigned fl, double m2, int total_spp, int n, int batches) {
    KY_NOFMA_BODY
    Px4 o;
    const double scale = n > 0 ? (double)total_spp / (double)n : 0.0;
    float c[3] = {(float)((double)r * (1.0 / KY_FIX_SCALE) * scale), (float)((double)g * (1.0 / KY_FIX_SCALE) * scale), (float)((double)b * (1.0 / KY_FIX_SCALE) * scale)};
    if (fl & 0x1ffu) {
        for (int ch = 0; ch < 3; ++ch) {
            const bool nan = (fl >> ch) & 1u, pinf = (fl >> (3 + ch)) & 1u, ninf = (fl >> (6 + ch)) & 1u;
            float v = c[ch];
            if (pinf) v = 1.f;
            if (ninf) v = 0.f;
            if (nan || (pinf && ninf)) v = 0.f;
            c[ch] = v < 0.f ? 0.f : v > 1.f ? 1.f : v;
        }
    }
    o.x = c[0]; o.y = c[1]; o.z = c[2];
    o.w = (batches >= 2 && n > 0) ? (float)(m2 / (double)(batches - 1) / (double)n) : 0.f;
    return o;
}

KY_HD inline bool is_surface(const Px4& gb) { return gb.w == (float)KY_DN_SURFACE; }

// ---- albedo demodulation (DESIGN.md "Denoise", "Albedo"; kyhip_frame_set_albedo_grid) ----
// A frame with an albedo grid divides a class-0 pixel's colour by the pixel's albedo a = {r, g, b} before the levels and multiplies it back behind them, so the
// levels filter what the light did and not what the surface's colour did.  Both steps use a' = max(a, 1/64) per channel: the floor keeps a black albedo from
// dividing by zero, and the round trip is the identity up to two float32 roundings whatever a is.  (a NaN channel takes the floor.)
//   demodulate  c <- (float)(c / a'),  v <- (float)(v / Y(a')^2)   exact where the noise is in the irradiance and the albedo is known
//   remodulate  c <- (float)(c * a'),  v stays (nothing reads it behind the levels)
// Pixels of class 1, 2 and 3 take neither step.
KY_HD inline double albedo_floor(float a) { return a > 0.015625f ? (double)a : 0.015625; }
KY_NOFMA_FN KY_HD inline Px4 demodulate_pixel(const Px4& c, const Px4& a) {
    KY_NOFMA_BODY
    const double ax = albedo_floor(a.x), ay = albedo_floor(a.y), az = albedo_floor(a.z);
    const double ya = 0.212671 * ax + 0.715160 * ay + 0.072169 * az;   // luminance's weights
    Px4 o;
    o.x = (float)((double)c.x / ax); o.y = (float)((double)c.y / ay); o.z = (float)((double)c.z / az);
    o.w = (float)((double)c.w / (ya * ya));
    return o;
}
KY_NOFMA_FN KY_HD inline Px4 remodulate_pixel(const Px4& c, const Px4& a) {
    KY_NOFMA_BODY
    Px4 o;
    o.x = (float)((double)c.x * albedo_floor(a.x)); o.y = (float)((double)c.y * albedo_floor(a.y)); o.z = (float)((double)c.z * albedo_floor(a.z));
    o.w = c.w;
    return o;
}

// One level at pixel (x, y) with its taps `step` pixels apart: the pixel's new {r, g, b, v}.  cv, ga, gb: width x height, film order.
//   v_bar  the (1 2 1)^T (1 2 1) / 16 average of v over the class-0 neighbours at distance 1 inside the film, renormalised by the weights used
//   tap q = p + (i, j) step, i, j = -2 .. 2 in row-major (j, i) order, inside the film and class 0:
//     h  = B[i] B[j]
//     wn = max(0, n_p . n_q) squared normal_squarings times
//     wp = 1 / (1 + xp^2)^2,  xp   = n_p . (P_q - P_p) / (sigma_plane t_p pix step)
//     wl = 1 / (1 + xl2)^2,   xl2  = (Y_p - Y_q)^2 / (sigma_luminance^2 v_bar + 1e-10)
//     w  = h wn wp wl
//   c' = sum w c_q / sum w,  v' = sum w^2 v_q / (sum w)^2.  The centre tap has w = 9 / 64: sum w > 0.
// Pixels that are not class 0 pass through.
// KEYED (a frame with guide bounces, kyhip_frame_set_guide_bounces): `key` holds one specular-chain key per pixel in film order, and a class-0 pixel's taps and
// its variance prefilter's neighbours are the class-0 pixels with THE SAME KEY -- one more condition on who is a tap, no other arithmetic.  !KEYED: `key` is not
// read, and the body is what it was before keys existed.
template <bool KEYED>
KY_NOFMA_FN KY_HD inline Px4 level_pixel_t(const Px4* __restrict__ cv, const Px4* __restrict__ ga, const Px4* __restrict__ gb, const uint64_t* __restrict__ key, int x,
                                           int y, int step, const LevelConst& k) {
    KY_NOFMA_BODY
    const size_t at = (size_t)y * (size_t)k.width + (size_t)x;
    const Px4 cp = cv[at], bp = gb[at];
    if (!is_surface(bp)) return cp;
    const Px4 ap = ga[at];
    const uint64_t kp = KEYED ? key[at] : 0;
    double vw = 0.0, vs = 0.0;
    for (int j = -1; j <= 1; ++j)
        for (int i = -1; i <= 1; ++i) {
            const int qx = x + i, qy = y + j;
            if (qx < 0 || qy < 0 || qx >= k.width || qy >= k.height) continue;
            const size_t q = (size_t)qy * (size_t)k.width + (size_t)qx;
            if (!is_surface(gb[q])) continue;
            if (KEYED && key[q] != kp) continue;
            const double h = tap3(i) * tap3(j);
            vw = vw + h;
            vs = vs + h * (double)cv[q].w;
        }
    const double v_bar = vs / vw;
    const double lum_den = k.sigma_l2 * v_bar + 1e-10;
    const double plane_raw = k.sigma_plane * (double)ap.w * k.pix * (double)step;
    const double plane_den = plane_raw > 1e-300 ? plane_raw : 1e-300;
    const double yp = luminance(cp);
    const double npx = (double)ap.x, npy = (double)ap.y, npz = (double)ap.z;
    double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sv = 0.0;
    for (int j = -2; j <= 2; ++j)
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * step, qy = y + j * step;
            if (qx < 0 || qy < 0 || qx >= k.width || qy >= k.height) continue;
            const size_t q = (size_t)qy * (size_t)k.width + (size_t)qx;
            const Px4 bq = gb[q];
            if (!is_surface(bq)) continue;
            if (KEYED && key[q] != kp) continue;
            const Px4 aq = ga[q], cq = cv[q];
            const double nd = npx * (double)aq.x + npy * (double)aq.y + npz * (double)aq.z;
            double wn = nd > 0.0 ? nd : 0.0;
            for (int s = 0; s < k.normal_squarings; ++s) wn = wn * wn;
            const double dx = (double)bq.x - (double)bp.x, dy = (double)bq.y - (double)bp.y, dz = (double)bq.z - (double)bp.z;
            const double xp = (npx * dx + npy * dy + npz * dz) / plane_den;
            const double pa = 1.0 + xp * xp;
            const double wp = 1.0 / (pa * pa);
            const double dl = yp - luminance(cq);
            const double la = 1.0 + dl * dl / lum_den;
            const double wl = 1.0 / (la * la);
            const double w = tap5(i) * tap5(j) * wn * wp * wl;
            sw = sw + w;
            sr = sr + w * (double)cq.x;
            sg = sg + w * (double)cq.y;
            sb = sb + w * (double)cq.z;
            sv = sv + w * w * (double)cq.w;
        }
    Px4 o;
    o.x = (float)(sr / sw); o.y = (float)(sg / sw); o.z = (float)(sb / sw);
    o.w = (float)(sv / (sw * sw));
    return o;
}
KY_NOFMA_FN KY_HD inline Px4 level_pixel(const Px4* __restrict__ cv, const Px4* __restrict__ ga, const Px4* __restrict__ gb, int x, int y, int step, const LevelConst& k) {
    KY_NOFMA_BODY
    return level_pixel_t<false>(cv, ga, gb, nullptr, x, y, step, k);
}

// ---- specular-chain keys (DESIGN.md "Denoise", "Guides beyond the first hit") ----
// A pixel's key: digit k, 10 bits at 10 k, is ((surface + 1) << 1) | (transmitted ? 1 : 0) of the chain's k-th delta vertex (the caller's surface index); bit 62
// marks a chain the frame's guide bounces did not resolve, which keeps its first digit only and the first hit's guides.  0: the first hit is no mirror and no glass.
constexpr int KY_DN_KEY_DIGIT_BITS = 10;
constexpr uint64_t KY_DN_KEY_UNRESOLVED = (uint64_t)1 << 62;
KY_HD inline uint64_t chain_digit(int surface, bool reflected) { return ((uint64_t)(surface + 1) << 1) | (reflected ? 0u : 1u); }
KY_HD inline uint64_t chain_unresolved(uint64_t key) { return KY_DN_KEY_UNRESOLVED | (key & (((uint64_t)1 << KY_DN_KEY_DIGIT_BITS) - 1)); }

// ---- temporal reuse (DESIGN.md "Denoise", "Temporal"; kyhip_frame_denoise_temporal) ----
// A history (kyhip_history) holds, in film order, what an earlier frame of the SAME scene under another camera left: hcv {r, g, b, v} accumulated, hga {n, t} and
// hgb {P, m} -- the class slot of guide B holds the accumulated sample count m (m > 0 says "class 0, key 0"; m = 0: nobody's tap, which is all a later frame asks).
// A class-0 pixel p of the current frame (key 0 where the frame is keyed) projects its point P_p through the HISTORY's camera (o', f', r', u' as ky_camera stores
// them), takes the up to four history pixels around the landing point as taps, and blends what they hold with its own mean, weighted by sample counts:
//   d = P_p - o',  z = d . f'   (history only if z > 0)
//   a = (d . r') / (r' . r'),  b = (d . u') / (u' . u'),  sx = W (0.5 + a / z) - 0.5,  sy = H (0.5 - b / z) - 0.5     (pixel (i, j)'s centre: sx = i, sy = j)
//   i0 = floor(sx), fx = sx - i0, j0 = floor(sy), fy = sy - j0   (a landing point with no tap inside the film, -1 < sx < W and -1 < sy < H failing, takes none)
//   tap q = (i0 + di, j0 + dj), dj outer, di inner, inside the film and m_q > 0:
//     h  = (di ? fx : 1 - fx) (dj ? fy : 1 - fy)
//     wn = max(0, n_p . n_q) squared normal_squarings times
//     wp = 1 / (1 + xp^2)^2,  xp = n_p . (P_q - P_p) / max(sigma_plane t_p pix, 1e-300)          (the level's own plane and normal tests: the disocclusion test)
//     w  = h wn wp
//   sw = sum w; history is refused unless sw > 0 and sw >= min_weight
//   c_h = sum w c_q / sw,  v_h = sum w^2 v_q / sw^2,  m_h = sum w m_q / sw
//   M = min(m_h, max_history n_p),  alpha = n_p / (n_p + M)
//   c = alpha c_p + (1 - alpha) c_h,  v = alpha^2 v_p + (1 - alpha)^2 v_h,  m = n_p + M
// Without history the pixel keeps the gather's bits and m = n_p.  A pixel that is not class 0, or whose key is not 0, passes through with m = 0: it neither gives
// nor takes history (a virtual image behind a mirror does not reproject by this formula).  n_p: the samples the frame holds (one count: no blocks here).
struct TemporalConst {
    int width, height;
    int normal_squarings, has_history;   // has_history 0: the history holds no picture, nothing of its buffers is read
    double n_p;                          // the samples per pixel the current frame holds
    double max_history, sigma_plane, min_weight;
    double pix;                          // the CURRENT camera's pixel width at unit distance (denoise_pixel_width)
    ky_camera then;                      // the camera of the frame that wrote the history
};
struct TemporalPixel {
    Px4 cv, gb;   // the history's new {r, g, b, v} and {P, m}
};
template <bool KEYED>
KY_NOFMA_FN KY_HD inline TemporalPixel temporal_pixel_t(const Px4* __restrict__ cv, const Px4* __restrict__ ga, const Px4* __restrict__ gb, const uint64_t* __restrict__ key,
                                                        const Px4* __restrict__ hcv, const Px4* __restrict__ hga, const Px4* __restrict__ hgb, int x, int y,
                                                        const TemporalConst& k) {
    KY_NOFMA_BODY
    const size_t at = (size_t)y * (size_t)k.width + (size_t)x;
    const Px4 cp = cv[at], bp = gb[at];
    TemporalPixel o;
    o.cv = cp;
    o.gb = Px4{bp.x, bp.y, bp.z, 0.f};
    if (!is_surface(bp)) return o;
    if (KEYED && key[at] != 0) return o;
    o.gb.w = (float)k.n_p;
    if (!k.has_history) return o;
    const Px4 ap = ga[at];
    const double dx = (double)bp.x - (double)k.then.position[0], dy = (double)bp.y - (double)k.then.position[1], dz = (double)bp.z - (double)k.then.position[2];
    const double fx_ = (double)k.then.front[0], fy_ = (double)k.then.front[1], fz_ = (double)k.then.front[2];
    const double rx = (double)k.then.right[0], ry = (double)k.then.right[1], rz = (double)k.then.right[2];
    const double ux = (double)k.then.up[0], uy = (double)k.then.up[1], uz = (double)k.then.up[2];
    const double z = dx * fx_ + dy * fy_ + dz * fz_;
    if (!(z > 0.0)) return o;
    const double a = (dx * rx + dy * ry + dz * rz) / (rx * rx + ry * ry + rz * rz);
    const double b = (dx * ux + dy * uy + dz * uz) / (ux * ux + uy * uy + uz * uz);
    const double sx = (double)k.width * (0.5 + a / z) - 0.5;
    const double sy = (double)k.height * (0.5 - b / z) - 0.5;
    if (!(sx > -1.0 && sx < (double)k.width && sy > -1.0 && sy < (double)k.height)) return o;   // (also a NaN: no tap inside the film)
    const double fi = floor(sx), fj = floor(sy);
    const double fx = sx - fi, fy = sy - fj;
    const int i0 = (int)fi, j0 = (int)fj;
    const double plane_raw = k.sigma_plane * (double)ap.w * k.pix;
    const double plane_den = plane_raw > 1e-300 ? plane_raw : 1e-300;
    const double npx = (double)ap.x, npy = (double)ap.y, npz = (double)ap.z;
    double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sv = 0.0, sm = 0.0;
    for (int dj = 0; dj <= 1; ++dj)
        for (int di = 0; di <= 1; ++di) {
            const int qx = i0 + di, qy = j0 + dj;
            if (qx < 0 || qy < 0 || qx >= k.width || qy >= k.height) continue;
            const size_t q = (size_t)qy * (size_t)k.width + (size_t)qx;
            const Px4 bq = hgb[q];
            if (!(bq.w > 0.f)) continue;
            const Px4 aq = hga[q], cq = hcv[q];
            const double h = (di ? fx : 1.0 - fx) * (dj ? fy : 1.0 - fy);
            const double nd = npx * (double)aq.x + npy * (double)aq.y + npz * (double)aq.z;
            double wn = nd > 0.0 ? nd : 0.0;
            for (int s = 0; s < k.normal_squarings; ++s) wn = wn * wn;
            const double ex = (double)bq.x - (double)bp.x, ey = (double)bq.y - (double)bp.y, ez = (double)bq.z - (double)bp.z;
            const double xp = (npx * ex + npy * ey + npz * ez) / plane_den;
            const double pa = 1.0 + xp * xp;
            const double wp = 1.0 / (pa * pa);
            const double w = h * wn * wp;
            sw = sw + w;
            sr = sr + w * (double)cq.x;
            sg = sg + w * (double)cq.y;
            sb = sb + w * (double)cq.z;
            sv = sv + w * w * (double)cq.w;
            sm = sm + w * (double)bq.w;
        }
    if (!(sw > 0.0 && sw >= k.min_weight)) return o;
    const double m_h = sm / sw, m_cap = k.max_history * k.n_p;
    const double M = m_h < m_cap ? m_h : m_cap;
    const double alpha = k.n_p / (k.n_p + M), beta = 1.0 - alpha;
    o.cv.x = (float)(alpha * (double)cp.x + beta * (sr / sw));
    o.cv.y = (float)(alpha * (double)cp.y + beta * (sg / sw));
    o.cv.z = (float)(alpha * (double)cp.z + beta * (sb / sw));
    o.cv.w = (float)(alpha * alpha * (double)cp.w + beta * beta * (sv / (sw * sw)));
    o.gb.w = (float)(k.n_p + M);
    return o;
}

// ---- the kernels (ky_denoise.hip); every pointer is device memory, `stream` a hipStream_t ----
constexpr int KY_DN_BLOCK = 256;
// guides of the whole film, traced once per frame: ga = {n, t}, gb = {P, class 0 / 1 / 2}.  Uploads the scene, enqueues and WAITS (the scene cache's slot is held
// by the context's lock until the kernel is done).
int denoise_guides_device(int device, const ky_scene* scene, int width, int height, void* ga, void* gb, void* stream);
// ... of a frame with guide bounces 1 .. KYHIP_GUIDE_MAX_BOUNCES: the camera ray followed through mirrors and glass (every sampler number 0.5) to the first surface
// that is neither, whose guides the pixel takes with t summed along the chain; `key`: width x height uint64_t, the chain's key.  Uploads, enqueues and WAITS alike.
int denoise_chain_guides_device(int device, const ky_scene* scene, int width, int height, int bounces, void* ga, void* gb, void* key, void* stream);
// compact tile order -> film order: cv = gather_pixel, gb = the traced guide with the class the frame's state gives it (3: flagged; 1: a block at 0 samples)
// (blocks: NULL, or the kyb::BlockState of every block of a frame that retires blocks, whose pixels stand at their block's own counts)
int denoise_gather_device(const void* ws, const void* noise_state, const void* blocks, const ShardConst& sh, int width, int height, int total_spp, int n_done, int batches,
                          const void* gb_traced, void* cv, void* gb, void* stream);
int denoise_level_device(const void* cv_in, void* cv_out, const void* ga, const void* gb, int step, const LevelConst& k, void* stream);
// the keyed level (level_pixel_t<true>): 8 more bytes per tap
int denoise_level_keyed_device(const void* cv_in, void* cv_out, const void* ga, const void* gb, const void* key, int step, const LevelConst& k, void* stream);
// clamp01 per channel and ADD into a film (device memory, or the device alias of a pinned host film): film_t::add_color
int denoise_add_device(const void* cv, float* film, size_t stride_px, int width, int height, void* stream);
// ---- of a frame with an albedo grid (kyhip_frame_set_albedo_grid) ----
constexpr int KY_DN_ALBEDO_MAX_GRID = KYHIP_ALBEDO_MAX_GRID;
// The albedo of the whole film, traced once per frame: `albedo` = width x height Px4 {r, g, b, w}, the mean over grid x grid camera rays per pixel of the colour
// the ray's specular chain (bounces 0 .. KYHIP_GUIDE_MAX_BOUNCES) ends on, and the number of them that ended on a surface that carries no lamp.  cam: the frame's
// camera form (the pixel filter and the lens as its passes carry them), tex: its texture set (set == NULL: none).  Uploads, enqueues and WAITS like the guides.
int denoise_albedo_device(int device, const ky_scene* scene, int width, int height, int bounces, int grid, const kyd::LensCam& cam, const kyd::TexConst& tex, void* albedo,
                          void* stream);
// denoise_gather_device that demodulates the class-0 pixels by `albedo` (demodulate_pixel), and denoise_add_device that remodulates them before the clamp
// (remodulate_pixel; gb: the classes the gather wrote)
int denoise_gather_albedo_device(const void* ws, const void* noise_state, const void* blocks, const ShardConst& sh, int width, int height, int total_spp, int n_done,
                                 int batches, const void* gb_traced, const void* albedo, void* cv, void* gb, void* stream);
int denoise_add_albedo_device(const void* cv, const void* gb, const void* albedo, float* film, size_t stride_px, int width, int height, void* stream);
// ---- temporal reuse (kyhip_frame_denoise_temporal) ----
// temporal_pixel_t over the film: the frame's cv / ga / gb (key: NULL, or the chain keys of a frame with guide bounces) and the history's OLD side (hcv, hga, hgb;
// not read when k.has_history is 0) -> the history's NEW side: ncv = the blended {r, g, b, v}, nga = the frame's {n, t}, ngb = {P, m}
int denoise_temporal_device(const void* cv, const void* ga, const void* gb, const void* key, const void* hcv, const void* hga, const void* hgb, void* ncv, void* nga,
                            void* ngb, const TemporalConst& k, void* stream);
}  // namespace kydn
