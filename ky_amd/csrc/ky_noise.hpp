/*
 * ky_noise.hpp -- a per-pixel noise estimate for a frame rendered in passes (kyhip_frame_track_noise ...; DESIGN.md "Noise").  A frame's accumulators change
 * by whole chunks only, so the difference between them after two passes is an exact batch sum: the estimator is batch means over the passes, kept per pixel as
 * the luminance sum at the last update and West's weighted sum of squares, 16 bytes.  The arithmetic is written ONCE here, as KY_HD functions with
 * floating-point contraction off: the device kernels (ky_noise.hip), the sanitizer build (kyhostcheck_noise, ky_hostcheck.cpp) and a NumPy restatement
 * (tests/test_noise.py) round alike.  Plain C++: part of `make sanitize`.
 */
#pragma once
#include <cmath>
#include <cstdint>

#include "ky_shard.hpp"

// no fused multiply-add in these functions, whatever the translation unit's flags say
#if defined(__clang__)
#define KY_NOFMA_FN
#define KY_NOFMA_BODY _Pragma("clang fp contract(off)")
#else
#define KY_NOFMA_FN __attribute__((optimize("fp-contract=off")))
#define KY_NOFMA_BODY
#endif

namespace kyn {
struct NoisePixel {
    double y_prev;   // the luminance sum of the samples done at the last update
    double m2;       // sum over the batches of n_k (batch mean - running mean)^2
};
// what a tracking frame's checkpoint appends to the state: this, then n_pix NoisePixel
struct NoiseTrailer {
    uint64_t magic;              // KY_NOISE_MAGIC
    int32_t batches, n_prev;     // updates so far; the samples done at the last one
};
constexpr uint64_t KY_NOISE_MAGIC = 0x314553494f4e4b59ull;   // "YKNOISE1"
enum { KY_NOISE_INSIDE = 0, KY_NOISE_FLAGGED = 1, KY_NOISE_PADDING = 2 };   // a pixel's class (noise_map_kernel)
// what the statistics kernels reduce: over the pixels inside the film
struct NoiseSums {
    long long pixels, flagged, above;
    double sum;
    float max;
    int pad_;
};

// color_t::luminance() (ky.cpp:249-255) of an accumulator triple, times total_spp: the chunk sums were scaled by 1 / total, so this is the SUM of the samples' luminances
KY_NOFMA_FN KY_HD inline double noise_luminance(long long r, long long g, long long b, int total_spp) {
    KY_NOFMA_BODY
    const double y = 0.212671 * (double)r + 0.715160 * (double)g + 0.072169 * (double)b;
    return y / 4294967296.0 * (double)total_spp;
}
// One batch: the samples (n_prev, n_now] with luminance sum y_now - y_prev.  West's weighted update: it never goes negative and has no Q - Y^2 / N cancellation.
// The first batch (n_prev == 0) adds 0.
KY_NOFMA_FN KY_HD inline void noise_update(NoisePixel& px, double y_now, int n_prev, int n_now) {
    KY_NOFMA_BODY
    if (n_prev > 0 && n_now > n_prev) {
        const double n = (double)(n_now - n_prev);
        const double d = y_now - px.y_prev;
        const double t = d / n - px.y_prev / (double)n_prev;
        const double w = n * (double)n_prev / (double)n_now;
        px.m2 = px.m2 + w * (t * t);
    }
    px.y_prev = y_now;
}
// Two estimates of one pixel over DISJOINT samples become one (a merge of two frames' sample ranges, ky_merge.hip; DESIGN.md "Slices"): a stands at n_a samples,
// b at n_b, y_merged is noise_luminance of the merged words.  noise_update's step with a batch that has a spread of its own (Chan's pairwise form of West's
// update): with b.m2 == 0 it IS noise_update(a, a.y_prev + b.y_prev, n_a, n_a + n_b) in m2, bit for bit.  With a count of 0 the other pair's m2 is taken.  y_prev
// becomes y_merged, not a.y_prev + b.y_prev: the next pass's batch difference is then exact.  Not symmetric in its last bits (mean_b - mean_a, a.m2 + b.m2 first):
// which frame receives and in which order it merges shows in m2's rounding, never in the words.
KY_NOFMA_FN KY_HD inline void noise_merge(NoisePixel& a, int n_a, const NoisePixel& b, int n_b, double y_merged) {
    KY_NOFMA_BODY
    if (n_a > 0 && n_b > 0) {
        const double w = (double)n_a * (double)n_b / (double)(n_a + n_b);
        const double t = b.y_prev / (double)n_b - a.y_prev / (double)n_a;
        a.m2 = a.m2 + b.m2 + w * (t * t);
    } else if (n_a <= 0) {
        a.m2 = b.m2;
    }
    a.y_prev = y_merged;
}
// One pixel of a merge, as ky_merge.hip's kernel and kyhostcheck_merge run it: the three words add as 64-bit integers (exact: the frame's term limit covers all of
// the frame's chunks, DESIGN.md "Slices"; written unsigned, two's complement), the flag words OR, and where both frames track noise (pa) the pairs merge at the
// merged words.
KY_HD inline void merge_pixel(long long* wa, const long long* wb, unsigned& fa, unsigned fb, NoisePixel* pa, const NoisePixel* pb, int total_spp, int n_a, int n_b) {
    for (int c = 0; c < 3; ++c) wa[c] = (long long)((unsigned long long)wa[c] + (unsigned long long)wb[c]);
    fa |= fb;
    if (pa) noise_merge(*pa, n_a, *pb, n_b, noise_luminance(wa[0], wa[1], wa[2], total_spp));
}
// The standard error of the pixel's mean luminance in units of the film's white: se / max(1, mean), se = sqrt(m2 / (batches - 1) / N).  +inf before the second
// batch; 0 for a pixel whose flag word has a NaN or +-inf bit (its resolved value is pinned by the flag rules).
KY_NOFMA_FN KY_HD inline float noise_value(const NoisePixel& px, int batches, int n_done, unsigned flags) {
    KY_NOFMA_BODY
    if (flags & 0x1ffu) return 0.f;
    if (batches < 2 || n_done < 1) return INFINITY;
    const double se = sqrt(px.m2 / (double)(batches - 1) / (double)n_done);
    const double mean = px.y_prev / (double)n_done;
    return (float)(se / (mean > 1.0 ? mean : 1.0));
}
// Pixel i of a shard's compact tile buffer -> its place in the film: film_add_kernel's de-interleave (ky_launch.hip).  A ragged edge tile's padding has
// x >= width or y >= height.
KY_HD inline void noise_pixel_xy(const ShardConst& sh, int i, int& x, int& y) {
    const int per_tile = sh.tile_w * sh.tile_h;
    const int k = i / per_tile, r = i % per_tile;
    const int tile = sh.tile_first + k * sh.tile_step;
    const int trow = tile / sh.tiles_x, tcol = (tile % sh.tiles_x + trow) % sh.tiles_x;
    x = tcol * sh.tile_w + r % sh.tile_w;
    y = trow * sh.tile_h + r / sh.tile_w;
}
// the order in which two partial results meet, everywhere: a + b with a the lower indices
KY_NOFMA_FN KY_HD inline NoiseSums noise_sums_add(const NoiseSums& a, const NoiseSums& b) {
    KY_NOFMA_BODY
    NoiseSums s;
    s.pixels = a.pixels + b.pixels; s.flagged = a.flagged + b.flagged; s.above = a.above + b.above;
    s.sum = a.sum + b.sum;
    s.max = a.max > b.max ? a.max : b.max;
    s.pad_ = 0;
    return s;
}
// one pixel's contribution (flagged pixels read 0 and count in `flagged`; padding counts nowhere)
KY_HD inline NoiseSums noise_sums_of(float v, int cls, float threshold) {
    NoiseSums s;
    s.pixels = cls != KY_NOISE_PADDING; s.flagged = cls == KY_NOISE_FLAGGED; s.above = cls == KY_NOISE_INSIDE && v > threshold;
    s.sum = cls == KY_NOISE_INSIDE ? (double)v : 0.0;
    s.max = cls == KY_NOISE_INSIDE ? v : 0.f;
    s.pad_ = 0;
    return s;
}

// ---- the trailer of a tracking frame's checkpoint (ky_frame_book.cpp, next to frame_state_check) ----
inline size_t noise_trailer_bytes(int n_pix) { return sizeof(NoiseTrailer) + (size_t)n_pix * sizeof(NoisePixel); }
// KY_OK and the trailer, or KY_ERR_INVALID_VALUE with the message: `bytes` after `state_bytes` hold no whole trailer, another magic, a batch count below 0,
// an n_prev that is not the header's samples done
int noise_trailer_check(const void* buf, size_t bytes, size_t state_bytes, int n_pix, int samples_done, NoiseTrailer* out);

// ---- the kernels (ky_noise.hip); every pointer is device memory, `stream` a hipStream_t ----
// (blocks: NULL, or the kyb::BlockState of every block of a frame that retires blocks, ky_blocks.hpp: a retired block's pairs are frozen, and its pixels' map values
// are taken at the block's own batch and sample counts)
int noise_update_device(const void* ws, void* state, const ShardConst& sh, int total_spp, int n_prev, int n_now, const void* blocks, void* stream);
int noise_map_device(const void* ws, const void* state, float* map, unsigned char* cls, const ShardConst& sh, int width, int height, int batches, int n_done,
                     const void* blocks, void* stream);
constexpr int KY_NOISE_BLOCK = 256;
inline int noise_blocks(int n_pix) { return (n_pix + KY_NOISE_BLOCK - 1) / KY_NOISE_BLOCK; }
// partials: noise_blocks(n_pix) + 1 NoiseSums; the result is the last one
int noise_stats_device(const float* map, const unsigned char* cls, int n_pix, float threshold, void* partials, void* stream);
// ky_merge.hip: merge_pixel over the n_pix pixels of two accumulator blocks of one shard (3 n_pix words, then n_pix flag words; src_ws is read only) and, where
// dst_state is given, over their n_pix NoisePixel (src_state then too); dst stands at n_dst samples held, src at n_src
int merge_device(void* dst_ws, const void* src_ws, void* dst_state, const void* src_state, int n_pix, int total_spp, int n_dst, int n_src, void* stream);
}  // namespace kyn
