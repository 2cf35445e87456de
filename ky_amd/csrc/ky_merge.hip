/*
 * ky_merge.hip -- the kernel of kyhip_frame_merge / kyhip_frame_merge_from (ky_frame.cpp; DESIGN.md "Slices"): two frames of one (scene, params) that hold
 * disjoint sample ranges become one.  Per pixel the three 64-bit words add, the flag words OR and, where both frames track noise, the {y_prev, m2} pairs merge
 * at the merged words -- merge_pixel, ky_noise.hpp, which kyhostcheck_merge runs as host code.
 *   merge_kernel   one thread per PAIR of pixels: six words are three 16-byte loads of each block (a pair begins 48 bytes into its block: aligned), two flag words
 *                  one 8-byte load, the two pairs two 16-byte loads; the same widths on the way back to dst.  A shard with an odd pixel count ends in a pair of one
 *                  pixel, which goes word by word.  A grid-stride loop over at most 2048 workgroups of 256.  No LDS, no atomics: it reads two blocks and writes one,
 *                  and is bound by memory (40 bytes per pixel and side with noise, 28 without).
 * Film-sized and apart from the render kernels, like ky_noise.hip.  gfx950 only.
 */
#include <hip/hip_runtime.h>

#include "ky_ctx.hpp"
#include "ky_noise.hpp"

using namespace kyn;

static_assert(sizeof(NoisePixel) == 16 && sizeof(ulonglong2) == 16 && sizeof(uint2) == 8 && sizeof(double2) == 16, "the merge kernel's 16- and 8-byte accesses");

constexpr int KY_MERGE_BLOCK = 256, KY_MERGE_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(KY_MERGE_BLOCK) void merge_kernel(unsigned long long* __restrict__ dst_words, const unsigned long long* __restrict__ src_words,
                                                                unsigned* __restrict__ dst_flags, const unsigned* __restrict__ src_flags, NoisePixel* __restrict__ dst_state,
                                                                const NoisePixel* __restrict__ src_state, int n_pix, int total_spp, int n_dst, int n_src) {
    const int n_pairs = (n_pix + 1) / 2;
    for (int k = blockIdx.x * KY_MERGE_BLOCK + threadIdx.x; k < n_pairs; k += gridDim.x * KY_MERGE_BLOCK) {
        const size_t i = 2 * (size_t)k;   // the pair's first pixel
        if (i + 1 < (size_t)n_pix) {
            const ulonglong2* a2 = (const ulonglong2*)(dst_words + 3 * i);
            const ulonglong2* b2 = (const ulonglong2*)(src_words + 3 * i);
            const ulonglong2 a[3] = {a2[0], a2[1], a2[2]}, b[3] = {b2[0], b2[1], b2[2]};
            uint2 fa = *(const uint2*)(dst_flags + i);
            const uint2 fb = *(const uint2*)(src_flags + i);
            long long w0[3] = {(long long)a[0].x, (long long)a[0].y, (long long)a[1].x}, w1[3] = {(long long)a[1].y, (long long)a[2].x, (long long)a[2].y};
            const long long v0[3] = {(long long)b[0].x, (long long)b[0].y, (long long)b[1].x}, v1[3] = {(long long)b[1].y, (long long)b[2].x, (long long)b[2].y};
            if (dst_state) {
                const double2 pa0 = *(const double2*)(dst_state + i), pa1 = *(const double2*)(dst_state + i + 1);
                const double2 pb0 = *(const double2*)(src_state + i), pb1 = *(const double2*)(src_state + i + 1);
                NoisePixel p0 = {pa0.x, pa0.y}, p1 = {pa1.x, pa1.y};
                const NoisePixel q0 = {pb0.x, pb0.y}, q1 = {pb1.x, pb1.y};
                merge_pixel(w0, v0, fa.x, fb.x, &p0, &q0, total_spp, n_dst, n_src);
                merge_pixel(w1, v1, fa.y, fb.y, &p1, &q1, total_spp, n_dst, n_src);
                *(double2*)(dst_state + i) = make_double2(p0.y_prev, p0.m2);
                *(double2*)(dst_state + i + 1) = make_double2(p1.y_prev, p1.m2);
            } else {
                merge_pixel(w0, v0, fa.x, fb.x, nullptr, nullptr, total_spp, n_dst, n_src);
                merge_pixel(w1, v1, fa.y, fb.y, nullptr, nullptr, total_spp, n_dst, n_src);
            }
            ulonglong2* o2 = (ulonglong2*)(dst_words + 3 * i);
            o2[0] = make_ulonglong2((unsigned long long)w0[0], (unsigned long long)w0[1]);
            o2[1] = make_ulonglong2((unsigned long long)w0[2], (unsigned long long)w1[0]);
            o2[2] = make_ulonglong2((unsigned long long)w1[1], (unsigned long long)w1[2]);
            *(uint2*)(dst_flags + i) = fa;
        } else {   // the last pixel of an odd count
            long long w[3] = {(long long)dst_words[3 * i], (long long)dst_words[3 * i + 1], (long long)dst_words[3 * i + 2]};
            const long long v[3] = {(long long)src_words[3 * i], (long long)src_words[3 * i + 1], (long long)src_words[3 * i + 2]};
            unsigned fa = dst_flags[i];
            if (dst_state) {
                NoisePixel p = dst_state[i];
                const NoisePixel q = src_state[i];
                merge_pixel(w, v, fa, src_flags[i], &p, &q, total_spp, n_dst, n_src);
                dst_state[i] = p;
            } else {
                merge_pixel(w, v, fa, src_flags[i], nullptr, nullptr, total_spp, n_dst, n_src);
            }
            for (int c = 0; c < 3; ++c) dst_words[3 * i + c] = (unsigned long long)w[c];
            dst_flags[i] = fa;
        }
    }
}

namespace kyn {
int merge_device(void* dst_ws, const void* src_ws, void* dst_state, const void* src_state, int n_pix, int total_spp, int n_dst, int n_src, void* stream) {
    if (n_pix <= 0) return KY_OK;
    if (!dst_ws || !src_ws || (dst_state && !src_state)) return kyh::fail(KY_ERR_INVALID_VALUE, "internal: merge without its buffers");
    // the 16-byte accesses: the blocks begin on 16 bytes (hipMalloc), a pair 48 bytes apart; the flag words begin 24 n_pix bytes in, a pair's 8 bytes apart
    if (((uintptr_t)dst_ws | (uintptr_t)src_ws | (uintptr_t)dst_state | (uintptr_t)src_state) & 15) return kyh::fail(KY_ERR_INVALID_VALUE, "internal: merge buffers off their 16-byte alignment");
    unsigned long long* dw = (unsigned long long*)dst_ws;
    const unsigned long long* sw = (const unsigned long long*)src_ws;
    const int n_pairs = (n_pix + 1) / 2;
    int blocks = (n_pairs + KY_MERGE_BLOCK - 1) / KY_MERGE_BLOCK;
    if (blocks > KY_MERGE_MAX_BLOCKS) blocks = KY_MERGE_MAX_BLOCKS;
    hipLaunchKernelGGL(merge_kernel, dim3(blocks), dim3(KY_MERGE_BLOCK), 0, (hipStream_t)stream, dw, sw, (unsigned*)(dw + (size_t)n_pix * 3), (const unsigned*)(sw + (size_t)n_pix * 3),
                       (NoisePixel*)dst_state, (const NoisePixel*)src_state, n_pix, total_spp, n_dst, n_src);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}
}  // namespace kyn
