/*
 * ky_noise.hip -- the kernels of a frame's per-pixel noise estimate (ky_noise.hpp; DESIGN.md "Noise"), film-sized and apart from the render kernels:
 * (A frame that also retires pixel blocks, ky_blocks.hpp, hands the first two its per-block state: retired blocks keep the estimate they retired with.)
 *   noise_update_kernel   once per pass that rendered something, behind the pass's render kernel: one thread per pixel reads the three accumulators and
 *                         advances the pixel's {y_prev, m2} by the batch the pass added;
 *   noise_map_kernel      {y_prev, m2} and the flag word -> one float per pixel of the compact tile buffer and the pixel's class (inside the film, flagged,
 *                         padding of a ragged edge tile);
 *   noise_stats_kernel    count, flagged, above a threshold, max and sum over the pixels inside the film: a wave64 reduction by cross-lane shuffles, the four
 *                         waves of a workgroup meet in LDS, one partial per workgroup;
 *   noise_final_kernel    one workgroup reduces the partials, each thread a contiguous run of them in index order, through the same tree.
 * No floating-point atomics and no order that depends on scheduling: two calls return identical bytes.  gfx950 only.
 */
#include <hip/hip_runtime.h>

#include "ky_blocks.hpp"
#include "ky_ctx.hpp"
#include "ky_noise.hpp"

using namespace kyn;
using kyb::BlockState;

static_assert(sizeof(NoisePixel) == 16 && sizeof(NoiseTrailer) == 16 && sizeof(NoiseSums) == 40, "the checkpoint trailer and the partials' layout");

// (blocks: the per-block state of a frame that retires blocks, ky_blocks.hpp, or NULL.  A retired block's pixels are not rendered any more: their pair is frozen.)
__global__ void noise_update_kernel(const unsigned long long* __restrict__ accum, NoisePixel* __restrict__ state, int n_pix, int total_spp, int n_prev, int n_now,
                                    const BlockState* __restrict__ blocks, ShardConst sh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    if (blocks && blocks[kyb::block_of_pixel(sh, i)].retired_at >= 0) return;
    const double y = noise_luminance((long long)accum[3 * (size_t)i], (long long)accum[3 * (size_t)i + 1], (long long)accum[3 * (size_t)i + 2], total_spp);
    NoisePixel px = state[i];
    noise_update(px, y, n_prev, n_now);
    state[i] = px;
}

__global__ void noise_map_kernel(const unsigned* __restrict__ flags, const NoisePixel* __restrict__ state, float* __restrict__ map, unsigned char* __restrict__ cls,
                                 ShardConst sh, int width, int height, int batches, int n_done, const BlockState* __restrict__ blocks) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sh.n_pix) return;
    if (blocks) {   // a retired block's pixels keep the value they had when it retired: its own batch and sample counts
        const BlockState b = blocks[kyb::block_of_pixel(sh, i)];
        if (b.retired_at >= 0) { batches = b.batches; n_done = b.retired_at; }
    }
    int x, y;
    noise_pixel_xy(sh, i, x, y);
    const unsigned fl = flags[i];
    map[i] = noise_value(state[i], batches, n_done, fl);
    cls[i] = x >= width || y >= height ? KY_NOISE_PADDING : (fl & 0x1ffu) ? KY_NOISE_FLAGGED : KY_NOISE_INSIDE;
}

// lane l receives lane l + delta's value (lanes without such a partner keep a copy of their own, which nobody reads)
__device__ inline NoiseSums sums_shfl_down(const NoiseSums& s, int delta) {
    NoiseSums r;
    r.pixels = __shfl_down(s.pixels, delta, 64); r.flagged = __shfl_down(s.flagged, delta, 64); r.above = __shfl_down(s.above, delta, 64);
    r.sum = __shfl_down(s.sum, delta, 64);
    r.max = __shfl_down(s.max, delta, 64);
    r.pad_ = 0;
    return r;
}
// The workgroup's 256 values -> thread 0's return value, by a fixed tree: inside a wavefront lane l takes lane l + 32, + 16, ... + 1 (the lower lanes on the left
// of every sum), then wave 0 adds the four waves' results in wave order.
__device__ inline NoiseSums block_reduce(NoiseSums s) {
    __shared__ NoiseSums wave_sums[KY_NOISE_BLOCK / 64];
#pragma unroll
    for (int delta = 32; delta >= 1; delta >>= 1) s = noise_sums_add(s, sums_shfl_down(s, delta));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_sums[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = wave_sums[0];
#pragma unroll
        for (int w = 1; w < KY_NOISE_BLOCK / 64; ++w) s = noise_sums_add(s, wave_sums[w]);
    }
    return s;
}

__global__ __launch_bounds__(KY_NOISE_BLOCK) void noise_stats_kernel(const float* __restrict__ map, const unsigned char* __restrict__ cls, int n_pix, float threshold,
                                                                      NoiseSums* __restrict__ partials) {
    const int i = blockIdx.x * KY_NOISE_BLOCK + threadIdx.x;
    const NoiseSums mine = i < n_pix ? noise_sums_of(map[i], cls[i], threshold) : noise_sums_of(0.f, KY_NOISE_PADDING, threshold);
    const NoiseSums s = block_reduce(mine);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(KY_NOISE_BLOCK) void noise_final_kernel(NoiseSums* __restrict__ partials, int n_partials) {
    const int per = (n_partials + KY_NOISE_BLOCK - 1) / KY_NOISE_BLOCK;
    const int first = (int)threadIdx.x * per;
    NoiseSums mine = noise_sums_of(0.f, KY_NOISE_PADDING, 0.f);
    for (int j = first; j < first + per && j < n_partials; ++j) mine = noise_sums_add(mine, partials[j]);
    const NoiseSums s = block_reduce(mine);
    if (threadIdx.x == 0) partials[n_partials] = s;
}

namespace kyn {
int noise_update_device(const void* ws, void* state, const ShardConst& sh, int total_spp, int n_prev, int n_now, const void* blocks, void* stream) {
    const int n_pix = sh.n_pix;
    if (n_pix <= 0) return KY_OK;
    hipLaunchKernelGGL(noise_update_kernel, dim3(noise_blocks(n_pix)), dim3(KY_NOISE_BLOCK), 0, (hipStream_t)stream, (const unsigned long long*)ws, (NoisePixel*)state, n_pix,
                       total_spp, n_prev, n_now, (const BlockState*)blocks, sh);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int noise_map_device(const void* ws, const void* state, float* map, unsigned char* cls, const ShardConst& sh, int width, int height, int batches, int n_done,
                     const void* blocks, void* stream) {
    if (sh.n_pix <= 0) return KY_OK;
    const unsigned* flags = (const unsigned*)((const unsigned long long*)ws + (size_t)sh.n_pix * 3);
    hipLaunchKernelGGL(noise_map_kernel, dim3(noise_blocks(sh.n_pix)), dim3(KY_NOISE_BLOCK), 0, (hipStream_t)stream, flags, (const NoisePixel*)state, map, cls, sh, width,
                       height, batches, n_done, (const BlockState*)blocks);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int noise_stats_device(const float* map, const unsigned char* cls, int n_pix, float threshold, void* partials, void* stream) {
    if (n_pix <= 0) return KY_OK;
    const int blocks = noise_blocks(n_pix);
    hipLaunchKernelGGL(noise_stats_kernel, dim3(blocks), dim3(KY_NOISE_BLOCK), 0, (hipStream_t)stream, map, cls, n_pix, threshold, (NoiseSums*)partials);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(noise_final_kernel, dim3(1), dim3(KY_NOISE_BLOCK), 0, (hipStream_t)stream, (NoiseSums*)partials, blocks);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}
}  // namespace kyn
