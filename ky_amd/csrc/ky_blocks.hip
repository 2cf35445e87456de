/*
 * ky_blocks.hip -- the kernels of a frame that retires pixel blocks between its passes (ky_blocks.hpp; DESIGN.md "Adaptive"), film-sized and apart from the
 * render kernels:
 *   blocks_init_kernel     one wavefront per block, its 64 lanes the block's 64 pixels: a block without a pixel inside the film (the padding of a ragged edge
 *                          tile) is retired at 0 samples, every other one is live;
 *   blocks_keep_kernel     retires the live blocks none of whose in-film pixels is set in a film-shaped mask (ballot);
 *   blocks_retire_kernel   the retire rule on the noise map: ballot + popcount of "inside and unflagged" and of "above the threshold", lane 0 decides;
 *   blocks_count / _scan / _scatter_kernel   the ascending list of the live blocks: a count per workgroup of 256 blocks, their exclusive prefix by one thread,
 *                          then every live block's place from its workgroup's prefix, the waves before it and the lanes before it.  No atomics: the list is
 *                          the same from run to run;
 *   blocks_resolve_kernel  resolve_frame_kernel's arithmetic (film_value, ky_film_value.hpp) with the scale total / (the block's samples), in double, before the one rounding.
 * gfx950 only.
 */
#include <hip/hip_runtime.h>

#include "ky_blocks.hpp"
#include "ky_ctx.hpp"
#include "ky_film_value.hpp"

using namespace kyb;

static_assert(sizeof(BlockState) == 8 && sizeof(BlockTrailer) == 16, "the checkpoint trailer's layout");
static_assert(KY_BLOCKS_GROUP == 256, "four wavefronts per compaction workgroup");

// the block this wavefront serves, or -1 (wave-uniform)
__device__ inline int wave_block(int n_blocks) {
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    return b < n_blocks ? b : -1;
}

__global__ __launch_bounds__(256) void blocks_init_kernel(BlockState* __restrict__ state, ShardConst sh, int width, int height) {
    const int b = wave_block(sh.n_blocks);
    if (b < 0) return;
    const int lane = threadIdx.x & 63;
    const bool inside = pixel_inside(sh, pixel_of_block(sh, b, lane), width, height);
    const bool any = __ballot(inside) != 0ull;
    if (lane == 0) state[b] = any ? BlockState{-1, 0} : BlockState{0, 0};
}

__global__ __launch_bounds__(256) void blocks_keep_kernel(BlockState* __restrict__ state, const unsigned char* __restrict__ mask, ShardConst sh, int width, int height,
                                                          int front, int batches) {
    const int b = wave_block(sh.n_blocks);
    if (b < 0) return;
    const int lane = threadIdx.x & 63;
    int x, y;
    const bool inside = pixel_inside(sh, pixel_of_block(sh, b, lane), width, height, &x, &y);
    const bool set = inside && mask[(size_t)y * (size_t)width + (size_t)x] != 0;
    const bool any = __ballot(set) != 0ull;
    if (lane == 0 && state[b].retired_at < 0 && !any) state[b] = BlockState{front, batches};
}

__global__ __launch_bounds__(256) void blocks_retire_kernel(BlockState* __restrict__ state, const float* __restrict__ map, const unsigned char* __restrict__ cls,
                                                            ShardConst sh, float threshold, float max_fraction_above, int min_batches, int front, int batches) {
    const int b = wave_block(sh.n_blocks);
    if (b < 0) return;
    const int lane = threadIdx.x & 63;
    const int i = pixel_of_block(sh, b, lane);
    const bool counted = cls[i] == kyn::KY_NOISE_INSIDE;
    const bool above = counted && map[i] > threshold;
    const int n_counted = __popcll(__ballot(counted)), n_above = __popcll(__ballot(above));
    if (lane == 0 && state[b].retired_at < 0 && block_retires(batches, min_batches, n_above, n_counted, max_fraction_above)) state[b] = BlockState{front, batches};
}

// the live blocks of this workgroup's 256: the lane's own flag, the number of live ones before it in the workgroup, and (thread 0's return of) their count
__device__ inline bool group_live(const BlockState* __restrict__ state, int n_blocks, int& before, int& total) {
    __shared__ int wave_n[KY_BLOCKS_GROUP / 64];
    const int b = (int)blockIdx.x * KY_BLOCKS_GROUP + (int)threadIdx.x;
    const bool live = b < n_blocks && state[b].retired_at < 0;
    const unsigned long long m = __ballot(live);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    total = 0;
#pragma unroll
    for (int w = 0; w < KY_BLOCKS_GROUP / 64; ++w) {
        if (w < wave) before += wave_n[w];
        total += wave_n[w];
    }
    return live;
}

__global__ __launch_bounds__(KY_BLOCKS_GROUP) void blocks_count_kernel(const BlockState* __restrict__ state, int n_blocks, int* __restrict__ counts) {
    int before, total;
    (void)group_live(state, n_blocks, before, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[0 .. n_groups) -> their exclusive prefix in place, the total in counts[n_groups]: one thread, in index order
__global__ void blocks_scan_kernel(int* __restrict__ counts, int n_groups) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int run = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int c = counts[g];
        counts[g] = run;
        run += c;
    }
    counts[n_groups] = run;
}

__global__ __launch_bounds__(KY_BLOCKS_GROUP) void blocks_scatter_kernel(const BlockState* __restrict__ state, int n_blocks, const int* __restrict__ counts, int* __restrict__ list) {
    int before, total;
    const bool live = group_live(state, n_blocks, before, total);
    const int at = counts[blockIdx.x] + before;
    if (live && at < n_blocks) list[at] = (int)blockIdx.x * KY_BLOCKS_GROUP + (int)threadIdx.x;   // (at < n_live <= n_blocks by construction: the list has n_blocks words)
}

__global__ void blocks_resolve_kernel(const unsigned long long* __restrict__ accum, const unsigned* __restrict__ flags, const BlockState* __restrict__ state,
                                      float* __restrict__ tiles, ShardConst sh, int total_spp, int front) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sh.n_pix) return;
    const int n = block_samples(state[block_of_pixel(sh, i)], front);
    const double scale = n > 0 ? (double)total_spp / (double)n : 0.0;
    const unsigned fl = flags[i];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tiles[3 * (size_t)i + ch] = film_value(accum[3 * (size_t)i + ch], fl, ch, scale);
}

namespace kyb {
static dim3 wave_grid(int n_blocks) { return dim3((unsigned)((n_blocks + 3) / 4)); }

int blocks_init_device(void* state, const ShardConst& sh, int width, int height, void* stream) {
    if (sh.n_blocks <= 0) return KY_OK;
    hipLaunchKernelGGL(blocks_init_kernel, wave_grid(sh.n_blocks), dim3(256), 0, (hipStream_t)stream, (BlockState*)state, sh, width, height);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int blocks_keep_device(void* state, const unsigned char* mask, const ShardConst& sh, int width, int height, int front, int batches, void* stream) {
    if (sh.n_blocks <= 0) return KY_OK;
    hipLaunchKernelGGL(blocks_keep_kernel, wave_grid(sh.n_blocks), dim3(256), 0, (hipStream_t)stream, (BlockState*)state, mask, sh, width, height, front, batches);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int blocks_retire_device(void* state, const float* map, const unsigned char* cls, const ShardConst& sh, float threshold, float max_fraction_above, int min_batches,
                         int front, int batches, void* stream) {
    if (sh.n_blocks <= 0) return KY_OK;
    hipLaunchKernelGGL(blocks_retire_kernel, wave_grid(sh.n_blocks), dim3(256), 0, (hipStream_t)stream, (BlockState*)state, map, cls, sh, threshold, max_fraction_above,
                       min_batches, front, batches);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int blocks_compact_device(const void* state, int n_blocks, int* list, void* scratch, void* stream) {
    if (n_blocks <= 0) return KY_OK;
    const int groups = blocks_groups(n_blocks);
    hipLaunchKernelGGL(blocks_count_kernel, dim3(groups), dim3(KY_BLOCKS_GROUP), 0, (hipStream_t)stream, (const BlockState*)state, n_blocks, (int*)scratch);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(blocks_scan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (int*)scratch, groups);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(blocks_scatter_kernel, dim3(groups), dim3(KY_BLOCKS_GROUP), 0, (hipStream_t)stream, (const BlockState*)state, n_blocks, (const int*)scratch, list);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}

int blocks_resolve_device(const void* ws, const void* state, float* d_tiles, const ShardConst& sh, int total_spp, int front, void* stream) {
    if (sh.n_pix <= 0) return KY_OK;
    const unsigned long long* accum = (const unsigned long long*)ws;
    const unsigned* flags = (const unsigned*)(accum + (size_t)sh.n_pix * 3);
    hipLaunchKernelGGL(blocks_resolve_kernel, dim3((sh.n_pix + 255) / 256), dim3(256), 0, (hipStream_t)stream, accum, flags, (const BlockState*)state, d_tiles, sh, total_spp, front);
    HIP_TRY(hipGetLastError());
    return KY_OK;
}
}  // namespace kyb
