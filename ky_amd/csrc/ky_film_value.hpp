/*
 * ky_film_value.hpp -- a fixed-point accumulator word -> the film value of its channel, written ONCE for the three resolve kernels (resolve_kernel and
 * resolve_frame_kernel, ky_launch.hip; blocks_resolve_kernel, ky_blocks.hip): their outputs are held bit-identical by the frame tests.  Not one of the device
 * headers the library embeds for its run-time instantiations: kyhip_kernel_source_hash does not move with it.
 */
#pragma once
#include "ky_shard.hpp"   // KY_FIX_SCALE

// Channel ch of a pixel whose accumulator word is `fixed` and whose flag word is fl: clamp01 (3726) of value x scale, the product in double before the one
// rounding to float (scale 1.0 is exact and folds away: resolve_kernel).  The flag word's nine bits pin what the word cannot hold: +inf -> 1, -inf -> 0, a NaN or
// both infinities -> 0 (clamp01 keeps NaN in the reference and its 8-bit image shows 0).
__device__ inline float film_value(unsigned long long fixed, unsigned fl, int ch, double scale) {
    float v = (float)((double)(long long)fixed * (1.0 / KY_FIX_SCALE) * scale);
    const bool nan = (fl >> ch) & 1u, pinf = (fl >> (3 + ch)) & 1u, ninf = (fl >> (6 + ch)) & 1u;
    if (pinf) v = 1.f;
    if (ninf) v = 0.f;
    if (nan || (pinf && ninf)) v = 0.f;
    return fminf(fmaxf(v, 0.f), 1.f);
}
