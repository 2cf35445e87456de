"""Does the stratified sampler pay?  A replay on the CPU oracle, no GPU: a pixel's estimate from N samples is computed many times under the random sampler's
numbers (sampler_restatement) and under the stratified sampler's (stratified_restatement, the shipped perm), each time through kyo_li_tape, and the two mean
squared errors against a many-sample reference are compared per pixel.  The reference quantity is the random sampler on the same oracle.

A replication is a pixel KEY of its own: the numbers of a sample are a function of (seed, pixel index, sample, N) alone, so replication r of pixel (x, y) reads the
tape of pixel index y w + x + r w h -- another pixel's numbers, an independent draw -- while the oracle traces pixel (x, y).  Seeds give the spread.

A helper module: tools/stratified_replay.py writes profiles/stratified_replay.txt with it, tests/test_stratified.py asserts on a smaller run of it."""
import numpy as np

import noise_restatement as NR
import sampler_expectation as E
import sampler_restatement as R
import stratified_restatement as S

CLAMP = 32.0
REFERENCE_SAMPLES = 8192


def keys_for(pixel_index, frame_pixels, reps, n_spp):
    """[reps * N, 2]: replication-major, the samples of one replication together."""
    pix = np.repeat(pixel_index + frame_pixels * np.arange(reps, dtype=np.uint64), n_spp)
    return np.stack([pix, np.tile(np.arange(n_spp, dtype=np.uint64), reps)], axis=1)


def luminances(O, scene, params, x, y, tape, clamp=CLAMP):
    li, _ = O.li_tape(scene, params, x, y, tape)
    return E.luminance(li, clamp)


def reference(O, scene, params, x, y, stride, gen):
    """The pixel's clamped mean luminance from REFERENCE_SAMPLES samples on a Mersenne Twister's numbers."""
    return float(luminances(O, scene, params, x, y, E.mt_tape_rows(gen, REFERENCE_SAMPLES, stride)).mean())


def estimates(O, scene, params, x, y, width, height, stride, seed, n_spp, reps, stratified):
    """[reps, N]: the clamped luminance of every sample of every replication."""
    keys = keys_for(np.uint64(y * width + x), np.uint64(width * height), reps, n_spp)
    tape = S.floats(seed, keys, n_spp, stride) if stratified else R.stream_floats(seed, keys, stride)
    return luminances(O, scene, params, x, y, tape).reshape(reps, n_spp)


def noise_estimate(samples, bounds):
    """samples [reps, N] -> [reps]: the frame's noise estimate before its normalisation, the standard error from the batch means of the passes that end at
    `bounds` (noise_restatement.update, one pass per boundary)."""
    cum = np.cumsum(samples, axis=1)
    y_prev, m2, n_prev = np.zeros(samples.shape[0]), np.zeros(samples.shape[0]), 0
    for d in bounds:
        y_prev, m2 = NR.update(y_prev, m2, cum[:, d - 1], n_prev, d)
        n_prev = d
    return np.sqrt(m2 / float(len(bounds) - 1) / float(n_prev))   # noise_value's `se`: the standard error of the mean if the batches were independent


def replay(O, scene, params, pixels, width, height, stride, seed, n_spp, reps, refs, bounds=None):
    """-> {"mse": [2, pixels] (random, stratified), "noise": [2, pixels] or None}: per pixel the mean squared error of the N-sample estimate against refs, and
    the mean noise estimate over the true standard error of the estimate."""
    mse = np.zeros((2, len(pixels)))
    noise = np.zeros((2, len(pixels))) if bounds else None
    for i, (x, y) in enumerate(pixels):
        for k, stratified in enumerate((False, True)):
            v = estimates(O, scene, params, x, y, width, height, stride, seed, n_spp, reps, stratified)
            est = v.mean(axis=1)
            mse[k, i] = float(((est - refs[i]) ** 2).mean())
            if bounds:
                true_se = float(est.std(ddof=1))
                noise[k, i] = float(noise_estimate(v, bounds).mean()) / true_se if true_se > 0 else np.nan
    return {"mse": mse, "noise": noise}


def ratios(mse):
    """-> (sum ratio, median per-pixel ratio, share of pixels below 1, pixels counted): stratified over random, over the pixels whose random MSE is not zero."""
    keep = mse[0] > 0
    r = mse[1, keep] / mse[0, keep]
    return float(mse[1, keep].sum() / mse[0, keep].sum()), float(np.median(r)), float((r < 1).mean()), int(keep.sum())


def edge_pixels(O, scene, params, width, height, want=64):
    """Pixels of a first-hit integrand that straddle an edge: those whose value varies most inside the pixel (64 probes on a Mersenne Twister's numbers)."""
    gen = np.random.Generator(np.random.MT19937(7))
    var = np.zeros(width * height)
    for i in range(width * height):
        var[i] = luminances(O, scene, params, i % width, i // width, E.mt_tape_rows(gen, 64, 4)).var()
    order = np.argsort(-var)[:want]
    return [(int(i % width), int(i // width)) for i in order if var[i] > 0]
