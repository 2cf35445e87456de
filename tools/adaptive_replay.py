#!/usr/bin/env python3
"""The block retire rule of DESIGN.md "Adaptive" replayed without a GPU (profiles/adaptive_replay.txt): the samples of the tests' Cornell 40 x 24, 500 spp frame
(tests/test_blocks_gpu.py, seed 1234) come from the CPU oracle (kyo li: the same streams, per-sample radiance), are cut into passes of at least L samples that
end on the frame's chunk boundaries, and feed the NumPy restatement of the estimator (tests/noise_restatement.py) and the rule, restated here in film order
(tests/blocks_restatement.py has it in compact tile order: a block retires when batches >= min_batches and above <= max_fraction_above * its pixels).  Prints per (threshold, fraction, pass
length): the samples each 8 x 8 block receives, how many blocks retire early, and the smallest relative distance from the threshold of a pixel that decides a
verdict -- the (allowed + 1)-th largest map value of a block when the rule is applied to it: the verdict flips when that value crosses the threshold."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from ky_amd import _abi as A, api
from oracle import kyoracle as O
import noise_restatement as R

W, H, SPP, MIN_BATCHES = 40, 24, 500, 3
scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
p = api.make_params(W, H, SPP)
lum = np.array([0.212671, 0.715160, 0.072169])
Y = np.stack([O.li(scene, p, i % W, i // W, 0, SPP).astype(np.float64) @ lum for i in range(W * H)])   # [pixel, sample], film order
cum = np.cumsum(Y, axis=1)
bounds = api.pass_boundaries(SPP)
block = (np.arange(W * H) // W // 8) * (W // 8) + (np.arange(W * H) % W) // 8                           # film order -> film block
n_blocks = (W // 8) * (H // 8)


def replay(threshold, fraction, length):
    y_prev, m2 = np.zeros(W * H), np.zeros(W * H)
    retired = np.full(n_blocks, -1)
    front, batches, margin = 0, 0, np.inf
    while front < SPP and (retired < 0).any():
        now = next(b for b in bounds if b >= min(front + length, SPP))
        live_px = retired[block] < 0
        y_new, m2_new = R.update(y_prev, m2, cum[:, now - 1], front, now)
        y_prev, m2 = np.where(live_px, y_new, y_prev), np.where(live_px, m2_new, m2)
        front, batches = now, batches + 1
        values = R.value(y_prev, m2, batches, front)
        if batches < MIN_BATCHES:
            continue
        for b in np.flatnonzero(retired < 0):
            v = np.sort(values[block == b])[::-1]
            allowed = int(np.floor(np.float64(np.float32(fraction)) * len(v)))
            if allowed >= len(v):
                retired[b] = front
                continue
            decider = float(v[allowed])
            margin = min(margin, abs(decider - threshold) / threshold)
            if int((v > np.float32(threshold)).sum()) <= np.float64(np.float32(fraction)) * len(v):
                retired[b] = front
    samples = np.where(retired < 0, SPP, retired)
    return samples, margin


print("Cornell %d x %d, %d spp, seed %d, %d blocks of 8 x 8; min_batches %d; passes end at the first chunk boundary at least L samples on" % (W, H, SPP, p.seed, n_blocks, MIN_BATCHES))
for threshold, fraction, length in ((0.008, 0.10, 100), (0.008, 0.10, 48), (0.004, 0.10, 100), (0.008, 0.0, 100), (0.016, 0.10, 100)):
    samples, margin = replay(threshold, fraction, length)
    early = samples[samples < SPP]
    print("threshold %.3f, fraction %.2f, passes of %d: %d of %d blocks retire early (the first at %s samples), %d run to %d; mean %.1f samples per pixel; "
          "closest deciding pixel %.0f %% from the threshold" % (threshold, fraction, length, len(early), n_blocks, early.min() if len(early) else "-",
                                                                  n_blocks - len(early), SPP, samples.mean(), 100 * margin))
    for row in samples.reshape(H // 8, W // 8):
        print("    " + " ".join("%4d" % s for s in row))
