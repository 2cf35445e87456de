#!/usr/bin/env python3
"""The figures of DESIGN.md "Noise" on how heavy-tailed the tests' frame is (profiles/noise_replay.txt).  No GPU: the samples of the Cornell 32 x 32, 500 spp
frame of tests/test_noise_gpu.py (seed 1234) are replayed on the CPU oracle (kyo li: the same streams, per-sample radiance), cut into the frame's chunks, and
fed to the NumPy restatement of the estimator (tests/noise_restatement.py), one chunk per pass.  Prints, per pass boundary, quantiles of the map next to the
plain per-sample standard error std / sqrt(N), and the share of pixels above test_render_until's threshold, 0.9 of the map's lower quartile at 112 samples."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from ky_amd import _abi as A, api
from oracle import kyoracle as O
import noise_restatement as R

W = H = 32
SPP = 500
scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
p = api.make_params(W, H, SPP)
lum = np.array([0.212671, 0.715160, 0.072169])
Y = np.stack([O.li(scene, p, i % W, i // W, 0, SPP).astype(np.float64) @ lum for i in range(W * H)])   # [pixel, sample]
cum = np.cumsum(Y, axis=1)
bounds = api.pass_boundaries(SPP)
y_prev, m2, n_prev, maps = np.zeros(W * H), np.zeros(W * H), 0, {}
for k, d in enumerate(bounds):
    y_prev, m2 = R.update(y_prev, m2, cum[:, d - 1], n_prev, d)
    n_prev = d
    maps[d] = R.value(y_prev, m2, k + 1, d)
threshold = 0.9 * float(np.quantile(maps[112], 0.25))
print("Cornell %d x %d, %d spp, seed %d, one chunk per pass; threshold %.6f = 0.9 x the map's lower quartile at 112 samples" % (W, H, SPP, p.seed, threshold))
print("samples batches   map: quartile   median  90th pct   std/sqrt(N): quartile   median  90th pct   share above the threshold")
for k, d in enumerate(bounds):
    if d < 48 or (d > 128 and d % 16 and d != SPP):
        continue
    se = Y[:, :d].std(axis=1, ddof=1) / np.sqrt(d) / np.maximum(1.0, Y[:, :d].mean(axis=1))
    q, s = np.quantile(maps[d], [0.25, 0.5, 0.9]), np.quantile(se, [0.25, 0.5, 0.9])
    print("%7d %7d        %.5f  %.5f   %.5f                 %.5f  %.5f   %.5f   %.3f" % (d, k + 1, q[0], q[1], q[2], s[0], s[1], s[2], (maps[d] > threshold).mean()))
