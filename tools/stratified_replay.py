#!/usr/bin/env python3
"""tools/stratified_replay.py [reps] [seeds] -> profiles/stratified_replay.txt: what the stratified sampler buys per sample.  No GPU: the
CPU oracle runs on the numbers of both samplers (tests/stratified_mse.py).  Per scene -- the 48 x 27 Veach and 32 x 32 Cornell frames and 64 pixels of
tests/sampler_expectation.py, and a camera-only integrand, KY_INTEGRATOR_BASECOLOR on the Cornell frame's pixels that straddle an edge -- and per sample count
(16, 64): the per-pixel mean squared error of the N-sample estimate (luminance clamped at 32) against an 8192-sample reference, stratified over random, as the
ratio of the sums, the median pixel's ratio and the share of pixels below 1; per seed, then over all seeds.  And the frame's noise estimate over the true
standard error of the estimate under both samplers (1 for independent samples; the passes are the frame's chunks)."""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from ky_amd import _abi as A, api
from oracle import kyoracle as O
import sampler_expectation as E
import stratified_mse as P

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
SEEDS = [1234, 99, 20260102, 7][:int(sys.argv[2]) if len(sys.argv) > 2 else 4]
O.load()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def case(name):
    if name == "basecolor":
        w, h, stride = 32, 32, 4
        scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
        params = lambda n: api.make_params(w, h, n, integrator=A.INTEGRATOR_BASECOLOR, max_path_depth=5)
        pixels = P.edge_pixels(O, scene, params(64), w, h)
    else:
        w, h, stride = E.SCENES[name]
        scene = E.scene_and_params(A, api, name, 64)[0]
        params = lambda n: E.scene_and_params(A, api, name, n)[1]
        pixels = E.pixels(name)
    return scene, params, pixels, w, h, stride


t0 = time.time()
say("stratified over random, per-pixel MSE of the N-sample estimate; %d replications per seed, seeds %s; reference %d samples, luminance clamped at %g" %
    (REPS, SEEDS, P.REFERENCE_SAMPLES, P.CLAMP))
for name in ("veach", "cornell", "basecolor"):
    scene, params, pixels, w, h, stride = case(name)
    gen = np.random.Generator(np.random.MT19937(2024))
    refs = [P.reference(O, scene, params(P.REFERENCE_SAMPLES), x, y, stride, gen) for x, y in pixels]
    for n_spp in (16, 64):
        bounds = api.pass_boundaries(n_spp)
        total, noise = np.zeros((2, len(pixels))), []
        for seed in SEEDS:
            out = P.replay(O, scene, params(n_spp), pixels, w, h, stride, seed, n_spp, REPS, refs, bounds)
            total += out["mse"]
            noise.append(out["noise"])
            s, m, b, k = P.ratios(out["mse"])
            say("%-9s N = %2d seed %-9d: sum %.3f  median %.3f  below 1: %.2f  (%d pixels)" % (name, n_spp, seed, s, m, b, k))
        s, m, b, k = P.ratios(total)
        nz = np.nanmedian(np.stack(noise), axis=(0, 2))
        say("%-9s N = %2d all seeds     : sum %.3f  median %.3f  below 1: %.2f  (%d pixels); noise estimate / true standard error, median pixel: random %.2f, stratified %.2f (%d passes)" %
            (name, n_spp, s, m, b, k, nz[0], nz[1], len(bounds)))
say("%.0f seconds" % (time.time() - t0))
with open(os.path.join(ROOT, "profiles", "stratified_replay.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
