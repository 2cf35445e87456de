#!/usr/bin/env python3
"""Prints the statistics battery of tests/test_sampler.py in full: every statistic on the project's keying next to its derived threshold, the period proof,
every mutant's verdict (the named defects a statistic must reject, and the blind spots no statistic rejects at this size), and the foreign-generator
check oracle against oracle.  Needs no GPU (the oracle is used for the last part only).  Its output is profiles/sampler_battery.txt:

    python tools/sampler_battery.py > profiles/sampler_battery.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import sampler_expectation as E  # noqa: E402
import sampler_restatement as R  # noqa: E402

WHAT = {"a": "per-dimension chi-square, 256 bins (255 df)", "b": "chi-square of consecutive dimension pairs, 16 x 16 bins (255 df)",
        "c": "r sqrt(n), one dimension between samples s and s + 1 of a pixel", "d": "r sqrt(n), one dimension between pixels p and p + 1, then rows y and y + 1",
        "e": "r sqrt(n) between dimensions j != k of one stream, first 8 dimensions",
        "f": "per-pixel chi-square, 16 bins over a pixel's samples, summed over pixels, in deviations of its null"}


def line(letter, label, stat):
    inside, worst, (lo, hi) = R.verdict(stat)
    vals = stat["values"]
    print("  (%s) %-22s %4d statistics  min %9.2f  max %9.2f  worst %9.2f  allowed %8.2f .. %8.2f  %s" %
          (letter, label, len(vals), min(vals), max(vals), worst, lo, hi, "inside" if inside else "REJECTED"))
    return inside


def main():
    print("sampler battery: tests/sampler_restatement.py's numbers; thresholds are the two-sided 1 - 1e-6 / T quantile of each family's null distribution")
    for letter in sorted(WHAT):
        print("  (%s) %s" % (letter, WHAT[letter]))
    print()
    print("period of the xoroshiro64 step over GF(2) (order of its 64 x 64 matrix = 2^64 - 1):")
    for abc in (R.ABC, (26, 9, 12), (25, 9, 13), (26, 8, 13), (26, 13, 9)):
        print("  (a, b, c) = %-12s %s" % (abc, "full period" if R.has_full_period(abc) else "NOT full period"))
    print()
    for name, (w, h, spp, k) in R.BATTERY_SETS.items():
        print("key set '%s': seed %d, %d x %d pixels, %d samples per pixel, %d numbers per stream (%d streams)" % (name, R.BATTERY_SEED, w, h, spp, k, w * h * spp))
        keys = R.frame_keys(w, h, spp)
        u = R.stream_floats(R.BATTERY_SEED, keys, k)
        for letter, stat in sorted(R.battery(u, w, h, spp).items()):
            line(letter, "project keying", stat)
        print("  (g) streams that share an initial state: %d" % R.shared_states(R.BATTERY_SEED, keys))
        print()
    w, h, spp, _ = R.BATTERY_SETS["first"]
    keys = R.frame_keys(w, h, spp)
    print("mutants on key set 'first', 16 numbers per stream (every statistic; the tests assert the rejections marked in tests/test_sampler.py's POWER):")
    for mutant, text in R.MUTANTS.items():
        print(" %s -- %s" % (mutant, text))
        u = R.stream_floats(R.BATTERY_SEED, keys, 16, mutant)
        rejected = [letter for letter, stat in sorted(R.battery(u, w, h, spp).items()) if not line(letter, mutant, stat)]
        shared = R.shared_states(R.BATTERY_SEED, keys, mutant)
        print("  (g) streams that share an initial state: %d" % shared)
        print("  => rejected by: %s" % (", ".join(rejected + (["g"] if shared else [])) or "NOTHING (a blind spot of the battery at this size)"))
    print()
    sp_keys = R.frame_keys(64, 16, 64)
    print("fp64 path (splitmix64), 16 x 16 pixels x 4 subpixels x 64 samples, 16 numbers per stream:")
    u = R.sp_words_to_double(R.sp_stream_words(R.BATTERY_SEED, sp_keys, 16))
    for letter, stat in sorted(R.battery(u, 64, 16, 64, only="abce").items()):
        line(letter, "project keying", stat)
    print("  (g) closest two stream starts on the cycle: %d steps (must exceed 256)" % R.sp_closest_starts(R.BATTERY_SEED, sp_keys))
    for mutant, text in R.SP_MUTANTS.items():
        print("  (g) %s -- %s: closest starts %d steps" % (mutant, text, R.sp_closest_starts(R.BATTERY_SEED, sp_keys, mutant)))
    print()
    print("expectation under a foreign generator, oracle on its own streams against the oracle on NumPy's MT19937(2024) tape (%d pixels x %d samples):" %
          (E.N_PIXELS, E.N_SAMPLES))
    from ky_amd import _abi as A, api
    from oracle import kyoracle as O
    for name in E.SCENES:
        own = E.own_samples(O.li, A, api, name)
        tape, most = E.tape_samples(O, A, api, name)
        ok, lines = E.check(own, tape, "  " + name)
        print("\n".join(lines))
        print("  %s: most numbers one sample drew: %d of %d; %s" % (name, most, E.SCENES[name][2], "holds" if ok else "FAILS"))
        for m, (dev, ratio, mean, sd) in E.batch_means_deviations(E.luminance(own, 32.0)).items():
            print("  %s batch means m = %2d: ratio %.4f, permutation null %.4f +- %.4f: %+.2f deviations (bound 4.5)" % (name, m, ratio, mean, sd, dev))
        if name == "cornell":
            bad, _ = E.tape_samples(O, A, api, name, repeat_draws=True)
            ok, lines = E.check(own, bad, "  cornell, tape whose every second draw repeats the one before")
            print("\n".join(lines))
            print("  => %s" % ("NOT rejected" if ok else "rejected"))
            # correlation BETWEEN samples does not move an expectation: the 'hash_before_sample' mutant leaves sum z^2 where independent samples put it
            scene, params = E.scene_and_params(A, api, name)
            ww, _, stride = E.SCENES[name]
            mut = []
            for x, y in E.pixels(name):
                k2 = np.stack([np.full(E.N_SAMPLES, y * ww + x, np.uint32), np.arange(E.N_SAMPLES, dtype=np.uint32)], axis=1)
                mut.append(O.li_tape(scene, params, x, y, R.stream_floats(params.seed, k2, stride, "hash_before_sample"))[0])
            ok, lines = E.check(np.stack(mut), tape, "  cornell, streams of the mutant 'hash_before_sample'")
            print("\n".join(lines))
            print("  => %s; sum z^2 stays where independent samples put it: this check does not see correlation between samples (its standard errors come "
                  "out too small, which can lift max |z| a little); the battery's (c) and (f) reject this mutant at 344 and 35 deviations" %
                  ("every condition holds" if ok else "a condition fails"))


if __name__ == "__main__":
    main()
