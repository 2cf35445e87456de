#!/usr/bin/env python3
"""tools/stratified_battery.py -> profiles/stratified_battery.txt: every figure of tests/test_stratified.py's battery on the stratified sampler's integer strata
(tests/stratified_restatement.py, no GPU): the shipped keys and perm, then each named defect under each statistic."""
import os
import sys
import warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sampler_restatement as R
import stratified_restatement as S

w, h, n = S.BATTERY_SET
lines = ["%d x %d pixels x %d samples, seed %d; (a) uniform over pixels per (sample, position); (b) positions d < e of one sample independent; (c) neighbouring pixels independent" %
         (w, h, n, S.BATTERY_SEED)]
cases = [("shipped", None, None)] + [(m, m, None) for m in S.MUTANTS] + [("drop_pixel_bit_0", None, "drop_pixel_bit_0")]
for label, mutant, pixel_mutant in cases:
    f = S.fine_strata(S.BATTERY_SEED, w, h, n, mutant, pixel_mutant)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for letter, stat in sorted(S.battery(f, n).items()):
            inside, worst, (lo, hi) = R.verdict(stat)
            lines.append("%-18s (%s) %4d statistics  min %10.2f  max %10.2f  worst %10.2f  allowed %.2f .. %.2f  %s" %
                         (label, letter, len(stat["values"]), min(stat["values"]), max(stat["values"]), worst, lo, hi, "inside" if inside else "REJECTED"))
print("\n".join(lines))
with open(os.path.join(ROOT, "profiles", "stratified_battery.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
