#!/usr/bin/env python3
"""The device cost of a pixel filter (profiles/filter_rates.txt is this tool's output, appended per run), table kernels, one GPU.
  tools/filter_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5; 64 spp)
  tools/filter_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720)
Per sampler (random, stratified), alternating, REPEATS times after WARMUP untimed rounds, medians of kyhip_kernel_ms of
  specialised   the frame as kyhip_render runs it: both_mis on the row of scene facts a filtered frame gives up
  plain         the same frame on the plain run-time-dispatched row (kyhip_set_specialisation(0)).  Under the random sampler both_mis keeps a fact-free row of its
                own with the switch off, so there this line and the filtered ones it is compared with render light_mis, whose frame does land on strategy -1
  tent          the frame under the tent of radius 2 (the closed-form warp)
  gaussian      ... under the default Gaussian (the table warp)
and the ratios filtered / plain (what the warp itself costs) and filtered / specialised (what a filtered frame costs its user), with the kernels' names."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ky_amd import api, _abi as A

WARMUP, REPEATS = 2, 9
args = [a for a in sys.argv[1:] if not a.startswith("--")]
what = args[0] if args else "cornell"
spp = int(args[1]) if len(args) > 1 else 64
lib = A.load_kyhip()
lib.kyhip_set_jit(0)
if what == "veach":
    w, h = 1280, 720
    scene = api.mis_scene(w, h)
else:
    w, h = 1024, 768
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA, w, h)
tent, gauss = api.pixel_filter(A.FILTER_TENT, 2.0), api.pixel_filter(A.FILTER_GAUSSIAN)


def timed(params, filter=None, specialise=True):
    prev = lib.kyhip_set_specialisation(1 if specialise else 0)
    try:
        api.render(scene, params, filter=filter)
    finally:
        lib.kyhip_set_specialisation(prev)
    return api.kernel_ms(0), lib.kyhip_last_kernel(0).decode().split(" [")[0]


lines = ["%s %d x %d, %d spp, %d repeats" % (what, w, h, spp, REPEATS)]
for sampler, kind in (("random", A.SAMPLER_RANDOM), ("stratified", A.SAMPLER_STRATIFIED)):
    both = api.make_params(w, h, spp, sampler=kind)
    like = both if kind == A.SAMPLER_STRATIFIED else api.make_params(w, h, spp, sampler=kind, direct_sample=A.DIRECT_LIGHT_MIS)   # what the plain row renders
    runs = (("specialised", both, None, True), ("plain", like, None, False), ("tent", like, tent, True), ("gaussian", like, gauss, True))
    if like is not both:
        runs += (("tent, both_mis", both, tent, True), ("gaussian, both_mis", both, gauss, True))
    ms, names = {}, {}
    for r in range(WARMUP + REPEATS):
        for name, params, flt, spec in runs:
            t, names[name] = timed(params, flt, spec)
            if r >= WARMUP:
                ms.setdefault(name, []).append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines.append("  %s sampler%s" % (sampler, "" if like is both else " (plain, tent and gaussian render light_mis: see the tool's text)"))
    for name, _, _, _ in runs:
        lines.append("    %-19s kernel %.3f ms (min %.3f, max %.3f)  %s" % (name, med[name], min(ms[name]), max(ms[name]), names[name]))
    lines.append("    tent / plain %.3f   gaussian / plain %.3f" % (med["tent"] / med["plain"], med["gaussian"] / med["plain"]))
    a, b = ("tent", "gaussian") if like is both else ("tent, both_mis", "gaussian, both_mis")
    lines.append("    tent / specialised %.3f   gaussian / specialised %.3f   (both_mis on both sides)" % (med[a] / med["specialised"], med[b] / med["specialised"]))
print("\n".join(lines))
with open(os.path.join(ROOT, "profiles", "filter_rates.txt"), "a") as f:
    f.write("\n".join(lines) + "\n")
