#!/usr/bin/env python3
"""The device cost of a stratified number (profiles/stratified_rates.txt is this tool's output, appended per run), table kernels, one GPU.
  tools/stratified_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5, both_mis; 64 spp)
  tools/stratified_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720)
The frame under the random and under the stratified sampler, alternating, REPEATS times after WARMUP untimed rounds: medians of kyhip_kernel_ms, their ratio, and
the kernels' names.  With a device listing built by tools/asm.sh (--listing FILE) and a resource log (--resources FILE: hipcc -Rpass-analysis=kernel-resource-usage),
the static instructions tools/asm_by_func.py attributes to the stratified draw and tools/resources.py's line for each stratified kernel are appended."""
import os
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ky_amd import api, _abi as A

WARMUP, REPEATS = 3, 15
args = [a for a in sys.argv[1:] if not a.startswith("--")]
what = args[0] if args else "cornell"
spp = int(args[1]) if len(args) > 1 else 64
opt = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i].startswith("--")}
lib = A.load_kyhip()
lib.kyhip_set_jit(0)
if what == "veach":
    w, h = 1280, 720
    scene = api.mis_scene(w, h)
else:
    w, h = 1024, 768
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA, w, h)
lines = []
ms, names = {}, {}
kinds = (("random", A.SAMPLER_RANDOM), ("stratified", A.SAMPLER_STRATIFIED))
for r in range(WARMUP + REPEATS):
    for name, kind in kinds:
        api.render(scene, api.make_params(w, h, spp, sampler=kind))
        if r >= WARMUP:
            ms.setdefault(name, []).append(api.kernel_ms(0))
        names[name] = lib.kyhip_last_kernel(0).decode()
med = {k: float(np.median(v)) for k, v in ms.items()}
lines.append("%s %d x %d, %d spp, %d repeats" % (what, w, h, spp, REPEATS))
for name, _ in kinds:
    lines.append("  %-10s kernel %.3f ms (min %.3f, max %.3f)  %s" % (name, med[name], min(ms[name]), max(ms[name]), names[name]))
lines.append("  stratified / random: %.3f" % (med["stratified"] / med["random"]))
if "--listing" in opt:
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asm_by_func.py"), opt["--listing"], "render_kernel_stratified"], capture_output=True, text=True).stdout
    lines += ["  " + l for l in out.splitlines() if any(fn in l for fn in ("strat_", "sampler_", "mix32"))]
if "--resources" in opt:
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resources.py"), opt["--resources"]], capture_output=True, text=True).stdout
    lines += ["  " + l for l in out.splitlines() if "render_kernel_stratified" in l]
print("\n".join(lines))
with open(os.path.join(ROOT, "profiles", "stratified_rates.txt"), "a") as f:
    f.write("\n".join(lines) + "\n")
