#!/usr/bin/env python3
"""The numbers of DESIGN.md "Passes" (profiles/pass_rates.txt), table kernels, one GPU: what rendering a frame in passes costs in kernel time.
  tools/pass_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5, both_mis; 1024 spp)
  tools/pass_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720)
One line for the one-shot frame (kyhip_render: the render kernel of kyhip_render_tiles_device), then the frame as a kyhip_frame in 1, 2, 4, 8 and 16 passes of
about equal sample counts and with one chunk per pass: the sum of the passes' kernel times, best of three frames after a warm-up.  Every pass but the last ends
on full-size chunks without the taper, so it pays a drain of up to one bulk item besides the launch's fixed cost; each frame is also checked against the
one-shot film, bit for bit."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ky_amd import api, _abi as A

what = sys.argv[1] if len(sys.argv) > 1 else "cornell"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
lib = A.load_kyhip()
lib.kyhip_set_jit(0)
W, H = (1024, 768) if what == "cornell" else (1280, 720)
scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H) if what == "cornell" else api.mis_scene(W, H)
p = api.make_params(W, H, spp)

api.render(scene, p)
one = []
for _ in range(3):
    want = api.render(scene, p)
    one.append(api.kernel_ms())
print("%s %d x %d, %d spp, %d chunks  [%s]" % (what, W, H, spp, len(api.pass_boundaries(spp)), lib.kyhip_last_kernel(0).decode()))
print("one shot                 kernel ms %s" % " ".join("%.2f" % m for m in one), flush=True)


def frame(min_samples):
    with api.Frame(scene, p) as f:
        ms = []
        while f.done < f.total:
            f.render(min_samples)
            ms.append(api.kernel_ms())
        return ms, np.array_equal(f.resolve(), want)


for n in (1, 2, 4, 8, 16, 0):
    min_samples = 1 if n == 0 else -(-spp // n)
    frame(min_samples)
    runs = [frame(min_samples) for _ in range(3)]
    best = min(runs, key=lambda r: sum(r[0]))[0]
    print("%-24s kernel ms %s  +%.2f ms, +%.1f %% on one shot, %.3f ms per extra pass; longest pass %.2f, shortest %.3f; film == one shot: %s" % (
        ("one chunk per pass: %d" % len(best)) if n == 0 else "%d passes (>= %d spp)" % (len(best), min_samples), " ".join("%.2f" % sum(r[0]) for r in runs),
        sum(best) - min(one), 100.0 * (sum(best) - min(one)) / min(one), (sum(best) - min(one)) / max(1, len(best) - 1), max(best), min(best),
        all(r[1] for r in runs)), flush=True)
