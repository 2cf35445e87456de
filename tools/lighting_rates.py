#!/usr/bin/env python3
"""The numbers of DESIGN.md section 3 "Light classes" (profiles/lighting_rates.txt), table kernels, one GPU: kernel time of three renders after a warm-up.
  tools/lighting_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5, both_mis): the unmasked render at depth 5, 0 and 1,
                                          then lighting 1 .. 7
  tools/lighting_rates.py veach [spp]     the same for bench.py --workload veach's geometry (1280 x 720)
  tools/lighting_rates.py cells [spp]     the four cells of `ky_drivers lighting_cells` (256 x 256, path_tracing_recursion_defered_t depth 10): emit, direct,
                                          indirect, all, and their sum
KYHIP_LIB selects another build of the library.  On a library without kyhip_render_lighting (a checkout of an earlier commit with a copy of this file) only the
unmasked lines are printed: they are that commit's side of the comparison."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ky_amd import api, _abi as A

what = sys.argv[1]
spp = int(sys.argv[2]) if len(sys.argv) > 2 else (1024 if what != "cells" else 64)
build = os.path.basename(os.environ.get("KYHIP_LIB", "libkyhip.so"))
masked = "kyhip_render_lighting" in A.KYHIP_SYMBOLS   # (an earlier commit's package: its unmasked lines only)
lib = A.load_kyhip()
lib.kyhip_set_jit(0)


def timed(scene, p, lighting=None, runs=3):
    kw = {} if lighting is None else {"lighting": lighting}
    api.render(scene, p, **kw)
    ms = []
    for _ in range(runs):
        film = api.render(scene, p, **kw)
        ms.append(api.kernel_ms())
    return ms, film


def line(tag, ms, film):
    print("%s %s %s spp %d: kernel ms %s  spread %.1f %%  film mean %.6f  [%s]" % (
        what, build, tag, spp, " ".join("%.2f" % m for m in ms), 100.0 * (max(ms) - min(ms)) / min(ms), film.mean(), lib.kyhip_last_kernel(0).decode()), flush=True)
    return min(ms)


if what in ("cornell", "veach"):
    W, H = (1024, 768) if what == "cornell" else (1280, 720)
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H) if what == "cornell" else api.mis_scene(W, H)
    for depth in (5, 0, 1):
        line("unmasked depth %d" % depth, *timed(scene, api.make_params(W, H, spp, max_path_depth=depth)))
    if masked:
        for m in range(1, 8):
            line("lighting %d" % m, *timed(scene, api.make_params(W, H, spp), lighting=m))
else:
    assert what == "cells"
    W = H = 256
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
    p = api.make_params(W, H, spp, integrator=A.INTEGRATOR_PATH_TRACING_RECURSION_DEFERED, max_path_depth=10)
    plain = line("unmasked (one of four renders)", *timed(scene, p))
    print("%s %s four unmasked renders: %.2f ms" % (what, build, 4 * plain))
    if masked:
        total = sum(line("lighting %d" % m, *timed(scene, p, lighting=m)) for m in (1, 2, 4, 31))
        print("%s %s the driver's four cells: %.2f ms" % (what, build, total))
