#!/usr/bin/env python3
"""The device cost of a thin lens (profiles/lens_rates.txt is this tool's output, appended per run), table kernels, one GPU.
  tools/lens_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5; 64 spp), the lens focused on the front ball
  tools/lens_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720), the lens focused on what the frame's centre shows
Lens radius: 2 % of the scene's diagonal.  Per sampler (random, stratified), alternating, REPEATS times after WARMUP untimed rounds, medians of kyhip_kernel_ms of
  specialised   the frame as kyhip_render runs it: both_mis on the row of scene facts a lens frame gives up
  filtered      the frame under the tent of radius 2 on the filtered run-time-dispatched row: what a lens row is but for the lens
  lens          the frame under the lens alone (the box filter: the lens row skips the warp)
  lens+tent     ... under the lens and the tent of radius 2
and the ratios lens+tent / filtered (the lens's own cost: two draws, the disk map, a varying origin, and no screen cull) and lens / specialised (what a lens
frame costs its user), with the kernels' names.  The lens frames are blurred pictures of the same scene: their paths differ from the sharp frame's, which is part
of what the ratios hold."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ky_amd import api, _abi as A
from oracle import kyoracle as O

WARMUP, REPEATS = 2, 9
args = [a for a in sys.argv[1:] if not a.startswith("--")]
what = args[0] if args else "cornell"
spp = int(args[1]) if len(args) > 1 else 64
lib = A.load_kyhip()
lib.kyhip_set_jit(0)
if what == "veach":
    w, h = 1280, 720
    scene = api.mis_scene(w, h)
    focus_px = (w // 2, h // 2)
else:
    w, h = 1024, 768
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA, w, h)
    focus_px = None
if focus_px is None:   # the front ball: the sphere hit nearest the camera on a coarse grid of pixels
    px = np.stack(np.meshgrid(np.arange(8, w, 16), np.arange(8, h, 16)), axis=-1).reshape(-1, 2)
    rays = api.kat_camera(scene.c.camera, (px + 0.5).astype(np.float32))
    hits = api.kat_scene_intersect(scene, np.concatenate([rays, np.full((len(rays), 1), np.inf, np.float32)], axis=1))
    ball = [i for i in range(len(px)) if hits[i, 0] and scene.c.shapes[scene.c.surfaces[int(hits[i, 8])].shape].kind == A.SHAPE_SPHERE]
    focus_px = tuple(int(v) for v in px[min(ball, key=lambda i: hits[i, 1])])
radius = 0.02 * 2 * float(O.world_bounding_sphere(scene)[3])
lens = api.lens(radius, api.focus_distance(scene, *focus_px))
tent = api.pixel_filter(A.FILTER_TENT, 2.0)


def timed(params, filter=None, lens=None):
    api.render(scene, params, filter=filter, lens=lens)
    return api.kernel_ms(0), lib.kyhip_last_kernel(0).decode().split(" [")[0]


lines = ["%s %d x %d, %d spp, %d repeats, lens radius %.4g focus %.4g (pixel %s)" % (what, w, h, spp, REPEATS, lens.radius, lens.focus_distance, focus_px)]
for sampler, kind in (("random", A.SAMPLER_RANDOM), ("stratified", A.SAMPLER_STRATIFIED)):
    both = api.make_params(w, h, spp, sampler=kind)
    runs = (("specialised", None, None), ("filtered", tent, None), ("lens", None, lens), ("lens+tent", tent, lens))
    ms, names = {}, {}
    for r in range(WARMUP + REPEATS):
        for name, flt, ln in runs:
            t, names[name] = timed(both, flt, ln)
            if r >= WARMUP:
                ms.setdefault(name, []).append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines.append("  %s sampler (both_mis on every line)" % sampler)
    for name, _, _ in runs:
        lines.append("    %-12s kernel %.3f ms (min %.3f, max %.3f)  %s" % (name, med[name], min(ms[name]), max(ms[name]), names[name]))
    lines.append("    lens+tent / filtered %.3f   lens / filtered %.3f   lens / specialised %.3f   lens+tent / specialised %.3f"
                 % (med["lens+tent"] / med["filtered"], med["lens"] / med["filtered"], med["lens"] / med["specialised"], med["lens+tent"] / med["specialised"]))
print("\n".join(lines))
with open(os.path.join(ROOT, "profiles", "lens_rates.txt"), "a") as f:
    f.write("\n".join(lines) + "\n")
