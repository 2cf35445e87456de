#!/usr/bin/env python3
"""The device cost of textures (profiles/texture_rates.txt is this tool's output, appended per run), table kernels, one GPU.
  tools/texture_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5; 64 spp): the floor's and the back wall's materials
  tools/texture_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720): the floor's (and wall's) material and the planks'
Frames: a 4 x 4 checker on the floor, a 256 x 256 bilinear image on a wall, and both.  Per sampler (random, stratified), alternating, REPEATS times after WARMUP
untimed rounds, medians of kyhip_kernel_ms of
  specialised     the frame with constant colours as kyhip_render runs it: both_mis on the row of scene facts a textured frame gives up
  lens row        the frame with constant colours on a lens row, under a lens of radius 1e-6 of the scene's diagonal: the pinhole's picture on the row a textured
                  row is shaped like (run-time dispatch, no scene facts, the lens's two draws, no screen cull)
  checker+lens, image+lens, both+lens    the textured frames under the same lens: over `lens row`, the texture's own cost
  checker, image, both                   the textured frames through the pinhole (the camera form's skips taken): over `specialised`, what the user gives up"""
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
    floor_surface, wall_surface = 0, 2
else:
    w, h = 1024, 768
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA, w, h)
    floor_surface, wall_surface = 3, 4
floor_m, wall_m = scene.c.surfaces[floor_surface].material, scene.c.surfaces[wall_surface].material
c0 = lambda m: np.array([scene.c.materials[m].color0[j] for j in range(3)], np.float32)
checker = api.texture_checker(floor_m, c0(floor_m), 0.25 * c0(floor_m), scale=(4, 4))
t = (np.arange(256) + 0.5) / 256
img = (0.5 + 0.5 * np.outer(np.sin(2 * np.pi * 3 * t), np.sin(2 * np.pi * 2 * t)))[:, :, None] * c0(wall_m)[None, None, :]
image = api.texture_image(wall_m, img.astype(np.float32), bilinear=True)
lens = api.lens(1e-6 * 2 * float(O.world_bounding_sphere(scene)[3]), api.focus_distance(scene, w // 2, h // 2))


def timed(params, lens=None, textures=None):
    api.render(scene, params, lens=lens, textures=textures)
    return api.kernel_ms(0), lib.kyhip_last_kernel(0).decode().split(" [")[0]


lines = ["%s %d x %d, %d spp, %d repeats, checker on material %d, 256 x 256 bilinear image on material %d, lens radius %.3g" % (what, w, h, spp, REPEATS, floor_m, wall_m, lens.radius)]
for sampler, kind in (("random", A.SAMPLER_RANDOM), ("stratified", A.SAMPLER_STRATIFIED)):
    both = api.make_params(w, h, spp, sampler=kind)
    runs = (("specialised", None, None), ("lens row", lens, None), ("checker+lens", lens, [checker]), ("image+lens", lens, [image]), ("both+lens", lens, [checker, image]),
            ("checker", None, [checker]), ("image", None, [image]), ("both", None, [checker, image]))
    ms, names = {}, {}
    for r in range(WARMUP + REPEATS):
        for name, ln, tx in runs:
            v, names[name] = timed(both, ln, tx)
            if r >= WARMUP:
                ms.setdefault(name, []).append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines.append("  %s sampler (both_mis on every line)" % sampler)
    for name, _, _ in runs:
        lines.append("    %-13s kernel %.3f ms (min %.3f, max %.3f)  %s" % (name, med[name], min(ms[name]), max(ms[name]), names[name]))
    lines.append("    over the lens row: checker %.3f  image %.3f  both %.3f    over the specialised row: checker %.3f  image %.3f  both %.3f"
                 % (med["checker+lens"] / med["lens row"], med["image+lens"] / med["lens row"], med["both+lens"] / med["lens row"],
                    med["checker"] / med["specialised"], med["image"] / med["specialised"], med["both"] / med["specialised"]))
print("\n".join(lines))
with open(os.path.join(ROOT, "profiles", "texture_rates.txt"), "a") as f:
    f.write("\n".join(lines) + "\n")
