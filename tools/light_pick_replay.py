#!/usr/bin/env python3
"""tools/light_pick_replay.py [spp]  (no GPU): sample_single_light's pick replayed on the CPU oracle's own vertices -- tests/light_pick_replay.py says how a sample
is put together from kyo_trace_li, kyo_li under KY_DIRECT_IDLE and kyo_kat_nee(48, light).  On the pixels of the statistical tests (the Veach frame and the
Cornell box with lamp and point light of single_light_scenes.stat_case, the sixteen pixels of the sixteen-lights room), spp samples each (1024), it prints
  - the per-vertex variance that the pick adds, mean over the vertices of  sum_l nee_l^2 / p_l - (sum_l nee_l)^2,  under the uniform, the power and the spatial
    pick with the uniform share a in {1/8, 1/4, 1/2};
  - per pixel set the summed per-pixel variance of a sample -- what every rule has, var_s(E), plus what the pick adds -- and its ratio to the uniform pick's;
  - "RATIO <case> <rule> <a> <value>" lines for the whole pixel set, which tests/test_light_pick_gpu.py reads from the committed output
    (profiles/light_pick_replay.txt) as what to expect of the GPU's samples.
Veach is split by the first surface a pixel's samples hit: floor and wall (matte), planks (plastic), and of the planks' pixels the highlights: those whose
mean is more than twice the planks' median."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from ky_amd import _abi as A, api
from oracle import kyoracle as O
import light_pick_restatement as R
from light_pick_replay import RULES, SHARES, Replay
from test_light_pick_gpu import _stat_pixels

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
for case in ("veach", "cornell_lamp_point", "sixteen_lights"):
    scene, W, H, pixels = _stat_pixels(case, A, api, O)
    rp = Replay(A, api, O, scene, W, H, pixels, spp)
    s = R.scene_view(api, scene)
    base = rp.base()
    ref = np.stack([np.asarray(O.li(scene, api.make_params(W, H, spp, seed=4321), x, y, 0, spp), np.float64) @ [0.212671, 0.715160, 0.072169] for (x, y) in pixels])
    fin = np.isfinite(ref).all(axis=1)
    print("%s: %d pixels x %d samples, %d lit vertices (%.2f per sample; %d dropped as not finite); mean luminance of the replay's both_mis %.5f, of the oracle's under another seed %.5f"
          % (case, len(pixels), spp, len(rp.nee), len(rp.nee) / (len(pixels) * spp), rp.dropped, base[fin].mean(), ref[fin].mean()))
    sets = {"all": np.ones(len(pixels), bool)}
    if case == "veach":
        plastic = np.array([s.materials[s.surfaces[int(k)].material].kind == A.MATERIAL_PLASTIC for k in rp.first_surface])
        mean = base.mean(axis=1)
        sets["floor and wall"] = ~plastic
        sets["planks"] = plastic
        sets["highlights"] = plastic & (mean > 2 * np.median(mean[plastic]))
    every = base.var(axis=1, ddof=1)
    uni_v, uni_px = rp.pick_variance("uniform")
    print("  %-16s %6s  %-8s %6s  %14s  %14s  %14s  %8s" % ("pixels", "count", "rule", "a", "per vertex", "pick, summed", "sample, summed", "ratio"))
    for name, m in sets.items():
        in_set = m[rp.pix]
        print("  %-16s %6d  %-8s %6s  %14.6e  %14.6e  %14.6e  %8.3f   (every rule's part of the sample's variance: %.6e)"
              % (name, int(m.sum()), "uniform", "-", uni_v[in_set].mean(), uni_px[m].sum(), (every + uni_px)[m].sum(), 1.0, every[m].sum()))
        for rule in RULES[1:]:
            for a in SHARES:
                pv, px = rp.pick_variance(rule, a)
                print("  %-16s %6d  %-8s %6.3f  %14.6e  %14.6e  %14.6e  %8.3f" % (name, int(m.sum()), rule, a, pv[in_set].mean(), px[m].sum(), (every + px)[m].sum(),
                                                                             (every + px)[m].sum() / (every + uni_px)[m].sum()))
    for rule in RULES[1:]:
        for a in SHARES:
            print("RATIO %s %s %.3f %.4f" % (case, rule, a, rp.ratio(rule, a)))
    sys.stdout.flush()
