#!/usr/bin/env python3
"""Where the denoise filter's default sigmas come from, and whether it denoises (profiles/denoise_replay.txt; DESIGN.md "Denoise").  No GPU: the samples of the
tests' Cornell 40 x 24, 500 spp frame (tests/test_denoise_gpu.py; three seeds) are replayed on the CPU oracle (kyo li: the same streams, per-sample radiance), cut
into the frame's chunks, one chunk per pass, and fed to the NumPy restatements of the noise estimate (tests/noise_restatement.py) and of the filter
(tests/denoise_restatement.py) at several (sigma_luminance, sigma_plane) pairs.  The guides are the oracle's camera and scene-intersect KATs on the pixel centres.
Prints the RMSE against a high-sample oracle frame, raw and denoised, at 112, 224 and 500 samples.

`chains` (profiles/denoise_chains_replay.txt; DESIGN.md "Denoise", "Guides beyond the first hit"): the same replay at the default sigmas with first-hit guides and
with specular-chain guides (four guide bounces: the oracle's trace_li under the debug sampler fed to tests/denoise_chains_restatement.py, taps of the same key
only), for the default scene and for the large mirror ball, at 48, 112, 224 and 500 samples: RMSE over the whole film and over the pixels whose key is not 0.

`albedo` (profiles/denoise_albedo_replay.txt; DESIGN.md "Denoise", "Albedo"): tests/texture_restatement.py's cornell_case -- a checker on the plastic floor, a
4 x 4 nearest image on the back wall, a checker on a mirror wall -- cut into constant-colour tiles (tiled()), which the unchanged oracle can trace; the same replay
at the default sigmas with today's filter and with albedo demodulation (tests/denoise_albedo_restatement.py) at albedo grids 1, 2, 4 and 8 and under both variance
rules (v / Y(a')^2, the one the library uses, and v Y(1 / a')^2).  The albedo is the oracle's camera and scene-intersect KATs at the sub-sample positions with the
tiled material's colour.  RMSE over the whole film and over the pixels whose centre first hits a textured surface, at 48, 112, 224 and 500 samples.

`temporal` (profiles/denoise_temporal_replay.txt; DESIGN.md "Denoise", "Temporal"): the Cornell box with both balls along a camera path
(tests/denoise_temporal_restatement.py: PATH_FRAMES frames of PATH_SPP samples, one chunk per pass, frame k with seed + k, dolly, sideways move and pan), every
frame's samples replayed on the oracle and fed through the NumPy restatements with specular-chain guides of one guide bounce: temporal + spatial against spatial
alone against raw on the LAST frame, over a scan of the temporal parameters.  RMSE against the oracle at truth_spp samples of the last frame, over the whole film
and over the non-floor pixels (the floor is Phong with exponent 90: its highlight is view-dependent, and history holds it where the earlier cameras saw it).

usage: tools/denoise_replay.py [truth_spp]
       tools/denoise_replay.py chains [truth_spp]
       tools/denoise_replay.py albedo [truth_spp]
       tools/denoise_replay.py temporal [truth_spp]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from ky_amd import _abi as A, api
from oracle import kyoracle as O
import noise_restatement as R
import denoise_restatement as D

W, H, SPP = 40, 24, 500
SEEDS = (1234, 101, 202, 303, 404)   # the first three are the GPU test's
AT = (112, 224, 500)
PAIRS = [(4.0, 1.0), (1.0, 1.0), (1.5, 1.0), (2.0, 1.0), (1.5, 0.25), (1.5, 0.1), (2.0, 0.25), (3.0, 0.25), (8.0, 1.0)]   # (4, 1): where the scan started; (1.5, 0.25): the defaults
CHAINS = sys.argv[1:2] == ["chains"]
ALBEDO = sys.argv[1:2] == ["albedo"]
TEMPORAL = sys.argv[1:2] == ["temporal"]
if CHAINS or ALBEDO or TEMPORAL:
    del sys.argv[1]
TRUTH_SPP = int(sys.argv[1]) if len(sys.argv) > 1 else 16384


def replay_chains():
    import denoise_chains_restatement as DC
    at = (48, 112, 224, 500)
    bounds = api.pass_boundaries(SPP)
    debug = api.make_params(W, H, 1, max_path_depth=8, sampler=A.SAMPLER_DEBUG)
    print("Cornell %d x %d, %d spp, one chunk per pass; truth: the oracle at %d spp; D.DEFAULTS; chain guides: %d guide bounces, taps of the same key only" % (
        W, H, SPP, TRUTH_SPP, DC.MAX_BOUNCES))
    print("RMSE of clamp01(picture) against the truth, over the whole film and over the pixels whose key is not 0 (\"chain\"); ratio = chain guides / first-hit guides")
    for name, flags in (("CB_DEFAULT_SCENE", A.CB_DEFAULT_SCENE), ("CB_LARGE_MIRROR | CB_LIGHT_AREA", A.CB_LARGE_MIRROR | A.CB_LIGHT_AREA)):
        scene = api.cornell_box_scene(flags, W, H)
        truth = O.render(scene, api.make_params(W, H, TRUTH_SPP, seed=987654)).astype(np.float64)
        ga0, gb0 = D.guides_from_hits(scene.c, O.kat_scene_intersect(scene, D.centre_rays(O.kat_camera, scene.c.camera, W, H)), W, H)
        cls, key, ga1, gb1 = DC.chains(lambda x, y: O.trace_li(scene, debug, x, y, 0), scene.c, W, H, DC.MAX_BOUNCES)
        on = key != 0
        pix = D.pixel_width(scene.c.camera, W)
        rmse = lambda film, sel: float(np.sqrt((((np.clip(film.astype(np.float64), 0, 1) - truth) ** 2)[sel]).mean()))
        print("\n== %s: %d of %d pixels first hit a mirror or glass: %d chains end on a surface, %d leave the box, %d distinct keys on the film" % (
            (name, int(on.sum()), W * H) + DC.counts(cls, key)[1:3] + (len(np.unique(key)),)))
        print(" seed samples batches | whole film: raw  first-hit     chains  ratio | chain pixels: raw  first-hit     chains  ratio | other pixels: first-hit     chains")
        ratios = {d: [] for d in at}
        for seed in SEEDS:
            p = api.make_params(W, H, SPP, seed=seed)
            rad = np.stack([O.li(scene, p, i % W, i // W, 0, SPP).astype(np.float64) for i in range(W * H)])
            cum = np.cumsum(rad, axis=1)
            y_prev, m2, n_prev = np.zeros(W * H), np.zeros(W * H), 0
            for k, d in enumerate(bounds):
                accum = np.rint(cum[:, d - 1] / SPP * 4294967296.0).astype(np.int64)
                y_prev, m2 = R.update(y_prev, m2, R.luminance(accum, SPP), n_prev, d)
                n_prev = d
                if d not in at:
                    continue
                cv = D.gather(accum, np.zeros(W * H, np.uint32), m2, SPP, d, k + 1).reshape(H, W, 4)
                first = D.denoise(cv, ga0, gb0, pix, **D.DEFAULTS)[..., :3]
                chain = DC.denoise(cv, ga1, gb1, key, pix, **D.DEFAULTS)[..., :3]
                everywhere = np.ones((H, W), bool)
                w3, c3 = [rmse(f, everywhere) for f in (cv[..., :3], first, chain)], [rmse(f, on) for f in (cv[..., :3], first, chain)]
                ratios[d].append((w3[2] / w3[1], c3[2] / c3[1]))
                print("%5d %7d %7d |          %.5f    %.5f    %.5f  %.3f |            %.5f    %.5f    %.5f  %.3f |                 %.5f    %.5f" % (
                    seed, d, k + 1, w3[0], w3[1], w3[2], w3[2] / w3[1], c3[0], c3[1], c3[2], c3[2] / c3[1], rmse(first, ~on), rmse(chain, ~on)))
        for d in at:
            r = np.array(ratios[d])
            print("at %3d samples: whole-film ratio %.3f .. %.3f, %d of %d seeds below 1; chain-pixel ratio %.3f .. %.3f, %d of %d below 1" % (
                d, r[:, 0].min(), r[:, 0].max(), int((r[:, 0] < 1).sum()), len(r), r[:, 1].min(), r[:, 1].max(), int((r[:, 1] < 1).sum()), len(r)))


def replay_albedo():
    import denoise_albedo_restatement as DA
    import texture_restatement as X
    at, grids, rules, seeds = (48, 112, 224, 500), (1, 2, 4, 8), ("y2", "inv"), SEEDS[:3]
    scene, textures = X.cornell_case(A, api, W, H)
    tiled = X.tiled(A, scene.scene, textures)
    truth = O.render(tiled, api.make_params(W, H, TRUTH_SPP, seed=987654)).astype(np.float64)
    ga, gb = D.guides_from_hits(tiled.scene, O.kat_scene_intersect(tiled, D.centre_rays(O.kat_camera, tiled.scene.camera, W, H)), W, H)
    pix = D.pixel_width(tiled.scene.camera, W)
    albedo = {g: DA.albedo(O, A, tiled, [], W, H, g, check_clean=False)[0] for g in grids}
    first = DA.albedo(O, A, scene, textures, W, H, 1, check_clean=False)[2][..., 0]
    materials = {t.material for t in textures}
    tex = np.isin(first, [s for s in range(scene.scene.surface_count) if scene.scene.surfaces[s].material in materials])
    everywhere = np.ones((H, W), bool)
    print("cornell_case %d x %d tiled (%d surfaces), %d spp, one chunk per pass; truth: the oracle at %d spp; D.DEFAULTS; %d of %d pixels first-hit a textured surface" % (
        W, H, tiled.scene.surface_count, SPP, TRUTH_SPP, int(tex.sum()), W * H))
    print("RMSE of clamp01(picture) against the truth.  today = the filter without an albedo; gG = demodulated by a G x G albedo, rule v / Y(a')^2; gG' = rule v Y(1 / a')^2")
    cols = ["g%d" % g for g in grids] + ["g%d'" % g for g in grids]
    print(" seed samples where    |     raw    today | " + " ".join("%8s" % c for c in cols) + " | g4 / today  g4 / raw  g1 / today  g4' / g4")
    table = {}
    for seed in seeds:
        frames = DA.replay(O, api, R, tiled, W, H, SPP, seed, at)
        for d in at:
            cv = frames[d]
            today = D.denoise(cv, ga, gb, pix, **D.DEFAULTS)
            out = {(g, r): DA.denoise(cv, ga, gb, albedo[g], pix, variance=r, **D.DEFAULTS) for g in grids for r in rules}
            for where, sel in (("film", everywhere), ("textured", tex)):
                e = {k: DA.rmse(v, truth, sel) for k, v in out.items()}
                raw, td = DA.rmse(cv, truth, sel), DA.rmse(today, truth, sel)
                table[(seed, d, where)] = (raw, td, e)
                print("%5d %7d %-8s | %.5f  %.5f | " % (seed, d, where, raw, td) + " ".join("%8.5f" % e[(g, r)] for r in rules for g in grids) +
                      " |      %.3f     %.3f       %.3f      %.3f" % (e[(4, "y2")] / td, e[(4, "y2")] / raw, e[(1, "y2")] / td, e[(4, "inv")] / e[(4, "y2")]))
    for where in ("film", "textured"):
        print("\n%s pixels, ranges over the %d seeds:" % (where, len(seeds)))
        for d in at:
            rows = [table[(s, d, where)] for s in seeds]
            rng = lambda f: "%.2f - %.2f" % (min(f(*r) for r in rows), max(f(*r) for r in rows))
            print("  at %3d samples: today / raw %s;  g4 / raw %s;  g4 / today %s;  g1 / raw %s;  g1 / today %s;  g8 / g4 %s;  g4' / g4 %s" % (
                d, rng(lambda raw, td, e: td / raw), rng(lambda raw, td, e: e[(4, "y2")] / raw), rng(lambda raw, td, e: e[(4, "y2")] / td),
                rng(lambda raw, td, e: e[(1, "y2")] / raw), rng(lambda raw, td, e: e[(1, "y2")] / td), rng(lambda raw, td, e: e[(8, "y2")] / e[(4, "y2")]),
                rng(lambda raw, td, e: e[(4, "inv")] / e[(4, "y2")])))
    n = len(seeds) * len(at)
    print("\ng4 below today in %d of %d cases on the textured pixels and %d of %d over the film; g4 below g1 in %d of %d (textured) and %d of %d (film)" % (
        sum(table[(s, d, "textured")][2][(4, "y2")] < table[(s, d, "textured")][1] for s in seeds for d in at), n,
        sum(table[(s, d, "film")][2][(4, "y2")] < table[(s, d, "film")][1] for s in seeds for d in at), n,
        sum(table[(s, d, "textured")][2][(4, "y2")] < table[(s, d, "textured")][2][(1, "y2")] for s in seeds for d in at), n,
        sum(table[(s, d, "film")][2][(4, "y2")] < table[(s, d, "film")][2][(1, "y2")] for s in seeds for d in at), n))


def replay_temporal():
    import denoise_albedo_restatement as DA
    import denoise_chains_restatement as DC
    import denoise_temporal_restatement as DT
    from screen_cull_scenes import cornell_with_camera
    n, spp, seeds = DT.PATH_FRAMES, DT.PATH_SPP, (DT.PATH_SEED, 101, 202)
    debug = api.make_params(W, H, 1, max_path_depth=8, sampler=A.SAMPLER_DEBUG)
    scan = [dict(DT.DEFAULTS)] + [dict(DT.DEFAULTS, max_history=m) for m in (1.0, 2.0, 4.0, 16.0)] + [dict(DT.DEFAULTS, min_weight=m) for m in (0.0, 0.25, 0.5)] + \
           [dict(DT.DEFAULTS, sigma_plane=sp) for sp in (0.1, 1.0)] + [dict(DT.DEFAULTS, normal_squarings=q) for q in (3, 10)]
    print("Cornell %d x %d with both balls, %d frames of %d spp (one chunk per pass, %d batches), frame k with seed + k, along the path dolly %g, sideways %g, pan %g; "
          "guide bounces 1; truth: the oracle at %d spp of the last frame; D.DEFAULTS for the levels" % (
              W, H, n, spp, len(api.pass_boundaries(spp)), DT.PATH_DOLLY, DT.PATH_SIDE, DT.PATH_PAN, TRUTH_SPP))
    print("RMSE of clamp01(picture) of the LAST frame against the truth; s = spatial alone, t = temporal alone (levels 0), t+s = temporal + spatial.  Over the whole "
          "film, over the pixels that do not first-hit the floor (plastic, Phong exponent 90), and over the pixels further than 2 pixels from a saturated one of the "
          "truth (a channel >= 0.9: the lamp, its edge pixels, its mirror images)")
    for tilt, name in ((0.0, "the lamp in view"), (DT.PATH_TILT, "tilted down by %g, the lamp out of view" % DT.PATH_TILT)):
        scenes = [cornell_with_camera(A, api, W, H, lambda cam, s=k / (n - 1): DT.path_camera(A, cam, s, tilt)) for k in range(n)]
        guides = []
        for scene in scenes:
            cls, key, ga, gb = DC.chains(lambda x, y: O.trace_li(scene, debug, x, y, 0), scene.scene, W, H, 1)
            guides.append((ga, gb, key))
        last = scenes[-1]
        truth = O.render(last, api.make_params(W, H, TRUTH_SPP, seed=987654)).astype(np.float64)
        c = last.scene
        first_hit = np.asarray(O.kat_scene_intersect(last, D.centre_rays(O.kat_camera, c.camera, W, H)), np.float32)
        surf = np.where(first_hit[:, 0] == 1, first_hit[:, 8], -1).astype(int).reshape(H, W)
        floor = np.isin(surf, [s for s in range(c.surface_count) if c.materials[c.surfaces[s].material].kind == A.MATERIAL_PLASTIC])
        bright = truth.max(axis=2) >= 0.9
        near = np.zeros_like(bright)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = np.clip(np.arange(H) + dy, 0, H - 1), np.clip(np.arange(W) + dx, 0, W - 1)
                near |= bright[ys][:, xs]
        where = (("film", np.ones((H, W), bool)), ("rest", ~floor), ("away", ~near))
        print("\n== %s: %d of %d pixels first-hit the floor, %d carry a chain key, %d of the truth's are saturated and %d lie within 2 pixels of one" % (
            name, int(floor.sum()), W * H, int((guides[-1][2] != 0).sum()), int(bright.sum()), int(near.sum())))
        frames = {seed: [DA.replay(O, api, R, scene, W, H, spp, seed + k, (spp,))[spp] for k, scene in enumerate(scenes)] for seed in seeds}
        print(" seed | max_history sigma_plane min_weight squarings |  film: raw        s        t      t+s  t+s / s | non-floor: s      t+s  t+s / s | away: s      t+s  t+s / s | took history")
        ratios = {}
        for t in scan:
            for seed in seeds:
                hist = DT.History()
                for k, scene in enumerate(scenes):
                    ga, gb, key = guides[k]
                    out = hist.step(frames[seed][k], ga, gb, key, scene.scene.camera, W, spp, D.DEFAULTS, temporal_params=t)
                cv = frames[seed][-1]
                ga, gb, key = guides[-1]
                spatial = DC.denoise(cv, ga, gb, key, D.pixel_width(c.camera, W), **D.DEFAULTS)
                e = {w: [DA.rmse(f, truth, sel) for f in (cv, spatial, hist.read()[0], out)] for w, sel in where}
                ratios.setdefault(tuple(sorted(t.items())), []).append([e[w][3] / e[w][1] for w, _ in where])
                print("%5d | %11g %11g %10g %9d | %.5f  %.5f  %.5f  %.5f    %.3f |    %.5f  %.5f    %.3f | %.5f  %.5f   %.3f | %d of %d" % (
                    seed, t["max_history"], t["sigma_plane"], t["min_weight"], t["normal_squarings"], e["film"][0], e["film"][1], e["film"][2], e["film"][3],
                    e["film"][3] / e["film"][1], e["rest"][1], e["rest"][3], e["rest"][3] / e["rest"][1], e["away"][1], e["away"][3], e["away"][3] / e["away"][1],
                    int(hist.took.sum()), W * H))
        print()
        for t, r in ratios.items():
            r = np.array(r)
            print("%s: t+s / s over the film %.3f .. %.3f (mean %.3f), non-floor %.3f .. %.3f (mean %.3f), away from saturated pixels %.3f .. %.3f (mean %.3f)" % (
                " ".join("%s %g" % kv for kv in t), r[:, 0].min(), r[:, 0].max(), r[:, 0].mean(), r[:, 1].min(), r[:, 1].max(), r[:, 1].mean(),
                r[:, 2].min(), r[:, 2].max(), r[:, 2].mean()))


if TEMPORAL:
    replay_temporal()
    sys.exit(0)
if CHAINS:
    replay_chains()
    sys.exit(0)
if ALBEDO:
    replay_albedo()
    sys.exit(0)

scene =api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
truth = O.render(scene, api.make_params(W, H, TRUTH_SPP, seed=987654)).astype(np.float64)
ga, gb = D.guides_from_hits(scene.c, O.kat_scene_intersect(scene, D.centre_rays(O.kat_camera, scene.c.camera, W, H)), W, H)
pix = D.pixel_width(scene.c.camera, W)
bounds = api.pass_boundaries(SPP)
rmse = lambda film: float(np.sqrt(((np.clip(film.astype(np.float64), 0, 1) - truth) ** 2).mean()))
print("Cornell %d x %d, %d spp, one chunk per pass; truth: the oracle at %d spp; classes: %s" % (
    W, H, SPP, TRUTH_SPP, " ".join("%d x %d" % (int((gb[..., 3] == c).sum()), c) for c in (0, 1, 2))))
print("RMSE of clamp01(picture) against the truth; ratio = denoised / raw.  levels 5, normal_squarings 7")
print(" seed samples batches      raw   " + "  ".join("sl %-4g sp %-4g" % pr for pr in PAIRS))
ratios = {pr: [] for pr in PAIRS}
for seed in SEEDS:
    p = api.make_params(W, H, SPP, seed=seed)
    rad = np.stack([O.li(scene, p, i % W, i // W, 0, SPP).astype(np.float64) for i in range(W * H)])   # [pixel (film order), sample, 3]
    cum = np.cumsum(rad, axis=1)
    y_prev, m2, n_prev = np.zeros(W * H), np.zeros(W * H), 0
    for k, d in enumerate(bounds):
        accum = np.rint(cum[:, d - 1] / SPP * 4294967296.0).astype(np.int64)   # the frame's accumulators: sums scaled by 1 / total, in 2^-32
        y_prev, m2 = R.update(y_prev, m2, R.luminance(accum, SPP), n_prev, d)
        n_prev = d
        if d not in AT:
            continue
        flags = np.zeros(W * H, np.uint32)
        cv = D.gather(accum, flags, m2, SPP, d, k + 1).reshape(H, W, 4)
        raw = rmse(cv[..., :3])
        row = []
        for pr in PAIRS:
            out = D.denoise(cv, ga, gb, pix, levels=5, normal_squarings=7, sigma_luminance=pr[0], sigma_plane=pr[1])
            row.append(rmse(out[..., :3]))
            ratios[pr].append(row[-1] / raw)
        print("%5d %7d %7d  %.5f   " % (seed, d, k + 1, raw) + "  ".join("%.5f (%.3f)" % (r, r / raw) for r in row))
print("largest ratio per pair:     " + "  ".join("sl %g sp %g: %.3f" % (pr + (max(ratios[pr]),)) for pr in PAIRS))
print("mean ratio per pair:        " + "  ".join("sl %g sp %g: %.3f" % (pr + (float(np.mean(ratios[pr])),)) for pr in PAIRS))
