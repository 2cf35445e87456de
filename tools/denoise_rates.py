#!/usr/bin/env python3
"""The numbers of DESIGN.md "Denoise" (profiles/denoise_rates.txt), table kernels, one GPU.
  tools/denoise_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5, both_mis; 512 spp)
  tools/denoise_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720)
hipEvent time (kyhip_frame_denoise_ms) of the guide trace and of the filter -- gather, levels and add in one span -- for 1 .. 6 levels into a pinned film, so
that the span holds kernels only: the increment from L - 1 to L levels is the level with step 2^(L - 1), and what one level's span holds beyond an increment is
the gather and the add.  Next to a 64-sample pass's render kernel (kyhip_kernel_ms) and the noise kernels (kyhip_frame_noise_ms).  Medians of five calls after
a warm-up.  Then, per guide bounce count 1 .. 4 (kyhip_frame_set_guide_bounces), a frame of its own: the chain trace and the keyed filter the same way.
  tools/denoise_rates.py albedo cornell|veach [spp]   (profiles/denoise_albedo_rates.txt; DESIGN.md "Denoise", "Albedo") the same two geometries under
tests/texture_restatement.py's texture sets: the albedo trace (kyhip_frame_albedo_ms) at grids 1, 2, 4 and 8 -- once per frame, so the median over five frames
each -- next to the guide trace and a 64-sample pass, and the default five-level filter's span with and without demodulation, medians of five calls.
  tools/denoise_rates.py temporal cornell|veach [spp]   (profiles/denoise_temporal_rates.txt; DESIGN.md "Denoise", "Temporal") two frames of the geometry at guide
bounces 0 and 1 that hand one history to each other: the temporal kernel's hipEvent span (kyhip_history_ms) next to one level's, measured in the same loop -- the
level as the increment of the filter's span from 1 to 6 levels over five -- medians of five calls."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ky_amd import api, _abi as A

ALBEDO = sys.argv[1:2] == ["albedo"]
TEMPORAL = sys.argv[1:2] == ["temporal"]
if ALBEDO or TEMPORAL:
    del sys.argv[1]
what = sys.argv[1] if len(sys.argv) > 1 else "cornell"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 512
lib = A.load_kyhip()
lib.kyhip_set_jit(0)
W, H = (1024, 768) if what == "cornell" else (1280, 720)
scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H) if what == "cornell" else api.mis_scene(W, H)
p = api.make_params(W, H, spp)
film = api.PinnedFilm(H, W)


def albedo_rates():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import texture_restatement as X
    tscene, textures = (X.cornell_case if what == "cornell" else X.veach_case)(A, api, W, H)
    tx = [t.to_api(api) for t in textures]

    def filter_span(f):
        f.denoise(film=film.array)   # warm-up; traces the guides and the albedo
        runs = []
        for _ in range(5):
            f.denoise(film=film.array)
            runs.append(f.denoise_ms()[1])
        return float(np.median(runs)), runs

    with api.Frame(tscene, p, noise=True, textures=tx) as f:
        f.render(64)
        first = api.kernel_ms()
        f.render(64)
        print("%s %d x %d under %d textures, %d spp; passes of 64: render kernel %.3f and %.3f ms  [%s]" % (
            what, W, H, len(tx), spp, first, api.kernel_ms(), lib.kyhip_last_kernel(0).decode()), flush=True)
        plain, runs = filter_span(f)
        print("no albedo: guide trace %.4f ms; filter, 5 levels: %.4f ms (five calls: %s)" % (f.denoise_ms()[0], plain, " ".join("%.4f" % r for r in runs)), flush=True)
    for bounces in (0, 2):
        for grid in (1, 2, 4, 8):
            traces, guides, spans = [], [], []
            for _ in range(5):
                with api.Frame(tscene, p, noise=True, textures=tx, guide_bounces=bounces, albedo=grid) as f:
                    f.render(64)
                    f.render(64)
                    span, runs = filter_span(f)
                    traces.append(f.albedo_ms())
                    guides.append(f.denoise_ms()[0])
                    spans.append(span)
            t = float(np.median(traces))
            print("%d guide bounces, albedo grid %d: albedo trace, once per frame: %.4f ms = %.3f ns per sub-sample = %.3f of a 64-sample pass (five frames: %s); guide "
                  "trace %.4f ms; demodulated filter, 5 levels: %.4f ms (plain: %.4f ms; five frames: %s)" % (
                      bounces, grid, t, t * 1e6 / (W * H * grid * grid), t / first, " ".join("%.4f" % r for r in traces), float(np.median(guides)),
                      float(np.median(spans)), plain, " ".join("%.4f" % r for r in spans)), flush=True)


def temporal_rates():
    for bounces in (0, 1):
        with api.History(W, H) as hist, api.Frame(scene, p, noise=True, guide_bounces=bounces) as f, api.Frame(scene, api.make_params(W, H, spp, seed=4321), noise=True,
                                                                                                                 guide_bounces=bounces) as g:
            for fr in (f, g):
                fr.render(64)
                fr.render(64)
                fr.denoise(film=film.array, history=hist)   # warm-up; traces the guides; the second call reads what the first one wrote
            rows = []
            for _ in range(5):
                spans = {}
                for levels in (1, 6):
                    for fr in (f, g):
                        fr.denoise(dict(levels=levels), film=film.array, history=hist)
                    spans[levels] = g.denoise_ms()[1]
                rows.append((hist.ms(), (spans[6] - spans[1]) / 5, spans[6]))
            t, level, six = (float(np.median([r[i] for r in rows])) for i in range(3))
            took = float((hist.read()[1] > f.done).mean())
            print("%s %d x %d, %d guide bounces: the temporal kernel %.4f ms = %.3f ns per pixel (five calls: %s); a %s level in the same loop %.4f ms (five: %s): "
                  "temporal / level %.3f; the six-level span with the temporal kernel in it %.4f ms; %.1f %% of the pixels took history" % (
                      what, W, H, bounces, t, t * 1e6 / (W * H), " ".join("%.4f" % r[0] for r in rows), "keyed" if bounces else "plain", level,
                      " ".join("%.4f" % r[1] for r in rows), t / level, six, 100 * took), flush=True)


if ALBEDO:
    albedo_rates()
    sys.exit(0)
if TEMPORAL:
    temporal_rates()
    sys.exit(0)
with api.Frame(scene, p, noise=True) as f:
    f.render(64)
    first = api.kernel_ms()
    f.render(64)
    print("%s %d x %d, %d spp; passes of 64: render kernel %.3f and %.3f ms  [%s]" % (what, W, H, spp, first, api.kernel_ms(), lib.kyhip_last_kernel(0).decode()), flush=True)
    f.noise_stats(0.01)
    up, ms = C.c_float(-1), C.c_float(-1)
    assert lib.kyhip_frame_noise_ms(f._f, C.byref(up), C.byref(ms)) == A.KY_OK
    print("noise update %.4f ms, map + statistics %.4f ms" % (up.value, ms.value))
    f.denoise(film=film.array)   # warm-up; traces the guides
    print("guide trace, once per frame: %.4f ms (%d pixels)" % (f.denoise_ms()[0], W * H), flush=True)
    spans = {}
    for levels in (1, 2, 3, 4, 5, 6):
        runs = []
        for _ in range(5):
            f.denoise(dict(levels=levels), film=film.array)
            runs.append(f.denoise_ms()[1])
        spans[levels] = float(np.median(runs))
        print("filter, %d levels: %.4f ms (five calls: %s)%s" % (levels, spans[levels], " ".join("%.4f" % r for r in runs),
                                                                "" if levels == 1 else "   the level with step %2d: %.4f ms" % (1 << (levels - 1), spans[levels] - spans[levels - 1])), flush=True)
    per_level = (spans[6] - spans[1]) / 5
    print("a level: %.4f ms = %.3f ns per pixel; gather + add: about %.4f ms; the default five levels: %.4f ms = %.3f of a 64-sample pass" % (
        per_level, per_level * 1e6 / (W * H), spans[1] - per_level, spans[5], spans[5] / first))
    a = f.denoise(film=np.zeros((H, W, 3), np.float32))
    b = f.denoise(film=np.zeros((H, W, 3), np.float32))
    print("a pageable film (device film, copy, host add): two calls identical: %s" % np.array_equal(a, b))
# guides beyond the first hit: the chain trace at 1 .. 4 guide bounces, and the keyed level next to the plain one (spans[...] above)
for bounces in range(0, A.GUIDE_MAX_BOUNCES + 1):   # (0: the first-hit trace and the plain filter once more, on a scene that is on the device already)
    with api.Frame(scene, p, noise=True, guide_bounces=bounces) as f:
        f.render(64)
        f.render(64)
        f.denoise(film=film.array)   # warm-up; traces the chains
        keys = f.guide_chains()
        keyed = {}
        for levels in (1, 5, 6):
            runs = []
            for _ in range(5):
                f.denoise(dict(levels=levels), film=film.array)
                runs.append(f.denoise_ms()[1])
            keyed[levels] = float(np.median(runs))
        per_level = (keyed[6] - keyed[1]) / 5
        print("%d guide bounces: %s trace, once per frame: %.4f ms (%d chain pixels, %d unresolved); %s filter, 1 / 5 / 6 levels: %.4f %.4f %.4f ms; a level: "
              "%.4f ms = %.3f ns per pixel (plain, above: %.4f ms); the default five levels: %.4f ms (plain, above: %.4f ms)" % (
                  bounces, "chain" if bounces else "first-hit", f.denoise_ms()[0], int((keys != 0).sum()), int((keys >> np.uint64(62)).sum()),
                  "keyed" if bounces else "plain", keyed[1], keyed[5], keyed[6], per_level,
                  per_level * 1e6 / (W * H), (spans[6] - spans[1]) / 5, keyed[5], spans[5]), flush=True)
