#!/usr/bin/env python3
"""The numbers of DESIGN.md section 3 "One light per vertex" (profiles/single_light_rates.txt), table kernels, one GPU:
  tools/single_light_rates.py veach <strategy> [spp]     kernel time of three renders after a warm-up, bench.py --workload veach's geometry (1280 x 720, depth 5)
  tools/single_light_rates.py unspec <strategy> [spp]    the same for configs[1]'s scene with kyhip_set_specialisation(0): strategy 32 runs the run-time-dispatched kernel
  tools/single_light_rates.py equal-time <budget ms> [reference spp]
      both_mis (48) at 4096 spp and sample_single_light (49, and 113 / 177: its light picked by power / by position) at the spp each reaches in <budget ms> of kernel time (its own full-frame rate, measured here),
      each against the oracle's both_mis film at <reference spp> under another seed, on the six tiles tests/test_configs_gpu.py takes of this frame
  tools/single_light_rates.py reference <reference spp> <file.npz>     only that oracle film (no GPU), saved; equal-time takes the file as a fourth argument
KYHIP_LIB selects another build of the library (tools/mkvariant.sh).  The file uses nothing that strategy 49 added to the Python package, so a copy of it in a
checkout of an earlier commit gives that commit's lines."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ky_amd import api, _abi as A

what = sys.argv[1]
build = os.path.basename(os.environ.get("KYHIP_LIB", "libkyhip.so"))
W, H = 1280, 720
TILES = [(20, 30), (40, 33), (60, 36), (10, 42), (70, 8), (52, 20)]   # tests/test_configs_gpu.py, test_c3_veach_full_size


def one_tile(p, tx, ty):
    q = A.RenderParams.from_buffer_copy(p)
    tiles_x = (p.width + p.tile_w - 1) // p.tile_w
    q.tile_first, q.tile_step = ty * tiles_x + (tx - ty) % tiles_x, 1 << 30   # (include/kyhip.h: tile rows are rotated by their index)
    return q


def cut(film, p, tx, ty):
    return film[ty * p.tile_h:(ty + 1) * p.tile_h, tx * p.tile_w:(tx + 1) * p.tile_w].astype(np.float64)


def reference(scene, ref_spp):
    from oracle import kyoracle as O
    return {t: cut(O.render(scene, one_tile(api.make_params(W, H, ref_spp, seed=99), *t)), api.make_params(W, H, 1), *t) for t in TILES}


if what == "reference":
    tiles = reference(api.mis_scene(W, H), int(sys.argv[2]))
    np.savez(sys.argv[3], spp=int(sys.argv[2]), **{"%d_%d" % t: v for t, v in tiles.items()})
    sys.exit(0)
lib = A.load_kyhip()
lib.kyhip_set_jit(0)


def timed(scene, p, runs=3):
    api.render(scene, p)
    ms = []
    for _ in range(runs):
        film = api.render(scene, p)
        ms.append(api.kernel_ms())
    return ms, film


if what in ("veach", "unspec"):
    strategy = int(sys.argv[2])
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    if what == "veach":
        scene = api.mis_scene(W, H)
    else:
        W, H = 1024, 768
        scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
        lib.kyhip_set_specialisation(0)
    ms, film = timed(scene, api.make_params(W, H, spp, direct_sample=strategy))
    print("%s %s strategy %d spp %d: kernel ms %s  Gsamples/s %s  film mean %.6f  [%s]" % (
        what, build, strategy, spp, " ".join("%.2f" % m for m in ms), " ".join("%.3f" % (W * H * spp / m / 1e6) for m in ms), film.mean(),
        lib.kyhip_last_kernel(0).decode()), flush=True)
else:
    assert what == "equal-time"
    budget_ms = float(sys.argv[2])
    ref_spp = int(sys.argv[3]) if len(sys.argv) > 3 else 131072
    scene = api.mis_scene(W, H)
    SINGLE = (49, 113, 177)   # sample_single_light with its light picked uniformly, by power, by position at the vertex
    ms48, _ = timed(scene, api.make_params(W, H, 4096, direct_sample=48))
    spp, ms = {48: 4096}, {48: ms48}
    for strategy in SINGLE:
        ms[strategy], _ = timed(scene, api.make_params(W, H, 4096, direct_sample=strategy))
        spp[strategy] = int(4096 * budget_ms / min(ms[strategy]))
    print("equal-time %s: budget %.1f ms of kernel time (both_mis at 4096 spp on the commit before); here at 4096 spp 48 takes %.1f ms, %s" % (
        build, budget_ms, min(ms48), ", ".join("%d %.1f ms -> %d spp" % (k, min(ms[k]), spp[k]) for k in SINGLE)), flush=True)
    t0 = time.time()
    if len(sys.argv) > 4:
        saved = np.load(sys.argv[4])
        assert int(saved["spp"]) == ref_spp
        ref = {t: saved["%d_%d" % t] for t in TILES}
    else:
        ref = reference(scene, ref_spp)
    print("reference: the oracle's both_mis at %d spp, seed 99, %d tiles of 16 x 16 in %.0f s (its own noise adds %s %% to the squared errors below)" % (
        ref_spp, len(TILES), time.time() - t0, " / ".join("%.1f" % (100.0 * spp[k] / ref_spp) for k in (48,) + SINGLE)), flush=True)
    print("%-12s %8s  %s  %9s" % ("strategy", "spp", "  ".join("tile %-8s" % (t,) for t in TILES), "all tiles"))
    total = {}
    for strategy in (48,) + SINGLE:
        p = api.make_params(W, H, spp[strategy], direct_sample=strategy)
        err = [cut(api.render(scene, one_tile(p, *t)), p, *t) - ref[t] for t in TILES]
        total[strategy] = float(np.sqrt(np.mean(np.concatenate([e.ravel() for e in err]) ** 2)))
        print("%-12s %8d  %s  %9.3e" % ("both_mis 48" if strategy == 48 else "single %d" % strategy, spp[strategy], "  ".join("%-13.3e" % np.sqrt(np.mean(e ** 2)) for e in err), total[strategy]))
    best = min(total, key=total.get)
    print("lowest error at equal kernel time: %d (RMSE ratios to 48: %s)" % (best, ", ".join("%d %.2f" % (k, total[k] / total[48]) for k in SINGLE)))
