#!/usr/bin/env python3
"""The numbers of DESIGN.md "Adaptive" (profiles/adaptive_rates.txt), table kernels, one GPU.
  tools/adaptive_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5, both_mis; 512 spp)
  tools/adaptive_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720)
1. The indirection's cost: the summed render-kernel time (kyhip_kernel_ms) of a block-tracking frame with the full list of live blocks against a plain frame cut
   into the same passes -- 1, 4 and 16 passes, three runs each after a warm-up, alternating.
2. The retire and compaction kernels per pass (kyhip_frame_blocks_ms: hipEvents around them), next to the noise kernels' (kyhip_frame_noise_ms).
3. The payoff: passes of 64 driven by hand until kyhip_frame_render_until's rule holds over the film, against passes of 64 each followed by
   kyhip_frame_retire_noisy, at the same threshold: summed kernel time, pixel-samples rendered, the statistics of the noise map at the end, and per pass the
   kernel time against the share of blocks still live."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ky_amd import api, _abi as A

what = sys.argv[1] if len(sys.argv) > 1 else "cornell"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 512
lib = A.load_kyhip()
lib.kyhip_set_jit(0)
W, H = (1024, 768) if what == "cornell" else (1280, 720)
scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H) if what == "cornell" else api.mis_scene(W, H)
p = api.make_params(W, H, spp)
want = api.render(scene, p)
print("%s %d x %d, %d spp, %d chunks  [%s]" % (what, W, H, spp, len(api.pass_boundaries(spp)), lib.kyhip_last_kernel(0).decode()), flush=True)


def in_passes(n_passes, blocks):
    per = -(-spp // n_passes)
    total, passes, name = 0.0, 0, ""
    with api.Frame(scene, p, blocks=blocks) as f:
        while f.done < f.total:
            f.render(per)
            total += api.kernel_ms()
            passes += 1
            name = lib.kyhip_last_kernel(0).decode().split(", pass:")[0]
        assert np.array_equal(f.resolve(), want)
    return total, passes, name


print("1. render-kernel time, a block-tracking frame with every block live against a plain frame, the same passes (ms; three runs; film == one shot in every run)")
for n in (1, 4, 16):
    for blocks in (False, True):
        in_passes(n, blocks)   # warm-up
    plain, listed = [], []
    for _ in range(3):   # alternating, so that a drift of the clocks falls on both alike
        plain.append(in_passes(n, False))
        listed.append(in_passes(n, True))
    a, b = np.array([r[0] for r in plain]), np.array([r[0] for r in listed])
    print("  %2d passes: plain %s (spread %.2f %%)   listed %s (spread %.2f %%)   listed / plain, medians: %+.2f %%" % (
        plain[0][1], " ".join("%.3f" % v for v in a), 100 * (a.max() - a.min()) / a.min(), " ".join("%.3f" % v for v in b), 100 * (b.max() - b.min()) / b.min(),
        100 * (np.median(b) / np.median(a) - 1)), flush=True)
print("     plain:  %s\n     listed: %s" % (plain[0][2], listed[0][2]))


def noise_ms(f):
    up, ms = C.c_float(-1), C.c_float(-1)
    assert lib.kyhip_frame_noise_ms(f._f, C.byref(up), C.byref(ms)) == A.KY_OK
    return up.value, ms.value


THRESHOLD, FRACTION, MIN_BATCHES, PER = 0.008, 0.10, 3, 64
print("2. + 3. threshold %.3f, at most %.2f of the pixels (of a block) above it, %d batches, passes of %d" % (THRESHOLD, FRACTION, MIN_BATCHES, PER))
for run in range(2):   # the first is the warm-up
    show = run == 1
    with api.Frame(scene, p, noise=True) as f:
        kernel = 0.0
        while True:
            f.render(PER)
            kernel += api.kernel_ms()
            st = f.noise_stats(THRESHOLD)
            if (st.batches >= MIN_BATCHES and st.above <= np.float64(np.float32(FRACTION)) * (st.pixels - st.flagged)) or f.done >= f.total:
                break
        if show:
            print("  whole frame (render_until's rule): stopped at %d of %d samples, render kernels %.3f ms, %d pixel-samples; map: above %d of %d, mean %.5f, max %.4f" % (
                f.done, spp, kernel, f.done * W * H, st.above, st.pixels, st.mean, st.max), flush=True)
    with api.Frame(scene, p, noise=True, blocks=True) as f:
        kernel, rows = 0.0, []
        n_blocks = f.block_stats().blocks
        while f.block_stats().live > 0 and f.done < f.total:
            live = f.block_stats().live
            f.render(PER)
            ms = api.kernel_ms()
            kernel += ms
            bs = f.retire_noisy(THRESHOLD, FRACTION, MIN_BATCHES)
            rows.append((f.done, live, ms, noise_ms(f), f.blocks_ms(), bs.live))
        st = f.noise_stats(THRESHOLD)
        bs = f.block_stats()
        if show:
            for done, live, ms, (up, mp), (rt, ls), after in rows:
                print("    pass to %4d spp: %6d of %d blocks live (%.3f), render %7.3f ms (%.3f of the first pass); update %.4f ms, map %.4f ms, retire %.4f ms, list %.4f ms; "
                      "%d live behind it" % (done, live, n_blocks, live / n_blocks, ms, ms / rows[0][2], up, mp, rt, ls, after), flush=True)
            print("  per block (render_adaptive's loop): front at %d of %d samples, %d of %d blocks still live, render kernels %.3f ms, %d pixel-samples (%.1f per pixel, "
                  "%d .. %d); map: above %d of %d, mean %.5f, max %.4f" % (f.done, spp, bs.live, bs.blocks, kernel, bs.pixel_samples, bs.pixel_samples / bs.pixels,
                                                                          bs.min_samples, bs.max_samples, st.above, st.pixels, st.mean, st.max), flush=True)
