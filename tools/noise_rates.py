#!/usr/bin/env python3
"""The numbers of DESIGN.md "Noise" (profiles/noise_rates.txt), table kernels, one GPU: what a frame's noise estimate costs next to its passes.
  tools/noise_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5, both_mis; 512 spp)
  tools/noise_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720)
The frame tracks noise and is rendered in passes of at least 64 samples, then again with one chunk per pass.  Per pass: the pass's render kernel
(kyhip_kernel_ms), the update kernel behind it and the map + statistics kernels of one kyhip_frame_noise_stats call (kyhip_frame_noise_ms: hipEvents on the
frame's stream around them), and the two as a share of the render kernel's time.  The complete frame is checked against the one-shot film, bit for bit."""
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
print("%s %d x %d, %d spp, %d chunks  [%s]" % (what, W, H, spp, len(api.pass_boundaries(spp)), lib.kyhip_last_kernel(0).decode()))


def frame(min_samples, show):
    rows = []
    with api.Frame(scene, p, noise=True) as f:
        while f.done < f.total:
            done = f.render(min_samples)
            kernel = api.kernel_ms()
            st = f.noise_stats(0.01)
            up, ms = C.c_float(-1), C.c_float(-1)
            assert lib.kyhip_frame_noise_ms(f._f, C.byref(up), C.byref(ms)) == A.KY_OK
            rows.append((done, kernel, up.value, ms.value, st))
            if show:
                print("  pass to %4d spp: render %8.3f ms, update %.4f ms, map + stats %.4f ms (%.2f %% of the pass); above 0.01: %d of %d, mean %.4g" % (
                    done, kernel, up.value, ms.value, 100.0 * (up.value + ms.value) / kernel, st.above, st.pixels, st.mean), flush=True)
        same = np.array_equal(f.resolve(), want)
    k, u, m = (sum(r[i] for r in rows) for i in (1, 2, 3))
    print("%d passes (>= %d spp): render %.2f ms, update %.3f ms (%.3f per pass, %.1f GB/s of 56 bytes per pixel: 24 + 16 read, 16 written), map + stats %.3f ms (%.3f per pass); "
          "noise / render %.2f %%; film == one shot: %s" % (len(rows), min_samples, k, u, u / len(rows), 56.0 * W * H / (u / len(rows) * 1e-3) / 1e9, m,
                                                            m / len(rows), 100.0 * (u + m) / k, same), flush=True)


for min_samples in (64, 1):
    frame(min_samples, False)          # warm-up
    frame(min_samples, min_samples == 64)
