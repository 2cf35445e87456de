#!/usr/bin/env python3
"""The numbers of DESIGN.md "Slices" (profiles/merge_rates.txt), table kernels, one GPU: what merging two frames' sample ranges costs.
  tools/merge_rates.py cornell [spp]   configs[1]'s geometry (1024 x 768, Cornell box with the lamp, depth 5, both_mis; 512 spp)
  tools/merge_rates.py veach [spp]     bench.py --workload veach's geometry (1280 x 720)
Two slices of the frame render one pass of at least 64 samples each (kyhip_kernel_ms: the yardstick of what a merge is next to).  Then, REPEATS times after
WARMUP untimed rounds and alternating in one loop: a fresh collector merges both slices frame to frame (kyhip_frame_merge_ms: hipEvents around the merge kernel,
which reads two accumulator blocks and writes one), and one hipMemcpyDtoDAsync of one block's bytes between two device buffers (torch events on the same stream: it
reads one block and writes one).  With noise the blocks are 44 bytes per pixel (three 64-bit words, a flag word, a 16-byte pair), else 28.  Medians, the spread,
the merge's rate over the 3 blocks it moves, and merge / copy: the byte counts alone would give 1.5.  The merged collector is checked against the NumPy sum of the
slices' saved words."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ky_amd import api, _abi as A

WARMUP, REPEATS = 5, 30
what = sys.argv[1] if len(sys.argv) > 1 else "cornell"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 512
lib = A.load_kyhip()
hip = A.load_hip_runtime()
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
lib.kyhip_set_jit(0)
W, H = (1024, 768) if what == "cornell" else (1280, 720)
scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H) if what == "cornell" else api.mis_scene(W, H)
p = api.make_params(W, H, spp)
n_pix = int(lib.kyhip_shard_float_count(C.byref(p))) // 3
bounds = api.slice_bounds(spp, 2)
dev = torch.device("cuda", 0)
print("%s %d x %d (%d pixels of the compact tile buffer), %d spp in two slices %s" % (what, W, H, n_pix, spp, bounds))


def median_and_spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


for noise in (False, True):
    per_pixel = 44 if noise else 28
    block = n_pix * per_pixel
    src, dst = torch.zeros(block, dtype=torch.uint8, device=dev), torch.empty(block, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    with api.Frame(scene, p, noise=noise, slice=(bounds[0], bounds[1])) as a, api.Frame(scene, p, noise=noise, slice=(bounds[1], bounds[2])) as b:
        pass_done = a.render(64)
        pass_ms = api.kernel_ms()
        kernel = lib.kyhip_last_kernel(0).decode()
        b.render(64)
        merges, copies = [], []
        for r in range(WARMUP + REPEATS):
            with api.Frame(scene, p, noise=noise, slice=(0, 0)) as collector:
                collector.merge(a)
                first = collector.merge_ms()
                collector.merge(b)
                second = collector.merge_ms()
                if r == 0:   # what the kernel computed, once: the words of both slices added
                    skip = 8 + 8 + 12 * 4 + 8 + 4 + 4
                    words = [np.frombuffer(f.save(), np.int64, n_pix * 3, skip) for f in (collector, a, b)]
                    assert np.array_equal(words[0], words[1] + words[2]) and collector.done == a.done + b.done
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), block, stream.cuda_stream) == 0
            e1.record(stream)
            e1.synchronize()
            if r >= WARMUP:
                merges += [first, second]
                copies.append(e0.elapsed_time(e1))
    m, m_lo, m_hi = median_and_spread(merges)
    c, c_lo, c_hi = median_and_spread(copies)
    print("noise %-3s %d bytes per pixel, blocks of %.1f MB: merge %.4f ms (%.4f .. %.4f over %d), %.0f GB/s of 3 blocks; DtoD copy of one block %.4f ms "
          "(%.4f .. %.4f over %d), %.0f GB/s of 2 blocks; merge / copy %.2f (bytes alone: 1.50); a pass to %d spp renders in %.3f ms: merge / pass %.3f %%  [%s]" % (
              "on:" if noise else "off:", per_pixel, block / 1e6, m, m_lo, m_hi, len(merges), 3.0 * block / (m * 1e-3) / 1e9, c, c_lo, c_hi, len(copies),
              2.0 * block / (c * 1e-3) / 1e9, m / c, pass_done, pass_ms, 100.0 * m / pass_ms, kernel), flush=True)
