#!/usr/bin/env python3
"""Generates tests/golden/denoise_chains.npz: the denoiser's specular chains (include/kyhip.h, kyhip_frame_set_guide_bounces) of the default Cornell box at 40 x 24
as the CPU oracle walks them -- oracle trace_li on every pixel's centre sample under the debug sampler, max_path_depth 8, fed to the chain walk of
tests/denoise_chains_restatement.py at 1, 2 and 4 guide bounces.  No GPU.  tests/test_denoise_chains.py regenerates and compares; the GPU test reads the file.

    python tests/golden/make_denoise_chains.py [out.npz]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np

import denoise_chains_restatement as DC

W, H, BOUNCES = 40, 24, (1, 2, 4)


def oracle_trace():
    """(the scene, trace(x, y) -> the oracle's rows of the pixel's centre sample, each pixel traced once)."""
    from ky_amd import _abi as A, api
    from oracle import kyoracle as O
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
    p = api.make_params(W, H, 1, max_path_depth=8, sampler=A.SAMPLER_DEBUG)
    rows = {}
    return scene, lambda x, y: rows[(x, y)] if (x, y) in rows else rows.setdefault((x, y), O.trace_li(scene, p, x, y, 0))


def oracle_chains(scene=None, trace=None):
    """{"cls_B", "key_B", "ga_B", "gb_B" for B in BOUNCES}: [H, W] float32, [H, W] uint64, [H, W, 4] float32 twice."""
    if trace is None:
        scene, trace = oracle_trace()
    out = {}
    for b in BOUNCES:
        out["cls_%d" % b], out["key_%d" % b], out["ga_%d" % b], out["gb_%d" % b] = DC.chains(trace, scene.c, W, H, b)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "denoise_chains.npz")
    data = oracle_chains()
    np.savez_compressed(path, **data)
    print("%s: %d bytes; at 4 bounces (chain pixels, on a surface, leaving the box, keys apart from 0): %s" % (
        path, os.path.getsize(path), DC.counts(data["cls_4"], data["key_4"])))
