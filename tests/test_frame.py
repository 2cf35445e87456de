"""CPU: the host arithmetic of a frame rendered in passes (include/kyhip.h, kyhip_frame_*) -- where a pass can end, and what a frame refuses before it
looks for a device.  The expected boundaries are derived by hand from the chunk schedule (ky_amd/csrc/ky_shard.hpp): the last 64 samples go in chunks of
4, the 128 before them in 8s, the 256 before those in 16s, and what is left in front in 24s -- whole ones: the rest of the last 24 joins the 16s."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import blocks_restatement as B
import noise_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_MAGIC = 0x31454D4152464B59   # "YKFRAME1"


def test_pass_boundaries_by_hand(api):
    b = api.pass_boundaries
    assert b(1) == [1]
    assert b(7) == [4, 7]
    assert b(64) == list(range(4, 65, 4))
    assert b(65) == [1] + list(range(5, 66, 4))               # one sample is left for the 8-sample segment
    assert b(471)[0] == 16 and 24 not in b(471)               # 23 samples before the taper: no whole bulk chunk
    assert b(472)[:2] == [24, 40]                             # 24: one
    v = b(500)   # taper from 52: bulk chunks cover [0, 48), 16s [48, 308), 8s [308, 436), 4s [436, 500)
    assert len(v) == 51 and v[:4] == [24, 48, 64, 80] and v[-2:] == [496, 500]
    i = v.index(304)
    assert v[i:i + 3] == [304, 308, 316]
    i = v.index(436)
    assert v[i:i + 2] == [436, 440]


def test_pass_boundaries_ascend_to_spp_in_steps_of_at_most_a_bulk_chunk(api):
    for spp in list(range(1, 131)) + list(range(447, 476)) + [1000, 1024, 4096]:
        v = api.pass_boundaries(spp)
        steps = [b - a for a, b in zip([0] + v, v)]
        assert v[-1] == spp and min(steps) >= 1 and max(steps) <= 24, (spp, v)


def test_pass_boundaries_arguments(A, api):
    lib = A.load_kyhip()
    assert lib.kyhip_pass_boundaries(0, None, 0) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_pass_boundaries(-5, None, 0) == A.KY_ERR_INVALID_VALUE
    with pytest.raises(api.KyError):
        api.pass_boundaries(0)
    out = (C.c_int * 4)(-1, -1, -1, -1)
    assert lib.kyhip_pass_boundaries(500, out, 3) == 51       # a short array still learns the count ...
    assert list(out) == [24, 48, 64, -1]                      # ... and holds what fits


def test_frame_refuses_invalid_params_before_any_device(A, api):
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    for bad in (api.make_params(16, 16, 0), api.make_params(16, 16, 4, integrator=7), api.make_params(16, 16, 4, direct_sample=50),
                api.make_params(16, 16, 4, tile_w=30)):
        f = C.c_void_p()
        assert lib.kyhip_frame_begin(0, scene.flat, C.byref(bad), C.byref(f)) == A.KY_ERR_INVALID_VALUE
        assert not f.value and b"invalid render params" in lib.kyhip_last_error()
    lib.kyhip_frame_end(None)   # returns


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_frame_without_a_gpu_is_a_loud_error(A, api):
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    p = api.make_params(16, 16, 8)
    f = C.c_void_p()
    assert lib.kyhip_frame_begin(0, scene.flat, C.byref(p), C.byref(f)) == A.KY_ERR_NO_DEVICE and not f.value
    with pytest.raises(api.KyError):
        api.Frame(scene, p)


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_checkpoint (ky_amd/csrc/ky_hostcheck.cpp): the sanitizer build when the suite runs inside `make sanitize`, else the
    same host-only sources built plainly."""
    if A.SANITIZE:
        lib = A.load_kyhip()
    else:
        target = os.path.join("build", "san", "libkyhip_host_plain.so")
        r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(os.path.join(ROOT, target))
    lib.kyhip_last_error.restype, lib.kyhip_last_error.argtypes = C.c_char_p, []
    lib.kyhostcheck_checkpoint.restype = C.c_int
    lib.kyhostcheck_checkpoint.argtypes = [A.PP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_int), C.c_void_p, C.c_size_t]
    return lib


@pytest.mark.parametrize("shard,n_tiles", [({}, 6), (dict(tile_first=1, tile_step=2), 3), (dict(tile_first=6), 0)])
def test_checkpoint_round_trip(shard, n_tiles, A, api, check):
    """A whole checkpoint written and read back without a device (ky_amd/csrc/ky_checkpoint.hpp): the block tests' frame -- 40 x 24 in tiles of 16, six tiles with
    ragged edge tiles, 24 blocks -- whole, as every second tile, and as a shard without tiles, for all four (noise, blocks).  The parts lie where the restatements
    of tests/noise_restatement.py and tests/blocks_restatement.py put them, back to back; the counts come back; the buffer cut by one byte at any part's end and
    the state of a frame with the other `blocks` are refused."""
    p = api.make_params(40, 24, 500, **shard)
    n_pix, n_blocks = n_tiles * 256, n_tiles * 4
    bounds = api.pass_boundaries(500)
    for noise, blocks, done in itertools.product((False, True), (False, True), (0, 24, 224, 500)):
        passes = bounds.index(done) + 1 if done else 0
        batches = passes if noise else 0           # what a frame rendered one chunk per pass would have
        # block 0 retired at the first pass (or at 0 before one), block 1 now, the others live; a frame without a noise estimate has no batch counts
        pairs = np.array([(-1, 0)] * n_blocks, np.int32).reshape(n_blocks, 2)
        if n_blocks:
            pairs[0] = (min(done, 24), 1 if noise and done else 0)
            pairs[1] = (done, batches)
        counts_in = (C.c_int * 4)(done, batches, done, passes + 3)
        at = (C.c_size_t * 6)()
        back = (C.c_int * 5)(*[-9] * 5)
        want_at = [R.HEADER_BYTES, R.HEADER_BYTES + n_pix * 28]
        want_at.append(want_at[-1] + (R.TRAILER_BYTES if noise else 0))
        want_at.append(want_at[-1] + (n_pix * 16 if noise else 0))
        want_at.append(want_at[-1] + (B.BLOCK_TRAILER_BYTES if blocks else 0))
        want_at.append(want_at[-1] + (8 * n_blocks if blocks else 0))
        total = want_at[-1]
        state = (C.c_ubyte * total)()
        def rc(check_bytes=total, check_blocks=blocks, out=None):
            return check.kyhostcheck_checkpoint(C.byref(p), noise, blocks, check_blocks, counts_in, pairs.ctypes.data_as(C.POINTER(C.c_int32)), check_bytes, at,
                                                back, out, total if out is not None else 0)
        assert rc(out=state) == A.KY_OK, check.kyhip_last_error()
        assert list(at) == want_at and sorted(at) == list(at)                       # the stated order, back to back: a part ends where the next begins
        if n_tiles == 0:                                                             # a shard without tiles: the header, and the two 16-byte trailers when it tracks
            assert total == R.HEADER_BYTES + (16 if noise else 0) + (16 if blocks else 0)
        assert list(back) == [passes, done, batches, done if noise else 0, passes + 3 if blocks else 0]
        # the bytes, read by the restatements
        raw = bytes(state)
        assert struct.unpack_from("<Q", raw, 0)[0] == (B.FRAME_BLOCKS_MAGIC if blocks else FRAME_MAGIC)
        if blocks:
            raw, got_pairs = B.split_blocks(raw, n_pix, n_blocks, noise)
            assert np.array_equal(got_pairs, pairs) and struct.unpack_from("<i", bytes(state), len(raw) + 12)[0] == passes + 3
        got_done, accum, flags, trailer = R.split_state(raw, n_pix)
        assert got_done == done and not np.any(accum) and not np.any(flags)
        assert (trailer is not None) == noise and (not noise or (tuple(trailer[:2]) == (batches, done) and not np.any(trailer[2]) and not np.any(trailer[3])))
        # one byte short of any part's end: refused
        for end in sorted(set(at)):
            assert rc(check_bytes=end - 1) == A.KY_ERR_INVALID_VALUE and b"frame state" in check.kyhip_last_error(), (noise, blocks, done, end)
        assert rc() == A.KY_OK
        # ... and by a frame with the other `blocks`: the header's magic
        assert rc(check_blocks=not blocks) == A.KY_ERR_INVALID_VALUE and b"pixel blocks" in check.kyhip_last_error()


CHILD = '''
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
from ky_amd import _abi as A, api
lib = A.load_kyhip()
assert A.SANITIZE == "asan"
for spp in list(range(1, 131)) + list(range(447, 476)) + [1000, 4096]:
    v = api.pass_boundaries(spp)
    assert v[-1] == spp and len(v) == lib.kyhostcheck_chunks(spp), spp
    short = (C.c_int * 2)()
    assert lib.kyhip_pass_boundaries(spp, short, 2) == len(v) and list(short)[:len(v)] == v[:2]
    for min_samples in (1, 7, 100, spp):
        p = api.make_params(40, 24, spp)
        n = lib.kyhostcheck_frame(C.byref(p), min_samples)
        assert n >= 1 and (n == len(v) if min_samples == 1 else n <= len(v)) and (n == 1 if min_samples == spp else True), (spp, min_samples, n)
assert lib.kyhip_pass_boundaries(0, None, 0) == A.KY_ERR_INVALID_VALUE
print("frame bookkeeping ok")
'''


@pytest.mark.skipif(os.environ.get("KY_SANITIZE") is not None, reason="already inside `make sanitize`'s sanitized pytest run")
def test_frame_bookkeeping_under_asan():
    """The frame's host side -- pass boundaries, which chunks a pass takes, what a checkpoint's header must agree in -- under -fsanitize=address,undefined, in a
    child process with the sanitizer runtime preloaded (tests/test_sanitize.py's way; kyhostcheck_frame, ky_amd/csrc/ky_hostcheck.cpp)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-s", "-C", root, os.path.join("build", "san", "libkyhip_host_asan.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = lambda name: subprocess.check_output(["g++", "-print-file-name=" + name], text=True).strip()
    env = dict(os.environ, KY_SANITIZE="asan", LD_PRELOAD=lib("libasan.so") + " " + lib("libubsan.so"), ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": root}], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    for mark in ("ERROR: AddressSanitizer", "runtime error:"):
        assert mark not in out, out[-4000:]
    assert r.returncode == 0 and "frame bookkeeping ok" in out, out[-3000:]
