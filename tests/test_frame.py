"""CPU: the host arithmetic of a frame rendered in passes (include/kyhip.h, kyhip_frame_*) -- where a pass can end, and what a frame refuses before it
looks for a device.  The expected boundaries are derived by hand from the chunk schedule (ky_amd/csrc/ky_shard.hpp): the last 64 samples go in chunks of
4, the 128 before them in 8s, the 256 before those in 16s, and what is left in front in 24s -- whole ones: the rest of the last 24 joins the 16s."""
import ctypes as C
import os

import pytest


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
