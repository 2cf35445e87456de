"""sample_single_light (direct_sample 49 = KY_DIRECT_SINGLE_LIGHT | KY_DIRECT_BOTH_MIS, ky.cpp:3813-3832) at the interface, without a GPU: the one new
accepted value of ky_render_params.direct_sample, what stays refused, the film bound's answer for it and the host mirror's create_integrator."""
import ctypes as C

import pytest


def test_constants(A):
    assert A.DIRECT_SINGLE_LIGHT == 1 and A.DIRECT_SINGLE_BOTH_MIS == (A.DIRECT_SINGLE_LIGHT | A.DIRECT_BOTH_MIS) == 49


def test_params_accept_49_only(A, api):
    lib = A.load_kyhip()
    ok = api.make_params(64, 64, 16, direct_sample=A.DIRECT_SINGLE_BOTH_MIS, tile_w=32, tile_h=32)
    assert lib.kyhip_shard_float_count(C.byref(ok)) == 4 * 32 * 32 * 3
    for bad in (1, 9, 17, 33, 50, 2 | 48, 1 | 4, 1 | 8, 1 | 16, 1 | 32):
        p = api.make_params(64, 64, 16, direct_sample=bad, tile_w=32, tile_h=32)
        assert lib.kyhip_shard_float_count(C.byref(p)) == A.KY_ERR_INVALID_VALUE, bad
        assert lib.kyhip_film_term_limit(C.byref(p), 5, 0, 1, None) == A.KY_ERR_INVALID_VALUE, bad


def test_film_term_limit_answers_for_49(A, api):
    """The count is both_mis's over all lights (an upper bound: one light per vertex pushes at most two rays); with the queue engine chosen a
    strategy-49 launch runs on the lane engine, so the answer is the lane engine's."""
    lib = A.load_kyhip()
    for spp, depth, n_lights in ((16, 5, 5), (256, 10, 16), (1, 1, 1)):
        p49 = api.make_params(64, 64, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS, max_path_depth=depth)
        p48 = api.make_params(64, 64, spp, direct_sample=A.DIRECT_BOTH_MIS, max_path_depth=depth)
        for deferred in (0, 1):
            l49, l48 = C.c_float(0), C.c_float(0)
            n49 = lib.kyhip_film_term_limit(C.byref(p49), n_lights, 0, deferred, C.byref(l49))
            n48 = lib.kyhip_film_term_limit(C.byref(p48), n_lights, 0, deferred, C.byref(l48))
            assert n49 == n48 > 0 and l49.value == l48.value >= 1.0
            assert lib.kyhip_film_term_limit(C.byref(p49), n_lights, 1, deferred, None) == n49


HOST_PROGRAM = r"""
#include "ky_amd/host/ky.hpp"
#include <cstdio>
int main() {
    using namespace ky;
    const direct_sample_enum_t single = direct_sample_enum_t::sample_single_light | direct_sample_enum_t::both_mis;
    std::printf("value %d\n", (int)single);
    for (int kind : {6, 9, 10, 11, 8, 7}) {
        auto integrator = create_integrator((integrator_enum_t)kind, 5, single, 0);
        std::printf("kind %d %d\n", kind, integrator != nullptr ? 1 : 0);
    }
    return 0;
}
"""


def test_mirror_creates_the_integrator(tmp_path):
    """A C++ caller of the mirror (ky_amd/host/ky.hpp), built as the examples are: create_integrator(kind, depth, sample_single_light | both_mis, device) returns
    an integrator for the kinds that do direct lighting (6, 9, 10, 11) and for 8, which ignores direct_sample; 7 (stochastic_raytracing) stays nullptr (4638)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    src = tmp_path / "mirror.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "mirror"
    lib = os.path.join(root, "ky_amd", "lib")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", root, "-I", os.path.join(root, "include"), "-o", str(exe), str(src), "-L", lib, "-lkyhip",
                           "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert lines[0] == "value 49"
    assert lines[1:7] == ["kind 6 1", "kind 9 1", "kind 10 1", "kind 11 1", "kind 8 1", "kind 7 0"], out.stdout
