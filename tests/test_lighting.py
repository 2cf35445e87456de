"""CPU: the host plan of a masked render (kyhip_lighting_plan, include/kyhip.h "Light classes") and its refusals; no device is touched."""
import ctypes as C

import pytest

MASKS = [1, 2, 3, 4, 5, 6, 7, 31]


def expected_plan(integrator, depth, mask):
    """The plan as include/kyhip.h words it: classes the launch can produce, a shorter path without the indirect class, two drop bits for the kernel."""
    m = mask & 7
    can = 3 if integrator == 6 else (1 | (2 if depth >= 1 else 0) | (4 if depth >= 2 else 0))
    m &= can
    if m == 0:
        return -1, 0
    eff = depth
    if integrator != 6 and not m & 4:
        eff = min(depth, 1) if m & 2 else 0
    k1 = integrator == 6 or eff >= 1
    return eff, (0 if m & 1 else 1) | (2 if not m & 2 and k1 else 0)


@pytest.mark.parametrize("integrator", [6, 10, 11])
@pytest.mark.parametrize("depth", [0, 1, 5])
def test_plan_table(integrator, depth, A, api):
    for mask in MASKS:
        got = api.lighting_plan(api.make_params(16, 16, 4, integrator=integrator, max_path_depth=depth), mask)
        assert got == expected_plan(integrator, depth, mask), (integrator, depth, mask, got)


def test_plan_literals(A, api):
    p5, p1, p0 = (api.make_params(16, 16, 4, max_path_depth=d) for d in (5, 1, 0))
    assert [api.lighting_plan(p5, m) for m in MASKS] == [(0, 0), (1, 1), (1, 0), (5, 3), (5, 2), (5, 1), (5, 0), (5, 0)]
    assert [api.lighting_plan(p1, m) for m in MASKS] == [(0, 0), (1, 1), (1, 0), (-1, 0), (0, 0), (1, 1), (1, 0), (1, 0)]
    assert [api.lighting_plan(p0, m) for m in MASKS] == [(0, 0), (-1, 0), (0, 0), (-1, 0), (0, 0), (-1, 0), (0, 0), (0, 0)]
    d5 = api.make_params(16, 16, 4, integrator=A.INTEGRATOR_DIRECT_LIGHTING, max_path_depth=5)
    assert [api.lighting_plan(d5, m) for m in MASKS] == [(5, 2), (5, 1), (5, 0), (-1, 0), (5, 2), (5, 1), (5, 0), (5, 0)]
    assert api.lighting_plan(p5, 7 | 24) == (5, 0) and api.lighting_plan(p5, 4 | 24) == (5, 3)


def test_refusals(A, api):
    lib = A.load_kyhip()
    p = api.make_params(16, 16, 4)
    depth, dropped = C.c_int(77), C.c_int(77)
    for bad in (0, -1, 32, 39, 7 | 8, 7 | 16, 1 | 8, 8, 16, 24):
        assert lib.kyhip_lighting_plan(C.byref(p), bad, C.byref(depth), C.byref(dropped)) == A.KY_ERR_INVALID_VALUE, bad
        assert b"lighting" in lib.kyhip_last_error(), bad
        assert (depth.value, dropped.value) == (77, 77)
    for integrator in (0, 1, 2, 8, 9):
        q = api.make_params(16, 16, 4, integrator=integrator)
        for mask in (1, 2, 3, 4, 5, 6):
            assert lib.kyhip_lighting_plan(C.byref(q), mask, None, None) == A.KY_ERR_INVALID_VALUE, (integrator, mask)
            assert b"integrator %d" % integrator in lib.kyhip_last_error()
        assert api.lighting_plan(q, 7) == (q.max_path_depth, 0) and api.lighting_plan(q, 31) == (q.max_path_depth, 0)
    assert lib.kyhip_lighting_plan(C.byref(api.make_params(16, 16, 0)), 7, None, None) == A.KY_ERR_INVALID_VALUE   # invalid params


def test_check_without_params(A):
    """kyhip_lighting_check: the refusals alone, by integrator and mask (what the mirror's set_lighting asks)"""
    lib = A.load_kyhip()
    for integrator in (6, 10, 11):
        assert all(lib.kyhip_lighting_check(integrator, m) == A.KY_OK for m in MASKS + [7 | 24, 2 | 24])
        assert all(lib.kyhip_lighting_check(integrator, m) == A.KY_ERR_INVALID_VALUE for m in (0, -3, 32, 8, 16, 24, 1 | 8, 7 | 16))
    for integrator in (0, 1, 2, 8, 9):
        assert lib.kyhip_lighting_check(integrator, 7) == A.KY_OK and lib.kyhip_lighting_check(integrator, 31) == A.KY_OK
        assert lib.kyhip_lighting_check(integrator, 3) == A.KY_ERR_INVALID_VALUE and b"integrator %d" % integrator in lib.kyhip_last_error()


def test_the_mirror_throws_for_what_the_library_refuses(A, api):
    """set_lighting / path_tracing_recursion_defered_t's constructor validate the mask when it is set: no device is needed to be told"""
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    for integrator, lighting in ((10, 0), (11, 8), (9, 3), (8, 4), (6, 32), (1, 2)):
        with pytest.raises(api.KyError) as e:
            api.render_host_api(scene, integrator, 5, 48, A.SAMPLER_RANDOM, 1, 16, 16, lighting=lighting)
        assert "lighting" in str(e.value), str(e.value)


def test_a_masked_instantiation_compiles(A, tmp_path, monkeypatch):
    """run-time instantiations take the drop bits as one more template argument (ky_render.hpp): the library's own sources compile with it"""
    import shutil
    if not (shutil.which("hipcc") or __import__("os").path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no ROCm compiler")
    monkeypatch.setenv("KYHIP_CACHE_DIR", str(tmp_path / "cache"))
    lib = A.load_kyhip()
    assert lib.kyhip_jit_compile(b"render_kernel<false, 48, false, false, 263, 11, false, 3>") > 4096, lib.kyhip_jit_status()
    assert lib.kyhip_jit_compile(b"render_kernel<false, 48, false, false, 263, 11, false, 4>") == A.KY_ERR_DEVICE   # two drop bits
