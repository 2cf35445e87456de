"""CPU: the film's range rule (DESIGN.md "Film").  A launch adds each pixel's radiance to a signed 32.32 fixed-point word in terms; the host
counts N, the most terms one word can receive in the launch, and gives the kernels the term limit T: a term at or beyond +-T is flagged, not
added.  For every launch the ABI accepts, N T <= 2^31 (the word cannot wrap) and T >= 1 (a flagged non-negative term alone makes the pixel 1);
a launch for which no such T exists is refused with KY_ERR_LIMIT."""
import ctypes as C
from fractions import Fraction

import numpy as np

from helpers import CustomScene, chunk_count as _chunk_count, make_light, make_material, make_shape


def _model_terms(A, spp, depth, n_lights, strategy, integrator, engine, deferred):
    """The count as DESIGN.md "Film" states it, which this test holds the host to (the kernels are held to it on the GPU, tests/test_film_accumulator_gpu.py): the queue engine adds one term per sample (film_add_sample); the lane engine one per chunk, plus, with
    deferred shadow rays, one per ray -- per sample at most `depth` shaded vertices, each pushing one ray per light (two under both_mis)."""
    iteration = integrator == A.INTEGRATOR_PATH_TRACING_ITERATION
    if engine == 1 and iteration:
        return spp
    n = _chunk_count(spp)
    per_light = {A.DIRECT_BOTH_MIS: 2, A.DIRECT_LIGHT_MIS: 1, A.DIRECT_LIGHT: 1}.get(strategy, 0)
    if deferred and iteration:
        n += spp * depth * n_lights * per_light
    return n


def test_chunk_count_model(A, api):
    """the chunk plan this file's model uses is the library's: without lights (or on the lane engine without deferred rays) N is the chunk count"""
    lib = A.load_kyhip()
    for spp in range(1, 3000):
        assert lib.kyhip_film_term_limit(C.byref(api.make_params(8, 8, spp)), 0, 0, 1, None) == _chunk_count(spp), spp


def test_term_limit_keeps_the_word_in_range(A, api):
    lib = A.load_kyhip()
    two31 = Fraction(2 ** 31)
    strategies = (A.DIRECT_IDLE, A.DIRECT_BSDF, A.DIRECT_LIGHT, A.DIRECT_BSDF_MIS, A.DIRECT_LIGHT_MIS, A.DIRECT_BOTH_MIS)
    integrators = (A.INTEGRATOR_PATH_TRACING_ITERATION, A.INTEGRATOR_PATH_TRACING_RECURSION, A.INTEGRATOR_DIRECT_LIGHTING)
    spps = (1, 2, 3, 24, 25, 64, 449, 1024, 4097, 65536, 1 << 20, (1 << 24) - 1, 1 << 24)
    accepted = refused = 0
    lim = C.c_float()
    for spp in spps:
        for depth in (0, 1, 5, 16, 250):
            for n_lights in (0, 1, 2, 5, 16):
                for strategy in strategies:
                    for integrator in integrators:
                        p = api.make_params(64, 48, spp, integrator=integrator, max_path_depth=depth, direct_sample=strategy)
                        for engine in (0, 1):
                            for deferred in (0, 1):
                                want = _model_terms(A, spp, depth, n_lights, strategy, integrator, engine, deferred)
                                lim.value = -1.0
                                n = lib.kyhip_film_term_limit(C.byref(p), n_lights, engine, deferred, C.byref(lim))
                                what = (spp, depth, n_lights, strategy, integrator, engine, deferred)
                                if want > 2 ** 31:   # no T >= 1 with N T <= 2^31
                                    assert n == A.KY_ERR_LIMIT and lim.value == 0.0, (what, n, lim.value)
                                    refused += 1
                                    continue
                                assert n == want, (what, n, want)
                                t = Fraction(float(lim.value))
                                assert 1 <= t <= Fraction(2e9) and n * t <= two31, (what, n, lim.value)
                                # and no larger float would do: T is 2^31 / N rounded down (or the 2e9 the conversion allows)
                                up = Fraction(float(np.nextafter(np.float32(lim.value), np.float32(np.inf))))
                                assert t == Fraction(2e9) or n * up > two31, (what, n, lim.value)
                                accepted += 1
    assert accepted > 0 and refused > 0
    # parameters the ABI refuses anyway
    bad = api.make_params(64, 48, 4, tile_w=30)
    assert lib.kyhip_film_term_limit(C.byref(bad), 1, 0, 0, None) == A.KY_ERR_INVALID_VALUE
    ok = api.make_params(64, 48, 4)
    assert lib.kyhip_film_term_limit(C.byref(ok), -1, 0, 0, None) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_film_term_limit(C.byref(ok), 1, 2, 0, None) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_film_term_limit(C.byref(ok), 1, 0, 0, None) == _chunk_count(4)
    assert lib.kyhip_film_term_limit(C.byref(ok), A.MAX_LIGHTS, 0, 1, None) > 0
    assert lib.kyhip_film_term_limit(C.byref(ok), A.MAX_LIGHTS + 1, 0, 1, None) == A.KY_ERR_INVALID_VALUE   # (and no overflow of the count)


def test_render_refuses_a_launch_without_a_term_limit(A, api):
    """kyhip_render refuses, before it touches a device, a launch whose count (with deferred shadow rays, the largest) leaves no T >= 1:
    2^24 spp at depth 250 with 16 lights under both_mis is 2.7e11 terms"""
    lib = A.load_kyhip()
    cam = A.Camera.from_buffer_copy(api.cornell_box_scene(A.CB_DEFAULT_SCENE, 8, 8).c.camera)
    lights = [make_light(A, A.LIGHT_POINT, (1.0, 1.0, 1.0), position=(0.1 * i, 0.5, 1.0)) for i in range(A.MAX_LIGHTS)]
    scene = CustomScene(A, cam, [make_shape(A, A.SHAPE_SPHERE, [(0, 0, 0)], radius=1.0)], [make_material(A, A.MATERIAL_MATTE, (1, 1, 1))], lights, [])
    scene.scene.surface_count = 0
    p = api.make_params(8, 8, 1 << 24, max_path_depth=250, direct_sample=A.DIRECT_BOTH_MIS)
    assert lib.kyhip_film_term_limit(C.byref(p), A.MAX_LIGHTS, 0, 1, None) == A.KY_ERR_LIMIT
    film = np.zeros((8, 8, 3), np.float32)
    assert lib.kyhip_render(0, scene.flat, C.byref(p), C.c_void_p(film.ctypes.data), 8) == A.KY_ERR_LIMIT
    assert b"too many terms per pixel" in lib.kyhip_last_error()
