"""Oracle-only controls of tests/test_lighting_gpu.py (CPU): on the scenes and pixels those tests use, the unmasked oracle itself says that every light class is
there to be found -- a kernel that dropped nothing, or the wrong term, would fail them -- and that the pixels marked for it receive emission through exactly
one and exactly two specular bounces (direct and indirect light by the k rule, include/kyhip.h "Light classes")."""
import numpy as np
import pytest

import lighting_scenes as L


@pytest.fixture(scope="module")
def terms(A, api, O):
    out = {}
    for name, (scene, w, h, _) in L.scenes(A, api).items():
        if name not in L.CONTROLLED:
            continue
        p = L.params(api, A, name, w, h)
        out[name] = [L.oracle_terms(A, O, scene, p, x, y, L.N_SAMPLES) for (x, y) in L.PIXELS[name]]
    return out


@pytest.mark.parametrize("name", L.CONTROLLED)
def test_every_class_is_present_on_a_quarter_of_the_pixels(name, terms):
    t = terms[name]
    n = len(t)
    emit = sum(bool(np.abs(l0).max() > 0) for l0, l1, lD in t)
    direct = sum(bool(np.abs(l1 - l0).max() > 0) for l0, l1, lD in t)
    indirect = sum(bool(np.abs(lD - l1).max() > 0) for l0, l1, lD in t)
    print(name, "pixels with emit / direct / indirect:", emit, direct, indirect, "of", n)
    assert 4 * emit >= n and 4 * direct >= n and 4 * indirect >= n, (emit, direct, indirect, n)


def test_the_open_room_is_lit_by_misses_of_every_class(A, api, O):
    """the scene that stands for "a miss is the emitter": an environment light and nothing else, seen by a quarter of ALL camera rays, and by paths after one and two bounces"""
    scene, w, h, _ = L.scenes(A, api)["open"]
    assert scene.scene.light_count == 1 and scene.scene.environment_light == 0 and scene.lights[0].kind == A.LIGHT_ENVIRONMENT
    p = L.params(api, A, "open", w, h, spp=4)
    f0, f1, f5 = (O.render(scene, L.at_depth(A, p, d)).astype(np.float64) for d in (0, 1, 5))
    assert (f0.max(axis=2) > 0).mean() >= 0.25
    assert (f1 - f0).mean() > 0.05 and (f5 - f1).mean() > 0.05


@pytest.mark.parametrize("name", ["cornell", "default", "open"])
def test_marked_pixels_receive_emission_through_specular_bounces(name, A, api, O):
    scene, w, h, _ = L.scenes(A, api)[name]
    p = L.params(api, A, name, w, h)
    assert L.ONE_SPECULAR[name] in L.PIXELS[name]
    one, _ = L.specular_emission(A, O, scene, p, *L.ONE_SPECULAR[name], L.N_SAMPLES)
    assert one >= 1, one
    if name in L.TWO_SPECULAR:
        assert L.TWO_SPECULAR[name] in L.PIXELS[name]
        _, two = L.specular_emission(A, O, scene, p, *L.TWO_SPECULAR[name], L.N_SAMPLES)
        assert two >= 1, two


def test_identity_reassembles_the_unmasked_radiance(terms):
    for l0, l1, lD in terms["cornell"]:
        np.testing.assert_allclose(L.identity(1, l0, l1, lD) + L.identity(2, l0, l1, lD) + L.identity(4, l0, l1, lD), lD, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(L.identity(7, l0, l1, lD), L.identity(5, l0, l1, lD) + L.identity(2, l0, l1, lD))
