"""sample_single_light's pick by power (direct_sample 113) and by position at the vertex (177) without a GPU: the two accepted values and what stays refused, the
film bound's answer, the host's tables (kyhip_scene_light_pick: emitter proxies and the power rule's probabilities) against the NumPy restatement, and the
restatement's own properties (tests/light_pick_restatement.py)."""
import ctypes as C

import numpy as np
import pytest

import light_pick_restatement as R
from helpers import CustomScene, make_light, make_material, make_shape
from light_pick_replay import Replay
from single_light_scenes import STAT_SPP, luminance, sixteen_lights_scene, stat_case, z_scores, z_verdict

REFUSED = (64, 128, 65, 129, 112, 176, 240, 241)


def test_constants(A):
    assert (A.DIRECT_PICK_POWER, A.DIRECT_PICK_SPATIAL) == (64, 128)
    assert A.DIRECT_SINGLE_POWER == (A.DIRECT_SINGLE_BOTH_MIS | A.DIRECT_PICK_POWER) == 113
    assert A.DIRECT_SINGLE_SPATIAL == (A.DIRECT_SINGLE_BOTH_MIS | A.DIRECT_PICK_SPATIAL) == 177
    assert A.PICK_UNIFORM_SHARE == R.SHARE and A.MAX_PROXIES == R.MAX_PROXIES
    assert C.sizeof(A.RenderParams) == 48                     # ky_render_params keeps its size


def test_accepted_and_refused_values(A, api):
    """113 and 177 pass valid_params at every entry that checks it first; the pick flags alone, together, or on another strategy are refused like 50."""
    lib = A.load_kyhip()
    scene = api.mis_scene(16, 16)
    for good in (A.DIRECT_SINGLE_POWER, A.DIRECT_SINGLE_SPATIAL):
        p = api.make_params(16, 16, 4, direct_sample=good)
        assert lib.kyhip_film_term_limit(C.byref(p), 5, 0, 1, None) > 0
        assert lib.kyhip_lighting_plan(C.byref(p), 7, None, None) == A.KY_OK
        f = C.c_void_p()
        rc = lib.kyhip_frame_begin(0, scene.flat, C.byref(p), C.byref(f))
        assert rc in (A.KY_OK, A.KY_ERR_NO_DEVICE), (good, rc, lib.kyhip_last_error())
        if f.value:
            lib.kyhip_frame_end(f)
    for bad in REFUSED:
        p = api.make_params(16, 16, 4, direct_sample=bad)
        assert lib.kyhip_film_term_limit(C.byref(p), 5, 0, 1, None) == A.KY_ERR_INVALID_VALUE, bad
        assert lib.kyhip_lighting_plan(C.byref(p), 7, None, None) == A.KY_ERR_INVALID_VALUE, bad
        f = C.c_void_p()
        assert lib.kyhip_frame_begin(0, scene.flat, C.byref(p), C.byref(f)) == A.KY_ERR_INVALID_VALUE and not f.value, bad
        assert b"invalid render params" in lib.kyhip_last_error()


def test_film_term_limit_is_49s(A, api):
    lib = A.load_kyhip()
    for spp, depth, n_lights in ((16, 5, 5), (256, 10, 16), (1, 1, 1)):
        p49 = api.make_params(64, 64, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS, max_path_depth=depth)
        for strategy in (A.DIRECT_SINGLE_POWER, A.DIRECT_SINGLE_SPATIAL):
            p = api.make_params(64, 64, spp, direct_sample=strategy, max_path_depth=depth)
            for engine in (0, 1):
                for deferred in (0, 1):
                    l49, l = C.c_float(0), C.c_float(0)
                    n49 = lib.kyhip_film_term_limit(C.byref(p49), n_lights, engine, deferred, C.byref(l49))
                    assert lib.kyhip_film_term_limit(C.byref(p), n_lights, engine, deferred, C.byref(l)) == n49 > 0 and l.value == l49.value


def twelve_lamps_scene(A, api):
    """Twelve sphere lamps, each carried by four surfaces of OTHER shapes (two small spheres, two rectangles): 12 + 48 proxies before the cap of 32"""
    cam = A.Camera.from_buffer_copy(api.cornell_box_scene(A.CB_DEFAULT_SCENE, 48, 40).c.camera)
    shapes = [make_shape(A, A.SHAPE_RECTANGLE, [(-2, -2, -1), (2, -2, -1), (2, 2, -1), (-2, 2, -1)])]
    materials = [make_material(A, A.MATERIAL_MATTE, (0.7, 0.7, 0.7)), make_material(A, A.MATERIAL_MATTE, (0, 0, 0))]
    surfaces, lights = [A.Surface(0, 0, -1)], []
    for i in range(12):
        x, y = -1.5 + 1.0 * (i % 4), -1.0 + 1.0 * (i // 4)
        shapes.append(make_shape(A, A.SHAPE_SPHERE, [(x, y, 0.5)], radius=0.05 + 0.005 * i))
        lights.append(make_light(A, A.LIGHT_AREA, (3.0 + i, 2.0, 1.0 + 0.5 * i), shape=len(shapes) - 1))
        for k in range(4):
            if k < 2:
                shapes.append(make_shape(A, A.SHAPE_SPHERE, [(x + 0.2 * k, y + 0.1, 0.2 + 0.1 * k)], radius=0.04))
            else:
                z, s = 0.8 + 0.01 * i + 0.05 * k, 0.06
                shapes.append(make_shape(A, A.SHAPE_RECTANGLE, [(x - s, y - s, z), (x - s, y + s, z), (x + s, y + s, z), (x + s, y - s, z)]))
            surfaces.append(A.Surface(len(shapes) - 1, 1, i))
    return CustomScene(A, cam, shapes, materials, lights, surfaces)


def _check_tables(A, api, scene):
    power, prox = api.scene_light_pick(scene)
    r_prox, first, r_power = R.host_tables(A, api, scene)
    assert prox.shape == r_prox.shape, (prox.shape, r_prox.shape)
    assert np.array_equal(prox[:, :2], r_prox[:, :2])                                          # light and kind
    assert np.allclose(prox[:, 2:], r_prox[:, 2:], rtol=2e-6, atol=1e-7), np.abs(prox - r_prox).max()
    assert np.allclose(power, r_power, rtol=2e-6, atol=0), (power, r_power)
    lights = prox[:, 0].astype(int)
    assert (np.diff(lights) >= 0).all()                                                        # a light's proxies are contiguous, in the lights' order
    nl = R.scene_view(api, scene).light_count
    assert abs(float(power[:nl].astype(np.float64).sum()) - 1.0) < 1e-6 and (power[nl:] == 0).all()
    assert (power[:nl] >= np.float32(R.SHARE / nl) * (1 - 1e-6)).all()
    assert np.array_equal(api.scene_light_pick(scene, A.PICK_POWER)[1], prox)                   # either rule: the same tables
    return power, prox, first


def test_host_tables_veach(A, api):
    """create_mis_scene: five sphere lamps, lights 1 and 2 sampling one ball and carried by another (3498-3499 against 3525-3526): 7 proxies; the lamp of radius
    0.5 and radiance 800 holds about 95 % of the power rule's picks"""
    scene = api.mis_scene(64, 36)
    power, prox, first = _check_tables(A, api, scene)
    assert len(prox) == 7 and list(np.diff(first)) == [1, 2, 2, 1, 1]
    assert (prox[:, 1] == R.SPHERE).all()
    # (the share of the power, w / W: with the defensive share a = 1/4 the stored probability is 0.05 + 0.75 x that, at most 0.8)
    share = (float(power[0]) - R.SHARE / 5) / (1 - R.SHARE)
    assert 0.93 < share < 0.97 and abs(float(power[0]) - (0.05 + 0.75 * share)) < 1e-7, power


def test_host_tables_every_kind(A, api, O):
    scene, kinds = sixteen_lights_scene(A, api, O)
    power, prox, first = _check_tables(A, api, scene)
    assert len(prox) == 16                                                                     # every lamp is its own carrier
    want = {"rect": R.PLANAR, "sphere": R.SPHERE, "point": R.POINT, "direction": R.DIRECTION, "environment": R.ENVIRONMENT}
    assert [int(k) for k in prox[:, 1]] == [want[k] for k in kinds]
    planar = prox[prox[:, 1] == R.PLANAR]
    assert np.allclose(planar[:, 9], 0.24 * 0.24, rtol=1e-5) and np.allclose(planar[:, 5], 0.12 * np.sqrt(2), rtol=1e-5) and (planar[:, 8] == -1).all()


def test_host_tables_cap(A, api):
    """12 lights x (1 + 4 carriers) = 60 proxies: the last seven lights lose their carriers' proxies, the first five keep all four"""
    scene = twelve_lamps_scene(A, api)
    power, prox, first = _check_tables(A, api, scene)
    assert len(prox) == R.MAX_PROXIES == 32
    assert list(np.diff(first)) == [5] * 5 + [1] * 7
    assert sorted(set(prox[first[0]:first[1], 1].astype(int))) == [R.SPHERE, R.PLANAR]


def test_refused_arguments(A, api):
    lib = A.load_kyhip()
    scene = api.mis_scene(16, 16)
    out = np.zeros(16, np.float32)
    assert lib.kyhip_scene_light_pick(scene.flat, 0, out.ctypes.data_as(C.c_void_p), None, 0) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_scene_light_pick(scene.flat, 3, out.ctypes.data_as(C.c_void_p), None, 0) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_scene_light_pick(scene.flat, 2, None, None, 4) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_scene_light_pick(scene.flat, 2, None, None, 0) == 7                        # the count alone


def _rows(rng, n, surfaces, box):
    rows = np.zeros((n, 16), np.float32)
    rows[:, 0:3] = rng.uniform(-box, box, (n, 3))
    for k in (3, 6):
        v = rng.normal(size=(n, 3))
        rows[:, k:k + 3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    rows[:, 9] = rng.integers(0, surfaces, n)
    rows[:, 10:16] = rng.uniform(0, 1, (n, 6))
    return rows


@pytest.mark.parametrize("which", ["veach", "sixteen_lights"])
def test_restatement_properties(which, A, api, O, rng):
    """p sums to 1, every p >= a / n, the picked light's p is the table's, and the one-pass selection picks each light as often as its p says"""
    scene = api.mis_scene(64, 36) if which == "veach" else sixteen_lights_scene(A, api, O)[0]
    s = R.scene_view(api, scene)
    nl = s.light_count
    rows = _rows(rng, 20000, s.surface_count, 6.0 if which == "veach" else 1.2)
    w = R.spatial_weights(A, api, scene, rows)
    p = R.spatial_p(w)
    assert np.isfinite(p).all() and np.abs(p.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-6
    assert (p >= np.float32(R.SHARE / nl) * (1 - 1e-6)).all()
    li, p_li, margin = R.select_spatial(rows[:, 15], w)
    assert np.abs(p_li - p[np.arange(len(rows)), li]).max() < 1e-6
    # frequencies against the mean of p: binomial, five standard deviations
    freq, mean_p = np.bincount(li, minlength=nl) / len(rows), p.astype(np.float64).mean(axis=0)
    assert (np.abs(freq - mean_p) <= 5 * np.sqrt(mean_p * (1 - mean_p) / len(rows)) + 1e-9).all(), (freq, mean_p)
    # the power rule: the same three properties of the host's table
    power = R.host_tables(A, api, scene)[2]
    lp, pp, _ = R.select_power(rows[:, 15], power, nl)
    assert np.array_equal(pp, power[lp])
    freq = np.bincount(lp, minlength=nl) / len(rows)
    assert (np.abs(freq - power[:nl]) <= 5 * np.sqrt(power[:nl] * (1 - power[:nl]) / len(rows)) + 1e-9).all(), (freq, power)


def test_restatement_edges(A, api, rng):
    """all weights zero: the uniform pick of 49 on u itself, p = 1 / n; a vertex at a proxy's centre (the d2 clamp) and a NaN normal: finite p that sums to 1"""
    scene = api.mis_scene(64, 36)
    s = R.scene_view(api, scene)
    u = np.array([0.0, 0.1, 0.25, 0.5, 0.999, 1 - 2.0 ** -24], np.float32)
    li, p, _ = R.select_spatial(u, np.zeros((len(u), 5), np.float32))
    assert list(li) == [0, 0, 1, 2, 4, 4] and (p == np.float32(0.2)).all()
    assert (R.spatial_p(np.zeros((3, 5), np.float32)) == np.float32(0.2)).all()
    rows = _rows(rng, 64, s.surface_count, 6.0)
    prox = R.host_tables(A, api, scene)[0]
    rows[:7, 0:3] = prox[:, 2:5]                      # at each proxy's centre
    rows[7:14, 3:6] = np.nan                          # a NaN normal
    rows[14:21, 6:9] = np.nan                         # a NaN wo
    w = R.spatial_weights(A, api, scene, rows)
    p = R.spatial_p(w)
    assert np.isfinite(w).all() and np.isfinite(p).all() and np.abs(p.astype(np.float64).sum(axis=1) - 1).max() < 1e-6
    li, p_li, _ = R.select_spatial(rows[:, 15], w)
    assert ((li >= 0) & (li < 5)).all() and np.isfinite(p_li).all() and (p_li >= np.float32(0.05) * (1 - 1e-6)).all()
    one = R.select_spatial(u, np.ones((len(u), 1), np.float32))
    assert (one[0] == 0).all() and (one[1] == 1).all()


@pytest.mark.parametrize("which", ["veach", "cornell_lamp_point", "sixteen_lights", "general_shapes"])
def test_restatement_against_its_float64_version(which, A, api, O, rng):
    """On the very rows tests/test_light_pick_gpu.py sends to the device -- scene hits with their pick numbers at the edges --: the float64 version of the same
    formulas gives the sixteen p within the GPU test's P_TOL and picks the same light but for rows within P_TOL of an edge, at most EDGE_SHARE of them.  So the
    exemption the GPU test grants is one the restatement's own rounding needs, and no wider."""
    from test_light_pick_gpu import EDGE_SHARE, P_TOL, pick_rows
    scene, _, rows = pick_rows(which, 2, A, api, O, rng)
    w32, w64 = R.spatial_weights(A, api, scene, rows), R.spatial_weights(A, api, scene, rows, np.float64)
    li, _, margin = R.select_spatial(rows[:, 15], w32)
    li64, _, _ = R.select_spatial(rows[:, 15], w64, np.float64)
    d = np.abs(R.spatial_p(w32).astype(np.float64) - R.spatial_p(w64, np.float64)).max()
    differ = li64 != li
    print("%s: largest |p32 - p64| %.2e; %d of %d rows pick another light in float64, %d of them beyond %g of an edge"
          % (which, d, int(differ.sum()), len(rows), int((differ & (margin > P_TOL)).sum()), P_TOL))
    assert len(rows) > 2000 and d <= P_TOL
    assert differ.mean() <= EDGE_SHARE and not (differ & (margin > P_TOL)).any()


_REPLAY = {}


def _veach_replay(A, api, O):
    """the oracle's vertices of the Veach stat case at STAT_SPP with every light's term at each: made once, left unchanged"""
    if "veach" not in _REPLAY:
        scene, W, H, pixels = stat_case("veach", A, api)
        _REPLAY["veach"] = (Replay(A, api, O, scene, W, H, pixels, STAT_SPP), scene, W, H, pixels)
    return _REPLAY["veach"]


def test_statistic_catches_a_forgotten_pick_probability(A, api, O):
    """With the oracle alone (tests/light_pick_replay.py): a sample whose light is picked by the spatial p and whose term is multiplied by n -- 1 / p forgotten --
    fails z_verdict on the Veach stat case at STAT_SPP against the oracle's both_mis under another seed, and the same sample over p passes.  So
    tests/test_light_pick_gpu.py's test_in_expectation_random_sampler has power against the likely bug.
    Measured (|mean z| in standard errors of the mean, share of pixels beyond 4; the bounds are 4 and 1 %): over p 0.28, 0 %; times n 145.1, 85 %."""
    rp, scene, W, H, pixels = _veach_replay(A, api, O)
    c = np.stack([luminance(O.li(scene, api.make_params(W, H, STAT_SPP, seed=4321), x, y, 0, STAT_SPP)) for (x, y) in pixels])
    fin = np.isfinite(c).all(axis=1)
    rng = np.random.default_rng(177)
    verdict = {}
    for forget in (False, True):
        z, _ = z_scores(rp.draw("spatial", R.SHARE, rng, forget_p=forget)[fin], c[fin])
        verdict[forget] = z_verdict(z)
        print("spatial pick, %s: %d pixels vary, |mean z| = %.2f standard errors, %.2f %% beyond 4" % ("times n" if forget else "over p", len(z), verdict[forget][1], 100 * verdict[forget][2]))
        assert len(z) >= 256
    assert verdict[False][0], verdict[False]
    assert not verdict[True][0] and verdict[True][1] > 2 * 4.0, verdict[True]


def test_replay_profile_is_the_tools_output(A, api, O):
    """profiles/light_pick_replay.txt's RATIO lines for Veach, which the GPU test's variance bound reads, are what the replay gives today"""
    import os
    rp = _veach_replay(A, api, O)[0]
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "light_pick_replay.txt")
    lines = [l.split() for l in open(path) if l.startswith("RATIO veach ")]
    assert len(lines) == 6
    for _, _, rule, a, value in lines:
        assert abs(rp.ratio(rule, float(a)) - float(value)) <= 2e-4 * max(1.0, float(value)), (rule, a, value, rp.ratio(rule, float(a)))
