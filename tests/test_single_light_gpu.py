"""sample_single_light (direct_sample 49, ky.cpp:3813-3832) on the GPU against the unchanged oracle, which has no strategy 49: everything is
expressed through its both_mis (48).
 - function level: kyhip_kat_single_light = n_lights x kyo_kat_nee(48, index) with the index from pick_u in numpy fp32, tolerances and the
   disagreement rule of tests/test_kat_nee_gpu.py, relative to the n-fold values;
 - whole path under the debug sampler on one-light scenes: 49 = the oracle's 48 (every number is 0.5: the extra draw cannot matter), the
   rule of tests/test_parity_gpu.py's debug-sampler frames;
 - whole path under the debug sampler on one delta light listed three / four times (the per-lane form with n > 1 and delta lights): 49 = the oracle's 48;
   tests/test_single_light_controls.py shows with the oracle alone that these scenes can fail;
 - whole path in expectation under the random sampler: a per-pixel z-score of luminance means, kyhip_kat_li at 49 against kyo_li at 48;
 - invariants: render = mean of kat_li, tile sizes, shard counts and a repeated device bit-identical, deferred shadow rays on and off, run-time
   instantiations against the table's kernels, the trace row's light bits, the kernel's name, a refused launch."""
import ctypes as C

import numpy as np
import pytest

from single_light_scenes import STAT_SPP, luminance, repeated_delta_scene, sixteen_lights_scene, stat_case, z_scores, z_verdict
from test_kat_nee_gpu import _compare, _vertices

pytestmark = pytest.mark.gpu


def _pick_us(n_lights):
    """0, the fp32 neighbours on both sides of every k / n, 1 - 2^-24"""
    us = [np.float32(0.0), np.float32(1.0) - np.float32(2.0 ** -24)]
    for k in range(1, n_lights):
        e = np.float32(k) / np.float32(n_lights)
        us += [e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1))]
    return np.array(us, np.float32)


def _index(u, n):
    return np.minimum((u.astype(np.float32) * np.float32(n)).astype(np.int32), n - 1)


SPHERE_LAMP = (2e-2, 0.01)     # tests/test_kat_nee_gpu.py's Veach pair (value tolerance, share of differing discrete outcomes): sphere lamps, the exponent-5000 lobe
OTHER_LIGHT = (5e-4, 0.002)    # ... and its Cornell pair; tests/test_scene_limits.py applies the two to its own rooms by the lamp's shape in the same way


def _scene(which, A, api, O=None):
    """-> scene, the box its vertices come from, per light its (value tolerance, share of differing discrete outcomes)"""
    if which == "veach":
        return api.mis_scene(64, 36), 6.0, [SPHERE_LAMP] * 5
    if which == "cornell_lamp_point":
        return api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA | A.CB_LIGHT_POINT, 64, 64), 1.2, [OTHER_LIGHT] * 2
    if which == "sixteen_lights":
        scene, kinds = sixteen_lights_scene(A, api, O)
        return scene, 1.2, [SPHERE_LAMP if k == "sphere" else OTHER_LIGHT for k in kinds]
    from test_parity_gpu import general_shapes_scene
    return general_shapes_scene(A, api), 1.2, [OTHER_LIGHT] * 3


def _light_count(scene):
    return int(scene.c.light_count) if hasattr(scene, "c") else int(scene.scene.light_count)


@pytest.mark.parametrize("which", ["veach", "cornell_lamp_point", "general_shapes", "sixteen_lights"])
def test_picked_light_term_by_term(which, A, api, O, rng):
    scene, box, classes = _scene(which, A, api, O)
    n_lights = _light_count(scene)
    assert n_lights == len(classes)
    base = _vertices(A, api, O, scene, rng, 4096, box)
    assert len(base) > 2000
    us = _pick_us(n_lights)
    rows = np.zeros((len(base), 16), np.float32)
    rows[:, :15] = base
    rows[:, 15] = rng.uniform(0, 1, len(base)).astype(np.float32)
    rows[:len(us), 15] = us                       # the edges of every light's interval
    idx = _index(rows[:, 15], n_lights)
    assert set(idx.tolist()) == set(range(n_lights))
    g = api.kat_single_light(scene, rows)
    c = np.zeros_like(g)
    for light in range(n_lights):
        m = idx == light
        c[m] = np.float32(n_lights) * O.kat_nee(scene, A.DIRECT_BOTH_MIS, light, rows[m][:, :15])
    fin = np.isfinite(c).all(axis=1) & np.isfinite(g).all(axis=1)
    assert np.isfinite(g).all() or not np.isfinite(c).all()
    total = 0
    for cls in sorted(set(classes)):               # the rows whose picked light belongs to one tolerance class together
        rows_of = fin & np.isin(idx, [l for l in range(n_lights) if classes[l] == cls])
        terms = flips = 0
        for half in (slice(0, 3), slice(3, 6)):
            t, f = _compare(g[rows_of][:, half], c[rows_of][:, half], cls[0])
            terms += t
            flips += f
        print("%s, tolerance %g: %d non-zero terms, %d differ in their discrete outcome" % (which, cls[0], terms, flips))
        assert flips <= cls[1] * max(terms, 1), (cls, flips, terms)
        total += terms
    assert total > 200, total


@pytest.mark.parametrize("flag", ["CB_LIGHT_AREA", "CB_LIGHT_POINT", "CB_LIGHT_DIRECTION", "CB_LIGHT_ENVIRONMENT"])
@pytest.mark.parametrize("integrator", [6, 9, 10, 11])
def test_one_light_scenes_debug_sampler(flag, integrator, A, api, O):
    W = H = 48
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | getattr(A, flag), W, H)
    p49 = api.make_params(W, H, 2, integrator=integrator, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_SINGLE_BOTH_MIS)
    p48 = api.make_params(W, H, 2, integrator=integrator, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_BOTH_MIS)
    g, c = api.render(scene, p49), O.render(scene, p48)
    d = np.abs(g - c).max(axis=2)
    assert c.mean() > 0.01
    assert (d > 1e-4).mean() < 2e-3, (d > 1e-4).mean()   # silhouette pixels may flip (tests/test_parity_gpu.py)
    for (x, y) in ((24, 24), (10, 30), (36, 12)):
        a, b = api.kat_li(scene, p49, x, y, 0, 2), O.li(scene, p48, x, y, 0, 2)
        assert np.allclose(a, b, atol=1e-4), (x, y, a, b)


@pytest.mark.parametrize("case", ["default_frame", "room_sphere_lamp", "room_lamp_large", "room_point_large", "room_lamp_64", "accumulator_environment"])
@pytest.mark.parametrize("integrator", [6, 11])
def test_other_one_light_scenes_debug_sampler(case, integrator, A, api, O):
    """The suite's other one-light scenes at 49 against the oracle's 48 under the debug sampler: ky's default frame (an environment light, small tables, the room
    a box), tests/test_scene_limits.py's rooms under a sphere lamp, at 64 surfaces, and with a scene-sized LDS block (65 surfaces, 33 materials: the LARGE kernels)
    under the lamp and under a point light, and tests/test_film_accumulator_gpu.py's sphere under an environment light."""
    from test_scene_limits import limits_room, W, H
    if case == "default_frame":
        scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
    elif case == "accumulator_environment":
        from helpers import CustomScene, make_light, make_material, make_shape
        cam = A.Camera.from_buffer_copy(api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H).c.camera)
        scene = CustomScene(A, cam, [make_shape(A, A.SHAPE_SPHERE, [(0.0, 0.0, 0.0)], radius=0.9)], [make_material(A, A.MATERIAL_MATTE, (0.6, 0.5, 0.4))],
                            [make_light(A, A.LIGHT_ENVIRONMENT, (0.5, 0.6, 0.7), world_radius=1.0)], [A.Surface(0, 0, -1)], environment_light=0)
    else:
        ns, nm, light = {"room_sphere_lamp": (16, 8, "sphere"), "room_lamp_large": (65, 33, "rect"), "room_point_large": (65, 33, "point"), "room_lamp_64": (64, 32, "rect")}[case]
        scene = limits_room(A, api, ns, nm, light, plastic=light != "rect")
    p49 = api.make_params(W, H, 2, integrator=integrator, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_SINGLE_BOTH_MIS)
    p48 = api.make_params(W, H, 2, integrator=integrator, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_BOTH_MIS)
    g, c = api.render(scene, p49), O.render(scene, p48)
    kernel = A.load_kyhip().kyhip_last_kernel(0)
    d = np.abs(g - c).max(axis=2)
    print("%s integrator %d: %d pixel(s) beyond 1e-4, largest %.2e, film mean %.4f [%s]" % (case, integrator, int((d > 1e-4).sum()), d.max(), c.mean(), kernel.decode()))
    assert c.mean() > 0.01 and b"strategy" in kernel
    assert ("large" in case) == (b"scene-sized LDS block" in kernel), kernel
    assert (d > 1e-4).mean() < 2e-3, (d > 1e-4).mean()   # silhouette pixels may flip (tests/test_parity_gpu.py)


@pytest.mark.parametrize("which", ["veach", "cornell_lamp_point"])
def test_tilings_shards_and_deferred_rays(which, A, api):
    lib = A.load_kyhip()
    lib.kyhip_last_kernel.restype = C.c_char_p
    scene = _scene(which, A, api)[0]
    W, H, spp = (64, 36, 32) if which == "veach" else (64, 64, 32)
    prev = lib.kyhip_set_shadow_queue(0)
    try:
        full = api.render(scene, api.make_params(W, H, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS))
        name = lib.kyhip_last_kernel(0)
        assert b"strategy 49" in name and b"sample_single_light: per-lane lights" in name and b"deferred" not in name, name
        assert np.isfinite(full).all() and full.mean() > 0.01
        other = api.render(scene, api.make_params(W, H, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS, tile_w=8, tile_h=24))
        assert np.array_equal(full, other)
        parts = np.zeros_like(full)
        for r in range(3):
            api.render(scene, api.make_params(W, H, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS, tile_first=r, tile_step=3), film=parts)
        assert np.array_equal(full, parts)
        lib.kyhip_set_shadow_queue(1)
        deferred = api.render(scene, api.make_params(W, H, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS))
        name = lib.kyhip_last_kernel(0)
        assert b"strategy 49" in name and b"deferred shadow rays" in name, name
        # the bound tests/test_random_scenes_gpu.py holds 48's two kernels to: the same picture up to the order of a pixel's sums and an ulp of fusing
        d = np.abs(deferred - full).max(axis=2)
        assert int((d > 2e-6).sum()) <= 10 and d.max() <= 0.25, (float(d.max()), int((d > 2e-6).sum()))
        e = lib.kyhip_set_engine(1)
        try:
            q = api.render(scene, api.make_params(W, H, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS))
            name = lib.kyhip_last_kernel(0)
            assert b"strategy 49" in name and b"lane engine" in name, name
            assert np.array_equal(q, deferred)
        finally:
            lib.kyhip_set_engine(e)
    finally:
        lib.kyhip_set_shadow_queue(prev)


@pytest.mark.parametrize("kind", ["point", "direction"])
@pytest.mark.parametrize("integrator", [6, 9, 10, 11])
def test_repeated_delta_lights_debug_sampler(kind, integrator, A, api, O):
    """One point light listed three times, one directional light four times: every number is 0.5, so the pick is light n / 2 and n times its estimate is the
    sum over the n identical lights -- 48's picture, through the per-lane form with n > 1 and delta lights (the BSDF half inactive, the light half's
    delta branch).  tests/test_single_light_controls.py: direct lighting is all of these pictures, and one light fewer moves over a quarter of the pixels."""
    W, H = 48, 40
    scene = repeated_delta_scene(A, api, O, kind, W, H)
    p49 = api.make_params(W, H, 2, integrator=integrator, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_SINGLE_BOTH_MIS)
    p48 = api.make_params(W, H, 2, integrator=integrator, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_BOTH_MIS)
    g, c = api.render(scene, p49), O.render(scene, p48)
    d = np.abs(g - c).max(axis=2)
    print("%s integrator %d: %d pixel(s) beyond 1e-4, largest %.2e, film mean %.4f" % (kind, integrator, int((d > 1e-4).sum()), d.max(), c.mean()))
    assert c.mean() > 0.01
    assert (d > 1e-4).mean() < 2e-3, (d > 1e-4).mean()   # silhouette pixels may flip (tests/test_parity_gpu.py)
    for (x, y) in ((24, 30), (8, 20), (40, 20), (24, 12), (14, 28), (34, 31)):   # floor, side walls, back wall, the two spheres
        a, b = api.kat_li(scene, p49, x, y, 0, 2), O.li(scene, p48, x, y, 0, 2)
        assert np.allclose(a, b, atol=1e-4), (x, y, a, b)


@pytest.mark.parametrize("which", ["veach", "cornell_lamp_point"])
def test_in_expectation_random_sampler(which, A, api, O):
    """kyhip_kat_li at 49 against kyo_li at 48 (another seed: independent samples), STAT_SPP samples on each pixel of a fixed interleaved set: the per-pixel
    z-score of the luminance means from the two sample variances.  Bounds from the normal law (single_light_scenes.z_verdict): |mean z| within four standard
    errors of the mean, at most 1 % of the pixels beyond |z| = 4.  Pixels where neither side varies (the background, a lamp seen directly) must agree to 1e-4.
    Oracle alone, same pixels and samples (tests/test_single_light_controls.py): 48 against 48 under another seed gives |mean z| = 0.40 (Veach) and 1.26
    (Cornell) standard errors with no pixel beyond 4 -- passes; 48 with its direct part n-fold (the pick probability left out) gives 376 and 225 standard
    errors with 98 % and 94 % of the pixels beyond 4 -- fails.  What this checks that nothing else does: the whole path with several lights under the random
    sampler -- the order of the draws (pick, random_light, random_bsdf), the factor n on the inline and the deferred weight."""
    scene, W, H, pixels = stat_case(which, A, api)
    p49 = api.make_params(W, H, STAT_SPP, seed=4321, direct_sample=A.DIRECT_SINGLE_BOTH_MIS)
    p48 = api.make_params(W, H, STAT_SPP, seed=1234, direct_sample=A.DIRECT_BOTH_MIS)
    g = np.stack([luminance(api.kat_li(scene, p49, x, y, 0, STAT_SPP)) for (x, y) in pixels])
    c = np.stack([luminance(O.li(scene, p48, x, y, 0, STAT_SPP)) for (x, y) in pixels])
    fin = np.isfinite(g).all(axis=1) & np.isfinite(c).all(axis=1)    # (the reference's own inf * 0 at exactly-grazing mirror hits)
    assert fin.sum() >= len(pixels) - 2
    z, fixed = z_scores(g[fin], c[fin])
    ok, mean_in_se, share = z_verdict(z)
    print("%s: %d pixels vary, |mean z| = %.2f standard errors of the mean, %.2f %% of them beyond 4 (largest |z| %.2f); fixed pixels differ by %.1e"
          % (which, len(z), mean_in_se, 100 * share, np.abs(z).max(), fixed))
    assert len(z) >= 256 and fixed <= 1e-4, (len(z), fixed)
    assert ok, (mean_in_se, share)


@pytest.mark.parametrize("which", ["veach", "cornell_lamp_point", "sixteen_lights"])
def test_render_is_the_mean_of_kat_li(which, A, api, O):
    """The film's pixel is the clamped mean of the samples kyhip_kat_li returns for it: the render kernels (per-lane rows, or the run-time-dispatched kernel for
    the sixteen lights) and the replay kernel consume the same numbers in the same order.  Bounds: tests/test_parity_gpu.py's between two kernels of the
    library (2e-5; with Veach's exponent-5000 lobe no pixel beyond 1.5e-3 and at most three beyond 2e-4)."""
    scene = _scene(which, A, api, O)[0]
    W, H = (48, 40) if which == "sixteen_lights" else ((64, 36) if which == "veach" else (64, 64))
    spp = 32
    p = api.make_params(W, H, spp, direct_sample=A.DIRECT_SINGLE_BOTH_MIS)
    film = api.render(scene, p)
    pixels = [(x, y) for y in range(3, H, 9) for x in range(2, W, 11)]
    d = []
    for (x, y) in pixels:
        li = api.kat_li(scene, p, x, y, 0, spp)
        if np.isfinite(li).all():
            d.append(np.abs(np.clip(li.astype(np.float64).mean(axis=0), 0, 1) - film[y, x]).max())
    d = np.array(d)
    print("%s: %d pixels, largest |film - mean of kat_li| %.2e, %d beyond 2e-4" % (which, len(d), d.max(), int((d > 2e-4).sum())))
    assert len(d) >= len(pixels) - 1 and film.mean() > 0.01
    assert d.max() <= (1.5e-3 if which == "veach" else 2e-5) and int((d > 2e-4).sum()) <= (3 if which == "veach" else 0), (float(d.max()), int((d > 2e-4).sum()))


@pytest.mark.parametrize("which", ["veach", "cornell_lamp_point"])
def test_repeated_device_and_run_time_instantiations(which, A, api, tmp_path, monkeypatch, no_boxes):
    """A device list repeating device 0 renders the same bits; KYHIP_JIT = 1 (kyhip_set_jit(1): the launch's own instantiation of strategy 49 with all of the
    scene's facts) against the table's kernel within tests/test_jit.py's bound, and sharding stays bit-identical under it."""
    monkeypatch.setenv("KYHIP_CACHE_DIR", str(tmp_path / "cache"))
    lib = A.load_kyhip()
    lib.kyhip_last_kernel.restype = C.c_char_p
    scene = _scene(which, A, api)[0]
    W, H = (64, 36) if which == "veach" else (64, 64)
    p = api.make_params(W, H, 32, direct_sample=A.DIRECT_SINGLE_BOTH_MIS)
    prev = lib.kyhip_set_jit(0)
    try:
        table = api.render(scene, p)
        table_kernel = lib.kyhip_last_kernel(0)
        assert b"strategy 49" in table_kernel and b"run-time instantiation" not in table_kernel, table_kernel
        assert np.array_equal(api.render_multi(scene, p, [0, 0, 0]), table)
        assert np.array_equal(api.render_multi(scene, p, [0, 0]), table)
        lib.kyhip_set_jit(1)
        own = api.render(scene, p)
        own_kernel = lib.kyhip_last_kernel(0)
        assert b"run-time instantiation" in own_kernel and b", 49, " in own_kernel and b"sample_single_light" in own_kernel, (own_kernel, lib.kyhip_jit_status())
        d = float(np.abs(own - table).max())
        print("%s: %s | max |difference| to the table's kernel %.2e" % (which, own_kernel.decode(), d))
        assert d < 2e-5 and table.max() > 0.1, (own_kernel, d)
        parts = np.zeros_like(own)
        for r in range(3):
            api.render(scene, api.make_params(W, H, 32, direct_sample=A.DIRECT_SINGLE_BOTH_MIS, tile_first=r, tile_step=3), film=parts)
        assert np.array_equal(parts, own)
        assert np.array_equal(api.render_multi(scene, p, [0, 0, 0]), own)
    finally:
        lib.kyhip_set_jit(prev)


@pytest.mark.parametrize("which", ["veach", "sixteen_lights"])
def test_trace_rows_carry_the_picked_light_only(which, A, api, O):
    """kyhip_kat_li_trace at 49: a vertex's light bits (row[24]: the BSDF halves, row[25]: the light halves, bit = light index) name at most ONE light, the
    same in both words; over the samples every light's bit shows up -- bit 15 of both words with sixteen lights -- and the traced radiance is kat_li's to 2e-4."""
    scene = _scene(which, A, api, O)[0]
    n = _light_count(scene)
    W, H = (64, 36) if which == "veach" else (48, 40)
    p = api.make_params(W, H, 64, direct_sample=A.DIRECT_SINGLE_BOTH_MIS)
    seen_b = seen_l = 0
    for (x, y) in ((W // 2, H - 8), (W // 3, H // 2), (2 * W // 3, H - 5)):
        li = api.kat_li(scene, p, x, y, 0, 64)
        for s in range(64):
            rows, li_s = api.kat_li_trace(scene, p, x, y, s)
            # (the trace keeps a vertex's two halves apart and adds their sum: an ulp per vertex; helpers.explain_sample's value tolerance)
            assert np.allclose(li_s, li[s], rtol=2e-4, atol=1e-6) or not np.isfinite(li[s]).all(), (x, y, s, li_s, li[s])
            for r in rows:
                b, l = int(r[24]), int(r[25])
                assert b < (1 << n) and l < (1 << n) and bin(b | l).count("1") <= 1, (x, y, s, b, l)
                seen_b |= b
                seen_l |= l
    print("%s: BSDF-half bits seen %s, light-half bits seen %s" % (which, bin(seen_b), bin(seen_l)))
    assert seen_l == (1 << n) - 1, bin(seen_l)            # every light was picked and lit something
    assert seen_b != 0 and (which != "sixteen_lights" or (seen_l >> 15) & 1)


def test_refused_launch_leaves_the_film_alone(A, api):
    scene = api.mis_scene(64, 36)
    film = np.full((36, 64, 3), 0.25, np.float32)
    for bad in (1, 50, 2 | 48):
        with pytest.raises(Exception):
            api.render(scene, api.make_params(64, 36, 4, direct_sample=bad), film=film)
        assert (film == 0.25).all()
