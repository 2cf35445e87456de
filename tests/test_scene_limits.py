"""The render kernels at the scene sizes where their form changes.

  <= 16 surfaces and <= 8 materials   KY_FEAT_SMALL_TABLES: the 16 / 8-entry static LDS block (every box row and every sphere-light row needs it)
  <= 64 surfaces and <= 32 materials  the 64 / 32-entry static block; beyond it the LARGE rows with a scene-sized dynamic block, and the queue
                                      engine hands the launch to the lane engine
  <= 64 surfaces                      estimate_by_bsdf's carrier query runs lane-per-surface (lane j tests surface j); beyond, trace_any over DScene::occ
  <= 4 carriers per area light        the carrier list and the fast path (KY_FEAT_CARRIERS); with 5, n_carriers = -1 and the slow path
  64 materials, 16 lights, 256 shapes the ABI's maxima: one more is refused with KY_ERR_LIMIT

One scene builder (limits_room) serves every case: an open room, a lamp, a large opaque HIDER sphere in a corner and a BLOCKER sphere that casts the
lamp's main shadow on the floor.  Padding surfaces are small spheres strictly inside the hider -- no ray reaches them, so they change the surface count
and not the image -- and padding materials are appended unused.  What decides the picture sits in the LAST row of each table: the blocker is the last
input sphere and so the last packed surface (planar surfaces, then spheres, then general shapes: pack_scene), the back wall and the blocker wear the last
material, the lamp is the last light.  A kernel that stages, masks or scans one row too few changes the film by far more than its tolerance; the
oracle-only checks below prove that for each sentinel."""
import ctypes as C
import re

import numpy as np
import pytest

from helpers import CustomScene, make_light, make_material, make_shape, rmse, rmse_with_explained_flips

W, H, SPP = 48, 40, 256
SIZES = [(16, 8), (17, 8), (16, 9), (33, 9), (64, 32), (65, 32), (64, 33), (20, 64)]   # (surfaces, materials) on both sides of each threshold
FEAT_CARRIERS, FEAT_SMALL, FEAT_OWN, FEAT_SPHERE_LIGHTS, FEAT_BOXES = 4, 128, 256, 32, 512
LARGE_BLOCK = "scene-sized LDS block"
QUEUE_ENGINE = "render_kernel_q (queue engine)"

ROOM_A, ROOM_B, ROOM_H = 1.3, 1.3, 1.28                 # test_random_scenes_gpu.random_room's room, axis-aligned
HIDER_C, HIDER_R = (-0.85, -0.85, -0.86), 0.4           # in the back left corner, 2 cm above the floor
PAD_R, PAD_REACH = 0.03, 0.3                            # padding: |offset| <= 0.3 from the hider's centre, radius 0.03 -> at least 0.07 inside it
BLOCKER_C, BLOCKER_R = (0.1, 0.45, -0.72), 0.55         # under and in front of the lamp: its shadow is the front of the floor
LAMP_C, LAMP_S = (0.0, -0.1), 0.25                      # the rectangle lamp's centre and half size, 2 cm under the ceiling
SIDE_PANELS = ((-0.8, -0.8), (0.8, -0.8), (-0.8, 0.7), (0.8, 0.7))   # further carriers of the lamp's light (half size 0.1)


def film_tolerance(spp):
    from test_parity_gpu import film_tolerance as tol
    return tol(spp)


def _rect(A, cx, cy, s, z):
    """a square in the plane z that faces down (random_room's lamps)"""
    return make_shape(A, A.SHAPE_RECTANGLE, [(cx - s, cy - s, z), (cx - s, cy + s, z), (cx + s, cy + s, z), (cx + s, cy - s, z)])


def _materials(A, n_materials, plastic, delta_padding):
    """0 white, 1 red, 2 green, 3 the emitters' black, 4 the hider's grey; then the unused padding; the LAST is the sentinel (back wall, blocker)"""
    mats = [make_material(A, A.MATERIAL_MATTE, (0.75, 0.75, 0.75)), make_material(A, A.MATERIAL_MATTE, (0.63, 0.065, 0.05)),
            make_material(A, A.MATERIAL_MATTE, (0.14, 0.45, 0.091)), make_material(A, A.MATERIAL_MATTE, (0, 0, 0)),
            make_material(A, A.MATERIAL_MATTE, (0.5, 0.5, 0.5))]
    kinds = (A.MATERIAL_MATTE, A.MATERIAL_PLASTIC, A.MATERIAL_MIRROR, A.MATERIAL_GLASS) if delta_padding else (A.MATERIAL_MATTE, A.MATERIAL_PLASTIC)
    for k in range(n_materials - 6):
        c = (0.9 - 0.013 * k, 0.55 - 0.008 * k, 0.1 + 0.012 * k)          # warm colours: far from the sentinel's blue, distinct from each other
        kind = kinds[k % len(kinds)]
        if kind == A.MATERIAL_PLASTIC:
            mats.append(make_material(A, kind, tuple(0.6 * x for x in c), (0.3, 0.3, 0.3), exponent=float(10 + k)))
        elif kind == A.MATERIAL_GLASS:
            mats.append(make_material(A, kind, (1, 1, 1), c, eta=1.4 + 0.005 * k))
        else:
            mats.append(make_material(A, kind, c))
    if plastic:
        mats.append(make_material(A, A.MATERIAL_PLASTIC, (0.08, 0.2, 0.6), (0.35, 0.35, 0.35), exponent=12.0))
    else:
        mats.append(make_material(A, A.MATERIAL_MATTE, (0.15, 0.4, 0.95)))
    assert len(mats) == n_materials
    return mats


def limits_room(A, api, n_surfaces, n_materials, light="rect", plastic=False, two_lights=False, carriers=1, sampled_is_carrier=True,
                shared_sphere=False, width=W, height=H):
    """The room with exactly n_surfaces surfaces and n_materials materials.
    light: "rect" (a rectangle lamp under the ceiling: Cornell's rows when it is its own and only carrier), "point" or "sphere" (a sphere lamp).
    two_lights: a dim point light first, the lamp last.  carriers: surfaces whose area_light is the rectangle lamp's light (panels under the ceiling; 0: the
    sampled rectangle is no surface); sampled_is_carrier False: the light samples a copy of the first panel that no surface uses.
    shared_sphere: light "sphere" whose light is carried by a second sphere as well (a sphere lamp of two bulbs)."""
    cam = A.Camera.from_buffer_copy(api.cornell_box_scene(A.CB_DEFAULT_SCENE, width, height).c.camera)
    a, b, h = ROOM_A, ROOM_B, ROOM_H
    R = lambda pts: make_shape(A, A.SHAPE_RECTANGLE, pts)
    S = lambda c, r: make_shape(A, A.SHAPE_SPHERE, [c], radius=r)
    last = n_materials - 1
    shapes = [R([(-a, -b, -h), (a, -b, -h), (a, b, -h), (-a, b, -h)]),       # floor
              R([(-a, -b, -h), (-a, -b, h), (a, -b, h), (a, -b, -h)]),       # back wall: the sentinel material
              R([(-a, -b, h), (-a, -b, -h), (-a, b, -h), (-a, b, h)]),       # left
              R([(a, -b, -h), (a, -b, h), (a, b, h), (a, b, -h)]),           # right
              R([(a, -b, h), (-a, -b, h), (-a, b, h), (a, b, h)])]           # ceiling
    surfaces = [A.Surface(0, 0, -1), A.Surface(1, last, -1), A.Surface(2, 1, -1), A.Surface(3, 2, -1), A.Surface(4, 0, -1)]
    lights = []
    if two_lights:
        lights.append(make_light(A, A.LIGHT_POINT, (4.0, 3.5, 3.0), position=(0.7, 0.5, 0.4)))
    lamp = len(lights)
    extra_shape = None
    if light == "rect":
        z = h - 0.02
        panels = [_rect(A, LAMP_C[0], LAMP_C[1], LAMP_S, z)] + [_rect(A, x, y, 0.1, z) for (x, y) in SIDE_PANELS]
        assert carriers <= len(panels)
        for k in range(carriers):
            shapes.append(panels[k])
            surfaces.append(A.Surface(len(shapes) - 1, 3, lamp))
        if carriers == 0 or not sampled_is_carrier:
            extra_shape = panels[0]                                       # the sampled rectangle, appended after the surfaces' shapes
        lights.append(make_light(A, A.LIGHT_AREA, (150.0, 130.0, 100.0), shape=5 if carriers and sampled_is_carrier else -2))
    elif light == "point":
        lights.append(make_light(A, A.LIGHT_POINT, (9.0, 8.0, 6.5), position=(LAMP_C[0], LAMP_C[1], 0.9)))
    else:
        assert light == "sphere"
    spheres = [(HIDER_C, HIDER_R, 4, -1)]
    rng = np.random.default_rng(5)
    n_fixed = len(surfaces) + 2 + (1 if light == "sphere" else 0) + (1 if shared_sphere else 0)
    n_pad = n_surfaces - n_fixed
    assert n_pad >= 0, (n_surfaces, n_fixed)
    for _ in range(n_pad):
        d = rng.normal(size=3)
        d *= rng.uniform(0.0, PAD_REACH) / np.linalg.norm(d)
        spheres.append((tuple(np.array(HIDER_C) + d), PAD_R, 4, -1))
    if light == "sphere":
        spheres.append(((LAMP_C[0], LAMP_C[1], 0.85), 0.15, 3, lamp))
        if shared_sphere:
            spheres.append(((0.75, 0.6, 0.9), 0.1, 3, lamp))              # a second bulb of the same light (the light samples the first)
        lights.append(make_light(A, A.LIGHT_AREA, (200.0, 180.0, 150.0), shape=-3))
    spheres.append((BLOCKER_C, BLOCKER_R, last, -1))                     # the sentinel: the last sphere, the last packed surface
    sphere_shape = {}
    for k, (c, r, m, li) in enumerate(spheres):
        shapes.append(S(c, r))
        surfaces.append(A.Surface(len(shapes) - 1, m, li))
        sphere_shape[k] = len(shapes) - 1
    if light == "sphere":
        lights[lamp].shape = sphere_shape[len(spheres) - 2 - (1 if shared_sphere else 0)]
    if extra_shape is not None:
        shapes.append(extra_shape)
        lights[lamp].shape = len(shapes) - 1
    assert len(surfaces) == n_surfaces
    return CustomScene(A, cam, shapes, _materials(A, n_materials, plastic, light != "sphere"), lights, surfaces)


def _feat(kernel):
    m = re.search(r"feat (\d+)", kernel)
    return int(m.group(1)) if m else None


def _is_small(ns, nm):
    return ns <= 16 and nm <= 8


def _is_large(ns, nm):
    return ns > 64 or nm > 32


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: scene facts, ABI limits, and that every sentinel decides the picture (oracle only)
# ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("light", ["rect", "point", "sphere"])
def test_small_tables_fact_at_its_threshold(light, A, api):
    for ns, nm in [(9, 6)] + SIZES:
        facts = api.scene_facts(limits_room(A, api, ns, nm, light))
        assert bool(facts & FEAT_SMALL) == _is_small(ns, nm), (light, ns, nm, facts)
        if light == "rect":      # one rectangle lamp that is its own carrier: the facts of the Cornell rows at every size
            assert facts & (1 | 2 | FEAT_CARRIERS | FEAT_OWN) == 1 + 2 + FEAT_CARRIERS + FEAT_OWN, (ns, nm, facts)
        if light == "sphere":    # padding materials are matte / plastic there: the sphere-light facts hold at every size
            assert facts & (FEAT_SPHERE_LIGHTS | FEAT_CARRIERS | 64) == FEAT_SPHERE_LIGHTS | FEAT_CARRIERS | 64, (ns, nm, facts)


def test_carrier_facts(A, api):
    """KY_FEAT_CARRIERS holds with 0 to KY_MAX_CARRIERS = 4 carriers on one light and is gone with 5; KY_FEAT_OWN_CARRIER holds only with exactly one
    carrier that is the sampled shape itself."""
    for n in (0, 1, 2, 3, 4, 5):
        facts = api.scene_facts(limits_room(A, api, 12, 8, "rect", carriers=n))
        assert bool(facts & FEAT_CARRIERS) == (n <= 4), (n, facts)
        assert bool(facts & FEAT_OWN) == (n == 1), (n, facts)
    facts = api.scene_facts(limits_room(A, api, 12, 8, "rect", carriers=1, sampled_is_carrier=False))
    assert facts & FEAT_CARRIERS and not facts & FEAT_OWN, facts
    facts = api.scene_facts(limits_room(A, api, 12, 8, "rect", carriers=2, sampled_is_carrier=False))
    assert facts & FEAT_CARRIERS and not facts & FEAT_OWN, facts
    facts = api.scene_facts(limits_room(A, api, 12, 8, "sphere", shared_sphere=True))
    assert facts & (FEAT_SPHERE_LIGHTS | FEAT_CARRIERS) == FEAT_SPHERE_LIGHTS | FEAT_CARRIERS and not facts & FEAT_OWN, facts


def _with_extra(A, scene, shapes=0, materials=0, lights=0):
    """a copy of a CustomScene with unused shapes / materials / point lights appended"""
    c = scene.scene
    sh = [A.Shape.from_buffer_copy(c.shapes[i]) for i in range(c.shape_count)]
    ma = [A.Material.from_buffer_copy(c.materials[i]) for i in range(c.material_count)]
    li = [A.Light.from_buffer_copy(c.lights[i]) for i in range(c.light_count)]
    su = [A.Surface.from_buffer_copy(c.surfaces[i]) for i in range(c.surface_count)]
    sh += [make_shape(A, A.SHAPE_SPHERE, [(0.0, 0.0, 5.0 + 0.01 * k)], radius=0.01) for k in range(shapes)]
    ma += [make_material(A, A.MATERIAL_MATTE, (0.01 * (k % 90), 0.2, 0.3)) for k in range(materials)]
    li += [make_light(A, A.LIGHT_POINT, (0.0, 0.0, 0.0), position=(0.0, 3.0, 0.5)) for k in range(lights)]
    return CustomScene(A, A.Camera.from_buffer_copy(c.camera), sh, ma, li, su)


def test_abi_maxima_accepted_one_more_refused(A, api):
    """64 materials, 16 lights, 256 shapes, 256 surfaces are packed; one more of any is refused with KY_ERR_LIMIT (never truncated to the maximum)."""
    lib = A.load_kyhip()
    base = limits_room(A, api, 12, 8, "rect")
    n_shapes, n_lights = base.scene.shape_count, base.scene.light_count
    for kw in (dict(materials=A.MAX_MATERIALS - 8), dict(lights=A.MAX_LIGHTS - n_lights), dict(shapes=A.MAX_SHAPES - n_shapes)):
        at = _with_extra(A, base, **kw)
        assert lib.kyhip_scene_facts(at.flat) >= 0, (kw, lib.kyhip_last_error())
        over = _with_extra(A, base, **{k: v + 1 for k, v in kw.items()})
        assert lib.kyhip_scene_facts(over.flat) == A.KY_ERR_LIMIT, kw
        assert b"exceeds device limits" in lib.kyhip_last_error()
    assert lib.kyhip_scene_facts(limits_room(A, api, A.MAX_SURFACES, 8, "point").flat) >= 0
    assert lib.kyhip_scene_facts(limits_room(A, api, A.MAX_SURFACES + 1, 8, "point").flat) == A.KY_ERR_LIMIT


def test_padding_changes_nothing_for_the_oracle(A, api, O):
    """The padding spheres lie strictly inside the hider, and the padding materials are unused: the oracle's film is the same to the bit with and without
    them -- which is what makes every pair of the GPU tests below a comparison of two kernel forms on ONE picture."""
    p = api.make_params(W, H, 64, tile_w=16, tile_h=8)
    for light in ("rect", "point"):
        bare, padded = limits_room(A, api, 8 if light == "rect" else 7, 6, light), limits_room(A, api, 65, 33, light)
        a, b = O.render(bare, p), O.render(padded, p)
        assert a.mean() > 0.02 and np.array_equal(a, b), (light, np.abs(a - b).max())


def test_every_sentinel_decides_the_picture(A, api, O):
    """Reading row N - 2 instead of N - 1, dropping the last lane or truncating a table: the oracle alone shows that each changes the film by at least
    20 x film_tolerance(SPP) -- so the GPU tests' tolerances cannot absorb such a defect."""
    p = api.make_params(W, H, SPP, tile_w=16, tile_h=8)
    floor = 20 * film_tolerance(SPP)
    for ns, nm, light, two in ((16, 8, "rect", False), (64, 32, "point", False), (65, 33, "rect", True)):
        scene = limits_room(A, api, ns, nm, light, plastic=light == "point", two_lights=two)
        ref = O.render(scene, p)
        # the surface table one row short: the blocker (the last packed surface) is gone
        scene.scene.surface_count = ns - 1
        moved = rmse(O.render(scene, p), ref)
        scene.scene.surface_count = ns
        assert moved > floor, ("surfaces", ns, nm, light, moved)
        # the back wall and the blocker read material N - 2
        sentinel = [i for i in range(ns) if scene.surfaces[i].material == nm - 1]
        assert sentinel == [1, ns - 1]
        for i in sentinel:
            scene.surfaces[i].material = nm - 2
        moved = rmse(O.render(scene, p), ref)
        assert moved > floor, ("materials", ns, nm, light, moved)
        for i in sentinel:
            scene.surfaces[i].material = nm - 1
        assert np.array_equal(O.render(scene, p), ref)
        if two:   # the lamp (the last light) with the colour of light N - 2
            keep = tuple(scene.lights[1].color)
            for j in range(3):
                scene.lights[1].color[j] = scene.lights[0].color[j]
            moved = rmse(O.render(scene, p), ref)
            for j in range(3):
                scene.lights[1].color[j] = keep[j]
            assert moved > floor, ("lights", ns, nm, light, moved)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU: which kernel form ran, the film against the oracle, and the same picture across each threshold
# ---------------------------------------------------------------------------------------------------------------------------------------------

_oracle_films = {}


def _oracle(O, key, scene, p):
    """The oracle's film of a room, by its content: padding does not change it (test_padding_changes_nothing_for_the_oracle), so all sizes share one."""
    key = key + (p.samples_per_pixel, p.direct_sample, p.max_path_depth)
    if key not in _oracle_films:
        _oracle_films[key] = O.render(scene, p)
    return _oracle_films[key]


def _parity(api, O, scene, p, g, c, what):
    """RMSE of the GPU film against the oracle's; pixels set aside only as rmse_with_explained_flips does (each differing sample explained)."""
    fin = np.isfinite(c).all(axis=2)
    assert np.isfinite(g).all() and g.min() >= 0 and g.max() <= 1 and fin.mean() > 0.995, what
    e = rmse(g[fin], c[fin])
    if e >= film_tolerance(p.samples_per_pixel):
        e_without, e_with, n = rmse_with_explained_flips(api, O, scene, p, g, c, max_exempt=8, threshold=5e-3)
        print("  %s: film RMSE %.2e with, %.2e without %d explained pixel(s)" % (what, e_with, e_without, n))
        e = e_without
    assert c[fin].mean() > 0.02 and e < film_tolerance(p.samples_per_pixel), (what, e)
    return e


class _Switches:
    """kyhip_set_engine / kyhip_set_shadow_queue for the length of a test, restored afterwards"""

    def __init__(self, lib):
        self.lib = lib
        self.prev = (lib.kyhip_set_engine(0), lib.kyhip_set_shadow_queue(-1))

    def render(self, api, scene, p, engine=0, shadow_queue=-1):
        self.lib.kyhip_set_engine(engine)
        self.lib.kyhip_set_shadow_queue(shadow_queue)
        g = api.render(scene, p)
        return g, self.lib.kyhip_last_kernel(0).decode()

    def close(self):
        self.lib.kyhip_set_engine(self.prev[0])
        self.lib.kyhip_set_shadow_queue(self.prev[1])


@pytest.fixture
def switches(A):
    s = _Switches(A.load_kyhip())
    yield s
    s.close()


def _assert_rows(kernel, ns, nm, small_row_expected, table_kernels):
    """(a): the LDS block the lane engine's kernel stages for this scene size"""
    assert (LARGE_BLOCK in kernel) == _is_large(ns, nm), (ns, nm, kernel)
    if table_kernels and not _is_large(ns, nm):
        feat = _feat(kernel)
        # the 16 / 8 block only where the scene fits it; where a row with it exists for this light (the lamp's and the sphere lamps'), it is taken
        assert not (feat & FEAT_SMALL) or _is_small(ns, nm), (ns, nm, kernel)
        assert not small_row_expected or bool(feat & FEAT_SMALL) == _is_small(ns, nm), (ns, nm, kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("light", ["rect", "point"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_kernel_form_and_oracle_at_size(size, light, A, api, O, switches, table_kernels):
    """Both engines at every size around the thresholds: the kernel that ran (lane engine: the small / static / scene-sized block; queue engine: itself
    exactly when the scene is not large, the lane engine's LARGE row otherwise) and its film against the oracle."""
    ns, nm = size
    plastic = light == "point"
    scene = limits_room(A, api, ns, nm, light, plastic=plastic)
    p = api.make_params(W, H, SPP, tile_w=16, tile_h=8)
    c = _oracle(O, (light, plastic), scene, p)
    g, k = switches.render(api, scene, p, engine=0)
    _assert_rows(k, ns, nm, light == "rect", table_kernels)
    if table_kernels and light == "rect" and not _is_large(ns, nm):
        assert "strategy 48" in k and _feat(k) & (1 | 2 | 4 | FEAT_OWN) == 1 + 2 + 4 + FEAT_OWN, k     # a Cornell-lamp row at every static size
        assert bool(_feat(k) & FEAT_BOXES) == _is_small(ns, nm), k      # the room's walls are a box's faces, but every box row needs the small tables
    e = _parity(api, O, scene, p, g, c, "%s %s lane" % (light, size))
    gq, kq = switches.render(api, scene, p, engine=1)
    assert (QUEUE_ENGINE in kq) == (not _is_large(ns, nm)) and (LARGE_BLOCK in kq) == _is_large(ns, nm), (size, kq)
    eq = _parity(api, O, scene, p, gq, c, "%s %s queue" % (light, size))
    print("%s %s: lane %s RMSE %.2e | queue engine -> %s RMSE %.2e" % (light, size, k, e, kq, eq))


@pytest.mark.gpu
def test_lamp_strategies_with_lane_63_the_blocker(A, api, O, switches, table_kernels):
    """64 surfaces, 32 materials: lane 63 of the lane-per-surface carrier query holds the blocker, material row 31 its colour; all six strategies."""
    scene = limits_room(A, api, 64, 32, "rect")
    for strategy in (A.DIRECT_BOTH_MIS, A.DIRECT_LIGHT_MIS, A.DIRECT_BSDF_MIS, A.DIRECT_LIGHT, A.DIRECT_BSDF, A.DIRECT_IDLE):
        p = api.make_params(W, H, SPP, direct_sample=strategy, tile_w=16, tile_h=8)
        c = _oracle(O, ("rect", False), scene, p)
        g, k = switches.render(api, scene, p)
        _assert_rows(k, 64, 32, False, table_kernels)
        if strategy == A.DIRECT_IDLE:   # emission only: the lamp itself, every path that finds it (no direct lighting)
            assert rmse(g, c) < film_tolerance(SPP), rmse(g, c)
            e = rmse(g, c)
        else:
            e = _parity(api, O, scene, p, g, c, "strategy %d" % strategy)
        print("rect (64, 32) strategy %d: %s RMSE %.2e" % (strategy, k, e))


# the pairs across each threshold: one padding surface or one unused material more, so that the oracle's picture is the same
PAIRS = [((16, 8), (17, 8)), ((16, 8), (16, 9)), ((64, 32), (65, 32)), ((64, 32), (64, 33)), ((33, 9), (20, 64))]


@pytest.mark.gpu
@pytest.mark.parametrize("light", ["rect", "point"])
@pytest.mark.parametrize("pair", PAIRS, ids=["%dx%d-%dx%d" % (a + b) for a, b in PAIRS])
def test_threshold_pairs_render_one_picture(pair, light, A, api, switches, table_kernels, no_boxes):
    """(c): the same room on both sides of a threshold -- two kernel forms, one picture."""
    films, kernels = [], []
    p = api.make_params(W, H, SPP, tile_w=16, tile_h=8)
    for ns, nm in pair:
        g, k = switches.render(api, limits_room(A, api, ns, nm, light, plastic=light == "point"), p)
        films.append(g)
        kernels.append(k)
    d = float(np.abs(films[0] - films[1]).max())
    print("%s %s -> %s: max |difference| %.2e  (%s | %s)" % (light, pair[0], pair[1], d, kernels[0], kernels[1]))
    # one kernel on both sides (the point light's row has no small-table form): padding only adds scans that find nothing -- the same bits.  Two kernels:
    # measured 6e-8 for the lamp, between the Cornell rows with and without the small tables and between the static and the scene-sized row alike;
    # the bound is test_specialised_instantiations_change_nothing's 2.4e-7 between rows (2e-5 for run-time instantiations, tests/test_jit.py's bound)
    bound = 0.0 if kernels[0] == kernels[1] else (2.4e-7 if table_kernels else 2e-5)
    assert d <= bound, (pair, light, d, kernels)
    # the queue engine on the static side agrees with the lane engine (test_engines_agree's bound) and hands the large side to the lane engine
    for (ns, nm), g in zip(pair, films):
        gq, kq = switches.render(api, limits_room(A, api, ns, nm, light, plastic=light == "point"), p, engine=1)
        dq = float(np.abs(gq - g).max())
        print("  %s queue engine: %s, max |difference| to the lane engine %.2e" % ((ns, nm), kq, dq))
        if _is_large(ns, nm):
            assert QUEUE_ENGINE not in kq and LARGE_BLOCK in kq and np.array_equal(gq, g), (ns, nm, kq)
        else:
            assert QUEUE_ENGINE in kq and dq <= 2e-5, (ns, nm, kq, dq)      # measured: at most 1.2e-7


@pytest.mark.gpu
def test_sphere_lamp_rows_need_the_small_tables(A, api, O, switches, table_kernels, no_boxes):
    """A sphere lamp at 16 and 17 surfaces: the sphere-light rows (KY_FEAT_VEACH) include the small tables, so one padding sphere more falls back to another
    row -- which must render the same picture, and the oracle's."""
    for strategy in (A.DIRECT_LIGHT_MIS, A.DIRECT_BSDF_MIS, A.DIRECT_BOTH_MIS):
        p = api.make_params(W, H, SPP, direct_sample=strategy, tile_w=16, tile_h=8)
        films = []
        for ns in (16, 17):
            scene = limits_room(A, api, ns, 8, "sphere", plastic=True)
            g, k = switches.render(api, scene, p)
            if table_kernels and strategy != A.DIRECT_BOTH_MIS:    # (both_mis has sphere-light rows with deferred shadow rays only: five lamps and more)
                assert bool(_feat(k) & FEAT_SPHERE_LIGHTS) == (ns == 16) and bool(_feat(k) & FEAT_SMALL) == (ns == 16), (ns, k)
            e = _parity(api, O, scene, p, g, _oracle(O, ("sphere", True), scene, p), "sphere lamp %d strategy %d" % (ns, strategy))
            films.append(g)
            print("sphere lamp (%d, 8) strategy %d: %s RMSE %.2e" % (ns, strategy, k, e))
        d = np.abs(films[0] - films[1]).max(axis=2)
        print("  16 -> 17 surfaces: max |difference| %.2e, %d pixel(s) beyond 2.4e-7" % (d.max(), int((d > 2.4e-7).sum())))
        # the sphere-light rows sample the lamp's cone with the reciprocal density (SceneRef::ipdf) and test its first carrier from the light's own record;
        # uniform-cone sampling cancels (ky.cpp:798, 1510-1512), so a light sample that grazes the lamp's silhouette can take the other outcome in one of the two
        # kernels -- test_recursion_look_up_rides_along's bound for the same effect.  Measured (light_mis): 2 pixels of 1920, 1.1e-3 and 3.1e-3, every other one
        # within 6e-8.  Under KYHIP_JIT=1 both sides carry the sphere-light facts and agree to the bit.
        assert int((d > 2.4e-7).sum()) <= 10 and d.max() < 1.0 / SPP + 1e-6, (strategy, float(d.max()), int((d > 2.4e-7).sum()))


@pytest.mark.gpu
def test_two_lights_deferred_rows_at_the_large_threshold(A, api, O, switches, table_kernels):
    """A point light and the lamp (the last light) at 64 and 65 surfaces with deferred shadow rays asked for: the deferred rows at 64, the LARGE row (which
    has no deferred form) at 65 -- one picture, the oracle's."""
    for strategy in (A.DIRECT_BOTH_MIS, A.DIRECT_LIGHT_MIS, A.DIRECT_LIGHT):
        p = api.make_params(W, H, SPP, direct_sample=strategy, tile_w=16, tile_h=8)
        films = []
        for ns in (64, 65):
            scene = limits_room(A, api, ns, 32, "rect", two_lights=True)
            g, k = switches.render(api, scene, p, shadow_queue=1)
            _assert_rows(k, ns, 32, False, table_kernels)
            assert not table_kernels or ("deferred shadow rays" in k) == (ns == 64), (ns, k)
            e = _parity(api, O, scene, p, g, _oracle(O, ("rect", False, "two"), scene, p), "two lights %d strategy %d" % (ns, strategy))
            films.append(g)
            print("two lights (%d, 32) strategy %d: %s RMSE %.2e" % (ns, strategy, k, e))
        d = np.abs(films[0] - films[1]).max(axis=2)
        print("  64 -> 65 surfaces: max |difference| %.2e, %d pixel(s) beyond 2e-6" % (d.max(), int((d > 2e-6).sum())))
        # deferred against inline: the same terms, added to a pixel in fixed point as they resolve instead of in float per vertex (test_random_room's bound;
        # measured here: at most 1.2e-7, no pixel beyond 2e-6).  A row of either table read one short moves whole regions, not ten pixels.
        assert int((d > 2e-6).sum()) <= 10 and d.max() <= 0.25, (strategy, float(d.max()), int((d > 2e-6).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("carriers", [0, 1, 2, 4, 5, "two bulbs"])
def test_carrier_counts(carriers, A, api, O, rng, switches, table_kernels):
    """One area light carried by 0, 1, 2, 4 and 5 surfaces (the fast path's carrier loop past k = 0, the n_carriers = -1 fallback, a light no surface shows),
    and a sphere lamp of two bulbs: the film against the oracle, and kat_nee term by term against the oracle at path vertices."""
    from test_kat_nee_gpu import _compare, _vertices
    if carriers == "two bulbs":
        scene, key = limits_room(A, api, 12, 8, "sphere", shared_sphere=True), ("sphere", "two bulbs")
    else:
        scene, key = limits_room(A, api, 12, 8, "rect", carriers=carriers), ("rect", "carriers", carriers)
    p = api.make_params(W, H, SPP, tile_w=16, tile_h=8)
    g, k = switches.render(api, scene, p)
    if table_kernels and carriers == 1:
        assert _feat(k) & FEAT_OWN, k
    e = _parity(api, O, scene, p, g, _oracle(O, key, scene, p), "carriers %s" % carriers)
    rows = _vertices(A, api, O, scene, rng, 4096, 1.2)
    assert len(rows) > 2000
    terms = flips = 0
    for strategy in (A.DIRECT_BSDF, A.DIRECT_LIGHT, A.DIRECT_BSDF_MIS, A.DIRECT_LIGHT_MIS, A.DIRECT_BOTH_MIS):
        gk, ck = api.kat_nee(scene, strategy, 0, rows), O.kat_nee(scene, strategy, 0, rows)
        fin = np.isfinite(ck).all(axis=1) & np.isfinite(gk).all(axis=1)
        assert fin.mean() > 0.999
        for half in (slice(0, 3), slice(3, 6)):
            t, f = _compare(gk[fin][:, half], ck[fin][:, half], 2e-2 if carriers == "two bulbs" else 5e-4)
            terms += t
            flips += f
    print("carriers %s: %s RMSE %.2e; kat_nee %d non-zero terms, %d differ in their discrete outcome" % (carriers, k, e, terms, flips))
    # (the Cornell KAT's bound; the sphere lamp's self-occlusion threshold, quirk 1, flips more: test_kat_nee_gpu's Veach bound.  Measured: no flip in any case)
    assert terms > 500 and flips <= (0.01 if carriers == "two bulbs" else 0.002) * terms, (terms, flips)


@pytest.mark.gpu
def test_abi_maxima_render_one_more_is_refused(A, api, O, switches):
    """64 materials, 16 lights and 256 shapes render (the unused ones change nothing); one more of any is refused with KY_ERR_LIMIT and the film is left alone."""
    lib = A.load_kyhip()
    base = limits_room(A, api, 12, 8, "rect")
    n_shapes, n_lights = base.scene.shape_count, base.scene.light_count
    p = api.make_params(W, H, 64, tile_w=16, tile_h=8)
    ref, _ = switches.render(api, base, p)
    for kw in (dict(materials=A.MAX_MATERIALS - 8), dict(lights=A.MAX_LIGHTS - n_lights), dict(shapes=A.MAX_SHAPES - n_shapes)):
        at = _with_extra(A, base, **kw)
        g, k = switches.render(api, at, p)
        e = rmse(g, O.render(at, p))
        print("%s: %s, RMSE against the oracle %.2e, max |difference| to the room without them %.2e" % (kw, k, e, np.abs(g - ref).max()))
        assert e < film_tolerance(64), (kw, e)
        over = _with_extra(A, base, **{key: v + 1 for key, v in kw.items()})
        film = np.full((H, W, 3), 0.25, np.float32)
        assert lib.kyhip_render(0, over.flat, C.byref(p), film.ctypes.data_as(C.c_void_p), W) == A.KY_ERR_LIMIT, kw
        assert (film == 0.25).all(), kw
