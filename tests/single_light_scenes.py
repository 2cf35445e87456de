"""Scenes of the sample_single_light tests (direct_sample 49) that no shipped scene offers: sixteen lights of mixed kinds (KYHIP_MAX_LIGHTS: a full table of
staged light records, indices up to 15, decision bits 15 and 31), and one delta light repeated n times (under the debug sampler the pick is light n / 2, and n
times one of n identical estimates is their sum: 49 renders 48's picture).  Shared by the GPU tests and the oracle-only controls."""
import numpy as np

from helpers import CustomScene, make_light, make_material, make_shape, unit

ROOM_A, ROOM_B, ROOM_H = 1.3, 1.3, 1.28                 # test_random_scenes_gpu.random_room's room, axis-aligned
STAT_SPP = 1024                                         # samples per pixel of the statistical test and of its oracle-only controls


def _room(A, api, width, height):
    """-> camera, shapes, materials, surfaces: five walls, a matte and a plastic sphere (no delta lobes: every vertex takes direct lighting)"""
    cam = A.Camera.from_buffer_copy(api.cornell_box_scene(A.CB_DEFAULT_SCENE, width, height).c.camera)
    a, b, h = ROOM_A, ROOM_B, ROOM_H
    R = lambda pts: make_shape(A, A.SHAPE_RECTANGLE, pts)
    shapes = [R([(-a, -b, -h), (a, -b, -h), (a, b, -h), (-a, b, -h)]),       # floor
              R([(-a, -b, -h), (-a, -b, h), (a, -b, h), (a, -b, -h)]),       # back wall
              R([(-a, -b, h), (-a, -b, -h), (-a, b, -h), (-a, b, h)]),       # left
              R([(a, -b, -h), (a, -b, h), (a, b, h), (a, b, -h)]),           # right
              R([(a, -b, h), (-a, -b, h), (-a, b, h), (a, b, h)]),           # ceiling
              make_shape(A, A.SHAPE_SPHERE, [(-0.55, -0.3, -0.83)], radius=0.45),
              make_shape(A, A.SHAPE_SPHERE, [(0.6, 0.35, -0.93)], radius=0.35)]
    materials = [make_material(A, A.MATERIAL_MATTE, (0.75, 0.75, 0.75)), make_material(A, A.MATERIAL_MATTE, (0.63, 0.065, 0.05)),
                 make_material(A, A.MATERIAL_MATTE, (0.14, 0.45, 0.091)), make_material(A, A.MATERIAL_MATTE, (0, 0, 0)),
                 make_material(A, A.MATERIAL_PLASTIC, (0.08, 0.2, 0.6), (0.35, 0.35, 0.35), exponent=12.0)]
    surfaces = [A.Surface(0, 0, -1), A.Surface(1, 0, -1), A.Surface(2, 1, -1), A.Surface(3, 2, -1), A.Surface(4, 0, -1), A.Surface(5, 0, -1), A.Surface(6, 4, -1)]
    return cam, shapes, materials, surfaces


def _set_world_radius(A, O, scene, n_lights):
    radius = float(O.world_bounding_sphere(scene)[3])      # direction / environment lights: preprocess() (3555-3574)
    for l in scene.lights[:n_lights]:
        if l.kind in (A.LIGHT_DIRECTION, A.LIGHT_ENVIRONMENT):
            l.world_radius = radius


SIXTEEN_KINDS = ("rect", "point", "sphere", "direction", "rect", "sphere", "point", "environment",
                 "sphere", "rect", "direction", "point", "rect", "sphere", "direction", "point")   # the LAST light (index 15) is a point light, 14 a directional one


def sixteen_lights_scene(A, api, O, width=48, height=40):
    """-> (scene, kinds): the room with KYHIP_MAX_LIGHTS = 16 lights: 4 rectangle lamps, 4 sphere lamps, 4 point, 3 directional lights and the environment"""
    cam, shapes, materials, surfaces = _room(A, api, width, height)
    lights, env = [], -1
    for li, k in enumerate(SIXTEEN_KINDS):
        col = (0.4 + 0.035 * li, 0.9 - 0.03 * li, 0.5 + 0.02 * ((7 * li) % 16))
        x, y = -0.9 + 0.6 * (li % 4), -0.8 + 0.5 * (li // 4)
        if k == "rect":
            z, s = ROOM_H - 0.02 - 0.01 * li, 0.12
            shapes.append(make_shape(A, A.SHAPE_RECTANGLE, [(x - s, y - s, z), (x - s, y + s, z), (x + s, y + s, z), (x + s, y - s, z)]))   # faces down
            lights.append(make_light(A, A.LIGHT_AREA, tuple(20 * c for c in col), shape=len(shapes) - 1))
            surfaces.append(A.Surface(len(shapes) - 1, 3, li))
        elif k == "sphere":
            shapes.append(make_shape(A, A.SHAPE_SPHERE, [(x, y, 0.55 + 0.02 * li)], radius=0.08))
            lights.append(make_light(A, A.LIGHT_AREA, tuple(30 * c for c in col), shape=len(shapes) - 1))
            surfaces.append(A.Surface(len(shapes) - 1, 3, li))
        elif k == "point":
            lights.append(make_light(A, A.LIGHT_POINT, tuple(2 * c for c in col), position=(x, y, 0.3 + 0.03 * li)))
        elif k == "direction":
            lights.append(make_light(A, A.LIGHT_DIRECTION, tuple(1.5 * c for c in col), direction=tuple(unit(np.array([0.1 * (li - 8), -1.0, -0.6])))))
        else:
            lights.append(make_light(A, A.LIGHT_ENVIRONMENT, tuple(0.5 * c for c in col)))
            env = li
    assert len(lights) == A.MAX_LIGHTS == 16
    scene = CustomScene(A, cam, shapes, materials, lights, surfaces, environment_light=env)
    _set_world_radius(A, O, scene, len(lights))
    return scene, SIXTEEN_KINDS


def repeated_delta_scene(A, api, O, kind, width=48, height=40):
    """The room under ONE delta light listed several times: "point" three times, "direction" four times"""
    cam, shapes, materials, surfaces = _room(A, api, width, height)
    if kind == "point":
        lights = [make_light(A, A.LIGHT_POINT, (0.7, 0.6, 0.5), position=(0.1, 0.3, 0.8)) for _ in range(3)]
    else:
        assert kind == "direction"
        lights = [make_light(A, A.LIGHT_DIRECTION, (0.8, 0.7, 0.6), direction=tuple(unit(np.array([0.3, -1.0, -0.8])))) for _ in range(4)]
    scene = CustomScene(A, cam, shapes, materials, lights, surfaces)
    _set_world_radius(A, O, scene, len(lights))
    return scene


def stat_case(which, A, api):
    """-> scene, W, H, the fixed interleaved pixel set (at least 256 pixels) of the statistical test"""
    if which == "veach":
        W, H = 64, 36
        return api.mis_scene(W, H), W, H, [(x, y) for y in range(1, H, 2) for x in range(2, W, 4)]                      # 16 x 18 = 288
    W = H = 64
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA | A.CB_LIGHT_POINT, W, H)
    return scene, W, H, [(x, y) for y in range(2, H, 4) for x in range(1 + (y // 4) % 2, W, 3)]                         # 16 staggered rows of 21: 336


def luminance(li):
    li = np.asarray(li, np.float64)
    return 0.212671 * li[:, 0] + 0.715160 * li[:, 1] + 0.072169 * li[:, 2]


def z_scores(a, b):
    """a, b: [pixels, S] luminances of two estimators -> (z of the pixels where either side varies, the largest |difference of means| relative to the mean
    among the pixels where neither does).  z = (mean a - mean b) / sqrt(var a / S + var b / S) with the two sample variances."""
    S = a.shape[1]
    ma, mb = a.mean(axis=1), b.mean(axis=1)
    se = np.sqrt(a.var(axis=1, ddof=1) / S + b.var(axis=1, ddof=1) / S)
    varies = se > 0
    fixed = np.abs(ma - mb)[~varies] / np.maximum(1.0, np.abs(mb)[~varies])
    return (ma - mb)[varies] / se[varies], (float(fixed.max()) if fixed.size else 0.0)


# Thresholds of the statistical test, from the normal law alone.  With P pixels of independent z ~ N(0, 1) the mean z has standard error 1 / sqrt(P): the bound
# is four of them (two-sided probability 6.3e-5).  A pixel lies beyond |z| = 4 with the same probability 6.3e-5, so among P <= 288 pixels the expected count is
# 0.018 and three or more have probability below 1e-6: the cap on the share is 1 % (at most two pixels of 256 ... 288), which also leaves a Student-t tail of
# the bright, rarely hit lamps room without admitting a bias (a factor n on the direct part puts most lit pixels beyond 4: the counter-example below).
Z_MEAN_SIGMAS = 4.0
Z_TAIL, Z_TAIL_SHARE = 4.0, 0.01


def z_verdict(z):
    """-> (passes, |mean z| in standard errors of the mean, share of pixels beyond Z_TAIL)"""
    mean_in_se = abs(float(z.mean())) * np.sqrt(len(z))
    share = float((np.abs(z) > Z_TAIL).mean())
    return mean_in_se <= Z_MEAN_SIGMAS and share <= Z_TAIL_SHARE, mean_in_se, share
