"""Scenes, pixels and oracle references of the light-class tests (kyhip_render_lighting, lighting_enum_t): shared by the GPU tests and the oracle-only controls.

A masked render keeps the contributions of the selected classes and changes nothing else of a sample, roulette starts at bounces > 3 and a sample's stream is a
prefix of itself: so, per camera sample, the classes are differences of the UNMASKED oracle at max_path_depth 0, 1 and D (`identity`).  direct_lighting_t (6)
ignores the depth: its emission is path_tracing_iteration_t's radiance at depth 0 (the camera ray's own hit), its estimate the rest of its own radiance."""
import functools

import numpy as np

from helpers import CustomScene

DEPTH = 5
N_SAMPLES = 16          # per pixel, per-sample tests (8-32 spp)
FILM_SPP = 16


def open_room_scene(A, api, width, height):
    """ky's default frame (the Cornell box under the environment light) WITHOUT its back wall: the camera looks through the room into the environment, so a camera
    ray's miss is the emitter (class emit), as is a miss after one bounce off the mirror ball (direct) or after the two refractions of the glass ball (indirect).
    The same shapes, materials, light (with its preprocessed world radius) and camera, copied from the host mirror's scene."""
    room = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT, width, height)   # (alive until the copies below are made)
    c = room.c
    copy = lambda T, arr, n: [T.from_buffer_copy(arr[i]) for i in range(n)]
    shapes, materials, lights = copy(A.Shape, c.shapes, c.shape_count), copy(A.Material, c.materials, c.material_count), copy(A.Light, c.lights, c.light_count)
    back = [i for i, sh in enumerate(shapes) if sh.kind == A.SHAPE_RECTANGLE and all(abs(sh.p[j][1] - sh.p[0][1]) < 1e-6 for j in range(4)) and sh.p[0][1] < -1.0
            and abs(sh.p[0][0] - sh.p[2][0]) > 2.0]
    assert len(back) == 1, back   # the wall in the plane y = -1.3 that spans the room
    surfaces = [A.Surface.from_buffer_copy(c.surfaces[i]) for i in range(c.surface_count) if c.surfaces[i].shape != back[0]]
    assert len(surfaces) == c.surface_count - 1
    return CustomScene(A, A.Camera.from_buffer_copy(c.camera), shapes, materials, lights, surfaces, environment_light=c.environment_light)


def scenes(A, api):
    """name -> (scene, width, height, the share of differing samples tests/test_parity_gpu.py allows kat_li against O.li on that scene)"""
    return {
        "cornell": (api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA | A.CB_LIGHT_POINT, 48, 48), 48, 48, 0.002),   # two lights, mirror and glass
        "veach": (api.mis_scene(64, 36), 64, 36, 0.014),                                                                         # deferred rays (test_li_per_sample_veach's share)
        "default": (api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT, 48, 48), 48, 48, 0.002),               # ky's default frame: lit by misses, none of them the camera ray's
        "open": (open_room_scene(A, api, 48, 48), 48, 48, 0.002),                                                                  # ... without its back wall: a camera ray's miss is the emitter
    }


# Fixed pixels (tests/test_lighting_controls.py shows, on the oracle alone, that every class is non-zero on a quarter of those that see the room, and that the
# marked ones receive emission after exactly one / exactly two specular bounces).  Found with the oracle; the GPU had no say.
PIXELS = {
    "cornell": [(22, 5), (24, 6), (26, 5), (21, 6), (24, 24), (4, 4), (45, 45), (8, 24), (24, 44), (17, 29), (33, 34), (13, 37)],    # the first four see the lamp
    "veach": [(53, 6), (46, 5), (39, 4), (32, 18), (4, 4), (20, 26), (46, 20), (32, 33), (13, 13), (53, 30), (24, 30), (36, 24)],    # the first three see a sphere lamp
    "default": [(24, 24), (4, 4), (16, 31), (33, 34), (45, 45), (24, 3), (13, 37), (34, 39), (16, 33), (26, 33), (24, 44), (8, 24)],
    "open": [(22, 10), (30, 14), (14, 16), (26, 17), (22, 20), (4, 4), (45, 45), (24, 44), (8, 24), (17, 28), (30, 32), (16, 33)],    # the first five look through the room into the environment
}
# The scenes whose pixels the oracle-only controls vouch for.  ky's default frame is not one of them: its room closes the view, no camera ray of it reaches the
# environment, and its emit class is empty -- the open room stands in for it wherever a miss has to BE the emitter; the default frame itself stays in the GPU tests
# as one more scene, for the table row it lands on.
CONTROLLED = ("cornell", "veach", "open")
ONE_SPECULAR = {"cornell": (17, 29), "default": (16, 33), "open": (17, 28)}    # emission reached through one mirror / glass bounce: direct light
TWO_SPECULAR = {"default": (26, 33), "open": (30, 32)}                         # ... through two (into the glass ball and out of it): indirect


def params(api, A, name, w, h, spp=N_SAMPLES, depth=DEPTH, integrator=None, **kw):
    return api.make_params(w, h, spp, integrator=A.INTEGRATOR_PATH_TRACING_ITERATION if integrator is None else integrator, max_path_depth=depth, **kw)


def at_depth(A, p, depth, integrator=None):
    q = A.RenderParams.from_buffer_copy(p)
    q.max_path_depth = depth
    if integrator is not None:
        q.integrator = integrator
    return q


def oracle_terms(A, O, scene, p, x, y, n):
    """-> (li(0), li(1), li(D)) of the unmasked oracle as float64 [n, 3]; integrator 6: (iteration's li(0), its own li, its own li)"""
    if p.integrator == A.INTEGRATOR_DIRECT_LIGHTING:
        l0 = O.li(scene, at_depth(A, p, 0, A.INTEGRATOR_PATH_TRACING_ITERATION), x, y, 0, n).astype(np.float64)
        l = O.li(scene, p, x, y, 0, n).astype(np.float64)
        return l0, l, l
    return tuple(O.li(scene, at_depth(A, p, d), x, y, 0, n).astype(np.float64) for d in (0, 1, p.max_path_depth))


def identity(mask, l0, l1, lD):
    """what lighting `mask` adds per sample, from the unmasked radiance at depth 0, 1 and D"""
    out = np.zeros_like(lD)
    if mask & 1:
        out = out + l0
    if mask & 2:
        out = out + (l1 - l0)
    if mask & 4:
        out = out + (lD - l1)
    return out


def differing(g, c):
    """tests/test_parity_gpu.py's li_agreement: a sample differs when it is off by more than 1e-3 of max(1e-3, |c|); non-finite oracle samples do not count.
    -> (differing, counted)"""
    fin = np.isfinite(c).all(1)
    d = np.abs(g[fin] - c[fin]).max(axis=1)
    s = np.maximum(1e-3, np.abs(c[fin]).max(axis=1))
    return int((d / s > 1e-3).sum()), int(fin.sum())


def specular_emission(A, O, scene, p, x, y, n):
    """-> (samples of the pixel that receive emission after exactly one specular bounce, after exactly two), from the oracle's vertex traces: the first
    (two) vertices are mirror / glass lobes -- which take no light estimate -- and the radiance grows between depth 0 and 1 (1 and 2)."""
    l0, l1, l2 = (O.li(scene, at_depth(A, p, d), x, y, 0, n).astype(np.float64) for d in (0, 1, 2))
    one = two = 0
    for s in range(n):
        rows = O.trace_li(scene, at_depth(A, p, 2), x, y, s)
        delta = [int(r[2]) in (1, 2) for r in rows]
        if len(rows) >= 1 and delta[0] and np.abs(l1[s] - l0[s]).max() > 0:
            one += 1
        if len(rows) >= 2 and delta[0] and delta[1] and np.abs(l2[s] - l1[s]).max() > 0:
            two += 1
    return one, two
