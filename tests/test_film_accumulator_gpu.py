"""The film accumulator on its own (DESIGN.md "Film").  Every render kernel adds a pixel's radiance to a signed 32.32 fixed-point word in terms
(the lane engine: one per pixel chunk, plus one per resolved deferred shadow ray; the queue engine: one per sample), and resolve_kernel turns the
word back into a float and applies clamp01 (ky.cpp:3726).  These tests render scenes whose every sample's radiance is known in advance -- an
environment light seen by every camera ray of an empty scene returns exactly its colour -- and compare the film with the exact value:

  (a) every sample is counted once, for spp on both sides of every segment of the chunk plan, on every way a frame is rendered;
  (b) the conversion rounds to nearest-even on the device, on both engines (the expected values are integers times 2^-32, compared with ==);
  (c) a pixel whose sum is beyond the word's range saturates, on every kernel family that flushes a pixel: no term sum may wrap;
  (d) the same behind shading (area + point light, every strategy, deferred shadow rays on and off, the queue engine), against the oracle."""
import numpy as np
import pytest

from helpers import CustomScene, chunk_count as _chunk_count, explain_pixel, make_light, make_material, make_shape

pytestmark = pytest.mark.gpu

U = 2.0 ** -32   # one unit of the accumulator


def _camera(A, api, W, H):
    return A.Camera.from_buffer_copy(api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H).c.camera)


def _env_scene(A, api, colour, W, H, behind=()):
    """An environment light of radiance `colour` and nothing in view: every camera sample returns exactly `colour`.  `behind`: surfaces (shapes
    given as (kind, points, radius)) placed behind the camera, where no ray of the frame goes -- they only decide which kernel renders it."""
    cam = _camera(A, api, W, H)
    pos, front = np.array(cam.position[:], np.float64), np.array(cam.front[:], np.float64)
    front /= np.linalg.norm(front)
    back = pos - 40.0 * front
    shapes = [make_shape(A, A.SHAPE_SPHERE, [(0, 0, 0)], radius=1.0)]
    surfaces = []
    for kind, pts, radius in behind:
        shapes.append(make_shape(A, kind, [tuple(back + np.array(p)) for p in pts], radius=radius))
        surfaces.append(A.Surface(len(shapes) - 1, 0, -1))
    sc = CustomScene(A, cam, shapes, [make_material(A, A.MATERIAL_MATTE, (0.5, 0.5, 0.5))],
                     [make_light(A, A.LIGHT_ENVIRONMENT, tuple(float(x) for x in colour), world_radius=1.0)], surfaces, environment_light=0)
    sc.scene.surface_count = len(surfaces)
    return sc


def _behind(A, what):
    if what == "triangle":
        return [(A.SHAPE_TRIANGLE, [(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (0.0, 1.0, 0.0)], 0.0)]
    if what == "many":   # more than KY_LDS_SURFACES (64) surfaces: the kernels with the scene-sized LDS block
        return [(A.SHAPE_SPHERE, [(0.5 * (i % 10), 0.5 * (i // 10), 0.0)], 0.2) for i in range(70)]
    return []


class _Switches:
    """Library switches changed by a test, restored in `finally`."""

    def __init__(self, lib):
        self.lib = lib
        self.prev = (lib.kyhip_set_engine(0), lib.kyhip_set_specialisation(1), lib.kyhip_set_shadow_queue(-1))

    def restore(self):
        self.lib.kyhip_set_engine(self.prev[0])
        self.lib.kyhip_set_specialisation(self.prev[1])
        self.lib.kyhip_set_shadow_queue(self.prev[2])


# ---- (a) every sample counted exactly once ----

SPPS = (1, 2, 3, 4, 5, 23, 24, 25, 63, 64, 65, 255, 256, 447, 448, 449, 1000, 4097)
FRAMES = ((1, 1), (37, 29), (130, 70))
TILES = ((8, 8), (16, 16), (32, 8))


def _count_bound(c, n_terms):
    """|pixel - c| for n_terms terms that add up to c: each term is a float product (a chunk's sum k x 0.75 is exact, k <= 24) by inv_spp, which is
    itself rounded -- 2^-24 relative each, c x (2^-23 + 2^-48) over all terms --, each term's conversion is off by half a unit at most, and the
    resolve rounds the sum to a float (half an ulp of c)."""
    return c * (2.0 ** -23 + 2.0 ** -48) + n_terms * 0.5 * U + 0.5 * np.spacing(np.float32(c)) + 1e-15


def test_every_sample_counted_once(A, api):
    lib = A.load_kyhip()
    sw = _Switches(lib)
    c = 0.75
    try:
        rng = np.random.default_rng(11)
        for spp in SPPS:
            lane_value = None
            for (W, H) in FRAMES:
                scene = _env_scene(A, api, (c, c, c), W, H)
                for (tw, th) in TILES:
                    p = api.make_params(W, H, spp, tile_w=tw, tile_h=th)
                    what = (spp, W, H, tw, th)
                    lib.kyhip_set_engine(0)
                    lane = api.render(scene, p)
                    assert b"queue engine" not in lib.kyhip_last_kernel(0), what
                    # one value for every pixel, every frame and every tiling (the chunk plan depends on spp only)
                    assert (lane == lane.flat[0]).all(), what
                    lane_value = lane.flat[0] if lane_value is None else lane_value
                    assert lane.flat[0] == lane_value, what
                    assert abs(float(lane_value) - c) <= _count_bound(c, _chunk_count(spp)), (what, float(lane_value) - c)
                    # three shards into one film, and kyhip_render_multi with its shards on one device: bit-identical to the whole frame
                    parts = np.zeros_like(lane)
                    for k in range(3):
                        api.render(scene, api.make_params(W, H, spp, tile_w=tw, tile_h=th, tile_first=k, tile_step=3), film=parts)
                    assert np.array_equal(parts, lane), what
                    assert np.array_equal(api.render_multi(scene, p, [0, 0]), lane), what
                    # the host film seam adds once, on top of what the film holds
                    base = rng.uniform(0, 1, lane.shape).astype(np.float32)
                    assert np.array_equal(api.render(scene, p, film=base.copy()), base + lane), what
                    # the queue engine: one term per sample
                    lib.kyhip_set_engine(1)
                    q = api.render(scene, p)
                    assert b"queue engine" in lib.kyhip_last_kernel(0), what
                    lib.kyhip_set_engine(0)
                    assert (q == q.flat[0]).all(), what
                    assert abs(float(q.flat[0]) - c) <= _count_bound(c, spp), (what, float(q.flat[0]) - c)
    finally:
        sw.restore()


# ---- (b) rounding of the conversion on the device ----

def _rne_units(a):
    """round-half-even(a x 2^32) for float64 a (np.rint rounds ties to even)"""
    return int(np.rint(np.float64(a) * 2.0 ** 32))


def _resolve(units):
    v = np.float32(units * U)    # (double)(long long) word * 2^-32, then float: as resolve_kernel
    return np.float32(min(max(v, 0.0), 1.0))


def test_conversion_rounds_to_nearest_even(A, api):
    lib = A.load_kyhip()
    sw = _Switches(lib)
    rng = np.random.default_rng(5)
    vals = [0.5 * U, 1.5 * U, 2.5 * U, 3.5 * U, 4.5 * U, float(np.nextafter(np.float32(2.0 ** -9), np.float32(0))), 2.0 ** -9,
            float(np.nextafter(np.float32(2.0 ** -9), np.float32(1))), 1.0 - 2.0 ** -24, float(np.float32(1e-40)), float(np.float32(3e-39)),
            -0.5 * U, -3.0 * U, -1e-6, -2.0 ** -20, 0.0]
    vals += [float(x) for x in np.exp2(rng.uniform(-40, -8, 300)).astype(np.float32)]
    vals = [float(np.float32(v)) for v in vals]
    while len(vals) % 3:
        vals.append(0.25)
    try:
        for engine in (0, 1):
            lib.kyhip_set_engine(engine)
            for spp in (1, 2):
                inv = np.float32(1.0 / spp)
                for i in range(0, len(vals), 3):
                    col = vals[i:i + 3]
                    g = api.render(_env_scene(A, api, col, 1, 1), api.make_params(1, 1, spp, tile_w=8, tile_h=8))
                    assert (b"queue engine" in lib.kyhip_last_kernel(0)) == (engine == 1)
                    for ch in range(3):
                        a = np.float32(col[ch])
                        if engine == 0:   # one chunk: (a + ... + a) x inv_spp = a exactly, one term
                            units = _rne_units(a)
                        else:             # one term per sample: a x inv_spp (exact for these spp), rounded each
                            units = spp * _rne_units(np.float32(a * inv))
                        want = _resolve(units)
                        assert g[0, 0, ch] == want, ("engine", engine, "spp", spp, "value", float(a), float(g[0, 0, ch]), float(want))
    finally:
        sw.restore()


# ---- (c) bright pixels saturate and never wrap ----

MAGS = (1.5e9, 2.0 ** 31 - 128, 2.0 ** 31, 2.2e9, 3e9, 1e10, 1e15, 3.4e38)
COLOURS = [(m, m, m) for m in MAGS] + [(-m, -m, -m) for m in MAGS] + \
          [(MAGS[i], -MAGS[(i + 3) % 8], MAGS[(i + 5) % 8]) for i in range(8)] + [(0.25, 2.2e9, -3e9), (-1e10, 0.5, 2.0 ** 31)]


def _families(A):
    """(name, setup(lib), scene extras, params overrides, what kyhip_last_kernel must contain)"""
    it = A.INTEGRATOR_PATH_TRACING_ITERATION
    f = [("table row", None, "", {}, b"integrator %d" % it),
         ("fact-free kernel", lambda lib: lib.kyhip_set_specialisation(0), "", {}, b"feat 0, integrator %d" % it),
         ("general shapes", None, "triangle", {}, b"general shapes"),
         ("large scene", None, "many", {}, b"scene-sized LDS block"),
         ("debug sampler", None, "", {"sampler": A.SAMPLER_DEBUG}, b"debug sampler"),
         ("queue engine", lambda lib: lib.kyhip_set_engine(1), "", {}, b"queue engine")]
    for integ in (A.INTEGRATOR_DIRECT_LIGHTING, A.INTEGRATOR_SIMPLE_PATH_TRACING_RECURSION, A.INTEGRATOR_PATH_TRACING_RECURSION,
                  A.INTEGRATOR_PATH_TRACING_RECURSION_DEFERED):
        f.append(("integrator %d" % integ, None, "", {"integrator": integ}, b"integrator %d" % integ))
    return f


def test_bright_pixels_saturate(A, api):
    lib = A.load_kyhip()
    sw = _Switches(lib)
    W = H = 8
    failures = []
    try:
        for name, setup, behind, over, kernel in _families(A):
            if setup:
                setup(lib)
            try:
                for colour in COLOURS:
                    scene = _env_scene(A, api, colour, W, H, _behind(A, behind))
                    want = np.clip(np.array(colour, np.float64), 0, 1).astype(np.float32)
                    for spp in (1, 4, 64, 1024):
                        g = api.render(scene, api.make_params(W, H, spp, tile_w=8, tile_h=8, **over))
                        k = lib.kyhip_last_kernel(0)
                        assert kernel in k, (name, k)
                        bad = np.flatnonzero((g != want).any(axis=2))
                        if bad.size:
                            failures.append((name, spp, colour, g.reshape(-1, 3)[bad[0]].tolist()))
            finally:
                sw.restore()
    finally:
        sw.restore()
    assert not failures, "%d renders off clamp01(colour), e.g. %s" % (len(failures), failures[:12])


# ---- (d) accumulation behind shading ----

def _room(A, api, sign):
    """tests/test_nonfinite_gpu.py's room, lit by an area light and a point light bright enough that the pixels they light sum past 2^31 while
    every chunk of them stays below the old per-chunk range check"""
    W, H = 48, 40
    camera = _camera(A, api, W, H)
    shapes = [
        make_shape(A, A.SHAPE_RECTANGLE, [(-1.3, -1.3, -1.28), (1.3, -1.3, -1.28), (1.3, 1.3, -1.28), (-1.3, 1.3, -1.28)]),
        make_shape(A, A.SHAPE_RECTANGLE, [(-1.3, -1.3, -1.28), (-1.3, -1.3, 1.28), (1.3, -1.3, 1.28), (1.3, -1.3, -1.28)]),
        make_shape(A, A.SHAPE_RECTANGLE, [(-0.4, -1.0, 0.2), (-0.4, -1.0, 0.9), (0.4, -1.0, 0.9), (0.4, -1.0, 0.2)]),
        make_shape(A, A.SHAPE_SPHERE, [(0.6, 0.0, -0.9)], radius=0.35),
    ]
    materials = [make_material(A, A.MATERIAL_MATTE, (0.7, 0.7, 0.7)), make_material(A, A.MATERIAL_MATTE, (0, 0, 0)),
                 make_material(A, A.MATERIAL_PLASTIC, (0.2, 0.2, 0.2), (0.5, 0.5, 0.5), exponent=30.0)]
    lights = [make_light(A, A.LIGHT_AREA, (sign * 3e10, sign * 1e10, sign * 3e9), shape=2),
              make_light(A, A.LIGHT_POINT, (sign * 3e10, sign * 1e10, sign * 3e9), position=(0.0, 0.5, 1.0))]
    surfaces = [A.Surface(0, 0, -1), A.Surface(1, 0, -1), A.Surface(2, 1, 0), A.Surface(3, 2, -1)]
    return CustomScene(A, camera, shapes, materials, lights, surfaces), W, H


def _check_against_oracle(api, O, scene, p, g, c, what):
    assert np.isfinite(g).all() and g.min() >= 0 and g.max() <= 1, what
    fin = np.isfinite(c)
    assert (g[~fin] == 0).all(), what
    sat = fin & ((c == 0) | (c == 1))
    off = (sat & (g != c)).any(axis=2)
    ys, xs = np.nonzero(off)
    assert len(ys) <= 6, (what, "saturated pixels off", len(ys), [(int(x), int(y), g[y, x].tolist(), c[y, x].tolist()) for y, x in zip(ys[:6], xs[:6])])
    keep = fin.copy()
    for y, x in zip(ys, xs):   # a decision flip in a pixel of such radiance moves it from 0 to 1 or back: explained sample by sample, or a failure
        kinds = explain_pixel(api, O, scene, p, int(x), int(y), value_tol=2e-4, geom_tol=1e-4)
        assert sum(v for k, v in kinds.items() if k != "within tolerance") > 0, (what, int(x), int(y), kinds)
        keep[y, x] = False
    rest = keep & ~sat
    if rest.any():
        d = np.abs(g[rest].astype(np.float64) - c[rest])
        assert d.max() < 2e-2 and np.sqrt(np.mean(d ** 2)) < 2e-3, (what, float(d.max()))


def test_shading_sums_saturate(A, api, O):
    lib = A.load_kyhip()
    sw = _Switches(lib)
    strategies = (A.DIRECT_BOTH_MIS, A.DIRECT_LIGHT_MIS, A.DIRECT_LIGHT, A.DIRECT_BSDF)
    deferrable = (A.DIRECT_BOTH_MIS, A.DIRECT_LIGHT_MIS, A.DIRECT_LIGHT)
    try:
        for sign in (1.0, -1.0):
            scene, W, H = _room(A, api, sign)
            for strategy in strategies:
                p = api.make_params(W, H, 64, direct_sample=strategy, tile_w=16, tile_h=8)
                with np.errstate(all="ignore"):
                    c = O.render(scene, p)
                assert (c == (1 if sign > 0 else 0)).mean() > 0.2     # much of the room is lit far beyond 1 (or below 0)
                for engine, sq in ((0, 1), (0, 0), (1, -1)):
                    lib.kyhip_set_engine(engine)
                    lib.kyhip_set_shadow_queue(sq)
                    g = api.render(scene, p)
                    k = lib.kyhip_last_kernel(0)
                    if engine == 1:
                        assert b"queue engine" in k, k
                    else:
                        assert (b"deferred shadow rays" in k) == (sq == 1 and strategy in deferrable), k
                    _check_against_oracle(api, O, scene, p, g, c, (sign, strategy, engine, sq))
                    if engine == 0 and strategy == A.DIRECT_BOTH_MIS:   # sharded against whole
                        parts = np.zeros_like(g)
                        for r in range(3):
                            api.render(scene, api.make_params(W, H, 64, direct_sample=strategy, tile_w=16, tile_h=8, tile_first=r, tile_step=3), film=parts)
                        assert np.array_equal(parts, g), (sign, sq)
                lib.kyhip_set_engine(0)
                lib.kyhip_set_shadow_queue(-1)
    finally:
        sw.restore()
