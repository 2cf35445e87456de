"""GPU: textures on material colours (ky_texture).  The probe kyhip_kat_texture against the NumPy restatement (tests/texture_restatement.py);
the textured kernels' samples and films against the CPU oracle on the TILED scene (every textured rectangle cut along its cells or texels into constant-colour
rectangles: same tape, same path, the colour at a vertex is the tile's); a checker of one colour against the untextured render; every way of cutting a textured
frame against the one-shot render, bit for bit; the textures as part of a frame's identity; one frame per textured row of the kernel table.
tests/test_texture.py holds the restatement and the tiling themselves."""
import ctypes as C

import numpy as np
import pytest

import filter_restatement as F
import test_filter_gpu as TF      # CAPS, params_of, sampler_kind
import test_lens_gpu as TL        # lens_of, and the oracle at a lens point
import test_stratified_gpu as T   # film_tolerance, film_of, large_scene
import texture_restatement as X
from helpers import make_material, make_shape, rmse

pytestmark = pytest.mark.gpu

SAMPLERS = ("random", "stratified")
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib(A):
    lib = A.load_kyhip()
    prev = lib.kyhip_set_jit(0)
    yield lib
    lib.kyhip_set_jit(prev)


def api_textures(api, textures):
    return [t.to_api(api) for t in textures]


def case_of(A, api, name, w, h):
    return X.veach_case(A, api, w, h) if name == "veach" else X.cornell_case(A, api, w, h)


# ---- 1. the probe is the restatement ----

def smooth_image():
    c = (np.arange(8) + 0.5) / 8
    g = 0.5 + 0.4 * np.outer(np.sin(2 * np.pi * c), np.sin(2 * np.pi * c))   # a product of two sines on 8 x 8 texels
    return np.stack([g, 0.5 * g, 1 - g], axis=2).astype(f32)


def probe_shapes(A):
    """name -> (ky_shape, 4096 world points of it).  The points are a jittered grid in the shape's own coordinates, so no fixed share of them sits on an edge."""
    gen = np.random.default_rng(20261021)
    s, t = gen.random(4096), gen.random(4096)
    out = {}
    quad = [(-1.0, 0.5, 2.0), (2.0, 0.5, 2.5), (2.0, 0.5, 6.0), (-1.0, 0.5, 6.5)]
    sh = make_shape(A, A.SHAPE_RECTANGLE, quad)
    P = np.array(quad)
    out["rectangle"] = (sh, P[0] + np.outer(s, P[1] - P[0]) + np.outer(t, P[3] - P[0]))
    skew = [(0.0, 0.0, 0.0), (3.0, 0.0, 0.0), (4.0, 2.5, 0.0), (-0.5, 2.0, 0.0)]   # no parallelogram: (u, v) is simply the definition
    P = np.array(skew)
    bil = (1 - s)[:, None] * ((1 - t)[:, None] * P[0] + t[:, None] * P[3]) + s[:, None] * ((1 - t)[:, None] * P[1] + t[:, None] * P[2])
    out["quad"] = (make_shape(A, A.SHAPE_RECTANGLE, skew), bil)
    tri = [(1.0, 1.0, 1.0), (3.0, 1.5, 0.5), (1.5, 3.0, 2.0)]
    P = np.array(tri)
    r = np.sqrt(s)
    out["triangle"] = (make_shape(A, A.SHAPE_TRIANGLE, tri), P[0] + np.outer(r * (1 - t), P[1] - P[0]) + np.outer(r * t, P[2] - P[0]))
    n = np.array([1.0, 2.0, 2.0]) / 3.0
    fs, ft = X.frame(n.astype(f32))
    rr, ph = 1.5 * np.sqrt(s), 2 * np.pi * t
    out["disk"] = (make_shape(A, A.SHAPE_DISK, [(0.5, -1.0, 2.0)], normal=n, radius=1.5),
                   np.array([0.5, -1.0, 2.0]) + np.outer(rr * np.cos(ph), fs.astype(f64)) + np.outer(rr * np.sin(ph), ft.astype(f64)))
    z, ph = 1 - 2 * s, 2 * np.pi * t
    d = np.stack([np.sqrt(1 - z * z) * np.cos(ph), z, np.sqrt(1 - z * z) * np.sin(ph)], axis=1)
    d[:6] = [(0, 1, 0), (0, -1, 0), (-1, 0, 0), (-1, 0, 1e-6), (-1, 0, -1e-6), (1, 0, 0)]   # both poles, the atan2 seam from either side
    out["sphere"] = (make_shape(A, A.SHAPE_SPHERE, [(1.0, 2.0, 3.0)], radius=0.75), np.array([1.0, 2.0, 3.0]) + 0.75 * d)
    return {k: (sh, p.astype(f32)) for k, (sh, p) in out.items()}


def probe_scene(A, api, shape):
    box = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    scene, _ = X.copy_scene(A, box.c)
    shapes, mats, lights, surfaces = scene._keep
    shapes.append(shape)
    mats.append(make_material(A, A.MATERIAL_MATTE, (0.5, 0.5, 0.5)))
    surfaces.append(A.Surface(len(shapes) - 1, len(mats) - 1, -1))
    from helpers import CustomScene
    return CustomScene(A, A.Camera.from_buffer_copy(box.c.camera), shapes, mats, lights, surfaces), len(surfaces) - 1, len(mats) - 1


# Largest |device - float64 restatement| over every shape kind, filter and wrap, against the largest |float32 restatement - float64 restatement|, which is what
# single precision costs; the device may differ from the float64 restatement by 4 x the latter.  Measured on one MI355X (u', v' in units of u', colours in units
# of the film's white):
UV_MEASURED, UV_REFERENCE = 1.47e-6, 1.47e-6           # (the sphere: u' = 5 u - ... through atan2; the planar kinds 4.9e-7 ... 9.5e-7)
COLOUR_MEASURED, COLOUR_REFERENCE = 8.93e-7, 8.93e-7   # (the device IS the float32 restatement on every one of the 5 x 5 x 4096 rows measured)
UV_CEILING, COLOUR_CEILING = 4 * UV_REFERENCE, 4 * COLOUR_REFERENCE


@pytest.mark.parametrize("name", ("rectangle", "quad", "triangle", "disk", "sphere"))
def test_the_probe_is_the_restatement(A, api, lib, name):
    shape, pts = probe_shapes(A)[name]
    scene, surface, material = probe_scene(A, api, shape)
    xs = X.Shape.of(shape)
    img = smooth_image()
    cases = [X.Tex(X.CHECKER, material, scale=(5, 3), offset=(0.37, -1.21), a=(0.9, 0.8, 0.1), b=(0.1, 0.2, 0.7))]
    for flags in (0, X.CLAMP, X.BILINEAR, X.BILINEAR | X.CLAMP):
        cases.append(X.Tex(X.IMAGE, material, flags, scale=(2.5, -1.75), offset=(-0.43, 0.61), texels=img))
    worst_uv = ref_uv = worst_c = ref_c = 0.0
    for tex in cases:
        got = api.kat_texture(scene, api_textures(api, [tex]), surface, pts)
        r32, r64 = X.probe(xs, tex, pts, f32), X.probe(xs, tex, pts, f64)
        assert got.dtype == f32 and np.isfinite(got).all()
        seam = np.abs(r32[:, 0].astype(f64) - r64[:, 0]) > 0.5 * abs(float(tex.scale[0]))   # the atan2 seam: u = 0 and u = 1 are one meridian
        e_uv = np.abs(got[:, :2].astype(f64) - r64[:, :2])
        e_ref = np.abs(r32[:, :2].astype(f64) - r64[:, :2])
        on_seam = seam | (e_uv[:, 0] > 0.5 * abs(float(tex.scale[0])))
        assert on_seam.sum() <= 4 and (name == "sphere" or on_seam.sum() == 0)
        worst_uv, ref_uv = max(worst_uv, e_uv[~on_seam].max()), max(ref_uv, e_ref[~on_seam].max())
        if tex.kind == X.IMAGE and tex.flags & X.BILINEAR:
            keep = ~on_seam
            worst_c = max(worst_c, np.abs(got[keep, 2:].astype(f64) - r64[keep, 2:]).max())
            ref_c = max(ref_c, np.abs(r32[keep, 2:].astype(f64) - r64[keep, 2:]).max())
        else:   # a checker or a nearest look-up: away from the cell and texel edges the colour is exact
            away = (X.edge_distance(tex, r64[:, 0], r64[:, 1]) >= 1e-4) & ~on_seam
            assert (~away).sum() <= 0.01 * len(pts), ((~away).sum(), name)   # (a property of the inputs)
            assert np.array_equal(got[away, 2:], r64[away, 2:].astype(f32)), (name, tex.kind, tex.flags)
    print("%s: u', v' device %.3g, float32 restatement %.3g; bilinear colours device %.3g, float32 restatement %.3g" % (name, worst_uv, ref_uv, worst_c, ref_c))
    assert worst_uv <= 4 * ref_uv and worst_uv <= UV_CEILING       # four times what single precision costs on these very rows, and no more than the recorded ceiling
    assert worst_c <= 4 * ref_c and worst_c <= COLOUR_CEILING


def test_the_probe_on_a_plastic_material_is_the_lobes_albedo(A, api, lib):
    scene, textures = X.cornell_case(A, api, 16, 16)
    floor = textures[0]
    m = scene.scene.materials[floor.material]
    assert m.kind == A.MATERIAL_PLASTIC
    pts = np.array([(-1.0, -1.0, -1.28), (-0.3, -1.0, -1.28)], f32)
    got = api.kat_texture(scene, api_textures(api, textures), 3, pts)
    want = X.probe(X.Shape.of(scene.scene.shapes[scene.scene.surfaces[3].shape]), floor, pts, f32)
    assert np.array_equal(got[:, 2:], (want[:, 2:] / f32(m.diffuse_probability)).astype(f32)) and not np.array_equal(got[0, 2:], got[1, 2:])


# ---- 2. paths equal the oracle on the tiled scene ----

_oracle_cache = {}


def oracle_samples(O, A, api, name, w, h, n_spp, sampler, integrator, composed):
    """(scene, textures, params, filter, lens, [h, w, N, 3] the oracle's samples on the tiled scene), computed once per case and shared"""
    key = (name, w, h, n_spp, sampler, integrator, composed)
    if key not in _oracle_cache:
        scene, textures = case_of(A, api, name, w, h)
        params = TF.params_of(api, A, w, h, n_spp, sampler, integrator=integrator)
        tiled = X.tiled(A, scene.scene, textures)
        stride = 256 if name == "veach" else 64
        if composed:
            f, flt = TF.both(api, TF.TENT2)
            lens, radius, focus = TL.lens_of(O, A, api, name, w, h)
            want = TL.oracle_samples(O, A, api, tiled, ("textured",) + key, params, stride, sampler, flt, radius, focus)
        else:
            f = lens = None
            want = np.zeros((h, w, n_spp, 3), f32)
            for y in range(h):
                for x in range(w):
                    want[y, x], _ = O.li_tape(tiled, params, x, y, F.tape(params.seed, y * w + x, n_spp, stride, TF.sampler_kind(A, sampler), None))
            want.setflags(write=False)
        _oracle_cache[key] = (scene, textures, params, f, lens, want)
    return _oracle_cache[key]


@pytest.mark.parametrize("form", ("both_mis", "basecolor", "tent2+lens"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("name", ("cornell", "veach"))
def test_paths_equal_the_oracle_on_the_tiled_scene(O, A, api, lib, name, n_spp, sampler, form):
    """kyhip_kat_li_textured against kyo_li_tape on tiled(...), every sample of every pixel, under tests/test_filter_gpu.py's caps as they stand (Cornell 32 x 32:
    0.2 % of samples, sums to 1e-4; Veach 48 x 27: 1.4 %, 5e-3).  tests/test_texture.py shows two tilings of one checker agreeing to half of that."""
    w, h, bad_share, sum_tol = TF.CAPS[name]
    assert (name, w, h) in (("cornell", 32, 32), ("veach", 48, 27))
    integrator = A.INTEGRATOR_BASECOLOR if form == "basecolor" else A.INTEGRATOR_PATH_TRACING_ITERATION
    scene, textures, params, f, lens, want = oracle_samples(O, A, api, name, w, h, n_spp, sampler, integrator, form == "tent2+lens")
    tx = api_textures(api, textures)
    bad = tot = 0
    sg = sc = 0.0
    for y in range(h):
        for x in range(w):
            g, c = api.kat_li(scene, params, x, y, 0, n_spp, filter=f, lens=lens, textures=tx), want[y, x]
            fin = np.isfinite(c).all(1)
            d = np.abs(g[fin] - c[fin]).max(axis=1)
            s = np.maximum(1e-3, np.abs(c[fin]).max(axis=1))
            bad += int((d / s > 1e-3).sum())
            tot += int(fin.sum())
            sg += float(np.minimum(g[fin], 10).sum())
            sc += float(np.minimum(c[fin], 10).sum())
    print("%s N = %d, %s, %s: %d of %d samples differ (cap %.0f), sums %.6g / %.6g" % (name, n_spp, sampler, form, bad, tot, bad_share * tot, sg, sc))
    assert bad <= bad_share * tot, (bad, tot)
    assert abs(sg - sc) <= sum_tol * max(sc, 1.0)


# ---- 3. the film is the mean of the oracle's samples ----

@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16, 17))
@pytest.mark.parametrize("size", (16, 32))
def test_film_is_the_mean_of_the_oracles_samples(O, A, api, lib, size, n_spp, sampler):
    scene, textures, params, _, _, want = oracle_samples(O, A, api, "cornell", size, size, n_spp, sampler, A.INTEGRATOR_PATH_TRACING_ITERATION, False)
    g, c = api.render(scene, params, textures=api_textures(api, textures)), T.film_of(want)
    kernel = lib.kyhip_last_kernel(0).decode()
    assert ", textured>" in kernel and "3 textures" in kernel and "strategy -1" in kernel and "run-time instantiation" not in kernel, kernel
    fin = np.isfinite(c).all(axis=2)
    assert (~fin).sum() <= 2 and np.isfinite(g).all() and g.min() >= 0 and g.max() <= 1
    e = rmse(g[fin], c[fin])
    print("cornell %d x %d, N = %d, %s: rmse %.3g, allowed %.3g" % (size, size, n_spp, sampler, e, T.film_tolerance(n_spp)))
    assert e < T.film_tolerance(n_spp)


# ---- 4. a checker with a == b is the constant; no textures is the untextured entry ----

@pytest.mark.parametrize("sampler", SAMPLERS)
def test_a_checker_of_one_colour_is_the_constant(A, api, lib, sampler):
    w = h = 32
    n_spp = 16
    scene, textures = X.cornell_case(A, api, w, h)
    p = TF.params_of(api, A, w, h, n_spp, sampler)
    flat = []
    for t in textures:
        c0 = [scene.scene.materials[t.material].color0[j] for j in range(3)]
        flat.append(X.Tex(X.CHECKER, t.material, scale=(4, 4), a=c0, b=c0))
    plain = api.render(scene, p)
    assert b"textured" not in lib.kyhip_last_kernel(0)
    g = api.render(scene, p, textures=api_textures(api, flat))
    assert b", textured>" in lib.kyhip_last_kernel(0)
    e = rmse(g, plain)
    print("%s: a == b == color0 against the untextured render: rmse %.3g, allowed %.3g" % (sampler, e, T.film_tolerance(n_spp)))
    assert e < T.film_tolerance(n_spp)   # (not bit for bit: the rows differ in which multiply-adds the compiler fuses)
    assert rmse(api.render(scene, p, textures=api_textures(api, textures)), plain) > 10 * T.film_tolerance(n_spp)   # ... and a real texture is seen


def test_no_textures_is_the_untextured_entry_bit_for_bit(O, A, api, lib):
    w = h = 16
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    p = TF.params_of(api, A, w, h, 16, "random")
    tent, lens = api.pixel_filter(A.FILTER_TENT, 2.0), TL.lens_of(O, A, api, "cornell", w, h)[0]
    for flt, ln in ((None, None), (tent, None), (tent, lens), (None, lens)):
        want = api.render(scene, p, filter=flt, lens=ln)
        name = lib.kyhip_last_kernel(0)
        film = np.zeros((h, w, 3), f32)
        rc = lib.kyhip_render_textured(0, api._scene_ptr(scene), None, 0, C.byref(p), C.byref(flt) if flt is not None else None, C.byref(ln) if ln is not None else None,
                                       film.ctypes.data_as(C.c_void_p), w)
        assert rc == A.KY_OK and np.array_equal(film, want) and lib.kyhip_last_kernel(0) == name and b"textured" not in name
    assert np.array_equal(api.kat_li(scene, p, 5, 6, 0, 8, textures=[]), api.kat_li(scene, p, 5, 6, 0, 8))
    dbg = api.make_params(w, h, 4, sampler=A.SAMPLER_DEBUG)   # no textured row for the debug sampler
    with pytest.raises(api.KyError):
        api.render(scene, dbg, textures=[api.texture_checker(1, (1, 1, 1), (0, 0, 0))])


# ---- 5. every cut of a textured frame is the one-shot film ----

@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("size", ((16, 16), (40, 24)), ids=("16x16", "40x24"))
def test_every_cut_of_a_textured_frame_is_the_one_shot_film(A, api, lib, size, sampler):
    """N = 17 (pass boundaries at 4 and 12), at 16 x 16 and at 40 x 24 (ragged 16 x 16 tiles)."""
    w, h = size
    n_spp = 17
    scene, textures = X.cornell_case(A, api, w, h)
    tx = api_textures(api, textures)
    p = TF.params_of(api, A, w, h, n_spp, sampler)
    whole = api.render(scene, p, textures=tx)
    assert whole.max() > 0.1 and not np.array_equal(whole, api.render(scene, p))
    bounds = api.pass_boundaries(n_spp)

    def in_passes(wants, **kw):
        with api.Frame(scene, p, textures=tx, **kw) as f:
            live = f.block_stats().live if kw.get("blocks") else 0
            for want in wants:
                if f.done < f.total:
                    f.render(want)
            assert f.done == n_spp
            if kw.get("blocks"):
                assert b"listed blocks" in lib.kyhip_last_kernel(0) and b", textured>" in lib.kyhip_last_kernel(0), lib.kyhip_last_kernel(0)
                assert f.block_stats().live == live > 0   # nothing retired
            return f.resolve()

    assert np.array_equal(in_passes((4, 8, n_spp)), whole)                 # passes of unequal length
    assert np.array_equal(in_passes((1, n_spp)), whole)
    assert np.array_equal(in_passes((4, 8, n_spp), noise=True), whole)     # ... while tracking noise
    assert np.array_equal(in_passes((4, 8, n_spp), blocks=True), whole)    # ... while tracking blocks, nothing retired (the listed rows)
    with api.Frame(scene, p, textures=tx) as f:                            # saved and resumed mid-frame
        f.render(1)
        state = f.save()
    with api.Frame(scene, p, textures=tx) as f:
        f.load(state)
        assert f.done == bounds[0]
        f.render(n_spp)
        assert np.array_equal(f.resolve(), whole)
    sb = api.slice_bounds(n_spp, 2)                                        # two slices merged in either order
    for order in ((0, 1), (1, 0)):
        frames = [api.Frame(scene, p, textures=tx, slice=(sb[k], sb[k + 1])) for k in range(2)]
        try:
            for f in frames:
                f.render(n_spp)
            with api.Frame(scene, p, textures=tx, slice=(0, 0)) as collector:
                for k in order:
                    collector.merge(frames[k])
                assert collector.done == n_spp and np.array_equal(collector.resolve(), whole), order
            frames[order[0]].merge(frames[order[1]].save())   # ... and into a slice itself, from a saved state
            assert np.array_equal(frames[order[0]].resolve(), whole)
        finally:
            for f in frames:
                f.close()
    assert np.array_equal(api.render_sliced(scene, p, [0, 0], 4, textures=tx), whole)


# ---- 6. identity ----

def test_textures_are_part_of_a_frames_identity(A, api, lib):
    w = h = 16
    scene, textures = X.cornell_case(A, api, w, h)
    p = TF.params_of(api, A, w, h, 17, "random")
    texel = [X.Tex(t.kind, t.material, t.flags, t.scale, t.offset, t.a, t.b, t.texels) for t in textures]
    texel[1].texels = texel[1].texels.copy()
    texel[1].texels[2, 1, 0] += f32(2.0 ** -20)                      # one texel, by a few units in its last place
    field = [X.Tex(t.kind, t.material, t.flags, t.scale, t.offset, t.a, t.b, t.texels) for t in textures]
    field[0].offset = np.array([0.0, 2.0 ** -20], f32)               # one descriptor field
    sets = {"set": api_textures(api, textures), "one texel": api_textures(api, texel), "one field": api_textures(api, field), "none": None}
    sb = api.slice_bounds(17, 2)
    states, slices = {}, {}
    for name, tx in sets.items():
        with api.Frame(scene, p, textures=tx) as f:
            f.render(1)
            states[name] = f.save()
        with api.Frame(scene, p, textures=tx, slice=(sb[1], sb[2])) as f:
            f.render(17)
            slices[name] = f.save()
    assert len({len(s) for s in states.values()}) == 1   # the checkpoint's layout and size do not change
    for mine, tx in sets.items():
        for theirs in sets:
            with api.Frame(scene, p, textures=tx) as f, api.Frame(scene, p, textures=tx, slice=(sb[0], sb[1])) as g:
                if mine == theirs:
                    f.load(states[theirs])
                    g.merge(slices[theirs])
                    assert f.done == api.pass_boundaries(17)[0] and g.done == 17 - sb[1]   # the state's one pass; the merged slice's samples, exactly
                else:
                    with pytest.raises(api.KyError):
                        f.load(states[theirs])
                    with pytest.raises(api.KyError):
                        g.merge(slices[theirs])
                    assert f.done == 0 and g.done == 0
    with api.Frame(scene, p, textures=sets["set"]) as f:   # after a pass the set stays
        f.render(1)
        with pytest.raises(api.KyError, match="holds samples"):
            f.set_textures(sets["one texel"])
        with pytest.raises(api.KyError, match="holds samples"):
            f.set_textures([])


# ---- 7. one frame per textured row ----

def row_scene(A, api, which, w, h):
    """-> (scene, [Tex], stride, what kyhip_last_kernel must name)"""
    from helpers import CustomScene
    if which == "shipped":
        scene, textures = X.cornell_case(A, api, w, h)
        return scene, textures, 64, "strategy -1, feat 0,"
    if which == "general":   # the Cornell box and one matte triangle: a shape the general kernels test inline
        scene, textures = X.cornell_case(A, api, w, h)
        shapes, mats, lights, surfaces = scene._keep
        shapes.append(make_shape(A, A.SHAPE_TRIANGLE, [(-0.9, 0.2, -1.0), (0.9, 0.2, -1.0), (0.0, 0.2, 0.6)]))
        mats.append(make_material(A, A.MATERIAL_MATTE, (0.7, 0.6, 0.2)))
        surfaces.append(A.Surface(len(shapes) - 1, len(mats) - 1, -1))
        return CustomScene(A, scene.scene.camera, shapes, mats, lights, surfaces), textures, 128, "strategy -1, general shapes, feat 0,"
    base = T.large_scene(A, api, w, h)   # more than 64 surfaces; a 4 x 4 checker on the wall the camera faces: 77 + 15 surfaces once tiled
    scene, idx = X.copy_scene(A, base.scene, {4: None})
    scene._keep_base = base
    return scene, [X.Tex(X.CHECKER, idx[4], scale=(4, 4), a=(0.8, 0.7, 0.2), b=(0.1, 0.2, 0.6))], 128, "strategy -1, general shapes, scene-sized LDS block"


@pytest.mark.parametrize("listed", (False, True), ids=("plain", "listed"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("which", ("shipped", "general", "large"))
def test_one_frame_per_textured_row(O, A, api, lib, which, sampler, listed):
    w = h = 16
    n_spp = 5
    scene, textures, stride, name = row_scene(A, api, which, w, h)
    tx = api_textures(api, textures)
    params = TF.params_of(api, A, w, h, n_spp, sampler)
    if listed:
        with api.Frame(scene, params, textures=tx, blocks=True) as f:
            f.render(n_spp)
            g = f.resolve()
    else:
        g = api.render(scene, params, textures=tx)
    kernel = lib.kyhip_last_kernel(0).decode()
    print(which, sampler, listed, "->", kernel)
    assert name in kernel and ", textured>" in kernel and ("listed blocks" in kernel) == listed and ("stratified sampler" in kernel) == (sampler == "stratified"), kernel
    tiled = X.tiled(A, scene.scene, textures)
    assert tiled.scene.surface_count <= 256
    samples = np.zeros((h, w, n_spp, 3), f32)
    for y in range(h):
        for x in range(w):
            samples[y, x], _ = O.li_tape(tiled, params, x, y, F.tape(params.seed, y * w + x, n_spp, stride, TF.sampler_kind(A, sampler), None))
    c = T.film_of(samples)
    fin = np.isfinite(c).all(axis=2)
    e = rmse(g[fin], c[fin])
    print("%s: rmse %.3g, allowed %.3g" % (which, e, T.film_tolerance(n_spp)))
    assert g.max() > 0 and (~fin).sum() <= 2 and e < T.film_tolerance(n_spp)


# ---- 8. the queue engine ----

def test_queue_engine_runs_the_lane_engine_and_says_so(A, api, lib):
    scene, textures = X.cornell_case(A, api, 16, 16)
    tx = api_textures(api, textures)
    p = TF.params_of(api, A, 16, 16, 5, "random")
    want = api.render(scene, p, textures=tx)
    prev = lib.kyhip_set_engine(1)
    try:
        got = api.render(scene, p, textures=tx)
        name = lib.kyhip_last_kernel(0).decode()
    finally:
        lib.kyhip_set_engine(prev)
    assert np.array_equal(got, want) and ", textured>" in name and "the queue engine has no textures" in name, name


# ---- 9. the host mirror and the driver ----

def driver_scene(A, api, w, h):
    """The scene `ky_drivers textured` builds, through the same host classes: the Cornell box with a 4 x 4 checker on the floor's material (plastic: its lobe
    probabilities are those of the checker's first colour) and an 8 x 8 image (red rises with x, green with y, in sixteenths) twice each way on the wall's."""
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    floor, wall = scene.c.surfaces[3].material, scene.c.surfaces[4].material
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    img = np.stack([(2 * x + 1) / 16.0, (2 * y + 1) / 16.0, np.full((8, 8), 0.25)], axis=2).astype(f32)
    scene.texture_checker(floor, (0.25, 0.25, 0.0625), (0.03125, 0.0625, 0.25), scale=(4, 4))
    scene.texture_image(wall, img, scale=(2, 2))
    return scene


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_the_host_mirror_renders_what_the_c_call_renders(A, api, lib, sampler):
    """texture_t materials through ky.hpp's integrator_t::render, render_passes and render_sliced against api.render(textures=) of the flattened set, bit for bit"""
    w = h = 32
    n_spp = 17
    scene = driver_scene(A, api, w, h)
    tx = scene.textures()
    assert len(tx) == 2 and [t.kind for t in tx] == [A.TEXTURE_IMAGE, A.TEXTURE_CHECKER]   # material order: the wall's material 4, the floor's 5
    p = TF.params_of(api, A, w, h, n_spp, sampler)
    want = api.render(scene, p, textures=tx)
    assert b", textured>" in lib.kyhip_last_kernel(0) and want.max() > 0.1
    got = api.render_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, TF.sampler_kind(A, sampler), n_spp, w, h)
    assert b", textured>" in lib.kyhip_last_kernel(0)
    assert np.array_equal(got, want)
    tent = api.pixel_filter(A.FILTER_TENT, 2.0)   # ... and in passes and in slices, under the film's filter
    want_f = api.render(scene, p, textures=tx, filter=tent)
    for mode in ("render", "passes", "sliced"):
        got = api.render_filtered_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, TF.sampler_kind(A, sampler), n_spp, w, h, tent, mode=mode)
        assert np.array_equal(got, want_f), mode


def test_the_textured_driver_writes_the_film_of_the_c_call(A, api, lib, tmp_path):
    """examples/ky_drivers.cpp `textured`: its BMP equals, byte for byte, the picture of api.render(textures=) of the same set through the numpy restatement of the writer"""
    import os
    import subprocess
    from oracle import film_writers as FW
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "bin", "ky_drivers")
    assert os.path.exists(exe), "examples/bin/ky_drivers is built by build()"
    out = subprocess.run([exe, "textured", "16", "64"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and ", textured>" in out.stdout, (out.stdout, out.stderr)
    scene = driver_scene(A, api, 64, 64)
    film = api.render(scene, api.make_params(64, 64, 16), textures=scene.textures())
    assert open(tmp_path / "textured.bmp", "rb").read() == FW.bmp_bytes(film)
