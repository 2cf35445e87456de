"""GPU: textures (ky_texture) where tests/test_texture_gpu.py does not look.  (B) The render kernels' look-up on every shape kind: the
first hit of every camera sample of X.shapes_case -- a sphere, a triangle, a disk, a quad that is no parallelogram, a face of the room's box, one material shared
by two kinds, the caller's surface order interleaved -- against the oracle's own first hit coloured by the float64 restatement, with a constant-colour control
run that sets the tolerance.  (C) Whole paths on those shapes under textures that show one colour over a whole surface, which the oracle can hold.  (D) Image
shapes that are not square, a full 16-texture set and edge coordinates through the probe.  (E) The other lighting strategies on the textured rows.
tests/test_texture.py holds the CPU side: the inputs' properties, the pins and the named defects."""
import ctypes as C

import numpy as np
import pytest

import filter_restatement as F
import test_filter_gpu as TF      # CAPS, params_of, sampler_kind
import test_stratified_gpu as T   # film_tolerance, film_of
import test_texture as TC         # shapes_expected (shared with the CPU tests)
import test_texture_gpu as TG     # probe_shapes, probe_scene, api_textures, the recorded probe ceilings
import texture_restatement as X
from helpers import CustomScene, make_material, make_shape, rmse

pytestmark = pytest.mark.gpu

SAMPLERS = ("random", "stratified")
f32, f64 = np.float32, np.float64
api_textures = TG.api_textures


@pytest.fixture(scope="module")
def lib(A):
    lib = A.load_kyhip()
    prev = lib.kyhip_set_jit(0)
    yield lib
    lib.kyhip_set_jit(prev)


def device_samples(api, scene, params, tx, w, h, n, **kw):
    out = np.zeros((h, w, n, 3), f32)
    for y in range(h):
        for x in range(w):
            out[y, x] = api.kat_li(scene, params, x, y, 0, n, textures=tx, **kw)
    return out


def rel(g, e):
    """tests/test_stratified_gpu.py's measure of one sample: the largest channel difference over the larger of the expected sample's largest channel and 1e-3"""
    return np.abs(g.astype(f64) - e).max(axis=-1) / np.maximum(1e-3, np.abs(e).max(axis=-1))


# ---- B. the first hit on every shape kind ----

# Measured on one MI355X, both scenes, N = 5 and 16, both samplers.  The control run -- every texture a checker with a == b, GPU basecolor against the oracle on
# constant colours -- : no sample differs, the largest relative difference of a sample on a textured surface is R0 (one rounding of colour / pi), the largest
# per-pixel film error CONTROL_PIXEL.  Textured: a clean checker or nearest sample is off by at most 4.01e-08 as well, i.e. it is the control's rounding and the
# right texel; the bilinear samples (the disk) by at most 1.63e-06 of the colour's unit where the float32 restatement's own distance from the float64 one on the
# same rows is 2.46e-07 ... 5.07e-07 (BILINEAR_REFERENCE, the largest); at most 1 bilinear sample of a frame is further off than 4 x its frame's figure.
R0_MEASURED = 4.01e-08
BILINEAR_REFERENCE = 5.07e-07
CONTROL_PIXEL_MEASURED = 2.98e-08
SAMPLE_CEILING, BILINEAR_CEILING, PIXEL_CEILING = 4 * max(R0_MEASURED, 2.0 ** -23), 4 * BILINEAR_REFERENCE, 2 * CONTROL_PIXEL_MEASURED


def control_expected(scene, E, flat):
    """the expected samples of the control set `flat` on E's first hits: k x the texture's one colour"""
    c = scene.scene
    by_material = {t.material: t for t in flat}
    colour = np.ones((len(E.surface), 3), f64)
    for s in range(c.surface_count):
        t = by_material.get(c.surfaces[s].material)
        if t is not None:
            colour[E.surface == s] = t.a.astype(f64)
    return E.k.astype(f64) * colour


def compare_first_hits(api, scene, textures, params, E, what):
    """-> (differing samples, total, r0, worst clean checker / nearest sample, worst bilinear sample in units of 4 e_ref k) after the assertions of section B"""
    h, w, n = E.shape
    flat = X.flat_textures(textures)
    ctrl = device_samples(api, scene, params, api_textures(api, flat), w, h, n).reshape(-1, 3)
    got = device_samples(api, scene, params, api_textures(api, textures), w, h, n).reshape(-1, 3)
    assert np.isfinite(got).all() and np.isfinite(ctrl).all()
    on = E.textured
    r_ctrl = rel(ctrl, control_expected(scene, E, flat))
    ctrl_bad = r_ctrl > 1e-3
    r0 = float(r_ctrl[on & ~ctrl_bad].max())
    tol = 4 * max(r0, 2.0 ** -23)
    r = rel(got, E.expected)
    plain = on & E.clean & ~E.bilinear
    bad_plain = plain & (r > tol)
    d_bil = np.abs(got.astype(f64) - E.expected).max(axis=1) / np.maximum(E.k.max(axis=1).astype(f64), 1e-30)   # in units of the texture's colour
    bil = on & E.clean & E.bilinear
    bad_bil = bil & (d_bil > 4 * E.e_ref)
    bad_off = ~on & (r > 1e-3)
    bad = int(bad_plain.sum() + bad_bil.sum() + bad_off.sum())
    worst_plain = float(r[plain & ~bad_plain].max())
    worst_bil = float(d_bil[bil & ~bad_bil].max()) if (bil & ~bad_bil).any() else 0.0
    print("%s: control: %d of %d samples differ, r0 %.3g; textured: %d differ (%d checker / nearest, %d bilinear, %d untextured; cap %.0f), worst clean sample %.3g (allowed %.3g), "
          "worst bilinear %.3g (allowed %.3g = 4 x %.3g), %d unclean left out"
          % (what, ctrl_bad.sum(), len(r), r0, bad, bad_plain.sum(), bad_bil.sum(), bad_off.sum(), 0.002 * len(r), worst_plain, tol, worst_bil, 4 * E.e_ref, E.e_ref, (on & ~E.clean).sum()))
    assert ctrl_bad.sum() <= 0.002 * len(r)                 # the control itself: silhouette decisions, GPU against oracle
    assert bad <= 0.002 * len(r), (bad_plain.sum(), bad_bil.sum(), bad_off.sum())
    return r0, worst_plain, worst_bil


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("which", ("general", "shipped"))
def test_first_hits_equal_the_oracles_first_hit_under_the_restatement(O, A, api, lib, which, n_spp, sampler):
    """kyhip_kat_li_textured under basecolor, every sample of every pixel at 32 x 32, against k x the float64 restatement's colour at the oracle's first hit
    (X.expected_samples).  A clean checker or nearest sample may differ by 4 max(r0, 2^-23) relative, r0 the control run's largest relative difference; a
    bilinear sample (the disk's; X.shapes_case says why not a ball's) by 4 x the float32 restatement's own distance from the float64 one on the same rows; at most
    0.2 % of all samples may differ, in the control and here (TF.CAPS["cornell"]: silhouette decisions).  Unclean samples -- within 1e-4 of a cell or texel edge or
    on a sphere's seam, at most 2 % of those on textured surfaces (tests/test_texture.py) -- are left out."""
    assert TF.CAPS["cornell"][:3] == (32, 32, 0.002)
    scene, textures, names, params, E = TC.shapes_expected(O, A, api, which, n_spp, sampler)
    r0, worst, worst_bil = compare_first_hits(api, scene, textures, params, E, "%s N = %d, %s" % (which, n_spp, sampler))
    assert worst <= SAMPLE_CEILING and worst_bil <= BILINEAR_CEILING   # ... and no more than the recorded ceilings


@pytest.mark.parametrize("listed", (False, True), ids=("plain", "listed"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("which", ("shipped", "general", "large"))
def test_films_of_the_shapes_cases(O, A, api, lib, which, n_spp, sampler, listed):
    """api.render(textures=) under basecolor on each textured row against the mean of the expected samples: RMSE below T.film_tolerance; and every pixel all of
    whose samples are clean within 2 x the control render's largest per-pixel error (plus, where a pixel holds bilinear samples, 4 x the restatement's float32
    cost).  Pixels in which the CONTROL is off by more than 1e-4 hold a silhouette decision and are left to the RMSE; there are at most 0.2 % x N of them."""
    scene, textures, names, params, E = TC.shapes_expected(O, A, api, which, n_spp, sampler)
    h, w, n = E.shape
    flat = X.flat_textures(textures)

    def film(tx):
        if listed:
            with api.Frame(scene, params, textures=tx, blocks=True) as f:
                f.render(n)
                return f.resolve()
        return api.render(scene, params, textures=tx)
    ctrl = film(api_textures(api, flat))
    g = film(api_textures(api, textures))
    kernel = lib.kyhip_last_kernel(0).decode()
    want = {"shipped": "strategy -1, feat 0,", "general": "strategy -1, general shapes, feat 0,", "large": "strategy -1, general shapes, scene-sized LDS block"}[which]
    assert want in kernel and ", textured>" in kernel and ("listed blocks" in kernel) == listed and ("stratified sampler" in kernel) == (sampler == "stratified"), kernel
    c = T.film_of(E.expected.reshape(h, w, n, 3))
    c_ctrl = T.film_of(control_expected(scene, E, flat).reshape(h, w, n, 3))
    e = rmse(g, c)
    err, err_ctrl = np.abs(g.astype(f64) - c).max(axis=2), np.abs(ctrl.astype(f64) - c_ctrl).max(axis=2)
    silhouette = err_ctrl > 1e-4
    clean = E.clean.reshape(h, w, n).all(axis=2) & ~silhouette
    bil = E.bilinear.reshape(h, w, n).any(axis=2)
    worst_ctrl = float(err_ctrl[~silhouette].max())
    allowed = 2 * worst_ctrl + np.where(bil, 4 * E.e_ref * float(E.k.max()), 0.0)
    print("%s N = %d, %s, %s: rmse %.3g (allowed %.3g); %d silhouette pixels; control's worst pixel %.3g, worst clean pixel %.3g without / %.3g with bilinear samples (allowed %.3g / %.3g)"
          % (which, n_spp, sampler, "listed" if listed else "plain", e, T.film_tolerance(n_spp), silhouette.sum(), worst_ctrl, err[clean & ~bil].max(),
             err[clean & bil].max() if (clean & bil).any() else 0.0, 2 * worst_ctrl, allowed.max()))
    assert g.max() > 0.1 and e < T.film_tolerance(n_spp)
    assert silhouette.sum() <= 0.002 * n * w * h
    assert (err[clean] <= allowed[clean]).all(), (err[clean] - allowed[clean]).max()
    assert err[clean & ~bil].max() <= PIXEL_CEILING   # ... and no more than the recorded ceiling


# ---- C. whole paths on non-rectangles: textures that show one colour over a whole surface ----

COLOUR_A, COLOUR_B, THIRD = (0.75, 0.5, 0.125), (0.125, 0.375, 0.75), (0.5, 0.0625, 0.5)


def one_colour_case(A, api, w, h, variant):
    """X.shapes_case's scene with the second ball on a PLASTIC material of its own and, on the ball, the triangle, the disk and the second ball, four textures that
    show one colour over the whole surface ((u, v) lies in [0, 1]^2): a checker of scale 0.5 (colour a), the same with offset (1, 0) (colour b), a 2 x 1 nearest
    clamped image with scale[0] = 0.5 and offset 0 (texel 0) or 0.5 (texel 1); `variant` rotates which surface takes which.  Every struct's color0 is THIRD.
    -> (scene, [Tex], the scene whose color0 is the colour the texture shows, the scene as the structs have it)"""
    scene, _, names = X.shapes_case(A, api, w, h)
    c = scene.scene
    shapes, mats, lights, surfaces = scene._keep
    surfaces = [A.Surface.from_buffer_copy(c.surfaces[i]) for i in range(c.surface_count)]
    mats = [A.Material.from_buffer_copy(c.materials[i]) for i in range(c.material_count)]
    mats.append(make_material(A, A.MATERIAL_PLASTIC, THIRD, (0.5, 0.5, 0.5), exponent=40.0))
    surfaces[names["ball2"]].material = len(mats) - 1
    image = np.array([[COLOUR_A, COLOUR_B]], f32)
    forms = [lambda m: (X.Tex(X.CHECKER, m, scale=(0.5, 0.5), a=COLOUR_A, b=COLOUR_B), COLOUR_A),
             lambda m: (X.Tex(X.CHECKER, m, scale=(0.5, 0.5), offset=(1, 0), a=COLOUR_A, b=COLOUR_B), COLOUR_B),
             lambda m: (X.Tex(X.IMAGE, m, X.CLAMP, scale=(0.5, 1), texels=image), COLOUR_A),
             lambda m: (X.Tex(X.IMAGE, m, X.CLAMP, scale=(0.5, 1), offset=(0.5, 0), texels=image), COLOUR_B)]
    textures, shown = [], {}
    for i, name in enumerate(("ball", "tri", "disk", "ball2")):
        m = surfaces[names[name]].material
        tex, colour = forms[(i + variant) % 4](m)
        textures.append(tex)
        shown[m] = colour
    struct_mats = [A.Material.from_buffer_copy(m) for m in mats]
    shown_mats = [A.Material.from_buffer_copy(m) for m in mats]
    for m, colour in shown.items():
        for j in range(3):
            struct_mats[m].color0[j] = THIRD[j]
            shown_mats[m].color0[j] = colour[j]     # (a plastic material keeps the probabilities of its struct colour)
    cam = A.Camera.from_buffer_copy(c.camera)
    return (CustomScene(A, cam, shapes, struct_mats, lights, surfaces), textures, CustomScene(A, cam, shapes, shown_mats, lights, surfaces), names)


def li_agreement(got, want):
    """tests/test_stratified_gpu.py's comparison of two sample arrays [..., 3] -> (differing, total, sum of got, sum of want)"""
    g, c = got.reshape(-1, 3), want.reshape(-1, 3)
    fin = np.isfinite(c).all(1)
    d = np.abs(g[fin] - c[fin]).max(axis=1)
    s = np.maximum(1e-3, np.abs(c[fin]).max(axis=1))
    return int((d / s > 1e-3).sum()), int(fin.sum()), float(np.minimum(g[fin], 10).sum()), float(np.minimum(c[fin], 10).sum())


def oracle_frame(O, A, scene, params, w, h, n, sampler, stride):
    out = np.zeros((h, w, n, 3), f32)
    for y in range(h):
        for x in range(w):
            out[y, x], _ = O.li_tape(scene, params, x, y, F.tape(params.seed, y * w + x, n, stride, TF.sampler_kind(A, sampler), None))
    return out


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("variant", (0, 1))
def test_whole_paths_on_non_rectangles_equal_the_oracle(O, A, api, lib, variant, n_spp, sampler):
    """kyhip_kat_li_textured under path tracing and both_mis, every sample at 32 x 32, against kyo_li_tape on the scene whose color0 is the colour the texture
    shows, under the Cornell caps as they stand; the structs hold a THIRD colour, and the oracle on that scene is outside the caps -- so the look-up is made at
    every depth that matters.  One of the surfaces is a plastic sphere: its struct colour fixes the lobe probabilities, the texture is its albedo."""
    w, h, bad_share, sum_tol = TF.CAPS["cornell"]
    scene, textures, shown, names = one_colour_case(A, api, w, h, variant)
    assert scene.scene.materials[scene.scene.surfaces[names["ball2"]].material].kind == A.MATERIAL_PLASTIC
    params = TF.params_of(api, A, w, h, n_spp, sampler)
    got = device_samples(api, scene, params, api_textures(api, textures), w, h, n_spp)
    bad, tot, sg, sc = li_agreement(got, oracle_frame(O, A, shown, params, w, h, n_spp, sampler, 128))
    bad3, _, _, sc3 = li_agreement(got, oracle_frame(O, A, scene, params, w, h, n_spp, sampler, 128))
    print("variant %d N = %d, %s: %d of %d samples differ (cap %.0f), sums %.6g / %.6g; against the structs' colour %d differ, sum %.6g"
          % (variant, n_spp, sampler, bad, tot, bad_share * tot, sg, sc, bad3, sc3))
    assert bad <= bad_share * tot and abs(sg - sc) <= sum_tol * max(sc, 1.0)
    assert bad3 > 10 * bad_share * tot and abs(sg - sc3) > 10 * sum_tol * max(sc3, 1.0)


# ---- D. image shapes, a full set and edge coordinates through the probe ----

IMAGE_SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (5, 3), (64, 2), (4096, 1), (1, 4096))   # (W, H)
# Largest |float32 restatement - float64 restatement| of a bilinear colour on these rows, measured on one MI355X, where the device IS the float32 restatement on
# every row (the same figures to three digits).  Texels reach (W + 1) / 8 and a texel is 1 / W of u' wide, so what float32 costs grows with W squared: it is
# the rounding of u' W - 0.5 times the texels' slope, not a defect.
SHAPES_COLOUR_MEASURED = {(1, 1): 0.0, (1, 7): 1.47e-06, (7, 1): 1.91e-06, (3, 5): 7.04e-07, (5, 3): 1.16e-06, (64, 2): 1.42e-04, (4096, 1): 0.108, (1, 4096): 0.169}


@pytest.mark.parametrize("size", IMAGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_probe_on_images_that_are_not_square(A, api, lib, size):
    """TG.test_the_probe_is_the_restatement's method on W x H images with asymmetric texels (X.texels_of), nearest and bilinear, repeating and clamped, on a
    rectangle and on a sphere: checker-like exactness for nearest >= 1e-4 from a texel edge, bilinear within 4 x what float32 costs on these rows."""
    W, H = size
    shapes = TG.probe_shapes(A)
    worst_c = ref_c = 0.0
    for name in ("rectangle", "sphere"):
        shape, pts = shapes[name]
        scene, surface, material = TG.probe_scene(A, api, shape)
        xs = X.Shape.of(shape)
        for flags in (0, X.CLAMP, X.BILINEAR, X.BILINEAR | X.CLAMP):
            tex = X.Tex(X.IMAGE, material, flags, scale=(2.5, -1.75), offset=(-0.43, 0.61), texels=X.texels_of(3, W, H))
            got = api.kat_texture(scene, api_textures(api, [tex]), surface, pts)
            r32, r64 = X.probe(xs, tex, pts, f32), X.probe(xs, tex, pts, f64)
            assert got.dtype == f32 and np.isfinite(got).all()
            on_seam = np.abs(got[:, 0].astype(f64) - r64[:, 0]) > 0.5 * abs(float(tex.scale[0]))
            assert on_seam.sum() <= 4 and (name == "sphere" or on_seam.sum() == 0)
            if flags & X.BILINEAR:
                keep = ~on_seam
                worst_c = max(worst_c, np.abs(got[keep, 2:].astype(f64) - r64[keep, 2:]).max())
                ref_c = max(ref_c, np.abs(r32[keep, 2:].astype(f64) - r64[keep, 2:]).max())
            else:
                away = (X.edge_distance(tex, r64[:, 0], r64[:, 1]) >= 1e-4) & ~on_seam
                # a property of the inputs: texel edges lie 1 / W apart in u' and the points' u' has density <= 2 |scale| (the sphere's v: pi / 2), so at
                # most this share is within 1e-4 of one -- most of the points on the 4096-texel axis, which are then simply not compared
                near = 2 * 2e-4 * (W * 2.5 + H * 1.75) + 0.01
                assert (~away).sum() <= near * len(pts) and away.sum() >= 300, ((~away).sum(), away.sum(), name)
                assert np.array_equal(got[away, 2:], r64[away, 2:].astype(f32)), (name, flags)
    print("%d x %d: bilinear colours device %.3g, float32 restatement %.3g" % (W, H, worst_c, ref_c))
    assert worst_c <= 4 * ref_c
    assert worst_c <= 4 * SHAPES_COLOUR_MEASURED[size]   # ... and no more than the recorded ceiling


def sixteen_case(A, api):
    """The Cornell box and 16 more surfaces -- rectangle, quad, triangle, disk, sphere in turn, TG.probe_shapes' -- each on a matte material of its own; texture i
    sits on material PERM[i] of those: a checker where i % 4 == 3, else a (5 + 11 i) x (3 + 9 i) image, nearest, bilinear or nearest clamped.  The images' first
    texels all differ and the last lies beyond 8192.  -> (scene, [Tex], [(surface, shape, points) of texture i])"""
    perm = [11, 2, 7, 14, 0, 9, 4, 13, 6, 1, 15, 8, 3, 12, 5, 10]
    kinds = ("rectangle", "quad", "triangle", "disk", "sphere")
    probe = TG.probe_shapes(A)
    box = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    scene, _ = X.copy_scene(A, box.c)
    shapes, mats, lights, surfaces = scene._keep
    m0, s0 = len(mats), len(surfaces)
    for j in range(16):
        shapes.append(probe[kinds[j % 5]][0])
        mats.append(make_material(A, A.MATERIAL_MATTE, (0.5, 0.5, 0.5)))
        surfaces.append(A.Surface(len(shapes) - 1, m0 + j, -1))
    scene = CustomScene(A, A.Camera.from_buffer_copy(box.c.camera), shapes, mats, lights, surfaces)
    textures, where = [], []
    for i in range(16):
        sc, off = (1.5 + 0.25 * i, -(1.25 + 0.125 * i)), (0.1 * i - 0.7, 0.3 - 0.05 * i)
        if i % 4 == 3:
            tex = X.Tex(X.CHECKER, m0 + perm[i], scale=sc, offset=off, a=((i + 1) / 32, 0.5, 0.25), b=(0.25, (i + 1) / 32, 0.75))
        else:
            tex = X.Tex(X.IMAGE, m0 + perm[i], (0, X.BILINEAR, X.CLAMP)[i % 4], scale=sc, offset=off, texels=X.texels_of(i, 5 + 11 * i, 3 + 9 * i))
        textures.append(tex)
        where.append((s0 + perm[i], probe[kinds[perm[i] % 5]][0], probe[kinds[perm[i] % 5]][1][:1024]))
    first = X.pack(textures)[1]
    assert len(set(first)) == 16 and first[-1] > 8192
    return scene, textures, where


SIXTEEN_COLOUR_MEASURED = 6.37e-04   # (the float32 restatement's distance from the float64 one, and the device's: the widest bilinear image here is 148 texels)


def test_a_full_set_of_sixteen_textures(A, api, lib):
    """One surface per texture through the probe against the restatement -- material order scrambled against texture order, every `first` different, the last
    beyond 8192 texels -- and the same textures as a set in another order: the same surface shows the same colours, bit for bit."""
    scene, textures, where = sixteen_case(A, api)
    tx = api_textures(api, textures)
    order = [5, 12, 0, 9, 15, 3, 7, 1, 14, 10, 2, 8, 13, 4, 11, 6]
    tx2 = api_textures(api, [textures[i] for i in order])
    worst_c = ref_c = 0.0
    for i, (surface, shape, pts) in enumerate(where):
        tex, xs = textures[i], X.Shape.of(shape)
        got = api.kat_texture(scene, tx, surface, pts)
        assert np.array_equal(api.kat_texture(scene, tx2, surface, pts), got), i
        r32, r64 = X.probe(xs, tex, pts, f32), X.probe(xs, tex, pts, f64)
        on_seam = np.abs(got[:, 0].astype(f64) - r64[:, 0]) > 0.5 * abs(float(tex.scale[0]))
        assert on_seam.sum() <= 4
        if tex.kind == X.IMAGE and tex.flags & X.BILINEAR:
            worst_c = max(worst_c, np.abs(got[~on_seam, 2:].astype(f64) - r64[~on_seam, 2:]).max())
            ref_c = max(ref_c, np.abs(r32[~on_seam, 2:].astype(f64) - r64[~on_seam, 2:]).max())
        else:
            away = (X.edge_distance(tex, r64[:, 0], r64[:, 1]) >= 1e-4) & ~on_seam
            assert away.sum() >= 300, (i, away.sum())
            assert np.array_equal(got[away, 2:], r64[away, 2:].astype(f32)), i
    print("sixteen textures: bilinear colours device %.3g, float32 restatement %.3g" % (worst_c, ref_c))
    assert worst_c <= 4 * ref_c
    assert worst_c <= 4 * SIXTEEN_COLOUR_MEASURED


def test_edge_coordinates_read_the_float32_restatements_texel(A, api, lib):
    """X.edge_cases(): u' exactly on integers and on k / W, at -2^-30, beyond +-1000, clamped beyond [0, 1], the rectangle's corners.  The colour of a checker or a
    nearest look-up is the FLOAT32 restatement's, exactly (the float64 one may sit on the other side of the edge; tests/test_texture.py pins the float32 one to
    hand-written texels); a bilinear look-up of the same image at the same points stays within TG.COLOUR_CEILING of it."""
    shape = make_shape(A, A.SHAPE_RECTANGLE, X.EDGE_RECT)
    scene, surface, material = TG.probe_scene(A, api, shape)
    xs = X.Shape.of(shape)
    for name, (tex, uvs) in X.edge_cases(material).items():
        pts = X.edge_points(uvs)
        got = api.kat_texture(scene, api_textures(api, [tex]), surface, pts)
        r32 = X.probe(xs, tex, pts, f32)
        assert np.array_equal(got[:, :2], r32[:, :2]) and np.array_equal(got[:, 2:], r32[:, 2:]), (name, got, r32)
        if tex.kind == X.IMAGE:
            bil = X.Tex(X.IMAGE, material, tex.flags | X.BILINEAR, tex.scale, tex.offset, texels=tex.texels)
            got = api.kat_texture(scene, api_textures(api, [bil]), surface, pts)
            worst = np.abs(got[:, 2:].astype(f64) - X.probe(xs, bil, pts, f32)[:, 2:]).max()
            print("%s: bilinear, device against the float32 restatement %.3g (allowed %.3g)" % (name, worst, TG.COLOUR_CEILING))
            assert worst <= TG.COLOUR_CEILING, name


# ---- E. the other lighting strategies on the textured rows ----

_tiled_cache = {}


def tiled_case(A, api, name, w, h):
    key = (name, w, h)
    if key not in _tiled_cache:
        scene, textures = TG.case_of(A, api, name, w, h)
        _tiled_cache[key] = (scene, textures, X.tiled(A, scene.scene, textures))
    return _tiled_cache[key]


def untextured_samples(api, scene, params, w, h, n):
    out = np.zeros((h, w, n, 3), f32)
    for y in range(h):
        for x in range(w):
            out[y, x] = api.kat_li(scene, params, x, y, 0, n)
    return out


_want_cache = {}


def strategy_samples(O, A, api, name, w, h, n_spp, sampler, strategy):
    """(scene, textures, params, [h, w, N, 3] what the tiled scene gives): kyo_li_tape for the strategies the oracle has (DIRECT_LIGHT_MIS, DIRECT_BSDF); for
    sample_single_light (49) and its power and spatial picks (113, 177), which it has not, the UNTEXTURED kernels' kyhip_kat_li on the tiled scene, code that
    tests/test_light_pick_gpu.py holds to its restatement -- there a vertex's colour is the tile's, so agreement pins "the spatial pick weighs a textured
    plastic vertex by its textured colour" (DESIGN.md section 13)."""
    key = (name, w, h, n_spp, sampler, strategy)
    if key not in _want_cache:
        scene, textures, tiled = tiled_case(A, api, name, w, h)
        params = TF.params_of(api, A, w, h, n_spp, sampler, direct_sample=strategy)
        if strategy in (A.DIRECT_LIGHT_MIS, A.DIRECT_BSDF):
            want = oracle_frame(O, A, tiled, params, w, h, n_spp, sampler, 256 if name == "veach" else 64)
        else:
            want = untextured_samples(api, tiled, params, w, h, n_spp)
        want.setflags(write=False)
        _want_cache[key] = (scene, textures, params, want)
    return _want_cache[key]


STRATEGIES = {"light_mis": 32, "bsdf": 4, "single_light": 49, "single_power": 113, "single_spatial": 177}


@pytest.mark.parametrize("strategy", tuple(STRATEGIES))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("name", ("cornell", "veach"))
def test_every_strategy_on_the_textured_rows(O, A, api, lib, name, n_spp, sampler, strategy):
    """kyhip_kat_li_textured under each direct_sample value the textured rows dispatch at run time and had never run, every sample of every pixel (Cornell
    32 x 32, Veach 48 x 27, whose plank's texture sits on plastic), against the tiled scene under TF.CAPS as they stand"""
    w, h, bad_share, sum_tol = TF.CAPS[name]
    assert (A.DIRECT_LIGHT_MIS, A.DIRECT_BSDF, A.DIRECT_SINGLE_BOTH_MIS, A.DIRECT_SINGLE_POWER, A.DIRECT_SINGLE_SPATIAL) == (32, 4, 49, 113, 177)
    scene, textures, params, want = strategy_samples(O, A, api, name, w, h, n_spp, sampler, STRATEGIES[strategy])
    assert params.direct_sample == STRATEGIES[strategy]
    got = device_samples(api, scene, params, api_textures(api, textures), w, h, n_spp)
    bad, tot, sg, sc = li_agreement(got, want)
    print("%s N = %d, %s, %s: %d of %d samples differ (cap %.0f), sums %.6g / %.6g" % (name, n_spp, sampler, strategy, bad, tot, bad_share * tot, sg, sc))
    assert tot >= 0.99 * w * h * n_spp and sg > 0
    assert bad <= bad_share * tot, (bad, tot)
    assert abs(sg - sc) <= sum_tol * max(sc, 1.0)


@pytest.mark.parametrize("strategy", tuple(STRATEGIES))
@pytest.mark.parametrize("name", ("cornell", "veach"))
def test_films_under_every_strategy(O, A, api, lib, name, strategy):
    """api.render(textures=) at 16 x 16, N = 5, against the mean of those samples; the launch is a textured row"""
    w = h = 16
    n_spp = 5
    scene, textures, params, want = strategy_samples(O, A, api, name, w, h, n_spp, "random", STRATEGIES[strategy])
    g, c = api.render(scene, params, textures=api_textures(api, textures)), T.film_of(want)
    kernel = lib.kyhip_last_kernel(0).decode()
    assert ", textured>" in kernel and "strategy -1" in kernel, kernel
    fin = np.isfinite(c).all(axis=2)
    e = rmse(g[fin], c[fin])
    print("%s, %s: rmse %.3g, allowed %.3g -- %s" % (name, strategy, e, T.film_tolerance(n_spp), kernel))
    assert (~fin).sum() <= 2 and g.max() > 0 and e < T.film_tolerance(n_spp)


def test_what_a_launch_under_a_texture_set_refuses(A, api, lib):
    """A texture set has no masked form and no row for the debug sampler, and takes no direct_sample value the untextured entries refuse: each is
    KY_ERR_INVALID_VALUE with the film and the samples untouched.  The masked form is refused in api.render, a ValueError: the C ABI has no entry that takes a set
    and a lighting mask -- kyhip_kat_li_lighting and kyhip_render_lighting take no set, kyhip_render_textured no mask -- so the launch's own refusal of a masked
    pass under a set cannot be reached from outside."""
    w = h = 16
    scene, textures = X.cornell_case(A, api, w, h)
    arr, n = api._texture_array(api_textures(api, textures))
    sp = api._scene_ptr(scene)
    film = np.full((h, w, 3), 0.25, f32)
    out = np.full((4, 3), 0.25, f32)
    with pytest.raises(ValueError, match="no masked form"):
        api.render(scene, api.make_params(w, h, 4), film=film, textures=api_textures(api, textures), lighting=A.LIGHTING_DIRECT)
    assert (film == 0.25).all()
    bad = [api.make_params(w, h, 4, sampler=A.SAMPLER_DEBUG)]
    for value in (1, 64, 128, 65, 112, 176, 49 | 64 | 128, 2, 177 + 256):   # single without both_mis, a pick without single, both picks, unknown bits
        bad.append(api.make_params(w, h, 4, direct_sample=value))
    for p in bad:
        assert lib.kyhip_render_textured(0, sp, arr, n, C.byref(p), None, None, film.ctypes.data_as(C.c_void_p), w) == A.KY_ERR_INVALID_VALUE, p.direct_sample
        assert lib.kyhip_kat_li_textured(0, sp, arr, n, C.byref(p), None, None, 3, 3, 0, 4, out.ctypes.data_as(C.c_void_p)) == A.KY_ERR_INVALID_VALUE, p.direct_sample
        assert (film == 0.25).all() and (out == 0.25).all()
    with api.Frame(scene, api.make_params(w, h, 4), textures=api_textures(api, textures)) as f:   # ... and a frame keeps its set once it holds a sample
        f.render(4)
        with pytest.raises(api.KyError):
            f.set_textures([])
