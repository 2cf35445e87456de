"""CPU: textures (ky_texture).  What kyhip_texture_check refuses, from the C ABI and from ky_amd.api; the NumPy restatement
(tests/texture_restatement.py) against what defines (u, v) and the two look-ups, with each named defect shown failing its check; and, on the CPU oracle alone, the
condition under which the tiled scene may stand in for a texture: two tilings of one checker trace the same paths to well inside the caps of the per-sample
comparison.  tests/test_texture_gpu.py holds the device against all this."""
import ctypes as C

import numpy as np
import pytest

import filter_restatement as F
import texture_restatement as X

f32, f64 = np.float32, np.float64


# ---- refusals ----

def small_scene(A, api):
    return api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)


def glass_material(scene):
    c = scene.c
    return next(i for i in range(c.material_count) if c.materials[i].kind == 2)


def test_what_the_check_refuses(A, api):
    lib = A.load_kyhip()
    scene = small_scene(A, api)
    sp = api._scene_ptr(scene)
    nan, inf = float("nan"), float("inf")
    img = np.full((2, 3, 3), 0.5, f32)

    def status(textures):
        arr, n = api._texture_array(textures)
        rc = lib.kyhip_texture_check(sp, arr, n)
        with_api = None
        try:
            api.texture_check(scene, textures)
        except api.KyError as e:
            with_api = str(e)
        assert (rc == A.KY_OK) == (with_api is None), (rc, with_api)
        return rc, lib.kyhip_last_error()

    ok = [api.texture_checker(1, (0.8, 0.8, 0.8), (0.1, 0.1, 0.1), scale=(4, -4), offset=(0.5, -3)), api.texture_image(3, img, bilinear=True, clamp=True),
          api.texture_checker(6, (1, 1, 1), (0, 0, 0)), api.texture_checker(5, (0, 0, 0), (0.2, 0.2, 0.2))]   # matte, matte, mirror, plastic
    assert status(ok)[0] == A.KY_OK and status([])[0] == A.KY_OK
    invalid = {
        "glass": [api.texture_checker(glass_material(scene), (1, 1, 1), (0, 0, 0))],
        "already": [api.texture_checker(1, (1, 1, 1), (0, 0, 0)), api.texture_image(1, img)],
        "out of range": [api.texture_checker(scene.c.material_count, (1, 1, 1), (0, 0, 0))],
        "out of range ": [api.texture_checker(-1, (1, 1, 1), (0, 0, 0))],
        "colours": [api.texture_checker(1, (1, nan, 1), (0, 0, 0))],
        "colours ": [api.texture_checker(1, (1, 1, 1), (0, -0.1, 0))],
        "colours  ": [api.texture_checker(1, (inf, 1, 1), (0, 0, 0))],
        "scale": [api.texture_checker(1, (1, 1, 1), (0, 0, 0), scale=(0, 1))],
        "scale ": [api.texture_image(1, img, scale=(1, 0))],
        "scale  ": [api.texture_checker(1, (1, 1, 1), (0, 0, 0), scale=(nan, 1))],
        "offset": [api.texture_checker(1, (1, 1, 1), (0, 0, 0), offset=(0, inf))],
        "scale   ": [api.texture_checker(1, (1, 1, 1), (0, 0, 0), scale=(1, -(2.0 ** 20 + 1)))],   # beyond KYHIP_MAX_TEXTURE_SCALE: floor(u') + floor(v') stays an exact int
        "offset ": [api.texture_image(1, img, offset=(2.0 ** 21, 0))],
    }
    assert status([api.texture_checker(1, (1, 1, 1), (0, 0, 0), scale=(2.0 ** 20, -2.0 ** 20), offset=(-2.0 ** 20, 2.0 ** 20))])[0] == A.KY_OK
    for word, bad in invalid.items():
        rc, msg = status(bad)
        assert rc == A.KY_ERR_INVALID_VALUE and word.strip().encode() in msg, (word, rc, msg)
    for k, v in ((0, -1.0), (5, nan), (17, inf)):   # one bad texel anywhere in the image
        texels = img.copy()
        texels.reshape(-1)[k] = v
        rc, msg = status([api.texture_image(1, texels)])
        assert rc == A.KY_ERR_INVALID_VALUE and b"texel" in msg
    null = api.texture_image(1, img)
    null.texels = None
    rc, msg = status([null])
    assert rc == A.KY_ERR_INVALID_VALUE and b"without texels" in msg
    for field, value, word in (("kind", 2, b"kind"), ("reserved", 1, b"reserved"), ("flags", 4, b"flags"), ("width", 0, b"texels")):
        t = api.texture_image(1, img)
        setattr(t, field, value)
        rc, msg = status([t])
        assert rc == A.KY_ERR_INVALID_VALUE and word in msg, (field, msg)
    assert lib.kyhip_texture_check(sp, None, 1) == A.KY_ERR_INVALID_VALUE and lib.kyhip_texture_check(sp, None, -1) == A.KY_ERR_INVALID_VALUE


def test_the_limits(A, api):
    lib = A.load_kyhip()
    base = small_scene(A, api)
    scene = X.copy_scene(A, base.c, {s: None for s in (0, 1, 2, 3, 4, 7, 8, 9, 10, 11)})[0]   # 17 materials that are not glass
    sp = api._scene_ptr(scene)
    mats = [i for i in range(scene.scene.material_count) if scene.scene.materials[i].kind != A.MATERIAL_GLASS]
    assert len(mats) >= 17

    def status(textures):
        arr, n = api._texture_array(textures)
        return lib.kyhip_texture_check(sp, arr, n), lib.kyhip_last_error()

    sixteen = [api.texture_checker(m, (1, 1, 1), (0, 0, 0)) for m in mats[:16]]
    assert status(sixteen)[0] == A.KY_OK
    rc, msg = status(sixteen + [api.texture_checker(mats[16], (1, 1, 1), (0, 0, 0))])
    assert rc == A.KY_ERR_LIMIT and b"at most 16" in msg
    with pytest.raises(api.KyError):
        api.texture_check(scene, sixteen + [api.texture_checker(mats[16], (1, 1, 1), (0, 0, 0))])
    assert status([api.texture_image(mats[0], np.zeros((1, 4096, 3), f32))])[0] == A.KY_OK
    for shape in ((1, 4097, 3), (4097, 1, 3)):
        rc, msg = status([api.texture_image(mats[0], np.zeros(shape, f32))])
        assert rc == A.KY_ERR_LIMIT and b"4096" in msg
    big = np.zeros((2048, 4096, 3), f32)   # 2^23 texels each: two fill the set, a third texel is one too many
    assert status([api.texture_image(mats[0], big), api.texture_image(mats[1], big)])[0] == A.KY_OK
    rc, msg = status([api.texture_image(mats[0], big), api.texture_image(mats[1], big), api.texture_image(mats[2], np.zeros((1, 1, 3), f32))])
    assert rc == A.KY_ERR_LIMIT and b"16777216" in msg


def test_the_device_entries_refuse_a_bad_set_before_they_look_for_a_device(A, api):
    lib = A.load_kyhip()
    scene = small_scene(A, api)
    sp = api._scene_ptr(scene)
    p = api.make_params(16, 16, 4)
    film = np.zeros((16, 16, 3), f32)
    bad, n = api._texture_array([api.texture_checker(glass_material(scene), (1, 1, 1), (0, 0, 0))])
    assert lib.kyhip_render_textured(0, sp, bad, n, C.byref(p), None, None, film.ctypes.data_as(C.c_void_p), 16) == A.KY_ERR_INVALID_VALUE
    assert b"glass" in lib.kyhip_last_error() and film.max() == 0
    out = np.zeros((4, 5), f32)
    assert lib.kyhip_kat_li_textured(0, sp, bad, n, C.byref(p), None, None, 3, 3, 0, 4, out.ctypes.data_as(C.c_void_p)) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_kat_texture(0, sp, bad, n, 0, out.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_frame_set_textures(None, None, 1) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_frame_set_textures(None, bad, 17) == A.KY_ERR_LIMIT
    assert lib.kyhip_frame_set_textures(None, bad, 1) == A.KY_ERR_INVALID_VALUE and b"frame is NULL" in lib.kyhip_last_error()
    with pytest.raises(api.KyError):
        api.render(scene, p, textures=[api.texture_checker(glass_material(scene), (1, 1, 1), (0, 0, 0))])
    assert C.sizeof(A.Texture) == 72


# ---- the restatement against the definitions; the named defects ----

QUAD = X.Shape(X.RECTANGLE, [(1, 2, 3), (4, 2, 3), (4, 2, 8), (1, 2, 8)], (0, 1, 0))   # 3 along u, 5 along v


def test_uv_of_each_shape_kind():
    for dtype in (f32, f64):
        u, v = X.uv(QUAD, QUAD.p, dtype)
        assert np.abs(u - [0, 1, 1, 0]).max() < 1e-6 and np.abs(v - [0, 0, 1, 1]).max() < 1e-6   # (1 / 9 and 1 / 25 are rounded to float32 once, by the host)
        tri = X.Shape(X.TRIANGLE, [(0, 0, 0), (2, 0, 0), (1, 3, 0)], (0, 0, 1))
        q = (tri.p[0] + f32(0.25) * (tri.p[1] - tri.p[0]) + f32(0.5) * (tri.p[2] - tri.p[0]))[None, :]
        u, v = X.uv(tri, np.concatenate([tri.p[:3], q]), dtype)
        assert np.abs(u - [0, 1, 0, 0.25]).max() < 1e-6 and np.abs(v - [0, 0, 1, 0.5]).max() < 1e-6
        disk = X.Shape(X.DISK, [(1, 1, 1)], (0, 0, 1), 2.0)
        s, t = X.frame(disk.normal)
        u, v = X.uv(disk, np.stack([disk.p[0], disk.p[0] + 2 * s, disk.p[0] - 2 * t]), dtype)
        assert np.abs(u - [0.5, 1, 0.5]).max() < 1e-6 and np.abs(v - [0.5, 0.5, 0]).max() < 1e-6
        ball = X.Shape(X.SPHERE, [(1, 2, 3)], radius=0.5)
        pts = ball.p[0] + f32(0.5) * np.array([(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, 1), (-1, 0, 0)], f32)
        u, v = X.uv(ball, pts, dtype)
        assert np.abs(v - [0, 1, 0.5, 0.5, 0.5]).max() < 1e-6 and np.abs(u[2:] - [0.5, 0.75, 1.0]).max() < 1e-6


def test_defect_u_and_v_swapped_on_the_rectangle():
    """the check: the corner p1 of a rectangle is (1, 0), p3 is (0, 1)"""
    def check(**kw):
        u, v = X.uv(QUAD, QUAD.p[[1, 3]], f64, **kw)
        return np.abs(u - [1, 0]).max() < 1e-6 and np.abs(v - [0, 1]).max() < 1e-6
    assert check() and not check(swap=True)


def test_defect_a_checker_keyed_on_the_floor_of_the_sum():
    """the check: over the centres of an 8 x 8 block of cells the colour is a where i + j is even"""
    tex = X.Tex(X.CHECKER, 0, a=(1, 1, 1), b=(0, 0, 0))
    i, j = np.meshgrid(np.arange(-4, 4), np.arange(-4, 4), indexing="ij")
    us, vs = (i.ravel() + 0.6).astype(f32), (j.ravel() + 0.7).astype(f32)
    want = np.where(((i + j).ravel() % 2 == 0)[:, None], tex.a, tex.b)

    def check(**kw):
        return np.array_equal(X.checker(tex, us, vs, **kw), want)
    assert check() and not check(parity="floor_of_sum")


def smooth_image(n=8):
    c = (np.arange(n) + 0.5) / n
    g = 0.5 + 0.4 * np.outer(np.sin(2 * np.pi * c), np.sin(2 * np.pi * c))
    return np.stack([g, 0.5 * g, 1 - g], axis=2).astype(f32)


def test_defect_bilinear_without_the_half():
    """the check: at a texel's centre, u' = (i + 0.5) / W, the bilinear value is the texel"""
    img = smooth_image()
    j, i = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    us, vs = ((i.ravel() + 0.5) / 8).astype(f32), ((j.ravel() + 0.5) / 8).astype(f32)
    for flags in (X.BILINEAR, X.BILINEAR | X.CLAMP):
        tex = X.Tex(X.IMAGE, 0, flags, texels=img)

        def check(**kw):
            return np.abs(X.bilinear(tex, us, vs, f64, **kw) - img[j.ravel(), i.ravel()]).max() < 1e-6
        assert check() and not check(half=False)


def test_defect_row_0_at_v_1():
    """the check: v' just above 0 reads row 0, v' just below 1 the last row -- nearest and bilinear (clamped)"""
    img = smooth_image()
    img[0] += 0.05   # (the smooth image's first and last rows mirror each other)
    us = ((np.arange(8) + 0.5) / 8).astype(f32)
    lo, hi = np.full(8, 1e-3, f32), np.full(8, 1 - 1e-3, f32)
    near, bil = X.Tex(X.IMAGE, 0, 0, texels=img), X.Tex(X.IMAGE, 0, X.BILINEAR | X.CLAMP, texels=img)

    def check(**kw):
        return (np.array_equal(X.nearest(near, us, lo, f32, **kw), img[0]) and np.array_equal(X.nearest(near, us, hi, f32, **kw), img[7]) and
                np.abs(X.bilinear(bil, us, lo, f64, **kw) - img[0]).max() < 1e-6 and np.abs(X.bilinear(bil, us, hi, f64, **kw) - img[7]).max() < 1e-6)
    assert check() and not check(row0="v1")


def test_wraps_and_the_two_precisions():
    gen = np.random.default_rng(11)
    img = smooth_image()
    us, vs = (gen.random(4096) * 6 - 3).astype(f32), (gen.random(4096) * 6 - 3).astype(f32)
    for flags in (0, X.CLAMP, X.BILINEAR, X.BILINEAR | X.CLAMP):
        tex = X.Tex(X.IMAGE, 0, flags, texels=img)
        a, b = X.lookup(tex, us, vs, f32), X.lookup(tex, us, vs, f64)
        assert np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
        if flags & X.BILINEAR:
            assert np.abs(a - b).max() < 1e-4   # (the fraction of u' W - 0.5 carries the rounding of u' W: 3 x 8 x 2^-24 x the image's slope)
        # repeat: whole periods further is the same colour -- bilinear to rounding, nearest exactly on every point that is no texel edge's neighbour
        far = X.lookup(tex, us.astype(f64) + 2, vs.astype(f64) - 1, f64)
        if not flags & X.CLAMP:
            if flags & X.BILINEAR:
                assert np.abs(far - b).max() < 1e-6
            else:
                away = X.edge_distance(tex, us.astype(f64), vs.astype(f64)) >= 1e-6
                assert away.sum() >= 0.99 * us.size and np.array_equal(far[away], b[away])
    clamp = X.Tex(X.IMAGE, 0, X.CLAMP, texels=img)
    assert np.array_equal(X.nearest(clamp, np.array([-5, 7], f32), np.array([0.5, 0.5], f32)), img[[4, 4], [0, 7]])


# ---- the cap's condition, on the oracle alone ----

@pytest.mark.parametrize("sampler", ("random", "stratified"))
def test_two_tilings_of_one_checker_trace_the_same_paths(O, A, api, sampler):
    """The 4 x 4 checker on the Cornell floor as 16 tiles and as 64 (2 x 2 tiles per cell), replayed through kyo_li_tape on the same tapes: Cornell 32 x 32, N = 16.
    A sample differs if it is off by more than 1e-3 relative (tests/test_stratified_gpu.py's rule); the two tilings differ in at most HALF of the cap that
    comparison has for this frame -- 0.2 % of samples, sums to 1e-4 -- so what a tiling's edges cost leaves the device half of it."""
    import test_filter_gpu as G
    w, h, bad_share, sum_tol = G.CAPS["cornell"]
    assert (w, h, bad_share, sum_tol) == (32, 32, 0.002, 1e-4)
    n = 16
    scene, textures = X.cornell_case(A, api, w, h, only_floor=True)
    coarse, fine = X.tiled(A, scene.scene, textures), X.tiled(A, scene.scene, textures, subdivide=2)
    assert coarse.scene.surface_count == scene.scene.surface_count + 15 and fine.scene.surface_count == scene.scene.surface_count + 63
    kind = F.SAMPLER_STRATIFIED if sampler == "stratified" else F.SAMPLER_RANDOM
    params = api.make_params(w, h, n, sampler=kind)
    bad = tot = 0
    sa = sb = 0.0
    for y in range(h):
        for x in range(w):
            tape = F.tape(params.seed, y * w + x, n, 64, kind, None)
            a, b = O.li_tape(coarse, params, x, y, tape)[0], O.li_tape(fine, params, x, y, tape)[0]
            fin = np.isfinite(a).all(1) & np.isfinite(b).all(1)
            d = np.abs(a[fin] - b[fin]).max(axis=1)
            s = np.maximum(1e-3, np.abs(b[fin]).max(axis=1))
            bad += int((d / s > 1e-3).sum())
            tot += int(fin.sum())
            sa += float(np.minimum(a[fin], 10).sum())
            sb += float(np.minimum(b[fin], 10).sum())
    print("%s: %d of %d samples differ between the tilings (allowed %.1f), sums %.6g / %.6g" % (sampler, bad, tot, 0.5 * bad_share * tot, sa, sb))
    assert tot >= 0.99 * w * h * n
    assert bad <= 0.5 * bad_share * tot
    assert abs(sa - sb) <= 0.5 * sum_tol * max(sb, 1.0)


# ---- the host mirror ----

def test_the_host_mirrors_flattening_yields_the_set_the_c_call_takes(A, api):
    """ky.hpp: checker_texture_t and image_texture_t on the textured overloads of plastic_material_t, matte_material_t and mirror_material_t; scene_t::flatten_textures()
    is the ky_texture array kyhip_texture_check accepts, field for field what api.texture_checker / api.texture_image build; a constant_texture_t-like plain
    material yields none; glass is refused."""
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    assert scene.textures() == []
    kinds = [scene.c.materials[i].kind for i in range(scene.c.material_count)]
    plastic, matte, mirror, glass = (kinds.index(k) for k in (A.MATERIAL_PLASTIC, A.MATERIAL_MATTE, A.MATERIAL_MIRROR, A.MATERIAL_GLASS))
    before = A.Material.from_buffer_copy(scene.c.materials[plastic])
    img = (np.arange(2 * 3 * 3, dtype=f32).reshape(2, 3, 3) + 1) / 32
    scene.texture_checker(plastic, (0.25, 0.25, 0.0625), (0.03125, 0.0625, 0.25), scale=(4, 4), offset=(0.5, 0.25))
    scene.texture_image(matte, img, bilinear=True, clamp=True, scale=(2, -2))
    scene.texture_checker(mirror, (0.9, 0.9, 0.9), (0.5, 0.25, 0.125))
    with pytest.raises(api.KyError, match="glass"):
        scene.texture_checker(glass, (1, 1, 1), (0, 0, 0))
    got = scene.textures()
    want = sorted([api.texture_checker(plastic, (0.25, 0.25, 0.0625), (0.03125, 0.0625, 0.25), scale=(4, 4), offset=(0.5, 0.25)),
                   api.texture_image(matte, img, bilinear=True, clamp=True, scale=(2, -2)), api.texture_checker(mirror, (0.9, 0.9, 0.9), (0.5, 0.25, 0.125))],
                  key=lambda t: t.material)
    assert len(got) == 3 and [t.material for t in got] == [t.material for t in want]   # in material order
    for g, w in zip(got, want):
        for field in ("kind", "material", "flags", "reserved", "width", "height"):
            assert getattr(g, field) == getattr(w, field), field
        for field in ("scale", "offset", "a", "b"):
            assert list(getattr(g, field)) == list(getattr(w, field)), field
        if g.kind == A.TEXTURE_IMAGE:
            assert np.array_equal(np.ctypeslib.as_array(g.texels, (2, 3, 3)), img)
    arr, n = api._texture_array(got)
    assert lib.kyhip_texture_check(api._scene_ptr(scene), arr, n) == A.KY_OK
    # the materials keep their kinds; the struct's colour is the texture's base colour, a plastic material's probabilities are that colour's
    after = scene.c.materials[plastic]
    assert [scene.c.materials[i].kind for i in range(scene.c.material_count)] == kinds
    assert list(after.color0) == [0.25, 0.25, 0.0625] and list(after.color1) == list(before.color1) and after.exponent == before.exponent
    lum = lambda c: f32(0.212671) * f32(c[0]) + f32(0.715160) * f32(c[1]) + f32(0.072169) * f32(c[2])
    d, s = lum(after.color0), lum(after.color1)
    assert abs(after.diffuse_probability - d / (d + s)) < 1e-6 and abs(after.diffuse_probability + after.specular_probability - 1) < 1e-6
    assert [sf.material for sf in (scene.c.surfaces[i] for i in range(scene.c.surface_count))].count(plastic) >= 1   # the surfaces carry the new material


# ---- tiled() refuses what it would cut wrongly ----

def test_tiled_refuses_a_parallelogram_whose_edges_are_not_orthogonal(A, api):
    """tex_uv's rectangle body is u = d . e1 / |e1|^2; on a sheared parallelogram that is not the coordinate tiled() cuts along, so it refuses one"""
    from helpers import make_material, make_shape
    box = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    for shear, refused in ((0.0, False), (1e-3, True), (0.3, True)):
        scene, _ = X.copy_scene(A, box.c)
        shapes, mats, lights, surfaces = scene._keep
        shapes.append(make_shape(A, A.SHAPE_RECTANGLE, [(-0.5, 0.0, -0.5), (0.5, 0.0, -0.5), (0.5 + shear, 0.0, 0.5), (-0.5 + shear, 0.0, 0.5)]))
        mats.append(make_material(A, A.MATERIAL_MATTE, (0.5, 0.5, 0.5)))
        surfaces.append(A.Surface(len(shapes) - 1, len(mats) - 1, -1))
        from helpers import CustomScene
        scene = CustomScene(A, A.Camera.from_buffer_copy(box.c.camera), shapes, mats, lights, surfaces)
        tex = [X.Tex(X.CHECKER, len(mats) - 1, scale=(2, 2), a=(1, 1, 1), b=(0, 0, 0))]
        if refused:
            with pytest.raises(AssertionError, match="orthogonal"):
                X.tiled(A, scene.scene, tex)
        else:
            assert X.tiled(A, scene.scene, tex).scene.surface_count == scene.scene.surface_count + 3
    for case in (X.cornell_case, X.veach_case):   # every shipped case is still cut
        scene, textures = case(A, api, 16, 16)
        assert X.tiled(A, scene.scene, textures).scene.surface_count > scene.scene.surface_count


# ---- the texel layout: three more named defects ----

def layout_set():
    """a checker, the 3 x 5 image and a 5 x 3 image behind it: the image's first texel is 2, and every defective index stays inside the array"""
    return [X.Tex(X.CHECKER, 0, a=(1, 1, 1), b=(0, 0, 0)), X.Tex(X.IMAGE, 1, texels=X.texels_of(0, 3, 5)), X.Tex(X.IMAGE, 2, texels=X.texels_of(1, 5, 3))]


def test_defects_of_the_texel_layout():
    """the check: at the centre of texel (x, y) of the 3 x 5 image -- image 0 -- a nearest look-up reads ((x + 1) / 8, (y + 1) / 8, 1 / 16)"""
    textures = layout_set()
    flat, first = X.pack(textures)
    assert first == [0, 2, 17] and len(flat) == 32
    y, x = np.meshgrid(np.arange(5), np.arange(3), indexing="ij")
    us, vs = ((x.ravel() + 0.5) / 3).astype(f32), ((y.ravel() + 0.5) / 5).astype(f32)
    want = np.stack([(x.ravel() + 1) / 8, (y.ravel() + 1) / 8, np.full(15, 1 / 16)], axis=1).astype(f32)

    def check(**kw):
        return np.array_equal(X.nearest_packed(textures, 1, us, vs, f32, **kw), want)
    assert check() and np.array_equal(X.nearest(textures[1], us, vs), want)
    for defect in ("transposed", "stride_h", "no_first"):
        assert not check(defect=defect), defect
    gen = np.random.default_rng(5)   # the packed look-up is the structured one
    us, vs = (gen.random(2048) * 6 - 3).astype(f32), (gen.random(2048) * 6 - 3).astype(f32)
    for i in (1, 2):
        assert np.array_equal(X.nearest_packed(textures, i, us, vs), X.nearest(textures[i], us, vs))


# What the float32 restatement must read at X.edge_cases()'s points, written by hand: texel (ix, iy) of a nearest look-up, 0 / 1 = colour a / b of a checker.
EDGE_PINS = {
    "on k / W": [(0, 0), (1, 0), (2, 0), (3, 0), (0, 0), (2, 1), (1, 0), (0, 0), (0, 0), (0, 0), (0, 0)],   # u' = 1 wraps to 0; so does every corner
    "-2^-30": [(3, 0), (1, 0), (2, 1)],            # -2^-30 - floor = 1.0f: index 4, capped at 3; 0.25 - 2^-30 is 0.25f (the float64 path reads texel 0 there)
    "beyond 1000": [(0, 0), (0, 0), (1, 0), (2, 0), (1, 1)],   # -2048, 2048, 0.25, -2047.5 (fraction 0.5), 2047.25
    "clamped": [(0, 1), (3, 0), (2, 1), (3, 0), (0, 1), (3, 1), (3, 0), (0, 0)],   # u' = 3 u - 1, v' = 1.5 - 2 v, both clamped to [0, 1 - 2^-24]
    "on k / 5": [(1, 1), (2, 2), (3, 1), (4, 0), (0, 1)],   # float(k / 5) 5 rounds to k; the float below 1 / 3 times 3 is 1 - 2^-24
    "checker on integers": [0, 1, 0, 1, 0, 0, 0, 0, 0, 0],
    "checker beyond 1000": [0, 0, 1, 0, 1],        # floor(-2047.5) = -2048
    "checker -2^-30": [1, 0, 0],                   # floor(-2^-30) = -1
}


def test_the_float32_restatement_at_edge_coordinates_reads_the_pinned_texels():
    rect = X.Shape(X.RECTANGLE, X.EDGE_RECT, (0, -1, 0))
    cases = X.edge_cases()
    assert set(cases) == set(EDGE_PINS)
    for name, (tex, uvs) in cases.items():
        pts = X.edge_points(uvs)
        u, v = X.uv(rect, pts, f32)
        assert np.array_equal(u, np.asarray(uvs, f32)[:, 0]) and np.array_equal(v, np.asarray(uvs, f32)[:, 1]), name   # (u, v) of these points is exact
        got = X.probe(rect, tex, pts, f32)
        assert np.abs(got[:, :2]).max() < 2.0 ** 24
        if tex.kind == X.CHECKER:
            want = np.where(np.array(EDGE_PINS[name])[:, None] == 0, tex.a[None, :], tex.b[None, :])
        else:
            want = np.array([tex.texels[iy, ix] for ix, iy in EDGE_PINS[name]])
        assert np.array_equal(got[:, 2:], want.astype(f32)), (name, got[:, 2:], want)
    # the float64 path does sit on the other side of an edge at one of them, which is why the device is held to the float32 path there
    tex, uvs = cases["-2^-30"]
    assert not np.array_equal(X.probe(rect, tex, X.edge_points(uvs), f64)[:, 2:].astype(f32), X.probe(rect, tex, X.edge_points(uvs), f32)[:, 2:])


# ---- the scene that textures every shape kind: properties of the inputs, and that the expected samples notice wrong plumbing ----

_expected_cache = {}


def shapes_expected(O, A, api, which, n_spp, sampler, with_k=True):
    """(scene, textures, names, params, X.expected_samples(...)) of X.shapes_case / _shipped / _large at 32 x 32, computed once per case and shared"""
    key = (which, n_spp, sampler, with_k)
    if key not in _expected_cache:
        case = {"general": X.shapes_case, "shipped": X.shapes_case_shipped, "large": X.shapes_case_large}[which]
        scene, textures, names = case(A, api, 32, 32)
        kind = F.SAMPLER_STRATIFIED if sampler == "stratified" else F.SAMPLER_RANDOM
        params = api.make_params(32, 32, n_spp, integrator=A.INTEGRATOR_BASECOLOR, sampler=kind)
        _expected_cache[key] = (scene, textures, names, params, X.expected_samples(O, A, scene, textures, params, with_k=with_k))
    return _expected_cache[key]


@pytest.mark.parametrize("sampler", ("random", "stratified"))
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("which", ("general", "shipped", "large"))
def test_the_shapes_cases_inputs(O, A, api, which, n_spp, sampler):
    """At most 2 % of the samples that land on textured surfaces lie within 1e-4 of a cell or texel edge or on a sphere's seam; every textured surface is seen;
    the set is one the library accepts."""
    scene, textures, names, params, E = shapes_expected(O, A, api, which, n_spp, sampler, with_k=False)
    api.texture_check(scene, [t.to_api(api) for t in textures])
    on = E.textured
    print("%s N = %d, %s: %d of %d samples on textured surfaces, %d of them unclean (allowed %.1f)" % (which, n_spp, sampler, on.sum(), on.size, (on & ~E.clean).sum(), 0.02 * on.sum()))
    assert on.sum() >= (0.02 if which == "large" else 0.25) * on.size   # (the large scene's balls are small)
    assert (on & ~E.clean).sum() <= 0.02 * on.sum()
    seen = [s for s in (names["balls"] if which == "large" else names.values()) if (E.surface == s).sum() >= (1 if which == "large" else 5)]
    if which == "large":
        assert len(seen) >= 16, len(seen)   # (of 33 records behind the one texture)
    else:
        assert len(seen) == len(names), (seen, names)


def test_the_first_hit_is_the_first_row_of_the_oracles_trace(O, A, api):
    """expected_samples takes the first hit from kyo_kat_camera and kyo_kat_scene_intersect on the tape's camera sample; under the random sampler, whose generator
    the oracle has, that is the first row of kyo_trace_li -- surface and position, bit for bit, every sample"""
    scene, textures, names, params, E = shapes_expected(O, A, api, "general", 5, "random", with_k=False)
    pt = api.make_params(32, 32, 5)
    surface, position = E.surface.reshape(32, 32, 5), E.position.reshape(32, 32, 5, 3)
    for y in range(32):
        for x in range(32):
            for s in range(5):
                rows = O.trace_li(scene, pt, x, y, s, max_rows=2)
                if surface[y, x, s] < 0:
                    assert len(rows) == 0
                else:
                    assert int(rows[0, 1]) == surface[y, x, s] and np.array_equal(rows[0, 3:6], position[y, x, s]), (x, y, s)


@pytest.mark.parametrize("sampler", ("random", "stratified"))
def test_the_expected_samples_move_when_the_plumbing_is_wrong(O, A, api, sampler):
    """Recomputed with the uv records rotated among the textured surfaces (a record read at the sorted index where the caller's was meant) and with the shared
    material's second surface -- the second ball -- given the triangle's record: each changes at least 25 % of the samples on the surfaces whose record moved."""
    scene, textures, names, params, E = shapes_expected(O, A, api, "general", 16, sampler, with_k=False)
    order = [names[n] for n in ("tri", "disk", "ball2", "quad", "wall", "ball")]
    for what, record_of in (("rotated", {s: order[(i + 1) % len(order)] for i, s in enumerate(order)}), ("shared", {names["ball2"]: names["tri"]})):
        wrong = X.expected_samples(O, A, scene, textures, params, with_k=False, record_of=record_of)
        rows = np.isin(E.surface, list(record_of))
        moved = (np.abs(wrong.expected[rows] - E.expected[rows]).max(axis=1) > 1e-3).sum()
        print("%s, %s: %d of %d samples move" % (sampler, what, moved, rows.sum()))
        assert rows.sum() >= 100 and moved >= 0.25 * rows.sum()
