"""Albedo demodulation in a frame's denoise filter, on the GPU (include/kyhip.h, kyhip_frame_set_albedo_grid ...; DESIGN.md "Denoise", "Albedo"): the albedo buffer
(denoise_albedo_kernel, ky_amd/csrc/ky_denoise.hip) against its restatement on the CPU oracle's camera and scene-intersect KATs with tests/texture_restatement.py's
colours; the demodulating gather and the remodulating add against the NumPy restatement fed the frame's own checkpoint, guides, keys and albedo; what grid 0 and
two calls return; and the claim: on textured surfaces the demodulated filter lies below the plain one and below the unfiltered mean."""
import ctypes as C

import numpy as np
import pytest

import denoise_albedo_restatement as DA
import denoise_restatement as D
import filter_restatement as F
import noise_restatement as R
import test_denoise_gpu as T
import texture_restatement as X

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 24, 500
REL = 4 * 2.0 ** -23
CAP = 0.02


def _case(A, api, w, h):
    scene, textures = X.cornell_case(A, api, w, h)
    return scene, textures, [t.to_api(api) for t in textures]


def _plain(A, api, flags, w, h):
    return api.cornell_box_scene(flags, w, h)


def _two_passes(f):
    f.render(16)
    f.render(16)


def _compare_albedo(got, want, clean, what):
    """Clean pixels within 4 x 2^-23 relative, w exact; at most 2 % of the film is not clean"""
    assert clean.mean() >= 1 - CAP, (what, clean.mean())
    g, c = got[clean].astype(np.float64), want[clean].astype(np.float64)
    err = np.abs(g[:, :3] - c[:, :3])
    rel = float((err / np.maximum(np.abs(c[:, :3]), 1e-300)).max())
    print("%s: %d of %d pixels not clean; largest relative |albedo - restatement| on the clean ones %.3e" % (what, int((~clean).sum()), clean.size, rel))
    assert (err <= REL * np.abs(c[:, :3])).all(), (what, rel)
    assert np.array_equal(got[clean][:, 3], want[clean][:, 3]), what
    return rel


ALBEDO_CASES = [("textured", 40, 24, 16, 16, 1), ("textured", 40, 24, 16, 16, 4), ("textured", 44, 21, 8, 8, 4), ("textured", 264, 40, 16, 16, 4),
                ("untextured", 40, 24, 16, 16, 4), ("textured", 40, 24, 16, 16, 3)]


@pytest.mark.parametrize("which,w,h,tile_w,tile_h,G", ALBEDO_CASES, ids=["%s_%dx%d_tile_%dx%d_grid_%d" % c for c in ALBEDO_CASES])
def test_the_albedo_buffer_against_the_restatement(which, w, h, tile_w, tile_h, G, A, api, O):
    """The restatement takes the oracle's first hit at every sub-sample position and texture_restatement's colour there (plastic: / diffuse_probability); the sum
    is float32 in visit order on both sides.  Clean pixels: every sub-sample >= 1e-4 from a cell or texel edge and the oracle's hit surface unchanged when the film
    point moves by +-1e-3 pixel.  264 x 40: a workgroup's 256 pixels straddle rows.  Grid 3: 1 / G is no power of two.
    Not clean on the oracle's own frames (counted on the CPU before any GPU run): 40 x 24 grid 1: 2 of 960; grid 4: 7; grid 3: 7; 44 x 21 grid 4: 4 of 924;
    264 x 40 grid 4: 12 of 10 560; untextured 40 x 24 grid 4: 4 -- all below the 2 % cap, so the texture scales stay where cornell_case has them."""
    if which == "textured":
        scene, textures, tx = _case(A, api, w, h)
    else:
        scene, textures, tx = _plain(A, api, A.CB_DEFAULT_SCENE, w, h), [], None
    with api.Frame(scene, api.make_params(w, h, 48, tile_w=tile_w, tile_h=tile_h), noise=True, textures=tx, albedo=G) as f:
        assert f.albedo_grid == G
        f.render(16)
        got = f.albedo()
    want, clean, first = DA.albedo(O, A, scene, textures, w, h, G)
    _compare_albedo(got, want, clean, "%s %d x %d grid %d" % (which, w, h, G))
    assert (got[..., 3] >= 0).all() and (got[..., 3] <= G * G).all() and np.isfinite(got).all()
    if which == "textured":   # the textures are seen: the floor's two checker colours over the plastic's diffuse probability, and the mirror wall's
        c = scene.scene
        floor = textures[0]
        pd = np.float32(c.materials[floor.material].diffuse_probability)
        for colour in (floor.a / pd, floor.b / pd):
            assert (np.abs(got[..., :3] - colour.astype(np.float32)).max(axis=2) <= 1e-6).sum() >= 4


@pytest.mark.parametrize("name", ["cornell_case", "large_mirror"])
def test_the_chain_colours(name, A, api, O):
    """Guide bounces 2: a pure pixel on a mirror (all G^2 sub-samples reflected onto one constant-colour surface, w == G^2) holds the mirror's colour x the colour of
    what it shows; at 0 bounces the same pixel holds the mirror's colour alone.  The restatement follows mirrors and glass in double (reflect or refract, offset
    origin) on the oracle's scene-intersect."""
    G = 4
    if name == "cornell_case":
        scene, textures, tx = _case(A, api, W, H)
    else:
        scene, textures, tx = _plain(A, api, A.CB_LARGE_MIRROR | A.CB_LIGHT_AREA, W, H), [], None
    c = DA.scene_c(scene)
    got = {}
    for bounces in (0, 2):
        with api.Frame(scene, api.make_params(W, H, 48), noise=True, textures=tx, guide_bounces=bounces, albedo=G) as f:
            f.render(16)
            got[bounces] = f.albedo()
    want0, clean0, first = DA.albedo(O, A, scene, textures, W, H, G, bounces=0)
    want2, clean2, _ = DA.albedo(O, A, scene, textures, W, H, G, bounces=2)
    kinds = np.array([c.materials[c.surfaces[s].material].kind for s in range(c.surface_count)])
    one_surface = (first == first[..., :1]).all(axis=2) & (first[..., 0] >= 0)
    on_mirror = one_surface & (kinds[np.maximum(first[..., 0], 0)] == A.MATERIAL_MIRROR)
    pure = on_mirror & clean0 & clean2 & (want2[..., 3] == G * G)
    assert pure.sum() >= 8, int(pure.sum())
    tol = lambda want: REL * np.abs(want.astype(np.float64))
    assert (np.abs(got[0][pure][:, :3].astype(np.float64) - want0[pure][:, :3]) <= tol(want0[pure][:, :3])).all()
    assert (np.abs(got[2][pure][:, :3].astype(np.float64) - want2[pure][:, :3]) <= tol(want2[pure][:, :3])).all()
    assert np.array_equal(got[2][pure][:, 3], want2[pure][:, 3])
    # at two bounces the pixel changes by the colour of what the mirror shows (a plastic floor's c0 = Kd / P_diff may exceed 1) ...
    ratio = got[2][pure][:, :3].astype(np.float64) / got[0][pure][:, :3]
    assert (np.abs(ratio - 1).max(axis=1) > 0.05).all()
    # ... and it IS mirror colour x the colour shown
    mirror_colour = got[0][pure][:, :3].astype(np.float64)
    shown = want2[pure][:, :3].astype(np.float64) / want0[pure][:, :3].astype(np.float64)
    assert np.allclose(got[2][pure][:, :3], mirror_colour * shown, rtol=1e-5, atol=0)
    print("%s: %d pure mirror pixels; what they show has albedo %.3f .. %.3f" % (name, int(pure.sum()), shown.min(), shown.max()))


def test_the_glass_branches(A, api, O):
    """The Cornell box's glass ball with colours of its own (reflection 0.9 0.8 0.7, transmission 0.6 0.7 0.8; the scene's are white).  At 0 guide bounces a pure
    pixel on the ball holds (1, 1, 1): glass the walk ends on multiplies by nothing.  At 1 bounce the ray enters (x transmission colour) and ends on the glass again,
    from inside: the transmission colour alone.  At 2 bounces it leaves (x transmission colour again) and ends on what lies behind: transmission^2 x that surface's
    colour.  The restatement is bsdf_sample_delta at u = 0.5 in double (tests/denoise_albedo_restatement.py, walk); 28 of the 28 pixels wholly on the ball are pure
    on the oracle at every bounce count."""
    G = 4
    handle = _plain(A, api, A.CB_DEFAULT_SCENE, W, H)
    base = handle.c
    assert base.materials[base.surfaces[6].material].kind == A.MATERIAL_GLASS
    glass = A.Material.from_buffer_copy(base.materials[base.surfaces[6].material])
    refl, trans = (0.9, 0.8, 0.7), (0.6, 0.7, 0.8)
    for j in range(3):
        glass.color0[j], glass.color1[j] = refl[j], trans[j]
    scene, _ = X.copy_scene(A, base, {6: glass})
    t = np.array(trans, np.float32)
    for bounces in (0, 1, 2):
        with api.Frame(scene, api.make_params(W, H, 48), noise=True, guide_bounces=bounces, albedo=G) as f:
            f.render(16)
            got = f.albedo()
        want, clean, first = DA.albedo(O, A, scene, [], W, H, G, bounces=bounces)
        pure = (first == 6).all(axis=2) & clean & (want[..., 3] == G * G)
        assert pure.sum() >= 20, (bounces, int(pure.sum()))
        err = np.abs(got[pure][:, :3].astype(np.float64) - want[pure][:, :3])
        assert (err <= REL * np.abs(want[pure][:, :3].astype(np.float64))).all(), (bounces, float(err.max()))
        assert np.array_equal(got[pure][:, 3], want[pure][:, 3])
        if bounces == 0:
            assert (got[pure][:, :3] == 1).all()
        elif bounces == 1:
            assert (np.abs(got[pure][:, :3].astype(np.float64) - t) <= REL * t).all()   # (sixteen float32 additions of 0.6 do not sum to 9.6 exactly)
        else:   # transmission^2 x the colour behind, which differs from pixel to pixel
            assert (np.abs(got[pure][:, :3].astype(np.float64) - t) > 0.01).any(axis=1).all() and len(np.unique(got[pure][:, :3], axis=0)) >= 3
        print("glass ball, %d guide bounces: %d pure pixels, albedo %.4f .. %.4f" % (bounces, int(pure.sum()), got[pure][:, :3].min(), got[pure][:, :3].max()))


def _restated(f, scene, w, h, total, params, bounces, n=None, batches=None, state=None, **tile):
    """The restatement's film for the frame as it stands: its checkpoint, its own guides, keys and albedo -> (film [h, w, 3], guide B, the gather's cv)"""
    n_pix = T._n_pix(w, h, **tile)
    done, accum, flags, (nb, n_prev, y_prev, m2) = R.split_state(f.save() if state is None else state, n_pix)
    cv = T._to_film(D.gather(accum, flags, m2, total, done if n is None else n, nb if batches is None else batches), w, h, **tile)
    ga, gb = f.guides()
    key = f.guide_chains() if bounces > 0 else None
    out = DA.denoise(cv, ga, gb, f.albedo(), D.pixel_width(DA.scene_c(scene).camera, w), key=key, **params)
    return np.clip(out[..., :3], 0.0, 1.0), gb, cv


def _compare(got, want, gb, cv, levels):
    """tests/test_denoise_albedo.py's bound, rtol = (levels + 2) x 2^-23 with atol = 0; pass-through pixels to the bit"""
    surface = gb[..., 3] == D.SURFACE
    assert np.array_equal(got[~surface], np.clip(cv[..., :3], 0, 1)[~surface])
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = float((err / np.maximum(want.astype(np.float64), 1e-300)).max())
    assert (err <= (levels + 2) * 2.0 ** -23 * want.astype(np.float64)).all(), rel
    return rel


KERNEL_CASES = [("textured", 40, 24, 16, 16, 0), ("textured", 44, 21, 8, 8, 2), ("textured", 264, 40, 16, 16, 0), ("untextured", 40, 24, 16, 16, 2)]


@pytest.mark.parametrize("which,w,h,tile_w,tile_h,bounces", KERNEL_CASES, ids=["%s_%dx%d_tile_%dx%d_bounces_%d" % c for c in KERNEL_CASES])
def test_kernels_against_the_restatement(which, w, h, tile_w, tile_h, bounces, A, api):
    """The demodulating gather, the levels and the remodulating add against the restatement fed the frame's own state; levels 1, 3 and 5; the plain and the keyed
    level kernels.  Measured on the MI355X: the largest relative difference is 0 in all four cases (printed); DESIGN.md "Albedo"."""
    if which == "textured":
        scene, textures, tx = _case(A, api, w, h)
    else:
        scene, textures, tx = _plain(A, api, A.CB_DEFAULT_SCENE, w, h), [], None
    tile = dict(tile_w=tile_w, tile_h=tile_h)
    worst = 0.0
    with api.Frame(scene, api.make_params(w, h, 48, **tile), noise=True, textures=tx, guide_bounces=bounces, albedo=4) as f:
        while f.render(16) < f.total:
            pass
        for levels in (1, 3, 5):
            params = dict(D.DEFAULTS, levels=levels)
            got = f.denoise(params)
            want, gb, cv = _restated(f, scene, w, h, 48, params, bounces, **tile)
            assert (gb[..., 3] == D.SURFACE).sum() > 400 and not np.array_equal(got, f.resolve(normalise=True))
            worst = max(worst, _compare(got, want, gb, cv, levels))
    print("largest relative |demodulated denoise - restatement| (%s %d x %d, tile %d x %d, %d bounces): %.3e" % (which, w, h, tile_w, tile_h, bounces, worst))


def test_adaptive_frame(A, api):
    """Retired blocks stand at their own counts in the demodulating gather too"""
    scene, textures, tx = _case(A, api, W, H)
    with api.Frame(scene, api.make_params(W, H, SPP), noise=True, blocks=True, textures=tx, albedo=4) as f:
        done, st = f.render_adaptive(T.THRESHOLD, T.FRACTION, T.MIN_BATCHES, 100)
        prefix, n, nb, state = T._block_counts(f, done)
        assert len(set(n[n > 0].tolist())) >= 2, sorted(set(n.tolist()))
        got = f.denoise()
        want, gb, cv = _restated(f, scene, W, H, SPP, D.DEFAULTS, 0, n=n, batches=nb, state=prefix)
        rel = _compare(got, want, gb, cv, D.DEFAULTS["levels"])
        assert np.array_equal(f.denoise(dict(levels=0)), f.resolve(normalise=True))
        print("adaptive textured frame: blocks at %s samples; largest relative |denoise - restatement| %.3e" % (sorted(set(n[n > 0].tolist())), rel))


def test_identity(A, api):
    """Grid 0 is the frame that never heard of an albedo, to the byte; two calls at grid 4 return identical bytes; levels = 0 is resolve(normalise=True)"""
    scene, textures, tx = _case(A, api, W, H)
    p = api.make_params(W, H, SPP)
    films = {}
    for name, kw in (("never", {}), ("zero", dict(albedo=0)), ("four", dict(albedo=4))):
        with api.Frame(scene, p, noise=True, textures=tx, **kw) as f:
            if name == "zero":
                f.set_albedo_grid(0)
            assert f.render(100) == 112 and f.render(100) == 224
            before = f.save()
            films[name] = f.denoise()
            assert np.array_equal(f.denoise(), films[name]) and f.save() == before
            assert np.array_equal(f.denoise(dict(levels=0)), f.resolve(normalise=True))
            assert f.albedo_grid == (4 if name == "four" else 0)
    assert films["never"].tobytes() == films["zero"].tobytes()
    assert not np.array_equal(films["four"], films["never"])


SEEDS = (1234, 101, 202)
_truth = {}


def _converged(A, api):
    """api.render(textures=...) at 16 384 samples, and the textured first-hit pixels (the oracle's first hit of the pixel centre), once.  Never modified."""
    if not _truth:
        from oracle import kyoracle as O
        scene, textures, tx = _case(A, api, W, H)
        film = api.render(scene, api.make_params(W, H, 16384, seed=987654), textures=tx)
        film.setflags(write=False)
        first = DA.albedo(O, A, scene, textures, W, H, 1, check_clean=False)[2][..., 0]
        materials = {t.material for t in textures}
        textured = np.isin(first, [s for s in range(scene.scene.surface_count) if scene.scene.surfaces[s].material in materials])
        _truth["film"], _truth["textured"] = film, textured
    return _truth["film"], _truth["textured"]


@pytest.mark.parametrize("seed", SEEDS)
def test_it_denoises(seed, A, api):
    """The textured cornell_case 40 x 24 at 112 and 224 samples, one chunk per pass: over the 320 pixels whose centre first hits a textured surface, the RMSE of
    denoise() with albedo=4 against api.render(textures=...) at 16 384 samples lies BELOW the same frame's albedo=0 denoise and BELOW resolve(normalise=True).  The
    condition is "below"; the ratios are printed and stand in DESIGN.md "Albedo" next to the CPU replay's (tools/denoise_replay.py albedo).  Measured on the MI355X:
    demodulated / today's 0.875 0.815 (seed 1234), 0.831 0.845 (101), 0.801 0.757 (202); demodulated / raw 0.749 0.850, 0.726 0.835, 0.561 0.726."""
    truth, sel = _converged(A, api)
    assert int(sel.sum()) == 320
    truth = truth.astype(np.float64)
    rmse = lambda film: float(np.sqrt((((film.astype(np.float64) - truth) ** 2)[sel]).mean()))
    scene, textures, tx = _case(A, api, W, H)
    p = api.make_params(W, H, SPP, seed=seed)
    with api.Frame(scene, p, noise=True, textures=tx) as plain, api.Frame(scene, p, noise=True, textures=tx, albedo=4) as demod:
        for at in (112, 224):
            for f in (plain, demod):
                while f.render(1) < at:
                    pass
                assert f.done == at
            assert np.array_equal(plain.resolve(normalise=True), demod.resolve(normalise=True))
            raw, today, mine = rmse(plain.resolve(normalise=True)), rmse(plain.denoise()), rmse(demod.denoise())
            print("seed %d at %d samples, textured pixels: RMSE raw %.5f today's filter %.5f demodulated %.5f: / today's %.3f, / raw %.3f" % (
                seed, at, raw, today, mine, mine / today, mine / raw))
            assert mine < today and mine < raw, (seed, at, raw, today, mine)


def test_under_a_filter_and_a_lens(A, api, O):
    """A tent of radius 2 and tests/test_lens_gpu.py's lens: the sub-sample rays go through the filter's warp and the lens (filter_restatement.warp,
    lens_restatement.disk / lens_ray), the albedo equals the restatement under the first test's bound and cap, and levels = 0 is resolve.  Not clean on the oracle's
    own frames: tent 18 of 960 (1.9 %: its sub-samples spread over five pixels; counted on the CPU before any GPU run), lens 6, both 12 (with the lens tests' focus,
    which a GPU KAT finds; 8 and 10 on the CPU with the same radius focused at 3.5)."""
    import test_lens_gpu as TL
    scene, textures, tx = _case(A, api, W, H)
    lens, radius, focus = TL.lens_of(O, A, api, "cornell", W, H)
    tent = api.pixel_filter(A.FILTER_TENT, 2.0)
    for what, kw, rs in (("tent", dict(filter=tent), dict(flt=F.Filter(F.TENT, 2.0))), ("lens", dict(lens=lens), dict(lens=(radius, focus))),
                         ("tent and lens", dict(filter=tent, lens=lens), dict(flt=F.Filter(F.TENT, 2.0), lens=(radius, focus)))):
        with api.Frame(scene, api.make_params(W, H, 48), noise=True, textures=tx, albedo=4, **kw) as f:
            _two_passes(f)
            got = f.albedo()
            assert np.array_equal(f.denoise(dict(levels=0)), f.resolve(normalise=True))
            assert np.isfinite(f.denoise()).all()
        want, clean, _ = DA.albedo(O, A, scene, textures, W, H, 4, **rs)
        _compare_albedo(got, want, clean, what)
    with api.Frame(scene, api.make_params(W, H, 48), noise=True, textures=tx, albedo=4) as f:   # ... and they are seen
        f.render(16)
        assert not np.array_equal(f.albedo(), got)


def test_refusals(A, api):
    scene, textures, tx = _case(A, api, W, H)
    p = api.make_params(W, H, SPP)
    with api.Frame(scene, p, noise=True, textures=tx) as f, api.Frame(scene, p, noise=True, textures=tx) as ref:
        for g in (f, ref):
            assert g.render(100) == 112 and g.render(100) == 224
        for bad in (-1, 9):
            with pytest.raises(api.KyError, match="albedo grid"):
                f.set_albedo_grid(bad)
        assert f.albedo_grid == 0
        with pytest.raises(api.KyError, match="no albedo"):
            f.albedo()
        assert f.albedo_ms() < 0
        want = ref.denoise()
        assert np.array_equal(f.denoise(), want)              # every refusal so far left the next denoise what it is
        with pytest.raises(api.KyError, match="guides are traced"):
            f.set_albedo_grid(4)                              # the guides are traced: the grid stays
        f.set_albedo_grid(0)                                  # (the value held is fine)
        assert f.albedo_grid == 0 and np.array_equal(f.denoise(), want)
    with api.Frame(scene, p, noise=True, textures=tx, albedo=4) as f:
        assert f.render(100) == 112 and f.render(100) == 224
        first = f.denoise()
        with pytest.raises(api.KyError, match="guides are traced"):
            f.set_albedo_grid(2)
        with pytest.raises(api.KyError, match="guides are traced"):
            f.set_guide_bounces(2)
        f.set_albedo_grid(4)
        assert f.albedo_grid == 4 and np.array_equal(f.denoise(), first)
        lib = A.load_kyhip()
        buf = np.full((H, W, 4), 7.0, np.float32)
        assert lib.kyhip_frame_albedo(f._f, None, W) == A.KY_ERR_INVALID_VALUE
        assert lib.kyhip_frame_albedo(f._f, C.c_void_p(buf.ctypes.data), W - 1) == A.KY_ERR_INVALID_VALUE and (buf == 7).all()
    with api.Frame(scene, api.make_params(W, H, SPP, tile_first=0, tile_step=2), noise=True, textures=tx, albedo=4) as f:   # a shard
        f.render(100)
        f.render(100)
        with pytest.raises(api.KyError, match="shard"):
            f.albedo()
        with pytest.raises(api.KyError, match="shard"):
            f.denoise()
    with api.Frame(scene, p, textures=tx, albedo=4) as f:     # no noise tracking
        f.render(100)
        with pytest.raises(api.KyError, match="kyhip error -1"):
            f.albedo()


def test_albedo_ms(A, api):
    scene, textures, tx = _case(A, api, W, H)
    with api.Frame(scene, api.make_params(W, H, SPP), noise=True, textures=tx, albedo=4) as f:
        assert f.albedo_ms() < 0
        f.render(100)
        f.render(100)
        assert f.albedo_ms() < 0                              # no call yet
        f.guides()                                            # the albedo is traced when the guides are
        a0 = f.albedo_ms()
        assert a0 > 0 and f.denoise_ms()[0] > 0
        f.albedo()
        f.denoise()
        f.render(100)
        f.denoise()
        assert f.albedo_ms() == a0                            # set once per frame


def test_host_classes(A, api):
    """integrator_t::render_denoised(..., guide_bounces, albedo_grid) through the C API of the host classes is the frame's denoise() with that grid"""
    scene = _plain(A, api, A.CB_DEFAULT_SCENE, W, H)
    args = (scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, SPP, W, H)
    film, done = api.render_denoised_host_api(*args, 100, 200, guide_bounces=2, albedo=4)
    off, _ = api.render_denoised_host_api(*args, 100, 200, guide_bounces=2, albedo=0)
    with api.Frame(scene, api.make_params(W, H, SPP), noise=True, guide_bounces=2, albedo=4) as f, \
            api.Frame(scene, api.make_params(W, H, SPP), noise=True, guide_bounces=2) as g:
        for fr in (f, g):
            assert fr.render(100) == 112 and fr.render(100) == 224 == done
        assert np.array_equal(f.denoise(), film) and np.array_equal(g.denoise(), off) and not np.array_equal(film, off)
    with pytest.raises(api.KyError, match="albedo grid"):
        api.render_denoised_host_api(*args, 100, 200, albedo=9)
