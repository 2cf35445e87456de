"""A frame's per-pixel noise estimate (include/kyhip.h, kyhip_frame_track_noise ...; DESIGN.md "Noise"): batch means over the frame's passes, kept by film-sized
kernels of their own (ky_amd/csrc/ky_noise.hip).  A tracking frame's film stays the one-shot film bit for bit; the kernels' values are compared with the NumPy
float64 restatement of tests/noise_restatement.py on the accumulators read out of checkpoints; and the estimate is compared with what it claims to measure, the
spread of the picture across seeds."""
import ctypes as C

import numpy as np
import pytest

import noise_restatement as R

pytestmark = pytest.mark.gpu

W, H = 40, 24   # 16 x 16 tiles: ragged tiles on the right and at the bottom
N_PIX = 6 * 256
LUM = np.array([0.212671, 0.715160, 0.072169])


def _scene(A, api, which, w=W, h=H):
    if which == "cornell":
        return api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    if which == "veach":
        return api.mis_scene(w, h)
    if which == "environment":
        return api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT, w, h)
    raise KeyError(which)


_one_shot = {}


def _reference(A, api, which, spp, w=W, h=H, **over):
    """api.render of the scene, once per (scene, params).  Never modified."""
    key = (which, spp, w, h, tuple(sorted(over.items())))
    if key not in _one_shot:
        film = api.render(_scene(A, api, which, w, h), api.make_params(w, h, spp, **over))
        film.setflags(write=False)
        _one_shot[key] = film
    return _one_shot[key]


def _saturating_scene(A, api, spp):
    """tests/test_frame_gpu.py::test_saturation_carries_across_passes's lamp: radiance 4 T, T the frame's term limit."""
    lib = A.load_kyhip()
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, spp)
    T = C.c_float(0)
    assert lib.kyhip_film_term_limit(C.byref(p), scene.c.light_count, 0, 0, C.byref(T)) > 0 and T.value >= 1
    for ch in range(3):
        scene.c.lights[0].color[ch] = 4.0 * T.value
    return scene, p


def _to_film(values, w=W, h=H, fill=0.0, **shard):
    """Compact tile order -> (h, w), padding dropped, pixels the shard does not own = fill."""
    x, y, inside = R.pixel_xy(len(values), w, h, **shard)
    out = np.full((h, w), fill, values.dtype)
    out[y[inside], x[inside]] = values[inside]
    return out


@pytest.mark.parametrize("spp", [500, 7])
@pytest.mark.parametrize("which", ["cornell", "veach", "environment"])
def test_a_tracking_frame_is_the_one_shot_film(which, spp, A, api):
    want = _reference(A, api, which, spp)
    scene = _scene(A, api, which)
    for min_samples in (1, 100):
        with api.Frame(scene, api.make_params(W, H, spp), noise=True) as f:
            while f.render(min_samples) < f.total:
                pass
            assert np.array_equal(f.resolve(), want), (which, spp, min_samples)


def test_state_sizes(A, api):
    scene = _scene(A, api, "cornell")
    with api.Frame(scene, api.make_params(W, H, 7)) as f:
        f.render(1)
        assert len(f.save()) == R.HEADER_BYTES + N_PIX * 28      # a frame that does not track: today's state
        with pytest.raises(api.KyError, match="kyhip error -1"):
            f.noise()
        with pytest.raises(api.KyError, match="kyhip error -1"):
            f.noise_stats(0.1)
        with pytest.raises(api.KyError, match="kyhip error -1"):
            f.render_until(0.1)
        assert A.load_kyhip().kyhip_frame_track_noise(f._f) == A.KY_ERR_INVALID_VALUE   # something is rendered
        assert A.load_kyhip().kyhip_frame_noise_ms(f._f, None, None) == A.KY_ERR_INVALID_VALUE
    with api.Frame(scene, api.make_params(W, H, 7), noise=True) as f:
        assert len(f.save()) == R.HEADER_BYTES + N_PIX * 28 + R.TRAILER_BYTES + N_PIX * 16
        lib, up, ms = A.load_kyhip(), C.c_float(7), C.c_float(7)
        assert lib.kyhip_frame_noise_ms(f._f, C.byref(up), C.byref(ms)) == A.KY_OK and up.value < 0 and ms.value < 0   # no pass, no map yet
        f.render(1)
        assert lib.kyhip_frame_noise_ms(f._f, C.byref(up), C.byref(ms)) == A.KY_OK and up.value > 0 and ms.value < 0
        f.noise_stats(0.1)
        assert lib.kyhip_frame_noise_ms(f._f, C.byref(up), None) == A.KY_OK and lib.kyhip_frame_noise_ms(f._f, None, C.byref(ms)) == A.KY_OK and ms.value > 0


@pytest.mark.parametrize("which,spp,min_samples", [("cornell", 500, 100), ("veach", 500, 1), ("environment", 7, 1)])
def test_estimator_against_its_restatement(which, spp, min_samples, A, api):
    """y_prev, m2 (the checkpoint's trailer) and the map (f.noise()) after every pass against NumPy float64 on the accumulators of the same checkpoint.
    y_prev: the same IEEE operations in the same order, no contraction: equal.  m2 and the map's double value: the same, where the device's double division and
    square root round correctly; 1e-12 relative allows them a few ulp each.  The map: the issue's bound is 1e-7 + 1e-5 * value (double rounding about 1e-9
    relative, the difference of near-constant pixels up to 1e-8 of white); tightened here to what the number formats give -- two double values that agree to
    1e-12 round to the same float32 or to neighbours, one float32 ulp, 1.2e-7 * value.  Measured on the MI355X: the largest relative difference is 0 in all
    three cases (every pixel's float32 equals the restatement's), so the one-ulp bound stands as the tight one; the test prints the figure."""
    scene = _scene(A, api, which)
    worst = 0.0
    with api.Frame(scene, api.make_params(W, H, spp), noise=True) as f:
        accums, dones = [], []
        while f.done < f.total:
            dones.append(f.render(min_samples))
            done, accum, flags, (batches, n_prev, y_prev, m2) = R.split_state(f.save(), N_PIX)
            accums.append(accum)
            assert (done, batches, n_prev) == (dones[-1], len(dones), dones[-1])
            want_y, want_m2, want_map = R.run(accums, dones, spp, flags)[-1]
            assert np.array_equal(y_prev, want_y)
            assert np.allclose(m2, want_m2, rtol=1e-12, atol=0) and (m2 >= 0).all()
            got = f.noise()
            want = _to_film(want_map)
            if len(dones) == 1:
                assert np.isinf(got).all() and np.isinf(want).all()
                continue
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            worst = max(worst, float((err / np.maximum(want, 1e-30)).max()))
            assert (err <= 1e-7 + 1e-5 * want).all()       # the issue's bound
            assert (err <= 1.2e-7 * want).all(), float((err / np.maximum(want, 1e-30)).max())
    print("largest relative |map - restatement| (%s, %d spp): %.3e" % (which, spp, worst))
    assert len(dones) >= 2


def test_a_shard_writes_its_own_pixels_only(A, api):
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, 7, tile_first=1, tile_step=2)
    n_pix = 3 * 256
    with api.Frame(scene, p, noise=True) as f:
        while f.render(1) < f.total:
            pass
        big = np.full((H, W + 8), -5.0, np.float32)
        got = f.noise(out=big[:, :W])
        done, accum, flags, (batches, n_prev, y_prev, m2) = R.split_state(f.save(), n_pix)
        st = f.noise_stats(0.0)
    assert (big[:, W:] == -5).all()                                  # beyond the rows' width: the ragged tiles' padding goes nowhere
    want = _to_film(R.value(y_prev, m2, batches, done, flags), fill=-5.0, tile_first=1, tile_step=2)
    own = want != -5
    assert own[:16, 16:32].all() and not own[:16, :16].any()         # tile 1 is this shard's, tile 0 the other one's
    assert (got[~own] == -5).all() and (got[own] >= 0).all()
    assert np.allclose(got[own], want[own], rtol=1.2e-7, atol=0)
    x, y, inside = R.pixel_xy(n_pix, W, H, tile_first=1, tile_step=2)
    assert st.pixels == int(inside.sum()) == int(own.sum()) and st.pixels < n_pix


def test_edges(A, api):
    scene = _scene(A, api, "cornell")
    with api.Frame(scene, api.make_params(W, H, 1), noise=True) as f:   # one sample: one batch
        done, st = f.render_until(0.5, 1.0, 2, 1)
        assert done == 1 == f.total and st.batches == 1 and st.above == st.pixels == W * H and np.isinf(st.max)   # complete, and nothing claims to be clean
        assert np.isinf(f.noise()).all()
    with api.Frame(scene, api.make_params(W, H, 7), noise=True) as f:   # chunks of 4 and 3
        assert f.render(1) == 4 and np.isinf(f.noise()).all()
        assert f.render(1) == 7
        m = f.noise()
        assert np.isfinite(m).all() and (m >= 0).all() and m.max() > 0
    with api.Frame(scene, api.make_params(W, H, 500, sampler=0), noise=True) as f:   # the debug sampler: every sample of a pixel is the same (measured: 4.5e-8)
        while f.render(100) < f.total:
            pass
        m = f.noise()
        print("debug sampler: largest map value %.3e" % m.max())
        assert (m <= 1e-6).all()
    scene, p = _saturating_scene(A, api, 7)
    with api.Frame(scene, p, noise=True) as f:
        while f.render(1) < f.total:
            pass
        m = f.noise()
        st = f.noise_stats(0.01)
        _, _, flags, _ = R.split_state(f.save(), N_PIX)
    flagged = _to_film(((flags & 0x1FF) != 0).astype(np.float32)) > 0
    assert st.flagged == int(flagged.sum()) > 0 and (m[flagged] == 0).all() and (m[~flagged] > 0).any()


@pytest.mark.parametrize("which", ["cornell", "saturating"])
def test_statistics_are_a_reduction_of_the_map(which, A, api):
    if which == "saturating":
        scene, p = _saturating_scene(A, api, 7)
    else:
        scene, p = _scene(A, api, "cornell"), api.make_params(W, H, 64)
    with api.Frame(scene, p, noise=True) as f:
        f.render(1)
        first = f.noise_stats(0.25)
        assert first.batches == 1 and first.above == first.pixels - first.flagged > 0 and np.isinf(first.max)   # one batch: every pixel is above anything
        while f.render(1) < f.total:
            pass
        m = f.noise()
        _, _, flags, _ = R.split_state(f.save(), N_PIX)
        flagged = _to_film(((flags & 0x1FF) != 0).astype(np.float32)) > 0
        good = m[~flagged]
        for threshold in (0.0, float(np.median(good)), float(good.max()), 1e9):
            a, b = f.noise_stats(threshold), f.noise_stats(threshold)
            assert bytes(a) == bytes(b)
            assert (a.batches, a.samples_done, a.pixels, a.flagged) == (len(api.pass_boundaries(p.samples_per_pixel)), f.total, W * H, int(flagged.sum()))
            assert a.above == int((good > np.float32(threshold)).sum()) and a.max == good.max() and a.threshold == np.float32(threshold)
            assert abs(a.mean - good.astype(np.float64).mean()) <= 1e-12 * a.mean
    assert (which == "saturating") == (a.flagged > 0)


W5 = H5 = 32
SEED_SETS = [range(100, 116), range(200, 216), range(300, 316)]
_conv = {}


def _converging(A, api):
    """Cornell 32 x 32, 500 spp, one chunk per pass: the maps at 112 and at 500 samples and the film."""
    if not _conv:
        with api.Frame(_scene(A, api, "cornell", W5, H5), api.make_params(W5, H5, 500), noise=True) as f:
            while f.render(1) < 112:
                pass
            assert f.done == 112
            _conv["map112"] = f.noise()
            while f.render(1) < f.total:
                pass
            _conv["map500"] = f.noise()
        for n in (112, 500):
            print("map at %d samples: quartile %.5f median %.5f 90th percentile %.5f" % ((n,) + tuple(np.quantile(_conv["map%d" % n], [0.25, 0.5, 0.9]))))
    return _conv


def _ratio(A, api, noise_map, spp, seeds):
    """sqrt(mean map^2) over sqrt(mean across-seed variance of the luminance of api.render at `spp`), over the pixels no seed clamps."""
    scene = _scene(A, api, "cornell", W5, H5)
    films = np.stack([api.render(scene, api.make_params(W5, H5, spp, seed=s)).astype(np.float64) for s in seeds])
    free = (films < 1).all(axis=(0, 3))
    var = (films @ LUM).var(axis=0, ddof=1)
    assert free.sum() > W5 * H5 // 2
    return float(np.sqrt((noise_map.astype(np.float64)[free] ** 2).mean()) / np.sqrt(var[free].mean()))


@pytest.mark.parametrize("samples", [500, 112])
def test_it_measures_noise(samples, A, api):
    """The yardstick is api.render: at 16 seeds, per unclamped pixel, the across-seed variance of the picture's luminance -- what the map's square estimates from
    ONE frame's batches.  Measured on the MI355X, three seed sets each (the test prints them; so does tools/measure_tolerances.py):
        500 samples (51 batches): 1.0266 1.0059 0.9811   largest deviation from 1: 0.0266
        112 samples  (6 batches): 1.0405 1.0369 0.9796   largest deviation from 1: 0.0405
    The bound is three times the largest deviation seen: 0.08 at 500 samples, 0.1215 at 112.  A ratio outside [2/3, 1.5] would be a bug in the estimator, not
    a tolerance."""
    noise_map = _converging(A, api)["map%d" % samples]
    ratios = [_ratio(A, api, noise_map, samples, seeds) for seeds in SEED_SETS]
    print("noise ratio at %d samples: %s" % (samples, " ".join("%.4f" % r for r in ratios)))
    bound = {500: 3 * 0.0266, 112: 3 * 0.0405}[samples]
    for r in ratios:
        assert 2 / 3 <= r <= 1.5 and abs(r - 1) <= bound, (ratios, bound)


def test_render_until(A, api):
    want = _reference(A, api, "cornell", 500, W5, H5)
    scene = _scene(A, api, "cornell", W5, H5)
    p = api.make_params(W5, H5, 500)
    # One chunk per pass and min_batches 6, as _converging's frame was rendered: the first verdict falls at 112 samples, where this frame's map IS map112 (same
    # seed, same passes).  There 75 % of the pixels lie at or above the map's lower quartile and more above 0.9 of it: not clean, the frame goes on.
    # This frame is heavy-tailed (a 32 x 32 Cornell box with the glass and the mirror sphere): its samples replayed on the CPU oracle (tools/noise_replay.py, profiles/noise_replay.txt) show the upper half of the
    # map barely falling between 112 and 500 samples -- fireflies keep landing -- so a verdict on the 95th percentile or the median would not come before the end.
    # The lower quartile, the pixels without them, falls like 1 / sqrt(samples) at first: in that replay the share above 0.9 of map112's quartile is 0.79 at 112
    # samples, passes 0.75 at 160 and is 0.67 at 500.
    fraction = 0.75
    threshold = 0.9 * float(np.quantile(_converging(A, api)["map112"], 1 - fraction))
    bounds = api.pass_boundaries(500)
    with api.Frame(scene, p, noise=True) as f:
        done, st = f.render_until(threshold, fraction, 6, 1)
        print("render_until: stopped at %d samples, %d of %d pixels above %.4g; at 112 samples %d, at 500 samples %d" % (
            done, st.above, st.pixels, threshold, int((_converging(A, api)["map112"] > threshold).sum()), int((_converging(A, api)["map500"] > threshold).sum())))
        assert 112 < done < 500 and done in bounds and done == f.done == st.samples_done
        assert st.batches >= 6 and st.above <= fraction * (st.pixels - st.flagged) and st.pixels == W5 * H5
        early = f.resolve(normalise=True)
        while f.render(100) < f.total:
            pass
        assert np.array_equal(f.resolve(), want)
    args = (scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, 500, W5, H5)
    film, host_done = api.render_until_host_api(*args, threshold, fraction, 6, 1)
    assert host_done == done and np.array_equal(film, early)
    with api.Frame(scene, p, noise=True) as f:
        done, st = f.render_until(0.0, fraction, 2, 100)     # nothing is ever that clean
        assert done == 500 == f.done and st.above > fraction * st.pixels
        assert np.array_equal(f.resolve(), want)


def test_save_end_begin_track_load_finish(A, api):
    want = _reference(A, api, "cornell", 500)
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, 500)
    with api.Frame(scene, p, noise=True) as f:
        while f.render(100) < f.total:
            pass
        whole_map = f.noise()
    with api.Frame(scene, p, noise=True) as f:
        assert f.render(100) == 112 and f.render(100) == 224
        state = f.save()
    api.render(_scene(A, api, "veach"), api.make_params(W, H, 16))   # something else in between
    with api.Frame(_scene(A, api, "cornell"), api.make_params(W, H, 500), noise=True) as f:
        f.load(state)
        assert f.done == 224 and f.noise_stats(0.0).batches == 2
        while f.render(100) < f.total:
            pass
        assert np.array_equal(f.resolve(), want) and np.array_equal(f.noise(), whole_map)
    with api.Frame(scene, api.make_params(W, H, 500, seed=99), noise=True) as g:
        first = g.render(50)
        with pytest.raises(api.KyError, match="kyhip error -1"):
            g.load(state)
        assert g.done == first and g.noise_stats(0.0).batches == 1
    plain_bytes = R.HEADER_BYTES + N_PIX * 28
    with api.Frame(scene, p, noise=True) as g:   # a tracking frame wants the trailer, whole and standing where the header stands
        moved = bytearray(state)
        moved[plain_bytes + 12:plain_bytes + 16] = (112).to_bytes(4, "little")
        for bad in (state[:plain_bytes], state[:-1], state[:plain_bytes] + bytes(len(state) - plain_bytes), bytes(moved)):
            with pytest.raises(api.KyError, match="kyhip error -1"):
                g.load(bad)
        assert g.done == 0 and g.noise_stats(0.0).batches == 0
    with api.Frame(scene, p) as g:               # a frame that does not track ignores it
        g.load(state)
        assert g.done == 224 and len(g.save()) == plain_bytes
        while g.render(100) < g.total:
            pass
        assert np.array_equal(g.resolve(), want)
