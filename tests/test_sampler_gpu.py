"""GPU: the device's random-number streams (kyhip_kat_sampler / kyhip_smallpt_kat_rng run the product's own sampler_pixel_key, sampler_start, sampler_next
and sp_rng_start, sp_next) against the NumPy restatements of tests/sampler_restatement.py, which share no code with them: bit for bit, zero differences.

The key sets include the two of tests/test_sampler.py's statistics battery in full, so the verdict reached there on the restatement's numbers holds for
the device's numbers without being computed again.  Then: the key convention of the KAT is tied to the one the render kernels use (path_begin), and the
whole path's expectation is compared with the oracle run under a foreign generator (tests/sampler_expectation.py)."""
import numpy as np
import pytest

import sampler_expectation as E
import sampler_restatement as R

pytestmark = pytest.mark.gpu
K = 256


def _decodes(bits, words):
    """Every pattern is a float in [0, 1) whose value is exactly (word >> 9) 2^-23."""
    f = bits.view(np.float32)
    assert np.all(f >= 0) and np.all(f < 1)
    assert np.array_equal((f.astype(np.float64) * 2.0 ** 23).astype(np.uint32), words >> np.uint32(9))


@pytest.mark.parametrize("name", sorted(R.BATTERY_SETS))
def test_device_streams_equal_the_restatement_on_the_battery_sets(api, name):
    w, h, spp, k = R.BATTERY_SETS[name]
    keys = R.frame_keys(w, h, spp)
    got = api.kat_sampler(R.BATTERY_SEED, keys, k)
    words = R.stream_words(R.BATTERY_SEED, keys, k)
    assert int(np.count_nonzero(got != R.words_to_float(words).view(np.uint32))) == 0
    _decodes(got, words)


@pytest.mark.parametrize("seed", R.EDGE_SEEDS)
def test_device_streams_equal_the_restatement_on_edge_keys(api, seed):
    keys = R.edge_keys(seed)
    got = api.kat_sampler(seed, keys, K)
    words = R.stream_words(seed, keys, K)
    assert int(np.count_nonzero(got != R.words_to_float(words).view(np.uint32))) == 0
    _decodes(got, words)
    assert np.all(api.kat_sampler(seed, keys, K, debug=True).view(np.float32) == np.float32(0.5))


def test_device_streams_equal_the_restatement_on_random_keys(api):
    """2^16 + 37 keys: many workgroups and a ragged last one; k = 1 and k = 255 beside 256."""
    gen = np.random.default_rng(20260102)
    keys = gen.integers(0, 1 << 32, size=((1 << 16) + 37, 2), dtype=np.uint64).astype(np.uint32)
    seed = int(gen.integers(0, 1 << 32))
    want = R.stream_bits(seed, keys, K)
    assert int(np.count_nonzero(api.kat_sampler(seed, keys, K) != want)) == 0
    assert np.array_equal(api.kat_sampler(seed, keys[:300], 255), want[:300, :255])
    assert np.array_equal(api.kat_sampler(seed, keys[:300], 1), want[:300, :1])


def test_sampler_kat_refuses_bad_arguments(api):
    keys = R.edge_keys(1)
    for k in (0, 257):
        with pytest.raises(api.KyError):
            api.kat_sampler(1, keys, k)
    with pytest.raises(api.KyError):
        api.smallpt_kat_rng(1, keys, 257)


@pytest.mark.parametrize("seed", R.EDGE_SEEDS)
def test_smallpt_streams_equal_the_restatement(api, seed):
    """The fp64 path's splitmix64 streams: edge keys, and (seed 1234) the key set of the CPU battery's smallpt statistics and random keys."""
    sets = [R.edge_keys(seed)]
    if seed == R.BATTERY_SEED:
        gen = np.random.default_rng(20260103)
        sets += [R.frame_keys(16 * 4, 16, 64)[:, :], gen.integers(0, 1 << 32, size=((1 << 14) + 5, 2), dtype=np.uint64).astype(np.uint32)]
    for keys in sets:
        k = K if keys.shape[0] < (1 << 15) else 16
        got = api.smallpt_kat_rng(seed, keys, k)
        words = R.sp_stream_words(seed, keys, k)
        assert int(np.count_nonzero(got != R.sp_words_to_double(words).view(np.uint64))) == 0
        d = got.view(np.float64)
        assert np.all(d >= 0) and np.all(d < 1)
        assert np.array_equal((d * 2.0 ** 53).astype(np.uint64), words >> np.uint64(11))


def test_render_path_addresses_the_streams_as_the_kat_does(A, api):
    """On 8 pixels of a 90 x 70 frame the first vertex of kyhip_kat_li_trace is the hit of the camera ray through (x + u0, y + u1), u0 and u1 being the
    RESTATEMENT's first two numbers of the key (seed, y W + x, s): path_begin keys its stream as the sampler KAT does and spends the first two numbers on
    the camera sample.  (Both engines run the same path_begin; test_engines_agree covers the rest.)

    Tolerances: the direction is one normalised fp32 vector computed by the same function in two kernels -- 2e-6 is 16 units in its last place, while half a
    pixel of the 90-wide film turns it by 5e-3; the position o + t d is held to 1e-4 of the scene's size, the agreement tests/test_mismatch_gpu.py asks
    of two traces of one sample."""
    w, h, seed = 90, 70, 1234
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    params = api.make_params(w, h, 512, seed=seed)
    gen = np.random.default_rng(8)
    cand = [(int(gen.integers(0, w)), int(gen.integers(0, h)), s) for s in (0, 1, 2, 7, 63, 64, 300, 511) * 3]
    seen = 0
    for x, y, s in cand:
        rows, _ = api.kat_li_trace(scene, params, x, y, s)
        if rows.shape[0] == 0 or rows[0, 0] != 0:
            continue   # the camera ray left the scene or ended on the lamp: no vertex is traced
        u = R.stream_floats(seed, np.array([[y * w + x, s]], np.uint32), 2)[0]
        pf = np.array([[np.float32(x) + u[0], np.float32(y) + u[1]]], np.float32)
        ray = np.concatenate([api.kat_camera(scene.c.camera, pf), np.full((1, 1), np.inf, np.float32)], axis=1)
        hit = api.kat_scene_intersect(scene, ray)[0]
        assert hit[0] == 1 and int(hit[8]) == int(rows[0, 1])
        assert np.abs(rows[0, 9:12] + ray[0, 3:6]).max() <= 2e-6                      # wo = -d
        size = max(1.0, float(np.abs(hit[2:5]).max()), float(np.abs(ray[0, :3]).max()))
        assert np.abs(rows[0, 3:6] - hit[2:5]).max() <= 1e-4 * size
        seen += 1
        if seen == 8:
            break
    assert seen == 8


# ---- expectation under a foreign generator ----

_samples = {}


def _scene_samples(O, A, api, name):
    """(the GPU's samples on its own streams, the oracle's under the Mersenne Twister's tape), computed once per scene and left unchanged."""
    if name not in _samples:
        gpu = E.own_samples(api.kat_li, A, api, name)
        tape, most = E.tape_samples(O, A, api, name)
        print("%s: most numbers one sample drew %d of %d" % (name, most, E.SCENES[name][2]))
        _samples[name] = (gpu, tape)
    return _samples[name]


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_expectation_agrees_with_the_oracle_under_a_foreign_generator(O, A, api, name):
    """Per pixel a Welch z between the GPU's 2048 samples and the tape-fed oracle's, on the luminance of min(Li, 1) and of min(Li, 32): sum z^2 at most
    the 1 - 1e-4 quantile of chi-square with as many degrees of freedom as pixels counted (115 at 64), max |z| <= 4.5, and a pixel without variance on
    either side has equal means.  Measured oracle against oracle (the reference's own spread; the GPU's samples are the oracle's but for a few decisions
    per million): Cornell 87 / 80, 4.1; Veach 68 / 71, 3.0; environment 60 / 60, 2.7; point 79 / 79, 2.9."""
    gpu, tape = _scene_samples(O, A, api, name)
    assert np.isfinite(gpu).all()
    ok, lines = E.check(gpu, tape, name)
    print("\n".join(lines))
    assert ok, lines


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_consecutive_samples_of_a_pixel_behave_as_independent_draws(O, A, api, name):
    """m var(means of m consecutive samples) / var(samples), averaged over the pixels, for m = 2, 8, 32, within 4.5 deviations of its own permutation null
    (the same values shuffled within each pixel, 200 shuffles): the independence ky_noise and the retire rule assume.  A weak detector -- it needs
    dependence strong enough to move the variance of short runs; measured on the oracle's samples: between -1.6 and +1.3 deviations."""
    gpu, _ = _scene_samples(O, A, api, name)
    for m, (dev, ratio, mean, sd) in E.batch_means_deviations(E.luminance(gpu, 32.0)).items():
        print("%s m = %d: ratio %.4f, null %.4f +- %.4f: %+.2f deviations" % (name, m, ratio, mean, sd, dev))
        assert abs(dev) <= 4.5, (name, m, dev)
