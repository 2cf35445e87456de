"""CPU: the random-number streams against restatements that share no code with them (tests/sampler_restatement.py).

The oracle's two generators must equal the restatements bit for bit; the xoroshiro step's period is PROVED from the restatement's own step (and four
neighbouring constant triples are shown not to have it, which pins (26, 9, 13) without a fixture); a battery of statistics on the restatement's numbers
for the keying the renders use must stay inside quantiles derived from each statistic's null distribution, and every statistic of the battery is shown
to reject a named defective variant.  tests/test_sampler_gpu.py then compares the DEVICE's bits with the same restatement on the battery's own key
sets, so the verdict reached here holds for the device's numbers.

Thresholds: a family of T statistics of one kind passes if each lies inside the two-sided 1 - 1e-6 / T quantile of its null distribution -- chi-square
with the stated degrees of freedom by Wilson-Hilferty, a standard normal for r sqrt(n) (sampler_restatement.chi2_bounds / family_z).

Measured with the project's keying (profiles/sampler_battery.txt holds every figure), set "first" (seed 1234, 64 x 64 pixels x 256 samples, 32 numbers),
each family: (a) 208 .. 305 inside 149 .. 401; (b) 209 .. 303 inside the same; worst (c) 2.0, (d) 2.1, (e) 2.6, (f) 2.3 deviations, inside 5.5 - 5.7."""
import numpy as np
import pytest

import sampler_expectation as E
import sampler_restatement as R

K = 256


# ---- the oracle's generators against the restatements, bit for bit ----

@pytest.mark.parametrize("seed", R.EDGE_SEEDS)
def test_oracle_streams_equal_the_restatement_on_edge_keys(O, seed):
    keys = R.edge_keys(seed)
    assert np.array_equal(O.kat_sampler(seed, keys, K), R.stream_bits(seed, keys, K))
    assert np.array_equal(O.smallpt_kat_rng(seed, keys, K), R.sp_stream_bits(seed, keys, K))


def test_edge_keys_reach_the_zero_hash_and_both_sides_of_the_wrap():
    keys = R.edge_keys(1234).astype(np.uint64)
    h = R.pixel_key(1234, keys[:, 0])
    total = h + (keys[:, 1] * np.uint64(R.GOLDEN32) & np.uint64(R.M32))
    assert np.count_nonzero(total >= np.uint64(1 << 32)) >= 7 and np.count_nonzero(total == np.uint64(R.M32)) >= 7
    s0, s1 = R.stream_state(1234, keys[:, 0], keys[:, 1])
    assert np.count_nonzero(s0 == 0) >= 7          # lowbias32(0) = 0: the stream then lives on s1 alone, which is odd, so never the all-zero state
    assert np.all(s1 & np.uint64(1) == 1)


def test_oracle_streams_equal_the_restatement_on_random_keys(O):
    gen = np.random.default_rng(20260101)
    keys = gen.integers(0, 1 << 32, size=(1 << 16, 2), dtype=np.uint64).astype(np.uint32)
    for seed in (1234, int(gen.integers(0, 1 << 32))):
        assert np.array_equal(O.kat_sampler(seed, keys, K), R.stream_bits(seed, keys, K))
        assert np.array_equal(O.smallpt_kat_rng(seed, keys, K), R.sp_stream_bits(seed, keys, K))


def test_oracle_debug_sampler_hands_out_one_half(O):
    bits = O.kat_sampler(1234, R.edge_keys(1234), 16, debug=True)
    assert np.all(bits.view(np.float32) == np.float32(0.5))


def test_numbers_lie_on_their_grids_inside_the_unit_interval():
    keys = R.edge_keys(99)
    words = R.stream_words(99, keys, K)
    f = R.words_to_float(words)
    assert f.dtype == np.float32 and f.min() >= 0 and f.max() < 1
    assert np.array_equal((f.astype(np.float64) * 2.0 ** 23).astype(np.uint32), words >> np.uint32(9))
    d = R.sp_words_to_double(R.sp_stream_words(99, keys, K))
    assert d.min() >= 0 and d.max() < 1
    # the largest words still map below one
    assert R.words_to_float(np.array([R.M32], np.uint32))[0] == np.float32(1 - 2.0 ** -23)
    assert R.sp_words_to_double(np.array([(1 << 64) - 1], np.uint64))[0] == 1 - 2.0 ** -53


def test_restatement_fed_as_a_tape_reproduces_the_oracle_samples(O, A, api):
    """Ties the restatement to the ORDER in which the path consumes a stream (camera sample first) and kyo_li_tape to kyo_li: bit for bit."""
    scene, params = E.scene_and_params(A, api, "cornell")
    w, _, stride = E.SCENES["cornell"]
    for x, y in E.pixels("cornell")[:8]:
        keys = np.stack([np.full(256, y * w + x, np.uint32), np.arange(256, dtype=np.uint32)], axis=1)
        li, used = O.li_tape(scene, params, x, y, R.stream_floats(params.seed, keys, stride))
        assert used.min() >= 2 and used.max() <= stride
        assert np.array_equal(li.view(np.uint32), O.li(scene, params, x, y, 0, 256).view(np.uint32))


def test_tape_overrun_is_reported(O, A, api):
    scene, params = E.scene_and_params(A, api, "cornell")
    with pytest.raises(ValueError):
        O.li_tape(scene, params, 16, 16, np.full((64, 2), 0.25, np.float32))   # two numbers: the camera sample alone


# ---- full period, proved ----

def test_gf2_matrix_is_the_step():
    """The matrix built from the one-bit states acts on any state as step() does: the step is linear over GF(2)."""
    t = R.gf2_matrix()
    gen = np.random.default_rng(3)
    for _ in range(64):
        s0, s1 = (np.uint64(v) for v in gen.integers(0, 1 << 32, size=2))
        _, t0, t1 = R.step(s0, s1)
        state = int(s0) | (int(s1) << 32)
        image = sum((bin(t[i] & state).count("1") & 1) << i for i in range(64))
        assert image == int(t0) | (int(t1) << 32)


def test_xoroshiro_step_has_full_period_and_its_neighbours_do_not():
    """T^(2^64 - 1) = I and T^((2^64 - 1) / p) != I for every prime factor p of 2^64 - 1: the step's order is 2^64 - 1, every non-zero state lies on one
    cycle.  The four neighbouring triples fail, so a wrong constant copied into device and oracle alike cannot hide here."""
    prod = 1
    for p in R.PRIME_FACTORS:
        prod *= p
    assert prod == (1 << 64) - 1
    assert R.ABC == (26, 9, 13)
    t, ident, n = R.gf2_matrix(R.ABC), R.gf2_identity(), (1 << 64) - 1
    assert R.gf2_pow(t, n) == ident
    for p in R.PRIME_FACTORS:
        assert R.gf2_pow(t, n // p) != ident, p
    assert R.has_full_period(R.ABC)
    for abc in ((26, 9, 12), (25, 9, 13), (26, 8, 13), (26, 13, 9)):
        assert not R.has_full_period(abc), abc


# ---- the battery ----

@pytest.fixture(scope="module")
def sets():
    """name -> (keys, float numbers of the project's keying), computed once and left unchanged."""
    out = {}
    for name, (w, h, spp, k) in R.BATTERY_SETS.items():
        keys = R.frame_keys(w, h, spp)
        out[name] = (keys, R.stream_floats(R.BATTERY_SEED, keys, k))
    return out


@pytest.mark.parametrize("name", sorted(R.BATTERY_SETS))
def test_battery_accepts_the_project_keying(sets, name):
    w, h, spp, k = R.BATTERY_SETS[name]
    keys, u = sets[name]
    failures = []
    for letter, stat in sorted(R.battery(u, w, h, spp).items()):
        inside, worst, (lo, hi) = R.verdict(stat)
        print("(%s) %s: %d statistics, worst %.2f, allowed %.2f .. %.2f" % (letter, name, len(stat["values"]), worst, lo, hi))
        if not inside:
            failures.append(letter)
    assert not failures
    assert R.shared_states(R.BATTERY_SEED, keys) == 0                      # (g)


def test_first_samples_of_a_pixel_start_from_different_words():
    """(h), exact: within one pixel s0 = lowbias32(h + s * odd) and the hash is a bijection, so 2^16 (indeed 2^32) sample indices give different s0."""
    for pixel in (0, 77, (1 << 24) - 1):
        s = np.arange(1 << 16, dtype=np.uint64)
        s0, _ = R.stream_state(R.BATTERY_SEED, np.full(s.shape, pixel, np.uint64), s)
        assert np.unique(s0).size == s.size
    x = np.arange(1 << 20, dtype=np.uint64) * np.uint64(4093)
    assert np.unique(R.lowbias32(x)).size == x.size


# mutant -> the statistics that must reject it on set "first" (measured: profiles/sampler_battery.txt)
POWER = [("hash_before_sample", "c"), ("hash_before_sample", "f"), ("s1_is_s0", "e"), ("repeat_draw", "b"), ("half_range", "a"),
         ("drop_pixel_bit_0", "d"), ("drop_pixel_bit_6", "d")]


@pytest.mark.parametrize("mutant,letter", POWER)
def test_battery_rejects_the_named_defect(mutant, letter):
    """A statistic stays in the battery only because it is seen to reject a defect somebody could write."""
    w, h, spp, k = R.BATTERY_SETS["first"]
    u = R.stream_floats(R.BATTERY_SEED, R.frame_keys(w, h, spp), 8 if letter == "e" else 16, mutant)
    inside, worst, (lo, hi) = R.verdict(R.battery(u, w, h, spp, only=letter)[letter])
    print("(%s) %s: worst %.2f, allowed %.2f .. %.2f" % (letter, mutant, worst, lo, hi))
    assert not inside


def test_shared_streams_are_counted():
    """(g): the two mutants whose pixel pairs share streams are seen as shared initial states -- half of the set's streams."""
    w, h, spp, _ = R.BATTERY_SETS["deep"]
    keys = R.frame_keys(w, h, spp)
    assert R.shared_states(R.BATTERY_SEED, keys, "drop_pixel_bit_0") == keys.shape[0] // 2
    assert R.shared_states(R.BATTERY_SEED, keys) == 0


def _sp_keys():
    """The fp64 path's keys of a 16 x 16 frame, 4 subpixels, 64 samples each."""
    return R.frame_keys(16 * 4, 16, 64)


def test_smallpt_streams_do_not_overlap():
    """(g) for splitmix64: all streams walk ONE cycle, so what matters is how far apart they start.  No two streams of the set start within 256 steps of
    each other (a path uses far fewer); the variant that counts the sample index in steps is seen to fail."""
    keys = _sp_keys()
    assert R.sp_closest_starts(R.BATTERY_SEED, keys) > 256
    assert R.sp_closest_starts(R.BATTERY_SEED, keys, "sample_as_offset") == 1
    # the position really is the number of steps: a stream's state after j steps lies j further on
    s = R.sp_stream_state(7, np.array([5], np.uint64), np.array([9], np.uint64))
    with np.errstate(over="ignore"):
        later = s + np.uint64(R.GOLDEN64) * np.uint64(100)
        assert int(R.sp_sequence_position(later)[0] - R.sp_sequence_position(s)[0]) == 100


def test_smallpt_numbers_pass_the_battery():
    """(a)-(c), (e) on the doubles of the fp64 path's keying (a 64 x 16 'frame' of subpixels, 64 samples, 16 numbers)."""
    keys = _sp_keys()
    u = R.sp_words_to_double(R.sp_stream_words(R.BATTERY_SEED, keys, 16))
    for letter, stat in sorted(R.battery(u, 64, 16, 64, only="abce").items()):
        inside, worst, (lo, hi) = R.verdict(stat)
        print("(%s) smallpt: worst %.2f, allowed %.2f .. %.2f" % (letter, worst, lo, hi))
        assert inside, letter


# ---- expectation under a foreign generator: the check itself, oracle against oracle ----

def test_foreign_generator_check_passes_and_can_fail(O, A, api):
    """The oracle on its own streams against the oracle on the Mersenne Twister's tape (tests/sampler_expectation.py): the check holds; with a tape whose
    every second draw repeats the one before it fails by a wide margin (measured: sum z^2 1864 / 611 against 115, max |z| 15), so it sees dependence
    inside a sample.  It does not see correlation between samples: the battery above does."""
    own = E.own_samples(O.li, A, api, "cornell")
    tape, most = E.tape_samples(O, A, api, "cornell")
    ok, lines = E.check(own, tape, "cornell, oracle against the tape-fed oracle")
    print("\n".join(lines), "\nmost numbers one sample drew:", most)
    assert ok
    bad, _ = E.tape_samples(O, A, api, "cornell", repeat_draws=True)
    ok, lines = E.check(own, bad, "cornell, repeated draws")
    print("\n".join(lines))
    assert not ok
    for clamp in E.CLAMPS:
        s, mz, k, bound, _ = E.welch(own, bad, clamp)
        assert s > 3 * bound and mz > E.MAX_ABS_Z
