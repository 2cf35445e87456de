"""CPU: the stratified sampler (KY_SAMPLER_STRATIFIED) on its NumPy restatement (tests/stratified_restatement.py, written from DESIGN.md section 5).

perm is a bijection at every size asked of it; a pixel's samples occupy their strata exactly; a battery on the integer strata, with bounds derived as in
tests/test_sampler.py (a family of T statistics passes if each lies inside the two-sided 1 - 1e-6 / T quantile of its null distribution), accepts the shipped
keying and rejects three named defects; the CPU oracle fed with the restatement's tape (kyo_li_tape) has the expectation it has under a Mersenne Twister's
tape; and a replay shows that the strata pay.  tests/test_stratified_gpu.py compares the DEVICE's bits with the same restatement.

Measured (profiles/stratified_battery.txt holds every figure), 64 x 64 pixels x 64 samples, seed 1234: (a) 1024 statistics 35 .. 110 inside 16 .. 158;
(b) 360 statistics 36 .. 93 inside 17 .. 155; (c) worst 2.3 deviations inside 5.7."""
import ctypes as C

import numpy as np
import pytest

import sampler_expectation as E
import sampler_restatement as R
import stratified_restatement as S

SPPS = (1, 2, 3, 4, 5, 7, 16, 17, 63, 64, 65, 500)
PIXELS = (0, 1, 2, 3, 31, 32, 1023, 1024, 4095, 65535, 65536, 1 << 20, (1 << 24) - 1, 1 << 24, 1 << 31, (1 << 32) - 1)


# ---- (1) perm is a bijection ----

def test_perm_is_a_bijection_up_to_300_and_around_two_to_the_16():
    keys = np.random.default_rng(11).integers(0, 1 << 32, 64, dtype=np.uint64)
    keys[:4] = (0, 1, 0x80000000, 0xFFFFFFFF)
    for n in list(range(1, 301)) + [(1 << 16) - 1, 1 << 16, (1 << 16) + 1]:
        i = np.arange(n, dtype=np.uint64)
        p = S.perm(i[None, :], n, keys[:, None])
        assert np.array_equal(np.sort(p, axis=1), np.broadcast_to(i, p.shape)), n


@pytest.mark.parametrize("key", (0, 0xFFFFFFFF, 0x9E3779B9, 1234567))
def test_perm_is_a_bijection_of_two_to_the_24(key):
    n = 1 << 24
    p = S.perm(np.arange(n, dtype=np.uint64), n, np.uint64(key))
    count = np.bincount(p.astype(np.int64), minlength=n)
    assert count.size == n and count.min() == 1 and count.max() == 1


# ---- (2) exact strata ----

@pytest.mark.parametrize("n_spp", SPPS)
def test_a_pixels_samples_occupy_their_strata_exactly(n_spp):
    m, n = S.grid(n_spp)
    assert m * m <= n_spp < (m + 1) * (m + 1) and (n - 1) * m < n_spp <= n * m
    k = 24
    for pixel in PIXELS:
        keys = S.pixel_keys(pixel, n_spp)
        st = S.strata(1234, keys, n_spp)
        for d in range(2, S.DIMS):   # Latin hypercube: the strata of the pixel's samples are a permutation of 0 .. N - 1
            assert np.array_equal(np.sort(st[:, d, 0]), np.arange(n_spp)), (pixel, d)
        cx, jx, cy, jy = st[:, 0, 0], st[:, 0, 1], st[:, 1, 0], st[:, 1, 1]
        assert cx.min() >= 0 and cx.max() < m and cy.min() >= 0 and cy.max() < n and jx.max() < n and jy.max() < m
        assert np.unique(cy * m + cx).size == n_spp          # no m x n cell holds two samples
        assert np.unique(cx * n + jx).size == n_spp          # no two samples share one of the m n fine columns
        assert np.unique(cy * m + jy).size == n_spp          # ... or one of the m n fine rows
        # the floats: in [0, 1), in the stratum the integers name, the raw stream's bits from position 16 on (and everywhere when N = 1)
        f = S.floats(1234, keys, n_spp, k)
        raw = R.stream_floats(1234, keys, k)
        assert f.dtype == np.float32 and f.min() >= 0 and f.max() < 1
        assert np.array_equal(f[:, S.DIMS:].view(np.uint32), raw[:, S.DIMS:].view(np.uint32))
        if n_spp == 1:
            assert np.array_equal(f.view(np.uint32), raw.view(np.uint32))
        # Each value is the exact one (stratum + r) / count after at most four fp32 roundings (two sums, two products) of numbers below one, and after a
        # reciprocal rounded once: it may reach its stratum's upper end, and miss either end by 2^-21 relative.  Nothing wider is allowed.
        x = f.astype(np.float64)
        slack = 2.0 ** -21
        fine = [(cx * n + jx, m * n), (cy * m + jy, m * n)] + [(st[:, d, 0], n_spp) for d in range(2, S.DIMS)]
        for d, (index, count) in enumerate(fine):
            lo, hi = index / count, (index + 1) / count
            assert np.all(x[:, d] >= lo * (1 - slack)) and np.all(x[:, d] <= hi * (1 + slack)), (pixel, d)


def test_the_largest_jitter_stays_below_one():
    """A stratum's last float would round to 1 in the last stratum: the clamp keeps it the largest float below 1."""
    assert S.BELOW_ONE == np.nextafter(np.float32(1), np.float32(0))
    top = (np.float32(499) + np.float32(1 - 2.0 ** -23)) * S.reciprocal(500)
    assert np.minimum(top, S.BELOW_ONE) < 1


# ---- (3) the battery ----

@pytest.fixture(scope="module")
def strata():
    w, h, n = S.BATTERY_SET
    return S.fine_strata(S.BATTERY_SEED, w, h, n)


def test_battery_accepts_the_shipped_keys_and_perm(strata):
    failures = []
    for letter, stat in sorted(S.battery(strata, S.BATTERY_SET[2]).items()):
        inside, worst, (lo, hi) = R.verdict(stat)
        print("(%s): %d statistics, %.2f .. %.2f, worst %.2f, allowed %.2f .. %.2f" % (letter, len(stat["values"]), min(stat["values"]), max(stat["values"]), worst, lo, hi))
        if not inside:
            failures.append(letter)
    assert not failures


# defect -> the statistic that must reject it (a statistic stays only because it is seen to reject a defect somebody could write)
# (pixels that all permute alike have no variance across the frame: (c) is then 0 / 0, which shows nothing -- its defect is a key that ignores ONE bit of the pixel index)
POWER = [("identity_perm", None, "a"), ("key_ignores_pixel", None, "a"), ("one_key", None, "b"), (None, "drop_pixel_bit_0", "c")]


@pytest.mark.parametrize("mutant,pixel_mutant,letter", POWER)
def test_battery_rejects_the_named_defect(mutant, pixel_mutant, letter):
    w, h, n = S.BATTERY_SET
    f = S.fine_strata(S.BATTERY_SEED, w, h, n, mutant, pixel_mutant)
    inside, worst, (lo, hi) = R.verdict(S.battery(f, n, only=letter)[letter])
    assert np.isfinite(worst)
    print("(%s) %s %s: worst %.2f, allowed %.2f .. %.2f" % (letter, mutant, pixel_mutant, worst, lo, hi))
    assert not inside


# ---- (4) unbiased through the whole path ----

def stratified_tape_samples(O, A, api, name, n=E.N_SAMPLES):
    """The oracle's radiance samples [pixels, n, 3] with every sample's numbers read from the restatement's stratified tape of a frame of n samples per pixel."""
    scene, params = E.scene_and_params(A, api, name, n)
    w, _, stride = E.SCENES[name]
    out = []
    for x, y in E.pixels(name):
        li, used = O.li_tape(scene, params, x, y, S.tape(params.seed, y * w + x, n, stride))
        assert int(used.max()) <= stride
        out.append(li)
    return np.stack(out)


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_expectation_is_the_foreign_generators(O, A, api, name):
    """The oracle under the stratified tape against the oracle under the Mersenne Twister's tape, sampler_expectation.check with its bounds.  Stratified samples
    of a pixel are negatively correlated, so their sample variance overstates the variance of their mean: Welch's standard error is conservative here, and the
    check loses power, not validity."""
    strat = stratified_tape_samples(O, A, api, name)
    mt, _ = E.tape_samples(O, A, api, name)
    ok, lines = E.check(strat, mt, name + ", stratified tape against the Mersenne Twister's")
    print("\n".join(lines))
    assert ok


def test_expectation_check_sees_a_stratified_tape_that_repeats_a_position(O, A, api):
    """... and it still has the power that matters: with one key for every position (positions 2 .. 15 of a sample share their stratum) the means move."""
    scene, params = E.scene_and_params(A, api, "cornell")
    w, _, stride = E.SCENES["cornell"]
    bad = np.stack([O.li_tape(scene, params, x, y, S.tape(params.seed, y * w + x, E.N_SAMPLES, stride, "one_key"))[0] for x, y in E.pixels("cornell")])
    mt, _ = E.tape_samples(O, A, api, "cornell")
    ok, lines = E.check(bad, mt, "cornell, one key for every position")
    print("\n".join(lines))
    assert not ok


# ---- (11) refusals that need no device: the host-only validation every entry shares ----

def test_host_validation_knows_three_sampler_kinds(A, api):
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 32, 32)
    rect = (C.c_int * 4)()

    def bound(params):
        return lib.kyhip_scene_screen_bound(api._scene_ptr(scene), C.byref(params), rect, None)

    assert A.SAMPLER_STRATIFIED == 2 and A.STRATIFIED_DIMS == S.DIMS
    assert bound(api.make_params(32, 32, 16, sampler=A.SAMPLER_STRATIFIED)) == A.KY_OK
    assert bound(api.make_params(32, 32, 1 << 24, sampler=A.SAMPLER_STRATIFIED)) == A.KY_OK
    assert bound(api.make_params(32, 32, (1 << 24) + 1, sampler=A.SAMPLER_STRATIFIED)) == A.KY_ERR_INVALID_VALUE
    assert bound(api.make_params(32, 32, 16, sampler=3)) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_abi_version() == 4


# ---- (5) it pays ----

def test_stratified_estimates_have_the_smaller_error(O, A, api):
    """tools/stratified_replay.py's experiment at a size a test can afford (profiles/stratified_replay.txt holds the full one): 16-sample estimates of the Veach
    frame's 64 pixels and of a camera-only integrand (first-hit base colour on the Cornell frame's pixels that straddle an edge), 24 replications under each of
    four seeds, mean squared error against 8192 samples of the random sampler on the same oracle.  Asserted: the Veach frame's MEDIAN pixel ratio and the
    camera-only SUM ratio, stratified over random, are below 1 by a margin taken from the replay's own spread -- the mean of the four seeds' figures plus four
    standard errors of that mean, the standard error estimated from the four.  (The Cornell frame's median is reported by the tool and not asserted: 0.8 - 1.1,
    inside its noise -- indirect light with heavy tails gains little.)"""
    import stratified_mse as P
    seeds, reps, n_spp = (1234, 99, 20260102, 7), 24, 16
    figures = {}
    for name in ("veach", "basecolor"):
        if name == "veach":
            w, h, stride = E.SCENES[name]
            scene = E.scene_and_params(A, api, name, n_spp)[0]
            params = lambda n: E.scene_and_params(A, api, "veach", n)[1]
            pixels = E.pixels(name)
        else:
            w, h, stride = 32, 32, 4
            scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
            params = lambda n: api.make_params(w, h, n, integrator=A.INTEGRATOR_BASECOLOR, max_path_depth=5)
            pixels = P.edge_pixels(O, scene, params(64), w, h)
            assert len(pixels) >= 32
        gen = np.random.Generator(np.random.MT19937(2024))
        refs = [P.reference(O, scene, params(P.REFERENCE_SAMPLES), x, y, stride, gen) for x, y in pixels]
        per_seed = [P.ratios(P.replay(O, scene, params(n_spp), pixels, w, h, stride, seed, n_spp, reps, refs)["mse"]) for seed in seeds]
        v = np.array([r[1] if name == "veach" else r[0] for r in per_seed])
        bound = float(v.mean() + 4.0 * v.std(ddof=1) / np.sqrt(len(v)))
        print("%s, N = %d: %s per seed %s, mean + 4 standard errors %.3f" % (name, n_spp, "median ratio" if name == "veach" else "sum ratio", np.round(v, 3), bound))
        figures[name] = bound
    assert figures["veach"] < 1 and figures["basecolor"] < 1, figures
