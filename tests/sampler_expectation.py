"""Expectation under a foreign generator: a pixel's mean radiance must not depend on WHICH uniform numbers feed the path.  The oracle is run with every
sample's numbers read from a tape (kyo_li_tape) that NumPy's Mersenne Twister fills -- no code of the project's generators takes part -- and its per-pixel
means are compared with those of samples drawn from the project's own streams (the GPU's in tests/test_sampler_gpu.py, the oracle's in tests/test_sampler.py).

What the comparison sees and what it does not: a tape whose every second draw repeats the one before is rejected at once (dependence INSIDE a sample
moves the expectation); correlation BETWEEN samples leaves every expectation where it was and passes -- that is what tests/test_sampler.py's battery and
batch_means_deviation below are for.  A helper module, not a test module."""
import math

import numpy as np

import sampler_restatement as R

N_SAMPLES = 2048
N_PIXELS = 64
CLAMPS = (1.0, 32.0)
SIGMA_Z2_TAIL = 1e-4     # sum of z^2: at most the 1 - 1e-4 quantile of chi-square with as many degrees of freedom as pixels counted
MAX_ABS_Z = 4.5
# name -> (width, height, numbers per sample on the tape): all both_mis at depth 5; a depth-5 Veach sample was seen to draw up to 117 numbers, a Cornell one 36
SCENES = {"cornell": (32, 32, 64), "veach": (48, 27, 256), "environment": (32, 32, 64), "point": (32, 32, 64)}


def scene_and_params(A, api, name, n=N_SAMPLES):
    w, h, _ = SCENES[name]
    if name == "veach":
        scene = api.mis_scene(w, h)
    else:
        flags = {"cornell": A.CB_DEFAULT_SCENE, "environment": A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT,
                 "point": A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_POINT}[name]
        scene = api.cornell_box_scene(flags, w, h)
    return scene, api.make_params(w, h, n, max_path_depth=5, direct_sample=A.DIRECT_BOTH_MIS)


def pixels(name):
    """The scene's 64 pixels (x, y): default_rng(5) draws them without replacement from the frame."""
    w, h, _ = SCENES[name]
    idx = np.random.default_rng(5).choice(w * h, N_PIXELS, replace=False)
    return [(int(i % w), int(i // w)) for i in idx]


def mt_tape_rows(gen, n, stride, repeat_draws=False):
    """n rows of `stride` uniform floats from NumPy's generator: 32-bit integers >> 9, times 2^-23, as float32 (the same 23-bit grid the project's
    numbers lie on).  repeat_draws: every second draw repeats the one before -- the defect the check must reject."""
    words = gen.integers(0, 1 << 32, size=(n, stride), dtype=np.uint32)
    rows = (words >> np.uint32(9)).astype(np.float32) * np.float32(2.0 ** -23)
    if repeat_draws:
        assert stride % 2 == 0
        rows[:, 1::2] = rows[:, 0::2]
    return rows


def tape_samples(O, A, api, name, n=N_SAMPLES, repeat_draws=False):
    """The oracle's radiance samples [pixels, n, 3] under the Mersenne Twister's numbers, and the most numbers one sample consumed."""
    scene, params = scene_and_params(A, api, name, n)
    stride = SCENES[name][2]
    gen = np.random.Generator(np.random.MT19937(2024))
    out, most = [], 0
    for x, y in pixels(name):
        li, used = O.li_tape(scene, params, x, y, mt_tape_rows(gen, n, stride, repeat_draws))
        assert int(used.max()) <= stride
        most = max(most, int(used.max()))
        out.append(li)
    return np.stack(out), most


def own_samples(li_fn, A, api, name, n=N_SAMPLES):
    """[pixels, n, 3] from li_fn(scene, params, x, y, 0, n): api.kat_li (the GPU's own streams) or O.li (the oracle's)."""
    scene, params = scene_and_params(A, api, name, n)
    return np.stack([li_fn(scene, params, x, y, 0, n) for x, y in pixels(name)])


def luminance(li, clamp):
    c = np.minimum(np.asarray(li, np.float64), clamp)
    return 0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2]


def chi2_upper(df, tail):
    """The 1 - tail quantile of chi-square with df degrees of freedom by Wilson-Hilferty."""
    z = R.normal_quantile(2.0 * tail)   # one-sided tail
    v = 2.0 / (9.0 * df)
    return df * (1.0 - v + z * math.sqrt(v)) ** 3


def welch(a, b, clamp):
    """a, b: [pixels, n, 3] -> (sum of z^2, max |z|, pixels counted, the bound on the sum, pixels whose zero-variance means differ)."""
    ya, yb = luminance(a, clamp), luminance(b, clamp)
    ma, mb = ya.mean(axis=1), yb.mean(axis=1)
    se2 = ya.var(axis=1, ddof=1) / ya.shape[1] + yb.var(axis=1, ddof=1) / yb.shape[1]
    counted = se2 > 0
    z = (ma[counted] - mb[counted]) / np.sqrt(se2[counted])
    flat_differ = int(np.count_nonzero(ma[~counted] != mb[~counted]))
    k = int(counted.sum())
    return float((z * z).sum()), float(np.abs(z).max()) if k else 0.0, k, chi2_upper(k, SIGMA_Z2_TAIL) if k else 0.0, flat_differ


def check(a, b, label=""):
    """-> (passes, report lines) of the comparison at both clamps."""
    ok, lines = True, []
    for clamp in CLAMPS:
        s, mz, k, bound, flat = welch(a, b, clamp)
        lines.append("%s clamp %g: sum z^2 %.1f (bound %.1f at %d pixels), max |z| %.2f (bound %.1f), flat pixels that differ %d" %
                     (label, clamp, s, bound, k, mz, MAX_ABS_Z, flat))
        ok = ok and s <= bound and mz <= MAX_ABS_Z and flat == 0
    return ok, lines


def batch_means_ratio(y, m):
    """y [pixels, n]: m * var(means of m consecutive samples) / var(samples), averaged over the pixels that vary.  1 in expectation for independent samples."""
    n = (y.shape[1] // m) * m
    v = y[:, :n].var(axis=1, ddof=1)
    keep = v > 0
    bm = y[keep, :n].reshape(int(keep.sum()), n // m, m).mean(axis=2)
    return float((m * bm.var(axis=1, ddof=1) / v[keep]).mean())


def batch_means_deviations(y, ms=(2, 8, 32), shuffles=200, seed=7):
    """Each m's ratio in deviations of its own permutation null: the same values shuffled within each pixel (one shuffle serves every m).
    -> {m: (deviations, ratio, null mean, null sd)}.  A weak detector: it sees samples of a pixel that lean on their neighbours in the stream's order,
    strongly enough to change the variance of short runs."""
    gen = np.random.default_rng(seed)
    null = {m: [] for m in ms}
    for _ in range(shuffles):
        p = gen.permuted(y, axis=1)
        for m in ms:
            null[m].append(batch_means_ratio(p, m))
    out = {}
    for m in ms:
        ratio, mean, sd = batch_means_ratio(y, m), float(np.mean(null[m])), float(np.std(null[m], ddof=1))
        out[m] = ((ratio - mean) / sd, ratio, mean, sd)
    return out
