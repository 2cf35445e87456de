"""The two random-number generators of the project restated in NumPy integers from their published recurrences and from DESIGN.md section 5 -- not from
ky_amd/csrc/ky_device.hpp, ky_amd/csrc/ky_smallpt.hpp or oracle/*.cpp, which the tests compare WITH this module:

  the render kernels'   xoroshiro64+ (Blackman / Vigna's 64-bit xoroshiro step, rotations and shift (a, b, c) = (26, 9, 13), output s0 + s1), one stream
                        per camera sample; with h = lowbias32(pixel_index ^ lowbias32(seed)) the state is s0 = lowbias32(h + sample * 0x9E3779B9),
                        s1 = (rotl(s0, 16) ^ h) | 1; a number is the output's upper 23 bits times 2^-23 as a float;
  the fp64 path's       splitmix64 (Steele / Lea / Flood: state += 0x9E3779B97F4A7C15, output the finaliser of the state), one stream per
                        (subpixel, sample), started at finaliser(finaliser(seed << 32 ^ subpixel_index) + sample * 0xD1B54A32D192ED03); a number is the
                        output's upper 53 bits times 2^-53 as a double.

lowbias32 is the two-multiplier integer finaliser 16 / 0x21f0aaad / 15 / 0x735a2d97 / 15 of the hash-prospector family.

`mutant=` names a deliberately defective variant; tests/test_sampler.py shows which statistic of its battery rejects which.  A helper module (like
noise_restatement.py), shared by tests/test_sampler.py, tests/test_sampler_gpu.py and tools/sampler_battery.py."""
import math

import numpy as np

M32 = 0xFFFFFFFF
GOLDEN32 = 0x9E3779B9
GOLDEN64 = 0x9E3779B97F4A7C15
SP_SAMPLE_STEP = 0xD1B54A32D192ED03
ABC = (26, 9, 13)

# name -> what is wrong (the statistic that has to notice is named in tests/test_sampler.py)
MUTANTS = {
    "hash_before_sample": "s0 = lowbias32(h) + sample * 0x9E3779B9: the per-sample hash is taken before the sample index is added",
    "s1_is_s0": "s1 = s0 | 1: the second state word repeats the first",
    "repeat_draw": "draw 5 hands out draw 4 again",
    "half_range": "the conversion scales by 2^-24: numbers lie in [0, 0.5)",
    "drop_pixel_bit_0": "the pixel key ignores bit 0 of the pixel index: x-neighbours (2i, 2i + 1) share their streams",
    "drop_pixel_bit_6": "the pixel key ignores bit 6 of the pixel index: in a 64-wide frame rows (2i, 2i + 1) share their streams",
    # not rejected by the battery at its size (DESIGN.md section 5 says so): kept so that the blind spots stay measured
    "no_outer_hash": "h = pixel_index ^ lowbias32(seed): the pixel key without its outer hash",
    "s1_is_key": "s1 = h | 1: the second state word is the pixel key alone",
    "low_bits": "the conversion keeps the output's low 23 bits instead of the high ones",
}
SP_MUTANTS = {
    "sample_as_offset": "state = finaliser(finaliser(key)) + sample * 0x9E3779B97F4A7C15: sample s starts s steps into sample 0's stream",
}


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & np.uint64(M32)


def lowbias32(x):
    """uint32 -> uint32, elementwise (carried in uint64 so that the products are exact before they are cut to 32 bits)."""
    x = _u32(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x21F0AAAD)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x735A2D97)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    return x


def rotl32(x, k):
    x = _u32(x)
    k = int(k) % 32
    if k == 0:
        return x
    return ((x << np.uint64(k)) | (x >> np.uint64(32 - k))) & np.uint64(M32)


def pixel_key(seed, pixel_index, mutant=None):
    pixel_index = _u32(pixel_index)
    if mutant == "drop_pixel_bit_0":
        pixel_index = pixel_index & np.uint64(M32 ^ 1)
    if mutant == "drop_pixel_bit_6":
        pixel_index = pixel_index & np.uint64(M32 ^ 64)
    inner = pixel_index ^ lowbias32(np.uint64(int(seed) & M32))
    return inner if mutant == "no_outer_hash" else lowbias32(inner)


def stream_state(seed, pixel_index, sample_index, mutant=None):
    """The state (s0, s1) a camera sample's stream starts from; uint64 arrays holding 32-bit values."""
    h = pixel_key(seed, pixel_index, mutant)
    step = (_u32(sample_index) * np.uint64(GOLDEN32)) & np.uint64(M32)
    if mutant == "hash_before_sample":
        s0 = (lowbias32(h) + step) & np.uint64(M32)
    else:
        s0 = lowbias32((h + step) & np.uint64(M32))
    if mutant == "s1_is_s0":
        s1 = s0 | np.uint64(1)
    elif mutant == "s1_is_key":
        s1 = h | np.uint64(1)
    else:
        s1 = (rotl32(s0, 16) ^ h) | np.uint64(1)
    return s0, s1


def step(s0, s1, abc=ABC):
    """One xoroshiro64 step: -> (output word s0 + s1 mod 2^32, s0', s1')."""
    a, b, c = abc
    out = (s0 + s1) & np.uint64(M32)
    s1 = s1 ^ s0
    s0n = rotl32(s0, a) ^ s1 ^ ((s1 << np.uint64(b)) & np.uint64(M32))
    s1n = rotl32(s1, c)
    return out, s0n, s1n


def stream_words(seed, keys2, k, mutant=None):
    """keys2 [n, 2] {pixel_index, sample_index} -> [n, k] uint32: the generator's output words, before the conversion."""
    keys2 = np.asarray(keys2, np.uint64)
    s0, s1 = stream_state(seed, keys2[:, 0], keys2[:, 1], mutant)
    out = np.empty((keys2.shape[0], k), np.uint32)
    for j in range(k):
        if mutant == "repeat_draw" and j == 5:
            out[:, 5] = out[:, 4]
            continue
        w, s0, s1 = step(s0, s1)
        out[:, j] = w.astype(np.uint32)
    return out


def words_to_float(words, mutant=None):
    """(word >> 9) * 2^-23 as float32: both factors and the product are exact in fp32."""
    words = np.asarray(words, np.uint32)
    if mutant == "low_bits":
        m = words & np.uint32(0x7FFFFF)
    else:
        m = words >> np.uint32(9)
    scale = np.float32(2.0 ** -24) if mutant == "half_range" else np.float32(2.0 ** -23)
    return m.astype(np.float32) * scale


def stream_floats(seed, keys2, k, mutant=None):
    return words_to_float(stream_words(seed, keys2, k, mutant), mutant)


def stream_bits(seed, keys2, k, mutant=None):
    """The bit patterns of stream_floats: what kyhip_kat_sampler / kyo_kat_sampler return."""
    return stream_floats(seed, keys2, k, mutant).view(np.uint32)


def gf2_matrix(abc=ABC):
    """The xoroshiro64 state transition as a 64 x 64 matrix over GF(2), built from step() on the 64 one-bit states: column i is the image of bit i of
    (s0 | s1 << 32).  Rows are packed into Python integers (bit j of rows[i] = entry (i, j))."""
    cols = []
    for i in range(64):
        s0 = np.uint64(1 << i) if i < 32 else np.uint64(0)
        s1 = np.uint64(1 << (i - 32)) if i >= 32 else np.uint64(0)
        _, t0, t1 = step(s0, s1, abc)
        cols.append(int(t0) | (int(t1) << 32))
    rows = [0] * 64
    for j, col in enumerate(cols):
        for i in range(64):
            if (col >> i) & 1:
                rows[i] |= 1 << j
    return rows


def gf2_identity(n=64):
    return [1 << i for i in range(n)]


def gf2_mul(a, b):
    """(a b) over GF(2) for row-packed matrices: row i of the product is the xor of the rows of b that row i of a selects."""
    out = []
    for ra in a:
        acc, j = 0, 0
        while ra:
            if ra & 1:
                acc ^= b[j]
            ra >>= 1
            j += 1
        out.append(acc)
    return out


def gf2_pow(m, e):
    result, base = gf2_identity(len(m)), m
    while e:
        if e & 1:
            result = gf2_mul(result, base)
        e >>= 1
        if e:
            base = gf2_mul(base, base)
    return result


PRIME_FACTORS = (3, 5, 17, 257, 641, 65537, 6700417)   # the prime factors of 2^64 - 1


def has_full_period(abc):
    """The step's order in GL(64, 2) is 2^64 - 1: T^(2^64 - 1) = I and T^((2^64 - 1) / p) != I for every prime factor p."""
    t = gf2_matrix(abc)
    n = (1 << 64) - 1
    ident = gf2_identity()
    if gf2_pow(t, n) != ident:
        return False
    return all(gf2_pow(t, n // p) != ident for p in PRIME_FACTORS)


# ---- the fp64 path's splitmix64 ----

def _mul64(x, c):
    """x * c mod 2^64 for a uint64 array and a Python constant (NumPy's uint64 product wraps, which is the arithmetic wanted)."""
    with np.errstate(over="ignore"):
        return x * np.uint64(c)


def splitmix_finalise(z):
    z = np.asarray(z, np.uint64)
    z = _mul64(z ^ (z >> np.uint64(30)), 0xBF58476D1CE4E5B9)
    z = _mul64(z ^ (z >> np.uint64(27)), 0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sp_stream_state(seed, subpixel_index, sample, mutant=None):
    key = np.uint64((int(seed) & M32) << 32) ^ _u32(subpixel_index)
    with np.errstate(over="ignore"):
        if mutant == "sample_as_offset":
            return splitmix_finalise(splitmix_finalise(key)) + _mul64(_u32(sample), GOLDEN64)
        return splitmix_finalise(splitmix_finalise(key) + _mul64(_u32(sample), SP_SAMPLE_STEP))


def sp_stream_words(seed, keys2, k, mutant=None):
    """keys2 [n, 2] {subpixel_index, sample} -> [n, k] uint64 output words."""
    keys2 = np.asarray(keys2, np.uint64)
    s = sp_stream_state(seed, keys2[:, 0], keys2[:, 1], mutant)
    out = np.empty((keys2.shape[0], k), np.uint64)
    for j in range(k):
        with np.errstate(over="ignore"):
            s = s + np.uint64(GOLDEN64)
        out[:, j] = splitmix_finalise(s)
    return out


def sp_words_to_double(words):
    """(word >> 11) * 2^-53: exact in fp64."""
    return (np.asarray(words, np.uint64) >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


def sp_stream_bits(seed, keys2, k, mutant=None):
    return sp_words_to_double(sp_stream_words(seed, keys2, k, mutant)).view(np.uint64)


def sp_sequence_position(state):
    """Where a state lies on the one cycle all splitmix64 streams walk: state = position * 0x9E3779B97F4A7C15 mod 2^64 (the increment is odd, so
    invertible); two streams overlap within k steps iff their positions differ by at most k."""
    inv = pow(GOLDEN64, -1, 1 << 64)
    return _mul64(np.asarray(state, np.uint64), inv)


# ---- the battery's key sets and statistics (plain NumPy float64; thresholds: normal_quantile, chi2_bounds) ----

def frame_keys(width, height, spp):
    """[width * height * spp, 2] uint32 {pixel_index, sample_index}, pixel-major (a reshape to [height, width, spp, ...] recovers the frame)."""
    pix = np.repeat(np.arange(width * height, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), width * height)
    return np.stack([pix, smp], axis=1)


EDGE_SEEDS = (0, 1, 1234, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)   # the ABI's seed is a uint32: all of them are carried
EDGE_PIXELS = (0, 1, (1 << 16) - 1, 1 << 16, (1 << 24) - 1, 1 << 31, (1 << 32) - 1)   # 2^24 - 1: the last pixel of the 4096 x 4096 stress frame
EDGE_SAMPLES = (0, 1, 16383, 1 << 16, (1 << 31) - 1, (1 << 32) - 1)


def edge_keys(seed):
    """Every edge pixel with every edge sample index, and per edge pixel the three sample indices at which h + sample * 0x9E3779B9 (mod 2^32) is
    0 (the sum wraps to the hash's fixed point: s0 = 0), 1 (wraps) and 2^32 - 1 (the largest sum that does not)."""
    keys = [(p, s) for p in EDGE_PIXELS for s in EDGE_SAMPLES]
    inv = pow(GOLDEN32, -1, 1 << 32)
    for p in EDGE_PIXELS:
        h = int(pixel_key(seed, p))
        for target in (0, 1, M32):
            s = (((target - h) & M32) * inv) & M32
            assert (h + s * GOLDEN32) & M32 == target
            keys.append((p, s))
    return np.array(keys, np.uint32)


BATTERY_SEED = 1234
BATTERY_SETS = {"first": (64, 64, 256, 32), "deep": (16, 16, 256, 128)}   # width, height, samples per pixel, numbers per stream


def normal_quantile(p_two_sided):
    """z with P(|Z| > z) = p for a standard normal Z: bisection on math.erfc, to 1e-12."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if math.erfc(mid / math.sqrt(2.0)) > p_two_sided:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def family_z(count):
    """A family of `count` statistics of one kind: each must lie inside the two-sided 1 - 1e-6 / count quantile of its null distribution."""
    return normal_quantile(1e-6 / count)


def chi2_bounds(df, count):
    """That quantile for chi-square with df degrees of freedom by Wilson-Hilferty: (X / df)^(1/3) is normal with mean 1 - 2 / (9 df) and variance
    2 / (9 df).  -> (low, high)."""
    z = family_z(count)
    v = 2.0 / (9.0 * df)
    return df * (1.0 - v - z * math.sqrt(v)) ** 3, df * (1.0 - v + z * math.sqrt(v)) ** 3


def chi2_uniform(u, bins):
    """Pearson's statistic of values in [0, 1) against `bins` equal cells (bins - 1 degrees of freedom); a value outside [0, 1) counts as an error."""
    u = np.asarray(u, np.float64).ravel()
    cell = np.floor(u * bins).astype(np.int64)
    assert cell.min() >= 0 and cell.max() < bins
    obs = np.bincount(cell, minlength=bins).astype(np.float64)
    exp = u.size / bins
    return float(((obs - exp) ** 2).sum() / exp)


def chi2_pairs(u, v, bins=16):
    """Pearson's statistic of the pairs (u, v) on bins x bins equal cells (bins^2 - 1 degrees of freedom)."""
    u = np.asarray(u, np.float64).ravel()
    v = np.asarray(v, np.float64).ravel()
    cell = np.floor(u * bins).astype(np.int64) * bins + np.floor(v * bins).astype(np.int64)
    obs = np.bincount(cell, minlength=bins * bins).astype(np.float64)
    exp = u.size / (bins * bins)
    return float(((obs - exp) ** 2).sum() / exp)


def corr_z(a, b):
    """Pearson's r of two equally long samples times sqrt(n): standard normal if they are independent."""
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    a = a - a.mean()
    b = b - b.mean()
    r = float((a * b).sum() / math.sqrt(float((a * a).sum()) * float((b * b).sum())))
    return r * math.sqrt(a.size)


def per_pixel_chi2_z(u_ps, bins=16):
    """u_ps [pixels, samples]: Pearson's statistic per pixel on `bins` cells over the pixel's samples, summed over pixels, as deviations from its null:
    mean pixels * (bins - 1); variance pixels * 2 (bins - 1)(1 - 1 / samples), which is exact for equal cells; normal by the sum over pixels."""
    u_ps = np.asarray(u_ps, np.float64)
    n_pix, n_s = u_ps.shape
    cell = np.floor(u_ps * bins).astype(np.int64) + bins * np.arange(n_pix, dtype=np.int64)[:, None]
    obs = np.bincount(cell.ravel(), minlength=bins * n_pix).astype(np.float64)
    exp = n_s / bins
    total = float(((obs - exp) ** 2).sum() / exp)
    mean = n_pix * (bins - 1.0)
    var = n_pix * 2.0 * (bins - 1.0) * (1.0 - 1.0 / n_s)
    return (total - mean) / math.sqrt(var)


def battery(u, width, height, spp, only=None):
    """u: float [width * height * spp, k] in frame_keys order.  -> {statistic: {"kind": "chi2" | "z", "df": ..., "values": [...]}} for the statistics
    (a)-(f) of tests/test_sampler.py; `only` (a string of letters) restricts the work."""
    k = u.shape[1]
    f = np.asarray(u, np.float64).reshape(height, width, spp, k)
    want = only or "abcdef"
    out = {}
    if "a" in want:
        out["a"] = {"kind": "chi2", "df": 255, "values": [chi2_uniform(f[..., j], 256) for j in range(k)]}
    if "b" in want:
        out["b"] = {"kind": "chi2", "df": 255, "values": [chi2_pairs(f[..., j], f[..., j + 1]) for j in range(k - 1)]}
    if "c" in want:
        out["c"] = {"kind": "z", "values": [corr_z(f[:, :, :-1, j], f[:, :, 1:, j]) for j in range(k)]}
    if "d" in want:
        out["d"] = {"kind": "z", "values": [corr_z(f[:, :-1, :, j], f[:, 1:, :, j]) for j in range(k)] +
                                           [corr_z(f[:-1, :, :, j], f[1:, :, :, j]) for j in range(k)]}
    if "e" in want:
        out["e"] = {"kind": "z", "values": [corr_z(f[..., i], f[..., j]) for i in range(8) for j in range(i + 1, 8)]}
    if "f" in want:
        out["f"] = {"kind": "z", "values": [per_pixel_chi2_z(f[..., j].reshape(height * width, spp)) for j in range(k)]}
    return out


def verdict(stat):
    """-> (inside, worst value, (low, high)) of one battery() entry against its family's quantile."""
    vals = stat["values"]
    if stat["kind"] == "chi2":
        lo, hi = chi2_bounds(stat["df"], len(vals))
        worst = max(vals, key=lambda v: max(v - hi, lo - v))
    else:
        hi = family_z(len(vals))
        lo = -hi
        worst = max(vals, key=abs)
    return all(lo <= v <= hi for v in vals), worst, (lo, hi)


def shared_states(seed, keys2, mutant=None):
    """(g) for the render kernels' streams: how many of the key set's streams start from a state another one also starts from."""
    keys2 = np.asarray(keys2, np.uint64)
    s0, s1 = stream_state(seed, keys2[:, 0], keys2[:, 1], mutant)
    packed = s0 | (s1 << np.uint64(32))
    return int(packed.size - np.unique(packed).size)


def sp_closest_starts(seed, keys2, mutant=None):
    """(g) for the fp64 path: the smallest distance, in steps along splitmix64's cycle, between the starts of two streams of the key set."""
    keys2 = np.asarray(keys2, np.uint64)
    pos = np.sort(sp_sequence_position(sp_stream_state(seed, keys2[:, 0], keys2[:, 1], mutant)))
    with np.errstate(over="ignore"):
        gaps = np.diff(pos)
        wrap = pos[0] - pos[-1]   # mod 2^64: the gap across the cycle's end
    return int(min(int(gaps.min()), int(wrap)))
