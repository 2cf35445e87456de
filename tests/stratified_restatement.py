"""The stratified sampler (KY_SAMPLER_STRATIFIED) restated in NumPy from DESIGN.md section 5, "The stratified sampler" -- not from ky_amd/csrc/ky_device.hpp,
which the tests compare WITH this module.  Integers are carried in uint64 and cut to 32 bits where the definition says so; every float operation is one
float32 operation, rounded on its own (NumPy fuses nothing), and the three reciprocals are float32(1) / float32(k) as the host computes them.

`mutant=` names a deliberately defective variant; tests/test_stratified.py shows which statistic of its battery rejects which.  A helper module (like
sampler_restatement.py), shared by tests/test_stratified.py, tests/test_stratified_gpu.py, tools/stratified_battery.py and tests/stratified_mse.py."""
import math

import numpy as np

import sampler_restatement as R

DIMS = 16                      # KYHIP_STRATIFIED_DIMS
MAX_SPP = 1 << 24
PERM_MUL = (0x9E3779B1, 0x85EBCA6B)
KEY_MUL = 0x85EBCA77
PURPOSE_CELL, PURPOSE_COLUMN, PURPOSE_ROW = 0, 1, 16   # the camera sample's three permutations; draw position d = 2 .. 15 is purpose d
BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)   # the largest float below 1

MUTANTS = {
    "one_key": "every draw position and every camera permutation takes purpose 0's key",
    "key_ignores_pixel": "the keys are hashed from the seed alone: every pixel permutes alike",
    "identity_perm": "perm(i, n, key) = i",
}

M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def grid(n_spp):
    """-> (m, n): m = floor(sqrt(N)) columns, n = ceil(N / m) rows, in integers."""
    m = math.isqrt(int(n_spp))
    return m, -(-int(n_spp) // m)


def reciprocal(k):
    return np.float32(1.0) / np.float32(k)


def bit_length(v):
    return int(v).bit_length()


def perm(i, n, key, mutant=None):
    """The keyed bijection of [0, n): i and key arrays (broadcast together), n an integer.  Cycle-walking on [0, 2^b), b the bit length of n - 1; h = ceil(b / 2)."""
    i, key = np.broadcast_arrays(_u64(i), _u64(key))
    i = i.copy()
    if mutant == "identity_perm":
        return i
    n = int(n)
    assert 1 <= n <= MAX_SPP and (i.size == 0 or int(i.max()) < n)
    b = bit_length(n - 1)
    mask = np.uint64((1 << b) - 1)
    h = np.uint64((b + 1) // 2)
    key = key & M32
    key1 = ((key >> np.uint64(11)) | (key << np.uint64(21))) & M32   # the key rotated right by 11 and by 22
    key2 = ((key >> np.uint64(22)) | (key << np.uint64(10))) & M32
    todo = np.ones(i.shape, bool)
    while todo.any():
        v = i[todo]
        v = (((v ^ key[todo]) * np.uint64(PERM_MUL[0])) & M32) & mask
        v = v ^ (v >> h)
        v = (((v ^ key1[todo]) * np.uint64(PERM_MUL[1])) & M32) & mask
        v = v ^ (v >> h)
        v = (v ^ key2[todo]) & mask
        i[todo] = v
        todo = i >= np.uint64(n)
    return i


def purpose_key(h, j, mutant=None):
    """k_j = lowbias32(h ^ ((j + 1) * 0x85EBCA77 mod 2^32))."""
    if mutant == "one_key":
        j = 0
    return R.lowbias32(_u64(h) ^ np.uint64(((int(j) + 1) * KEY_MUL) & 0xFFFFFFFF))


def _pixel_key(seed, pixel_index, mutant=None):
    if mutant == "key_ignores_pixel":
        return R.pixel_key(seed, np.zeros_like(_u64(pixel_index)))
    return R.pixel_key(seed, pixel_index)


def strata(seed, keys2, n_spp, k=DIMS, mutant=None):
    """keys2 [n, 2] {pixel_index, sample_index} -> the integer strata of the first min(k, 16) draw positions, int64 [n, min(k, 16), 2]:
    positions 2 .. 15: {perm(s, N, k_d), 0}; position 0: {cx, perm(cy, n, k_x)}; position 1: {cy, perm(cx, m, k_y)}."""
    keys2 = _u64(keys2)
    h, s = _pixel_key(seed, keys2[:, 0], mutant), keys2[:, 1]
    assert int(s.max()) < n_spp
    m, n = grid(n_spp)
    kk = min(k, DIMS)
    out = np.zeros((keys2.shape[0], kk, 2), np.int64)
    c = perm(s, n_spp, purpose_key(h, PURPOSE_CELL, mutant), mutant)
    cx, cy = c % np.uint64(m), c // np.uint64(m)
    if kk > 0:
        out[:, 0, 0], out[:, 0, 1] = cx, perm(cy, n, purpose_key(h, PURPOSE_COLUMN, mutant), mutant)
    if kk > 1:
        out[:, 1, 0], out[:, 1, 1] = cy, perm(cx, m, purpose_key(h, PURPOSE_ROW, mutant), mutant)
    for d in range(2, kk):
        out[:, d, 0] = perm(s, n_spp, purpose_key(h, d, mutant), mutant)
    return out


def floats(seed, keys2, n_spp, k, mutant=None):
    """-> float32 [n, k]: the numbers the sample of each key hands out, in order."""
    raw = R.stream_floats(seed, keys2, k)          # r_d: the stream is stepped once per draw whatever becomes of the number
    out = raw.copy()
    st = strata(seed, keys2, n_spp, k, mutant)
    m, n = grid(n_spp)
    inv_N, inv_m, inv_n = reciprocal(n_spp), reciprocal(m), reciprocal(n)
    f = lambda a: a.astype(np.float32)
    if k > 0:
        t = (f(st[:, 0, 1]) + raw[:, 0]) * inv_n
        out[:, 0] = (f(st[:, 0, 0]) + t) * inv_m
    if k > 1:
        t = (f(st[:, 1, 1]) + raw[:, 1]) * inv_m
        out[:, 1] = (f(st[:, 1, 0]) + t) * inv_n
    for d in range(2, min(k, DIMS)):
        out[:, d] = (f(st[:, d, 0]) + raw[:, d]) * inv_N
    kk = min(k, DIMS)
    out[:, :kk] = np.minimum(out[:, :kk], BELOW_ONE)
    assert out.dtype == np.float32
    return out


def bits(seed, keys2, n_spp, k, mutant=None):
    """What kyhip_kat_sampler_kind(KY_SAMPLER_STRATIFIED) returns."""
    return floats(seed, keys2, n_spp, k, mutant).view(np.uint32)


def pixel_keys(pixel_index, n_spp):
    """[N, 2]: every sample of one pixel."""
    return np.stack([np.full(n_spp, pixel_index, np.uint64), np.arange(n_spp, dtype=np.uint64)], axis=1)


def tape(seed, pixel_index, n_spp, stride, mutant=None, first=0, count=None):
    """float32 [count, stride]: the tape kyo_li_tape reads for samples first .. first + count - 1 of the pixel under a frame of n_spp samples per pixel."""
    keys = pixel_keys(pixel_index, n_spp)[first:first + (n_spp - first if count is None else count)]
    return floats(seed, keys, n_spp, stride, mutant)


# ---- the battery on the integer strata (tests/test_stratified.py; thresholds: sampler_restatement.chi2_bounds / family_z) ----

BATTERY_SEED = R.BATTERY_SEED
BATTERY_SET = (64, 64, 64)          # width, height, samples per pixel: 4096 pixels, an 8 x 8 camera grid
BATTERY_SAMPLES = (0, 1, 63)        # the sample indices whose strata are looked at across the frame's pixels in (b) and (c)


def fine_strata(seed, width, height, n_spp, mutant=None, pixel_mutant=None):
    """int64 [height, width, N, 16]: per pixel, sample and draw position the index of the finest stratum the definition names -- positions 2 .. 15:
    perm(s, N, k_d) of N; position 0: the fine column cx n + perm(cy, n, k_x) of m n; position 1: the fine row cy m + perm(cx, m, k_y) of m n.
    pixel_mutant: a sampler_restatement.pixel_key mutant (a pixel key that ignores one bit of the pixel index)."""
    keys = R.frame_keys(width, height, n_spp).astype(np.uint64)
    if pixel_mutant == "drop_pixel_bit_0":
        keys[:, 0] &= np.uint64(0xFFFFFFFE)
    st = strata(seed, keys, n_spp, DIMS, mutant)
    m, n = grid(n_spp)
    out = st[:, :, 0].copy()
    out[:, 0] = st[:, 0, 0] * n + st[:, 0, 1]
    out[:, 1] = st[:, 1, 0] * m + st[:, 1, 1]
    return out.reshape(height, width, n_spp, DIMS)


def _chi2_cells(cell, n_cells):
    obs = np.bincount(np.asarray(cell, np.int64).ravel(), minlength=n_cells).astype(np.float64)
    exp = cell.size / n_cells
    return float(((obs - exp) ** 2).sum() / exp)


def battery(f, n_spp, only=None):
    """f: fine_strata's array for a frame whose strata counts (N, and m n for the camera) are multiples of 8.
    (a) over the frame's pixels the stratum of sample s at position d is uniform: Pearson on all its strata, one statistic per (s, d);
    (b) the strata at positions d < e of one sample are independent: Pearson on 8 x 8 coarse cells over the pixels, per pair and per s of BATTERY_SAMPLES;
    (c) the strata of neighbouring pixels are independent: r sqrt(n) between x- and y-neighbours, per position and per s of BATTERY_SAMPLES."""
    height, width, n, dims = f.shape
    m, nn = grid(n_spp)
    count = np.array([m * nn, m * nn] + [n_spp] * (dims - 2))
    assert np.all(count % 8 == 0)
    want, out = only or "abc", {}
    if "a" in want:
        vals = [_chi2_cells(f[:, :, s, d], int(count[d])) for s in range(n) for d in range(dims)]
        assert len(set(count)) == 1   # one df for the family
        out["a"] = {"kind": "chi2", "df": int(count[0]) - 1, "values": vals}
    coarse = f * 8 // count   # 0 .. 7
    if "b" in want:
        out["b"] = {"kind": "chi2", "df": 63, "values": [_chi2_cells(coarse[:, :, s, d] * 8 + coarse[:, :, s, e], 64)
                                                         for s in BATTERY_SAMPLES for d in range(dims) for e in range(d + 1, dims)]}
    if "c" in want:
        g = (f + 0.5) / count
        out["c"] = {"kind": "z", "values": [R.corr_z(g[:, :-1, s, d], g[:, 1:, s, d]) for s in BATTERY_SAMPLES for d in range(dims)] +
                                           [R.corr_z(g[:-1, :, s, d], g[1:, :, s, d]) for s in BATTERY_SAMPLES for d in range(dims)]}
    return out
