"""The pixel filters (include/kyhip.h, ky_pixel_filter) restated in NumPy, independently of ky_amd/csrc: the analytic 1-D laws, the
inverse-CDF table by bisection in double on the analytic CDF, the warp in float32 exactly as the device writes it, and the tape that makes the CPU oracle render a
filtered sample -- kyo_li_tape hands a sample's numbers out from a row, and its camera sample adds the first two to the pixel's corner whatever they are.
Not a test: tests/test_filter.py and tests/test_filter_gpu.py import it."""
import math

import numpy as np

import sampler_restatement as R
import stratified_restatement as S

BOX, TENT, GAUSSIAN, BLACKMAN_HARRIS = 0, 1, 2, 3
TABLE = 256
BH = (0.35875, 0.48829, 0.14128, 0.01168)
SAMPLER_RANDOM, SAMPLER_STRATIFIED = 1, 2   # ky_sampler_kind

f32 = np.float32


class Filter:
    """kind, radius (pixels), param (the Gaussian's sigma): what a ky_pixel_filter says.  A box has radius 0.5 whatever it was given."""

    def __init__(self, kind, radius=None, param=0.0):
        defaults = {BOX: (0.5, 0.0), TENT: (2.0, 0.0), GAUSSIAN: (1.5, 0.5), BLACKMAN_HARRIS: (2.0, 0.0)}
        self.kind = kind
        self.radius = float(f32(defaults[kind][0] if (radius is None or kind == BOX) else radius))
        self.param = float(f32(defaults[kind][1] if (kind == GAUSSIAN and not param) else param))

    def __repr__(self):
        return "Filter(%d, %g, %g)" % (self.kind, self.radius, self.param)


def density(flt, x):
    """The unnormalised 1-D density at x (float64 array), zero outside (-R, R)."""
    x = np.asarray(x, np.float64)
    R_ = flt.radius
    t = x / R_
    if flt.kind == BOX:
        w = np.ones_like(x)
    elif flt.kind == TENT:
        w = 1.0 - np.abs(t)
    elif flt.kind == GAUSSIAN:
        s = flt.param
        w = np.exp(-x * x / (2 * s * s)) - math.exp(-R_ * R_ / (2 * s * s))
    else:
        w = BH[0] + BH[1] * np.cos(np.pi * t) + BH[2] * np.cos(2 * np.pi * t) + BH[3] * np.cos(3 * np.pi * t)
    return np.where(np.abs(x) < R_, np.maximum(w, 0.0), 0.0)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def cdf(flt, x):
    """The analytic distribution F over [-R, R] at x (float64 array): erf for the Gaussian, the integrated cosine series for Blackman-Harris."""
    x = np.asarray(x, np.float64)
    R_ = flt.radius
    t = x / R_
    if flt.kind == BOX:
        return 0.5 * (1.0 + t)
    if flt.kind == TENT:
        return np.where(t < 0, 0.5 * (1 + t) ** 2, 1 - 0.5 * (1 - t) ** 2)
    if flt.kind == GAUSSIAN:
        s = flt.param
        k = s * math.sqrt(math.pi / 2)
        c = math.exp(-R_ * R_ / (2 * s * s))
        e_r = math.erf(R_ / (s * math.sqrt(2)))
        return (k * (_erf(x / (s * math.sqrt(2))) + e_r) - c * (x + R_)) / (2 * k * e_r - 2 * c * R_)
    series = sum(BH[j] / j * np.sin(j * np.pi * t) for j in (1, 2, 3)) / np.pi
    return ((t + 1.0) * BH[0] + series) / (2 * BH[0])


def table(flt, n=TABLE):
    """float32 [n + 1]: F^-1(i / n) by bisection in double on the analytic CDF (all entries at once, 80 halvings: the bracket is below one double's spacing long
    before that), rounded once; the two ends are -R and +R by definition of the support."""
    u = np.arange(n + 1, dtype=np.float64) / n
    lo = np.full(n + 1, -flt.radius)
    hi = np.full(n + 1, flt.radius)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        below = cdf(flt, mid) < u
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    out = (0.5 * (lo + hi)).astype(f32)
    out[0], out[n] = f32(-flt.radius), f32(flt.radius)
    return out


def warp(flt, u, tab=None, shift=0.0):
    """float32: the offset from the pixel's corner for each u in [0, 1), operation by operation as the device's filter_offset: every product, sum and fused
    multiply-add rounded once to float32.  (A float32 fma is computed here in float64 and rounded: the product of two float32 is exact in float64, the sum is
    rounded to 53 bits and then to 24, which differs from the single rounding by one float32 ulp only where the 53-bit sum lands on a float32 tie -- within the
    GPU test's bound of 2^-21 R.)  tab: the table to read (default: table(flt)).  shift: added to the 0.5 -- 0 is the definition; -0.5 is
    the named defect `centred on the pixel's corner`, which tests/test_filter.py must reject."""
    u = np.asarray(u, f32)
    half = f32(0.5 + shift)
    if flt.kind == TENT:
        two_u = f32(2) * u
        with np.errstate(invalid="ignore"):
            w = np.where(u < f32(0.5), np.sqrt(two_u, dtype=f32) - f32(1), f32(1) - np.sqrt(np.maximum(f32(2) - two_u, f32(0)), dtype=f32)).astype(f32)
        return (np.float64(f32(flt.radius)) * w.astype(np.float64) + np.float64(half)).astype(f32)
    tab = table(flt) if tab is None else np.asarray(tab, f32)
    t = (u * f32(TABLE)).astype(f32)
    i = np.minimum(t.astype(np.int32), TABLE - 1)
    fr = (t - i.astype(f32)).astype(f32)
    a, b = tab[i], tab[i + 1]
    x = (fr.astype(np.float64) * (b - a).astype(f32).astype(np.float64) + a.astype(np.float64)).astype(f32)
    return (half + x).astype(f32)


def raw_tape(seed, pixel_key, n_spp, stride, sampler):
    """float32 [N, stride]: the unfiltered numbers of every sample of the pixel -- sampler_restatement's stream, or stratified_restatement's."""
    if sampler == SAMPLER_STRATIFIED:
        return S.tape(seed, pixel_key, n_spp, stride)
    return R.stream_floats(seed, S.pixel_keys(pixel_key, n_spp), stride)


def tape(seed, pixel_key, n_spp, stride, sampler, flt, tab=None, shift=0.0):
    """raw_tape's rows with columns 0 and 1 -- the camera sample -- replaced by the filter's offsets."""
    out = np.array(raw_tape(seed, pixel_key, n_spp, stride, sampler), f32)
    if flt is not None and flt.kind != BOX:
        out[:, 0] = warp(flt, out[:, 0], tab, shift)
        out[:, 1] = warp(flt, out[:, 1], tab, shift)
    return out


def table_deviation(flt, tab, n_u=1 << 16):
    """max |F(x(u)) - u| over u = (k + 0.5) / n_u: how far the piecewise-linear inverse CDF `tab` strays from the analytic one (x in double)."""
    u = (np.arange(n_u, dtype=np.float64) + 0.5) / n_u
    t = u * TABLE
    i = np.minimum(t.astype(np.int64), TABLE - 1)
    tab = np.asarray(tab, np.float64)
    x = tab[i] + (t - i) * (tab[i + 1] - tab[i])
    return float(np.abs(cdf(flt, x) - u).max())
