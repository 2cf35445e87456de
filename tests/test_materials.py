"""CPU: what the host leaves a material's lobes in DMat::exp_flags (pack_material, ky_amd/csrc/ky_pack.cpp) -- whether the exponent is integral and odd (the sign and
the NaN of a negative base's power), whether the two colours are black (bsdf_continue reads that in place of is_black(bs.f)), and the bound F below which a whole
wavefront skips the Phong power -- through kyhostcheck_material (ky_amd/csrc/ky_hostcheck.cpp: the file the sanitizer builds hold too), against Python's arithmetic."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import make_material

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPONENTS = [1e-3, 0.5, 1.0, 2.0, 3.0, 151.0, 152.0, 5000.0, 1e6, 16777216.0, 3e38, 0.0, -1.0, math.inf, math.nan]


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_material: the sanitizer build when the suite runs inside `make sanitize`, else the same sources built plainly."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    lib.kyhostcheck_material.restype, lib.kyhostcheck_material.argtypes = A.KYHOSTCHECK_SYMBOLS["kyhostcheck_material"]
    return lib


def packed(check, m):
    """(exp_flags, c0 as packed, c1 as packed)"""
    flags = C.c_int32(0)
    colours = np.zeros(6, np.float32)
    assert check.kyhostcheck_material(C.byref(m), C.byref(flags), colours.ctypes.data) == 0
    return flags.value & 0xFFFFFFFF, colours[:3], colours[3:]


def power_floor(flags):
    return np.array([flags & 0xFFFF0000], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("exponent", EXPONENTS, ids=lambda e: "%g" % e)
def test_exponent_bits(exponent, A, check):
    m = make_material(A, A.MATERIAL_PLASTIC, (0.2, 0.15, 0.1), (0.6, 0.6, 0.6), exponent=exponent)
    e = float(np.float32(exponent))                                    # the exponent as the material holds it
    flags, c0, c1 = packed(check, m)
    # bit 0: std::pow(negative, e) has a value; bit 1: that value is negative.  (Every float of 2^24 or more is an even integer.)
    integral = math.isfinite(e) and e.is_integer()
    odd = integral and int(abs(e)) % 2 == 1
    assert bool(flags & 1) == integral and bool(flags & 2) == odd, (exponent, hex(flags))
    assert flags & 4 and flags & 8                                      # neither lobe's colour is black
    F = float(power_floor(flags))
    assert flags & 0xFFF0 == 0                                          # (nothing else lives in the word)
    if not (math.isfinite(e) and e > 0):
        assert F == 0.0, (exponent, F)
    elif F != 0.0:   # a bound is optional (0: nothing is skipped), a wrong one is not: |x|^e must lie below the smallest denormal, 2^-149, with room for the device's logarithm
        assert 0.0 < F < 1.0
        assert e * math.log2(F) <= -150.0, (exponent, F, e * math.log2(F))
    if exponent in (151.0, 152.0, 5000.0, 1e6):                         # ... and where 2^(-151 / e) is a float inside (0, 1) it is there
        want = np.array([np.exp2(np.float32(-151.0) / np.float32(e), dtype=np.float32)], np.float32).view(np.uint32)[0] & 0xFFFF0000
        assert flags & 0xFFFF0000 == int(want) and F > 0.0


def test_exponent_bound_is_plastic_only(A, check):
    for kind, kw in ((A.MATERIAL_MATTE, {}), (A.MATERIAL_MIRROR, {}), (A.MATERIAL_GLASS, {"eta": 1.5})):
        flags, _, _ = packed(check, make_material(A, kind, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), exponent=90.0, **kw))
        assert flags & 0xFFFF0000 == 0


def test_black_bits(A, check):
    """color_t::is_black is `every channel <= 0`: a NaN channel is NOT black, and neither is a colour with one positive channel among negative ones."""
    nan = math.nan
    cases = [((0, 0, 0), False), ((0, 0, 1e-30), True), ((-1, -2, 0), False), ((-1, 0.5, -1), True), ((nan, 0, 0), True), ((nan, nan, nan), True), ((0, -0.0, 0), False),
             ((1.5, 0.2, 0), True), ((math.inf, 0, 0), True)]
    for kind, kw in ((A.MATERIAL_MATTE, {}), (A.MATERIAL_MIRROR, {}), (A.MATERIAL_GLASS, {"eta": 1.5})):
        for colour, lit in cases:
            for other, other_lit in cases[:2]:
                flags, c0, c1 = packed(check, make_material(A, kind, colour, other, **kw))
                assert bool(flags & 4) == lit and bool(flags & 8) == other_lit, (kind, colour, other, hex(flags))
                flags, _, _ = packed(check, make_material(A, kind, other, colour, **kw))
                assert bool(flags & 4) == other_lit and bool(flags & 8) == lit, (kind, colour, other, hex(flags))


def test_black_bits_of_plastic_lobes(A, check):
    """Plastic divides each lobe's colour by the lobe's probability: a black diffuse colour has probability 0 and packs as 0 / 0 = NaN, which is not black -- like
    the reference's own Kd / 0 --, and the lobe is never picked; the Phong lobe's factor c1 = cs (n + 2) / (n + 1) is black when the specular colour is 0 / 0 likewise."""
    flags, c0, c1 = packed(check, make_material(A, A.MATERIAL_PLASTIC, (0, 0, 0), (0.6, 0.6, 0.6), exponent=8.0))
    assert np.isnan(c0).all() and flags & 4 and flags & 8
    assert np.allclose(c1, 0.6 * 10.0 / 9.0, rtol=1e-6)
    flags, c0, c1 = packed(check, make_material(A, A.MATERIAL_PLASTIC, (0.2, 0.15, 0.1), (0, 0, 0), exponent=8.0))
    assert np.isnan(c1).all() and flags & 4 and flags & 8
    assert np.allclose(c0, (0.2, 0.15, 0.1), rtol=1e-6)
    # a lobe that is picked and black: the bit is clear
    m = make_material(A, A.MATERIAL_PLASTIC, (0.2, 0.15, 0.1), (0.6, 0.6, 0.6), exponent=8.0)
    for j in range(3):
        m.color1[j] = 0.0
    flags, c0, c1 = packed(check, m)
    assert flags & 4 and not flags & 8 and (c1 == 0).all()
    m = make_material(A, A.MATERIAL_PLASTIC, (0.2, 0.15, 0.1), (0.6, 0.6, 0.6), exponent=8.0)
    for j in range(3):
        m.color0[j] = -0.5
    flags, c0, c1 = packed(check, m)
    assert not flags & 4 and flags & 8
