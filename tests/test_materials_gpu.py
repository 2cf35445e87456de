"""GPU: the lobes across material parameters that no shipped scene has -- exponents that are zero, fractional, odd, or large enough that the power underflows;
glass that is thinner than air, no interface at all, or diamond; colours that are black or above one -- through both pieces of lobe code the library holds: the
reference-shaped pair (kyhip_kat_bsdf: bsdf_sample / bsdf_eval_pdf) and what the render kernels execute (kyhip_kat_bsdf_continue: bsdf_continue /
bsdf_eval_parts), plus a small room whose plastic and matte surfaces are seen from behind.  The oracle is the reference restated (oracle/ky_oracle.cpp); a
non-integral exponent gives the reference's own NaN (std::pow of a negative base), and the device must put its NaN on the same entries.

Inputs: 4096 rows of test_parity_gpu.bsdf_inputs on seed 1 (26 % of them with n.wo < 0), the same for every material; the oracle's answer is computed once per
material and shared.

Tolerances are measured, not chosen (tools/measure_tolerances.py prints them): per material and per group of columns -- values, pdfs, directions -- the 0.999
quantile of the device's error against the oracle, MEASURED below; the bound is 4 x that, never below 2e-4 (directions: never below what test_kat_bsdf asks of
them), and 100 x the bound for the largest error.  Values and pdfs are relative on max(|c|, 1e-4) as in test_kat_bsdf, directions absolute."""
import numpy as np
import pytest

from helpers import CustomScene, make_light, make_material, make_shape, explain_pixel, prove_ties, rmse, unit
from test_parity_gpu import STRATEGIES, bsdf_inputs, film_tolerance, li_agreement

pytestmark = pytest.mark.gpu

N_ROWS = 4096
DIFFUSE, SPECULAR = (0.2, 0.15, 0.1), (0.6, 0.6, 0.6)
GLASS_R, GLASS_T = (1.0, 0.9, 0.8), (0.7, 0.8, 1.0)
BLACK = (0.0, 0.0, 0.0)
PLASTIC_EXPONENTS = [0.0, 0.5, 1.0, 2.0, 2.5, 7.0, 8.0, 151.0, 152.0, 1000.5, 20000.0]

# name -> (kind, c0, c1, eta, exponent)
GRID = {}
for _e in PLASTIC_EXPONENTS:
    GRID["plastic%g" % _e] = ("plastic", DIFFUSE, SPECULAR, 0.0, _e)
GRID["plastic8_black_diffuse"] = ("plastic", BLACK, SPECULAR, 0.0, 8.0)
GRID["plastic8_black_specular"] = ("plastic", DIFFUSE, BLACK, 0.0, 8.0)
for _eta in (0.75, 1.0, 1.0003, 1.33, 2.42):
    GRID["glass%g" % _eta] = ("glass", GLASS_R, GLASS_T, _eta, 0.0)
GRID["glass1.5_black_T"] = ("glass", GLASS_R, BLACK, 1.5, 0.0)
GRID["glass1.5_black_R"] = ("glass", BLACK, GLASS_T, 1.5, 0.0)
GRID["mirror_black"] = ("mirror", BLACK, BLACK, 0.0, 0.0)
GRID["mirror_bright"] = ("mirror", (1.2, 0.9, 0.5), BLACK, 0.0, 0.0)
GRID["matte_black"] = ("matte", BLACK, BLACK, 0.0, 0.0)
GRID["matte_bright"] = ("matte", (1.5, 0.2, 0.0), BLACK, 0.0, 0.0)

NON_INTEGRAL = ("plastic0.5", "plastic2.5", "plastic1000.5")
ODD = ("plastic1", "plastic7", "plastic151")
# the sampled-lobe flags the oracle gives on these inputs: reflection 1 | transmission 2, diffuse 4 | glossy 8 | specular 16
ORACLE_FLAGS = {"plastic": {5, 9}, "plastic8_black_diffuse": {9}, "plastic8_black_specular": {5}, "glass": {17, 18}, "glass1": {18}, "mirror": {17}, "matte": {5}}

V_COLS, P_COLS, WI_COLS = [0, 1, 2, 8, 9, 10], [6, 11], [3, 4, 5]          # kyhip_kat_bsdf's 13 columns: values, pdfs, the sampled direction
C_WEIGHT, C_PARTS, C_PDF, C_WI = [3, 4, 5], [8, 9, 10], [11], [0, 1, 2]      # kyhip_kat_bsdf_continue's 12 columns

FLOOR = 2e-4                                                                # the matte bound of test_kat_bsdf
WI_FLOOR = {"plastic": 5e-5, "glass": 2e-6, "mirror": 2e-6, "matte": 2e-6}  # test_kat_bsdf's bounds on the direction

# MEASURED[test][material] = the 0.999 quantile of the error of (values, pdfs, direction) on an MI355X (the largest error in brackets in the comment behind it)
MEASURED = {
    "grid": {
        "plastic0":                 (0.0e+00, 3.5e-06, 4.8e-07),   # max (0.0e+00, 4.1e-05, 1.3e-06)
        "plastic0.5":               (1.1e-06, 7.6e-06, 5.4e-07),   # max (1.8e-05, 4.1e-05, 3.6e-06)
        "plastic1":                 (4.3e-06, 1.7e-05, 5.1e-07),   # max (3.7e-05, 1.1e-04, 1.3e-06)
        "plastic2":                 (3.8e-06, 1.4e-05, 5.0e-07),   # max (1.6e-05, 4.7e-05, 1.3e-06)
        "plastic2.5":               (3.3e-06, 9.5e-06, 5.4e-07),   # max (7.9e-06, 4.1e-05, 1.4e-06)
        "plastic7":                 (3.7e-06, 5.0e-06, 6.8e-07),   # max (4.7e-06, 4.1e-05, 2.3e-06)
        "plastic8":                 (4.4e-06, 6.2e-06, 9.5e-07),   # max (5.4e-06, 4.1e-05, 3.8e-06)
        "plastic151":               (7.2e-05, 7.2e-05, 4.0e-06),   # max (8.1e-05, 8.1e-05, 6.0e-05)
        "plastic152":               (7.3e-05, 7.3e-05, 3.1e-06),   # max (9.1e-05, 9.1e-05, 6.0e-05)
        "plastic1000.5":            (4.8e-04, 4.8e-04, 6.2e-06),   # max (5.4e-04, 5.4e-04, 1.8e-05)
        "plastic20000":             (9.5e-03, 9.5e-03, 2.7e-05),   # max (1.2e-02, 1.2e-02, 7.6e-05)
        "plastic8_black_diffuse":   (4.6e-06, 5.1e-06, 8.1e-07),   # max (5.4e-06, 1.1e-05, 3.8e-06)
        "plastic8_black_specular":  (0.0e+00, 2.1e-05, 9.7e-07),   # max (0.0e+00, 4.4e-04, 6.5e-06)
        "glass0.75":                (3.0e-06, 2.2e-06, 4.2e-07),   # max (9.7e-06, 2.2e-05, 1.3e-06)
        "glass1":                   (5.7e-04, 0.0e+00, 3.7e-06),   # max (4.6e-03, 6.0e-08, 8.8e-06)
        "glass1.0003":              (7.9e-05, 1.2e-05, 1.6e-06),   # max (1.9e-03, 4.9e-04, 7.3e-06)
        "glass1.33":                (3.5e-06, 2.1e-06, 3.6e-07),   # max (1.8e-05, 1.8e-05, 6.3e-07)
        "glass2.42":                (2.4e-06, 9.5e-07, 5.6e-07),   # max (6.3e-06, 6.6e-06, 1.4e-06)
        "glass1.5_black_T":         (2.3e-06, 1.6e-06, 4.2e-07),   # max (1.2e-05, 2.4e-05, 1.8e-06)
        "glass1.5_black_R":         (1.0e-06, 1.6e-06, 4.2e-07),   # max (1.2e-05, 2.4e-05, 1.8e-06)
        "mirror_black":             (0.0e+00, 0.0e+00, 3.6e-07),   # max (0.0e+00, 0.0e+00, 4.2e-07)
        "mirror_bright":            (1.8e-06, 0.0e+00, 3.6e-07),   # max (6.3e-06, 0.0e+00, 4.2e-07)
        "matte_black":              (0.0e+00, 2.1e-05, 9.7e-07),   # max (0.0e+00, 4.4e-04, 6.5e-06)
        "matte_bright":             (0.0e+00, 2.1e-05, 9.7e-07),   # max (0.0e+00, 4.4e-04, 6.5e-06)
    },
    "continue": {
        "plastic0":                 (1.6e-05, 4.9e-07, 4.8e-07),   # max (4.7e-05, 1.8e-05, 1.3e-06)
        "plastic0.5":               (1.9e-05, 8.5e-06, 6.5e-07),   # max (2.3e-04, 1.8e-05, 3.6e-06)
        "plastic1":                 (1.9e-05, 1.7e-05, 5.2e-07),   # max (5.6e-04, 3.6e-05, 1.3e-06)
        "plastic2":                 (1.1e-05, 1.1e-05, 4.9e-07),   # max (4.2e-05, 1.8e-05, 1.3e-06)
        "plastic2.5":               (7.7e-06, 7.4e-06, 5.4e-07),   # max (6.4e-05, 1.8e-05, 1.3e-06)
        "plastic7":                 (7.7e-06, 4.1e-06, 7.9e-07),   # max (4.9e-05, 1.8e-05, 2.3e-06)
        "plastic8":                 (8.6e-06, 4.8e-06, 7.5e-07),   # max (3.2e-05, 1.8e-05, 3.8e-06)
        "plastic151":               (5.4e-05, 5.4e-05, 3.6e-06),   # max (6.3e-05, 6.3e-05, 3.2e-05)
        "plastic152":               (5.4e-05, 5.4e-05, 2.5e-06),   # max (6.1e-04, 6.4e-05, 6.2e-06)
        "plastic1000.5":            (3.6e-04, 3.6e-04, 6.3e-06),   # max (4.2e-04, 4.2e-04, 1.8e-05)
        "plastic20000":             (5.9e-03, 5.9e-03, 2.7e-05),   # max (3.8e-02, 7.1e-03, 7.6e-05)
        "plastic8_black_diffuse":   (1.2e-05, 4.8e-06, 4.8e-07),   # max (5.8e-05, 5.5e-06, 3.8e-06)
        "plastic8_black_specular":  (5.2e-07, 2.5e-06, 9.7e-07),   # max (1.2e-06, 2.1e-05, 6.5e-06)
        "glass0.75":                (2.8e-06, 0.0e+00, 4.2e-07),   # max (8.6e-06, 0.0e+00, 1.3e-06)
        "glass1":                   (3.8e-06, 0.0e+00, 3.7e-06),   # max (1.5e-05, 0.0e+00, 8.8e-06)
        "glass1.0003":              (2.4e-06, 0.0e+00, 1.6e-06),   # max (8.7e-06, 0.0e+00, 7.3e-06)
        "glass1.33":                (2.8e-06, 0.0e+00, 3.6e-07),   # max (8.6e-06, 0.0e+00, 6.3e-07)
        "glass2.42":                (2.8e-06, 0.0e+00, 5.6e-07),   # max (8.6e-06, 0.0e+00, 1.4e-06)
        "glass1.5_black_T":         (3.8e-06, 0.0e+00, 3.0e-07),   # max (8.6e-06, 0.0e+00, 3.6e-07)
        "glass1.5_black_R":         (2.1e-07, 0.0e+00, 4.7e-07),   # max (3.0e-07, 0.0e+00, 1.8e-06)
        "mirror_black":             (0.0e+00, 0.0e+00, 0.0e+00),   # max (0.0e+00, 0.0e+00, 0.0e+00)
        "mirror_bright":            (2.8e-06, 0.0e+00, 3.6e-07),   # max (8.6e-06, 0.0e+00, 4.2e-07)
        "matte_black":              (0.0e+00, 2.5e-06, 0.0e+00),   # max (0.0e+00, 2.1e-05, 0.0e+00)
        "matte_bright":             (4.4e-07, 2.5e-06, 9.7e-07),   # max (1.3e-06, 2.1e-05, 6.5e-06)
    },
    "skip": {
        152:                        (2.7e-40, 3.4e-40),   # max (2.7e-40, 3.4e-40)
        1000.5:                     (1.9e-34, 2.5e-34),   # max (1.9e-34, 2.5e-34)
        5000:                       (1.2e-17, 1.5e-17),   # max (1.2e-17, 1.6e-17)
        20000:                      (1.8e-06, 1.8e-06),   # max (1.8e-06, 1.9e-06)
    },
}


def material(A, name):
    kind, c0, c1, eta, exponent = GRID[name]
    return make_material(A, {"plastic": A.MATERIAL_PLASTIC, "glass": A.MATERIAL_GLASS, "mirror": A.MATERIAL_MIRROR, "matte": A.MATERIAL_MATTE}[kind], c0, c1, eta=eta, exponent=exponent)


def bounds(test, name):
    """(values, pdfs, direction) bounds of one material in one test: 4 x the measured quantile, floored"""
    q = MEASURED[test][name]
    return max(4 * q[0], FLOOR), max(4 * q[1], FLOOR), max(4 * q[2], WI_FLOOR[GRID[name][0]])


_inputs = {}
_oracle = {}


def inputs(seed=1):
    if seed not in _inputs:
        _inputs[seed] = bsdf_inputs(np.random.default_rng(seed), N_ROWS)
        _inputs[seed].setflags(write=False)
    return _inputs[seed]


def oracle_rows(A, O, name):
    """O.kat_bsdf of one material on the shared inputs: computed once, read-only"""
    if name not in _oracle:
        _oracle[name] = O.kat_bsdf(material(A, name), inputs())
        _oracle[name].setflags(write=False)
    return _oracle[name]


def rel_err(g, c):
    """test_kat_bsdf's error: relative, with everything below 1e-4 (denormal results among it) measured against 1e-4.  Entries that are NaN on both sides count 0."""
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    err = np.abs(g - c) / np.maximum(np.abs(c), 1e-4)
    return np.where(np.isnan(g) & np.isnan(c), 0.0, err)


def abs_err(g, c):
    """assert_close_q's error: |g - c| / max(1, |c|)"""
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    return np.abs(g - c) / np.maximum(1.0, np.abs(c))


def figures(err):
    """(0.999 quantile, maximum) of an error array; (0, 0) of an empty one"""
    err = np.asarray(err, np.float64).ravel()
    return (float(np.quantile(err, 0.999)), float(err.max())) if err.size else (0.0, 0.0)


def check_figures(what, err, bound):
    q, top = figures(err)
    print("%s: quantile %.3e max %.3e bound %.3e" % (what, q, top, bound))
    assert q <= bound, (what, q, bound)
    assert top <= 100 * bound, (what, top, 100 * bound)


def expected_continue(c, x):
    """What path_tracing_iteration_t makes of the oracle's BSDF sample (4586-4597), in float64 from O.kat_bsdf's rows: the direction, the factor
    f |n.wi| / pdf, whether the path goes on -- pdf != 0 and f not black, where a NaN channel is not black (4588) --, and the specular flag."""
    c64, n = np.asarray(c, np.float64), np.asarray(x[:, 0:3], np.float64)
    f, wi, pdf = c64[:, 0:3], c64[:, 3:6], c64[:, 6]
    with np.errstate(all="ignore"):
        weight = f * np.abs((n * wi).sum(1))[:, None] / pdf[:, None]
        ok = (pdf != 0) & ~(f <= 0).all(1)
    return {"wi": wi, "weight": weight, "ok": ok, "specular": c64[:, 12], "parts": c64[:, 8:11], "pdf": c64[:, 11]}


def grid_errors(g, c):
    """kyhip_kat_bsdf against the oracle on the rows whose sampled flags agree: the errors of (values, pdfs, direction)"""
    same = g[:, 7] == c[:, 7]
    gs, cs = g[same], c[same]
    return rel_err(gs[:, V_COLS], cs[:, V_COLS]), rel_err(gs[:, P_COLS], cs[:, P_COLS]), abs_err(gs[:, WI_COLS], cs[:, WI_COLS])


def continue_errors(k, e, same):
    """kyhip_kat_bsdf_continue against expected_continue: weight and the parts' values / the parts' pdf / the direction.  Weight and direction on the rows where
    both sides continue the path, the parts on every row of `same`."""
    both = same & e["ok"] & (k[:, 6] != 0)
    values = np.concatenate([rel_err(k[both][:, C_WEIGHT], e["weight"][both]).ravel(), rel_err(k[same][:, C_PARTS], e["parts"][same]).ravel()])
    return values, rel_err(k[same][:, C_PDF], e["pdf"][same][:, None]), abs_err(k[both][:, C_WI], e["wi"][both])


def cos_o_of(x):
    return (np.asarray(x[:, 0:3], np.float64) * np.asarray(x[:, 3:6], np.float64)).sum(1)


def flag_set(name):
    kind = GRID[name][0]
    return ORACLE_FLAGS.get(name, ORACLE_FLAGS[kind])


@pytest.mark.parametrize("name", list(GRID))
def test_kat_bsdf_grid(name, A, api, O):
    x, c = inputs(), oracle_rows(A, O, name)
    g = api.kat_bsdf(material(A, name), x)
    assert np.array_equal(g[:, 12], c[:, 12])                                         # is_delta
    assert set(c[:, 7].astype(int)) == flag_set(name)
    same = g[:, 7] == c[:, 7]
    assert same.mean() >= 0.999, (name, int((~same).sum()))                           # lobe picks and Fresnel ties: the bound of test_kat_bsdf
    gs, cs = g[same], c[same]
    # NaN on the same entries; nothing infinite on either side
    assert np.array_equal(np.isnan(gs), np.isnan(cs)), (name, int(np.isnan(gs).sum()), int(np.isnan(cs).sum()))
    assert not np.isinf(c).any() and not np.isinf(g).any()
    nan_share = np.isnan(c).any(axis=1).mean()
    if name in NON_INTEGRAL:     # std::pow(negative, non-integer): the eval columns of rows in wo's hemisphere with a negative cosine to the mirror direction
        assert 0.03 <= nan_share <= 0.08, (name, nan_share)
        assert not np.isnan(c[:, [0, 1, 2, 3, 4, 5, 6, 7, 11, 12]]).any()
    else:
        assert nan_share == 0 and not np.isnan(g).any()
    b_val, b_pdf, b_wi = bounds("grid", name)
    e_val, e_pdf, e_wi = grid_errors(g, c)
    check_figures(name + " values", e_val, b_val)
    check_figures(name + " pdfs", e_pdf, b_pdf)
    q, top = figures(e_wi)
    print("%s direction: quantile %.3e max %.3e bound %.3e" % (name, q, top, b_wi))
    assert q <= b_wi and top <= max(100 * b_wi, 2e-3), (name, q, top, b_wi)            # (test_kat_bsdf's hard bound where 100 x the bound is below it)
    if name == "plastic0":       # pow(x, 0) = 1: the pdf is the lobe's norm (0 + 1) / 2 pi, whatever the direction
        norm = np.float32(0.15915494309189535)
        at = c[:, 11] == norm
        assert at[c[:, 7] == 9].all() and at.sum() > 1000
        assert (g[at, 11] == norm).all()
    if name in ODD:              # an odd power of a negative base is negative
        neg = cs[:, 8:11] < -1e-30                                                     # (below that a result is a zero on the scale of rel_err)
        assert neg.sum() > 30, (name, int(neg.sum()))
        assert (gs[:, 8:11][neg] < 0).all()
    if name == "glass1":         # no interface: the Fresnel term is 0, nothing reflects
        assert (g[:, 7] == 18).all() and (c[:, 7] == 18).all()
    if name.startswith("glass"):  # total internal reflection in the refraction branch (f = 0, pdf = 0) on the same rows
        assert np.array_equal(gs[:, 6] == 0, cs[:, 6] == 0)


def moved_row(row, rng_, eps=3e-5):
    """the row with its random numbers and wo moved by eps (tie proofs: helpers.prove_ties)"""
    r = row.copy()
    r[6:8] = np.clip(r[6:8] + eps * rng_.uniform(-1, 1, 2), 0.0, np.float32(1) - np.float32(2.0 ** -24)).astype(np.float32)
    r[3:6] = unit(r[3:6] + eps * rng_.uniform(-1, 1, 3)).astype(np.float32)
    return r


@pytest.mark.parametrize("name", list(GRID))
def test_kat_bsdf_continue(name, A, api, O):
    x, c = inputs(), oracle_rows(A, O, name)
    m = material(A, name)
    e = expected_continue(c, x)
    k = api.kat_bsdf_continue(m, x, flat_phong=False)
    g = api.kat_bsdf(m, x)
    same = g[:, 7] == c[:, 7]
    assert same.mean() >= 0.999
    assert set(np.unique(k[:, 6])) <= {0.0, 1.0}
    assert np.array_equal(k[:, 7], e["specular"])
    # whether the path goes on
    k_ok = k[:, 6] != 0
    differ = same & (k_ok != e["ok"])
    print("%s ok: %d of %d rows differ, %d continue" % (name, int(differ.sum()), N_ROWS, int(e["ok"].sum())))
    if GRID[name][0] in ("mirror", "glass"):   # a delta lobe ends a path on a black colour or a pdf of 0: a constant of the material and a branch both sides took alike
        assert not differ.any()
    assert differ.sum() <= 1e-3 * N_ROWS, (name, int(differ.sum()))
    cos_o = cos_o_of(x)
    for i in np.flatnonzero(differ):       # every exception is a tie: u1 at 0 (the Phong sample's pdf underflows there), or the sample in the surface's plane
        cos_i = float((np.asarray(x[i, 0:3], np.float64) * e["wi"][i]).sum())
        assert x[i, 7] <= 2.0 ** -23 or abs(cos_o[i] * cos_i) <= 1e-6, (name, i, x[i], k[i], c[i])
    prove_ties([(i, x[i]) for i in np.flatnonzero(differ)], lambda i: bool(k_ok[i]),
               lambda row: bool(expected_continue(O.kat_bsdf(m, row[None]), row[None])["ok"][0]), moved_row, np.random.default_rng(3), "path continues, " + name)
    if name in ("mirror_black", "matte_black"):
        assert not k_ok.any() and not e["ok"].any()
    if name in ("glass1.5_black_T", "glass1.5_black_R"):   # ... ends exactly on the rows that took the black branch
        ended = c[:, 7] == (18 if name.endswith("T") else 17)
        assert ended.sum() > 100 and (~ended).sum() > 100 and np.array_equal(e["ok"], ~ended)
    if name in ("plastic8_black_diffuse", "plastic8_black_specular"):
        assert set(g[:, 7].astype(int)) == flag_set(name)
    # where both continue: the direction and the factor; the two-factor evaluation against eval / pdf on every row, NaN where the oracle's is
    assert np.array_equal(np.isnan(k[same][:, 8:12]), np.isnan(c[same][:, 8:12]))
    both = same & e["ok"] & k_ok
    assert not np.isnan(k[both][:, 0:6]).any() and np.isfinite(e["weight"][both]).all()
    b_val, b_pdf, b_wi = bounds("continue", name)
    e_val, e_pdf, e_wi = continue_errors(k, e, same)
    check_figures(name + " weight and parts", e_val, b_val)
    check_figures(name + " parts' pdf", e_pdf, b_pdf)
    q, top = figures(e_wi)
    print("%s direction: quantile %.3e max %.3e bound %.3e" % (name, q, top, b_wi))
    assert q <= b_wi and top <= max(100 * b_wi, 2e-3), (name, q, top, b_wi)
    # the flat-Phong variant drops the back-side flip and nothing else: from the front it is the same code, bit for bit
    flat = api.kat_bsdf_continue(m, x, flat_phong=True)
    front = cos_o >= 0
    assert np.array_equal(flat[front].view(np.uint32), k[front].view(np.uint32))
    assert (cos_o < 0).mean() >= 0.2
    if name == "plastic8":       # behind a Phong lobe the flip moves the sample away from the lobe's axis: the reference ends some of those paths and continues others
        back_phong = (cos_o < 0) & (c[:, 7] == 9)
        assert (back_phong & e["ok"]).sum() > 50 and (back_phong & ~e["ok"]).sum() > 50
        assert not np.array_equal(flat[back_phong].view(np.uint32), k[back_phong].view(np.uint32))   # (and the flip is there to be dropped)


# ---- the wave-wide skip of the Phong power (phong_pow_lobe) ----

SKIP_EXPONENTS = [152.0, 1000.5, 5000.0, 20000.0]


def power_floor(exponent):
    """DMat::exp_flags' upper half as documented: F = 2^(-151 / exponent) in float32, cut to its upper 16 bits"""
    f = np.exp2(np.float32(-151.0) / np.float32(exponent), dtype=np.float32)
    return (np.array([f], np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)[0]


def skip_rows(exponent):
    """Waves of 64 rows with the normal along z and wo = n, so that the mirror direction is n and wi_eval = (sin, 0, cos) has cos_alpha = cos exactly on both
    sides.  -> (rows, {wave name: slice}).  A row with a NEGATIVE cos_alpha in wo's hemisphere needs a tilted wo: wo and wi 60 degrees off the normal on the same
    side, cos_alpha = cos 120 = -0.5 (below every F here)."""
    F = float(power_floor(exponent))
    integral = float(exponent).is_integer()
    rng_ = np.random.default_rng(int(exponent))
    top = min(F * (1 + 2.0 ** -6), 1.0)
    waves = {}
    cos = []

    def add(name, values):
        assert len(values) % 64 == 0
        waves[name] = slice(len(cos), len(cos) + len(values))
        cos.extend(values)
    below = rng_.uniform(0.5 * F, F, 64)
    below[0], below[1] = F, 0.0
    if integral:
        below[2::2] *= -1                                               # (wo = n: these leave wo's hemisphere, the power is skipped all the same)
    add("skip", list(below))
    band = np.sort(rng_.uniform(F, top, 8 * 64))                        # eight waves in ascending order: each covers an eighth of the band
    band[0], band[-1] = F, top
    add("band", list(band))
    vote = list(below)
    vote[17] = 0.999
    add("vote", vote)
    add("band_vote", list(band[:63]) + [0.999])                         # the band's first wave with a lane that forces the power: the skip must not show
    add("first_normal", list(rng_.uniform(2.0 ** (-122.0 / exponent), 2.0 ** (-118.0 / exponent), 64)))   # the power's first results that are normal floats
    if not integral:
        add("negative", list(np.abs(below)))
    c = np.array(cos, np.float64)
    n = len(c)
    rows = np.zeros((n, 12), np.float32)
    rows[:, 2] = 1.0
    rows[:, 5] = 1.0
    rows[:, 6:8] = rng_.uniform(0.05, 0.95, (n, 2))
    rows[:, 8], rows[:, 10] = np.sqrt(np.maximum(0.0, 1 - c * c)), c
    rows[:, 11] = 0.0                                                   # lobe_u = 0: the Phong lobe
    if not integral:                                                    # one lane of an otherwise skipped wave with a negative base in wo's hemisphere: NaN, on that row only
        i = waves["negative"].start + 29
        s, h = np.sqrt(0.75), 0.5
        rows[i, 3:6] = (s, 0.0, h)
        rows[i, 8:11] = (s, 0.0, h)
    return rows, waves


def skip_errors(g, c, waves):
    """the band's errors: (values, pdfs); directions are not what these rows are about"""
    b = waves["band"]
    return rel_err(g[b][:, 8:11], c[b][:, 8:11]), rel_err(g[b][:, [11]], c[b][:, [11]])


@pytest.mark.parametrize("exponent", SKIP_EXPONENTS)
def test_phong_power_skip(exponent, A, api, O):
    m = make_material(A, A.MATERIAL_PLASTIC, DIFFUSE, SPECULAR, exponent=exponent)
    rows, waves = skip_rows(exponent)
    F = power_floor(exponent)
    assert 0 < F < 1 and float(exponent) * np.log2(np.float64(F)) <= -150
    g, c = api.kat_bsdf(m, rows), O.kat_bsdf(m, rows)
    k = api.kat_bsdf_continue(m, rows, flat_phong=False)
    ev, kv = [8, 9, 10, 11], [8, 9, 10, 11]
    assert (c[:, 7] == 9).all() and (g[:, 7] == 9).all()
    # zero exactly where the oracle's is zero, in every wave and through both evaluations; NaN where the oracle's is
    zero = c[:, ev] == 0
    assert zero[waves["skip"]].all() and zero.mean() > 0.1
    assert (g[:, ev][zero] == 0).all() and (k[:, kv][zero] == 0).all()
    assert np.array_equal(np.isnan(g[:, ev]), np.isnan(c[:, ev])) and np.array_equal(np.isnan(k[:, kv]), np.isnan(c[:, ev]))
    if "negative" in waves:
        w = waves["negative"]
        lane = np.isnan(c[w][:, 8:11]).all(axis=1)
        assert lane.sum() == 1 and lane[29] and not np.isnan(c[:, 11]).any()
        assert np.isnan(c[:, ev]).sum() == 3
    else:
        assert not np.isnan(c).any()
    # the lane that forces the vote has its value, the others their zeros
    v = waves["vote"].start + 17
    assert c[v, 11] > 0 and rel_err(g[v, ev], c[v, ev]).max() <= bounds_skip(exponent)[0]
    # the skip does not show: rows evaluated alone and next to a lane that forces the power give the same bits
    first = slice(waves["band"].start, waves["band"].start + 63)
    again = slice(waves["band_vote"].start, waves["band_vote"].start + 63)
    assert np.array_equal(g[first][:, ev].view(np.uint32), g[again][:, ev].view(np.uint32))
    assert np.array_equal(k[first][:, kv].view(np.uint32), k[again][:, kv].view(np.uint32))
    others = np.arange(64) != 17                                                              # (the vote wave differs from the skipped one in lane 17 only; -0 and +0 are one zero)
    assert np.array_equal(g[waves["skip"]][others][:, ev].view(np.uint32) & 0x7FFFFFFF, g[waves["vote"]][others][:, ev].view(np.uint32) & 0x7FFFFFFF)
    # ... and F is not too large: a whole wave whose powers are normal floats, 2^-122 and more, has them (on rel_err's scale they would pass as zeros).  This is where a
    # bound that is too high shows on the device: its exp2 gives zero for everything below 2^-126, so a margin of -140 in place of -151 changes no result (tried: this
    # test passes, a margin of -100 fails here), and the margin itself is held by the host's test (tests/test_materials.py: e log2 F <= -150)
    w = waves["first_normal"]
    assert (np.abs(c[w][:, ev]) >= 2.0 ** -126).all()
    assert (g[w][:, ev] != 0).all() and (k[w][:, kv] != 0).all()
    # just above F both sides agree (a denormal result is a zero on rel_err's scale)
    b_val, b_pdf = bounds_skip(exponent)
    e_val, e_pdf = skip_errors(g, c, waves)
    check_figures("exponent %g band values" % exponent, e_val, b_val)
    check_figures("exponent %g band pdfs" % exponent, e_pdf, b_pdf)
    e_val, e_pdf = skip_errors(k, c, waves)
    check_figures("exponent %g band parts" % exponent, e_val, b_val)
    check_figures("exponent %g band parts' pdf" % exponent, e_pdf, b_pdf)


def bounds_skip(exponent):
    q = MEASURED["skip"][exponent]
    return max(4 * q[0], FLOOR), max(4 * q[1], FLOOR)


# ---- a room whose plastic and matte surfaces are seen from behind ----

ROOM_W, ROOM_H = 48, 40
# caller's surface indices of the surfaces the room is about
ROOM_FLOOR, ROOM_TRIANGLE, ROOM_PLASTIC_DISK, ROOM_MATTE_DISK, ROOM_GLASS, ROOM_GLASS_BLACK_T, ROOM_MIRROR = 0, 5, 6, 7, 8, 9, 10


def materials_room(A, api):
    """A matte room (camera at +y looking along -y, z up; the wall behind the camera is open) with a rectangle lamp under the ceiling and a point light, and in it:
    a free-standing plastic triangle (exponent 2) whose stored normal points away from the camera; a plastic disk (exponent 7) that faces the camera and turns its
    back to the lamp; a matte disk facing away from the camera; a glass ball of eta 1.33 with R != T; a glass ball that transmits nothing; a mirror brighter than
    white in one channel; and a plastic floor of exponent 0.  Triangles and disks keep their stored normal (only rectangles turn towards the ray), so these are
    the vertices with n.wo < 0, and a plastic surface that is no rectangle takes KY_FEAT_FLAT_PHONG from the scene."""
    cam = api.cornell_box_scene(A.CB_DEFAULT_SCENE, ROOM_W, ROOM_H)
    camera = A.Camera.from_buffer_copy(cam.c.camera)
    S = A
    shapes = [
        make_shape(A, S.SHAPE_RECTANGLE, [(-1.3, -1.3, -1.28), (1.3, -1.3, -1.28), (1.3, 1.3, -1.28), (-1.3, 1.3, -1.28)]),          # 0 floor
        make_shape(A, S.SHAPE_RECTANGLE, [(-1.3, -1.3, -1.28), (-1.3, -1.3, 1.28), (1.3, -1.3, 1.28), (1.3, -1.3, -1.28)]),          # 1 back wall
        make_shape(A, S.SHAPE_RECTANGLE, [(-1.3, -1.3, -1.28), (-1.3, 1.3, -1.28), (-1.3, 1.3, 1.28), (-1.3, -1.3, 1.28)]),          # 2 left wall
        make_shape(A, S.SHAPE_RECTANGLE, [(1.3, -1.3, -1.28), (1.3, 1.3, -1.28), (1.3, 1.3, 1.28), (1.3, -1.3, 1.28)]),              # 3 right wall
        make_shape(A, S.SHAPE_RECTANGLE, [(-1.3, -1.3, 1.28), (1.3, -1.3, 1.28), (1.3, 1.3, 1.28), (-1.3, 1.3, 1.28)]),              # 4 ceiling
        make_shape(A, S.SHAPE_TRIANGLE, [(-1.05, -0.35, -0.9), (-0.15, -0.25, -0.9), (-0.6, -0.3, 0.15)]),                           # 5 plastic triangle, normal towards -y
        make_shape(A, S.SHAPE_DISK, [(0.65, -0.2, -0.25)], normal=tuple(unit(np.array([0.2, 0.9, -0.5]))), radius=0.38),             # 6 plastic disk: faces the camera, back to the lamp
        make_shape(A, S.SHAPE_DISK, [(-0.7, -0.1, 0.7)], normal=tuple(unit(np.array([0.1, -1.0, 0.25]))), radius=0.3),               # 7 matte disk, normal away from the camera
        make_shape(A, S.SHAPE_SPHERE, [(0.15, 0.35, -0.93)], radius=0.35),                                                            # 8 glass ball, eta 1.33
        make_shape(A, S.SHAPE_SPHERE, [(-0.8, 0.55, -0.98)], radius=0.3),                                                             # 9 glass ball, black T
        make_shape(A, S.SHAPE_RECTANGLE, [(1.25, -1.0, -0.6), (1.25, 0.2, -0.6), (1.25, 0.2, 0.6), (1.25, -1.0, 0.6)]),                 # 10 mirror on the right wall
        make_shape(A, S.SHAPE_RECTANGLE, [(-0.4, -0.4, 1.25), (0.4, -0.4, 1.25), (0.4, 0.4, 1.25), (-0.4, 0.4, 1.25)], flip=True),    # 11 lamp (faces down)
    ]
    materials = [
        make_material(A, S.MATERIAL_PLASTIC, DIFFUSE, SPECULAR, exponent=0.0),                    # 0 floor
        make_material(A, S.MATERIAL_MATTE, (0.7, 0.7, 0.7)),                                      # 1 walls
        make_material(A, S.MATERIAL_MATTE, (0.2, 0.6, 0.3)),                                      # 2 left wall, matte disk
        make_material(A, S.MATERIAL_PLASTIC, DIFFUSE, SPECULAR, exponent=2.0),                    # 3 triangle
        make_material(A, S.MATERIAL_PLASTIC, (0.1, 0.15, 0.3), SPECULAR, exponent=7.0),           # 4 plastic disk
        make_material(A, S.MATERIAL_GLASS, GLASS_R, GLASS_T, eta=1.33),                           # 5
        make_material(A, S.MATERIAL_GLASS, GLASS_R, BLACK, eta=1.5),                              # 6
        make_material(A, S.MATERIAL_MIRROR, (1.2, 0.9, 0.5)),                                     # 7
        make_material(A, S.MATERIAL_MATTE, BLACK),                                                # 8 lamp backing
    ]
    lights = [make_light(A, S.LIGHT_AREA, (18, 16, 12), shape=11), make_light(A, S.LIGHT_POINT, (0.3, 0.3, 0.3), position=(0.0, 0.9, 0.9))]
    surfaces = [A.Surface(0, 0, -1), A.Surface(1, 1, -1), A.Surface(2, 2, -1), A.Surface(3, 1, -1), A.Surface(4, 1, -1), A.Surface(5, 3, -1), A.Surface(6, 4, -1),
                A.Surface(7, 2, -1), A.Surface(8, 5, -1), A.Surface(9, 6, -1), A.Surface(10, 7, -1), A.Surface(11, 8, 0)]
    return CustomScene(A, camera, shapes, materials, lights, surfaces)


# one pixel per surface the room is about (its first hit there, found with the oracle), and one on the back wall; every oracle sample of them is finite
ROOM_PIXELS = {(30, 36): ROOM_FLOOR, (16, 24): ROOM_TRIANGLE, (30, 22): ROOM_PLASTIC_DISK, (14, 11): ROOM_MATTE_DISK, (24, 32): ROOM_GLASS, (10, 31): ROOM_GLASS_BLACK_T,
               (37, 20): ROOM_MIRROR, (24, 20): 1}
FEAT_FLAT_PHONG = 2048


def kernel_modes(lib):
    """the library's kernel choice as the suite runs it, and -- where that is run-time instantiation -- the table's kernels as well"""
    now = lib.kyhip_set_jit(0)
    lib.kyhip_set_jit(now)
    return [now] if now == 0 else [now, 0]


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_materials_room(strategy, A, api, O):
    import re
    scene = materials_room(A, api)
    lib = A.load_kyhip()
    assert not api.scene_facts(scene) & FEAT_FLAT_PHONG                               # a plastic triangle and a plastic disk: the flip behind a Phong lobe is live code
    params = api.make_params(ROOM_W, ROOM_H, 128, direct_sample=strategy)
    pixels = list(ROOM_PIXELS)
    finite = total = 0
    for (x, y), surface in ROOM_PIXELS.items():
        rows = O.trace_li(scene, params, x, y, 0)
        assert int(rows[0, 1]) == surface, ((x, y), int(rows[0, 1]), surface)
        if surface in (ROOM_TRIANGLE, ROOM_MATTE_DISK):
            assert float(np.dot(rows[0, 6:9], rows[0, 9:12])) < -0.5                    # seen from behind
        c = O.li(scene, params, x, y, 0, 128)
        finite += int(np.isfinite(c).all(1).sum())
        total += 128
    assert finite >= 0.99 * total
    prev = lib.kyhip_set_jit(0)
    lib.kyhip_set_jit(prev)
    try:
        for mode in kernel_modes(lib):
            lib.kyhip_set_jit(mode)
            bad, tot, sg, sc = li_agreement(api, O, scene, params, pixels)
            print("room, strategy %d, kernel mode %d: %d of %d samples differ, sums %.6f %.6f" % (strategy, mode, bad, tot, sg, sc))
            # test_general_shapes_scene's rule: at most 0.2 % of the samples differ, and each of them is explained vertex by vertex (helpers.explain_pixel)
            assert bad <= 0.002 * tot, (bad, tot)
            assert abs(sg - sc) <= 1e-3 * max(sc, 1.0)
            if bad:
                for (x, y) in pixels:
                    explain_pixel(api, O, scene, params, x, y)
            if strategy == 48:
                p = api.make_params(ROOM_W, ROOM_H, 512, tile_w=16, tile_h=8)
                g, c = api.render(scene, p), O.render(scene, p)
                kernel = lib.kyhip_last_kernel(0).decode()
                feat = re.search(r"feat (\d+)", kernel)
                assert feat and not int(feat.group(1)) & FEAT_FLAT_PHONG, kernel         # the launch did not carry the flat-Phong fact
                assert c.mean() > 0.02 and np.isfinite(g).all() and np.isfinite(c).all()
                assert rmse(g, c) < film_tolerance(512), rmse(g, c)
    finally:
        lib.kyhip_set_jit(prev)
