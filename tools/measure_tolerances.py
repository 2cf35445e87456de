import sys, os
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "/root/repo")); sys.path.insert(0, os.path.join(os.environ.get("GRAFT_REPO_ROOT", "/root/repo"), "tests"))
import numpy as np
from ky_amd import _abi as A, api
from oracle import kyoracle as O
def rmse(a,b): return float(np.sqrt(np.mean((np.asarray(a,np.float64)-np.asarray(b,np.float64))**2)))
ONLY = sys.argv[1:]   # nothing: every section; "frames": films, per-sample radiance and the noise estimate; "materials": the lobes across material parameters
if not ONLY or "frames" in ONLY:
    for (w, h, spp, depth) in ((1, 1, 1, 5), (13, 7, 3, 5), (13, 7, 64, 0), (13, 7, 16, 250)):
        sc = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h); p = api.make_params(w, h, spp, max_path_depth=depth)
        print("edge", w, h, spp, depth, "%.3e" % rmse(api.render(sc, p), O.render(sc, p)))
    for case in ["cornell_area", "cornell_env", "cornell_point", "cornell_direction", "veach", "cornell_depth16", "direct_lighting"]:
        kw = {}
        if case != "veach":
            flag = {"cornell_area": A.CB_LIGHT_AREA, "cornell_env": A.CB_LIGHT_ENVIRONMENT, "cornell_point": A.CB_LIGHT_POINT, "cornell_direction": A.CB_LIGHT_DIRECTION, "cornell_depth16": A.CB_LIGHT_AREA, "direct_lighting": A.CB_LIGHT_AREA}[case]
            W, H = 48, 40; scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | flag, W, H)
            if case == "cornell_depth16": kw["max_path_depth"] = 16
            if case == "direct_lighting": kw["integrator"] = A.INTEGRATOR_DIRECT_LIGHTING
        else:
            W, H = 64, 36; scene = api.mis_scene(W, H)
        p = api.make_params(W, H, 1024, tile_w=16, tile_h=8, **kw)
        g, c = api.render(scene, p), O.render(scene, p)
        fin = np.isfinite(c).all(axis=2)
        print("film", case, "%.3e" % rmse(g[fin], c[fin]), "nonfinite", int((~fin).sum()))
    # smoke
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 64, 64); params = api.make_params(64, 64, 32)
    print("smoke %.3e" % rmse(api.render(scene, params), O.render(scene, params)))
    # per-sample all light flags/strategies
    import test_parity_gpu as T
    for flag in ("area","direction","point","environment"):
        f = {"area": A.CB_LIGHT_AREA, "direction": A.CB_LIGHT_DIRECTION, "point": A.CB_LIGHT_POINT, "environment": A.CB_LIGHT_ENVIRONMENT}[flag]
        scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | f, 64, 64)
        for strat in T.STRATEGIES:
            params = api.make_params(64, 64, 128, direct_sample=strat)
            pixels = [(32, 32), (5, 5), (21, 42), (44, 45), (60, 61), (32, 4), (18, 50), (46, 52)]
            bad, tot, sg, sc = T.li_agreement(api, O, scene, params, pixels)
            print("li cornell", flag, strat, bad, tot, "%.2e" % (abs(sg-sc)/max(sc,1)))
    scene = api.mis_scene(96, 54)
    for depth in (5,16):
        for strat in T.STRATEGIES:
            params = api.make_params(96, 54, 128, direct_sample=strat, max_path_depth=depth)
            pixels = [(48, 27), (5, 5), (30, 40), (70, 30), (48, 50), (20, 20), (80, 45), (60, 8)]
            bad, tot, sg, sc = T.li_agreement(api, O, scene, params, pixels)
            print("li veach", depth, strat, bad, tot, "%.2e" % (abs(sg-sc)/max(sc,1)))
    # the noise estimate against the across-seed spread of the picture (tests/test_noise_gpu.py::test_it_measures_noise): three seed sets per sample count
    import test_noise_gpu as N
    conv = N._converging(A, api)
    for samples in (500, 112):
        print("noise ratio", samples, " ".join("%.4f" % N._ratio(A, api, conv["map%d" % samples], samples, seeds) for seeds in N.SEED_SETS))
# the lobes across material parameters (tests/test_materials_gpu.py): per material the 0.999 quantile and the maximum of the device's error against the oracle, for
# values / pdfs / the sampled direction, through kyhip_kat_bsdf ("grid"), kyhip_kat_bsdf_continue ("continue") and just above the Phong power's zero bound ("skip").
# The test's MEASURED tables are these quantiles; its bounds are 4 x them, floored.
if not ONLY or "materials" in ONLY:
    import test_materials_gpu as M
    x = M.inputs()
    fmt = lambda fig: "(" + ", ".join("%.1e" % q for q, _ in fig) + "),   # max (" + ", ".join("%.1e" % t for _, t in fig) + ")"
    for name in M.GRID:
        m, c = M.material(A, name), M.oracle_rows(A, O, name)
        g, k = api.kat_bsdf(m, x), api.kat_bsdf_continue(m, x, flat_phong=False)
        same = g[:, 7] == c[:, 7]
        print("grid     %-26s" % ('"%s":' % name), fmt([M.figures(e) for e in M.grid_errors(g, c)]), " flags differ on", int((~same).sum()))
        e = M.expected_continue(c, x)
        print("continue %-26s" % ('"%s":' % name), fmt([M.figures(e_) for e_ in M.continue_errors(k, e, same)]), " ok differs on", int((same & ((k[:, 6] != 0) != e["ok"])).sum()))
    for exponent in M.SKIP_EXPONENTS:
        m = M.make_material(A, A.MATERIAL_PLASTIC, M.DIFFUSE, M.SPECULAR, exponent=exponent)
        rows, waves = M.skip_rows(exponent)
        g, k, c = api.kat_bsdf(m, rows), api.kat_bsdf_continue(m, rows, flat_phong=False), O.kat_bsdf(m, rows)
        fig = [max(M.figures(a), M.figures(b)) for a, b in zip(M.skip_errors(g, c, waves), M.skip_errors(k, c, waves))]
        v = waves["vote"].start + 17
        print("skip     %-26s" % ("%g:" % exponent), fmt(fig), " the voting lane %.1e" % float(M.rel_err(g[v, 8:12], c[v, 8:12]).max()))
# sample_single_light's pick by power and by position (tests/test_light_pick_gpu.py): per scene and rule the largest |p - restatement| over the sixteen
# probabilities of 4096 rows, the rows that pick another light, and how many of those lie beyond P_TOL of an edge.  The test's P_TOL is 4 x the largest difference.
if not ONLY or "light_pick" in ONLY:
    import test_light_pick_gpu as P
    for which in ("veach", "cornell_lamp_point", "sixteen_lights", "general_shapes"):
        for rule in ("power", "spatial"):
            rng = np.random.default_rng(20240229)
            scene, _, rows = P.pick_rows(which, P.RULES[rule][0], A, api, O, rng)
            nl = P._light_count(scene)
            g, li, p, p16, margin = P.pick_agreement(P.RULES[rule][0], A, api, scene, rows)
            d = np.abs(g[:, 2:2 + nl].astype(np.float64) - p16)
            differ = g[:, 0].astype(np.int64) != li
            print("light_pick %-18s %-7s rows %d  max |p - restatement| %.3e (0.999 quantile %.3e)  index differs on %d, beyond P_TOL of an edge %d, largest margin among them %.3e"
                  % (which, rule, len(rows), d.max(), np.quantile(d.max(axis=1), 0.999), int(differ.sum()), int((differ & (margin > P.P_TOL)).sum()), float(margin[differ].max()) if differ.any() else 0.0))
# pixel filters (tests/test_filter.py; no GPU): how far the library's 256-interval inverse-CDF table strays from the analytic CDF (the test's DEVIATION), and the
# two quadratures of the centring test against each other -- the restatement's warp of a 16 x 16 grid of u through kyo_li_tape against the oracle's 16x-supersampled
# base-colour picture weighted by the analytic filter (the test's CENTRING; its bound is 2 x these) -- with the same for a warp centred on the pixel's corner
if not ONLY or "filter" in ONLY:
    import filter_restatement as F
    import test_filter as TF
    for case, _ in TF.DEVIATION:
        f, flt = TF.both(api, *case)
        print("filter table deviation", flt, "%.4e" % F.table_deviation(flt, api.filter_table(f)))
    O.load()
    base = TF.basecolor.__wrapped__(O, A, api) if hasattr(TF.basecolor, "__wrapped__") else None
    if base is not None:
        for kind, radius, param, _ in TF.CENTRING:
            flt = F.Filter(kind, radius, param)
            print("filter centring", flt, "rmse %.4e" % TF.centring_rmse(O, base, flt), "corner-centred %.4e" % TF.centring_rmse(O, base, flt, shift=-0.5))
# the lens's disk map (tests/test_lens_gpu.py; one GPU): the largest deviation of the device's lens_disk from the double restatement over the test's 2^16 pairs --
# the test's DISK_MEASURED, of which it allows four times and never more than 1e-5 -- and from the float32 restatement, whose quotient is correctly rounded
if not ONLY or "lens" in ONLY:
    import lens_restatement as L
    import test_lens_gpu as TL
    u = TL.disk_inputs()
    got = api.kat_lens(u).astype(np.float64)
    print("lens disk map: %d pairs, max |device - double restatement| %.4e, max |device - float32 restatement| %.4e, largest |point| - 1 %.3e"
          % (u.shape[0], np.abs(got - L.disk(u, np.float64)).max(), np.abs(got - L.disk(u, np.float32)).max(), float(np.hypot(got[:, 0], got[:, 1]).max() - 1)))
