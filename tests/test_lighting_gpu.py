"""GPU: light classes (kyhip_render_lighting / kyhip_kat_li_lighting, include/kyhip.h "Light classes") against the UNCHANGED oracle -- per camera sample a class is
a difference of the unmasked radiance at max_path_depth 0, 1 and D (tests/lighting_scenes.py) -- and against the library's own unmasked kernels.  The oracle-only
controls of these scenes and pixels are tests/test_lighting_controls.py.  Tolerances: tests/test_parity_gpu.py's for kat_li against O.li on the same scenes
(a sample differs beyond 1e-3 of max(1e-3, |c|); share 0.2 % on the Cornell scenes, 1.4 % on Veach) and its film bound, never wider.

Measured (MI355X): no sample differs on the Cornell scenes (0 of 1344 per integrator), 8 of 1344 (integrator 11) and 4 of 1344 (10) on Veach, all in the masks with the
indirect class; films 5e-8 (Cornell, lighting 3), 1.4e-3 (Veach, lighting 3 at 16 spp), lighting 4 on the controls' pixels 2e-6 / 5.5e-4; the partition: 0 of 192 everywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lighting_scenes as L
from helpers import rmse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def film_tolerance(spp):   # tests/test_parity_gpu.py
    return 1e-3 * max(1.0, np.sqrt(1024.0 / spp))


@pytest.fixture(scope="module")
def S(A, api):
    return L.scenes(A, api)


_terms = {}


def terms(A, O, S, name, p, x, y):
    key = (name, p.integrator, p.max_path_depth, p.direct_sample, x, y)
    if key not in _terms:
        _terms[key] = L.oracle_terms(A, O, S[name][0], p, x, y, L.N_SAMPLES)
    return _terms[key]


def per_sample_share(A, api, O, S, name, p, masks):
    scene, w, h, share = S[name]
    bad = tot = 0
    worst = {}
    for (x, y) in L.PIXELS[name]:
        l0, l1, lD = terms(A, O, S, name, p, x, y)
        for m in masks:
            g = api.kat_li_lighting(scene, p, m, x, y, 0, L.N_SAMPLES).astype(np.float64)
            b, t = L.differing(g, L.identity(m, l0, l1, lD))
            bad, tot = bad + b, tot + t
            worst[m] = worst.get(m, 0) + b
    print("%s integrator %d depth %d: %d of %d samples differ (allowed share %.3f); per mask %s" % (name, p.integrator, p.max_path_depth, bad, tot, share, worst))
    return bad, tot, share


SCENES = ["cornell", "veach", "default", "open"]   # "open": the default frame without its back wall, where a camera ray's miss is the emitter (tests/lighting_scenes.py)


@pytest.mark.parametrize("integrator", [11, 10, 6])
@pytest.mark.parametrize("name", SCENES)
def test_per_sample_against_the_oracle(name, integrator, A, api, O, S):
    p = L.params(api, A, name, S[name][1], S[name][2], integrator=integrator)
    bad, tot, share = per_sample_share(A, api, O, S, name, p, (1, 2, 3) if integrator == 6 else (1, 2, 3, 4, 5, 6, 7))
    assert tot > 0 and bad <= share * tot, (bad, tot)


def test_per_sample_at_depth_10_recursion_defered(A, api, O, S):
    p = L.params(api, A, "cornell", 48, 48, depth=10, integrator=10)
    bad, tot, share = per_sample_share(A, api, O, S, "cornell", p, (1, 2, 3, 4, 5, 6, 7))
    assert bad <= share * tot, (bad, tot)


@pytest.mark.parametrize("queue", [0, 1])
def test_veach_with_and_without_deferred_rays(queue, A, api, O, S):
    """kyhip_set_shadow_queue 0 / 1: the sphere lights' masked row with deferred rays, and the fact-free inline one"""
    lib = A.load_kyhip()
    scene, w, h, _ = S["veach"]
    p = L.params(api, A, "veach", w, h, spp=L.FILM_SPP)
    prev = lib.kyhip_set_shadow_queue(queue)
    try:
        ref = O.render(scene, L.at_depth(A, p, 1))
        g = api.render(scene, p, lighting=3)
        assert rmse(g, ref) < film_tolerance(L.FILM_SPP), rmse(g, ref)
        kernel = lib.kyhip_last_kernel(0)
        parts = sum(api.render(scene, p, lighting=m).astype(np.float64) for m in (1, 2, 4))   # (no pixel of this frame reaches the clamp in one class only: see below)
        full = api.render(scene, p).astype(np.float64)
        low = full.max(axis=2) < 0.999
        assert np.abs(parts - full)[low].max() < 1e-4, np.abs(parts - full)[low].max()
        assert (b"deferred shadow rays" in lib.kyhip_last_kernel(0)) == bool(queue), lib.kyhip_last_kernel(0)
        assert b"lighting 3: depth 1" in kernel, kernel
    finally:
        lib.kyhip_set_shadow_queue(prev)


@pytest.mark.parametrize("name", SCENES)
def test_films(name, A, api, O, S):
    scene, w, h, _ = S[name]
    p = L.params(api, A, name, w, h, spp=L.FILM_SPP)
    for mask, depth in ((3, 1), (1, 0)):
        g, c = api.render(scene, p, lighting=mask), O.render(scene, L.at_depth(A, p, depth))
        fin = np.isfinite(c).all(axis=2)
        e = rmse(g[fin], c[fin])
        print(name, "lighting", mask, "against the oracle at depth", depth, "RMSE", e)
        assert (~fin).sum() <= 2 and e < film_tolerance(L.FILM_SPP), (mask, e)
    g = api.render(scene, p, lighting=4)
    want = []
    for (x, y) in L.PIXELS[name]:
        l0, l1, lD = L.oracle_terms(A, O, scene, p, x, y, L.FILM_SPP)
        want.append(np.clip((lD - l1).mean(axis=0), 0, 1))
    got = np.array([g[y, x] for (x, y) in L.PIXELS[name]], np.float64)
    e = rmse(got, np.array(want))
    print(name, "lighting 4 on the controls' pixels: RMSE", e)
    assert e < film_tolerance(L.FILM_SPP), e


@pytest.mark.parametrize("case", ["48", "49", "4", "8", "debug"])
@pytest.mark.parametrize("name", SCENES)
def test_partition_on_the_gpu_alone(name, case, A, api, S):
    """emit + direct + indirect = the unmasked sample, per sample: the test of the stream position (a draw too few at the dropped estimate moves every later one)"""
    scene, w, h, share = S[name]
    kw = {"sampler": A.SAMPLER_DEBUG} if case == "debug" else {"direct_sample": int(case)}
    p = L.params(api, A, name, w, h, **kw)
    bad = tot = 0
    for (x, y) in L.PIXELS[name]:
        full = api.kat_li(scene, p, x, y, 0, L.N_SAMPLES).astype(np.float64)
        parts = sum(api.kat_li_lighting(scene, p, m, x, y, 0, L.N_SAMPLES).astype(np.float64) for m in (1, 2, 4))
        fin = np.isfinite(full).all(1)
        ok = np.all(np.abs(parts[fin] - full[fin]) <= 1e-6 + 2e-4 * np.abs(full[fin]), axis=1)   # helpers.explain_sample's value tolerance
        bad, tot = bad + int((~ok).sum()), tot + int(fin.sum())
    print(name, case, ": %d of %d samples off" % (bad, tot))
    assert tot > 0 and bad <= share * tot, (bad, tot)


@pytest.mark.parametrize("name", ["lamp", "cornell", "default", "open"])
def test_table_rows_partition_the_frame(name, A, api, O, S, table_kernels):
    """The compile-time rows (drop 1, 2, 3), which the per-sample entries never run, at film level: below the clamp a frame is the sum of its classes, lighting 5 is the
    frame without lighting 2, lighting 6 the frame without lighting 1; and lighting 2 against the oracle's depth 1 minus depth 0.  "lamp": configs[1]'s scene, whose
    masked rows carry all of its facts; "default" / "open": the environment light's full-facts rows; "cornell" (two lights): the fact-free rows."""
    lib = A.load_kyhip()
    if name == "lamp":
        scene, w, h = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 48, 48), 48, 48
    else:
        scene, w, h, _ = S[name]
    p = L.params(api, A, name, w, h, spp=L.FILM_SPP)
    f, kernel = {}, {}
    for m in (1, 2, 4, 5, 6, 7):
        f[m] = api.render(scene, p, lighting=m).astype(np.float64)
        kernel[m] = lib.kyhip_last_kernel(0)
    low = f[7].max(axis=2) < 0.999   # (classes are non-negative: below the frame's clamp none of them is clamped either)
    assert low.mean() > 0.5
    for what, a in (("1 + 2 + 4", f[1] + f[2] + f[4]), ("5 + 2", f[5] + f[2]), ("6 + 1", f[6] + f[1])):
        d = np.abs(a - f[7])[low].max()
        print(name, what, "against the frame: largest difference", d)
        assert d < 1e-4, (what, d)   # float sums of the same terms in another order; a term dropped or kept wrongly is 1e-2 and more on these frames
    assert f[2][low].max() > 0.05 and f[4][low].max() > 0.05
    if name in ("lamp", "cornell", "open"):
        assert f[1].max() > 0.05      # the camera sees an emitter: lighting 2, 4, 6 drop a non-zero term at the first vertex
        assert np.abs(f[6] - f[7]).max() > 0.05
    c1, c0 = O.render(scene, L.at_depth(A, p, 1)).astype(np.float64), O.render(scene, L.at_depth(A, p, 0)).astype(np.float64)
    fin = np.isfinite(c1).all(axis=2) & (c1.max(axis=2) < 0.999) & (c0.max(axis=2) < 0.999)   # below the oracle's own clamps the difference of its films is the class
    e = rmse(f[2][fin], (c1 - c0)[fin])
    print(name, "lighting 2 against the oracle's depth 1 - depth 0: RMSE", e)
    assert fin.mean() > 0.5 and e < film_tolerance(L.FILM_SPP), e
    if table_kernels:
        for m, drop in ((2, 1), (6, 1), (5, 2), (4, 3)):
            assert b"strategy 48" in kernel[m] and (b", drop %d>" % drop) in kernel[m], (m, kernel[m])
        facts = {"lamp": b"feat 3975", "default": b"feat 3728", "open": b"feat 3728", "cornell": b"feat 0"}[name]
        assert facts in kernel[4] and facts in kernel[5], (kernel[4], kernel[5])


def test_all_is_kyhip_render(A, api, S):
    lib = A.load_kyhip()
    for name in ("cornell", "veach"):
        scene, w, h, _ = S[name]
        p = L.params(api, A, name, w, h, spp=L.FILM_SPP)
        plain = api.render(scene, p)
        plain_kernel = lib.kyhip_last_kernel(0)
        for mask in (7, 31):
            assert np.array_equal(api.render(scene, p, lighting=mask), plain)
            assert lib.kyhip_last_kernel(0) == plain_kernel


@pytest.mark.parametrize("mask", [2, 4, 5])
def test_tiles_and_shards_are_bit_identical(mask, A, api, S):
    scene, w, h, _ = S["cornell"]
    base = api.render(scene, api.make_params(w, h, L.FILM_SPP, tile_w=16, tile_h=16), lighting=mask)
    assert base.max() > 0
    assert np.array_equal(api.render(scene, api.make_params(w, h, L.FILM_SPP, tile_w=32, tile_h=8), lighting=mask), base)
    acc = np.zeros_like(base)
    for r in range(3):
        api.render(scene, api.make_params(w, h, L.FILM_SPP, tile_w=16, tile_h=16, tile_first=r, tile_step=3), film=acc, lighting=mask)
    assert np.array_equal(acc, base)
    assert np.array_equal(api.render(scene, api.make_params(w, h, L.FILM_SPP), film=base.copy(), lighting=mask), base + base)   # it adds


def test_kernel_names_and_engine(A, api, S, table_kernels):
    lib = A.load_kyhip()
    scene, w, h, _ = S["cornell"]
    p = L.params(api, A, "cornell", w, h, spp=4)
    api.render(scene, p, lighting=4)
    name = lib.kyhip_last_kernel(0)
    assert name.endswith(b", lighting 4: emission at the first vertex and its direct light dropped"), name
    if table_kernels:
        assert b"drop 3" in name and b"strategy 48" in name, name
    api.render(scene, p, lighting=3)
    assert lib.kyhip_last_kernel(0).endswith(b", lighting 3: depth 1")
    api.render(scene, L.params(api, A, "cornell", w, h, spp=4, integrator=10), lighting=6)
    name = lib.kyhip_last_kernel(0)
    assert name.endswith(b", lighting 6: emission at the first vertex dropped"), name
    if table_kernels:
        assert b"drop bits per launch" in name, name
    prev = lib.kyhip_set_engine(1)
    try:
        lane = api.render(scene, p, lighting=5)
        assert b"lane engine: the queue engine has no masked form" in lib.kyhip_last_kernel(0) and b"render_kernel<" in lib.kyhip_last_kernel(0)
    finally:
        lib.kyhip_set_engine(prev)
    assert np.array_equal(api.render(scene, p, lighting=5), lane)


def test_nothing_selected_and_refusals_leave_the_film_alone(A, api, S):
    lib = A.load_kyhip()
    scene, w, h, _ = S["cornell"]
    film = np.full((h, w, 3), 0.25, np.float32)
    api.render(scene, L.params(api, A, "cornell", w, h, spp=4, depth=1), film=film, lighting=4)
    api.render(scene, L.params(api, A, "cornell", w, h, spp=4, integrator=6), film=film, lighting=4)
    assert np.all(film == 0.25)
    for p, mask in ((L.params(api, A, "cornell", w, h, spp=4), 0), (L.params(api, A, "cornell", w, h, spp=4), 8 | 1), (L.params(api, A, "cornell", w, h, spp=4), 32),
                    (L.params(api, A, "cornell", w, h, spp=4, integrator=9), 3), (L.params(api, A, "cornell", w, h, spp=4, integrator=1), 1)):
        with pytest.raises(api.KyError):
            api.render(scene, p, film=film, lighting=mask)
        with pytest.raises(api.KyError):
            api.kat_li_lighting(scene, p, mask, 3, 3, 0, 4)
    assert np.all(film == 0.25)


def test_a_run_time_instantiation_agrees_with_the_table(A, api, S, tmp_path, monkeypatch, no_boxes):
    monkeypatch.setenv("KYHIP_CACHE_DIR", str(tmp_path / "cache"))
    lib = A.load_kyhip()
    scene, w, h, _ = S["cornell"]
    p = L.params(api, A, "cornell", w, h, spp=L.FILM_SPP)
    prev = lib.kyhip_set_jit(0)
    try:
        table = api.render(scene, p, lighting=4)
        lib.kyhip_set_jit(1)
        own = api.render(scene, p, lighting=4)
        name = lib.kyhip_last_kernel(0)
        assert b"run-time instantiation" in name and b", 11, false, 3>" in name and b"lighting 4" in name, (name, lib.kyhip_jit_status())
        assert np.abs(own - table).max() < 2e-5 and table.max() > 0.1, float(np.abs(own - table).max())   # tests/test_jit.py's bound
    finally:
        lib.kyhip_set_jit(prev)


def test_driver_lighting_cells(A, api, tmp_path):
    """ky_drivers lighting_cells = the reference's render_lighting_enum (ky.cpp:4907-4935) made to work: emit, direct, indirect, all"""
    from oracle import film_writers as FW
    exe = os.path.join(ROOT, "examples", "bin", "ky_drivers")
    subprocess.check_call([exe, "lighting_cells", "8", "64"], cwd=tmp_path, stdout=subprocess.DEVNULL)
    got = open(tmp_path / "lighting_cells.bmp", "rb").read()
    assert got[:2] == b"BM" and len(got) == 54 + 3 * 64 * 4 * 64
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 64, 64)
    grid = np.zeros((64, 4 * 64, 3), np.float32)
    for cell, e in enumerate((1, 2, 4, 31)):
        api.render_host_api(scene, 10, 10, 48, A.SAMPLER_RANDOM, 8, 64, 64, grid=(1, 4), cell=cell, film=grid, lighting=e)
    assert got == FW.bmp_bytes(grid)
    cells = [grid[:, 64 * i:64 * (i + 1)].astype(np.float64) for i in range(4)]
    assert cells[0].max() > 0.5 and cells[1].max() > 0.1 and cells[2].max() > 0.05
    low = cells[3].max(axis=2) < 0.999   # below the clamp the classes add up to the beauty image (a clamped pixel's classes may sum to more)
    d = np.abs(cells[3] - (cells[0] + cells[1] + cells[2]))[low]
    assert low.mean() > 0.9 and d.max() < 1e-4, (low.mean(), d.max())
