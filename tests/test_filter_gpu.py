"""GPU: pixel filters by importance-sampling the camera sample (ky_pixel_filter).  The device's warp against the NumPy restatement
(tests/filter_restatement.py); the filtered kernels' samples and films against the CPU oracle fed the restatement's tape (kyo_li_tape adds a tape's first two
numbers to the pixel's corner whatever they are); the box filter and the debug sampler against the unfiltered render, bit for bit; every way of cutting a filtered
frame against the one-shot filtered render, bit for bit; the filter as part of a frame's identity; the screen cull's wider rectangle; one frame per filtered row
of the kernel table.  tests/test_filter.py holds the restatement itself against the analytic filters, centred on the pixel's centre."""
import ctypes as C

import numpy as np
import pytest

import filter_restatement as F
import test_stratified_gpu as T   # its scenes, film_tolerance, film_of and -- from its parametrisation -- the caps of the per-sample comparison
from helpers import rmse

pytestmark = pytest.mark.gpu

SAMPLERS = ("random", "stratified")
TENT2 = (F.TENT, 2.0, 0.0)
GAUSS = (F.GAUSSIAN, 1.5, 0.5)


@pytest.fixture(scope="module")
def lib(A):
    lib = A.load_kyhip()
    prev = lib.kyhip_set_jit(0)
    yield lib
    lib.kyhip_set_jit(prev)


def both(api, case):
    kind, radius, param = case
    return api.pixel_filter(kind, radius, param or None), F.Filter(kind, radius, param)


def sampler_kind(A, sampler):
    return A.SAMPLER_STRATIFIED if sampler == "stratified" else A.SAMPLER_RANDOM


def params_of(api, A, w, h, spp, sampler, **kw):
    kw.setdefault("max_path_depth", 5)
    kw.setdefault("direct_sample", A.DIRECT_BOTH_MIS)
    return api.make_params(w, h, spp, sampler=sampler_kind(A, sampler), **kw)


# ---- the warp ----

WARP_CASES = ((F.BOX, None, 0.0), (F.TENT, 0.5, 0.0), (F.TENT, 1.0, 0.0), (F.TENT, 2.0, 0.0), (F.TENT, 4.0, 0.0), (F.GAUSSIAN, 0.5, 0.5), (F.GAUSSIAN, 1.5, 0.5),
              (F.GAUSSIAN, 4.0, 1.0), (F.BLACKMAN_HARRIS, 0.5, 0.0), (F.BLACKMAN_HARRIS, 1.0, 0.0), (F.BLACKMAN_HARRIS, 2.0, 0.0),
              (F.BLACKMAN_HARRIS, 4.0, 0.0))


def warp_inputs():
    one = np.float32(1)
    half = np.float32(0.5)
    edge = np.array([0.0, 2.0 ** -24, np.nextafter(half, np.float32(0)), half, np.nextafter(half, one), 1 - 2.0 ** -24], np.float32)
    knots = np.arange(F.TABLE + 1, dtype=np.float32) / F.TABLE
    around = np.concatenate([knots, np.nextafter(knots, np.float32(-1)), np.nextafter(knots, np.float32(2))])
    around = around[(around >= 0) & (around < 1)]
    gen = np.random.default_rng(20261020)
    return np.concatenate([edge, around, gen.random((1 << 16) + 37, dtype=np.float32)])   # many workgroups and a ragged last one


@pytest.mark.parametrize("case", WARP_CASES, ids=str)
def test_warp_is_the_restatements(api, case):
    """|device - restatement| <= 2^-21 R: one ulp from v_sqrt_f32, one from the difference at worst cancellation near u = 0.5, one from the fma, with headroom;
    the table kinds have no square root and are usually exact."""
    f, flt = both(api, case)
    u = warp_inputs()
    got, want = api.kat_filter(f, u), F.warp(flt, u)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(flt, "%d numbers, largest error %.3g (bound %.3g), %d differ" % (u.size, err.max(), 2.0 ** -21 * flt.radius, int((err > 0).sum())))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert err.max() <= 2.0 ** -21 * flt.radius
    assert got.min() >= 0.5 - flt.radius and got.max() <= 0.5 + flt.radius


def test_warp_refuses_what_it_cannot_index(A, api):
    f = api.pixel_filter(A.FILTER_GAUSSIAN)
    for bad in (1.0, -0.25, float("nan")):
        with pytest.raises(api.KyError):
            api.kat_filter(f, np.array([0.25, bad], np.float32))
    with pytest.raises(api.KyError):
        api.kat_filter(A.PixelFilter(A.FILTER_TENT, 5.0, 0.0, 0), np.array([0.25], np.float32))


# ---- paths and films against the oracle on the restatement's tape ----

_oracle_cache = {}


def oracle_samples(O, A, api, scene, key, params, stride, sampler, flt):
    """[h, w, N, 3]: the oracle's radiance of every sample of every pixel on the restatement's filtered tape.  Computed once per case and shared."""
    if key not in _oracle_cache:
        h, w, n = params.height, params.width, params.samples_per_pixel
        tab = F.table(flt) if flt.kind in (F.GAUSSIAN, F.BLACKMAN_HARRIS) else None
        out = np.zeros((h, w, n, 3), np.float32)
        for y in range(h):
            for x in range(w):
                out[y, x], _ = O.li_tape(scene, params, x, y, F.tape(params.seed, y * w + x, n, stride, sampler_kind(A, sampler), flt, tab))
        out.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def shipped_case(O, A, api, name, w, h, n_spp, sampler, case):
    scene, params = T.scene_of(A, api, name, w, h), params_of(api, A, w, h, n_spp, sampler)
    f, flt = both(api, case)
    want = oracle_samples(O, A, api, scene, (name, w, h, n_spp, sampler, case), params, 256 if name == "veach" else 64, sampler, flt)
    return scene, params, f, want


def caps_of_the_stratified_comparison():
    """name -> (w, h, bad_share, sum_tol): the frames and caps tests/test_stratified_gpu.py's per-sample comparison is parametrised with, read from its marks."""
    for mark in T.test_paths_equal_the_oracle_on_the_restatements_numbers.pytestmark:
        if mark.name == "parametrize" and mark.args[0].startswith("name,"):
            return {row[0]: row[1:] for row in mark.args[1]}
    raise AssertionError("tests/test_stratified_gpu.py no longer parametrises its comparison by name")


CAPS = caps_of_the_stratified_comparison()


@pytest.mark.parametrize("case", (TENT2, GAUSS), ids=("tent2", "gaussian"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("name", ("cornell", "veach"))
def test_paths_equal_the_oracle_on_the_filtered_tape(O, A, api, lib, name, n_spp, sampler, case):
    """kyhip_kat_li_filtered against kyo_li_tape, every sample of every pixel: tests/test_stratified_gpu.py's comparison -- a sample differs if it is off by more
    than 1e-3 relative -- under its caps for these two frames (Cornell 32 x 32: 0.2 % of samples, sums to 1e-4; Veach 48 x 27: 1.4 %, 5e-3).  A filter moves
    camera rays, not what a path does at a vertex."""
    w, h, bad_share, sum_tol = CAPS[name]
    assert (name, w, h) in (("cornell", 32, 32), ("veach", 48, 27))
    scene, params, f, want = shipped_case(O, A, api, name, w, h, n_spp, sampler, case)
    bad = tot = 0
    sg = sc = 0.0
    for y in range(h):
        for x in range(w):
            g, c = api.kat_li(scene, params, x, y, 0, n_spp, filter=f), want[y, x]
            fin = np.isfinite(c).all(1)
            d = np.abs(g[fin] - c[fin]).max(axis=1)
            s = np.maximum(1e-3, np.abs(c[fin]).max(axis=1))
            bad += int((d / s > 1e-3).sum())
            tot += int(fin.sum())
            sg += float(np.minimum(g[fin], 10).sum())
            sc += float(np.minimum(c[fin], 10).sum())
    print("%s N = %d, %s, %s: %d of %d samples differ (cap %.0f), sums %.6g / %.6g" % (name, n_spp, sampler, case, bad, tot, bad_share * tot, sg, sc))
    assert bad <= bad_share * tot, (bad, tot)
    assert abs(sg - sc) <= sum_tol * max(sc, 1.0)


@pytest.mark.parametrize("case", (TENT2, GAUSS), ids=("tent2", "gaussian"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16, 17))
@pytest.mark.parametrize("size", (16, 32))
def test_film_is_the_mean_of_the_oracles_samples(O, A, api, lib, size, n_spp, sampler, case):
    scene, params, f, want = shipped_case(O, A, api, "cornell", size, size, n_spp, sampler, case)
    g, c = api.render(scene, params, filter=f), T.film_of(want)
    kernel = lib.kyhip_last_kernel(0).decode()
    assert "pixel filter" in kernel and "strategy -1" in kernel and "run-time instantiation" not in kernel, kernel
    fin = np.isfinite(c).all(axis=2)
    assert (~fin).sum() <= 2 and np.isfinite(g).all() and g.min() >= 0 and g.max() <= 1
    e = rmse(g[fin], c[fin])
    print("cornell %d x %d, N = %d, %s, %s: rmse %.3g, allowed %.3g" % (size, size, n_spp, sampler, case, e, T.film_tolerance(n_spp)))
    assert e < T.film_tolerance(n_spp)


# ---- the box, the debug sampler, the tent ----

def test_box_is_render_and_debug_ignores_the_filter(A, api, lib):
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 32, 32)
    tent = api.pixel_filter(A.FILTER_TENT, 2.0)
    for sampler in SAMPLERS:
        p = params_of(api, A, 32, 32, 16, sampler)
        plain = api.render(scene, p)
        plain_kernel = lib.kyhip_last_kernel(0)
        boxed = api.render(scene, p, filter=api.pixel_filter(A.FILTER_BOX))
        assert lib.kyhip_last_kernel(0) == plain_kernel and b"pixel filter" not in plain_kernel
        assert np.array_equal(boxed, plain)
        filtered = api.render(scene, p, filter=tent)
        name = lib.kyhip_last_kernel(0).decode()
        assert "pixel filter" in name and "tent filter, radius 2" in name, name
        assert not np.array_equal(filtered, plain) and filtered.max() > 0.1
        # a frame with the box filter set is the plain frame too
        with api.Frame(scene, p, filter=api.pixel_filter(A.FILTER_BOX)) as f:
            f.render(16)
            assert np.array_equal(f.resolve(), plain) and f.filter.kind == A.FILTER_BOX
    p = api.make_params(32, 32, 4, sampler=A.SAMPLER_DEBUG)
    plain = api.render(scene, p)
    plain_kernel = lib.kyhip_last_kernel(0)
    assert np.array_equal(api.render(scene, p, filter=tent), plain) and lib.kyhip_last_kernel(0) == plain_kernel
    with api.Frame(scene, p, filter=tent) as f:   # ... and as a frame: today's kernels
        f.render(4)
        assert np.array_equal(f.resolve(), plain) and b"debug sampler" in lib.kyhip_last_kernel(0) and b"pixel filter" not in lib.kyhip_last_kernel(0)
    assert np.array_equal(api.kat_li(scene, p, 7, 9, 0, 4, filter=tent), api.kat_li(scene, p, 7, 9, 0, 4))


def test_queue_engine_runs_the_lane_engine_and_says_so(A, api, lib):
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    p = params_of(api, A, 16, 16, 5, "random")
    tent = api.pixel_filter(A.FILTER_TENT, 2.0)
    want = api.render(scene, p, filter=tent)
    prev = lib.kyhip_set_engine(1)
    try:
        got = api.render(scene, p, filter=tent)
        name = lib.kyhip_last_kernel(0).decode()
    finally:
        lib.kyhip_set_engine(prev)
    assert np.array_equal(got, want) and "lane engine: the queue engine has no pixel filter" in name and "pixel filter" in name, name


# ---- cuts ----

@pytest.mark.parametrize("case", (TENT2, GAUSS), ids=("tent2", "gaussian"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("size", ((16, 16), (20, 13)), ids=("16x16", "20x13"))
def test_every_cut_of_a_filtered_frame_is_the_one_shot_film(A, api, lib, size, sampler, case):
    """N = 17 (pass boundaries at 4 and 12) at 16 x 16 and at 20 x 13, which is no multiple of the 16 x 16 tile nor of the 8 x 8 block."""
    w, h = size
    n_spp = 17
    scene, p = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), params_of(api, A, w, h, n_spp, sampler)
    f_ = both(api, case)[0]
    whole = api.render(scene, p, filter=f_)
    assert whole.max() > 0.1 and not np.array_equal(whole, api.render(scene, p))
    bounds = api.pass_boundaries(n_spp)

    def in_passes(**kw):
        with api.Frame(scene, p, filter=f_, **kw) as f:
            live = f.block_stats().live if kw.get("blocks") else 0
            for want in (4, 8, n_spp):
                if f.done < f.total:
                    f.render(want)
            assert f.done == n_spp
            if kw.get("blocks"):
                assert b"listed blocks" in lib.kyhip_last_kernel(0) and b"pixel filter" in lib.kyhip_last_kernel(0), lib.kyhip_last_kernel(0)
                assert f.block_stats().live == live > 0   # every block kept
            return f.resolve()

    assert np.array_equal(in_passes(), whole)                     # passes
    assert np.array_equal(in_passes(noise=True), whole)           # ... while tracking noise
    assert np.array_equal(in_passes(blocks=True), whole)          # ... while tracking blocks, every block kept (the listed rows)
    with api.Frame(scene, p, filter=f_) as f:                     # saved and loaded mid-frame
        f.render(1)
        state = f.save()
    with api.Frame(scene, p, filter=f_) as f:
        f.load(state)
        assert f.done == bounds[0]
        f.render(n_spp)
        assert np.array_equal(f.resolve(), whole)
    for n_slices in (2, 3):                                       # slices merged in both orders
        sb = api.slice_bounds(n_spp, n_slices)
        for order in (list(range(n_slices)), list(range(n_slices))[::-1]):
            frames = [api.Frame(scene, p, filter=f_, slice=(sb[k], sb[k + 1])) for k in range(n_slices)]
            try:
                for f in frames:
                    f.render(n_spp)
                with api.Frame(scene, p, filter=f_, slice=(0, 0)) as collector:
                    for k in order:
                        collector.merge(frames[k])
                    assert collector.done == n_spp and np.array_equal(collector.resolve(), whole), (n_slices, order)
                if n_slices == 2:   # ... and into a slice itself, from a saved state
                    frames[order[0]].merge(frames[order[1]].save())
                    assert np.array_equal(frames[order[0]].resolve(), whole)
            finally:
                for f in frames:
                    f.close()
    assert np.array_equal(api.render_sliced(scene, p, [0, 0], 4, filter=f_), whole)


def test_the_host_mirror_reads_the_filter_from_the_film(A, api, lib):
    """film_t::set_filter (ky.hpp) through render, render_passes, render_sliced and render_until: api.render(filter=)'s film, bit for bit."""
    w, h, n_spp = 20, 13, 17
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    for sampler in SAMPLERS:
        p = params_of(api, A, w, h, n_spp, sampler)
        for f_ in (api.pixel_filter(A.FILTER_TENT, 2.0), api.pixel_filter(A.FILTER_BLACKMAN_HARRIS, 1.0)):
            whole = api.render(scene, p, filter=f_)
            for mode in ("render", "passes", "sliced", "until"):
                got = api.render_filtered_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, p.sampler, n_spp, w, h, f_, mode=mode)
                assert np.array_equal(got, whole), (sampler, f_.kind, mode)
        plain = api.render(scene, p)
        assert np.array_equal(api.render_filtered_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, p.sampler, n_spp, w, h,
                                                           api.pixel_filter(A.FILTER_BOX)), plain)
    with pytest.raises(api.KyError):   # film_t::set_filter refuses what kyhip_filter_check refuses
        api.render_filtered_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, 4, w, h, A.PixelFilter(A.FILTER_TENT, 9.0, 0.0, 0))


# ---- identity ----

def test_the_filter_is_part_of_a_frames_identity(A, api, lib):
    scene, p = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16), params_of(api, A, 16, 16, 17, "random")
    filters = {"plain": None, "tent2": api.pixel_filter(A.FILTER_TENT, 2.0), "tent1": api.pixel_filter(A.FILTER_TENT, 1.0), "gaussian": api.pixel_filter(A.FILTER_GAUSSIAN)}
    sb = api.slice_bounds(17, 2)
    states, slices = {}, {}
    for name, flt in filters.items():
        with api.Frame(scene, p, filter=flt) as f:
            f.render(1)
            states[name] = f.save()
        with api.Frame(scene, p, filter=flt, slice=(sb[1], sb[2])) as f:
            f.render(17)
            slices[name] = f.save()
    assert len({len(s) for s in states.values()}) == 1 and len({len(s) for s in slices.values()}) == 1   # the checkpoint's layout and size do not change
    for mine, flt in filters.items():
        for theirs in filters:
            with api.Frame(scene, p, filter=flt) as f, api.Frame(scene, p, filter=flt, slice=(sb[0], sb[1])) as g, \
                    api.Frame(scene, p, filter=filters[theirs], slice=(sb[1], sb[2])) as other:
                other.render(17)
                if mine == theirs:
                    f.load(states[theirs])
                    g.merge(slices[theirs])
                    continue
                for attempt in (lambda: f.load(states[theirs]), lambda: g.merge(slices[theirs]), lambda: g.merge(other)):
                    with pytest.raises(api.KyError) as e:
                        attempt()
                    assert "filter" in str(e.value), (mine, theirs, str(e.value))
                assert f.done == 0 and g.done == 0
    # the refusal names this frame's filter where it has one
    with api.Frame(scene, p, filter=filters["gaussian"]) as f:
        with pytest.raises(api.KyError) as e:
            f.load(states["plain"])
        assert "box filter" in str(e.value) and "Gaussian filter, radius 1.5, sigma 0.5" in str(e.value)
    # set_filter after the first pass, after a load and after a merge
    with api.Frame(scene, p) as f:
        f.set_filter(filters["tent1"])
        f.set_filter(filters["tent2"])
        got = f.filter
        assert (got.kind, got.radius) == (A.FILTER_TENT, 2.0)
        f.render(1)
        with pytest.raises(api.KyError):
            f.set_filter(filters["tent2"])
        with pytest.raises(api.KyError):
            f.set_filter(api.pixel_filter(A.FILTER_BOX))
    with api.Frame(scene, p) as f:
        f.load(states["plain"])
        with pytest.raises(api.KyError):
            f.set_filter(filters["tent2"])
    with api.Frame(scene, p, slice=(sb[0], sb[1])) as g:
        g.merge(slices["plain"])
        with pytest.raises(api.KyError):
            g.set_filter(filters["tent2"])


# ---- the screen cull ----

def test_the_cull_reads_a_wider_rectangle_under_a_filter(A, api, lib):
    """The Cornell box at 96 x 72 (tests/test_screen_cull_gpu.py's frame): the plain live rectangle begins at x = 8, so the frame's first column of 8 x 8 blocks
    is dead for the box filter -- and under a tent of radius 4, whose offsets reach 3.5 pixels to the left of a pixel's corner, the pixels just left of x = 8 see
    the box.  The film is the same with the cull on and off; the filtered rectangle is the plain one grown by 4 and clamped; and with the base-colour integrator
    a pixel outside the plain rectangle is not black.  An implementation that forgets the widening skips that block with the cull on and fails the first
    assertion: confirmed by building a scratch copy of the library without the `if constexpr (FILTER)` line of the work decoder (ky_render.hpp), not in the tree."""
    from test_screen_cull_gpu import on_and_off
    w, h = 96, 72
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    tent4 = api.pixel_filter(A.FILTER_TENT, 4.0)
    p = params_of(api, A, w, h, 16, "random", integrator=A.INTEGRATOR_BASECOLOR)
    (x0, y0, x1, y1), dead, total = api.scene_screen_bound(scene, p)
    assert x0 == 8 and dead >= 9
    rect, dead_f, total_f = api.scene_screen_bound(scene, p, filter=tent4)
    assert rect == (max(x0 - 4, 0), max(y0 - 4, 0), min(x1 + 4, w), min(y1 + 4, h)) and total_f == total and dead_f < dead
    for params in (p, params_of(api, A, w, h, 16, "stratified", integrator=A.INTEGRATOR_BASECOLOR), params_of(api, A, w, h, 16, "random")):
        on, off = on_and_off(lib, lambda: api.render(scene, params, filter=tent4))
        assert b"pixel filter" in lib.kyhip_last_kernel(0)
        assert np.array_equal(on, off)
        assert on[:, :x0].any(), "no pixel left of the plain rectangle saw the box"
        assert not on[:, :rect[0]].any() and not on[:, rect[2]:].any()
    with api.Frame(scene, p, filter=tent4, blocks=True) as f:   # the listed rows read the same rectangle
        f.render(16)
        assert np.array_equal(f.resolve(), on_and_off(lib, lambda: api.render(scene, p, filter=tent4))[1])


# ---- one frame per filtered row ----

@pytest.mark.parametrize("listed", (False, True), ids=("plain", "listed"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("which", ("general", "large"))
def test_one_frame_per_filtered_row(O, A, api, lib, which, sampler, listed):
    """A scene with general quads, triangles and disks, and the Cornell box with 65 more balls (more than 64 surfaces), at 16 x 16, N = 4, under the tent of
    radius 2: the film is the mean of the oracle's samples on the filtered tape, and kyhip_last_kernel names the general, the large and the listed filtered rows."""
    w = h = 16
    n_spp = 4
    scene = T.general_scene(A, api) if which == "general" else T.large_scene(A, api, w, h)
    params = params_of(api, A, w, h, n_spp, sampler, direct_sample=A.DIRECT_LIGHT_MIS if which == "general" else A.DIRECT_BOTH_MIS)
    f_, flt = both(api, TENT2)
    with api.Frame(scene, params, filter=f_, blocks=listed) as f:
        f.render(n_spp)
        g = f.resolve()
    kernel = lib.kyhip_last_kernel(0).decode()
    print(which, sampler, listed, "->", kernel)
    assert "pixel filter" in kernel and "general shapes" in kernel and "strategy -1" in kernel and "run-time instantiation" not in kernel, kernel
    assert ("scene-sized LDS block" in kernel) == (which == "large") and ("listed blocks" in kernel) == listed and ("stratified sampler" in kernel) == (sampler == "stratified"), kernel
    if not listed:
        assert np.array_equal(api.render(scene, params, filter=f_), g)
    want = oracle_samples(O, A, api, scene, (which, sampler), params, 128, sampler, flt)
    c = T.film_of(want)
    fin = np.isfinite(c).all(axis=2)
    e = rmse(g[fin], c[fin])
    print("%s: rmse %.3g, allowed %.3g" % (which, e, T.film_tolerance(n_spp)))
    assert g.max() > 0 and (~fin).sum() <= 2 and e < T.film_tolerance(n_spp)


def test_refusals_before_any_device_work(A, api, lib):
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    p = params_of(api, A, 16, 16, 4, "random")
    film = np.zeros((16, 16, 3), np.float32)
    bad = A.PixelFilter(A.FILTER_GAUSSIAN, 1.5, 0.0, 0)
    assert lib.kyhip_render_filtered(0, api._scene_ptr(scene), C.byref(p), C.byref(bad), film.ctypes.data_as(C.c_void_p), 16) == A.KY_ERR_INVALID_VALUE
    assert b"sigma" in lib.kyhip_last_error() and film.max() == 0
    with pytest.raises(api.KyError):
        api.kat_li(scene, p, 3, 3, 0, 4, filter=bad)
    with pytest.raises(ValueError):
        api.render(scene, p, filter=api.pixel_filter(A.FILTER_TENT), lighting=A.LIGHTING_DIRECT)
    with api.Frame(scene, p) as f:
        with pytest.raises(api.KyError):
            f.set_filter(bad)
        assert f.filter.kind == A.FILTER_BOX
    sp = params_of(api, A, 16, 16, 5, "stratified")
    with pytest.raises(api.KyError):
        api.kat_li(scene, sp, 3, 3, 0, 6, filter=api.pixel_filter(A.FILTER_TENT))   # sample 5 of 5: the stratified sampler's own refusal
