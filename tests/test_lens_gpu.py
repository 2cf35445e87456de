"""GPU: the thin lens (ky_lens).  The device's disk map against the NumPy restatement (tests/lens_restatement.py); the lens kernels' samples and
films against the CPU oracle, which is a pinhole camera: called once per sample with the camera at that sample's lens point and a tape whose first two numbers are
the shifted film point (kyo_li_tape adds them to the pixel's corner whatever they are); the pinhole and the debug sampler against today's render, bit for bit; every
way of cutting a lens frame against the one-shot lens render, bit for bit; the lens as part of a frame's identity; the screen cull, which a lens launch must not
apply; one frame per lens row of the kernel table; the host mirror.  tests/test_lens.py holds the restatement and the geometry without a device."""
import ctypes as C

import numpy as np
import pytest

import filter_restatement as F
import lens_restatement as L
import test_filter_gpu as TF       # both(), params_of(), sampler_kind(), CAPS: the per-sample comparison's frames and caps, read from tests/test_stratified_gpu.py's marks
import test_stratified_gpu as T   # scene_of, film_tolerance, film_of, general_scene, large_scene
from helpers import rmse

pytestmark = pytest.mark.gpu

SAMPLERS = TF.SAMPLERS
TENT2 = TF.TENT2
GAUSS = TF.GAUSS
# the largest |device - double restatement| of the disk map over test_the_disk_map_is_the_restatements's 2^16 pairs, measured on an MI355X
# (tools/measure_tolerances.py lens); the test allows four times that and never more than CEILING
DISK_MEASURED = 1.116e-7
DISK_CEILING = 1e-5


@pytest.fixture(scope="module")
def lib(A):
    lib = A.load_kyhip()
    prev = lib.kyhip_set_jit(0)
    yield lib
    lib.kyhip_set_jit(prev)


# ---- the disk map ----

def disk_inputs():
    one = np.float32(1) - np.float32(2.0 ** -24)
    edge = np.array([[0.5, 0.5], [0, 0], [0, one], [one, 0], [one, one], [0, 0.5], [0.5, 0], [one, 0.5], [0.5, one], [0.25, 0.25], [0.75, 0.25], [0.25, 0.75]], np.float32)
    half = np.float32(0.5)
    near = np.array([[np.nextafter(half, np.float32(1)), half], [half, np.nextafter(half, np.float32(0))], [np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1))]], np.float32)
    gen = np.random.default_rng(20261021)
    rnd = gen.random(((1 << 16) - edge.shape[0] - near.shape[0], 2), dtype=np.float32)
    return np.concatenate([edge, near, rnd])   # 2^16 pairs


def test_the_disk_map_is_the_restatements(api):
    u = disk_inputs()
    assert u.shape == (1 << 16, 2)
    got = api.kat_lens(u)
    want64, want32 = L.disk(u, np.float64), L.disk(u, np.float32)
    err = np.abs(got.astype(np.float64) - want64).max()
    print("disk map: %d pairs, largest |device - double restatement| %.4g (bound %.4g = 4 x %.4g measured, ceiling %.0e); against the float32 restatement %.4g, %d of %d values differ"
          % (u.shape[0], err, 4 * DISK_MEASURED, DISK_MEASURED, DISK_CEILING, np.abs(got.astype(np.float64) - want32).max(), int((got != want32).sum()), got.size))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert 4 * DISK_MEASURED <= DISK_CEILING
    assert err <= 4 * DISK_MEASURED
    assert np.array_equal(got[0], [0, 0])
    assert (np.hypot(got[:, 0].astype(np.float64), got[:, 1].astype(np.float64)) <= 1 + 4 * DISK_MEASURED).all()
    for bad in (1.0, -0.25, float("nan")):
        with pytest.raises(api.KyError):
            api.kat_lens(np.array([[0.25, bad]], np.float32))


# ---- paths and films against the oracle, a pinhole at every sample's lens point ----

_lens_cache = {}
_oracle_cache = {}


def lens_of(O, A, api, name, w, h):
    """(ky_lens, radius, focus): Cornell -- radius 2 % of the scene's diagonal, focused on the front ball; Veach -- likewise, focused on the middle plate."""
    key = (name, w, h)
    if key not in _lens_cache:
        scene = T.scene_of(A, api, name, w, h)
        radius = 0.02 * 2 * float(O.world_bounding_sphere(scene)[3])
        focus = focus_on(O, A, api, scene, name, w, h)
        _lens_cache[key] = (api.lens(radius, focus), radius, focus)
    return _lens_cache[key]


def focus_on(O, A, api, scene, name, w, h):
    """api.focus_distance at the pixel that shows the front ball (Cornell: the sphere hit nearest the camera) or the middle plate (Veach: in the frame's centre
    column, the hit of median distance among the column's hits on rectangles), found with the oracle's scene intersection."""
    cam = L.Camera(scene.flat.contents.camera)
    px = np.stack(np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5), axis=-1).reshape(-1, 2).astype(np.float32)
    rays = O.kat_camera(scene.flat.contents.camera, px)
    hits = O.kat_scene_intersect(scene, np.concatenate([rays, np.full((rays.shape[0], 1), np.inf, np.float32)], axis=1))
    kinds = np.array([scene.c.shapes[scene.c.surfaces[int(s)].shape].kind if hit else -1 for hit, s in zip(hits[:, 0], hits[:, 8])])
    if name == "cornell":
        on = np.where((kinds == A.SHAPE_SPHERE) & (hits[:, 0] != 0))[0]
        i = on[np.argmin(hits[on, 1])]
    else:
        col = np.where((np.abs(px[:, 0] - (w // 2 + 0.5)) < 0.25) & (hits[:, 0] != 0) & (kinds == A.SHAPE_RECTANGLE))[0]
        i = col[np.argsort(hits[col, 1])[len(col) // 2]]
    x, y = int(px[i, 0]), int(px[i, 1])
    d = api.focus_distance(scene, x, y)
    want = float((hits[i, 2:5].astype(np.float64) - cam.position.astype(np.float64)) @ cam.front.astype(np.float64))
    assert abs(d - want) <= 1e-4 * want, (d, want)   # the device's scene intersection and the oracle's see the same surface at that pixel
    return d


def oracle_pixels(O, A, api, scene, params, stride, sampler, flt, radius, focus, pixels):
    """{(x, y): [N, 3]}: the oracle's radiance of every lens sample of the listed pixels"""
    cam = L.Camera(scene.flat.contents.camera)
    lc = L.lens_const(cam, radius, focus)
    tab = F.table(flt) if flt is not None and flt.kind in (F.GAUSSIAN, F.BLACKMAN_HARRIS) else None
    orc = L.OracleLens(O, A, scene, params)
    out = {}
    for x, y in pixels:
        rows, origins = L.sample_rows(cam, lc, params.seed, y * params.width + x, x, y, params.samples_per_pixel, stride, TF.sampler_kind(A, sampler), flt, tab)
        out[(x, y)] = orc.pixel(x, y, rows, origins)
    return out


def oracle_samples(O, A, api, scene, key, params, stride, sampler, flt, radius, focus):
    """[h, w, N, 3]: ... of every pixel.  Computed once per case and shared."""
    if key not in _oracle_cache:
        h, w, n = params.height, params.width, params.samples_per_pixel
        got = oracle_pixels(O, A, api, scene, params, stride, sampler, flt, radius, focus, [(x, y) for y in range(h) for x in range(w)])
        out = np.zeros((h, w, n, 3), np.float32)
        for (x, y), v in got.items():
            out[y, x] = v
        out.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def shipped_case(O, A, api, name, w, h, n_spp, sampler, case):
    scene, params = T.scene_of(A, api, name, w, h), TF.params_of(api, A, w, h, n_spp, sampler)
    f, flt = TF.both(api, case) if case is not None else (None, None)
    lens, radius, focus = lens_of(O, A, api, name, w, h)
    want = oracle_samples(O, A, api, scene, (name, w, h, n_spp, sampler, case), params, 256 if name == "veach" else 64, sampler, flt, radius, focus)
    return scene, params, f, lens, want


@pytest.mark.parametrize("case", (None, TENT2), ids=("lens", "lens+tent2"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("name", ("cornell", "veach"))
def test_paths_equal_the_oracle_at_the_lens_point(O, A, api, lib, name, n_spp, sampler, case):
    """kyhip_kat_li_lens against kyo_li_tape, every sample of every pixel: tests/test_stratified_gpu.py's comparison -- a sample differs if it is off by more than
    1e-3 relative -- under its caps for these two frames (Cornell 32 x 32: 0.2 % of samples, sums to 1e-4; Veach 48 x 27: 1.4 %, 5e-3).  A lens moves a camera
    ray's origin and direction, not what a path does at a vertex; a ray formed otherwise than section 12 says moves every sample."""
    w, h, bad_share, sum_tol = TF.CAPS[name]
    assert (name, w, h) in (("cornell", 32, 32), ("veach", 48, 27))
    scene, params, f, lens, want = shipped_case(O, A, api, name, w, h, n_spp, sampler, case)
    bad = tot = 0
    sg = sc = 0.0
    for y in range(h):
        for x in range(w):
            g, c = api.kat_li(scene, params, x, y, 0, n_spp, filter=f, lens=lens), want[y, x]
            fin = np.isfinite(c).all(1)
            d = np.abs(g[fin] - c[fin]).max(axis=1)
            s = np.maximum(1e-3, np.abs(c[fin]).max(axis=1))
            bad += int((d / s > 1e-3).sum())
            tot += int(fin.sum())
            sg += float(np.minimum(g[fin], 10).sum())
            sc += float(np.minimum(c[fin], 10).sum())
    print("%s N = %d, %s, %s, lens radius %.4g focus %.4g: %d of %d samples differ (cap %.0f), sums %.6g / %.6g"
          % (name, n_spp, sampler, case, lens.radius, lens.focus_distance, bad, tot, bad_share * tot, sg, sc))
    assert bad <= bad_share * tot, (bad, tot)
    assert abs(sg - sc) <= sum_tol * max(sc, 1.0)


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("n_spp", (5, 16, 17))
@pytest.mark.parametrize("size", (16, 32))
def test_film_is_the_mean_of_the_oracles_samples(O, A, api, lib, size, n_spp, sampler):
    scene, params, _, lens, want = shipped_case(O, A, api, "cornell", size, size, n_spp, sampler, None)
    g, c = api.render(scene, params, lens=lens), T.film_of(want)
    kernel = lib.kyhip_last_kernel(0).decode()
    assert ", lens>" in kernel and "lens radius" in kernel and "strategy -1" in kernel and "run-time instantiation" not in kernel, kernel
    fin = np.isfinite(c).all(axis=2)
    assert (~fin).sum() <= 2 and np.isfinite(g).all() and g.min() >= 0 and g.max() <= 1
    e = rmse(g[fin], c[fin])
    print("cornell %d x %d, N = %d, %s: rmse %.3g, allowed %.3g" % (size, size, n_spp, sampler, e, T.film_tolerance(n_spp)))
    assert e < T.film_tolerance(n_spp)


# ---- the pinhole, the debug sampler ----

def test_the_pinhole_is_render_and_debug_ignores_the_lens(O, A, api, lib):
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 32, 32)
    lens = lens_of(O, A, api, "cornell", 32, 32)[0]
    tent = api.pixel_filter(A.FILTER_TENT, 2.0)
    film = np.zeros((32, 32, 3), np.float32)
    for sampler in SAMPLERS:
        p = TF.params_of(api, A, 32, 32, 16, sampler)
        for flt in (None, tent):
            plain = api.render(scene, p, filter=flt)
            plain_kernel = lib.kyhip_last_kernel(0)
            for pinhole in (api.lens(0.0, 0.0), api.lens(0.0, 3.0)):
                assert np.array_equal(api.render(scene, p, filter=flt, lens=pinhole), plain)
                assert lib.kyhip_last_kernel(0) == plain_kernel and b"lens" not in plain_kernel
            film[:] = 0   # ... and a NULL lens
            assert lib.kyhip_render_lens(0, api._scene_ptr(scene), C.byref(p), C.byref(flt) if flt is not None else None, None, film.ctypes.data_as(C.c_void_p), 32) == A.KY_OK
            assert np.array_equal(film, plain) and lib.kyhip_last_kernel(0) == plain_kernel
            blurred = api.render(scene, p, filter=flt, lens=lens)
            name = lib.kyhip_last_kernel(0).decode()
            assert ", lens>" in name and "lens radius" in name and ("tent filter, radius 2" if flt is not None else "box filter") in name, name
            assert not np.array_equal(blurred, plain) and blurred.max() > 0.1
            with api.Frame(scene, p, filter=flt, lens=api.lens(0.0, 1.0)) as f:   # a frame with the pinhole set is the plain frame too
                f.render(16)
                assert np.array_equal(f.resolve(), plain) and f.lens.radius == 0 and f.lens.focus_distance == 0
        assert np.array_equal(api.kat_li(scene, p, 7, 9, 0, 16, lens=api.lens(0.0, 0.0)), api.kat_li(scene, p, 7, 9, 0, 16))
    p = api.make_params(32, 32, 4, sampler=A.SAMPLER_DEBUG)
    plain = api.render(scene, p)
    plain_kernel = lib.kyhip_last_kernel(0)
    assert np.array_equal(api.render(scene, p, lens=lens), plain) and lib.kyhip_last_kernel(0) == plain_kernel
    assert np.array_equal(api.render(scene, p, lens=lens, filter=tent), plain) and lib.kyhip_last_kernel(0) == plain_kernel
    with api.Frame(scene, p, lens=lens) as f:   # ... and as a frame: today's kernels
        f.render(4)
        assert np.array_equal(f.resolve(), plain) and b"debug sampler" in lib.kyhip_last_kernel(0) and b"lens" not in lib.kyhip_last_kernel(0)
    assert np.array_equal(api.kat_li(scene, p, 7, 9, 0, 4, lens=lens), api.kat_li(scene, p, 7, 9, 0, 4))


def test_queue_engine_runs_the_lane_engine_and_says_so(O, A, api, lib):
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    p = TF.params_of(api, A, 16, 16, 5, "random")
    lens = lens_of(O, A, api, "cornell", 16, 16)[0]
    want = api.render(scene, p, lens=lens)
    prev = lib.kyhip_set_engine(1)
    try:
        got = api.render(scene, p, lens=lens)
        name = lib.kyhip_last_kernel(0).decode()
    finally:
        lib.kyhip_set_engine(prev)
    assert np.array_equal(got, want) and "lane engine: the queue engine has no lens" in name and ", lens>" in name and "lens radius" in name, name


# ---- cuts ----

@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("size", ((16, 16), (40, 24)), ids=("16x16", "40x24"))
def test_every_cut_of_a_lens_frame_is_the_one_shot_film(O, A, api, lib, size, sampler):
    """Lens + Gaussian, N = 17 (pass boundaries at 4 and 12), at 16 x 16 and at 40 x 24 (ragged 16 x 16 tiles)."""
    w, h = size
    n_spp = 17
    scene, p = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), TF.params_of(api, A, w, h, n_spp, sampler)
    f_ = TF.both(api, GAUSS)[0]
    lens = lens_of(O, A, api, "cornell", w, h)[0]
    whole = api.render(scene, p, filter=f_, lens=lens)
    assert whole.max() > 0.1 and not np.array_equal(whole, api.render(scene, p, filter=f_))
    bounds = api.pass_boundaries(n_spp)

    def in_passes(wants, **kw):
        with api.Frame(scene, p, filter=f_, lens=lens, **kw) as f:
            live = f.block_stats().live if kw.get("blocks") else 0
            for want in wants:
                if f.done < f.total:
                    f.render(want)
            assert f.done == n_spp
            if kw.get("blocks"):
                assert b"listed blocks" in lib.kyhip_last_kernel(0) and b", lens>" in lib.kyhip_last_kernel(0), lib.kyhip_last_kernel(0)
                assert f.block_stats().live == live > 0   # nothing retired
            return f.resolve()

    assert np.array_equal(in_passes((4, 8, n_spp)), whole)                 # passes of unequal length
    assert np.array_equal(in_passes((1, n_spp)), whole)
    assert np.array_equal(in_passes((4, 8, n_spp), noise=True), whole)     # ... while tracking noise
    assert np.array_equal(in_passes((4, 8, n_spp), blocks=True), whole)    # ... while tracking blocks, nothing retired (the listed rows)
    with api.Frame(scene, p, filter=f_, lens=lens) as f:                   # saved and resumed mid-frame
        f.render(1)
        state = f.save()
    with api.Frame(scene, p, filter=f_, lens=lens) as f:
        f.load(state)
        assert f.done == bounds[0]
        f.render(n_spp)
        assert np.array_equal(f.resolve(), whole)
    sb = api.slice_bounds(n_spp, 2)                                        # two slices merged in either order
    for order in ((0, 1), (1, 0)):
        frames = [api.Frame(scene, p, filter=f_, lens=lens, slice=(sb[k], sb[k + 1])) for k in range(2)]
        try:
            for f in frames:
                f.render(n_spp)
            with api.Frame(scene, p, filter=f_, lens=lens, slice=(0, 0)) as collector:
                for k in order:
                    collector.merge(frames[k])
                assert collector.done == n_spp and np.array_equal(collector.resolve(), whole), order
            frames[order[0]].merge(frames[order[1]].save())   # ... and into a slice itself, from a saved state
            assert np.array_equal(frames[order[0]].resolve(), whole)
        finally:
            for f in frames:
                f.close()
    assert np.array_equal(api.render_sliced(scene, p, [0, 0], 4, filter=f_, lens=lens), whole)


# ---- identity ----

def test_the_lens_is_part_of_a_frames_identity(A, api, lib):
    scene, p = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16), TF.params_of(api, A, 16, 16, 17, "random")
    lenses = {"pinhole": None, "lens": api.lens(0.05, 2.0), "wider": api.lens(0.06, 2.0), "nearer": api.lens(0.05, 1.5)}
    sb = api.slice_bounds(17, 2)
    states, slices = {}, {}
    for name, lens in lenses.items():
        with api.Frame(scene, p, lens=lens) as f:
            f.render(1)
            states[name] = f.save()
        with api.Frame(scene, p, lens=lens, slice=(sb[1], sb[2])) as f:
            f.render(17)
            slices[name] = f.save()
    assert len({len(s) for s in states.values()}) == 1 and len({len(s) for s in slices.values()}) == 1   # the checkpoint's layout and size do not change
    for mine, lens in lenses.items():
        for theirs in lenses:
            with api.Frame(scene, p, lens=lens) as f, api.Frame(scene, p, lens=lens, slice=(sb[0], sb[1])) as g, \
                    api.Frame(scene, p, lens=lenses[theirs], slice=(sb[1], sb[2])) as other:
                other.render(17)
                if mine == theirs:
                    f.load(states[theirs])
                    g.merge(slices[theirs])
                    continue
                for attempt in (lambda: f.load(states[theirs]), lambda: g.merge(slices[theirs]), lambda: g.merge(other)):
                    with pytest.raises(api.KyError) as e:
                        attempt()
                    assert "lens" in str(e.value), (mine, theirs, str(e.value))
                assert f.done == 0 and g.done == 0
    with api.Frame(scene, p, lens=lenses["lens"]) as f:   # the refusal names this frame's lens where it has one
        with pytest.raises(api.KyError) as e:
            f.load(states["pinhole"])
        assert "without a lens" in str(e.value) and "lens radius 0.05, focus 2" in str(e.value)
    with api.Frame(scene, p, lens=lenses["lens"], filter=api.pixel_filter(A.FILTER_TENT, 2.0)) as f:   # a lens frame with another filter is another frame
        with pytest.raises(api.KyError):
            f.load(states["lens"])
    # set_lens after the first pass, after a load and after a merge
    with api.Frame(scene, p) as f:
        f.set_lens(lenses["wider"])
        f.set_lens(lenses["lens"])
        got = f.lens
        assert (got.radius, got.focus_distance) == (lenses["lens"].radius, 2.0)
        f.render(1)
        with pytest.raises(api.KyError) as e:
            f.set_lens(lenses["lens"])
        assert "lens" in str(e.value)
        with pytest.raises(api.KyError):
            f.set_lens(api.lens(0.0, 0.0))
    with api.Frame(scene, p) as f:
        f.load(states["pinhole"])
        with pytest.raises(api.KyError):
            f.set_lens(lenses["lens"])
    with api.Frame(scene, p, slice=(sb[0], sb[1])) as g:
        g.merge(slices["pinhole"])
        with pytest.raises(api.KyError):
            g.set_lens(lenses["lens"])
    with api.Frame(scene, p) as f:   # a refused lens leaves the frame's lens what it was
        with pytest.raises(api.KyError):
            f.set_lens(A.Lens(0.05, 0.0, (0, 0)))
        assert f.lens.radius == 0


# ---- the screen cull ----

def test_a_lens_launch_culls_nothing(O, A, api, lib):
    """The Cornell box at 96 x 72 (tests/test_screen_cull_gpu.py's frame): the pinhole's live rectangle begins at x = 8, so the frame's first column of 8 x 8 blocks
    is dead for the pinhole.  A wide lens focused far in front of the box -- at a tenth of the front ball's depth, where a scene point at depth z moves on the film
    by l (1 / focus - 1 / z), many pixels -- smears the box over that column: the oracle's samples, traced on the CPU, light a pixel there.  The film is the same
    with the cull on and off, and that pixel is lit.  A build whose lens rows read the pinhole's rectangle skips the column with the cull on and fails both."""
    from test_screen_cull_gpu import on_and_off
    w, h, n_spp = 96, 72, 16
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    p = TF.params_of(api, A, w, h, n_spp, "random")
    (x0, y0, x1, y1), dead, total = api.scene_screen_bound(scene, p)
    assert x0 == 8 and dead >= 9
    _, radius, ball = lens_of(O, A, api, "cornell", w, h)
    radius, focus = 4 * radius, 0.1 * ball
    lens = api.lens(radius, focus)
    assert api.scene_screen_bound(scene, p, lens=lens) == ((0, 0, w, h), 0, total)
    column = [(x, y) for x in range(4, 8) for y in range(h // 2 - 4, h // 2 + 4)]   # inside block column 0, which the pinhole never lights
    want = oracle_pixels(O, A, api, scene, p, 64, "random", None, radius, focus, column)
    lit = max(column, key=lambda xy: float(want[xy].sum()))
    mean = want[lit].astype(np.float64).mean(axis=0)
    print("pixel %s of the pinhole's dead column: the oracle's mean %s" % (lit, mean))
    assert mean.max() > 1e-3, "the oracle lights no pixel of the pinhole's dead column under this lens"
    for params in (p, TF.params_of(api, A, w, h, n_spp, "stratified")):
        on, off = on_and_off(lib, lambda: api.render(scene, params, lens=lens))
        assert b", lens>" in lib.kyhip_last_kernel(0)
        assert np.array_equal(on, off)
        assert on[lit[1], lit[0]].max() > 0 and on[:, :x0].any()
    assert abs(float(on_and_off(lib, lambda: api.render(scene, p, lens=lens))[0][lit[1], lit[0]].max()) - float(np.clip(mean, 0, 1).max())) <= 0.05   # ... by the oracle's light
    with api.Frame(scene, p, lens=lens, blocks=True) as f:   # the listed rows read the same rectangle
        f.render(n_spp)
        assert np.array_equal(f.resolve(), on_and_off(lib, lambda: api.render(scene, p, lens=lens))[1])


# ---- one frame per lens row ----

@pytest.mark.parametrize("listed", (False, True), ids=("plain", "listed"))
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("which", ("shipped", "general", "large"))
def test_one_frame_per_lens_row(O, A, api, lib, which, sampler, listed):
    """The Cornell box, a scene with general quads, triangles and disks, and the Cornell box with 65 more balls (more than 64 surfaces), at 16 x 16, N = 4, under a
    lens: the film is the mean of the oracle's samples, and kyhip_last_kernel names the plain, the general, the large and the listed lens rows -- all twelve."""
    w = h = 16
    n_spp = 4
    scene = {"shipped": lambda: api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), "general": lambda: T.general_scene(A, api), "large": lambda: T.large_scene(A, api, w, h)}[which]()
    params = TF.params_of(api, A, w, h, n_spp, sampler, direct_sample=A.DIRECT_LIGHT_MIS if which == "general" else A.DIRECT_BOTH_MIS)
    cam = L.Camera(scene.flat.contents.camera)
    sphere = O.world_bounding_sphere(scene)
    radius = 0.02 * 2 * float(sphere[3])
    focus = float((sphere[:3].astype(np.float64) - cam.position.astype(np.float64)) @ cam.front.astype(np.float64))
    lens = api.lens(radius, focus)
    with api.Frame(scene, params, lens=lens, blocks=listed) as f:
        f.render(n_spp)
        g = f.resolve()
    kernel = lib.kyhip_last_kernel(0).decode()
    print(which, sampler, listed, "->", kernel)
    assert ", lens>" in kernel and "strategy -1" in kernel and "run-time instantiation" not in kernel, kernel
    assert ("general shapes" in kernel) == (which != "shipped") and ("scene-sized LDS block" in kernel) == (which == "large"), kernel
    assert ("listed blocks" in kernel) == listed and ("stratified sampler" in kernel) == (sampler == "stratified"), kernel
    if not listed:
        assert np.array_equal(api.render(scene, params, lens=lens), g)
    want = oracle_samples(O, A, api, scene, ("row", which, sampler), params, 128, sampler, None, radius, focus)
    c = T.film_of(want)
    fin = np.isfinite(c).all(axis=2)
    e = rmse(g[fin], c[fin])
    print("%s: rmse %.3g, allowed %.3g" % (which, e, T.film_tolerance(n_spp)))
    assert g.max() > 0 and (~fin).sum() <= 2 and e < T.film_tolerance(n_spp)


# ---- the host mirror ----

def test_the_host_mirror_reads_the_lens_from_the_camera(O, A, api, lib):
    """camera_t::set_lens (ky.hpp) through render, render_passes and render_sliced: api.render(lens=)'s film, bit for bit; the scene's camera is the pinhole again
    afterwards; what kyhip_lens_check refuses is refused by set_lens."""
    w, h, n_spp = 20, 13, 17
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    lens = lens_of(O, A, api, "cornell", w, h)[0]
    for sampler in SAMPLERS:
        p = TF.params_of(api, A, w, h, n_spp, sampler)
        whole, plain = api.render(scene, p, lens=lens), api.render(scene, p)
        assert not np.array_equal(whole, plain)
        for mode in ("render", "passes", "sliced"):
            got = api.render_lens_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, p.sampler, n_spp, w, h, lens, mode=mode)
            assert np.array_equal(got, whole), (sampler, mode)
            assert b", lens>" in lib.kyhip_last_kernel(0)
        assert np.array_equal(api.render_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, p.sampler, n_spp, w, h), plain)
        assert np.array_equal(api.render_lens_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, p.sampler, n_spp, w, h, api.lens(0.0, 0.0)), plain)
    with pytest.raises(api.KyError):
        api.render_lens_host_api(scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, 4, w, h, A.Lens(0.05, -1.0, (0, 0)))
