"""A frame rendered in passes (include/kyhip.h, kyhip_frame_*; DESIGN.md "Passes").  A pixel's samples are cut into chunks by a schedule that depends on the
sample count only, work items are queued chunk by chunk, samples are keyed by their absolute index and chunk sums enter an integer accumulator: a frame
whose passes end on chunk boundaries is therefore the one-shot frame BIT FOR BIT, whatever the passes, whatever is rendered between them, and across a
save and a load.  Every comparison with a one-shot film here is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 40, 24   # 16 x 16 tiles: ragged tiles on the right and at the bottom


def _kernel(lib):
    return lib.kyhip_last_kernel(0)


def _scene(A, api, which, w=W, h=H):
    if which == "cornell":
        return api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    if which == "veach":
        return api.mis_scene(w, h)
    if which == "environment":
        return api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT, w, h)
    raise KeyError(which)


_one_shot = {}


def _reference(A, api, which, spp, **over):
    """api.render of the scene, once per (scene, params): (film, the kernel it ran on).  Never modified."""
    key = (which, spp, tuple(sorted(over.items())))
    if key not in _one_shot:
        film = api.render(_scene(A, api, which), api.make_params(W, H, spp, **over))
        film.setflags(write=False)
        _one_shot[key] = (film, _kernel(A.load_kyhip()))
    return _one_shot[key]


def _in_passes(api, lib, scene, p, min_samples):
    """The frame in passes of at least min_samples: (film, the `done` of each pass, the kernels of the passes without their pass suffix)."""
    dones, kernels = [], set()
    with api.Frame(scene, p) as f:
        assert (f.done, f.total) == (0, p.samples_per_pixel)
        while f.done < f.total:
            dones.append(f.render(min_samples))
            k = _kernel(lib)
            assert b", pass: chunks " in k, k
            kernels.add(k.split(b", pass:")[0])
        return f.resolve(), dones, kernels


CASES = [("cornell", {}), ("veach", {}), ("environment", {}), ("cornell", {"sampler": 0, "integrator": 9})]


@pytest.mark.parametrize("spp", [500, 7])
@pytest.mark.parametrize("which,over", CASES, ids=["cornell", "veach", "environment", "debug_recursion"])
def test_passes_equal_one_shot(which, over, spp, A, api, table_kernels):
    lib = A.load_kyhip()
    want, kernel = _reference(A, api, which, spp, **over)
    if table_kernels:
        assert {"veach": b"deferred shadow rays", "debug_recursion": b"debug sampler, strategy -1"}.get(
            "debug_recursion" if over else which, b"render_kernel<") in kernel, kernel
    scene = _scene(A, api, which)
    bounds = api.pass_boundaries(spp)
    for min_samples in (1, 100, spp):
        film, dones, kernels = _in_passes(api, lib, scene, api.make_params(W, H, spp, **over), min_samples)
        assert kernels == {kernel}, (kernels, kernel)   # both sides on one kernel: nothing but the passes differs
        assert set(dones) <= set(bounds) and dones == sorted(set(dones)) and dones[-1] == spp
        if min_samples == 1:
            assert dones == bounds                      # one chunk per pass
        if min_samples == spp:
            assert dones == [spp]
        if min_samples == 100 and spp == 500:
            assert dones == [112, 224, 324, 428, 500]   # each the first boundary at least 100 beyond the last
        assert np.array_equal(film, want), (which, spp, min_samples, float(np.abs(film - want).max()))


def test_pass_note_names_chunks_and_samples(A, api):
    lib = A.load_kyhip()
    with api.Frame(_scene(A, api, "cornell"), api.make_params(W, H, 500)) as f:
        assert f.render(48) == 48
        assert _kernel(lib).endswith(b", pass: chunks 0..1 of 51, samples 0..48 of 500")
        assert f.render(260) == 308
        assert _kernel(lib).endswith(b", pass: chunks 2..18 of 51, samples 48..308 of 500")


def test_a_shard_in_passes(A, api):
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, 500, tile_first=1, tile_step=2)
    base = np.full((H, W, 3), 0.25, np.float32)
    want = api.render(scene, p, film=base.copy())
    with api.Frame(scene, p) as f:
        while f.render(100) < f.total:
            pass
        got = f.resolve(film=base.copy())
    assert np.array_equal(got, want)
    untouched = (want == base).all(axis=2)
    assert untouched[:16, :16].all() and not untouched[:16, 16:32].all()   # tile 0 belongs to the other shard, tile 1 to this one


@pytest.mark.parametrize("spp", [7, 500])
def test_saturation_carries_across_passes(spp, A, api):
    """A lamp of radiance 4 T, T the frame's term limit.  At 7 spp (chunks of 4 and 3 samples, T = 2^30) each chunk sum of a pixel that sees the lamp is beyond
    T: it sets the pixel's +inf flag and adds nothing -- under the WHOLE frame's T in every pass (a one-chunk pass's own count would give 2e9, and the
    second chunk's 1.8e9 would be added).  At 500 spp the 51 chunk sums stay below T and add up to 4 T, inside the word's range."""
    lib = A.load_kyhip()
    p = api.make_params(W, H, spp)
    scene = _scene(A, api, "cornell")
    lamp = np.argwhere((api.render(scene, api.make_params(W, H, 1, max_path_depth=0)) > 0).all(axis=2))   # emission alone: pixels that look at the lamp
    assert len(lamp) > 0
    y, x = (int(v) for v in lamp[len(lamp) // 2])
    T = C.c_float(0)
    assert lib.kyhip_film_term_limit(C.byref(p), scene.c.light_count, 0, 0, C.byref(T)) > 0 and T.value >= 1
    for ch in range(3):
        scene.c.lights[0].color[ch] = 4.0 * T.value
    want = api.render(scene, p)
    assert (want[y, x] == 1.0).all()
    for min_samples in (1, 100):
        with api.Frame(scene, p) as f:
            while f.render(min_samples) < f.total:
                pass
            got = f.resolve()
        assert np.array_equal(got, want) and (got[y, x] == 1.0).all()


W4 = H4 = 64
_preview = {}


def _preview_film(A, api):
    """Cornell 64 x 64, 500 spp, stopped at the first boundary >= 100: (done, the normalised film, sum / total at that point, a second resolve onto the first)."""
    if not _preview:
        scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W4, H4)
        with api.Frame(scene, api.make_params(W4, H4, 500)) as f:
            done = f.render(100)
            mean = f.resolve(normalise=True)
            part = f.resolve(normalise=False)
            twice = f.resolve(normalise=True, film=mean.copy())
            assert f.done == done
        _preview.update(done=done, mean=mean, part=part, twice=twice, scene=scene)
    return _preview


def test_preview_is_the_mean_of_the_samples_done(A, api):
    """Bound: tests/test_single_light_gpu.py::test_render_is_the_mean_of_kat_li's for a Cornell film against its replay, 2e-5, no pixel set aside.  (The chunk
    sums are scaled by 1 / 500 before the fixed-point rounding, 2.3e-10 per term, and by 500 / done in double at the resolve: far below the bound.)"""
    pv = _preview_film(A, api)
    done = pv["done"]
    assert done == min(b for b in api.pass_boundaries(500) if b >= 100) == 112
    p = api.make_params(W4, H4, 500)
    d = []
    for y in range(3, H4, 9):
        for x in range(2, W4, 11):
            li = api.kat_li(pv["scene"], p, x, y, 0, done).astype(np.float64)
            d.append(np.abs(np.clip(li.mean(axis=0), 0, 1) - pv["mean"][y, x]).max())
    print("largest |preview - mean of kat_li| over %d pixels: %.2e" % (len(d), max(d)))
    assert max(d) <= 2e-5, max(d)
    below = pv["mean"] < 1
    err = np.abs(pv["part"].astype(np.float64) - pv["mean"].astype(np.float64) * done / 500)[below].max()
    print("largest |sum / total - mean x done / total|: %.2e" % err)
    assert below.any() and err <= 1e-6
    assert np.array_equal(pv["twice"], pv["mean"] + pv["mean"])   # a resolve ADDS, and leaves the frame as it was


def test_save_end_begin_load_finish(A, api):
    lib = A.load_kyhip()
    spp = 500
    want, kernel = _reference(A, api, "cornell", spp)
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, spp)
    with api.Frame(scene, p) as f:
        done = f.render(100)
        state = f.save()
    assert done == 112
    api.render(_scene(A, api, "veach"), api.make_params(W, H, 16))   # something else in between
    with api.Frame(_scene(A, api, "cornell"), api.make_params(W, H, spp)) as f:
        f.load(state)
        assert f.done == done
        while f.render(100) < f.total:
            assert _kernel(lib).split(b", pass:")[0] == kernel
        assert np.array_equal(f.resolve(), want)
    others = [("cornell", spp, {"seed": 99}, W, H), ("cornell", 499, {}, W, H), ("environment", spp, {}, W, H), ("cornell", spp, {}, W + 8, H)]
    for which, n, over, w, h in others:
        q = api.make_params(w, h, n, **over)
        own = api.render(_scene(A, api, which, w, h), q)
        with api.Frame(_scene(A, api, which, w, h), q) as g:
            first = g.render(50)
            with pytest.raises(api.KyError, match="kyhip error -1"):
                g.load(state)
            assert g.done == first
            while g.render(200) < g.total:
                pass
            assert np.array_equal(g.resolve(), own), (which, n, over, w, h)
    with api.Frame(scene, p) as f:
        for cut in (len(state) - 1, len(state) // 2, 8, 0):
            with pytest.raises(api.KyError, match="kyhip error -1"):
                f.load(state[:cut])
        assert f.done == 0
        assert lib.kyhip_frame_state_bytes(f._f) == len(state)
        assert lib.kyhip_frame_save(f._f, C.create_string_buffer(16), 16) == A.KY_ERR_INVALID_VALUE


def test_interleaved_frames_and_renders(A, api):
    want_a, _ = _reference(A, api, "cornell", 500)
    want_b, _ = _reference(A, api, "veach", 7)
    other, _ = _reference(A, api, "environment", 7)
    pa, pb, po = api.make_params(W, H, 500), api.make_params(W, H, 7), api.make_params(W, H, 7)
    with api.Frame(_scene(A, api, "cornell"), pa) as a, api.Frame(_scene(A, api, "veach"), pb) as b:
        while a.done < a.total:
            a.render(100)
            assert np.array_equal(api.render(_scene(A, api, "environment"), po), other)
            if b.done < b.total:
                b.render(1)
        assert b.done == b.total
        assert np.array_equal(a.resolve(), want_a) and np.array_equal(b.resolve(), want_b)


def test_edges(A, api):
    lib = A.load_kyhip()
    want, kernel = _reference(A, api, "cornell", 7)
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, 7)
    with api.Frame(scene, p) as f:
        fresh = f.resolve(normalise=True)
        assert not fresh.any()                               # nothing done: nothing added
        with pytest.raises(api.KyError, match="kyhip error -1"):
            f.render(0)
        assert f.render(1000) == 7
        last = _kernel(lib)
        assert f.render(1) == 7 and _kernel(lib) == last     # complete: nothing launched
        assert f.done == f.total == 7
        assert np.array_equal(f.resolve(), want) and np.array_equal(f.resolve(normalise=True), want)
    prev = lib.kyhip_set_engine(1)   # the queue engine renders no passes: the frame runs on the lane engine and says so
    try:
        with api.Frame(scene, p) as f:
            f.render(4)
            k = _kernel(lib)
            assert b"lane engine" in k and k.startswith(kernel), k
            f.render(4)
            got = f.resolve()
    finally:
        lib.kyhip_set_engine(prev)
    assert np.array_equal(got, want)


def test_host_mirror(A, api):
    pv = _preview_film(A, api)
    args = (pv["scene"], A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, 500, W4, H4)
    seen = []
    early = api.render_passes_host_api(*args, 100, on_pass=lambda done, total: seen.append((done, total)) or False)
    assert seen == [(pv["done"], 500)]
    assert np.array_equal(early, pv["mean"])
    seen = []
    full = api.render_passes_host_api(*args, 100, on_pass=lambda done, total: seen.append((done, total)) or True)
    dones = [d for d, _ in seen]
    assert dones == sorted(set(dones)) and dones[-1] == 500 and set(dones) <= set(api.pass_boundaries(500)) and all(t == 500 for _, t in seen)
    assert np.array_equal(full, api.render_host_api(*args))
