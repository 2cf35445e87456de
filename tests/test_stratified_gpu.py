"""GPU: the stratified sampler (KY_SAMPLER_STRATIFIED) on the device against its NumPy restatement (tests/stratified_restatement.py) and
against the CPU oracle fed with the restatement's numbers (kyo_li_tape) -- streams bit for bit, paths and films to the tolerances tests/test_parity_gpu.py
applies under the random sampler, and every way of cutting a frame (passes, slices, shards, checkpoints) bit for bit against the one-shot film."""
import ctypes as C

import numpy as np
import pytest

import sampler_expectation as E
import sampler_restatement as R
import stratified_restatement as S
from helpers import rmse

pytestmark = pytest.mark.gpu

SPPS = (1, 2, 3, 4, 5, 7, 16, 17, 63, 64, 65, 500)


def film_tolerance(spp):
    """tests/test_parity_gpu.py's: RMSE below 1e-3 at 1024 samples per pixel, 1e-3 sqrt(1024 / spp) below that."""
    return 1e-3 * max(1.0, np.sqrt(1024.0 / spp))


def strat_params(api, A, w, h, spp, **kw):
    return api.make_params(w, h, spp, max_path_depth=5, direct_sample=A.DIRECT_BOTH_MIS, sampler=A.SAMPLER_STRATIFIED, **kw)


# ---- (6) streams ----

@pytest.mark.parametrize("k", (1, 17, 32))
def test_device_streams_equal_the_restatement(A, api, k):
    for seed in R.EDGE_SEEDS:
        for n_spp in SPPS:
            samples = sorted({0, 1, n_spp // 2, n_spp - 1} & set(range(n_spp)))
            keys = np.array([(p, s) for p in R.EDGE_PIXELS for s in samples], np.uint32)
            got = api.kat_sampler_kind(A.SAMPLER_STRATIFIED, seed, n_spp, keys, k)
            assert np.array_equal(got, S.bits(seed, keys, n_spp, k)), (seed, n_spp)


def test_device_streams_equal_the_restatement_on_many_random_keys(A, api):
    """2^16 + 37 keys at N = 500: many workgroups and a ragged last one; every sample index of the frame occurs."""
    gen = np.random.default_rng(20260102)
    n = (1 << 16) + 37
    keys = np.stack([gen.integers(0, 1 << 32, n, dtype=np.uint64), gen.integers(0, 500, n, dtype=np.uint64)], axis=1).astype(np.uint32)
    keys[:500, 1] = np.arange(500)
    for k in (1, 17, 32):
        got = api.kat_sampler_kind(A.SAMPLER_STRATIFIED, 1234, 500, keys, k)
        assert int(np.count_nonzero(got != S.bits(1234, keys, 500, k))) == 0, k


def test_one_sample_per_pixel_is_the_random_stream(A, api):
    keys = np.array([(p, 0) for p in R.EDGE_PIXELS], np.uint32)
    assert np.array_equal(api.kat_sampler_kind(A.SAMPLER_STRATIFIED, 99, 1, keys, 32), api.kat_sampler(99, keys, 32))


def test_the_older_kinds_through_the_new_entry(A, api):
    keys = R.edge_keys(1234)
    assert np.array_equal(api.kat_sampler_kind(A.SAMPLER_RANDOM, 1234, 7, keys, 32), api.kat_sampler(1234, keys, 32))
    assert np.array_equal(api.kat_sampler_kind(A.SAMPLER_DEBUG, 1234, 7, keys, 32), api.kat_sampler(1234, keys, 32, debug=True))


# ---- (7) paths, (8) frames ----

def scene_of(A, api, name, w, h):
    return api.mis_scene(w, h) if name == "veach" else api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)


_oracle_cache = {}


def oracle_samples(O, A, api, name, w, h, n_spp):
    """[h, w, N, 3]: the oracle's radiance of every sample of every pixel, its numbers read from the restatement's tape.  Computed once per case and shared."""
    key = (name, w, h, n_spp)
    if key not in _oracle_cache:
        scene, params = scene_of(A, api, name, w, h), strat_params(api, A, w, h, n_spp)
        stride = 256 if name == "veach" else 64
        out = np.zeros((h, w, n_spp, 3), np.float32)
        for y in range(h):
            for x in range(w):
                out[y, x], used = O.li_tape(scene, params, x, y, S.tape(params.seed, y * w + x, n_spp, stride))
        out.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def film_of(samples):
    """clamp01 of the per-pixel mean, as render() resolves it: the sum in double, one rounding."""
    return np.clip(samples.astype(np.float64).mean(axis=2), 0.0, 1.0).astype(np.float32)


@pytest.mark.parametrize("n_spp", (5, 16))
@pytest.mark.parametrize("name,w,h,bad_share,sum_tol", (("cornell", 32, 32, 0.002, 1e-4), ("veach", 48, 27, 0.014, 5e-3)))
def test_paths_equal_the_oracle_on_the_restatements_numbers(O, A, api, name, w, h, bad_share, sum_tol, n_spp):
    """kyhip_kat_li under the stratified sampler against kyo_li_tape fed by the restatement, every sample of every pixel of the frame: tests/test_parity_gpu.py's
    comparison (li_agreement) and its bounds for these scenes under the random sampler -- a sample differs if it is off by more than 1e-3 relative; at most
    0.2 % (Cornell) / 1.4 % (Veach: shadow rays at the sphere lights' self-occlusion threshold) may, and the sums clamped at 10 agree to 1e-4 / 5e-3."""
    scene, params = scene_of(A, api, name, w, h), strat_params(api, A, w, h, n_spp)
    want = oracle_samples(O, A, api, name, w, h, n_spp)
    bad = tot = 0
    sg = sc = 0.0
    for y in range(h):
        for x in range(w):
            g, c = api.kat_li(scene, params, x, y, 0, n_spp), want[y, x]
            fin = np.isfinite(c).all(1)
            d = np.abs(g[fin] - c[fin]).max(axis=1)
            s = np.maximum(1e-3, np.abs(c[fin]).max(axis=1))
            bad += int((d / s > 1e-3).sum())
            tot += int(fin.sum())
            sg += float(np.minimum(g[fin], 10).sum())
            sc += float(np.minimum(c[fin], 10).sum())
    print("%s N = %d: %d of %d samples differ, sums %.6g / %.6g" % (name, n_spp, bad, tot, sg, sc))
    assert bad <= bad_share * tot, (bad, tot)
    assert abs(sg - sc) <= sum_tol * max(sc, 1.0)


@pytest.mark.parametrize("n_spp", (5, 16, 17))
@pytest.mark.parametrize("size", (16, 32))
def test_film_is_the_mean_of_the_oracles_samples(O, A, api, size, n_spp):
    scene, params = scene_of(A, api, "cornell", size, size), strat_params(api, A, size, size, n_spp)
    g, c = api.render(scene, params), film_of(oracle_samples(O, A, api, "cornell", size, size, n_spp))
    fin = np.isfinite(c).all(axis=2)
    assert (~fin).sum() <= 2 and np.isfinite(g).all() and g.min() >= 0 and g.max() <= 1
    e = rmse(g[fin], c[fin])
    print("cornell %d x %d, N = %d: rmse %.3g, allowed %.3g" % (size, size, n_spp, e, film_tolerance(n_spp)))
    assert e < film_tolerance(n_spp)


def test_one_sample_film_is_the_random_film(A, api):
    for size in (16, 32):
        scene = scene_of(A, api, "cornell", size, size)
        assert np.array_equal(api.render(scene, strat_params(api, A, size, size, 1)),
                              api.render(scene, api.make_params(size, size, 1, max_path_depth=5, direct_sample=A.DIRECT_BOTH_MIS)))
    # ... and with more samples the two samplers differ
    scene = scene_of(A, api, "cornell", 16, 16)
    assert not np.array_equal(api.render(scene, strat_params(api, A, 16, 16, 5)), api.render(scene, api.make_params(16, 16, 5)))


@pytest.mark.parametrize("n_spp", (5, 16, 17))
@pytest.mark.parametrize("size", (16, 32))
def test_every_way_of_cutting_a_frame_is_the_one_shot_film(A, api, size, n_spp):
    """Passes, slices, a shard and a checkpoint: a stratum is a function of (seed, pixel, sample, N, position), so none of them can show."""
    scene, params = scene_of(A, api, "cornell", size, size), strat_params(api, A, size, size, n_spp)
    whole = api.render(scene, params)
    bounds = api.pass_boundaries(n_spp)
    # passes, unequal where the frame has the boundaries for it (N = 5: 4 + 1; 16: 4 + 8 + 4; 17: 4 + 8 + 5)
    with api.Frame(scene, params) as f:
        n_passes = 0
        for want in (4, 8, n_spp):
            if f.done < f.total:
                f.render(want)
                n_passes += 1
        assert f.done == n_spp and n_passes == min(3, len(bounds))
        assert np.array_equal(f.resolve(), whole)
    # two slices merged
    sb = api.slice_bounds(n_spp, 2)
    with api.Frame(scene, params, slice=(sb[0], sb[1])) as a, api.Frame(scene, params, slice=(sb[1], sb[2])) as b:
        a.render(n_spp)
        b.render(n_spp)
        a.merge(b)
        assert np.array_equal(a.resolve(), whole)
    # a shard: every second 16 x 16 tile, from the second on
    part = api.render(scene, strat_params(api, A, size, size, n_spp, tile_first=1, tile_step=2))
    mine = part.any(axis=2)
    assert np.array_equal(part[mine], whole[mine]) and (size == 16 or mine.any())
    rest = api.render(scene, strat_params(api, A, size, size, n_spp, tile_first=0, tile_step=2), film=part.copy())
    assert np.array_equal(rest, whole)
    # a checkpoint after the first pass, resumed in another frame
    with api.Frame(scene, params) as f:
        f.render(1)
        state = f.save()
    with api.Frame(scene, params) as f:
        f.load(state)
        assert f.done == bounds[0]
        f.render(n_spp)
        assert np.array_equal(f.resolve(), whole)


# ---- (9) one frame per table row ----

def general_scene(A, api):
    from test_parity_gpu import general_shapes_scene
    return general_shapes_scene(A, api)


def large_scene(A, api, w, h):
    """The Cornell box and 65 small matte and mirror balls: more than 64 surfaces."""
    from helpers import CustomScene, make_material, make_shape
    box_handle = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    box = box_handle.c
    shapes = [A.Shape.from_buffer_copy(box.shapes[i]) for i in range(box.shape_count)]
    mats = [A.Material.from_buffer_copy(box.materials[i]) for i in range(box.material_count)]
    lights = [A.Light.from_buffer_copy(box.lights[i]) for i in range(box.light_count)]
    surfaces = [A.Surface(box.surfaces[i].shape, box.surfaces[i].material, box.surfaces[i].area_light) for i in range(box.surface_count)]
    mats += [make_material(A, A.MATERIAL_MATTE, (0.6, 0.5, 0.3)), make_material(A, A.MATERIAL_MIRROR, (0.9, 0.9, 0.9))]
    r = np.random.default_rng(4)
    for k in range(65):
        shapes.append(make_shape(A, A.SHAPE_SPHERE, [(r.uniform(-1.0, 1.0), r.uniform(-1.0, 1.0), r.uniform(-1.1, 1.0))], radius=0.07))
        surfaces.append(A.Surface(len(shapes) - 1, len(mats) - 2 + (k & 1), -1))
    scene = CustomScene(A, A.Camera.from_buffer_copy(box.camera), shapes, mats, lights, surfaces)
    scene._keep_handle = box_handle
    return scene


def row_case(A, api, which, w, h):
    """-> (scene, params keywords, stride, render keywords, Frame keywords, what kyhip_last_kernel must name)."""
    strat = "render_kernel<stratified sampler, "
    if which == "cornell":
        return api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), {}, 64, {}, None, strat + "strategy 48, feat "
    if which == "veach":
        return api.mis_scene(w, h), {}, 256, {}, None, strat + "strategy 48, deferred shadow rays"
    if which == "environment":
        return api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT, w, h), {}, 64, {}, None, strat + "strategy 48, feat"
    if which == "general":
        return general_scene(A, api), {"direct_sample": A.DIRECT_LIGHT_MIS}, 128, {}, None, strat + "strategy -1, general shapes, feat 0,"
    if which == "plain":   # no row of facts holds light_mis under this sampler: the run-time-dispatched kernel
        return api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), {"direct_sample": A.DIRECT_LIGHT_MIS}, 64, {}, None, strat + "strategy -1, feat 0,"
    if which == "large":
        return large_scene(A, api, w, h), {}, 128, {}, None, strat + "strategy -1, general shapes, scene-sized LDS block"
    if which == "masked":
        return api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), {}, 64, {"lighting": 2}, None, "drop bits per launch"
    if which == "listed":
        return api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), {}, 64, {}, {"blocks": True}, "listed blocks"
    # the masked and listed twins of the general-shapes and large-scene rows
    if which == "general_masked":
        return general_scene(A, api), {"direct_sample": A.DIRECT_LIGHT_MIS}, 128, {"lighting": 2}, None, "general shapes, feat 0, integrator 11, drop bits per launch"
    if which == "large_masked":
        return large_scene(A, api, w, h), {}, 128, {"lighting": 2}, None, "general shapes, scene-sized LDS block, feat 0, integrator 11, drop bits per launch"
    if which == "general_listed":
        return general_scene(A, api), {"direct_sample": A.DIRECT_LIGHT_MIS}, 128, {}, {"blocks": True}, "general shapes, feat 0, integrator 11, listed blocks"
    if which == "large_listed":
        return large_scene(A, api, w, h), {}, 128, {}, {"blocks": True}, "general shapes, scene-sized LDS block, feat 0, integrator 11, listed blocks"
    raise KeyError(which)


@pytest.mark.parametrize("which", ("cornell", "veach", "environment", "plain", "general", "large", "masked", "listed", "general_masked", "large_masked", "general_listed", "large_listed"))
def test_one_frame_per_table_row(O, A, api, table_kernels, which):
    """16 x 16, N = 5 (a ragged 2 x 3 camera grid) on each kernel the table gained: the film is the mean of the oracle's samples on the restatement's numbers."""
    w = h = 16
    n_spp = 5
    lib = A.load_kyhip()
    scene, pkw, stride, rkw, fkw, name = row_case(A, api, which, w, h)
    kw = dict(max_path_depth=5, direct_sample=A.DIRECT_BOTH_MIS, sampler=A.SAMPLER_STRATIFIED)
    kw.update(pkw)
    params = api.make_params(w, h, n_spp, **kw)
    if fkw:
        with api.Frame(scene, params, **fkw) as f:
            f.render(n_spp)
            g = f.resolve()
    else:
        g = api.render(scene, params, **rkw)
    kernel = lib.kyhip_last_kernel(0).decode()
    print(which, "->", kernel)
    if table_kernels:
        assert "stratified sampler" in kernel and name in kernel and "run-time instantiation" not in kernel, kernel
        assert ("feat 0," in kernel) == (which not in ("cornell", "veach", "environment")), kernel   # the three headline rows are rows of scene facts
    samples = np.zeros((h, w, n_spp, 3), np.float32)
    for y in range(h):
        for x in range(w):
            tape = S.tape(params.seed, y * w + x, n_spp, stride)
            if rkw.get("lighting") == 2:   # lighting 2, the direct class alone: per sample the oracle at depth 1 minus the oracle at depth 0 (tests/test_lighting_gpu.py:
                # lighting 3 is the oracle at depth 1, lighting 1 the oracle at depth 0), both on the same numbers
                at = lambda depth: api.make_params(w, h, n_spp, **dict(kw, max_path_depth=depth))
                samples[y, x] = O.li_tape(scene, at(1), x, y, tape)[0] - O.li_tape(scene, at(0), x, y, tape)[0]
            else:
                samples[y, x], _ = O.li_tape(scene, params, x, y, tape)
    c = film_of(samples)
    fin = np.isfinite(c).all(axis=2)
    e = rmse(g[fin], c[fin])
    print("%s: rmse %.3g, allowed %.3g" % (which, e, film_tolerance(n_spp)))
    assert g.max() > 0 and (~fin).sum() <= 2 and e < film_tolerance(n_spp)


_masked_cache = {}


@pytest.mark.parametrize("boxes", (1, 0))
def test_masked_and_traced_samples_equal_the_oracle(O, A, api, boxes):
    """kyhip_kat_li_lighting and kyhip_kat_li_trace under the stratified sampler, every sample of eight pixels of the 16 x 16 Cornell frame at N = 16: the direct
    class alone is the oracle at depth 1 minus the oracle at depth 0 on the restatement's numbers (tests/test_lighting_gpu.py), and a traced sample ends with
    the radiance the oracle gives that sample; the comparison and bound are test_paths_equal_the_oracle_on_the_restatements_numbers' for this scene.
    boxes: kyhip_set_boxes -- with the box traversal the trace is the replay kernel's form with boxes, without it the one form no other test launches; the oracle's
    numbers, computed once, are the same for both."""
    w = h = n_spp = 16
    scene, params = scene_of(A, api, "cornell", w, h), strat_params(api, A, w, h, n_spp)
    at = lambda depth: api.make_params(w, h, n_spp, max_path_depth=depth, direct_sample=A.DIRECT_BOTH_MIS, sampler=A.SAMPLER_STRATIFIED)
    lib = A.load_kyhip()
    prev = lib.kyhip_set_boxes(boxes)
    try:
        bad = tot = 0
        for x, y in ((8, 8), (2, 13), (13, 2), (5, 5), (10, 4), (4, 10), (15, 15), (0, 7)):
            if (x, y) not in _masked_cache:
                tape = S.tape(params.seed, y * w + x, n_spp, 64)
                _masked_cache[x, y] = (O.li_tape(scene, params, x, y, tape)[0], O.li_tape(scene, at(1), x, y, tape)[0] - O.li_tape(scene, at(0), x, y, tape)[0])
            full, direct = _masked_cache[x, y]
            traced = np.stack([api.kat_li_trace(scene, params, x, y, s)[1] for s in range(n_spp)])
            rows, _ = api.kat_li_trace(scene, params, x, y, 0)
            assert len(rows) >= 1 and rows[0][0] == 0
            for g, c in ((api.kat_li_lighting(scene, params, 2, x, y, 0, n_spp), direct), (traced, full)):
                fin = np.isfinite(c).all(1)
                d = np.abs(g[fin] - c[fin]).max(axis=1)
                bad += int((d / np.maximum(1e-3, np.abs(c[fin]).max(axis=1)) > 1e-3).sum())
                tot += int(fin.sum())
    finally:
        lib.kyhip_set_boxes(prev)
    print("boxes %d: %d of %d samples differ" % (boxes, bad, tot))
    assert tot >= 250 and bad <= 0.002 * tot, (bad, tot)


# ---- (10) run-time instantiation ----

def test_run_time_instantiation_renders_the_tables_film(A, api, tmp_path, monkeypatch, no_boxes):
    """A stratified launch outside the table (light_mis on the Cornell box) with kyhip_set_jit(1): its own kernel, named so, and the film of the table's
    run-time-dispatched kernel within tests/test_jit.py's tolerance between an instantiation and the table (below 2e-5 per channel, the box traversal off:
    only the instantiation would have it)."""
    monkeypatch.setenv("KYHIP_CACHE_DIR", str(tmp_path / "cache"))
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 32, 32)
    params = api.make_params(32, 32, 16, direct_sample=A.DIRECT_LIGHT_MIS, sampler=A.SAMPLER_STRATIFIED)
    prev = lib.kyhip_set_jit(0)
    try:
        table = api.render(scene, params)
        assert "run-time instantiation" not in lib.kyhip_last_kernel(0).decode()
        lib.kyhip_set_jit(1)
        own = api.render(scene, params)
        name = lib.kyhip_last_kernel(0).decode()
        assert "run-time instantiation" in name and "stratified sampler, strategy 32" in name and "render_kernel<2, 32," in name, (name, lib.kyhip_jit_status())
        assert np.abs(own - table).max() < 2e-5 and table.max() > 0.1, float(np.abs(own - table).max())
    finally:
        lib.kyhip_set_jit(prev)


# ---- (11) refusals, each before any device work ----

def test_refusals(A, api):
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 16, 16)
    film = np.zeros((16, 16, 3), np.float32)

    def render_rc(params):
        return lib.kyhip_render(0, api._scene_ptr(scene), C.byref(params), film.ctypes.data_as(C.c_void_p), 16)

    assert render_rc(api.make_params(16, 16, 4, sampler=3)) == A.KY_ERR_INVALID_VALUE
    assert render_rc(api.make_params(16, 16, (1 << 24) + 1, sampler=A.SAMPLER_STRATIFIED)) == A.KY_ERR_INVALID_VALUE
    assert film.max() == 0
    p = strat_params(api, A, 16, 16, 5)
    with pytest.raises(api.KyError):
        api.kat_li(scene, p, 3, 3, 0, 6)            # sample 5 of 5
    with pytest.raises(api.KyError):
        api.kat_li(scene, p, 3, 3, 5, 1)
    with pytest.raises(api.KyError):
        api.kat_li_trace(scene, p, 3, 3, 5)
    assert api.kat_li(scene, p, 3, 3, 4, 1).shape == (1, 3)
    keys = np.array([(0, 4), (1, 5)], np.uint32)
    with pytest.raises(api.KyError):
        api.kat_sampler_kind(A.SAMPLER_STRATIFIED, 1, 5, keys, 4)      # key 1: sample 5 of 5
    with pytest.raises(api.KyError):
        api.kat_sampler_kind(A.SAMPLER_STRATIFIED, 1, (1 << 24) + 1, keys, 4)
    with pytest.raises(api.KyError):
        api.kat_sampler_kind(3, 1, 5, keys[:1], 4)
    assert api.kat_sampler_kind(A.SAMPLER_STRATIFIED, 1, 6, keys, 4).shape == (2, 4)
