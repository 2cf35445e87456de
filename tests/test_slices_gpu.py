"""Slices: a frame's sample ranges rendered apart and merged (include/kyhip.h "Slices"; DESIGN.md "Slices").  A pixel's samples are keyed by their absolute
index, cut into chunks by a schedule of the sample count alone, and chunk sums enter 64-bit integer words under the whole frame's term limit: frames that
rendered disjoint chunks of one (scene, params) hold words whose integer sum is the one-shot frame's, whatever the slices, the order of the merges, the device or
the process.  Every film and state comparison here is np.array_equal or bytes equality; the noise pairs are compared bit for bit with the NumPy restatement of
tests/slices_restatement.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_restatement as R
import slices_restatement as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H = 40, 24   # 16 x 16 tiles: ragged tiles on the right and at the bottom
N_PIX = 3 * 2 * 16 * 16
INVALID = "kyhip error -1"


def _kernel(lib):
    return lib.kyhip_last_kernel(0).split(b", pass:")[0]


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
    """Once per (scene, params), never modified: (api.render's film, the kernel it ran on, the accumulator and flag part of a complete kyhip_frame_begin frame's
    save)."""
    key = (which, spp, tuple(sorted(over.items())))
    if key not in _one_shot:
        scene, p = _scene(A, api, which), api.make_params(W, H, spp, **over)
        film = api.render(scene, p)
        film.setflags(write=False)
        kernel = _kernel(A.load_kyhip())
        with api.Frame(scene, p) as f:
            f.render(spp)
            assert f.done == spp
            words = S.accum_part(f.save(), N_PIX)
        _one_shot[key] = (film, kernel, words)
    return _one_shot[key]


def _render_to_end(f, min_samples, lib=None, kernels=None):
    """Passes until the frame's owned range is rendered: a pass that adds nothing (`done` counts merged samples too, so it says nothing about the owned range)."""
    before = -1
    while f.done != before:
        before = f.done
        f.render(min_samples)
        if kernels is not None and f.done != before:
            kernels.add(_kernel(lib))
    return f


CASES = [("cornell", {}), ("veach", {}), ("environment", {}), ("cornell", {"sampler": 0, "integrator": 9})]


@pytest.mark.parametrize("spp,n", [(500, 2), (500, 3), (500, 8), (7, 2)])
@pytest.mark.parametrize("which,over", CASES, ids=["cornell", "veach", "environment", "debug_recursion"])
def test_slices_equal_one_shot(which, over, spp, n, A, api):
    lib = A.load_kyhip()
    want, kernel, want_words = _reference(A, api, which, spp, **over)
    scene, p = _scene(A, api, which), api.make_params(W, H, spp, **over)
    bounds = api.slice_bounds(spp, n)
    states, kernels = [], set()
    for k in range(n):
        with api.Frame(scene, p, slice=(bounds[k], bounds[k + 1])) as f:
            assert (f.done, f.total, f.own, f.coverage) == (0, spp, (bounds[k], bounds[k + 1]), [])
            _render_to_end(f, 100, lib, kernels)
            assert f.coverage == [(bounds[k], bounds[k + 1])] and f.render(100) == f.done      # complete: its owned range is rendered
            states.append(f.save())
    assert kernels == {kernel}, (kernels, kernel)   # every pass and the one-shot render on one kernel: nothing but the slicing differs
    assert len({len(s) for s in states}) == 1       # one state size: one gather of equal-length buffers
    for order in (range(1, n), range(n - 1, 0, -1)):
        with api.Frame(scene, p, slice=(bounds[0], bounds[1])) as root:
            root.load(states[0])
            for k in order:
                root.merge(states[k])
            assert root.coverage == [(0, spp)] and root.done == spp
            assert np.array_equal(root.resolve(), want), (which, spp, n, list(order))
            assert S.accum_part(root.save(), N_PIX) == want_words


def test_collector_preview(A, api):
    spp = 500
    want, _, _ = _reference(A, api, "cornell", spp)
    scene, p = _scene(A, api, "cornell"), api.make_params(W, H, spp)
    bounds = api.slice_bounds(spp, 3)
    frames = [api.Frame(scene, p, slice=(bounds[k], bounds[k + 1])) for k in range(3)]
    try:
        for f in frames:
            f.render(50)
        states = [f.save() for f in frames]
        parts = [S.split_slice_state(s, N_PIX) for s in states]
        held = sum(part[0] for part in parts)
        assert [part[0] for part in parts] == [f.done for f in frames] and 0 < held < spp
        with api.Frame(scene, p, slice=(0, 0)) as collector:
            assert collector.own == (0, 0) and collector.render(100) == 0      # it owns nothing and renders nothing
            for s in states:
                collector.merge(s)
            assert collector.done == held and collector.coverage == [(bounds[k], bounds[k] + parts[k][0]) for k in range(3)]
            got_held, words, flags, _, (first, end, front, ranges) = S.split_slice_state(collector.save(), N_PIX)
            assert (got_held, first, end, front, ranges) == (held, 0, 0, 0, collector.coverage)
            assert np.array_equal(words, parts[0][1] + parts[1][1] + parts[2][1]) and np.array_equal(flags, parts[0][2] | parts[1][2] | parts[2][2])
            preview = collector.resolve(normalise=True)
            assert np.array_equal(preview, S.film_of(words, flags, float(spp) / float(held), W, H))
            assert preview.any() and np.array_equal(collector.resolve(), S.film_of(words, flags, 1.0, W, H))
        # the slices go on afterwards and still end at the one-shot film
        for f in frames:
            _render_to_end(f, 100)
        frames[0].merge(frames[2])
        frames[0].merge(frames[1])
        assert np.array_equal(frames[0].resolve(), want)
    finally:
        for f in frames:
            f.close()


@pytest.mark.parametrize("spp", [7, 500])
def test_saturation_across_slices(spp, A, api):
    """tests/test_frame_gpu.py::test_saturation_carries_across_passes's lamp of radiance 4 T, T the whole frame's term limit.  At 7 spp (chunks of 4 and 3, one per
    slice) each slice's chunk sum of a pixel that sees the lamp is beyond T: both slices set the +inf flag and add nothing.  At 500 spp the 51 chunk sums stay
    below T and add up across the two slices' words, inside the word's range, to a mean beyond T that no flag marks -- exactly the words of the one-shot frame.
    (Measured on the MI355X: the lamp pixel's mean is 2.2755 T per channel, 9.58e7 with T = 42107520, in the sliced and in the one-shot frame alike, not the 4 T of
    the lamp's radiance: what reaches the pixel is less than the bare radiance.  The test therefore asserts the exact statement, the words of the complete
    kyhip_frame_begin frame, and that the sum passes T, instead of the figure 4 T.)"""
    lib = A.load_kyhip()
    p = api.make_params(W, H, spp)
    scene = _scene(A, api, "cornell")
    lamp = np.argwhere((api.render(scene, api.make_params(W, H, 1, max_path_depth=0)) > 0).all(axis=2))
    y, x = (int(v) for v in lamp[len(lamp) // 2])
    T = C.c_float(0)
    assert lib.kyhip_film_term_limit(C.byref(p), scene.c.light_count, 0, 0, C.byref(T)) > 0 and T.value >= 1
    for ch in range(3):
        scene.c.lights[0].color[ch] = 4.0 * T.value
    want = api.render(scene, p)
    assert (want[y, x] == 1.0).all()
    with api.Frame(scene, p) as whole:
        whole.render(spp)
        want_words = S.accum_part(whole.save(), N_PIX)
    bounds = api.slice_bounds(spp, 2)
    px, py, _ = R.pixel_xy(N_PIX, W, H)
    i = int(np.flatnonzero((px == x) & (py == y))[0])
    with api.Frame(scene, p, slice=(0, bounds[1])) as a, api.Frame(scene, p, slice=(bounds[1], spp)) as b:
        _render_to_end(a, 100), _render_to_end(b, 100)
        parts = [S.split_slice_state(f.save(), N_PIX) for f in (a, b)]
        a.merge(b)
        got = a.resolve()
        merged = a.save()
        _, words, flags, _, _ = S.split_slice_state(merged, N_PIX)
    assert np.array_equal(got, want) and (got[y, x] == 1.0).all() and S.accum_part(merged, N_PIX) == want_words
    pinf = 0b111 << 3
    if spp == 7:
        assert all(int(part[2][i]) & pinf == pinf for part in parts) and int(flags[i]) & pinf == pinf
    else:
        assert int(flags[i]) & 0x1FF == 0 and all(int(part[2][i]) & 0x1FF == 0 for part in parts)
        total = words[i].astype(np.float64) / 4294967296.0
        each = [part[1][i].astype(np.float64) / 4294967296.0 for part in parts]
        print("the lamp pixel's words: %s = %s + %s, 4 T = %g" % (total, each[0], each[1], 4.0 * T.value))
        assert (total > T.value).all() and (total <= 4.0 * T.value).all() and all((0 < e).all() and (e < total).all() for e in each)   # beyond T, from two parts
        assert np.array_equal(words[i], parts[0][1][i] + parts[1][1][i])


def test_merge_refusals(A, api):
    spp = 500
    scene, p = _scene(A, api, "cornell"), api.make_params(W, H, spp)
    bounds = api.slice_bounds(spp, 3)
    assert bounds == [0, 160, 332, 500]

    def one_pass_state(which="cornell", slice=(0, 160), noise=False, blocks=False, **over):
        q = api.make_params(W, H, over.pop("spp", spp), **over)
        with api.Frame(_scene(A, api, which), q, slice=slice, noise=noise, blocks=blocks) as f:
            f.render(50)
            return f.save()

    good = one_pass_state()
    with api.Frame(scene, p, slice=(160, 332)) as dst:
        assert dst.render(50) == 64 and dst.coverage == [(160, 224)]
        before = dst.save()
        refused = {
            "overlapping coverage": one_pass_state(slice=(160, 332)),
            "a part of the unrendered owned range": one_pass_state(slice=(224, 332)),
            "another seed": one_pass_state(seed=99),
            "another spp": one_pass_state(spp=496, slice=(0, 48)),
            "another scene": one_pass_state("environment"),
            "another shard": one_pass_state(tile_first=1, tile_step=2),
            "short by a byte": good[:-1],
            "a header alone": good[:R.HEADER_BYTES],
            "nothing": b"",
            "a block-tracking frame's state": one_pass_state(slice=None, blocks=True),
        }
        for what, state in refused.items():
            with pytest.raises(api.KyError, match=INVALID):
                dst.merge(state)
            assert dst.save() == before and dst.coverage == [(160, 224)], what
        with api.Frame(scene, p, blocks=True) as blocky, api.Frame(scene, p, slice=(160, 332)) as twin, api.Frame(scene, p, slice=(224, 332)) as inside:
            blocky.render(50), twin.render(50), inside.render(50)
            for src in (blocky, twin, inside, dst):          # frame to frame: the same refusals, and a frame does not merge itself
                with pytest.raises(api.KyError, match=INVALID):
                    dst.merge(src)
                assert dst.save() == before
            held = blocky.save()
            for src in (good, dst):                           # a block-tracking frame receives nothing
                with pytest.raises(api.KyError, match=INVALID):
                    blocky.merge(src)
            assert blocky.save() == held
        with api.Frame(scene, p) as whole:                    # a frame that owns every sample receives nothing
            plain = whole.save()
            for src in (good, dst):
                with pytest.raises(api.KyError, match=INVALID):
                    whole.merge(src)
            assert whole.save() == plain
        with pytest.raises(api.KyError, match=INVALID):       # blocks retire on frames that own all their samples only
            api.Frame(scene, p, slice=(160, 332), blocks=True)
        with api.Frame(scene, p, slice=(160, 332), noise=True) as tracking:
            tracking.render(50)
            held = tracking.save()
            with pytest.raises(api.KyError, match=INVALID):   # a tracking frame needs the other frame's pairs
                tracking.merge(good)
            with pytest.raises(api.KyError, match=INVALID):
                tracking.merge(dst)
            assert tracking.save() == held
            tracking.merge(one_pass_state(noise=True))
            assert tracking.coverage == [(0, 64), (160, 224)] and tracking.noise_stats(0.0).batches == 2
        dst.merge(one_pass_state(noise=True))                 # a frame that does not track ignores the trailer
        assert dst.coverage == [(0, 64), (160, 224)] and dst.done == 128 and dst.save() != before and dst.merge_ms() > 0
        with pytest.raises(api.KyError, match=INVALID):       # ... and holds those samples now
            dst.merge(good)
    for bad in ((0, 100), (100, 160), (332, 160), (-1, 160), (160, 501)):
        with pytest.raises(api.KyError, match=INVALID):
            api.Frame(scene, p, slice=bad)


def _pairs_film(values, fill=0.0):
    x, y, inside = R.pixel_xy(N_PIX, W, H)
    out = np.full((H, W), fill, values.dtype)
    out[y[inside], x[inside]] = values[inside]
    return out


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _check_noise(api, f, words, flags, y, m2, batches, held):
    """The frame's saved pairs, map and statistics against restated ones, bit for bit."""
    got_held, got_words, got_flags, (got_batches, n_prev, got_y, got_m2), _ = S.split_slice_state(f.save(), N_PIX)
    assert (got_held, got_batches, n_prev) == (held, batches, held) and f.done == held
    assert np.array_equal(got_words, words) and np.array_equal(got_flags, flags)
    assert np.array_equal(_bits(got_y), _bits(y)) and np.array_equal(_bits(got_m2), _bits(m2))
    value = R.value(y, m2, batches, held, flags)
    assert np.array_equal(f.noise(), _pairs_film(value)) and np.isfinite(value).all()
    _, _, inside = R.pixel_xy(N_PIX, W, H)
    flagged = (flags & 0x1FF) != 0
    counted = inside & ~flagged
    threshold = float(np.median(value[counted]))
    st = f.noise_stats(threshold)
    assert (st.batches, st.samples_done, st.pixels, st.flagged) == (batches, held, W * H, int((inside & flagged).sum()))
    assert st.above == int((value[counted] > np.float32(threshold)).sum()) and st.max == value[counted].max()
    total = S.stats_sum(np.where(counted, value.astype(np.float64), 0.0))
    assert _bits(st.mean) == _bits(total / float(counted.sum()))


@pytest.mark.parametrize("n", [2, 3])
def test_noise_merges(n, A, api):
    spp = 500
    want, _, _ = _reference(A, api, "cornell", spp)
    scene, p = _scene(A, api, "cornell"), api.make_params(W, H, spp)
    bounds = api.slice_bounds(spp, n)
    frames = [api.Frame(scene, p, slice=(bounds[k], bounds[k + 1]), noise=True) for k in range(n)]
    try:
        root = frames[0]
        root.render(50), root.render(50)                       # the root: two batches of its own range so far
        for f in frames[1:]:
            _render_to_end(f, 50)
        parts = [S.split_slice_state(f.save(), N_PIX) for f in frames]
        assert all(part[3][0] >= 2 for part in parts)          # at least two batches each
        held, words, flags, (batches, _, y, m2), _ = parts[0]
        for k in range(1, n):                                  # one slice as a saved state, the others frame to frame
            root.merge(frames[k].save() if k == 1 else frames[k])
            n_b, words_b, flags_b, (batches_b, _, y_b, m2_b), _ = parts[k]
            words, flags, (y, m2) = S.merge(words, flags, words_b, flags_b, spp, (y, m2), held, (y_b, m2_b), n_b)
            held, batches = held + n_b, batches + batches_b
            _check_noise(api, root, words, flags, y, m2, batches, held)
        # one more pass of the root's own range: the batch is the difference to the MERGED luminance
        before = held
        root.render(50)
        held = root.done
        _, words, flags, _, _ = S.split_slice_state(root.save(), N_PIX)
        y, m2 = R.update(y, m2, R.luminance(words, spp), before, held)
        _check_noise(api, root, words, flags, y, m2, batches + 1, held)
        _render_to_end(root, 50)
        assert root.coverage == [(0, spp)] and np.array_equal(root.resolve(), want)
        # the merged whole-film frame is denoised like any other
        first, second = root.denoise(), root.denoise()
        assert first.tobytes() == second.tobytes() and np.isfinite(first).all() and first.any()
        assert np.array_equal(root.denoise({"levels": 0}), root.resolve(normalise=True))
    finally:
        for f in frames:
            f.close()


def test_slice_checkpoint(A, api):
    spp = 500
    scene, p = _scene(A, api, "cornell"), api.make_params(W, H, spp)
    for noise in (False, True):
        with api.Frame(scene, p, slice=(160, 332), noise=noise) as f:
            f.render(50)
            middle = f.save()
            _render_to_end(f, 50)
            whole = f.save()
        assert len(middle) == len(whole) == R.HEADER_BYTES + N_PIX * 28 + ((R.TRAILER_BYTES + N_PIX * 16) if noise else 0) + S.SLICE_TRAILER_BYTES
        with api.Frame(scene, p, slice=(160, 332), noise=noise) as g:
            g.load(middle)
            assert g.done == 64 and g.coverage == [(160, 224)] and g.save() == middle
            _render_to_end(g, 50)
            assert g.save() == whole                              # the interrupted slice is the uninterrupted one, byte for byte
        with api.Frame(scene, p, noise=noise) as plain:
            plain.render(50)
            plain_state = plain.save()
            assert len(plain_state) == len(middle) - S.SLICE_TRAILER_BYTES
            with pytest.raises(api.KyError, match=INVALID):       # a plain frame refuses a slice's state
                plain.load(middle)
            assert plain.save() == plain_state
        for other in ((160, 500), (0, 332), (224, 332), (0, 0)):   # a frame of another owned range refuses it, and a slice a plain frame's
            with api.Frame(scene, p, slice=other, noise=noise) as g:
                fresh = g.save()
                for state in (middle, plain_state):
                    with pytest.raises(api.KyError, match=INVALID):
                        g.load(state)
                assert g.save() == fresh and g.done == 0
        with api.Frame(scene, p, slice=(0, spp), noise=noise) as same:   # (0, spp) IS kyhip_frame_begin: the same checkpoint bytes
            same.render(50)
            assert same.save() == plain_state and same.own == (0, spp)


def test_merge_from_equals_merge(A, api):
    spp = 500
    scene, p = _scene(A, api, "veach"), api.make_params(W, H, spp)
    for noise in (False, True):
        with api.Frame(scene, p, slice=(0, 160), noise=noise) as a, api.Frame(scene, p, slice=(0, 160), noise=noise) as b, \
                api.Frame(scene, p, slice=(160, 500), noise=noise) as src:
            for f in (a, b, src):
                f.render(50), f.render(50)
            state = src.save()
            a.merge(state)
            b.merge(src)
            assert a.save() == b.save() and src.save() == state      # identical receivers, and the source unchanged
            assert a.merge_ms() > 0 and b.merge_ms() > 0 and src.merge_ms() < 0
            assert a.coverage == [(0, a.done - src.done), (160, 160 + src.done)]


def test_slice_of_a_shard(A, api):
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, 500, tile_first=1, tile_step=2)
    base = np.full((H, W, 3), 0.25, np.float32)
    want = api.render(scene, p, film=base.copy())
    with api.Frame(scene, p, slice=(0, 160)) as a, api.Frame(scene, p, slice=(160, 500)) as b:
        _render_to_end(a, 100), _render_to_end(b, 100)
        a.merge(b.save())
        got = a.resolve(film=base.copy())
    assert np.array_equal(got, want)
    untouched = (want == base).all(axis=2)
    assert untouched[:16, :16].all() and not untouched[:16, 16:32].all()   # tile 0 belongs to the other shard, tile 1 to this one


def test_render_sliced_api(A, api):
    spp = 500
    want, _, _ = _reference(A, api, "cornell", spp)
    scene, p = _scene(A, api, "cornell"), api.make_params(W, H, spp)
    seen, previews = [], []

    def on_pass(done, total, preview):
        seen.append((done, total))
        if len(seen) in (1, 2):
            previews.append(preview(denoise=len(seen) == 2))

    got = api.render_sliced(scene, p, [0, 0, 0], 100, on_pass=on_pass, noise=True)
    assert np.array_equal(got, want)
    dones = [d for d, _ in seen]
    assert dones == sorted(set(dones)) and dones[-1] == spp and all(t == spp for _, t in seen)
    assert len(previews) == 2 and all(v.shape == (H, W, 3) and np.isfinite(v).all() and v.any() for v in previews)
    assert np.array_equal(api.render_sliced(scene, p, [0, 0], 64, film=np.full((H, W, 3), 0.25, np.float32)), api.render(scene, p, film=np.full((H, W, 3), 0.25, np.float32)))


def test_host_mirror(A, api):
    """integrator_t::render_sliced (ky_amd/host/ky.hpp) with devices {0, 0}: render()'s film."""
    scene = _scene(A, api, "cornell")
    args = (scene, A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, 500, W, H)
    assert np.array_equal(api.render_sliced_host_api(*args, [0, 0], 100), api.render_host_api(*args))
    assert np.array_equal(api.render_sliced_host_api(*args, [0], 100), api.render_host_api(*args))


RANK_SCRIPT = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch.distributed as tdist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
tdist.init_process_group("gloo", rank=rank, world_size=world)
from ky_amd import api, _abi as A, dist as kd
scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, %(w)d, %(h)d)
film = kd.render_sliced_distributed(scene, api.make_params(%(w)d, %(h)d, 500), rank, world, device_index=0, min_samples_per_pass=100)
assert (film is None) == (rank != 0)
if rank == 0:
    np.save(%(out)r, film)
tdist.barrier()
tdist.destroy_process_group()
print("SLICED_OK", rank)
'''


def test_sliced_two_ranks_one_gpu(tmp_path, A, api):
    want, _, _ = _reference(A, api, "cornell", 500)
    out = str(tmp_path / "film.npy")
    script = tmp_path / "sliced_rank.py"
    script.write_text(RANK_SCRIPT % {"root": ROOT, "w": W, "h": H, "out": out})
    port = str(29800 + os.getpid() % 300)
    procs = [subprocess.Popen([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp_path,
                              env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)) for r in range(2)]
    try:
        for r, proc in enumerate(procs):
            stdout, stderr = proc.communicate(timeout=240)   # each rank under its own limit
            assert proc.returncode == 0 and "SLICED_OK %d" % r in stdout, (r, stdout[-1000:], stderr[-3000:])
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
    assert np.array_equal(np.load(out), want)
