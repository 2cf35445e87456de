"""Adaptive sampling (include/kyhip.h, kyhip_frame_track_blocks ...; DESIGN.md "Adaptive"): a frame that retires 8 x 8 pixel blocks between its passes and
renders the live ones only, through the render kernels' listed form (ky_amd/csrc/ky_render.hpp, LISTED) and the film-sized kernels of ky_amd/csrc/ky_blocks.hip.
With nothing retired such a frame is the one-shot film; a retired block is the never-retiring frame at the block's sample count, bit for bit (integer
accumulators, samples keyed by absolute index); retiring by noise is held against NumPy on the map the device itself returns."""
import ctypes as C

import numpy as np
import pytest

import blocks_restatement as B
import noise_restatement as R

pytestmark = pytest.mark.gpu

W, H = 40, 24   # 16 x 16 tiles: ragged tiles on the right and at the bottom; 24 blocks, 15 with pixels inside
SPP = 500
PASSES = [112, 224, 324, 428, 500]   # passes of at least 100 samples


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


def _to_film(values, tile=16, fill=0, **shard):
    """Compact tile order -> (H, W), padding dropped, pixels the shard does not own = fill."""
    x, y, inside = R.pixel_xy(len(values), W, H, tile=tile, **shard)
    out = np.full((H, W) + values.shape[1:], fill, values.dtype)
    out[y[inside], x[inside]] = values[inside]
    return out


@pytest.mark.parametrize("spp", [500, 7])
@pytest.mark.parametrize("which,over", [("cornell", {}), ("veach", {}), ("environment", {}), ("cornell", {"sampler": 0})],
                         ids=["cornell", "veach", "environment", "debug_sampler"])
def test_nothing_retired_is_the_frame(which, over, spp, A, api, table_kernels):
    """A block-tracking frame rendered to the end without a retirement against api.render: every pass runs the listed twin of the one-shot launch's kernel -- the
    same instantiation with one load more per work item -- so the expectation is 0; the bound is the project's bound between two rows of the kernel table, 2.4e-7
    (tests/test_parity_gpu.py, test_specialised_instantiations_change_nothing).  Measured on the MI355X: the largest |difference| is 0.0 in all eight cases (the
    test prints it).  Two block-tracking frames cut into different passes run the same kernel on integer accumulators: array_equal."""
    lib = A.load_kyhip()
    want, kernel = _reference(A, api, which, spp, **over)
    scene = _scene(A, api, which)
    films = []
    for min_samples in (1, 100):
        with api.Frame(scene, api.make_params(W, H, spp, **over), blocks=True) as f:
            kernels = set()
            while f.done < f.total:
                f.render(min_samples)
                k = _kernel(lib)
                assert k.endswith(b", blocks: 15 of 24 live"), k
                kernels.add(k.split(b", pass:")[0])
            if table_kernels:   # the twin: the one-shot launch's row, listed
                assert kernels == {kernel.replace(b">", b", listed blocks>", 1)}, (kernels, kernel)
            st = f.block_stats()
            assert (st.blocks, st.live, st.samples_done, st.min_samples, st.max_samples, st.pixels, st.pixel_samples) == (24, 15, spp, spp, spp, W * H, W * H * spp)
            assert (f.sample_map() == spp).all()
            films.append(f.resolve())
    worst = max(float(np.abs(film.astype(np.float64) - want.astype(np.float64)).max()) for film in films)
    print("largest |block-tracking frame - one-shot film| (%s, %d spp): %.3e" % ("debug sampler" if over else which, spp, worst))
    assert worst <= 2.4e-7
    assert np.array_equal(films[0], films[1])


def _film_blocks(own):
    """The film's 8 x 8 blocks the shard owns, in raster order: [(bx, by)]."""
    return [(bx, by) for by in range(H // 8) for bx in range(W // 8) if own[by * 8, bx * 8]]


def _mask_of(blocks):
    m = np.zeros((H, W), np.uint8)
    for bx, by in blocks:
        m[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = 1
    return m


@pytest.mark.parametrize("tile,shard", [(16, {}), (16, dict(tile_first=1, tile_step=2)), (32, {})], ids=["whole", "shard_1_2", "tiles_32"])
def test_a_retired_block_is_the_frame_at_its_count(tile, shard, A, api):
    """Frame U tracks blocks and retires nothing; frame A renders the same passes and retires blocks by keep() between them.  A's sample map is the expected one, its
    normalised picture is, block by block, U's preview at the block's count, and its accumulators are U's at that pass: all array_equal."""
    lib = A.load_kyhip()
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, SPP, tile_w=tile, tile_h=tile, **shard)
    n_pix = int(lib.kyhip_shard_float_count(C.byref(p))) // 3
    n_blocks = n_pix // 64
    previews, accums = {}, {}
    with api.Frame(scene, p, blocks=True) as u:
        own = u.sample_map(out=np.full((H, W), -1, np.int32)) == 0
        for want_done in PASSES:
            assert u.render(100) == want_done
            previews[want_done] = u.resolve(normalise=True)
            prefix, st = B.split_blocks(u.save(), n_pix, n_blocks, noise=False)
            accums[want_done] = R.split_state(prefix, n_pix)[1]
            assert (st[:, 0] <= 0).all()
    blocks = _film_blocks(own)
    assert len(blocks) == {(16, 0): 15, (16, 1): 8, (32, 0): 15}[(tile, len(shard) // 2)]
    if not shard:
        assert blocks[0] == (0, 0) and blocks[-1] == (4, 2)        # the top-left block; the one in-film block of the ragged bottom-right tile
    # what is kept alive after passes 1, 2 and 3
    step1 = [b for b in blocks if b not in (blocks[0], blocks[-1])]
    step2 = [b for b in step1 if (b[0] + b[1]) % 2 == 1]
    step3 = step2[1:2]
    expected = np.zeros((H, W), np.int32)
    for b in blocks:
        count = 112 if b not in step1 else 224 if b not in step2 else 324 if b not in step3 else 500
        expected[b[1] * 8:b[1] * 8 + 8, b[0] * 8:b[0] * 8 + 8] = count
    assert len(step3) == 1 and sorted(set(expected[own].tolist())) == [112, 224, 324, 500]
    with api.Frame(scene, p, blocks=True) as a:
        for want_done, keep in zip(PASSES, (step1, step2, step3, step3, step3)):
            assert a.render(100) == want_done
            live = a.block_stats().live
            assert _kernel(lib).endswith(b", blocks: %d of %d live" % (live, n_blocks)), _kernel(lib)
            a.keep(_mask_of(keep))
            assert a.block_stats().live == len(keep)
        assert a.done == SPP
        assert np.array_equal(a.sample_map(), expected)
        st = a.block_stats()
        assert (st.blocks, st.live, st.passes, st.min_samples, st.max_samples, st.pixels, st.pixel_samples) == (n_blocks, 1, 5, 112, 500, int(own.sum()), int(expected.sum()))
        got = a.resolve(normalise=True)
        prefix, bst = B.split_blocks(a.save(), n_pix, n_blocks, noise=False)
        acc = R.split_state(prefix, n_pix)[1]
        count_compact = B.samples_per_pixel(bst, SPP, n_pix, tile)
        assert np.array_equal(_to_film(count_compact.astype(np.int32), tile, **shard), expected)
        for count in (112, 224, 324, 500):
            sel = expected == count
            assert sel.any() and np.array_equal(got[sel], previews[count][sel]), count
            pix = count_compact == count
            assert np.array_equal(acc[pix], accums[count][pix]), count
        assert (got[~own] == 0).all()
        # the last block retires: nothing is left to render
        a.keep(np.zeros((H, W), np.uint8))
        assert a.block_stats().live == 0 and np.array_equal(a.sample_map(), expected)
        kernel, ms = _kernel(lib), api.kernel_ms(0)
        assert a.render(100) == SPP == a.done
        assert _kernel(lib) == kernel and api.kernel_ms(0) == ms and a.block_stats().passes == 5
        assert np.array_equal(a.resolve(normalise=True), got)
        film = np.full((H, W, 3), 0.25, np.float32)
        with pytest.raises(api.KyError, match="kyhip error -1"):
            a.resolve(film=film)
        assert (film == 0.25).all()
    with api.Frame(scene, p, blocks=True) as a:        # retired before anything is rendered: blocks at 0 samples add nothing, and the others are the preview
        a.keep(_mask_of(step1))
        assert a.render(100) == 112
        got = a.resolve(normalise=True)
        gone = (a.sample_map() == 0) & own
        assert gone.sum() == 2 * 64 and (got[gone] == 0).all() and np.array_equal(got[~gone], previews[112][~gone])
        a.keep(np.zeros((H, W), np.uint8))             # ... and with none live the front stays where it is
        assert a.render(100) == 112 == a.done and a.block_stats().passes == 1


THRESHOLD, FRACTION, MIN_BATCHES = 0.008, 0.10, 3
N_PIX, N_BLOCKS = 6 * 256, 24
_hand = {}


def _by_hand(A, api):
    """The Cornell frame driven by hand, render(100) then retire_noisy, every step held against NumPy on the map the device returns; the state after step 3."""
    if _hand:
        return _hand
    hand = {}          # (the cache is filled at the end only: a run that fails half way leaves nothing behind for the next caller)
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, SPP)
    x, y, in_film = R.pixel_xy(N_PIX, W, H)
    inside = B.inside_count(N_PIX, W, H)
    pix_of = B.pixel_of_block(N_BLOCKS)
    state = B.initial_state(inside)
    frozen = np.full((H, W), np.nan, np.float32)
    accums, dones, runs = [], [], []
    worst = 0.0
    with api.Frame(scene, p, noise=True, blocks=True) as f:
        while f.block_stats().live > 0 and f.done < f.total:
            dones.append(f.render(100))
            m = f.noise()
            assert np.array_equal(m[~np.isnan(frozen)], frozen[~np.isnan(frozen)])          # retired pixels show their frozen value
            prefix, before = B.split_blocks(f.save(), N_PIX, N_BLOCKS, noise=True)
            assert np.array_equal(before, state)
            done, accum, flags, (batches, n_prev, y_prev, m2) = R.split_state(prefix, N_PIX)
            assert (done, batches, n_prev) == (dones[-1], len(dones), dones[-1])
            accums.append(accum)
            runs.append(R.run(accums, dones, SPP, flags)[-1])
            # the pairs and the map per block, at the block's own counts: a live block stands at this step, a retired one at the step it retired in
            step_of = np.array([len(dones) - 1 if s < 0 else (dones.index(s) if s > 0 else 0) for s in state[:, 0]])[B.block_of_pixel(N_PIX)]
            want_y = np.choose(step_of, [r[0] for r in runs])
            want_m2 = np.choose(step_of, [r[1] for r in runs])
            want_map = np.choose(step_of, [r[2] for r in runs])
            rendered = in_film & (B.samples_per_pixel(state, done, N_PIX) > 0)
            assert np.array_equal(y_prev[rendered], want_y[rendered])
            assert np.allclose(m2[rendered], want_m2[rendered], rtol=1e-12, atol=0)
            if len(dones) > 1:
                got_c, want_c = m[y[in_film], x[in_film]].astype(np.float64), want_map[in_film].astype(np.float64)
                err = np.abs(got_c - want_c)
                worst = max(worst, float((err / np.maximum(want_c, 1e-30)).max()))
                assert (err <= 1e-7 + 1e-5 * want_c).all() and (err <= 1.2e-7 * want_c).all()
            # the expected retirements from the device's own map, a float32 compare
            values = np.zeros(N_PIX, np.float32)
            values[in_film] = m[y[in_film], x[in_film]]
            counted = in_film & ((flags & 0x1FF) == 0)
            state = B.retire(state, values, counted, THRESHOLD, FRACTION, MIN_BATCHES, done, batches)
            st = f.retire_noisy(THRESHOLD, FRACTION, MIN_BATCHES)
            _, after = B.split_blocks(f.save(), N_PIX, N_BLOCKS, noise=True)
            assert np.array_equal(after, state)
            assert np.array_equal(f.sample_map(), _to_film(B.samples_per_pixel(state, done, N_PIX).astype(np.int32)))
            assert st.live == int((state[:, 0] < 0).sum()) and st.samples_done == done and st.passes == len(dones)
            newly = (after[:, 0] == done) & (before[:, 0] < 0)
            for b in np.flatnonzero(newly):
                sel = pix_of[b][in_film[pix_of[b]]]
                frozen[y[sel], x[sel]] = m[y[sel], x[sel]]
            if len(dones) == 3:
                hand["state3"] = f.save()
        print("retiring by noise: retired at %s; largest relative |map - restatement| %.3e" % (sorted(state[inside > 0, 0].tolist()), worst))
        hand.update(film=f.resolve(normalise=True), samples=f.sample_map(), noise=f.noise(), stats=bytes(f.block_stats()), state=state, inside=inside, dones=dones)
    _hand.update(hand)
    return _hand


def test_retiring_by_noise(A, api):
    """Threshold 0.008, at most a tenth of a block's pixels above it, three batches, passes of 100.  The CPU oracle's replay of this frame (tools/adaptive_replay.py,
    profiles/adaptive_replay.txt) retires 7 of the 15 blocks early, none before 324 samples, with the closest deciding pixel 42 % from the threshold; the GPU
    differs from the oracle in 0-1 of 1024 Cornell samples, so the condition below -- at least 5 retire early and at least 5 run to the end -- holds with room."""
    hand = _by_hand(A, api)
    at = hand["state"][hand["inside"] > 0, 0]
    at = np.where(at < 0, SPP, at)
    assert int((at < SPP).sum()) >= 5 and int((at == SPP).sum()) >= 5 and at.min() >= PASSES[MIN_BATCHES - 1]
    with api.Frame(_scene(A, api, "cornell"), api.make_params(W, H, SPP), noise=True, blocks=True) as f:
        done, st = f.render_adaptive(THRESHOLD, FRACTION, MIN_BATCHES, 100)
        assert done == f.done == hand["dones"][-1]
        assert bytes(st) == hand["stats"] == bytes(f.block_stats())
        assert np.array_equal(f.resolve(normalise=True), hand["film"])
        assert np.array_equal(f.sample_map(), hand["samples"])
        assert np.array_equal(f.noise(), hand["noise"])
        assert st.pixel_samples == int(hand["samples"].sum()) < W * H * SPP
    # ... and through the C++ host classes: integrator_t::render_adaptive
    args = (_scene(A, api, "cornell"), A.INTEGRATOR_PATH_TRACING_ITERATION, 5, A.DIRECT_BOTH_MIS, A.SAMPLER_RANDOM, SPP, W, H)
    film, counts, host_st = api.render_adaptive_host_api(*args, THRESHOLD, FRACTION, MIN_BATCHES, 100)
    assert np.array_equal(film, hand["film"]) and np.array_equal(counts, hand["samples"]) and bytes(host_st) == hand["stats"]


def test_checkpoint(A, api):
    hand = _by_hand(A, api)
    scene = _scene(A, api, "cornell")
    p = api.make_params(W, H, SPP)
    state3 = hand["state3"]
    with api.Frame(scene, p, noise=True, blocks=True) as f:
        f.load(state3)
        assert f.done == 324 and f.save() == state3 and f.block_stats().passes == 3   # the passes are part of the state
        while f.block_stats().live > 0 and f.done < f.total:
            f.render(100)
            f.retire_noisy(THRESHOLD, FRACTION, MIN_BATCHES)
        assert np.array_equal(f.resolve(normalise=True), hand["film"])
        assert np.array_equal(f.sample_map(), hand["samples"])
        assert np.array_equal(f.noise(), hand["noise"])
    with api.Frame(scene, p, noise=True) as g:          # a frame that does not track blocks
        g.render(100)
        plain = g.save()
        with pytest.raises(api.KyError, match="kyhip error -1"):
            g.load(state3)
        assert g.done == 112 and g.save() == plain
    at = R.HEADER_BYTES + N_PIX * 28 + R.TRAILER_BYTES + N_PIX * 16
    with api.Frame(scene, p, noise=True, blocks=True) as g:
        fresh = g.save()
        moved = bytearray(state3)
        live = int(np.flatnonzero(B.split_blocks(state3, N_PIX, N_BLOCKS, noise=True)[1][:, 0] < 0)[0])
        moved[at + 16 + 8 * live:at + 20 + 8 * live] = (101).to_bytes(4, "little")            # no pass ends at 101 samples
        beyond = bytearray(state3)
        beyond[at + 16 + 8 * live:at + 20 + 8 * live] = (428).to_bytes(4, "little")           # a pass ends there, but the state stands at 324
        other = bytearray(state3)
        other[at + 8:at + 12] = (N_BLOCKS - 1).to_bytes(4, "little")
        retired = int(np.flatnonzero(B.split_blocks(state3, N_PIX, N_BLOCKS, noise=True)[1][:, 0] == 324)[0])
        batches = bytearray(state3)
        batches[at + 20 + 8 * retired:at + 24 + 8 * retired] = (4).to_bytes(4, "little")       # four batches where the noise estimate has three
        for bad in (plain, state3[:at], state3[:at + 16], state3[:-1], bytes(moved), bytes(beyond), bytes(other), bytes(batches)):
            with pytest.raises(api.KyError, match="kyhip error -1"):
                g.load(bad)
            assert g.done == 0 and g.block_stats().live == 15 and g.save() == fresh
        g.load(state3)
        assert g.done == 324


def test_entries_need_their_tracking(A, api):
    scene = _scene(A, api, "cornell")
    lib = A.load_kyhip()
    with api.Frame(scene, api.make_params(W, H, 7)) as f:
        for call in (lambda: f.keep(np.ones((H, W))), lambda: f.sample_map(), lambda: f.block_stats(), lambda: f.retire_noisy(0.1), lambda: f.render_adaptive(0.1)):
            with pytest.raises(api.KyError, match="kyhip error -1"):
                call()
        f.render(1)
        assert lib.kyhip_frame_track_blocks(f._f) == A.KY_ERR_INVALID_VALUE     # something is rendered
    with api.Frame(scene, api.make_params(W, H, 7), blocks=True) as f:          # blocks without noise: keep() works, the noise rule does not
        with pytest.raises(api.KyError, match="kyhip error -1"):
            f.retire_noisy(0.1)
        assert lib.kyhip_frame_track_noise(f._f) == A.KY_OK                      # either order
        retire_ms, list_ms = f.blocks_ms()
        assert retire_ms < 0 and list_ms > 0                                     # no retire kernel yet; the first list was made when tracking began
        assert f.retire_noisy(0.1).live == 15
        assert min(f.blocks_ms()) > 0
    for noise in (False, True):   # a shard without tiles has no blocks: its front advances by bookkeeping alone, like a plain frame's empty shard
        with api.Frame(scene, api.make_params(W, H, 7, tile_first=6, tile_step=1), noise=noise, blocks=True) as f:
            assert f.block_stats().blocks == 0 and f.render(1) == 4 and f.render(1) == 7 == f.done and f.block_stats().passes == 2
        with api.Frame(scene, api.make_params(W, H, 7, tile_first=6, tile_step=1), noise=True, blocks=True) as f:
            done, st = (f.render_adaptive(0.1, 0.1, 2, 1) if noise else f.render_until(0.0, 0.0, 2, 1))
            assert done == 7


def test_render_until_ends_when_no_block_is_live(A, api):
    """kyhip_frame_render on a block-tracking frame without a live block renders nothing and leaves the front: kyhip_frame_render_until must not wait for a front
    that never comes, nor for a verdict that cannot change.  Threshold 0: no pixel is ever that clean, so only the missing live block ends the call."""
    scene = _scene(A, api, "cornell")
    with api.Frame(scene, api.make_params(W, H, SPP), noise=True, blocks=True) as f:
        assert f.render(100) == 112 and f.render(100) == 224
        f.keep(np.zeros((H, W), np.uint8))
        assert f.block_stats().live == 0
        done, st = f.render_until(0.0, 0.0, 2, 100)
        assert done == 224 == f.done == st.samples_done and st.batches == 2 and st.above > 0 and f.block_stats().passes == 2
        done, bs = f.render_adaptive(0.0, 0.0, 2, 100)
        assert done == 224 and bs.live == 0 and bs.passes == 2
    with api.Frame(scene, api.make_params(W, H, SPP), noise=True, blocks=True) as f:   # the last blocks retire inside the loop
        done, bs = f.render_adaptive(1e9, 1.0, 2, 100)      # everything is that clean: all retire behind the second pass
        assert done == 224 and bs.live == 0 and (f.sample_map() == 224).all()
        done, st = f.render_until(0.0, 0.0, 2, 100)
        assert done == 224 and st.samples_done == 224
        with api.Frame(scene, api.make_params(W, H, SPP), noise=True, blocks=True) as g:   # with live blocks render_until is what it is on any frame
            done, st = g.render_until(0.0, 0.0, 2, 100)
            assert done == SPP == g.done and g.block_stats().live == 15


def test_a_run_time_instantiation_takes_the_form_as_a_template_argument(A, api, tmp_path, monkeypatch, no_boxes):
    """kyhip_set_jit(1): a frame whose launch is no row of the table gets its own kernel, and a block-tracking frame the listed form of it (`..., 0, true>`: no drop
    bits, LISTED), a cache key of its own.  The two are one instantiation apart from the decoder's load: the expectation is 0, the bound the between-rows 2.4e-7."""
    monkeypatch.setenv("KYHIP_CACHE_DIR", str(tmp_path / "cache"))
    lib = A.load_kyhip()
    w, h = 64, 48
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_POINT, w, h)
    p = api.make_params(w, h, 64)
    prev = lib.kyhip_set_jit(1)
    try:
        films, kernels = [], []
        for blocks in (False, True):
            with api.Frame(scene, p, blocks=blocks) as f:
                while f.render(24) < f.total:
                    pass
                kernels.append(_kernel(lib))
                films.append(f.resolve())
        assert all(b"run-time instantiation" in k for k in kernels), (kernels, lib.kyhip_jit_status())
        assert b", 0, true>" in kernels[1] and b", 0, true>" not in kernels[0] and kernels[1].endswith(b", blocks: 48 of 48 live")
        worst = float(np.abs(films[0].astype(np.float64) - films[1].astype(np.float64)).max())
        print("largest |listed instantiation - plain instantiation|: %.3e" % worst)
        assert worst <= 2.4e-7 and films[0].max() > 0.1
    finally:
        lib.kyhip_set_jit(prev)
