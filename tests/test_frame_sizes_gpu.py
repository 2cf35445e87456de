"""Frames in passes, the noise estimate and the block kernels (DESIGN.md "Passes", "Noise", "Adaptive") at the frame sizes where their form changes.  The other
GPU tests of these run on a 40 x 24 frame (24 blocks, 6 noise partials, every work item a wavefront's own index, no block partly inside the film).  Here:

BIG, 264 x 512 at 16 x 16 tiles: 544 tiles, 139 264 compact pixels, 2176 blocks of which 2112 have pixels inside the film.
  - the live-list compaction (ky_amd/csrc/ky_blocks.hip) works on 8 groups of 256 blocks and one of 128, so the offsets across a group's wavefronts and across groups
    are not 0;
  - noise_final_kernel (ky_amd/csrc/ky_noise.hip) reduces 544 partials, three per thread with a ragged last thread (182 threads are used); the shard
    tile_first=1, tile_step=3 has 181 partials, one per thread with idle threads: the other side of that boundary;
  - a pass has more work items than any grid has wavefronts, so items come from the atomic work counter (ky_amd/csrc/ky_render.hpp): with chunk_first > 0, and
    through the live list.  The tests ASSERT n_items > 32 x CUs for those passes: a CU holds at most 32 wavefronts, whatever occupancy the kernel reaches.
RAGGED, 44 x 21 with tiles 16 x 16, 32 x 8, 8 x 24 and 8 x 8: blocks partly inside the film (4 columns, 5 rows, 4 x 5 in the corner), tiles that are not square
(blocks_w != tile_h / 8) and the tile that is one block.

What is asserted is what the small tests assert: integer accumulators and samples keyed by absolute index make every comparison between frames array_equal; the
noise values are held against the NumPy float64 restatement with test_noise_gpu.py's bounds; block decisions against tests/blocks_restatement.py on the map the
device itself returns."""
import re

import numpy as np
import pytest

import blocks_restatement as B
import noise_restatement as R
from test_blocks_gpu import _kernel, _scene

pytestmark = pytest.mark.gpu

SPP = 500
PASSES = [112, 224, 324, 428, 500]      # render(100) on the 500-sample schedule
                                        # (the schedule and the sizes' figures are pinned on the CPU: tests/test_blocks.py)
SHARD_1_3 = dict(tile_first=1, tile_step=3)


class Shape:
    """A frame's geometry, restated: the compact buffer's pixels in the film and its blocks."""

    def __init__(self, w, h, tile_w, tile_h, **shard):
        self.w, self.h, self.tile, self.shard = w, h, dict(tile_w=tile_w, tile_h=tile_h), shard
        tiles = -(-w // tile_w) * -(-h // tile_h)
        self.n_tiles = -(-(tiles - shard.get("tile_first", 0)) // shard.get("tile_step", 1))
        self.n_pix = self.n_tiles * tile_w * tile_h
        self.n_blocks = self.n_pix // 64
        self.x, self.y, self.in_film = R.pixel_xy(self.n_pix, w, h, **self.tile, **shard)
        self.inside = B.inside_count(self.n_pix, w, h, **self.tile, **shard)
        self.block_of = B.block_of_pixel(self.n_pix, **self.tile)
        self.pixel_of = B.pixel_of_block(self.n_blocks, **self.tile)
        self.own = self.to_film(np.ones(self.n_pix, bool), False)

    def params(self, api, spp):
        return api.make_params(self.w, self.h, spp, **self.tile, **self.shard)

    def to_film(self, values, fill=0):
        """Compact tile order -> (h, w), padding dropped, pixels the shard does not own = fill."""
        out = np.full((self.h, self.w) + values.shape[1:], fill, values.dtype)
        out[self.y[self.in_film], self.x[self.in_film]] = values[self.in_film]
        return out

    def from_film(self, film, fill=0):
        """(h, w) -> compact tile order; padding = fill."""
        out = np.full((self.n_pix,) + film.shape[2:], fill, film.dtype)
        out[self.in_film] = film[self.y[self.in_film], self.x[self.in_film]]
        return out

    def mask(self, blocks):
        return B.keep_mask(blocks, self.n_pix, self.w, self.h, **self.tile, **self.shard)

    def split(self, state, noise, blocks):
        """A checkpoint -> (samples done, accumulators, flag words, noise trailer or None, [n_blocks, 2] block state or None)."""
        bst = None
        if blocks:
            state, bst = B.split_blocks(state, self.n_pix, self.n_blocks, noise=noise)
        return R.split_state(state, self.n_pix) + (bst,)


BIG = Shape(264, 512, 16, 16)
BIG_SHARD = Shape(264, 512, 16, 16, **SHARD_1_3)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _note_chunks(note):
    m = re.search(rb", pass: chunks (\d+)\.\.(\d+) of (\d+)", note)
    assert m, note
    return int(m.group(1)), int(m.group(2)) - int(m.group(1)) + 1


def _assert_counter_fed(note, blocks_in_launch, plan_entry):
    """The pass behind `note` rendered the restated chunks, and its launch had more items than the device has wavefront slots: at most min(grid, slots) items are
    wavefronts' own indices, every other one is an id from the atomic counter."""
    first, chunks = _note_chunks(note)
    assert (first, chunks) == plan_entry[:2], (note, plan_entry)
    n_items, slots = blocks_in_launch * chunks, 32 * _cus()
    assert n_items > slots, "pass %r: %d items do not exceed %d wavefront slots: the work counter is not reached" % (note, n_items, slots)
    return n_items


_ref = {}


def _one_shot(A, api, which):
    """api.render of BIG at 500 spp, once per scene: (film, kernel).  Never modified."""
    if which not in _ref:
        film = api.render(_scene(A, api, which, BIG.w, BIG.h), BIG.params(api, SPP))
        film.setflags(write=False)
        _ref[which] = (film, _kernel(A.load_kyhip()))
    return _ref[which]


# ---- (a) passes fed from the work counter ----
@pytest.mark.parametrize("which", ["cornell", "veach"])
def test_counter_fed_passes_equal_one_shot(which, A, api, table_kernels):
    """A plain frame of BIG in passes of render(100): every pass has 2176 x (6 .. 17) items, beyond 32 x CUs, so from its second item on a wavefront decodes
    c = id / n_blocks + chunk_first from a counter id, with chunk_first > 0 from the second pass on.  The film is the one-shot film and the accumulators behind
    each pass are those of a frame cut at every chunk (2176 items a pass: every item a wavefront's own index): array_equal."""
    lib = A.load_kyhip()
    want, kernel = _one_shot(A, api, which)
    if table_kernels and which == "veach":
        assert b"deferred shadow rays" in kernel, kernel      # the row whose per-wavefront stacks are indexed by the full grid
    scene, p, plan = _scene(A, api, which, BIG.w, BIG.h), BIG.params(api, SPP), B.pass_plan(SPP, 100)
    accums = {}
    with api.Frame(scene, p) as f:
        for entry in plan:
            assert f.render(100) == entry[2]
            note = _kernel(lib)
            assert note.split(b", pass:")[0] == kernel, (note, kernel)
            _assert_counter_fed(note, BIG.n_blocks, entry)
            accums[entry[2]] = BIG.split(f.save(), False, False)[1]
        film = f.resolve()
    assert np.array_equal(film, want), float(np.abs(film - want).max())
    with api.Frame(scene, p) as g:
        for done in B.chunk_ends(SPP):
            assert g.render(1) == done
            if done in accums:
                assert np.array_equal(BIG.split(g.save(), False, False)[1], accums[done]), done
        assert np.array_equal(g.resolve(), want)


# ---- the never-retiring block-tracking frame of BIG: (b), and the yardstick of (c) and (e) ----
_never = {}


def _never_retiring(A, api, which):
    """Frame U: tracks blocks, retires nothing, passes of render(100).  Per pass its preview and accumulators; the film, the notes and the statistics at the end."""
    if which not in _never:
        lib = A.load_kyhip()
        u = dict(previews={}, accums={}, notes=[])
        with api.Frame(_scene(A, api, which, BIG.w, BIG.h), BIG.params(api, SPP), blocks=True) as f:
            for done in PASSES:
                assert f.render(100) == done
                u["notes"].append(_kernel(lib))
                u["previews"][done] = f.resolve(normalise=True)
                _, accum, _, _, bst = BIG.split(f.save(), False, True)
                u["accums"][done] = accum
                assert np.array_equal(bst, B.initial_state(BIG.inside))
            u["film"], u["stats"], u["samples"] = f.resolve(), f.block_stats(), f.sample_map()
        _never[which] = u
    return _never[which]


@pytest.mark.parametrize("which", ["cornell", "veach"])
def test_nothing_retired_is_the_frame_at_big(which, A, api, table_kernels):
    """test_blocks_gpu.py::test_nothing_retired_is_the_frame at BIG: the list holds 2112 of 2176 blocks (every group of the compaction contributes, the 64 holes are
    the padding blocks), and the first pass's 2112 x 6 items exceed 32 x CUs: list[id % n_live] with counter ids.  The expectation is 0; the bound is the
    project's bound between two rows of the kernel table, 2.4e-7; measured on the MI355X: 0.0 for both scenes (the test prints it).  The second cutting, one chunk
    a pass, has 2112 items a pass: wavefronts' own indices."""
    lib = A.load_kyhip()
    want, kernel = _one_shot(A, api, which)
    u = _never_retiring(A, api, which)
    plan = B.pass_plan(SPP, 100)
    for note, entry in zip(u["notes"], plan):
        assert note.endswith(b", blocks: 2112 of 2176 live"), note
        if table_kernels:
            assert note.split(b", pass:")[0] == kernel.replace(b">", b", listed blocks>", 1), (note, kernel)
    _assert_counter_fed(u["notes"][0], 2112, plan[0])
    st = u["stats"]
    assert (st.blocks, st.live, st.passes, st.samples_done, st.min_samples, st.max_samples, st.pixels, st.pixel_samples) == (
        2176, 2112, 5, SPP, SPP, SPP, 264 * 512, 264 * 512 * SPP)
    assert (u["samples"] == SPP).all()
    with api.Frame(_scene(A, api, which, BIG.w, BIG.h), BIG.params(api, SPP), blocks=True) as f:
        while f.render(1) < f.total:
            pass
        assert _kernel(lib).endswith(b", blocks: 2112 of 2176 live")
        assert f.block_stats().pixels == 264 * 512 and f.block_stats().passes == len(B.chunk_ends(SPP))
        other = f.resolve()
    worst = max(float(np.abs(film.astype(np.float64) - want.astype(np.float64)).max()) for film in (u["film"], other))
    print("largest |block-tracking frame - one-shot film| at 264 x 512 (%s, %d spp): %.3e" % (which, SPP, worst))
    assert worst <= 2.4e-7
    assert np.array_equal(u["film"], other)


def _held_against_never_retiring(shape, a, u_previews, u_accums, state, front, noise):
    """Frame `a` with the restated block state `state` ([n_blocks] retired_at) at `front`: its sample map, statistics, picture and accumulators are, block by
    block, the never-retiring frame's at the block's count."""
    retired_at = np.stack([state, np.zeros_like(state)], axis=1)
    count_compact = B.samples_per_pixel(retired_at, front, shape.n_pix, **shape.tile)
    expected = shape.to_film(count_compact.astype(np.int32))
    assert np.array_equal(a.sample_map(), expected)
    in_film_blocks = shape.inside > 0
    per_block = np.where(state >= 0, state, front)
    st = a.block_stats()
    assert (st.blocks, st.live, st.samples_done, st.min_samples, st.max_samples, st.pixels, st.pixel_samples) == (
        shape.n_blocks, int((state < 0).sum()), front, int(per_block[in_film_blocks].min()), int(per_block[in_film_blocks].max()), int(shape.in_film.sum()),
        int(expected.astype(np.int64).sum()))
    got = a.resolve(normalise=True)
    _, acc, _, _, bst = shape.split(a.save(), noise, True)
    assert np.array_equal(bst[:, 0], state)
    counts = sorted(set(per_block[in_film_blocks].tolist()))
    covered = np.zeros(shape.n_pix, bool)
    for count in counts:
        sel = (expected == count) & shape.own
        pix = (count_compact == count) & shape.in_film
        assert sel.any() and pix.any()
        if count == 0:
            assert (got[sel] == 0).all() and (acc[pix] == 0).all()
        else:
            assert np.array_equal(got[sel], u_previews[count][sel]), count
            assert np.array_equal(acc[pix], u_accums[count][pix]), count
        covered |= pix
    assert np.array_equal(covered, shape.in_film)          # every pixel inside the film was compared
    assert (got[~shape.own] == 0).all()
    return counts


# ---- (c) retired blocks across wave and group boundaries ----
def test_retired_blocks_across_waves_and_groups(A, api):
    """test_blocks_gpu.py::test_a_retired_block_is_the_frame_at_its_count at BIG, the kept sets chosen in block-index space so that the compaction (group_live,
    blocks_count / _scan / _scatter_kernel: groups of 256 blocks, four wavefronts each) meets every case it distinguishes.  Behind pass 1: a group with nothing
    live (256..511), a group's wavefront with nothing live (64..127), a group with its first and last block only (512, 767), a group alternating live and retired
    (768..1023), the last, partial group with its last block only.  These retire 799 of the 2112 in-film blocks: 1313 stay (not three quarters: the five cases
    alone take more than a quarter), and 1313 x 7 items of pass 2 still exceed 32 x CUs on 256 CUs, which the test asserts.  Behind pass 2 every index that is a
    multiple of 3 goes, behind pass 3 every index that is 1 modulo 7: holes in every group and wavefront.  A wrong list entry adds samples to a retired block, a
    missing one leaves a live block short, a duplicate adds twice: each shows in the accumulators, compared array_equal with the never-retiring frame's."""
    lib = A.load_kyhip()
    u = _never_retiring(A, api, "cornell")
    idx, in_film = np.arange(BIG.n_blocks), BIG.inside > 0
    last = int(np.flatnonzero(in_film)[-1])
    gone = ((idx >= 256) & (idx < 512)) | ((idx >= 64) & (idx < 128)) | ((idx > 512) & (idx < 767)) | ((idx >= 768) & (idx < 1024) & (idx % 2 == 1)) | (
        (idx >= 2048) & (idx != last))
    keep1 = in_film & ~gone
    keep2 = keep1 & (idx % 3 != 0)
    keep3 = keep2 & (idx % 7 != 1)
    per_wave = keep1[:2048].reshape(8, 4, 64).sum(axis=2)
    assert last >= 2048 and in_film[[512, 767]].all() and per_wave[1].sum() == 0 and per_wave[0, 1] == 0 and (per_wave[0, [0, 2, 3]] > 0).all()
    assert per_wave[2].tolist() == [1, 0, 0, 1] and per_wave[3].tolist() == [32] * 4 and int(keep1[2048:].sum()) == 1
    assert (int(keep1.sum()), int(keep2.sum()), int(keep3.sum())) == (1313, 875, 748)
    assert all((k.reshape(-1, 64)[:34].sum(axis=1) < 64).all() for k in (keep2, keep3))          # holes in every wavefront
    plan = B.pass_plan(SPP, 100)
    state = B.initial_state(BIG.inside)[:, 0]
    fed = []
    with api.Frame(_scene(A, api, "cornell", BIG.w, BIG.h), BIG.params(api, SPP), blocks=True) as a:
        for entry, keep in zip(plan, (keep1, keep2, keep3, keep3, keep3)):
            live = int((state < 0).sum())
            assert a.render(100) == entry[2]
            note = _kernel(lib)
            assert note.endswith(b", blocks: %d of %d live" % (live, BIG.n_blocks)), note
            if entry[2] in (224, 428, 500):        # passes behind a retirement whose items exceed the wavefront slots: through the list, from the counter
                fed.append(_assert_counter_fed(note, live, entry))
            a.keep(BIG.mask(np.flatnonzero(keep)))
            state = np.where((state < 0) & ~keep, entry[2], state)
            assert a.block_stats().live == int((state < 0).sum()) == int(keep.sum())
        assert a.done == SPP and a.block_stats().passes == 5
        counts = _held_against_never_retiring(BIG, a, u["previews"], u["accums"], state, SPP, noise=False)
    assert counts == [112, 224, 324, 500]
    print("retired across waves and groups: live 2112 -> 1313 -> 875 -> 748; counter-fed passes of %s items" % fed)


# ---- (d) noise statistics beyond 256 partials ----
def _stats_against_numpy(shape, f, m, flags, batches, done):
    """noise_stats at four thresholds: two calls return identical bytes, and every field is NumPy's on the map `m` the device returned.  (A block retired before
    its second batch keeps +inf: then the maximum and the mean are +inf too.)"""
    flagged = shape.to_film((flags & 0x1FF) != 0, False)
    good = m[shape.own & ~flagged]
    finite = good[np.isfinite(good)]
    for threshold in (0.0, float(np.median(finite)), float(finite.max()), 1e9):
        a, b = f.noise_stats(threshold), f.noise_stats(threshold)
        assert bytes(a) == bytes(b)
        assert (a.batches, a.samples_done, a.pixels, a.flagged) == (batches, done, int(shape.in_film.sum()), int((flagged & shape.own).sum()))
        assert a.above == int((good > np.float32(threshold)).sum()) and a.max == good.max() and a.threshold == np.float32(threshold)
        if len(finite) < len(good):
            assert np.isinf(a.mean) and a.mean > 0
        else:
            assert abs(a.mean - good.astype(np.float64).mean()) <= 1e-12 * a.mean


def _map_bounds(got_c, want_c):
    """test_noise_gpu.py::test_estimator_against_its_restatement's bounds on the map: +inf where the restatement has it, else the issue's 1e-7 + 1e-5 * value
    and the tight one, one float32 ulp.  Returns the largest relative difference."""
    inf = np.isinf(want_c)
    assert np.array_equal(np.isinf(got_c), inf)
    got_c, want_c = got_c[~inf], want_c[~inf]
    if not len(want_c):
        return 0.0
    err = np.abs(got_c - want_c)
    worst = float((err / np.maximum(want_c, 1e-30)).max())
    assert (err <= 1e-7 + 1e-5 * want_c).all()
    assert (err <= 1.2e-7 * want_c).all(), worst
    return worst


def _noise_frame_against_restatement(A, api, shape, spp, min_samples, which="cornell", blocks=False, record=None):
    """A noise-tracking frame (blocks: one that tracks blocks too and retires none, so the noise kernels read the per-block state) rendered to the end: y_prev, m2
    and the map behind every pass against the restatement on the checkpoint's accumulators (test_noise_gpu.py::test_estimator_against_its_restatement's bounds:
    equal, 1e-12 relative, one float32 ulp), and the statistics behind every pass from the second against NumPy on the map the device returns.
    record: a dict that receives, per sample count, the frame's preview and accumulators."""
    lib = A.load_kyhip()
    worst, accums, dones = 0.0, [], []
    with api.Frame(_scene(A, api, which, shape.w, shape.h), shape.params(api, spp), noise=True, blocks=blocks) as f:
        while f.done < f.total:
            dones.append(f.render(min_samples))
            done, accum, flags, (batches, n_prev, y_prev, m2), bst = shape.split(f.save(), True, blocks)
            accums.append(accum)
            assert (done, batches, n_prev) == (dones[-1], len(dones), dones[-1])
            if blocks:
                assert np.array_equal(bst, B.initial_state(shape.inside))
                assert _kernel(lib).endswith(b", blocks: %d of %d live" % (int((shape.inside > 0).sum()), shape.n_blocks))
            if record is not None:
                record[done] = (f.resolve(normalise=True), accum)
            want_y, want_m2, want_map = R.run(accums, dones, spp, flags)[-1]
            assert np.array_equal(y_prev, want_y)
            assert np.allclose(m2, want_m2, rtol=1e-12, atol=0) and (m2 >= 0).all()
            got = f.noise(out=np.full((shape.h, shape.w), -5.0, np.float32))
            assert (got[~shape.own] == -5).all()
            got_c, want_c = shape.from_film(got)[shape.in_film].astype(np.float64), want_map[shape.in_film].astype(np.float64)
            if len(dones) == 1:
                assert np.isinf(got_c).all() and np.isinf(want_c).all()
                continue
            worst = max(worst, _map_bounds(got_c, want_c))
            _stats_against_numpy(shape, f, f.noise(), flags, len(dones), done)
        assert len(dones) >= 3
        if blocks:
            st = f.block_stats()
            assert (st.pixels, st.pixel_samples, st.live) == (int(shape.in_film.sum()), int(shape.in_film.sum()) * spp, int((shape.inside > 0).sum()))
    return worst, len(dones)


class _Ledger:
    """What test_blocks_gpu.py's _by_hand keeps of a frame that tracks noise AND retires blocks, for any shape: behind every pass the frame's pairs and map are, block
    by block, the restatement's on the frame's own accumulators at the BLOCK's counts -- a live block stands at this pass, a retired one at the pass it retired
    behind, with that pass's batch count -- a retired block's pixels show the map value they had when it retired, and the statistics are NumPy's on the map."""

    def __init__(self, shape, spp):
        self.shape, self.spp, self.accums, self.dones, self.runs, self.worst = shape, spp, [], [], [], 0.0
        self.frozen = np.full((shape.h, shape.w), np.nan, np.float32)

    def after_pass(self, f, state):
        """state: the restated [n_blocks, 2] block state the pass was rendered with.  Returns (map, flags, done, batches)."""
        sh = self.shape
        m = f.noise()
        done, accum, flags, (batches, n_prev, y_prev, m2), bst = sh.split(f.save(), True, True)
        assert np.array_equal(bst, state)
        self.dones.append(done)
        self.accums.append(accum)
        assert (batches, n_prev) == (len(self.dones), done)
        self.runs.append(R.run(self.accums, self.dones, self.spp, flags)[-1])
        was = ~np.isnan(self.frozen)
        assert np.array_equal(m[was], self.frozen[was])                      # retired pixels show their frozen value
        step_of = np.array([len(self.dones) - 1 if s < 0 else (self.dones.index(s) if s > 0 else 0) for s in state[:, 0]])[sh.block_of]
        at = (step_of, np.arange(sh.n_pix))
        want_y, want_m2, want_map = (np.stack([r[k] for r in self.runs])[at] for k in range(3))
        rendered = sh.in_film & (B.samples_per_pixel(state, done, sh.n_pix, **sh.tile) > 0)
        assert rendered.any() and np.array_equal(y_prev[rendered], want_y[rendered])
        assert np.allclose(m2[rendered], want_m2[rendered], rtol=1e-12, atol=0)
        self.worst = max(self.worst, _map_bounds(sh.from_film(m)[rendered].astype(np.float64), want_map[rendered].astype(np.float64)))
        if len(self.dones) >= 2:
            _stats_against_numpy(sh, f, m, flags, batches, done)
        return m, flags, done, batches

    def retired(self, before, after, m):
        """The blocks that retired between the two states keep the map `m` they retired with."""
        sh = self.shape
        for b in np.flatnonzero((after[:, 0] >= 0) & (before[:, 0] < 0)):
            sel = sh.pixel_of[b][sh.in_film[sh.pixel_of[b]]]
            self.frozen[sh.y[sel], sh.x[sel]] = m[sh.y[sel], sh.x[sel]]


@pytest.mark.parametrize("shape", [BIG, BIG_SHARD], ids=["544_partials", "181_partials"])
def test_noise_statistics_beyond_256_partials(shape, A, api):
    """noise_final_kernel with three partials per thread and a ragged last thread (BIG), and with one per thread and idle threads (its shard 1 of 3).  Measured
    on the MI355X: every pixel's float32 equals the restatement's in both cases (largest relative difference 0; the test prints it)."""
    worst, passes = _noise_frame_against_restatement(A, api, shape, SPP, 100)
    assert passes == 5
    print("largest relative |map - restatement| at 264 x 512 (%d partials): %.3e" % (-(-shape.n_pix // 256), worst))


# ---- (e) retiring by noise at BIG ----
QUANTILE, FRACTION, MIN_BATCHES = 0.85, 0.10, 3


def test_retiring_by_noise_at_big(A, api):
    """Behind three passes the retire rule with the threshold at a quantile of the device's own map, at most a tenth of a block's pixels above it: the block state
    is the restatement's on that map (a float32 compare, as test_blocks_gpu.py's _by_hand).  The two remaining passes render the live blocks through the list --
    pass 4's items exceed 32 x CUs -- and every block is the never-retiring frame at its count.  The quantile is 0.85, not the median: on this frame the map is
    heavy-tailed (median 0.0016, 90th percentile 0.017) and at the median only 97 of the 2112 in-film blocks have so few pixels above it, fewer than the tenth
    the test wants on either side; measured on the MI355X with the restatement, quantile 0.60 / 0.70 / 0.75 / 0.80 / 0.85 / 0.90 / 0.95 retire 201 / 303 / 397 /
    572 / 824 / 1409 / 1662.  0.85 (threshold 0.01335) leaves both sides farthest from a tenth: 824 retire, 1288 stay."""
    lib = A.load_kyhip()
    u = _never_retiring(A, api, "cornell")
    plan = B.pass_plan(SPP, 100)
    state = B.initial_state(BIG.inside)
    in_film_blocks = BIG.inside > 0
    ledger = _Ledger(BIG, SPP)
    with api.Frame(_scene(A, api, "cornell", BIG.w, BIG.h), BIG.params(api, SPP), noise=True, blocks=True) as f:
        for entry in plan[:3]:
            assert f.render(100) == entry[2]
            m, flags, done, batches = ledger.after_pass(f, state)
        assert (done, batches) == (324, 3)
        counted = BIG.in_film & ((flags & 0x1FF) == 0)
        values = BIG.from_film(m)
        threshold = float(np.quantile(values[counted], QUANTILE))
        before = state
        state = B.retire(state, values, counted, threshold, FRACTION, MIN_BATCHES, done, batches, **BIG.tile)
        retired, stay = int((state[in_film_blocks, 0] == 324).sum()), int((state[in_film_blocks, 0] < 0).sum())
        print("retiring by noise at 264 x 512: threshold %.5g (quantile %.2f of the map), %d blocks retire at 324, %d stay" % (threshold, QUANTILE, retired, stay))
        assert retired + stay == 2112 and retired >= 212 and stay >= 212        # at least a tenth each
        st = f.retire_noisy(threshold, FRACTION, MIN_BATCHES)
        assert np.array_equal(BIG.split(f.save(), True, True)[4], state)
        assert (st.live, st.samples_done, st.passes) == (stay, 324, 3)
        ledger.retired(before, state, m)
        assert np.array_equal(f.noise(), m)                                      # retiring moves no value of the map
        for entry in plan[3:]:
            assert f.render(100) == entry[2]
            note = _kernel(lib)
            assert note.endswith(b", blocks: %d of %d live" % (stay, BIG.n_blocks)), note
            if entry[2] == 428:
                _assert_counter_fed(note, stay, entry)
            ledger.after_pass(f, state)        # the retired blocks' pairs and map values stay, the live ones' advance
        counts = _held_against_never_retiring(BIG, f, u["previews"], u["accums"], state[:, 0], SPP, noise=True)
    assert counts == [324, 500]
    print("retiring by noise at 264 x 512: largest relative |map - restatement|, retired blocks frozen: %.3e" % ledger.worst)


# ---- (f) ragged frames and other tile shapes ----
RW, RH, RSPP = 44, 21, 64
RPASSES = [16, 32, 48, 64]
TILES = [(16, 16), (32, 8), (8, 24), (8, 8)]


@pytest.mark.parametrize("tile_w,tile_h", TILES, ids=["%dx%d" % t for t in TILES])
def test_ragged_frame(tile_w, tile_h, A, api):
    """44 x 21: the right-hand blocks have 4 columns inside the film, the bottom ones 5 rows, the corner 4 x 5.  pixel_inside per lane, kyhip_frame_keep's mask,
    the retire rule's `counted` and ky_block_stats::pixels on such blocks, under tiles that are not square and the tile that is one block."""
    lib = A.load_kyhip()
    shape = Shape(RW, RH, tile_w, tile_h)
    scene, p = _scene(A, api, "cornell", RW, RH), shape.params(api, RSPP)
    assert set(shape.inside.tolist()) - {0} == {20, 32, 40, 64} and int(shape.inside.sum()) == RW * RH
    n_live = int((shape.inside > 0).sum())
    assert n_live == 18
    fresh = B.initial_state(shape.inside)
    bx, by = shape.x[shape.pixel_of[:, 0]] // 8, shape.y[shape.pixel_of[:, 0]] // 8          # each block's place in the film's grid of 8 x 8 blocks
    block_at = {(int(i), int(j)): b for b, (i, j) in enumerate(zip(bx, by))}
    corner, left_of_corner, right_edge, left_edge = block_at[(5, 2)], block_at[(4, 2)], block_at[(5, 0)], block_at[(0, 0)]
    assert (shape.inside[[corner, left_of_corner, right_edge, left_edge]] == (20, 40, 32, 64)).all()

    def kept_by(mask):
        with api.Frame(scene, p, noise=True, blocks=True) as g:
            assert g.block_stats().pixels == RW * RH and g.block_stats().live == n_live
            assert np.array_equal(shape.split(g.save(), True, True)[4], fresh)
            g.keep(mask)
            at = shape.split(g.save(), True, True)[4][:, 0]
            assert set(at.tolist()) <= {-1, 0}
            return set(np.flatnonzero(at < 0).tolist())

    one = np.zeros((RH, RW), np.uint8)
    one[RH - 1, RW - 1] = 1                                    # the film's last pixel: one pixel of the corner block's 4 x 5 inside
    assert kept_by(one) == {corner}
    assert kept_by(shape.mask([left_of_corner])) == {left_of_corner}      # every film pixel of its neighbour, none of its own
    # what the right-hand block's padding lanes would read without the inside test: x = 44 .. 47 of row y is x = 0 .. 3 of row y + 1 in the mask
    wrapped = np.zeros((RH, RW), np.uint8)
    wrapped[1:8, 0:4] = 1
    assert kept_by(wrapped) == {left_edge}
    one[:] = 0
    one[0, RW - 1] = 1
    assert kept_by(one) == {right_edge}

    # the never-retiring frame, blocks=True and noise=True: per pass its preview and accumulators; its pairs, map and statistics against the restatement (the noise
    # kernels read the per-block state: block_of_pixel under this tile, the padding blocks retired at 0)
    record = {}
    worst, passes = _noise_frame_against_restatement(A, api, shape, RSPP, 16, blocks=True, record=record)
    assert passes == 4 and sorted(record) == RPASSES
    previews, accums = {d: record[d][0] for d in record}, {d: record[d][1] for d in record}
    # frame A: the corner block and two others go by keep() behind pass 1 (one batch: their map value stays +inf), then the retire rule behind pass 3 (half of
    # a block's counted pixels may lie above the median of the live pixels).  The blocks of the bottom row and one of the right-hand column are still live then:
    # the rule decides blocks with counted = 40 and 32.  Behind every pass the ledger holds pairs, map and statistics against the restatement per block.
    state = fresh.copy()
    early = {corner, right_edge, left_edge}
    ledger = _Ledger(shape, RSPP)
    with api.Frame(scene, p, noise=True, blocks=True) as a:
        assert a.render(16) == 16
        m, _, _, _ = ledger.after_pass(a, state)
        a.keep(shape.mask([b for b in range(shape.n_blocks) if b not in early]))
        before, state = state, state.copy()
        state[sorted(early)] = (16, 1)
        assert np.array_equal(shape.split(a.save(), True, True)[4], state)
        ledger.retired(before, state, m)
        for want_done in (32, 48):
            assert a.render(16) == want_done
            assert _kernel(lib).endswith(b", blocks: %d of %d live" % (n_live - 3, shape.n_blocks))
            m, flags, done, batches = ledger.after_pass(a, state)
        counted = shape.in_film & ((flags & 0x1FF) == 0)
        values = shape.from_film(m)
        live_pix = counted & (state[shape.block_of, 0] < 0)
        threshold = float(np.median(values[live_pix]))
        n_counted = counted[shape.pixel_of].sum(axis=1)
        edge_live = (state[:, 0] < 0) & (n_counted > 0) & (n_counted < 64)
        assert sorted(n_counted[edge_live].tolist()) == [32, 40, 40, 40, 40, 40]      # what the rule's `counted` is on the live edge blocks
        before = state
        state = B.retire(state, values, counted, threshold, 0.5, 3, done, batches, **shape.tile)
        st = a.retire_noisy(threshold, 0.5, 3)
        assert np.array_equal(shape.split(a.save(), True, True)[4], state)
        ledger.retired(before, state, m)
        went = (state[:, 0] == 48)
        retired, stay = int(went.sum()), int((state[:, 0] < 0).sum())
        print("ragged frame, tile %d x %d: %d blocks retire at 48 (counted %s), %d stay (counted %s); largest relative |map - restatement| %.3e never retiring" % (
            tile_w, tile_h, retired, sorted(n_counted[went].tolist()), stay, sorted(n_counted[state[:, 0] < 0].tolist()), worst))
        assert st.live == stay and retired >= 1 and stay >= 1                          # both verdicts occur ...
        assert (went & edge_live).any() and (~went & edge_live).any()                  # ... each of them on a block with counted < 64
        assert a.render(16) == 64
        assert _kernel(lib).endswith(b", blocks: %d of %d live" % (stay, shape.n_blocks))
        ledger.after_pass(a, state)
        counts = _held_against_never_retiring(shape, a, previews, accums, state[:, 0], RSPP, noise=True)
    assert counts == [16, 48, 64]
    print("ragged frame, tile %d x %d: largest relative |map - restatement| with blocks retired at 16 and 48: %.3e" % (tile_w, tile_h, ledger.worst))
