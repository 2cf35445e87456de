"""CPU: the arithmetic of a frame that retires pixel blocks (ky_amd/csrc/ky_blocks.hpp; DESIGN.md "Adaptive") and what its entry points refuse before any device.
The header's functions run here as host code (kyhostcheck_blocks, ky_amd/csrc/ky_hostcheck.cpp) against the NumPy restatement of tests/blocks_restatement.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import blocks_restatement as B
import noise_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_blocks: the sanitizer build when the suite runs inside `make sanitize`, else the same sources built plainly."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    lib.kyhostcheck_blocks.restype, lib.kyhostcheck_blocks.argtypes = A.KYHOSTCHECK_SYMBOLS["kyhostcheck_blocks"]
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _geometry(check, p, n_pix):
    n_blocks = n_pix // 64
    block = np.full(n_pix, -1, np.int32)
    pixel = np.full((n_blocks, 64), -1, np.int32)
    inside = np.full(n_blocks, -1, np.int32)
    assert check.kyhostcheck_blocks(C.byref(p), _ptr(block), _ptr(pixel), _ptr(inside), None, 0, None, None, 0.0, 0.0, 2, 0, 0, None, 0, 0, 0, 0) == 0
    return block, pixel, inside


def _rule(check, p, state, values, cls, threshold, fraction, min_batches, front, batches, init=0):
    state = np.ascontiguousarray(state, np.int32).copy()
    values = np.ascontiguousarray(values, np.float32)
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8)
    assert check.kyhostcheck_blocks(C.byref(p), None, None, None, _ptr(state), init, _ptr(values), _ptr(cls), threshold, fraction, min_batches, front, batches,
                                    None, 0, 0, 0, 0) == 0
    return state


SHARD_1_3 = dict(tile_first=1, tile_step=3)
# (w, h, tile_w, tile_h, shard, n_tiles, n_inside): n_tiles and n_inside (blocks with a pixel inside the film) where the case pins them, else None
MAP_CASES = [(40, 24, 16, 16, {}, 6, 15), (40, 24, 16, 16, dict(tile_first=1, tile_step=2), 3, None), (40, 24, 32, 32, {}, 2, None)]
# tiles that are not square (blocks_w != tile_h / 8) and the tile that is one block (blocks_per_tile == 1), whole and as a shard
MAP_CASES += [(40, 24, tw, th, shard, None, None) for (tw, th) in ((32, 8), (8, 24), (8, 8)) for shard in ({}, SHARD_1_3)]
# films that are no multiple of 8: blocks partly inside
MAP_CASES += [(w, h, tw, th, shard, None, None) for (w, h) in ((44, 21), (33, 17)) for (tw, th) in ((16, 16), (32, 8), (8, 24), (8, 8)) for shard in ({}, SHARD_1_3)]
# the frame of tests/test_frame_sizes_gpu.py: 544 tiles, 2176 blocks = 8 groups of 256 and one of 128; as a shard 181 tiles
MAP_CASES += [(264, 512, 16, 16, {}, 544, 2112), (264, 512, 16, 16, SHARD_1_3, 181, None)]


def _case_id(c):
    w, h, tw, th, shard = c[:5]
    return "%dx%d_tile_%dx%d%s" % (w, h, tw, th, "_shard_%d_%d" % (shard["tile_first"], shard["tile_step"]) if shard else "")


# (the first three cases keep the ids they had before the others came: the same tests under the same names)
MAP_IDS = ["16-shard0-6-15", "16-shard1-3-None", "32-shard2-2-None"] + [_case_id(c) for c in MAP_CASES[3:]]


@pytest.mark.parametrize("w,h,tile_w,tile_h,shard,n_tiles,n_inside", MAP_CASES, ids=MAP_IDS)
def test_pixel_block_map(w, h, tile_w, tile_h, shard, n_tiles, n_inside, api, check):
    tile = dict(tile_w=tile_w, tile_h=tile_h)
    p = api.make_params(w, h, 500, **tile, **shard)
    tiles_film = -(-w // tile_w) * -(-h // tile_h)
    first, step = shard.get("tile_first", 0), shard.get("tile_step", 1)
    tiles_own = -(-(tiles_film - first) // step)
    if n_tiles is not None:
        assert tiles_own == n_tiles
    n_pix = tiles_own * tile_w * tile_h
    block, pixel, inside = _geometry(check, p, n_pix)
    assert np.array_equal(block, B.block_of_pixel(n_pix, **tile))
    assert np.array_equal(pixel, B.pixel_of_block(n_pix // 64, **tile))
    if tile_w == tile_h:   # `tile=` means a square tile
        assert np.array_equal(block, B.block_of_pixel(n_pix, tile_w)) and np.array_equal(pixel, B.pixel_of_block(n_pix // 64, tile_w))
    assert np.array_equal(block[pixel], np.repeat(np.arange(n_pix // 64)[:, None], 64, axis=1))      # the two are inverses
    assert np.array_equal(np.sort(pixel.ravel()), np.arange(n_pix))
    want_inside = B.inside_count(n_pix, w, h, **tile, **shard)
    assert np.array_equal(inside, want_inside)
    if n_inside is not None:
        assert len(inside) == {(40, 24): 24, (264, 512): 2176}[(w, h)] and int((inside > 0).sum()) == n_inside
    if (w, h) == (264, 512) and not shard:   # the padding blocks: two in each of the 32 tiles of the ragged right-hand column (264 = 16 * 16 + 8)
        assert int((inside == 0).sum()) == 64 and set(inside.tolist()) == {0, 64}
        assert np.array_equal(np.flatnonzero(inside == 0) % 2, np.tile([1, 1], 32)) and len(set(np.flatnonzero(inside == 0) // 4)) == 32
    if w % 8 or h % 8:
        assert ((inside > 0) & (inside < 64)).any()                                                   # a block partly inside the film
    # a block is an 8 x 8 square of the film: its pixels' coordinates span 8 columns and 8 rows from a multiple of 8
    x, y, in_film = R.pixel_xy(n_pix, w, h, **tile, **shard)
    bx, by = x[pixel], y[pixel]
    assert (bx.min(axis=1) % 8 == 0).all() and (by.min(axis=1) % 8 == 0).all()
    assert np.array_equal(bx - bx.min(axis=1, keepdims=True), np.tile(np.arange(64) % 8, (n_pix // 64, 1)))
    assert np.array_equal(by - by.min(axis=1, keepdims=True), np.tile(np.arange(64) // 8, (n_pix // 64, 1)))
    # every in-film pixel lies in exactly one block: no two compact pixels of the shard share a film pixel, and over the whole film every film pixel is hit
    hits = np.bincount((y * w + x)[in_film], minlength=w * h)
    assert hits.max() == 1 and (shard or hits.min() == 1)
    whole = B.inside_count(tiles_film * tile_w * tile_h, w, h, **tile)
    assert int(whole.sum()) == w * h                                                                  # the whole film's blocks hold every pixel once
    if shard:                                                                                         # ... and the shards of one step share them out
        parts = [B.inside_count(-(-(tiles_film - f) // step) * tile_w * tile_h, w, h, **tile, tile_first=f, tile_step=step) for f in range(step)]
        assert sum(int(part.sum()) for part in parts) == w * h
    # the mask of a set of blocks: their in-film pixels and nothing else
    some = list(range(0, n_pix // 64, 3))
    mask = B.keep_mask(some, n_pix, w, h, **tile, **shard)
    assert mask.dtype == np.uint8 and mask.shape == (h, w) and int(mask.sum()) == int(inside[some].sum())
    assert (mask[y[in_film], x[in_film]] == np.isin(block, some)[in_film]).all()


def test_sizes_and_schedule_the_gpu_tests_rely_on(api):
    """The figures tests/test_frame_sizes_gpu.py stands on, computed here: the 264 x 512 frame's blocks, compaction groups and noise partials, and the chunk
    schedule restated (B.chunk_ends, B.pass_plan) against kyhip_pass_boundaries."""
    n_pix = 544 * 256
    inside = B.inside_count(n_pix, 264, 512)
    assert (len(inside), int((inside > 0).sum()), int((inside == 0).sum())) == (2176, 2112, 64)
    assert -(-2176 // 256) == 9 and 2176 % 256 == 128                                   # the compaction: 8 groups of 256 blocks and one of 128
    partials = -(-n_pix // 256)
    per = -(-partials // 256)
    assert (partials, per, -(-partials // per), partials % per) == (544, 3, 182, 1)      # noise_final_kernel: three per thread, the 182nd thread has one
    assert -(-(181 * 256) // 256) == 181                                                 # the shard 1 of 3: one per thread, 75 threads idle
    for spp in (500, 512, 64, 25, 7, 1):
        assert B.chunk_ends(spp) == api.pass_boundaries(spp), spp
    plan = B.pass_plan(500, 100)
    assert [p[2] for p in plan] == [112, 224, 324, 428, 500] and [p[1] for p in plan] == [6, 7, 8, 13, 17] and [p[0] for p in plan] == [0, 6, 13, 21, 34]
    assert [p[2] for p in B.pass_plan(500, 1)] == B.chunk_ends(500) and B.pass_plan(500, 500) == [(0, 51, 500)]
    assert B.pass_plan(64, 16) == [(0, 4, 16), (4, 4, 32), (8, 4, 48), (12, 4, 64)]
    # 32 wavefronts x 256 CUs = 8192 slots: every render(100) pass of the whole frame, and of 1313 live blocks in pass 2, has more items
    assert min(2176 * p[1] for p in plan) > 8192 and 1313 * plan[1][1] > 8192


def test_retire_rule(api, check):
    w, h, n_pix = 40, 24, 6 * 256
    p = api.make_params(w, h, 500)
    _, pixel, inside = _geometry(check, p, n_pix)
    _, _, in_film = R.pixel_xy(n_pix, w, h)
    cls = np.where(in_film, 0, 2).astype(np.uint8)
    first = _rule(check, p, np.zeros((24, 2)), np.zeros(n_pix), cls, 0.5, 0.0, 2, 0, 0, init=1)[:, 0]
    assert np.array_equal(first, B.initial_state(inside)[:, 0]) and (first[inside == 0] == 0).all() and (first[inside > 0] == -1).all()   # all-padding blocks: retired at 0
    live = B.initial_state(inside)
    # +inf (before the second batch) never retires, whatever the fraction below 1
    got = _rule(check, p, live, np.full(n_pix, np.inf), cls, 1e30, 0.99, 2, 112, 5)
    assert np.array_equal(got, live)
    # ... nor anything before min_batches
    got = _rule(check, p, live, np.zeros(n_pix), cls, 0.5, 1.0, 3, 48, 2)
    assert np.array_equal(got, live)
    got = _rule(check, p, live, np.zeros(n_pix), cls, 0.5, 0.0, 3, 64, 3)
    assert (got[inside > 0] == (64, 3)).all() and np.array_equal(got[inside == 0], live[inside == 0])   # retired blocks stay what they were
    # a flagged pixel holds nothing back: block 0 is clean but for one pixel, noisy or flagged
    values = np.zeros(n_pix, np.float32)
    values[pixel[0, 9]] = 7.0
    values[pixel[1]] = 7.0
    noisy = _rule(check, p, live, values, cls, 0.5, 0.0, 2, 112, 4)
    assert noisy[0, 0] == -1 and noisy[1, 0] == -1 and noisy[2, 0] == 112
    flagged = cls.copy()
    flagged[pixel[0, 9]] = 1
    flagged[pixel[1]] = 1                 # every pixel of block 1 flagged: nothing counted, nothing above
    got = _rule(check, p, live, values, flagged, 0.5, 0.0, 2, 112, 4)
    assert tuple(got[0]) == (112, 4) and tuple(got[1]) == (112, 4)
    # the fraction comparison at equality: 16 of a full block's 64 above with fraction 0.25 retires, 17 does not; a 37 x 21 film has ragged blocks (5 x 8 pixels
    # inside on the right edge): there 10 of 40 retire and 11 do not
    for (fw, fh, want_n) in ((w, h, 64), (37, 21, 40)):
        q = api.make_params(fw, fh, 500)
        _, qpixel, qinside = _geometry(check, q, n_pix)
        _, _, q_in = R.pixel_xy(n_pix, fw, fh)
        qcls = np.where(q_in, 0, 2).astype(np.uint8)
        qlive = B.initial_state(qinside)
        block = int(np.flatnonzero(qinside == want_n)[1])
        inside_lanes = np.flatnonzero(q_in[qpixel[block]])
        assert len(inside_lanes) == want_n
        for above, retires in ((want_n // 4, True), (want_n // 4 + 1, False)):
            values = np.zeros(n_pix, np.float32)
            values[qpixel[block, inside_lanes[:above]]] = 1.0
            values[~q_in] = 9.0           # padding counts nowhere
            got = _rule(check, q, qlive, values, qcls, 0.5, 0.25, 2, 224, 2)
            assert (got[block, 0] == 224) == retires
            assert np.array_equal(got, B.retire(qlive, values, qcls == 0, 0.5, 0.25, 2, 224, 2))
    # `counted`, not 64, is what the fraction multiplies: a 44 x 21 film's corner block has 4 x 5 pixels inside.  With fraction 0.10, 0.10 * 20 = 2 lets two pixels
    # lie above and not three, where 0.10 * 64 = 6.4 would let six: three above keep the corner block live and retire a whole block of the same film.
    q = api.make_params(44, 21, 500)
    _, qpixel, qinside = _geometry(check, q, n_pix)
    _, _, q_in = R.pixel_xy(n_pix, 44, 21)
    qcls = np.where(q_in, 0, 2).astype(np.uint8)
    qlive = B.initial_state(qinside)
    corner, whole = int(np.flatnonzero(qinside == 20)[0]), int(np.flatnonzero(qinside == 64)[0])
    assert sorted(set(qinside.tolist())) == [0, 20, 32, 40, 64] and (qinside == 20).sum() == 1
    for above, corner_retires in ((2, True), (3, False)):
        assert (above <= float(np.float32(0.10)) * 20.0) == corner_retires and above <= float(np.float32(0.10)) * 64.0
        values = np.zeros(n_pix, np.float32)
        for block in (corner, whole):
            values[qpixel[block, np.flatnonzero(q_in[qpixel[block]])[:above]]] = 1.0
        values[~q_in] = 9.0
        got = _rule(check, q, qlive, values, qcls, 0.5, 0.10, 2, 224, 2)
        assert (got[corner, 0] == 224) == corner_retires and got[whole, 0] == 224
        assert np.array_equal(got, B.retire(qlive, values, qcls == 0, 0.5, 0.10, 2, 224, 2))
    # the threshold itself is not above it
    values = np.full(n_pix, np.float32(0.008), np.float32)
    assert (_rule(check, p, live, values, cls, 0.008, 0.0, 2, 24, 2)[inside > 0, 0] == 24).all()
    # random maps against the restatement
    rng = np.random.default_rng(5)
    for fraction in (0.0, 0.1, 0.5, 1.0):
        values = rng.uniform(0, 0.02, n_pix).astype(np.float32)
        c = np.where(in_film, (rng.uniform(size=n_pix) < 0.05).astype(np.uint8), 2).astype(np.uint8)
        got = _rule(check, p, live, values, c, 0.01, fraction, 3, 308, 3)
        assert np.array_equal(got, B.retire(live, values, c == 0, 0.01, fraction, 3, 308, 3))


def test_trailer_refusals(A, api, check):
    p = api.make_params(40, 24, 500)
    n_blocks, offset, done = 24, 200, 224
    def state(magic=B.BLOCKS_MAGIC, n=n_blocks, pairs=None, cut=0, passes=2):
        pairs = np.array([(-1, 0)] * n_blocks if pairs is None else pairs, np.int32)
        s = bytes(offset) + struct.pack("<Qii", magic, n, passes) + pairs.tobytes()
        return s[:len(s) - cut]
    def rc(s, samples_done=done, noise_batches=2):
        return check.kyhostcheck_blocks(C.byref(p), None, None, None, None, 0, None, None, 0.0, 0.0, 2, 0, 0, s, len(s), offset, samples_done, noise_batches)
    def one(value, batches=2):
        return [(value, batches)] + [(-1, 0)] * (n_blocks - 1)
    assert rc(state()) == A.KY_OK
    assert rc(state() + b"xx") == A.KY_OK
    for good in (24, 112, 224):                         # values of kyhip_pass_boundaries(500) up to the header's samples done
        assert rc(state(pairs=one(good))) == A.KY_OK
        assert rc(state(pairs=one(good, batches=0))) == A.KY_OK and rc(state(pairs=one(good, batches=1))) == A.KY_OK
    assert rc(state(pairs=one(0, batches=0))) == A.KY_OK                    # ... and 0, where nothing was rendered: no batch either
    assert rc(state(pairs=one(112, batches=0)), noise_batches=0) == A.KY_OK   # a frame that tracks no noise: every count is 0
    bad = [state(cut=1), state(cut=8 * n_blocks), state()[:offset], state()[:offset - 8], state(magic=B.BLOCKS_MAGIC ^ 1), state(magic=R.NOISE_MAGIC),
           state(n=n_blocks - 1), state(n=n_blocks + 1),
           state(pairs=one(101)), state(pairs=one(1)), state(pairs=one(-2)),       # no pass ends there
           state(pairs=one(308)), state(pairs=one(500)),                            # beyond the header's samples done
           state(pairs=one(112, batches=-1)), state(passes=-1),
           state(pairs=one(112, batches=3)),                                        # more batches than the noise estimate has
           state(pairs=one(0, batches=1)), state(pairs=one(-1, batches=1))]         # batches on a block nothing was rendered of, and on a live one
    for s in bad:
        assert rc(s) == A.KY_ERR_INVALID_VALUE
    assert rc(state(pairs=one(224)), samples_done=112) == A.KY_ERR_INVALID_VALUE
    assert rc(state(pairs=one(112, batches=1)), noise_batches=0) == A.KY_ERR_INVALID_VALUE


def test_arguments_are_refused_before_any_device(A):
    lib = A.load_kyhip()
    st = A.BlockStats()
    done = C.c_int(-7)
    mask = (C.c_ubyte * 4)()
    buf = (C.c_int32 * 4)()
    E = A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_frame_track_blocks(None) == E and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_keep(None, mask, 2) == E and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_keep(None, None, 2) == E and b"mask is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_sample_map(None, buf, 2) == E and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_block_stats(None, C.byref(st)) == E and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_block_stats(None, None) == E and b"out is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_retire_noisy(None, 0.01, 0.1, 3, C.byref(st)) == E and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_retire_noisy(None, 0.01, 0.1, 3, None) == E and b"out is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_render_adaptive(None, 0.01, 0.1, 3, 100, C.byref(done), C.byref(st)) == E and b"frame is NULL" in lib.kyhip_last_error()
    assert lib.kyhip_frame_render_adaptive(None, 0.01, 0.1, 3, 100, C.byref(done), None) == E and b"out is NULL" in lib.kyhip_last_error()
    for threshold in (-1.0, -1e-30, float("nan")):
        assert lib.kyhip_frame_retire_noisy(None, threshold, 0.1, 3, C.byref(st)) == E and b"threshold" in lib.kyhip_last_error()
        assert lib.kyhip_frame_render_adaptive(None, threshold, 0.1, 3, 100, None, C.byref(st)) == E and b"threshold" in lib.kyhip_last_error()
    for fraction in (-0.01, 1.5, float("nan")):
        assert lib.kyhip_frame_retire_noisy(None, 0.01, fraction, 3, C.byref(st)) == E and b"max_fraction_above" in lib.kyhip_last_error()
        assert lib.kyhip_frame_render_adaptive(None, 0.01, fraction, 3, 100, None, C.byref(st)) == E and b"max_fraction_above" in lib.kyhip_last_error()
    for min_batches in (1, 0, -3):
        assert lib.kyhip_frame_retire_noisy(None, 0.01, 0.1, min_batches, C.byref(st)) == E and b"min_batches" in lib.kyhip_last_error()
        assert lib.kyhip_frame_render_adaptive(None, 0.01, 0.1, min_batches, 100, None, C.byref(st)) == E and b"min_batches" in lib.kyhip_last_error()
    assert lib.kyhip_frame_render_adaptive(None, 0.01, 0.1, 3, 0, None, C.byref(st)) == E and b"min_samples_per_pass" in lib.kyhip_last_error()
    assert done.value == -7


def test_stats_struct_layout(A, tmp_path):
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "kyhip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(ky_block_stats), ' \
           'offsetof(ky_block_stats, passes), offsetof(ky_block_stats, max_samples), offsetof(ky_block_stats, pixel_samples));return 0;}'
    (tmp_path / "sz.c").write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "sz.c"), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    assert got == [C.sizeof(A.BlockStats), A.BlockStats.passes.offset, A.BlockStats.max_samples.offset, A.BlockStats.pixel_samples.offset]
