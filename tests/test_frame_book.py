"""CPU: whole life cycles of a frame's bookkeeping without a device.  FrameBook (ky_amd/csrc/ky_frame_book.hpp) is everything a kyhip_frame is apart from its device
memory; kyhip_frame_*'s entries ask it and commit to it around their device work (ky_amd/csrc/ky_frame.cpp), and kyhostcheck_book (ky_amd/csrc/ky_hostcheck.cpp) asks
and commits with no device work in between, on up to five books and four state slots.  The frame is the suite's small ragged one: 40 x 24 in tiles of 16, 500 samples,
whose pass boundaries are derived by hand in tests/test_frame.py.  (kyhip_frame_keep has no operation here: the rule of the keep kernel is no function of
ky_blocks.hpp that a host could call, so blocks never retire in these scripts; tests/test_blocks_gpu.py covers keep on the device.)"""
import itertools

import numpy as np
import pytest

from frame_book_script import (INVALID, LOAD, MERGE, MERGE_FROM, NOTHING, OK, PASS, SAVE, TRACK_BLOCKS, TRACK_NOISE, load_book_library, run_book, state_of)

W, H, SPP = 40, 24, 500
SHARDS = [{}, dict(tile_first=1, tile_step=2), dict(tile_first=6)]   # whole, every second tile, none (tests/test_frame.py: test_checkpoint_round_trip)
SLICES = [(0, 48), (48, 308), (308, 500)]


@pytest.fixture(scope="module")
def check(A):
    return load_book_library(A)


@pytest.mark.parametrize("shard", SHARDS, ids=["whole", "every-second-tile", "no-tiles"])
@pytest.mark.parametrize("min_samples", [1, 7, 100, 500])
def test_passes(min_samples, shard, api, check):
    p = api.make_params(W, H, SPP, **shard)
    bounds = api.pass_boundaries(SPP)
    records, _ = run_book(check, p, [(0, SPP)], [(TRACK_NOISE, 0)] + [(PASS, 0, min_samples)] * 55)
    assert all(r["status"] == OK for r in records)
    fronts = [r["front"] for r in records]
    advanced = [b for a, b in zip(fronts, fronts[1:]) if b != a]
    assert fronts[0] == 0 and advanced == sorted(set(advanced)) and set(advanced) <= set(bounds) and advanced[-1] == SPP and fronts[-1] == SPP
    steps = [b - a for a, b in zip([0] + advanced, advanced)]
    assert all(s >= min_samples for s in steps[:-1])
    if min_samples == 1:
        assert advanced == bounds and len(advanced) == 51
    if min_samples == SPP:
        assert advanced == [SPP]
    n = 0
    for before, r in zip(records, records[1:]):
        n += r["front"] != before["front"]
        assert r["batches"] == n and r["n_prev"] == r["held"] == r["front"]
        assert r["ranges"] == ([(0, r["front"])] if r["front"] else []) and (r["own_first"], r["own_end"]) == (0, SPP)
    assert state_of(records[-1]) == state_of(records[len(advanced)])   # a pass on a complete frame: nothing moves


def render_slices(noise=True):
    """three slices and a collector (book 3), each rendered to its end in passes of at least 100 and saved into the slot of its number"""
    ops = [(TRACK_NOISE, b) for b in range(4)] if noise else []
    for b in range(4):
        ops += [(PASS, b, 100)] * 4 + [(SAVE, b, b)]
    return ops


def test_slices(api, check):
    p = api.make_params(W, H, SPP)
    books = SLICES + [(0, 0)]
    ops = render_slices()
    base, slots = run_book(check, p, books, ops)
    assert all(r["status"] == OK for r in base)
    last = {op[1]: r for op, r in zip(ops, base)}   # each book's record behind its save
    assert [last[b]["held"] for b in range(4)] == [48, 260, 192, 0] and [last[b]["front"] for b in range(4)] == [48, 308, 500, 0]
    assert [last[b]["ranges"] for b in range(4)] == [[(0, 48)], [(48, 308)], [(308, 500)], []]
    assert [(last[b]["own_first"], last[b]["own_end"]) for b in range(4)] == books
    assert last[3]["batches"] == 0 and all(last[b]["batches"] >= 1 and last[b]["n_prev"] == last[b]["held"] for b in range(3))
    assert len({len(s) for s in slots}) == 1 and all(last[b]["state_bytes"] == len(slots[0]) for b in range(4))   # all slices of a frame: states of one size
    # every pass of a slice ends on a boundary of the whole frame and inside its owned range
    bounds = set(api.pass_boundaries(SPP))
    for op, r in zip(ops, base):
        assert r["front"] in bounds | {0} and r["own_first"] <= r["front"] <= r["own_end"]
    total = sum(last[b]["batches"] for b in range(3))
    for order in itertools.permutations(range(3)):
        records, _ = run_book(check, p, books, ops + [(MERGE, 3, s) for s in order])
        merged = records[len(ops):]
        assert all(r["status"] == OK for r in merged)
        assert merged[-1]["ranges"] == [(0, SPP)] and merged[-1]["held"] == SPP and merged[-1]["batches"] == total and merged[-1]["n_prev"] == SPP
        assert merged[-1]["front"] == 0                               # a collector's front never moves: what it holds is merged
        assert [r["held"] for r in merged] == list(np.cumsum([last[s]["held"] for s in order]))
        if order[:2] in ((0, 2), (2, 0)):
            assert merged[1]["ranges"] == [(0, 48), (308, 500)] and merged[1]["n_ranges"] == 2 and merged[1]["held"] == 240
    # from another book instead of its saved state: the same record
    records, _ = run_book(check, p, books, ops + [(MERGE_FROM, 3, s) for s in (2, 0, 1)])
    by_state, _ = run_book(check, p, books, ops + [(MERGE, 3, s) for s in (2, 0, 1)])
    assert records[len(ops):] == by_state[len(ops):]


FRESH, RENDERED = [(0, SPP)], [(PASS, 0, 24)]
REFUSALS = {
    "min_samples 0": (FRESH, [], (PASS, 0, 0), b"a pass renders at least one sample per pixel"),
    "noise after a pass": (FRESH, RENDERED, (TRACK_NOISE, 0), b"noise is tracked from a frame's first pass"),
    "blocks after a pass": (FRESH, RENDERED, (TRACK_BLOCKS, 0), b"blocks are tracked from a frame's first pass"),
    "noise after a load": (FRESH * 2, [(SAVE, 1, 0), (LOAD, 0, 0)], (TRACK_NOISE, 0), b"noise is tracked from a frame's first pass"),
    "blocks after a load": (FRESH * 2, [(SAVE, 1, 0), (LOAD, 0, 0)], (TRACK_BLOCKS, 0), b"blocks are tracked from a frame's first pass"),
    "noise after a merge": ([(0, 0), (0, 48)], [(PASS, 1, 48), (SAVE, 1, 0), (MERGE, 0, 0)], (TRACK_NOISE, 0), b"noise is tracked from a frame's first pass"),
    "blocks after a merge": ([(0, 0), (0, 48)], [(PASS, 1, 48), (SAVE, 1, 0), (MERGE, 0, 0)], (TRACK_BLOCKS, 0), b"blocks retire on a frame that owns them all"),
    "blocks on a slice": ([(48, 308)], [], (TRACK_BLOCKS, 0), b"the frame owns samples 48..308 of 500"),
    "merge into an owner of all": ([(0, SPP), (0, 48)], [(PASS, 1, 48), (SAVE, 1, 0)], (MERGE, 0, 0), b"the receiving frame owns all 500 samples"),
    "merge from a book into an owner of all": ([(0, SPP), (0, 48)], [(PASS, 1, 48)], (MERGE_FROM, 0, 1), b"the receiving frame owns all 500 samples"),
    "merge of an owned range": ([(0, 308), (0, 48)], [(PASS, 1, 48), (SAVE, 1, 0)], (MERGE, 0, 0), b"would count them twice"),
    "merge of a held range": ([(0, 0), (0, 48)], [(PASS, 1, 48), (SAVE, 1, 0), (MERGE, 0, 0)], (MERGE, 0, 0), b"are held twice"),
    "merge of itself": ([(0, 48)], [(PASS, 0, 48)], (MERGE_FROM, 0, 0), b"a frame holds its own samples already"),
    "merge without a noise trailer": ([(0, 0), (0, 48)], [(TRACK_NOISE, 0), (PASS, 1, 48), (SAVE, 1, 0)], (MERGE, 0, 0), b"the state carries no valid noise trailer"),
    "load one byte short": (FRESH * 2, [(PASS, 1, 24), (SAVE, 1, 0)], (LOAD, 0, 0, 1), b"the frame's state has"),
    "load of a slice one byte short": ([(48, 308)] * 2, [(PASS, 1, 24), (SAVE, 1, 0)], (LOAD, 0, 0, 1), b"hold no slice trailer"),
    "load of another slice's state": ([(48, 308), (0, 48)], [(PASS, 1, 24), (SAVE, 1, 0)], (LOAD, 0, 0), b"saved by the slice of samples 0..48, this frame owns 48..308"),
    "load of a blocks frame's state": (FRESH * 2, [(TRACK_BLOCKS, 1), (PASS, 1, 24), (SAVE, 1, 0)], (LOAD, 0, 0), b"saved by a frame that retires pixel blocks, this one does neither"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_leave_the_book_as_it_was(case, api, check):
    books, before, refused, message = REFUSALS[case]
    p = api.make_params(W, H, SPP)
    records, _ = run_book(check, p, books, before + [(NOTHING, refused[1]), refused])
    assert all(r["status"] == OK for r in records[:-1]), case
    assert records[-1]["status"] == INVALID and message in check.kyhip_last_error(), (case, check.kyhip_last_error())
    assert state_of(records[-1]) == state_of(records[-2])
    # ... and goes on as a book that was never asked: the same passes as one without the refused operation
    tail = [(PASS, refused[1], 100)] * 3
    with_refusal, _ = run_book(check, p, books, before + [refused] + tail)
    without, _ = run_book(check, p, books, before + tail)
    assert with_refusal[-3:] == without[-3:]


@pytest.mark.parametrize("shard", SHARDS[:2], ids=["whole", "every-second-tile"])
@pytest.mark.parametrize("own,noise,blocks", [((0, SPP), False, False), ((0, SPP), True, False), ((0, SPP), False, True), ((0, SPP), True, True),
                                              ((48, 308), False, False), ((48, 308), True, False)])
def test_save_and_load(own, noise, blocks, shard, api, check):
    """At every fifth boundary: what one book saves, a fresh book of the same description loads, and the two go on alike to the end."""
    p = api.make_params(W, H, SPP, **shard)
    bounds = [b for b in api.pass_boundaries(SPP) if own[0] < b <= own[1]]
    track = [(op, b) for b in (0, 1) for op, on in ((TRACK_NOISE, noise), (TRACK_BLOCKS, blocks)) if on]
    for k in range(5, len(bounds) + 1, 5):
        ops = track + [(PASS, 0, 1)] * k + [(SAVE, 0, 2), (LOAD, 1, 2), (NOTHING, 0)]
        rest = len(bounds) - k + 1
        ops += [(PASS, 0, 1), (PASS, 1, 1)] * rest
        records, slots = run_book(check, p, [own, own], ops)
        assert all(r["status"] == OK for r in records)
        at = len(track) + k
        saved, loaded, original = records[at], records[at + 1], records[at + 2]
        assert saved["front"] == bounds[k - 1] and saved["held"] == bounds[k - 1] - own[0] and len(slots[2]) == saved["state_bytes"]
        assert state_of(loaded) == state_of(saved) == state_of(original)
        assert loaded["batches"] == (k if noise else 0) and loaded["passes"] == (k if blocks else 0)
        # the ragged frame: 5 x 3 of a whole shard's 6 x 4 blocks have a pixel inside; tiles 1, 3 and 5 lie at (column, row) (1, 0), (1, 1) and (0, 1) -- a tile row's
        # columns are rotated by its number (noise_pixel_xy, ky_noise.hpp) --, which have 4 + 2 + 2.  Nothing retires without a device.
        if blocks:
            assert loaded["n_live"] == (8 if shard else 15)
        following = records[at + 3:]
        for a, b in zip(following[0::2], following[1::2]):
            assert state_of(a) == state_of(b)
        assert following[-1]["front"] == own[1] and following[-1]["held"] == own[1] - own[0]
        assert state_of(following[-1]) == state_of(following[-3])     # the pass behind the last one moved nothing
