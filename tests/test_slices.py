"""CPU: slices of a frame's samples (include/kyhip.h "Slices"; DESIGN.md "Slices") without a device -- where a frame is cut (kyhip_slice_bounds), the union of
sample ranges and what it refuses, the slice trailer of a checkpoint and what a load refuses of it, and a merge's arithmetic (ky_amd/csrc/ky_noise.hpp: merge_pixel,
noise_merge) against the NumPy restatement of tests/slices_restatement.py, bit for bit.  The headers' functions run as host code through kyhostcheck_slices and
kyhostcheck_merge (ky_amd/csrc/ky_hostcheck.cpp: the file the sanitizer builds hold too).  dist.gather_states runs over gloo."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed as tdist
import torch.multiprocessing as mp

import noise_restatement as R
import slices_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, LIMIT = 0, -1, -2
W, H = 40, 24


@pytest.fixture(scope="module")
def check(A):
    """The library that holds kyhostcheck_slices and kyhostcheck_merge: the sanitizer build inside `make sanitize`, else the same sources built plainly."""
    if A.SANITIZE:
        return A.load_kyhip()
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    for name in ("kyhostcheck_slices", "kyhostcheck_merge", "kyhostcheck_noise"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = A.KYHOSTCHECK_SYMBOLS[name]
    return lib


def _ints(values):
    return np.ascontiguousarray(np.asarray(values, np.int32).ravel())


def _bounds(check, spp, n):
    out = np.full(max(n, 0) + 1, -7, np.int32)
    return check.kyhostcheck_slices(0, None, None, spp, None, n, out.ctypes.data, None, None, 0, None), [int(v) for v in out]


@pytest.mark.parametrize("spp", [7, 48, 500, 1024])
def test_slice_bounds(spp, api, check):
    boundaries = api.pass_boundaries(spp)
    for n in range(1, len(boundaries) + 1):
        rc, b = _bounds(check, spp, n)
        assert rc == OK and len(b) == n + 1 and b[0] == 0 and b[-1] == spp
        assert set(b[1:]) <= set(boundaries) and all(x < y for x, y in zip(b, b[1:])), (spp, n, b)
    assert _bounds(check, spp, len(boundaries) + 1)[0] == INVALID
    assert _bounds(check, spp, 0)[0] == INVALID
    assert _bounds(check, spp, len(boundaries))[1] == [0] + boundaries   # as many slices as chunks: one chunk each


def test_slice_bounds_pinned(api, check):
    """500 / 3: 166.67 lies between the 16-sample chunk ends 160 and 176 (48 + 16 j), nearer to 160; 333.33 between the 8-sample chunk ends 332 and 340 (308 + 8 j),
    nearer to 332.  7 / 2: 3.5 is nearest to the chunk end 4 (the other is 7).  48 / 2: 24 is a chunk end."""
    assert {160, 176, 332, 340} <= set(api.pass_boundaries(500)) and api.pass_boundaries(7) == [4, 7]
    assert _bounds(check, 500, 3) == (OK, [0, 160, 332, 500])
    assert _bounds(check, 7, 2) == (OK, [0, 4, 7])
    assert _bounds(check, 48, 2) == (OK, [0, 24, 48])
    assert _bounds(check, 0, 1)[0] == INVALID and _bounds(check, (1 << 24) + 1, 1)[0] == INVALID
    # a tie goes to the lower boundary: 48 samples are twelve chunks of 4; in 8 slices 6 lies midway between 4 and 8, 18 between 16 and 20, 30 and 42 likewise
    assert api.pass_boundaries(48) == list(range(4, 49, 4))
    assert _bounds(check, 48, 8) == (OK, [0, 4, 12, 16, 24, 28, 36, 40, 48])
    assert api.slice_bounds(500, 3) == [0, 160, 332, 500]   # the product library's entry


def _union(check, a, b):
    out, counts = np.zeros(4 * S.MAX_RANGES + 4, np.int32), np.zeros(8, np.int32)
    ia, ib = _ints(a), _ints(b)
    rc = check.kyhostcheck_slices(1, None, ia.ctypes.data, len(a), ib.ctypes.data, len(b), out.ctypes.data, counts.ctypes.data, None, 0, None)
    n = int(counts[0])
    return rc, [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)] if rc == OK else None


def test_coverage_union(check):
    assert _union(check, [(0, 48)], [(48, 160)]) == (OK, [(0, 160)])                      # adjacent ranges join
    assert _union(check, [(48, 160)], [(0, 48)]) == (OK, [(0, 160)])
    assert _union(check, [(0, 48), (160, 224)], [(48, 160), (332, 500)]) == (OK, [(0, 224), (332, 500)])
    assert _union(check, [], [(4, 7)]) == (OK, [(4, 7)]) and _union(check, [], []) == (OK, [])
    for a, b in (([(0, 48)], [(24, 64)]), ([(0, 48)], [(0, 48)]), ([(24, 64)], [(0, 48)]), ([(0, 500)], [(160, 164)]), ([(0, 48), (24, 64)], [])):
        assert _union(check, a, b)[0] == INVALID, (a, b)                                    # overlaps are refused
    # order independence: every way of dealing these ranges to the two sides, in either order, gives one union
    ranges = [(0, 24), (24, 48), (64, 80), (112, 224), (308, 316), (436, 440), (496, 500)]
    want = [(0, 48), (64, 80), (112, 224), (308, 316), (436, 440), (496, 500)]
    rng = np.random.default_rng(3)
    for _ in range(20):
        order = rng.permutation(len(ranges))
        k = int(rng.integers(0, len(ranges) + 1))
        a, b = [ranges[i] for i in order[:k]], [ranges[i] for i in order[k:]]
        assert _union(check, a, b) == (OK, want) and _union(check, b, a) == (OK, want)
    # 32 ranges are held, a 33rd is KY_ERR_LIMIT, and a range that joins two of the 32 is still accepted
    many = [(4 * i, 4 * i + 2) for i in range(S.MAX_RANGES)]
    assert _union(check, many[:20], many[20:]) == (OK, many)
    assert _union(check, many, [(1000, 1004)])[0] == LIMIT
    assert _union(check, many[:16] + [(1000, 1004)], many[16:])[0] == LIMIT
    rc, got = _union(check, many, [(2, 4)])
    assert rc == OK and got == [(0, 6)] + many[2:]


OWN, FRONT, COVER = (160, 332), 224, [(0, 48), (160, 224), (436, 500)]   # a slice of the 500-sample frame, partly rendered, that has received two other ranges
HELD = 48 + 64 + 64
SAMPLES_DONE_AT, SEED_AT = R.HEADER_BYTES - 8, 16 + 5 * 4   # FrameHeader: magic, source hash, the twelve params (the seed is the sixth), scene hash, samples_done, n_pix


def _trailer_state(A, api, check, noise, own=OWN, front=FRONT, cover=COVER, batches=3):
    """(the host-side parts of such a slice's checkpoint as a bytearray, where its slice trailer begins, where its noise trailer does)"""
    p = api.make_params(W, H, 500)
    a, b, extra = _ints([own[0], own[1], front]), _ints(cover), _ints([int(noise), batches])
    out, counts = np.zeros(2 * S.MAX_RANGES, np.int32), np.zeros(8, np.int32)
    dummy = C.create_string_buffer(16)
    assert check.kyhostcheck_slices(2, C.byref(p), a.ctypes.data, 3, b.ctypes.data, len(cover), out.ctypes.data, counts.ctypes.data, dummy, 0, extra.ctypes.data) == OK
    total, at_slice, at_noise = (int(v) for v in counts[:3])
    buf = C.create_string_buffer(total)
    assert check.kyhostcheck_slices(2, C.byref(p), a.ctypes.data, 3, b.ctypes.data, len(cover), out.ctypes.data, counts.ctypes.data, buf, total, extra.ctypes.data) == OK
    return bytearray(buf.raw), at_slice, at_noise


def _trailer_check(A, api, check, state, noise, own=OWN):
    p = api.make_params(W, H, 500)
    a, extra = _ints([own[0], own[1]]), _ints([int(noise), 0])
    out, counts = np.zeros(2 * S.MAX_RANGES, np.int32), np.zeros(8, np.int32)
    buf = (C.c_char * len(state)).from_buffer_copy(bytes(state))
    rc = check.kyhostcheck_slices(3, C.byref(p), a.ctypes.data, 2, None, 0, out.ctypes.data, counts.ctypes.data, buf, len(state), extra.ctypes.data)
    n = int(counts[5])
    return rc, [int(v) for v in counts[:5]], [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
def test_slice_trailer_round_trip(noise, A, api, check):
    state, at_slice, at_noise = _trailer_state(A, api, check, noise)
    n_pix = 3 * 2 * 256
    assert at_noise == R.HEADER_BYTES + n_pix * 28 and at_slice == at_noise + (16 + n_pix * 16 if noise else 0) and len(state) == at_slice + S.SLICE_TRAILER_BYTES
    held, _, _, trailer, (first, end, front, ranges) = S.split_slice_state(bytes(state), n_pix)
    assert (held, first, end, front, ranges) == (HELD, OWN[0], OWN[1], FRONT, COVER) and (trailer is not None) == noise
    rc, counts, ranges = _trailer_check(A, api, check, state, noise)
    chunks_at_224 = api.pass_boundaries(500).index(224) + 1
    assert rc == OK and counts == [chunks_at_224, HELD, 3 if noise else 0, HELD if noise else 0, FRONT] and ranges == COVER
    # every slice of the frame has a state of this size, whatever it holds: a collector, an untouched slice, a full coverage
    for own, front, cover in (((0, 0), 0, []), ((0, 160), 0, []), ((0, 160), 160, [(0, 500)])):
        other, _, _ = _trailer_state(A, api, check, noise, own, front, cover)
        assert len(other) == len(state)
        assert _trailer_check(A, api, check, other, noise, own)[0] == OK
    # a longer buffer is accepted, a shorter one refused; a tracking frame refuses the state of one that does not track
    assert _trailer_check(A, api, check, state + b"\0" * 8, noise)[0] == OK
    assert _trailer_check(A, api, check, state[:-1], noise)[0] == INVALID
    if not noise:
        assert _trailer_check(A, api, check, state, True)[0] == INVALID


def _patched(state, at, fmt, *values):
    out = bytearray(state)
    struct.pack_into(fmt, out, at, *values)
    return out


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
def test_slice_trailer_refusals(noise, A, api, check):
    """One field at a time.  The trailer: magic (8), own_first, own_end, front, n_ranges, then the ranges."""
    state, at, at_noise = _trailer_state(A, api, check, noise)
    refused = lambda s, own=OWN: _trailer_check(A, api, check, s, noise, own)[0] == INVALID
    assert _trailer_check(A, api, check, state, noise)[0] == OK
    assert refused(state, (160, 340)) and refused(state, (48, 332)) and refused(state, (0, 500))      # another owned range (the last: a plain frame, another magic)
    assert refused(_patched(state, at + 8, "<ii", 160, 340))                                           # ... in the trailer
    assert refused(_patched(state, at + 8, "<ii", 160, 333))                                           # an owned range off the boundaries
    assert refused(_patched(state, at, "<Q", S.SLICE_MAGIC ^ 1)) and refused(_patched(state, 0, "<Q", R.NOISE_MAGIC))
    plain_magic, = struct.unpack_from("<Q", bytes(_trailer_state(A, api, check, noise, (0, 500), 0, [])[0]), 0)
    assert plain_magic != S.SLICE_FRAME_MAGIC and refused(_patched(state, 0, "<Q", plain_magic))      # a plain frame's header on a slice's state
    for front in (144, 340, 230, -1):                                                                  # a front before, behind the owned range, on no boundary
        assert refused(_patched(state, at + 16, "<i", front)), front
    assert refused(_patched(state, at + 16, "<i", 240))                                                # a boundary inside, but the coverage says 160..224
    assert refused(_patched(state, at + 20, "<i", 33)) and refused(_patched(state, at + 20, "<i", -1)) and refused(_patched(state, at + 20, "<i", 2))
    ranges = at + 24
    assert refused(_patched(state, ranges, "<4i", 160, 224, 0, 48))                                    # not ascending
    assert refused(_patched(state, ranges, "<4i", 0, 176, 160, 224))                                   # not disjoint
    assert refused(_patched(state, ranges, "<2i", 0, 50))                                              # not on a boundary
    assert refused(_patched(state, ranges, "<2i", 48, 48)) and refused(_patched(state, ranges, "<2i", 64, 48))
    assert refused(_patched(_patched(state, ranges, "<4i", 0, 160, 160, 224), SAMPLES_DONE_AT, "<i", HELD + 112))   # adjacent ranges that are not joined
    assert refused(_patched(_patched(state, ranges + 8, "<2i", 176, 224), SAMPLES_DONE_AT, "<i", HELD - 16))        # inside the owned range: not from its first sample
    assert refused(_patched(_patched(state, ranges + 16, "<2i", 308, 500), SAMPLES_DONE_AT, "<i", HELD + 128))      # another frame's range reaches into the owned one
    assert refused(_patched(_patched(_patched(state, ranges + 8, "<2i", 436, 500), at + 20, "<i", 2), SAMPLES_DONE_AT, "<i", HELD - 64))   # nothing of the owned range held
    assert struct.unpack_from("<i", bytes(state), SAMPLES_DONE_AT)[0] == HELD
    assert refused(_patched(state, SAMPLES_DONE_AT, "<i", HELD + 16)) and refused(_patched(state, SAMPLES_DONE_AT, "<i", 0))   # a held count that disagrees with the header
    if noise:
        assert refused(_patched(state, at_noise + 12, "<i", HELD - 16))                                # ... with the noise trailer's n_prev
        assert refused(_patched(state, at_noise + 8, "<i", -1))


def _merge_state(A, api, check, state, own, mine, tracks_noise=False, tracks_blocks=False):
    """merge_source_check + merge_accept of a saved state by a frame of the 500-sample params that owns `own` and holds `mine`: (status, the union)."""
    p = api.make_params(W, H, 500)
    a, b, extra = _ints(own), _ints(mine), _ints([int(tracks_noise), int(tracks_blocks)])
    out, counts = np.zeros(4 * S.MAX_RANGES, np.int32), np.zeros(8, np.int32)
    buf = (C.c_char * len(state)).from_buffer_copy(bytes(state))
    rc = check.kyhostcheck_slices(4, C.byref(p), a.ctypes.data, 2, b.ctypes.data, len(mine), out.ctypes.data, counts.ctypes.data, buf, len(state), extra.ctypes.data)
    return rc, [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(int(counts[0]))] if rc == OK else None


def test_merge_acceptance(A, api, check):
    """What kyhip_frame_merge decides on the host, on synthetic states: the state of the slice above (it holds COVER) offered to other frames."""
    state, _, _ = _trailer_state(A, api, check, True)
    assert _merge_state(A, api, check, state, (0, 0), []) == (OK, COVER)                                    # a collector takes it
    assert _merge_state(A, api, check, state, (48, 160), [(48, 112)], True) == (OK, [(0, 112), (160, 224), (436, 500)])
    assert _merge_state(A, api, check, state, (48, 160), [(48, 112), (224, 308)], True) == (OK, [(0, 112), (160, 308), (436, 500)])
    assert _merge_state(A, api, check, state, (224, 332), [])[0] == OK
    assert _merge_state(A, api, check, state, (0, 0), [(24, 64)])[0] == INVALID                             # intersects the coverage
    assert _merge_state(A, api, check, state, (24, 112), [])[0] == INVALID                                  # ... the owned range, not yet rendered
    assert _merge_state(A, api, check, state, (0, 500), [])[0] == INVALID                                   # a frame that owns everything
    assert _merge_state(A, api, check, state, (0, 0), [], False, True)[0] == INVALID                        # a frame that retires blocks
    assert _merge_state(A, api, check, state[:-1], (0, 0), [])[0] == INVALID and _merge_state(A, api, check, state[:40], (0, 0), [])[0] == INVALID
    assert _merge_state(A, api, check, _patched(state, SEED_AT, "<I", 4321), (0, 0), [])[0] == INVALID   # another seed
    assert _merge_state(A, api, check, _patched(state, 8, "<Q", 1), (0, 0), [])[0] == INVALID               # another source hash
    silent, _, _ = _trailer_state(A, api, check, False)
    assert _merge_state(A, api, check, silent, (0, 0), [], True)[0] == INVALID                              # a tracking frame, a state without noise trailer
    assert _merge_state(A, api, check, silent, (0, 0), [], False) == (OK, COVER)
    assert _merge_state(A, api, check, state, (0, 0), [], False) == (OK, COVER)                             # a frame that does not track ignores the trailer
    # 30 ranges of the receiver's own plus the state's three: KY_ERR_LIMIT
    mine = [(50 + 4 * i, 52 + 4 * i) for i in range(27)] + [(226, 232), (240, 248), (300, 302)]
    assert _merge_state(A, api, check, state, (0, 0), mine)[0] == LIMIT
    # a plain frame's state holds [0, its samples done)
    plain, _, _ = _trailer_state(A, api, check, False, (0, 500), 0, [])
    assert _merge_state(A, api, check, _patched(plain, SAMPLES_DONE_AT, "<i", 160), (160, 332), [(160, 224)]) == (OK, [(0, 224)])
    assert _merge_state(A, api, check, _patched(plain, SAMPLES_DONE_AT, "<i", 161), (160, 332), [])[0] == INVALID
    assert _merge_state(A, api, check, _patched(plain, SAMPLES_DONE_AT, "<i", 176), (160, 332), [])[0] == INVALID


def _host_merge(check, words_a, flags_a, words_b, flags_b, total, pairs_a=None, n_a=0, pairs_b=None, n_b=0):
    wa, wb = np.array(words_a, np.int64, order="C"), np.ascontiguousarray(words_b, np.int64)
    fa, fb = np.array(flags_a, np.uint32, order="C"), np.ascontiguousarray(flags_b, np.uint32)
    pa = pb = None
    if pairs_a is not None:
        pa, pb = np.ascontiguousarray(np.stack(pairs_a, axis=1), np.float64), np.ascontiguousarray(np.stack(pairs_b, axis=1), np.float64)
    rc = check.kyhostcheck_merge(wa.ctypes.data, wb.ctypes.data, fa.ctypes.data, fb.ctypes.data, None if pa is None else pa.ctypes.data,
                                 None if pb is None else pb.ctypes.data, len(fa), total, n_a, n_b)
    assert rc == OK
    return wa, fa, None if pa is None else (pa[:, 0], pa[:, 1])


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_merge_matches_the_numpy_restatement(check):
    rng = np.random.default_rng(11)
    n, total = 301, 500
    edge = np.array([(1 << 62) - 1, -(1 << 62), (1 << 62) - 12345, -(1 << 62) + 999, -1, 0, 1, -(1 << 40)], np.int64)
    words_a = rng.integers(-(1 << 40), 1 << 44, (n, 3))
    words_b = rng.integers(-(1 << 40), 1 << 44, (n, 3))
    words_a[:8, 0], words_b[:8, 0] = edge, edge[::-1]          # sums near +-2^62 stay inside the word; negatives
    words_a[8:16, 1], words_b[8:16, 1] = edge, -edge // 2
    flags_a, flags_b = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    flags_a[20:29] = 1 << np.arange(9)                          # all nine flag bits, on either side and on both
    flags_b[24:33] = 1 << np.arange(9)
    flags_b[40] = 0x1FF
    n_a, n_b = 176, 168
    ya, yb = rng.uniform(0, 2 * n_a, n), rng.uniform(0, 2 * n_b, n)
    ya[50:60] = yb[50:60] * n_a / n_b                           # equal means (to rounding) ...
    ya[60], yb[60] = 0.5 * n_a, 0.5 * n_b                       # ... and exactly equal ones
    ya[61:70] = yb[61:70] / n_b * n_a * (1 + 1e-12)             # means 1e-12 apart, relative
    m2a, m2b = rng.uniform(0, 3, n), rng.uniform(0, 3, n)
    m2b[70:80] = 0
    for (ca, cb) in ((n_a, n_b), (0, n_b), (n_a, 0), (0, 0), (4, 3)):
        pa, pb = (ya.copy(), m2a.copy()), (yb.copy(), m2b.copy())
        if ca == 0:
            pa = (np.zeros(n), np.zeros(n))
        w, f, pairs = _host_merge(check, words_a, flags_a, words_b, flags_b, total, pa, ca, pb, cb)
        rw, rf, rpairs = S.merge(words_a, flags_a, words_b, flags_b, total, pa, ca, pb, cb)
        assert np.array_equal(w, rw) and np.array_equal(f, rf)
        assert np.array_equal(_bits(pairs[0]), _bits(rpairs[0])) and np.array_equal(_bits(pairs[1]), _bits(rpairs[1])), (ca, cb)
        assert np.array_equal(_bits(pairs[0]), _bits(R.luminance(rw, total)))    # y_prev is the merged words' luminance, not a sum of the two
        if cb == 0 and ca > 0:
            assert np.array_equal(_bits(pairs[1]), _bits(pa[1]))
        if ca == 0:
            assert np.array_equal(_bits(pairs[1]), _bits(pb[1]))
    assert int(rw[0, 0]) == (1 << 62) - 1 - (1 << 40) and int(rw[1, 0]) == -(1 << 62) + 1 and (rw[:16] < 0).any()
    assert np.array_equal(f[20:33], flags_a[20:33] | flags_b[20:33]) and f[40] == 0x1FF and f[26] == (1 << 6 | 1 << 2)
    w, f, pairs = _host_merge(check, words_a, flags_a, words_b, flags_b, total)   # frames that track no noise
    assert np.array_equal(w, rw) and np.array_equal(f, rf) and pairs is None
    # the side that receives shows in m2's last bits at most: the two orders agree to rounding
    ab = S.merge(words_a, flags_a, words_b, flags_b, total, (ya, m2a), n_a, (yb, m2b), n_b)[2][1]
    ba = S.merge(words_b, flags_b, words_a, flags_a, total, (yb, m2b), n_b, (ya, m2a), n_a)[2][1]
    assert np.allclose(ab, ba, rtol=1e-14, atol=0)


def test_merging_a_batch_without_spread_is_noise_update(check):
    """A frame at n_prev samples that receives the next pass's batch as a frame of its own with m2 = 0: noise_update's m2, bit for bit -- against the restatement's
    update and against kyhostcheck_noise (noise_update itself as host code)."""
    rng = np.random.default_rng(5)
    n, total = 257, 500
    for n_prev, n_now in ((112, 224), (24, 48), (4, 7), (436, 500), (48, 308)):
        first = rng.integers(0, 1 << 40, (n, 3))
        batch = rng.integers(0, 1 << 40, (n, 3))
        y1, y2 = R.luminance(first, total), R.luminance(first + batch, total)
        m2 = rng.uniform(0, 2, n)
        _, want = R.update(y1, m2, y2, n_prev, n_now)
        _, _, pairs = _host_merge(check, first, np.zeros(n, np.uint32), batch, np.zeros(n, np.uint32), total, (y1, m2), n_prev, (y2 - y1, np.zeros(n)), n_now - n_prev)
        assert np.array_equal(_bits(pairs[1]), _bits(want)) and np.array_equal(_bits(pairs[0]), _bits(y2))
    # ... and from a fresh estimate through the host's noise_update: two passes, then the same two as a merge
    acc = np.ascontiguousarray(np.stack([first, first + batch]))
    done = np.array([112, 224], np.int32)
    state, out = np.zeros((2, n, 2), np.float64), np.zeros((2, n), np.float32)
    assert check.kyhostcheck_noise(acc.ctypes.data, done.ctypes.data, 2, n, total, None, state.ctypes.data, out.ctypes.data, None, 0, 0, 0, 0) == OK
    y1, y2 = R.luminance(first, total), R.luminance(first + batch, total)
    _, _, pairs = _host_merge(check, first, np.zeros(n, np.uint32), batch, np.zeros(n, np.uint32), total, (y1, np.zeros(n)), 112, (y2 - y1, np.zeros(n)), 112)
    assert np.array_equal(_bits(pairs[1]), _bits(state[1, :, 1])) and np.array_equal(_bits(pairs[0]), _bits(state[1, :, 0])) and (pairs[1] > 0).any()


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    from ky_amd import dist
    state = bytes((rank * 37 + i * (rank + 1)) % 251 for i in range(4099))
    got = dist.gather_states(state, rank, world)
    if rank == 0:
        q.put([bytes(g) for g in got])
    else:
        assert got is None
    tdist.barrier()
    tdist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gather_states_over_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == [bytes((r * 37 + i * (r + 1)) % 251 for i in range(4099)) for r in range(world)]   # every rank's bytes, in rank order
