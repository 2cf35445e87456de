"""What tests/test_frame_book.py and tests/test_frame_book_gpu.py share: kyhostcheck_book (ky_amd/csrc/ky_hostcheck.cpp) from Python -- scripts of operations on the
books of up to five frames (FrameBook, ky_amd/csrc/ky_frame_book.hpp) and four state slots, and one record per operation."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
MAX_RANGES = 32
RECORD = 11 + 2 * MAX_RANGES
FIELDS = ("status", "front", "held", "n_ranges", "own_first", "own_end", "batches", "n_prev", "passes", "n_live", "state_bytes")
PASS, SAVE, LOAD, MERGE, MERGE_FROM, TRACK_NOISE, TRACK_BLOCKS, NOTHING = range(8)
SCENE_HASH = 0x1234


def bind_book(A, lib):
    lib.kyhip_last_error.restype, lib.kyhip_last_error.argtypes = C.c_char_p, []
    lib.kyhostcheck_book.restype = C.c_int
    lib.kyhostcheck_book.argtypes = [A.PP, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def load_book_library(A, sanitized=True):
    """The library that holds kyhostcheck_book: the sanitizer build inside `make sanitize` (sanitized: where the caller accepts it), else the same host-only sources
    built plainly, which load next to libkyhip.so (-Bsymbolic)."""
    if A.SANITIZE and sanitized:
        return bind_book(A, A.load_kyhip())
    target = os.path.join("build", "san", "libkyhip_host_plain.so")
    r = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(os.path.join(ROOT, target))
    for name in ("kyhostcheck_slices",):
        getattr(lib, name).restype, getattr(lib, name).argtypes = A.KYHOSTCHECK_SYMBOLS[name]
    return bind_book(A, lib)


def run_book(check, p, books, ops, scene_hash=SCENE_HASH, source_hash=0, slot_capacity=1 << 18):
    """The script `ops` ({operation, book, arg, arg2}; short ones are padded with zeros) on the books that own `books`: (one record per operation as a dict with the
    coverage under "ranges", the four slots' bytes).  source_hash: the kernel source hash the books' headers carry (0: the host-only library's own, which differs from
    libkyhip.so's by the compiler that built it)."""
    own = np.ascontiguousarray(np.asarray(books, np.int32).ravel())
    script = np.zeros((len(ops), 4), np.int32)
    for k, op in enumerate(ops):
        script[k, :len(op)] = op
    records = np.full((max(len(ops), 1), RECORD), -77, np.int32)
    slots = np.zeros((4, slot_capacity), np.uint8)
    sizes = (C.c_size_t * 4)()
    rc = check.kyhostcheck_book(C.byref(p), scene_hash, source_hash, own.ctypes.data, len(books), script.ctypes.data, len(ops), records.ctypes.data, slots.ctypes.data, slot_capacity, sizes)
    assert rc == OK, check.kyhip_last_error()
    assert all(n <= slot_capacity for n in sizes)
    out = []
    for r in records[:len(ops)]:
        d = dict(zip(FIELDS, (int(v) for v in r[:11])))
        d["ranges"] = [(int(r[11 + 2 * i]), int(r[12 + 2 * i])) for i in range(d["n_ranges"])]
        assert not r[11 + 2 * d["n_ranges"]:].any()
        out.append(d)
    return out, [slots[i, :sizes[i]].tobytes() for i in range(4)]


def state_of(record):
    return {k: v for k, v in record.items() if k != "status"}
