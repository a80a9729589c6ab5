"""not gpu: the workspace walker of the library (reazonspeech_amd/csrc/rs_arena.h) compiled on its own with g++.

One layout of mixed pieces is run twice, as every entry point of the library does it: on an arena without a base (the
*_workspace_bytes query) and on an arena over a buffer (the launch).  Both passes must end at the same size, the measuring pass
must hand out null pointers only, every carved pointer must be 256-aligned and sit at the base plus the aligned sizes before it,
and a piece of no elements must take no room.

The header also holds the one Conv2dSubsampling chunk rule (rs_sub_chunk_rule).  Its reserve must cover chunk * per-utterance
bytes and never shrink as an utterance grows, which chunk * per-utterance itself does wherever the chunk steps down."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(os.path.dirname(HERE), "reazonspeech_amd", "csrc")

# (element size, elements) in layout order: int32 x 7, no floats, uint16 x 130, double x 33, one byte
PIECES = [(4, 7), (4, 0), (2, 130), (8, 33), (1, 1)]

SOURCE = r"""
#include <stdint.h>
#include "rs_arena.h"

struct Pieces { int32_t* a; float* none; uint16_t* b; double* c; char* d; };

static Pieces layout(rs_arena& ar) {
    Pieces p;
    p.a = ar.take<int32_t>(7);
    p.none = ar.take<float>(0);
    p.b = ar.take<uint16_t>(130);
    p.c = ar.take<double>(33);
    p.d = ar.take<char>(1);
    return p;
}

extern "C" size_t run_layout(void* base, uintptr_t* out) {
    rs_arena ar(base);
    const Pieces p = layout(ar);
    out[0] = (uintptr_t)p.a; out[1] = (uintptr_t)p.none; out[2] = (uintptr_t)p.b; out[3] = (uintptr_t)p.c; out[4] = (uintptr_t)p.d;
    return ar.bytes();
}
extern "C" size_t align_of(size_t x) { return rs_align(x); }
extern "C" size_t sub_chunk(size_t per_utt, size_t bound, size_t grid_rows, int B, int* chunk) {
    const rs_sub_chunk c = rs_sub_chunk_rule(per_utt, bound, grid_rows, B);
    *chunk = c.chunk;
    return c.reserve;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("arena")
    src, so = d / "arena_layout.cpp", d / "libarena_layout.so"
    src.write_text(SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", HEADER_DIR, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.run_layout.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    lib.run_layout.restype = ctypes.c_size_t
    lib.align_of.argtypes = [ctypes.c_size_t]
    lib.align_of.restype = ctypes.c_size_t
    lib.sub_chunk.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.sub_chunk.restype = ctypes.c_size_t
    return lib


def align(x):
    return (x + 255) // 256 * 256


def test_alignment_rule(lib):
    for x in (0, 1, 255, 256, 257, 4096, 2 ** 31 + 1):
        assert lib.align_of(x) == align(x)


def test_measuring_and_carving_passes_agree(lib):
    measured = (ctypes.c_size_t * len(PIECES))()
    n_measure = lib.run_layout(None, measured)
    assert list(measured) == [0] * len(PIECES)                       # no base: null pointers only

    raw = ctypes.create_string_buffer(n_measure + 512)
    base = align(ctypes.addressof(raw))                              # a 256-aligned base inside the buffer, as the device allocator gives
    carved = (ctypes.c_size_t * len(PIECES))()
    n_carve = lib.run_layout(ctypes.c_void_p(base), carved)
    assert n_carve == n_measure == sum(align(size * n) for size, n in PIECES)

    at = base
    for k, (size, n) in enumerate(PIECES):
        assert carved[k] == at and carved[k] % 256 == 0, (k, carved[k] - base, at - base)
        at += align(size * n)
    assert carved[1] == carved[2]                                    # the zero-length piece advanced nothing
    assert at - base == n_carve


def sub_chunk(lib, per_utt, bound, grid_rows, B):
    chunk = ctypes.c_int(-1)
    reserve = lib.sub_chunk(per_utt, bound, grid_rows, B, ctypes.byref(chunk))
    return chunk.value, reserve


def test_chunk_rule_reserve_covers_the_chunk_and_is_monotone(lib):
    bound, B, rows = 1 << 30, 96, 100
    ladder = range(10 << 20, 12 << 20, 4096)                         # bound / per_utt falls from 102 to 85: the chunk steps down below B
    got = [sub_chunk(lib, per_utt, bound, rows, B) for per_utt in ladder]
    for per_utt, (chunk, reserve) in zip(ladder, got):
        assert chunk == min(B, bound // per_utt)
        assert reserve == min(B * per_utt, bound) >= chunk * per_utt
    reserves = [r for _, r in got]
    used = [c * p for p, (c, _) in zip(ladder, got)]
    assert all(a <= b for a, b in zip(reserves, reserves[1:]))
    assert any(a > b for a, b in zip(used, used[1:]))                # what the reserve must not follow


def test_chunk_rule_limits(lib):
    assert sub_chunk(lib, 1000, 1 << 30, 10, 7) == (7, 7000)         # everything fits: the whole batch, its own size
    assert sub_chunk(lib, (1 << 30) + 8, 1 << 30, 10, 7) == (1, (1 << 30) + 8)    # one utterance above the bound still runs, alone
    assert sub_chunk(lib, 1000, 1 << 30, 30000, 8) == (2, 8000)      # the grid limit: 2 x 30000 rows <= 65535 < 3 x 30000
    assert sub_chunk(lib, 1000, 1 << 30, 70000, 8) == (1, 8000)
