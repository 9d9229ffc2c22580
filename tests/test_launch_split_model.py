"""CPU-only: the rule that splits one launch of the tile kernel into two kernels on two streams (bsgs_internal.h bsgs_launch_split, exported by the TEST library only
as bsgs_debug_launch_split) against a restatement in Python, over every launch size up to 400 tiles, scratch in one buffer and in pieces, pair walk or not.

The parts must be disjoint and cover [0, n); both even when the launch walks two tiles per block; in pieces mode the boundary lies on a piece boundary, so that
part 1's pieces are none of part 0's, and every piece either part touches exists; launches below two chunks and pieces of one tile stay one kernel."""
import ctypes
import os

import pytest

CHUNK = 64                                                    # BSGS_TILE_CHUNK


def model(n, piece, pieces, chunk, pair):
    """first tile of part 1, 0 = one kernel"""
    if n < 2 * chunk or piece == 1:
        return 0
    if piece:
        n0 = (n // 2 + piece // 2) // piece * piece           # the piece boundary nearest n / 2
        if -(-n // piece) > pieces:
            return 0
    else:
        n0 = n // 2 + (1 if n % 2 == 0 and (n // 2) % 2 else 0)
    if not 0 < n0 < n or (pair and (n0 % 2 or (n - n0) % 2)):
        return 0
    return n0


@pytest.fixture(scope="module")
def split():
    import pybsgs
    if not os.path.exists(pybsgs.TEST_LIB_PATH):
        pytest.fail("make -C bsgs-cuda_amd builds build/libbsgs_hip_test.so")
    L = ctypes.CDLL(pybsgs.TEST_LIB_PATH)
    u32 = ctypes.c_uint32
    L.bsgs_debug_launch_split.argtypes = [u32, u32, u32, u32, u32, ctypes.POINTER(u32)]

    def f(n, piece, pieces, chunk, pair):
        out = u32(12345)
        assert L.bsgs_debug_launch_split(n, piece, pieces, chunk, int(pair), ctypes.byref(out)) == 0
        return out.value
    return f


def test_split_rule_is_exported_by_the_test_library_only():
    import subprocess
    import pybsgs
    hooks = ("bsgs_debug_launch_split", "bsgs_debug_last_split")
    for path, exported in ((pybsgs.LIB_PATH, False), (pybsgs.TEST_LIB_PATH, True)):
        r = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        names = {line.split()[-1] for line in r.stdout.splitlines() if line.split()}
        assert "bsgs_collect" in names, path                                                 # nm did list this library's symbols
        for h in hooks:
            assert (h in names) == exported, (path, h)


def test_split_rule_against_the_model_for_every_launch_size(split):
    shapes = [(0, 0)] + [(piece, pieces) for piece in (1, 2, 4, 8, 16, 32, 64, 128, 256) for pieces in (1, 2, 3, 5, 6, 7, 32)]
    seen_split = seen_whole = 0
    for piece, pieces in shapes:
        for pair in (False, True):
            for n in range(0, 401):
                n0 = split(n, piece, pieces, CHUNK, pair)
                tag = (n, piece, pieces, pair, n0)
                assert n0 == model(n, piece, pieces, CHUNK, pair), tag
                if n0 == 0:
                    seen_whole += 1
                    continue
                seen_split += 1
                part0, part1 = range(0, n0), range(n0, n)
                assert len(part0) > 0 and len(part1) > 0 and part0.stop == part1.start and part0.start == 0 and part1.stop == n, tag     # disjoint, cover [0, n)
                assert n >= 2 * CHUNK, tag
                if pair:
                    assert len(part0) % 2 == 0 and len(part1) % 2 == 0, tag
                if n % 2 == 0:
                    assert len(part0) % 2 == 0 and len(part1) % 2 == 0, tag                     # an even launch never turns into two odd kernels
                if piece:
                    assert piece >= 2 and n0 % piece == 0, tag                                   # on a piece boundary
                    used0 = {k // piece for k in part0}
                    used1 = {k // piece for k in part1}
                    assert not (used0 & used1), tag                                              # part 1's pieces are not part 0's
                    assert max(used1) < pieces, tag                                              # every piece touched exists
                    # part 1 addresses its pieces from its own first tile: local tile j lies in piece table entry j // piece = global piece - n0 // piece
                    assert {(k - n0) // piece + n0 // piece for k in part1} == used1, tag
    assert seen_split > 1000 and seen_whole > 1000


def test_split_rule_at_the_shapes_the_engine_runs(split):
    # the headline: 192 tiles, six pieces of 32 tiles -> 96 | 96, three pieces each
    assert split(192, 32, 6, CHUNK, True) == 96
    # the full-size tests: 144 tiles in five pieces (4.5 -> the boundary nearest 72 is 64), 72 tiles stay whole (below two chunks)
    assert split(144, 32, 5, CHUNK, True) == 64
    assert split(72, 32, 3, CHUNK, True) == 0
    # one buffer: 128 -> 64 | 64; 130 has an odd half -> 66 | 64; an odd launch is never a pair walk -> 64 | 65
    assert split(128, 0, 0, CHUNK, True) == 64
    assert split(130, 0, 0, CHUNK, True) == 66
    assert split(129, 0, 0, CHUNK, False) == 64
    assert split(127, 0, 0, CHUNK, False) == 0
    # a pair walk cannot take an odd part: the launch stays whole (the engine never asks: an odd launch is not a pair walk)
    assert split(129, 0, 0, CHUNK, True) == 0
    # a chunk of 0 tiles (never built) splits nothing
    assert split(192, 32, 6, 0, True) == 0
