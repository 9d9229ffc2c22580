"""Two tiles per block (giant_kernel.hip.h tile_pair_walk, BSGS_TILES_PER_BLOCK): the quad-chain kernel walks one slice of the giants for tiles 2u and 2u + 1
in ONE batch inversion.  The hit lists must be the oracle's and the one-tile-per-block kernel's, whatever the pair holds: the same giant hit in both tiles, an
equal-x giant in the second tile, code 5 on both tiles; odd and narrow launches fall back to one tile per block; the XCD-chunked block map; the probe digests are per tile."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

O_QUIRK = 1                    # oracle flag O_QUIRK_NEGMODP (oracle/bsgs_ref.h)


@pytest.fixture(scope="module")
def O():
    import oracle_lib
    oracle_lib.lib()
    return oracle_lib


def _device(tpb):
    import pybsgs
    os.environ["BSGS_TILES_PER_BLOCK"] = str(tpb)
    try:
        return pybsgs.Device(0)
    finally:
        del os.environ["BSGS_TILES_PER_BLOCK"]


def _ref(O, centres, g2, t, b, p, gpu, htsz, flags=0):
    out = []
    for k, Pt in enumerate(centres):
        r, _ = O.tile_ref(Pt, g2, t, b, p, gpu, htsz, flags, 65536)
        out += [(k, c, i) for c, i in r]
    return out


def _build_case(O, seed, t, b, p, w, htsz, nplant, tiles):
    """real giants; a table of random keys into which the keys of x(P +- G2[i]) of the planted tiles are put, plus x of centre 0 (code 5) and x(2P) of a
    centre equal to giant 77 (code 4).  Tiles: the planted ones, then the pairs (same centre twice: every hit at the same giant index in both tiles),
    (centre 0 twice: code 5 on both tiles), (planted, the equal-x centre: the doubling in the second tile of a pair)."""
    rnd = random.Random(seed)
    g2 = O.build_g2(t, b, p, w)
    n = t * b * p
    centres = [O.pt_mul(rnd.randrange(1, 2**128)) for _ in range(tiles)]
    eq = O.g2_unpack(g2, t, b, p, 77)
    keys = [rnd.getrandbits(64) for _ in range(w - nplant * tiles - 2)]
    for Pt in centres:
        for _ in range(nplant):
            i = rnd.randrange(n)
            _, xm, xp, _ = O.tile_xs(Pt, O.g2_unpack(g2, t, b, p, i), 0)
            keys.append((xm if rnd.random() < 0.5 else xp) & (2**64 - 1))
    keys.append(centres[0][0] & (2**64 - 1))
    is_eq, _, _, xd = O.tile_xs(eq, O.g2_unpack(g2, t, b, p, 77), 0)
    assert is_eq
    keys.append(xd & (2**64 - 1))
    gpu, _ = O.pack_tables_from_keys(np.array(keys, dtype=np.uint64), htsz)
    return g2, gpu, centres + [centres[1], centres[1], centres[0], centres[0], centres[2], eq]


@pytest.fixture(scope="module")
def case(O):
    t, b, p, w, htsz = 64, 8, 12, 1 << 16, 14                   # T = 512: two 256-thread slices, 12 giants per thread (6 quads of the pair walk)
    g2, gpu, centres = _build_case(O, 5151, t, b, p, w, htsz, 12, 8)
    return t, b, p, w, htsz, g2, gpu, centres


@pytest.mark.parametrize("layout", [2, 4])
def test_pair_walk_matches_oracle_and_one_tile_blocks(O, case, layout):
    t, b, p, w, htsz, g2, gpu, centres = case
    ref = _ref(O, centres, g2, t, b, p, gpu, htsz)
    assert any(c == 5 for k, c, _ in ref if k == len(centres) - 4) and any(c == 5 for k, c, _ in ref if k == len(centres) - 3)
    assert any(c == 4 and i == 77 for k, c, i in ref if k == len(centres) - 1)          # the doubling of the equal-x giant, second tile of its pair
    same = len(centres) - 6
    assert [(c, i) for k, c, i in ref if k == same] == [(c, i) for k, c, i in ref if k == same + 1] != []
    got = {}
    for tpb in (1, 2):
        d = _device(tpb)
        d.upload_g2(g2, t, b, p)
        d.upload_htgpu(gpu, 1 << htsz, w, layout)
        hits, n, _ = d.run(centres, 65536)
        assert d.last_kernel() == "giant_pair2_kernel<2, false, true>"
        assert d.last_tiles_per_block() == tpb
        got[tpb] = hits
        assert n == len(ref) and hits == ref, (tpb, layout)
        # odd launch: one tile per block whatever the switch
        hits, n, _ = d.run(centres[:5], 65536)
        assert d.last_tiles_per_block() == 1
        assert hits == [h for h in ref if h[0] < 5]
        d.close()
    assert got[1] == got[2]


def test_pair_walk_quirk_mode(O, case):
    t, b, p, w, htsz, g2, gpu, centres = case
    ref = _ref(O, centres, g2, t, b, p, gpu, htsz, O_QUIRK)
    d = _device(2)
    d.upload_g2(g2, t, b, p)
    d.upload_htgpu(gpu, 1 << htsz, w, 2)
    d.set_flags(1)
    hits, n, _ = d.run(centres, 65536)
    assert d.last_tiles_per_block() == 2
    assert n == len(ref) and hits == ref
    d.close()


def test_pair_walk_digest_per_tile(O, case):
    """debug_flags & 8: one (xor, sum) of the probed keys per (tile, engine thread) -- the same from a pair block as from two one-tile blocks"""
    t, b, p, w, htsz, g2, gpu, centres = case
    ref = _ref(O, centres, g2, t, b, p, gpu, htsz)
    out = {}
    for tpb in (1, 2):
        d = _device(tpb)
        d.upload_g2(g2, t, b, p)
        d.upload_htgpu(gpu, 1 << htsz, w, 2)
        dg, hits, nh = d.run_digest(centres, 65536)
        assert d.last_tiles_per_block() == tpb
        assert hits == ref
        out[tpb] = dg
        d.close()
    assert (out[1] == out[2]).all()
    assert (out[2][:, :, 0] != 0).all()                         # every (tile, thread) wrote its own digest


def test_chunked_map_and_narrow_launch(O):
    """T = 2048: eight blocks per tile, the XCD-chunked block map of the production shape.  A two-tile launch at this geometry takes the narrow batching
    (more threads, 128 giants per thread) and one tile per block; with the narrow copy off (BSGS_NARROW_LAUNCHES=0) the same launch runs two tiles per
    block over the chunked map.  Both give the oracle's hits."""
    t, b, p, w, htsz = 256, 8, 256, 1 << 16, 14
    g2, gpu, centres = _build_case(O, 7373, t, b, p, w, htsz, 8, 3)
    centres = centres[:2]
    ref = _ref(O, centres, g2, t, b, p, gpu, htsz)
    assert any(c == 5 for k, c, _ in ref if k == 0)
    d = _device(2)
    d.upload_g2(g2, t, b, p)
    d.upload_htgpu(gpu, 1 << htsz, w, 2)
    hits, n, _ = d.run(centres, 65536)
    assert d.last_batching() == (4096, 128) and d.last_tiles_per_block() == 1
    assert n == len(ref) and hits == ref
    d.close()
    os.environ["BSGS_NARROW_LAUNCHES"] = "0"
    try:
        d = _device(2)
    finally:
        del os.environ["BSGS_NARROW_LAUNCHES"]
    d.upload_g2(g2, t, b, p)
    d.upload_htgpu(gpu, 1 << htsz, w, 2)
    hits, n, _ = d.run(centres, 65536)
    assert d.last_batching() == (2048, 256) and d.last_tiles_per_block() == 2
    assert n == len(ref) and hits == ref
    d.close()
