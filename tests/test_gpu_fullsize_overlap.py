"""Launch overlap at the metric's size (GPU): the scratch of the default kernel lies in PIECES of 32 tiles there, and a queued launch goes out as two kernels whose
piece tables must not overlap -- 192 tiles as 96 | 96 (pieces 0-2 | 3-5), 144 tiles as 64 | 80 (pieces 0-1 | 2-4).  Two kernels that shared a piece would run at the
same time on the same scratch and lose or invent hits without any error.

Every tile carries a planted hit: the walk's centres are (m0 + k * d) * G with m0 = 100 * 2w + 1000 and d = 87383 * 2w + 1, so tile k must report code 1 at giant
99 + 87383 k with b' = 1000 + k -- the giant index sweeps the whole range of 2^24, and the first and last tile of each part, the tiles either side of the cut and every piece edge
are covered because every tile is.  The mirrored walk (-m0, -d) gives code 2 at the same giants.  Beyond the analytic hits only 32-bit hash collisions may appear
(2 * 2^24 * 4 / 2^32 = 0.031 per tile), and the COMPLETE lists must equal those of an engine opened with BSGS_LAUNCH_OVERLAP=0.  Launches are queued with
enqueue_walk / enqueue_raw + collect: the synchronous run calls never split.  Runs in the TEST library: it reports where the most recent launch was cut."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
WEXP, HTSZ = 30, 28
T, B, P = 256, 256, 256
STEP = 87383                                   # giants between the planted hits of neighbouring tiles: 99 + 191 * 87383 < 2^24
KERNEL = "giant_pair2_kernel<2, false, true>"


def _scenarios(dev, img, w, overlap):
    """the three queued scenarios on one engine; returns their sorted complete hit lists"""
    import pybsgs
    from pybsgs import ecpy
    m0, d = 100 * 2 * w + 1000, STEP * 2 * w + 1
    A = ecpy.addpubg(w)
    dev.generate_g2(A[0], A[1], T, B, P)
    dev.upload_htgpu_device(img.data_ptr(), 1 << HTSZ, w, pybsgs.TABLE_LINES64)
    dev.set_tiles_per_launch(192)                                                          # the default while 72 GiB are free; fixed here so that the cuts do not depend on that
    out = {}

    def done(name, launches, split):
        hits, n, _ = dev.collect()
        assert n == len(hits)
        cp = dev.chain_placement()
        assert cp["pieces"] == 6 and cp["tiles_per_piece"] == 32, cp                       # sized for a full launch of 192 tiles, as without overlap
        assert dev.debug_last_split() == (split if overlap else 0), (name, dev.debug_last_split())
        assert dev.launch_count() - l0 == launches and dev.last_kernel() == KERNEL and dev.last_tiles_per_block() == 2
        out[name] = sorted(hits)

    dev.set_walk(ecpy.mul(m0), ecpy.mul(d))
    l0 = dev.launch_count()
    dev.enqueue_walk(0, 192)                                                                # 96 | 96
    done("walk192", 1, 96)
    l0 = dev.launch_count()
    dev.enqueue_walk(0, 192)                                                                # 96 | 96, then 64 | 80 behind it: pieces 2 and 3-4 change streams
    dev.enqueue_walk(48, 144)
    done("walk192+144", 2, 64)
    dev.set_walk(ecpy.mul(N - m0), ecpy.mul(N - d))                                         # the mirrored walk, its centres uploaded by the host
    centres = dev.walk_centres(0, 144)
    assert centres[0] == ecpy.mul(N - m0) and centres[143] == ecpy.mul((N - m0 - 143 * d) % N)
    l0 = dev.launch_count()
    dev.enqueue_raw(b"".join(pybsgs.le32(x) + pybsgs.le32(y) for x, y in centres), 144)    # 64 | 80
    done("raw144", 1, 64)
    return out


def test_split_launches_with_scratch_in_pieces_at_full_size(request, monkeypatch):
    from conftest import rerun_in_test_library
    if rerun_in_test_library(request):
        return
    import pybsgs
    w = 1 << WEXP
    img = torch.empty((1 << HTSZ) + 1 + w, dtype=torch.int32, device="cuda:0")
    res = {}
    for overlap in (True, False):
        monkeypatch.setenv("BSGS_LAUNCH_OVERLAP", "1" if overlap else "0")                  # read when the engine is opened
        dev = pybsgs.Device(0)
        if overlap:
            dev.build_baby_tables_device(w, HTSZ, img.data_ptr())
        res[overlap] = _scenarios(dev, img, w, overlap)
        dev.close()
    on, off = res[True], res[False]
    # (queued tile, walk tile) of every tile of a scenario, and the code its planted hit has
    cases = {"walk192": ([(k, k) for k in range(192)], 1),
             "walk192+144": ([(k, k) for k in range(192)] + [(192 + k, 48 + k) for k in range(144)], 1),
             "raw144": ([(k, k) for k in range(144)], 2)}
    for name, (tiles, code) in cases.items():
        assert on[name] == off[name], name                                                  # complete lists, hash collisions included
        want = {(q, code, 99 + STEP * s) for q, s in tiles}
        got = set(on[name])
        assert want <= got, (name, sorted(want - got)[:8])
        assert len(on[name]) == len(got)                                                    # nothing reported twice
        # everything else is a 32-bit hash collision: 0.031 per tile expected (6 / 10.5 / 4.5 per scenario); 40 is beyond any Poisson tail that matters
        assert len(got) - len(want) <= 40, (name, len(got) - len(want))
        assert all(0 <= q < len(tiles) for q, _, _ in got), name                           # tile numbering: queued + k
