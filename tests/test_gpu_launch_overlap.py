"""Launch overlap (bsgs_hip.hip launch_tiles): a launch of 2 x BSGS_TILE_CHUNK tiles or more goes out as two kernels on two streams with disjoint halves of the scratch,
the centres on a third stream.  The hit lists must not know: complete lists equal with BSGS_LAUNCH_OVERLAP=1 and =0 (fresh child processes, the test library: it
reports whether a launch was split; queued with enqueue + collect: the synchronous run calls stay one kernel), and equal to the oracle's tile model on the planted tiles -- the first and last tile of each part, the tiles either side of
the boundary, the last tile of the launch -- for an even launch, an odd one, one whose half is odd, one below two chunks (stays one kernel), reference-quirk mode
with listed giants, three enqueues before one collect, and host-uploaded centres.  Two geometries: T = 2048 (eight blocks per tile: the XCD-chunk block map) and
T = 512 (the plain block map).  Small shapes: 2^16 keys in 2^14 buckets of 64-byte lines, 8 giants per thread; one GPU process per switch setting."""
import json
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O_QUIRK = 1                    # oracle flag O_QUIRK_NEGMODP (oracle/bsgs_ref.h)
CHUNK = 64                     # BSGS_TILE_CHUNK
W, HTSZ = 1 << 16, 14
GEOMS = {"xcd_chunk_map": (64, 32, 8), "plain_map": (64, 8, 8)}
SIZES = (2 * CHUNK, 2 * CHUNK + 1, 2 * CHUNK + 2, 100)                    # even, odd, half odd, below two chunks
# walk tiles: every part's first and last tile and both sides of every boundary, for every size, and of the five launches of MULTI (cut at walk tiles 64, 192 and 124)
PLANTED = (0, 1, 63, 64, 65, 66, 99, 123, 124, 125, 127, 128, 129, 189, 191, 192, 255, 256, 299)
MULTI = ((0, 300), (60, 128), (120, 70))                                  # (first walk tile, tiles) of three enqueues before one collect
KERNEL = "giant_pair2_kernel<2, false, true>"


def expected_split(n):
    """one-buffer scratch: n / 2, made even when n is even; below two chunks one kernel"""
    if n < 2 * CHUNK:
        return 0
    return n // 2 + (1 if n % 2 == 0 and (n // 2) % 2 else 0)


def _build_geometry(O, name, t, b, p):
    rnd = random.Random("launch overlap " + name)
    n, T = t * b * p, t * b
    img = np.frombuffer(O.build_g2(t, b, p, W), dtype=np.uint32).copy()
    listed = (5, n - 3)                                                    # giants made to trip the reference's NEGMODP: word 0 of Gy above 0xFFFFFC2F
    for i in listed:
        tid, j = divmod(i, p)
        img[8 * n + (j * 8 + 7) * T + tid] = 0xFFFFFFF0
    g2 = img.tobytes()
    P0, D = O.pt_mul(rnd.randrange(1, 2**200)), O.pt_mul(rnd.randrange(1, 2**200))
    ntiles = max(f + m for f, m in MULTI)
    centres = [P0]
    for _ in range(ntiles - 1):
        centres.append(O.pt_add(centres[-1], D))
    plant = []
    for s in PLANTED:
        for _ in range(3):
            i = rnd.choice([k for k in range(n) if k not in listed])
            _, xm, xp, _ = O.tile_xs(centres[s], O.g2_unpack(g2, t, b, p, i), 0)
            plant.append((xm if rnd.random() < 0.5 else xp) & (2**64 - 1))
        # listed giants: the QUIRK x of the first (a hit in reference-quirk mode only), the CORRECT x of the second (a hit in the default mode only)
        xq = O.tile_xs(centres[s], O.g2_unpack(g2, t, b, p, listed[0]), O_QUIRK)[1]
        xc = O.tile_xs(centres[s], O.g2_unpack(g2, t, b, p, listed[0]), 0)[1]
        assert xq != xc
        plant.append(xq & (2**64 - 1))
        plant.append(O.tile_xs(centres[s], O.g2_unpack(g2, t, b, p, listed[1]), 0)[1] & (2**64 - 1))
    keys = [rnd.getrandbits(64) for _ in range(W - len(plant))] + plant
    gpu, _ = O.pack_tables_from_keys(np.array(keys, dtype=np.uint64), HTSZ)
    ref = {}
    for flags in (0, O_QUIRK):
        for s in PLANTED:
            r, nr = O.tile_ref(centres[s], g2, t, b, p, gpu, HTSZ, flags, 65536)
            assert nr == len(r) >= 4
            ref[(flags, s)] = sorted((i, c) for c, i in r)
    return dict(t=t, b=b, p=p, g2=g2, gpu=gpu, P0=P0, D=D, centres=centres, listed=listed, ref=ref)


def _run_engine(case_path, out_path):
    """child process: every scenario on one engine per geometry, with whatever BSGS_LAUNCH_OVERLAP says"""
    for q in (ROOT, os.path.join(ROOT, "bsgs-cuda_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, q)
    import torch  # noqa: F401  (first: torch ships its own HIP runtime)
    import pybsgs
    with open(case_path, "rb") as f:
        geoms = pickle.load(f)
    out = {}
    for name, g in geoms.items():
        t, b, p = g["t"], g["b"], g["p"]
        dev = pybsgs.Device(0)
        dev.upload_g2(g["g2"], t, b, p)
        dev.upload_htgpu(g["gpu"], 1 << HTSZ, W, pybsgs.TABLE_LINES64)
        dev.set_walk(g["P0"], g["D"])
        assert dev.walk_centres(0, 3) == g["centres"][:3] and dev.walk_centres(129, 1) == g["centres"][129:130]
        r = {"engine_geometry": dev.engine_geometry()}

        def record(hits, total, l0):
            return dict(hits=hits, total=total, launches=dev.launch_count() - l0, split=dev.debug_last_split(), tpb=dev.last_tiles_per_block(),
                        kernel=dev.last_kernel(), batching=dev.last_batching())

        for n in SIZES:
            dev.set_tiles_per_launch(n)
            l0 = dev.launch_count()
            dev.enqueue_walk(0, n)
            hits, total, _ = dev.collect()
            r["walk%d" % n] = record(hits, total, l0)
            l0 = dev.launch_count()
            hits, total, _ = dev.run_walk(0, n)                        # the synchronous call: nothing follows its launch, it stays one kernel
            r["lone%d" % n] = record(hits, total, l0)
        dev.set_tiles_per_launch(2 * CHUNK)
        dev.set_flags(pybsgs.FLAG_REFERENCE_QUIRKS)
        r["listed"] = dev.quirk_count()
        l0 = dev.launch_count()
        dev.enqueue_walk(0, 2 * CHUNK)
        hits, total, _ = dev.collect()
        r["quirks"] = record(hits, total, l0)
        dev.set_flags(0)
        l0 = dev.launch_count()
        for first, m in MULTI:
            dev.enqueue_walk(first, m)
        hits, total, _ = dev.collect()
        r["multi"] = record(hits, total, l0)
        m = 2 * CHUNK + 2
        dev.set_tiles_per_launch(m)
        l0 = dev.launch_count()
        dev.enqueue_raw(b"".join(pybsgs.le32(x) + pybsgs.le32(y) for x, y in g["centres"][:m]), m)
        hits, total, _ = dev.collect()
        r["raw"] = record(hits, total, l0)
        r["placement"] = dev.chain_placement()
        dev.close()
        out[name] = r
    with open(out_path, "w") as f:
        json.dump(out, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the oracle's side once, then the engine twice: overlap on (the default) and off"""
    import oracle_lib as O
    import pybsgs
    O.lib()
    assert os.path.exists(pybsgs.TEST_LIB_PATH), "make -C bsgs-cuda_amd builds build/libbsgs_hip_test.so"
    geoms = {name: _build_geometry(O, name, *tbp) for name, tbp in GEOMS.items()}
    d = tmp_path_factory.mktemp("launch_overlap")
    case_path = str(d / "case.pickle")
    with open(case_path, "wb") as f:
        pickle.dump(geoms, f)
    res = {}
    for switch in ("1", "0"):
        out_path = str(d / ("engine_%s.json" % switch))
        env = dict(os.environ, BSGS_LAUNCH_OVERLAP=switch, BSGS_LIB_PATH=pybsgs.TEST_LIB_PATH)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case_path, out_path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        with open(out_path) as f:
            res[switch] = json.load(f)
    return geoms, res


def _by_tile(hits):
    got = {}
    for tile, code, idx in hits:
        got.setdefault(tile, []).append((idx, code))
    return {k: sorted(v) for k, v in got.items()}


@pytest.mark.parametrize("name", sorted(GEOMS))
@pytest.mark.parametrize("n", SIZES)
def test_split_launch_hit_lists_equal_serial_and_oracle(runs, name, n):
    geoms, res = runs
    on, off = res["1"][name]["walk%d" % n], res["0"][name]["walk%d" % n]
    assert on["total"] == len(on["hits"]) and off["total"] == len(off["hits"])
    assert on["hits"] == off["hits"]                                                       # complete lists, false positives included
    got = _by_tile(on["hits"])
    planted = [s for s in PLANTED if s < n]
    n0 = expected_split(n)
    assert {0, n - 1} <= set(planted) and (n0 == 0 or {n0 - 1, n0} <= set(planted))
    for s in planted:
        assert got.get(s, []) == geoms[name]["ref"][(0, s)], (n, s)
    for r, split in ((on, n0), (off, 0)):
        assert r["launches"] == 1 and r["kernel"] == KERNEL and r["tpb"] == (2 if n % 2 == 0 else 1)       # one LOGICAL launch; the pair walk as for one kernel
        assert r["split"] == split and r["batching"] == list(res["1"][name]["engine_geometry"])
    if n0:
        assert n0 % 2 == 0 or n % 2 == 1                                                    # an even launch: two even parts
    for switch in ("1", "0"):
        lone = res[switch][name]["lone%d" % n]
        assert lone["split"] == 0 and lone["launches"] == 1 and lone["hits"] == on["hits"]  # bsgs_run_walk: one kernel whatever the switch says


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_split_launch_in_reference_quirk_mode(runs, name):
    geoms, res = runs
    on, off = res["1"][name]["quirks"], res["0"][name]["quirks"]
    assert res["1"][name]["listed"] == res["0"][name]["listed"] == len(geoms[name]["listed"]) >= 1
    assert on["hits"] == off["hits"] and on["total"] == len(on["hits"]) == off["total"]
    assert on["split"] == CHUNK and off["split"] == 0
    got = _by_tile(on["hits"])
    q, c = geoms[name]["listed"]
    for s in (s for s in PLANTED if s < 2 * CHUNK):
        assert got.get(s, []) == geoms[name]["ref"][(O_QUIRK, s)], s
        assert (q, 2) in got[s] and (c, 2) not in got[s]                                    # the quirk's x of one listed giant, not the correct x of the other: each part ran its own fix-up
    plain = _by_tile(res["1"][name]["walk%d" % (2 * CHUNK)]["hits"])
    assert all((c, 2) in plain[s] and (q, 2) not in plain[s] for s in PLANTED if s < 2 * CHUNK)


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_three_enqueues_one_collect(runs, name):
    """300 + 128 + 70 tiles at 128 per launch: split, split, 44 whole, split, 70 whole -- the scratch changes hands between the streams three times"""
    geoms, res = runs
    on, off = res["1"][name]["multi"], res["0"][name]["multi"]
    assert on["hits"] == off["hits"] and on["total"] == len(on["hits"]) == off["total"]
    want, queued = {}, 0
    for first, m in MULTI:
        for s in PLANTED:
            if first <= s < first + m:
                want[queued + s - first] = geoms[name]["ref"][(0, s)]                      # tile numbering: queued + k
        queued += m
    got = _by_tile(on["hits"])
    assert {k: v for k, v in got.items() if k in want} == want
    # the cuts of the three split launches (walk tiles 64 and 192 of the first enqueue, 124 of the second) have planted tiles on both sides
    assert {63, 64, 191, 192, 300 + 123 - 60, 300 + 124 - 60} <= set(want)
    launches = sum(-(-m // (2 * CHUNK)) for _, m in MULTI)
    assert on["launches"] == off["launches"] == launches == 5                               # logical launches, however many kernels
    assert on["split"] == 0 and off["split"] == 0                                           # the last one (70 tiles) was one kernel


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_host_uploaded_centres(runs, name):
    geoms, res = runs
    on, off = res["1"][name]["raw"], res["0"][name]["raw"]
    m = 2 * CHUNK + 2
    assert on["hits"] == off["hits"] == res["1"][name]["walk%d" % m]["hits"] and on["total"] == len(on["hits"])
    assert on["split"] == expected_split(m) == 66 and off["split"] == 0 and on["launches"] == off["launches"] == 1
    got = _by_tile(on["hits"])
    for s in (s for s in PLANTED if s < m):
        assert got.get(s, []) == geoms[name]["ref"][(0, s)], s


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_switch_off_is_one_kernel_on_one_buffer(runs, name):
    _, res = runs
    for switch in ("1", "0"):
        cp = res[switch][name]["placement"]
        assert cp["pieces"] == 0 and cp["tiles_per_piece"] == 0 and cp["graded"] == 0, cp   # the scratch is where and what it was: one buffer at these sizes
    off = res["0"][name]
    assert all(off[k]["split"] == 0 and off[k]["kernel"] == KERNEL for k in off if isinstance(off[k], dict) and "split" in off[k])
    assert list(off["engine_geometry"]) == [GEOMS[name][0] * GEOMS[name][1], GEOMS[name][2]]


if __name__ == "__main__":
    _run_engine(sys.argv[1], sys.argv[2])
