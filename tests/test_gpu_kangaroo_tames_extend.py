"""GPU: the load into a growing tame table and its sorted read (csrc/kangaroo_tames_extend.hip) against the model (tests/kangaroo_tames_extend_model.py), through
pybsgs: the case lists of tests/kangaroo_tames_extend_cases.py -- probe chains, a chain that wraps, equal tags in a wave and across waves and blocks, tags an
insert stored before, tag 0, ragged sizes -- with the four counts compared exactly and the table as a set; then the sorted read at the sizes around the sort's
tile, on tags that differ in one byte only, with constant digits, cut, and on 2^20 + 37 uniform tags loaded in two chunks.  The smallest herd: 64 kangaroos.
Then bsgs_mi355x end to end at the shape of tests/test_gpu_kangaroo_tames_cli.py (range 2^35 .. +2^36, dp 6, 512 kangaroos, the same eight planted keys): a table
of 4096 entries planned for 16384 is extended to 16384, and twice to 8192 with two seeds and merged; the readers accept the results and the searches find the keys."""
import os
import re
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_tames_extend_cases as XC
import kangaroo_tames_extend_model as XM
import kangaroo_tames_gen_model as GM
import kangaroo_tames_model as TM
import kangaroo_tames_sym_model as TS
from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

LOAD_CASES = XC.load_cases()
SORT_CASES = XC.sort_cases()


@pytest.fixture(scope="module")
def jump_table():
    return K.jump_table(K.Stream(11), 1 << 30)


@pytest.fixture(scope="module")
def dev(jump_table):
    import pybsgs
    d = pybsgs.Device(0)
    scalars, jumps = jump_table
    d.kangaroo_setup(jumps, scalars, 0, XC.HERD, 1, XC.CAP)
    yield d
    d.close()


def check_table(dev, table):
    """what the device holds is the model's tag set, each tag with one of its candidate offsets, by both reads"""
    got = dev.kangaroo_tames_gen_read()
    assert len(got) == GM.entries(table) and sorted(t for t, _ in got) == sorted(table["cand"])
    assert all(d in table["cand"][t] for t, d in got)
    srt, n = dev.kangaroo_tames_gen_read_sorted()
    assert n == len(got) and srt == sorted(got)
    return dict(got)


@pytest.mark.parametrize("case", sorted(LOAD_CASES))
def test_load(dev, case):
    dev.kangaroo_tames_gen_begin(XC.CAPACITY)
    table = GM.new_table(XC.CAPACITY, XC.CAP)
    for what, items in LOAD_CASES[case]:
        if what == "insert":
            table, want = GM.insert(table, items)
            back, n_entries = dev.kangaroo_tames_gen_insert(items)
            assert len(back) == sum(want.values()) and n_entries == GM.entries(table)
        else:
            table, want = XM.load(table, items)
            stored, dup, zero, full, n_entries = dev.kangaroo_tames_gen_load([t for t, _ in items], [d for _, d in items])
            print(case, "device", (stored, dup, zero, full, n_entries), "model", want)
            assert {"stored": stored, "duplicate": dup, "zero": zero, "full": full} == want
            assert stored + dup + zero + full == len(items) and n_entries == GM.entries(table)
    stored = check_table(dev, table)
    if case == "equal_tags":                                          # exactly one of the copies is stored
        x, y = LOAD_CASES[case][0][1][0][0], LOAD_CASES[case][0][1][64 + 5][0]
        assert stored[x] in range(1000, 1064) and stored[y] in {1000 + 64 * w + 5 for w in range(1, 9)}


def test_the_insert_and_the_walk_see_loaded_tags(dev, jump_table):
    scalars, jumps = jump_table
    states = [(p[0], p[1], t, 0) for t in range(1, 65) for p in [K.start(None, t, False)]]
    want_states, recs = K.walk(states, jumps, scalars, 1, 0)          # dp 0: one record per kangaroo and step
    assert len(recs) == 64 and not any(fl & K.DEAD for _, _, _, fl, _ in recs)
    walk_tags = sorted({x & GM.M64 for x, _, _, _, _ in recs})
    dev.kangaroo_tames_gen_begin(XC.CAPACITY)
    table = GM.new_table(XC.CAPACITY, XC.CAP)
    table, want = XM.load(table, [(t, XC.f(t)) for t in walk_tags])
    assert dev.kangaroo_tames_gen_load(walk_tags, [XC.f(t) for t in walk_tags]) == (len(walk_tags), 0, 0, 0, len(walk_tags))
    # an insert of records: a loaded tag is a duplicate, a new one is stored
    new = 0x5555555555555555
    assert new not in walk_tags
    back, n_entries = dev.kangaroo_tames_gen_insert([(walk_tags[3], 1, 0), (new, 2, 0)])
    assert [(r["x"], r["reason"]) for r in back] == [(walk_tags[3], GM.GEN_DUPLICATE)] and n_entries == len(walk_tags) + 1
    # the walk behind a load: the herd has not moved, and every record of the launch finds its tag there
    dev.kangaroo_upload(0, states)
    got, seen, n_entries, dropped, _ = dev.kangaroo_run_tames_gen(1)
    assert seen == 64 and dropped == 0 and n_entries == len(walk_tags) + 1
    assert sorted(r["x"] & GM.M64 for r in got) == sorted(x & GM.M64 for x, _, _, _, _ in recs) and {r["reason"] for r in got} == {GM.GEN_DUPLICATE}
    assert dev.kangaroo_download(0, 64) == want_states
    stored = dict(dev.kangaroo_tames_gen_read())
    assert stored == {**{t: XC.f(t) for t in walk_tags}, new: 2}


@pytest.mark.parametrize("case", sorted(SORT_CASES))
def test_sorted_read(dev, case):
    tags, cut = SORT_CASES[case]
    dev.kangaroo_tames_gen_begin(max(1, len(tags)))
    table, want = XM.load(GM.new_table(max(1, len(tags)), XC.CAP), [(t, XC.f(t)) for t in tags])
    assert dev.kangaroo_tames_gen_load(tags, [XC.f(t) for t in tags]) == (len(tags), 0, 0, 0, len(tags))
    model, n_model = XM.read_sorted(table, cut)
    got, n = dev.kangaroo_tames_gen_read_sorted(cut)
    assert n == n_model == len(tags)                                  # always the full count
    assert got == [(t, next(iter(c))) for t, c in model] == [(t, XC.f(t)) for t in sorted(tags)[:cut]]
    assert sorted(dev.kangaroo_tames_gen_read()) == [(t, XC.f(t)) for t in sorted(tags)]      # the table was only read
    assert dev.kangaroo_tames_gen_read_sorted(cut) == (got, n)


def test_sorted_read_of_two_chunks_of_uniform_tags(dev):
    import numpy as np
    n = XM.LOAD_CHUNK + 37                                            # no multiple of the wave or of the staging chunk
    rng = np.random.default_rng(5)
    tags = np.unique(rng.integers(1, 1 << 63, size=n + 4096, dtype=np.uint64) * np.uint64(2) + np.uint64(1))
    assert len(tags) >= n
    tags = rng.permutation(tags)[:n]
    d = np.empty((n, 2), dtype=np.uint64)
    d[:, 0] = tags * np.uint64(0x9E3779B97F4A7C15)
    d[:, 1] = tags ^ np.uint64(0xA5A5A5A5A5A5A5A5)
    dev.kangaroo_tames_gen_begin(n)
    assert dev.kangaroo_tames_gen_load(tags.tobytes(), d.tobytes()) == (n, 0, 0, 0, n)
    order = np.argsort(tags)
    (tb, db), count = dev.kangaroo_tames_gen_read_sorted(raw=True)
    assert count == n and tb == tags[order].tobytes() and db == d[order].tobytes()
    # the same pairs once more: every one a duplicate, the table as it was
    assert dev.kangaroo_tames_gen_load(tags.tobytes(), d.tobytes()) == (0, n, 0, 0, n)
    cut = 3 * XM.SORT_TILE + 1
    (tb, db), count = dev.kangaroo_tames_gen_read_sorted(cut, raw=True)
    assert count == n and tb == tags[order][:cut].tobytes() and db == d[order][:cut].tobytes()
    dev.kangaroo_tames_gen_begin(XC.CAPACITY)                         # (the large table is released)


def test_states(jump_table):
    import pybsgs
    scalars, jumps = jump_table
    d = pybsgs.Device(0)
    try:
        for call in (lambda: d.kangaroo_tames_gen_load([1], [1]), d.kangaroo_tames_gen_read_sorted):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_setup first"):
                call()
        d.kangaroo_setup(jumps, scalars, 0, 64, 1, 64)
        for call in (lambda: d.kangaroo_tames_gen_load([1], [1]), d.kangaroo_tames_gen_read_sorted):
            with pytest.raises(pybsgs.BsgsError, match="error -3: bsgs_kangaroo_tames_gen_begin first"):
                call()
        d.kangaroo_tames_gen_begin(64)
        assert d.kangaroo_tames_gen_read_sorted() == ([], 0)
        assert d.kangaroo_tames_gen_load([5, 6, 5, 0], [1, 2, 3, 4]) == (2, 1, 1, 0, 2)
        assert d.kangaroo_tames_gen_read_sorted(0) == ([], 2)         # the count alone
        got, n = d.kangaroo_tames_gen_read_sorted(1)
        assert n == 2 and len(got) == 1 and got[0][0] == 5 and got[0][1] in (1, 3)
    finally:
        d.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
LO, W = 1 << 35, 1 << 36
SEED = "0x7a3e5"
WALK = ["-dp", "6", "-kn", "512"]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def run_host(args, cwd, ranged=True, timeout=300):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    rng = ["-pk", "%x" % LO, "-pke", "%x" % (LO + W - 1)] if ranged else []
    r = subprocess.run([EXE, "-kangaroo", "-dir", str(cwd)] + rng + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def planted():
    """the keys of tests/test_gpu_kangaroo_tames_cli.py"""
    rng = K.Stream(836)
    ks = [LO + 1 + rng.u64() % ((1 << 20) - 1), LO + W - 1 - rng.u64() % ((1 << 20) - 1)]
    while len(ks) < 8:
        k = LO + 1 + rng.u128() % (W - 1)
        if k not in ks:
            ks.append(k)
    return ks[2:5] + ks[:1] + ks[5:] + ks[1:2]


def finds_the_keys(tmp_path, table, flag, entries):
    ks = planted()
    tmp_path.mkdir(exist_ok=True)
    (tmp_path / "keys.txt").write_text("\n".join(compressed(mul(k)) for k in ks) + "\n")
    out = run_host([flag, str(table), "-infile", str(tmp_path / "keys.txt"), "-kn", "512", "-kseed", SEED], tmp_path)
    assert "Found 8 of 8" in out and "[verify] tame table: %d entries" % entries in out
    lines = (tmp_path / "win.txt").read_bytes().decode().split("\r\n")
    keys = sorted(int(ln.split(": 0x")[1], 16) for ln in lines if ln.startswith("KEY["))
    assert keys == sorted(ks)
    assert re.search(r"\(0 dropped\), \d+ matches, 0 false matches", out), out[-1500:]


def steps_of(out):
    return float(re.search(r"Tame table \S+: \d+ entries, ([0-9.e+]+) steps", out).group(1))


def parse(path, model=TM):
    with open(path, "rb") as f:
        return model.parse_file(f.read())


def same_walk(a, b):
    return all(a[k] == b[k] for k in a if k not in ("steps", "seed", "entries"))


def extended(base, out, T):
    """out holds T entries by base's walk, and every entry of base at or below out's last tag with its d"""
    assert len(out["entries"]) == T and same_walk(base, out) and out["steps"] > base["steps"]
    got = dict(out["entries"])
    last = out["entries"][-1][0]
    below = [(t, d) for t, d in base["entries"] if t <= last]
    assert below and all(got.get(t) == d for t, d in below)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """a table of 4096 entries whose walk is planned for 16384: (its path, its fields)"""
    d = tmp_path_factory.mktemp("tames_small")
    out = run_host(["-ktamesgen", "a.tames", "-ktamesdev", "-ktn", "4096", "-ktnplan", "16384", "-kseed", SEED] + WALK, d)
    assert "Plan: mean jump m = 32768," in out                        # the plan of 16384 entries (tests/test_gpu_kangaroo_tames_gen_cli.py), not of 4096
    print("steps: 4096 entries planned for 16384: %.4e" % steps_of(out))
    return d / "a.tames", parse(d / "a.tames")


def test_extend(tmp_path, small):
    path, a = small
    out = run_host(["-ktamesgen", "out.tames", "-ktamesdev", "-ktamesfrom", str(path), "-ktn", "16384", "-kseed", "0x11", "-kn", "512"], tmp_path, ranged=False)
    assert "Loaded 4096 entries of the table into GPU memory, 0 duplicates" in out and "[verify] tame table: 4096 entries" in out and "[verify] tame table: 16384 entries" in out
    f = parse(tmp_path / "out.tames")
    extended(a, f, 16384)
    assert f["seed"] == 0x11 and abs(f["steps"] - steps_of(out)) <= 1e-3 * f["steps"]
    print("steps: 4096 extended to 16384: %.4e in all (%.4e before)" % (f["steps"], a["steps"]))
    r = subprocess.run([EXE, "-selftest", "kangaroo-tames", str(tmp_path / "out.tames"), "%x" % LO, "%x" % (LO + W - 1)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "entries 16384" in r.stdout.split("\n") and r.stdout.strip().endswith("ok"), r.stderr
    finds_the_keys(tmp_path / "search", tmp_path / "out.tames", "-ktames", 16384)
    # the output may be the input: the table is read before anything is written
    run_host(["-ktamesgen", "out.tames", "-ktamesdev", "-ktamesfrom", "out.tames", "-ktn", "16400", "-kseed", "0x12", "-kn", "512", "-dp", "6"], tmp_path)
    extended(f, parse(tmp_path / "out.tames"), 16400)


def test_two_extensions_merged(tmp_path, small):
    path, a = small
    for seed in ("2", "3"):
        run_host(["-ktamesgen", "e%s.tames" % seed, "-ktamesdev", "-ktamesfrom", str(path), "-ktn", "8192", "-kseed", seed, "-kn", "512"], tmp_path, ranged=False)
    e2, e3 = parse(tmp_path / "e2.tames"), parse(tmp_path / "e3.tames")
    extended(a, e2, 8192)
    extended(a, e3, 8192)
    out = run_host(["-ktamesmerge", "e2.tames,e3.tames", "-ktamesgen", "m.tames"], tmp_path, ranged=False)
    union, dropped = XM.merge([e2["entries"], e3["entries"]])
    assert "%d distinct tags, %d dropped" % (len(union), dropped) in out and "[verify] tame table: %d entries" % len(union) in out
    assert 8192 < len(union) <= 2 * 8192 - 1 and dropped >= 1
    want = TM.pack_file(dp=e2["dp"], pk=e2["pk"], pke=e2["pke"], steps=e2["steps"] + e3["steps"], seed=2, m=e2["m"], scalars=e2["scalars"], entries=union)
    assert (tmp_path / "m.tames").read_bytes() == want
    print("steps: two extensions to 8192 merged: %d entries, %.4e + %.4e steps (%.4e of them the shared table's, counted twice)" % (len(union), e2["steps"], e3["steps"], a["steps"]))
    finds_the_keys(tmp_path / "search", tmp_path / "m.tames", "-ktames", len(union))


def test_the_symmetric_walk_extended(tmp_path):
    out = run_host(["-ktamesgen", "a.tames", "-kwalk", "sym", "-ktamesdev", "-ktn", "4096", "-ktnplan", "16384", "-kseed", SEED] + WALK, tmp_path)
    a = parse(tmp_path / "a.tames", TS)
    out = run_host(["-ktamesgen", "out.tames", "-kwalk", "sym", "-ktamesdev", "-ktamesfrom", "a.tames", "-ktn", "16384", "-kseed", "0x11", "-kn", "512"], tmp_path, ranged=False)
    assert "Loaded 4096 entries of the table into GPU memory, 0 duplicates" in out
    f = parse(tmp_path / "out.tames", TS)
    extended(a, f, 16384)
    assert f["R"] == 1024 and f["scale"] == 1.0
    print("steps: symmetric walk, 4096 extended to 16384: %.4e in all (%.4e before)" % (f["steps"], a["steps"]))
    finds_the_keys(tmp_path / "search", tmp_path / "out.tames", "-ktamessym", 16384)
