"""GPU: bsgs_mi355x -kangaroo -kdpshard through the command line (host/host_kangaroo.cpp KeyMode, host/host_kangaroo_dptable.h; DESIGN.md 10, "divided over
engines"), two engines on GPU 0 (-d 0,0): a planted 44-bit key, plain and -ksym, found with nothing dropped, two engines and two tables named; a 48-bit search
stopped by -ksteps 1 whose work file holds both shards -- 2 engines, unique tags, global kangaroo ids below 2 kn whose type is their half of their engine's
herd, entries that stand at their offsets, as many as "in the table" -- and resumes to the key with the flag and without it, as a file made by plain -d 0,0
resumes with the flag; and -kdpshard -d 0 alone finds the same key.  One host process at a time, each under its own time limit."""
import os
import re
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_workfile as WF
from pybsgs.ecpy import add, mul, neg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
LO48, BITS48 = 0x3 << 100 | (0x5A << 48), 48
KEY48 = LO48 + (1 << BITS48) // 3
SMALL = ["-kdpn", "1048576"]                                          # 2^20 entries per engine: dp 5 and 32768 kangaroos per engine at this width, by the plan's rule
KN, DP = 32768, 5


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def run_host(args, cwd, timeout=120):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-dir", str(cwd)] + args, capture_output=True, text=True, timeout=timeout)


def job(key, lo, bits, d="0,0"):
    return ["-pb", compressed(mul(key)), "-pk", "%x" % lo, "-pke", "%x" % (lo + (1 << bits) - 1), "-d", d]


def found(r, cwd, key):
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1000:]
    lines = (cwd / "win.txt").read_bytes().decode().split("\r\n")
    assert lines[0] == "KEY[1]: 0x%064x" % key and lines[1] == " " * 3 + "Pub: " + compressed(mul(key))
    assert not (cwd / "kangaroo.work").exists()


def closing(out):
    m = re.search(r"Job time [0-9.]+s, [0-9.e+]+ kangaroo steps, (\d+) DPs \((\d+) in the table, (\d+) dropped\)", out)
    assert m, out[-2000:]
    return tuple(int(v) for v in m.groups())


LO44, BITS44 = 0x7 << 90 | (0xC3 << 44), 44
KEY44 = LO44 + 0x5DEECE66D1 % (1 << BITS44)


@pytest.mark.parametrize("walk", ["plain", "sym"])
def test_a_planted_44_bit_key(tmp_path, walk):
    r = run_host(job(KEY44, LO44, BITS44) + ["-kdpshard", "-kseed", "0x44"] + (["-ksym"] if walk == "sym" else []), tmp_path)
    found(r, tmp_path, KEY44)
    assert "Kangaroo: 2 engine(s) x " in r.stdout
    assert re.search(r"distinguished points stay in GPU memory \(-kdpshard\): 2 tables, one per engine, of 8388608 entries, \d+ slots each, [0-9.]+ GiB in all", r.stdout), r.stdout[:2500]
    dps, in_table, dropped = closing(r.stdout)
    assert dropped == 0 and 0 < in_table <= dps
    engines = re.findall(r"Engine (\d) \(GPU #0\): (\d+) records, (\d+) routed to other engines", r.stdout)
    assert [e[0] for e in engines] == ["0", "1"]
    records, routed = sum(int(e[1]) for e in engines), sum(int(e[2]) for e in engines)
    print("%s: %d DPs, %d in the table, %d records to the collector, %d routed" % (walk, dps, in_table, records, routed))
    assert records < dps // 8 + 64                                    # what reached the collector is the hand-backs, not the walk's records
    assert dps // 4 < routed < 3 * dps // 4 + 64                      # about half of the points belong to the other engine


def test_one_engine_finds_the_same_key(tmp_path):
    r = run_host(job(KEY44, LO44, BITS44, "0") + ["-kdpshard", "-kseed", "0x44"], tmp_path)
    found(r, tmp_path, KEY44)
    assert "Kangaroo: 1 engine(s) x " in r.stdout and "(-kdpshard): 1 tables" in r.stdout
    assert re.search(r"Engine 0 \(GPU #0\): \d+ records, 0 routed to other engines", r.stdout)
    assert closing(r.stdout)[2] == 0


@pytest.fixture(scope="module")
def stopped(tmp_path_factory):
    """a 48-bit search with -kdpshard -d 0,0 stopped after its first launches, and the same search without the flag: (directory, output, parsed work file)
    each.  A seed whose first launch already finds the key is passed over (three are tried)."""
    for seed in ("0x48", "0x49", "0x4a"):
        made = {}
        for name, extra in (("shard", ["-kdpshard"] + SMALL), ("host", ["-kn", str(KN), "-dp", str(DP)])):
            d = tmp_path_factory.mktemp("%s_%s" % (name, seed))
            r = run_host(job(KEY48, LO48, BITS48) + ["-kseed", seed, "-ksteps", "1"] + extra, d)
            if r.returncode == 0:
                break
            assert r.returncode == 3, r.stdout[-2500:] + r.stderr[-1000:]
            made[name] = (d, r.stdout, WF.parse((d / "kangaroo.work").read_bytes(), states=False))
        if len(made) == 2:
            return made
    raise AssertionError("all three seeds found the key in their first launch")


def test_the_work_file_holds_both_shards(stopped):
    d, out, w = stopped["shard"]
    assert re.search(r"Kangaroo: 2 engine\(s\) x %d kangaroos \(\d+ per thread\), -dp %d, " % (KN, DP), out), out[:2500]
    dps, in_table, dropped = closing(out)
    assert dropped == 0 and w["dropped"] == 0 and "WARNING" not in out
    assert w["engines"] == 2 and w["version"] == 1 and w["dp"] == DP and w["herd"] == KN
    assert w["table"] == len(w["entries"]) == in_table > 1000        # the entry count is the header's, and what the closing line calls "in the table"
    assert w["dps"] == dps >= in_table
    tags = [e[0] for e in w["entries"]]
    assert len(set(tags)) == len(tags)
    assert {e[3] for e in w["entries"]} == {0, 1} and all(e[2] < 2 * KN for e in w["entries"])
    assert {e[2] // KN for e in w["entries"]} == {0, 1}
    assert all((e[3] == 1) == (e[2] % KN >= KN // 2) for e in w["entries"])      # the owner's type is its half of its engine's herd
    Q = add(mul(KEY48), neg(mul(LO48)))
    for x64, dd, kid, typ in w["entries"][:: max(1, len(tags) // 12)]:          # a dozen entries stand at their offsets, with the top dp bits of x zero
        p = K.start(Q, K.signed128(dd), typ == 1)
        assert p[0] & ((1 << 64) - 1) == x64 and K.is_dp(p[0], DP)
    for e in (0, 1):
        assert "[verify] herd %d: %d kangaroos at their offsets" % (e, KN) in out


@pytest.mark.parametrize("flag", [True, False])
def test_the_file_resumes_with_the_flag_and_without_it(stopped, tmp_path, flag):
    d, out, w = stopped["shard"]
    work = tmp_path / "saved.work"
    work.write_bytes((d / "kangaroo.work").read_bytes())
    r = run_host(job(KEY48, LO48, BITS48) + ["-wl", str(work)] + (["-kdpshard"] + SMALL if flag else []), tmp_path)
    found(r, tmp_path, KEY48)
    assert "Resumed: %d steps, %d DPs" % (w["steps"], w["table"]) in r.stdout
    assert re.search(r"\[verify\] table: %d entries" % w["table"], r.stdout)
    assert ("-kdpshard" in r.stdout) == flag
    if flag:
        loaded = [int(n) for n in re.findall(r"\[startup\] table \(GPU memory\), (\d+) entries", r.stdout)]
        assert len(loaded) == 2 and sum(loaded) == w["table"] - sum(1 for e in w["entries"] if e[0] == 0), r.stdout[:3000]
        assert closing(r.stdout)[2] == 0 and closing(r.stdout)[1] >= w["table"]


def test_a_file_made_without_the_flag_resumes_with_it(stopped, tmp_path):
    d, out, w = stopped["host"]
    assert w["table"] > 1000 and w["engines"] == 2
    work = tmp_path / "saved.work"
    work.write_bytes((d / "kangaroo.work").read_bytes())
    r = run_host(job(KEY48, LO48, BITS48) + ["-wl", str(work), "-kdpshard"] + SMALL, tmp_path)
    found(r, tmp_path, KEY48)
    assert "Resumed: %d steps, %d DPs" % (w["steps"], w["table"]) in r.stdout
    loaded = [int(n) for n in re.findall(r"\[startup\] table \(GPU memory\), (\d+) entries", r.stdout)]
    assert len(loaded) == 2 and sum(loaded) == w["table"] - sum(1 for e in w["entries"] if e[0] == 0), r.stdout[:3000]
    dps, in_table, dropped = closing(r.stdout)
    assert dropped == 0 and in_table >= w["table"]
