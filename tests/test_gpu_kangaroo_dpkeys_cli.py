"""GPU: bsgs_mi355x -kangaroo -infile -kdpkeys through the command line (host/host_kangaroo_list.h; DESIGN.md 10, "the table of a key list in device
memory"), plain and -kwalk sym: 16 planted keys in a 44-bit range found with nothing dropped and only the hand-backs over the bus; a 48-bit search of 16
keys stopped by -ksteps whose work file holds the device table -- as many entries as the header says, unique tags, the owner words of the list, entries that
stand at their offsets -- and resumes without the flag to all keys, as a file made without the flag resumes with it; a work file with a damaged table entry
is refused at -wl -kdpkeys by the verification's own line.  One host process at a time, each under its own time limit.

The plan of the 44-bit search, -dp 4 -kn 65536: tests/kangaroo_multi_model.py at dp 4 with the herd scaled to the range (16 keys; 24 bits, 64 kangaroos;
28 bits, 256 kangaroos; three seeds each) meets 25 .. 30 duplicates a search whatever the width -- 0.6 .. 0.9 % of the DPs at 24 bits, 0.13 .. 0.20 % at 28
bits, falling with sqrt(W) -- far below the 1/16 at which the pairs alone would reach the bound on the records over the bus."""
import os
import re
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_multi_workfile as WF3
import kangaroo_symlist_workfile as WF4
from pybsgs.ecpy import add, mul, neg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
WALKS = ["plain", "sym"]
LO44, W44 = 0x7 << 90 | (0xC3 << 44), 1 << 44
LO48, W48 = 0x3 << 100 | (0x5A << 48), 1 << 48
PLAN44 = ["-dp", "4", "-kn", "65536", "-kdpn", "16777216"]
PLAN48 = ["-dp", "8", "-kn", "65536"]                                 # (a dp at which the run without the flag keeps its DPs in the host's map)
TABLE48 = ["-kdpn", "16777216"]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def run_host(args, cwd, lo, W, timeout=300):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-dir", str(cwd), "-pk", "%x" % lo, "-pke", "%x" % (lo + W - 1)] + args, capture_output=True, text=True, timeout=timeout)


def planted(n, seed, lo, W):
    rng = K.Stream(seed)
    ks = []
    while len(ks) < n:
        k = lo + 1 + rng.u128() % (W - 1)
        if k not in ks:
            ks.append(k)
    return ks


def write_keys(path, ks, walk):
    path.write_text("\n".join(compressed(mul(k)) for k in ks) + "\n")
    return ["-infile", str(path), "-d", "0"] + (["-kwalk", "sym"] if walk == "sym" else [])


def win_blocks(cwd):
    lines = (cwd / "win.txt").read_bytes().decode().split("\r\n")
    return {int(l[4:l.index("]")]): int(l.split("0x")[1], 16) for l in lines if l.startswith("KEY[")}, [l for l in lines if l.startswith("KEY[")]


def closing(out):
    m = re.search(r"Job time [0-9.]+s, [0-9.e+]+ kangaroo steps, (\d+) DPs \((\d+) in the table, (\d+) dropped\)", out)
    assert m, out[-2000:]
    return tuple(int(v) for v in m.groups())


def all_found(r, cwd, ks):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "Found %d of %d" % (len(ks), len(ks)) in r.stdout
    blocks, lines = win_blocks(cwd)
    assert len(lines) == len(ks) and blocks == {i + 1: k for i, k in enumerate(ks)}
    assert not (cwd / "kangaroo.work").exists()


# ---- 6. sixteen planted keys -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
def test_sixteen_planted_keys(tmp_path, walk):
    ks = planted(16, 44, LO44, W44)
    r = run_host(write_keys(tmp_path / "keys.txt", ks, walk) + ["-kdpkeys", "-kseed", "0x44"] + PLAN44, tmp_path, LO44, W44)
    all_found(r, tmp_path, ks)
    assert "Kangaroo: 1 engine(s) x 65536 kangaroos" in r.stdout
    assert re.search(r"distinguished points stay in GPU memory \(-kdpkeys\): table of 16777216 entries, \d+ slots, [0-9.]+ GiB", r.stdout), r.stdout[:2500]
    dps, in_table, dropped = closing(r.stdout)
    assert dropped == 0 and 0 < in_table <= dps
    records = int(re.search(r"Engine 0 \(GPU #0\): (\d+) records", r.stdout).group(1))
    print("%s: %d DPs, %d in the table, %d records over the bus" % (walk, dps, in_table, records))
    assert records < dps // 8 + 64                                    # what crossed the bus is the hand-backs, not the walk's records


# ---- 7. the work file ----------------------------------------------------------------------------------------------------------------------------------------------
KS48 = planted(16, 48, LO48, W48)


def read_work(path, walk):
    return (WF4 if walk == "sym" else WF3).read(path)


def table_offset(w, walk):
    """where the table section of the parsed file begins"""
    head = 168 if walk == "sym" else 144
    return head + 4 + sum(1 + (32 if k is not None else 0) for k in w["keys"]) + 24 + (48 if walk == "sym" else 24) * len(w["links"])


@pytest.fixture(scope="module", params=WALKS)
def stopped(request, tmp_path_factory):
    """a 48-bit search of 16 keys with -kdpkeys stopped after its first launch, and the same search without the flag: (directory, output, parsed work file)
    each.  A seed whose first launch already solves everything is passed over (three are tried)."""
    walk = request.param
    for seed in ("0x48", "0x49", "0x4a"):
        made = {"walk": walk}
        for name, extra in (("dev", ["-kdpkeys"] + TABLE48), ("host", [])):
            d = tmp_path_factory.mktemp("%s_%s_%s" % (walk, name, seed))
            r = run_host(write_keys(d / "keys.txt", KS48, walk) + PLAN48 + ["-kseed", seed, "-ksteps", "1"] + extra, d, LO48, W48)
            if r.returncode == 0:
                break
            assert r.returncode == 3, r.stdout[-2500:] + r.stderr[-1000:]
            made[name] = (d, r.stdout, read_work(d / "kangaroo.work", walk))
        if len(made) == 3:
            return made
    raise AssertionError("all three seeds solved every key in their first launch")


def test_the_work_file_holds_the_device_table(stopped):
    walk = stopped["walk"]
    d, out, w = stopped["dev"]
    dps, in_table, dropped = closing(out)
    assert dropped == 0 and w["dropped"] == 0
    assert len(w["entries"]) == in_table > 1000                      # as many entries as the header says (the reader takes that many), "in the table"
    assert w["dps"] == dps >= in_table and w["version"] == (4 if walk == "sym" else 3) and w["dp"] == 8 and w["herd"] == 65536 and w["engines"] == 1
    tags = [e[0] for e in w["entries"]]
    assert len(set(tags)) == len(tags)
    # the owners are exactly the tame one and those of the sixteen keys, bit 31 only in version 4
    if walk == "sym":
        assert {e[3] for e in w["entries"]} == set(range(17)) and {e[4] for e in w["entries"]} == {False, True}
        assert not any(e[4] for e in w["entries"] if e[3] == 0)
    else:
        assert {e[3] for e in w["entries"]} == set(range(17))
    assert all(e[2] < 65536 and (e[3] != 0) == (e[2] >= 32768) for e in w["entries"])      # an owner's type is its half of the herd
    base = neg(mul(LO48 + W48 // 2 if walk == "sym" else LO48))
    for e in w["entries"][:: max(1, len(tags) // 12)]:                # a dozen entries stand at sigma * Q_k + d * G, with the top dp bits of x zero
        x64, dd, kid, owner = e[:4]
        if owner:
            Q = add(mul(KS48[owner - 1]), base)
            p = K.start(neg(Q) if walk == "sym" and e[4] else Q, dd, True)
        else:
            p = K.start(None, dd, False)
        assert p[0] & ((1 << 64) - 1) == x64 and K.is_dp(p[0], 8)
    assert "[verify] herd 0: 65536 kangaroos at their offsets" in out


def test_a_file_made_with_the_flag_resumes_without_it(stopped, tmp_path):
    walk = stopped["walk"]
    d, out, w = stopped["dev"]
    work = tmp_path / "saved.work"
    work.write_bytes((d / "kangaroo.work").read_bytes())
    (tmp_path / "win.txt").write_bytes((d / "win.txt").read_bytes() if (d / "win.txt").exists() else b"")
    r = run_host(write_keys(tmp_path / "keys.txt", KS48, walk) + ["-wl", str(work)], tmp_path, LO48, W48)
    all_found(r, tmp_path, KS48)
    assert "Resumed: %d steps, %d DPs" % (w["steps"], len(w["entries"])) in r.stdout
    assert re.search(r"\[verify\] table: %d entries" % len(w["entries"]), r.stdout)
    assert "-kdpkeys" not in r.stdout


def test_a_file_made_without_the_flag_resumes_with_it(stopped, tmp_path):
    walk = stopped["walk"]
    d, out, w = stopped["host"]
    assert len(w["entries"]) > 1000
    work = tmp_path / "saved.work"
    work.write_bytes((d / "kangaroo.work").read_bytes())
    (tmp_path / "win.txt").write_bytes((d / "win.txt").read_bytes() if (d / "win.txt").exists() else b"")
    r = run_host(write_keys(tmp_path / "keys.txt", KS48, walk) + ["-wl", str(work), "-kdpkeys"] + TABLE48, tmp_path, LO48, W48)
    all_found(r, tmp_path, KS48)
    assert "Resumed: %d steps, %d DPs" % (w["steps"], len(w["entries"])) in r.stdout
    assert re.search(r"\[verify\] table: %d entries" % len(w["entries"]), r.stdout)
    loaded = len(w["entries"]) - sum(1 for e in w["entries"] if e[0] == 0)
    assert re.search(r"\[startup\] table \(GPU memory\), %d entries" % loaded, r.stdout), r.stdout[:3000]
    dps, in_table, dropped = closing(r.stdout)
    assert dropped == 0 and in_table >= len(w["entries"])


def test_a_damaged_table_entry_is_refused(stopped, tmp_path):
    walk = stopped["walk"]
    d, out, w = stopped["dev"]
    data = bytearray((d / "kangaroo.work").read_bytes())
    data[table_offset(w, walk) + 32 * 3 + 8 + 2] ^= 0x04              # one bit of d of table entry 3
    work = tmp_path / "saved.work"
    work.write_bytes(bytes(data))
    assert read_work(work, walk)["entries"][3][1] == w["entries"][3][1] ^ 0x40000
    r = run_host(write_keys(tmp_path / "keys.txt", KS48, walk) + ["-wl", str(work), "-kdpkeys"] + TABLE48, tmp_path, LO48, W48)
    assert r.returncode not in (0, 3), r.stdout[-1500:] + r.stderr[-800:]
    assert "Recovery file is damaged: table entry 3 does not match its offset" in r.stderr, r.stderr[-800:]
    assert "table (GPU memory)" not in r.stdout and "Job time" not in r.stdout      # nothing was loaded, nothing walked
    assert work.read_bytes() == bytes(data) and not (tmp_path / "kangaroo.work").exists()
