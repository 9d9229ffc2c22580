"""GPU: bsgs_mi355x -kangaroo -kdpdev through the command line (host/host_kangaroo.cpp KeyMode; DESIGN.md 10, "the table of distinguished points in device
memory"): a planted 44-bit key, plain and -ksym, found with nothing dropped; a 48-bit search stopped by -ksteps whose work file holds the device table -- as many
entries as the header says, unique tags, entries that stand at their offsets -- and resumes without the flag to the key, as a file made without the flag
resumes with it; a work file with a damaged table entry is refused at -wl -kdpdev by the verification's own line.  One host process at a time, each under its
own time limit."""
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
SMALL = ["-kdpn", "1048576"]                                          # a table of 2^20 entries: dp 6 and a herd of 32768 at this width, by the plan's rule


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def run_host(args, cwd, timeout=120):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-dir", str(cwd)] + args, capture_output=True, text=True, timeout=timeout)


def job(key, lo, bits):
    return ["-pb", compressed(mul(key)), "-pk", "%x" % lo, "-pke", "%x" % (lo + (1 << bits) - 1), "-d", "0"]


def found(r, cwd, key):
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1000:]
    lines = (cwd / "win.txt").read_bytes().decode().split("\r\n")
    assert lines[0] == "KEY[1]: 0x%064x" % key and lines[1] == " " * 3 + "Pub: " + compressed(mul(key))
    assert not (cwd / "kangaroo.work").exists()


def closing(out):
    m = re.search(r"Job time [0-9.]+s, [0-9.e+]+ kangaroo steps, (\d+) DPs \((\d+) in the table, (\d+) dropped\)", out)
    assert m, out[-2000:]
    return tuple(int(v) for v in m.groups())


@pytest.mark.parametrize("walk", ["plain", "sym"])
def test_a_planted_44_bit_key(tmp_path, walk):
    lo, bits = 0x7 << 90 | (0xC3 << 44), 44
    key = lo + 0x5DEECE66D1 % (1 << bits)
    args = job(key, lo, bits)
    if walk == "sym":
        args = args[:-2]                                              # without -d: one engine on GPU #0 all the same, however many GPUs the machine has
    r = run_host(args + ["-kdpdev", "-kseed", "0x44"] + (["-ksym"] if walk == "sym" else []), tmp_path)
    found(r, tmp_path, key)
    assert "Kangaroo: 1 engine(s) x " in r.stdout and ("no -d given, one engine on GPU #0" in r.stdout) == (walk == "sym")
    assert re.search(r"distinguished points stay in GPU memory \(-kdpdev\): table of 16777216 entries, \d+ slots, [0-9.]+ GiB", r.stdout), r.stdout[:2500]
    dps, in_table, dropped = closing(r.stdout)
    assert dropped == 0 and 0 < in_table <= dps
    records = int(re.search(r"Engine 0 \(GPU #0\): (\d+) records", r.stdout).group(1))
    print("%s: %d DPs, %d in the table, %d records over the bus" % (walk, dps, in_table, records))
    assert records < dps // 8 + 64                                    # what crossed the bus is the hand-backs, not the walk's records


@pytest.fixture(scope="module")
def stopped(tmp_path_factory):
    """a 48-bit search with -kdpdev stopped after its first launch, and the same search without the flag: (directory, output, parsed work file) each.  A seed
    whose first launch already finds the key is passed over (three are tried)."""
    for seed in ("0x48", "0x49", "0x4a"):
        made = {}
        for name, extra in (("dev", ["-kdpdev"] + SMALL), ("host", ["-kn", "32768", "-dp", "6"])):
            d = tmp_path_factory.mktemp("%s_%s" % (name, seed))
            r = run_host(job(KEY48, LO48, BITS48) + ["-kseed", seed, "-ksteps", "1"] + extra, d)
            if r.returncode == 0:
                break
            assert r.returncode == 3, r.stdout[-2500:] + r.stderr[-1000:]
            made[name] = (d, r.stdout, WF.parse((d / "kangaroo.work").read_bytes(), states=False))
        if len(made) == 2:
            return made
    raise AssertionError("all three seeds found the key in their first launch")


def test_the_work_file_holds_the_device_table(stopped):
    d, out, w = stopped["dev"]
    assert re.search(r"Kangaroo: 1 engine\(s\) x 32768 kangaroos \(\d+ per thread\), -dp 6, ", out), out[:2500]
    dps, in_table, dropped = closing(out)
    assert dropped == 0 and w["dropped"] == 0
    assert w["table"] == len(w["entries"]) == in_table > 1000        # the entry count is the header's, and what the closing line calls "in the table"
    assert w["dps"] == dps >= in_table and w["version"] == 1 and w["dp"] == 6 and w["herd"] == 32768
    tags = [e[0] for e in w["entries"]]
    assert len(set(tags)) == len(tags)
    assert {e[3] for e in w["entries"]} == {0, 1} and all(e[2] < 32768 for e in w["entries"])
    assert all((e[3] == 1) == (e[2] >= 16384) for e in w["entries"])  # the owner's type is its half of the herd
    Q = add(mul(KEY48), neg(mul(LO48)))
    for x64, dd, kid, typ in w["entries"][:: max(1, len(tags) // 12)]:          # a dozen entries stand at their offsets, with the top dp bits of x zero
        p = K.start(Q, K.signed128(dd), typ == 1)
        assert p[0] & ((1 << 64) - 1) == x64 and K.is_dp(p[0], 6)
    assert "[verify] herd 0: 32768 kangaroos at their offsets" in out


def test_a_file_made_with_the_flag_resumes_without_it(stopped, tmp_path):
    d, out, w = stopped["dev"]
    work = tmp_path / "saved.work"
    work.write_bytes((d / "kangaroo.work").read_bytes())
    r = run_host(job(KEY48, LO48, BITS48) + ["-wl", str(work)], tmp_path)
    found(r, tmp_path, KEY48)
    assert "Resumed: %d steps, %d DPs" % (w["steps"], w["table"]) in r.stdout
    assert re.search(r"\[verify\] table: %d entries" % w["table"], r.stdout)
    assert "-kdpdev" not in r.stdout


def test_a_file_made_without_the_flag_resumes_with_it(stopped, tmp_path):
    d, out, w = stopped["host"]
    assert w["table"] > 1000
    work = tmp_path / "saved.work"
    work.write_bytes((d / "kangaroo.work").read_bytes())
    r = run_host(job(KEY48, LO48, BITS48) + ["-wl", str(work), "-kdpdev"] + SMALL, tmp_path)
    found(r, tmp_path, KEY48)
    assert "Resumed: %d steps, %d DPs" % (w["steps"], w["table"]) in r.stdout
    assert re.search(r"\[verify\] table: %d entries" % w["table"], r.stdout)
    loaded = w["table"] - sum(1 for e in w["entries"] if e[0] == 0)
    assert re.search(r"\[startup\] table \(GPU memory\), %d entries" % loaded, r.stdout), r.stdout[:3000]
    dps, in_table, dropped = closing(r.stdout)
    assert dropped == 0 and in_table >= w["table"]


def test_a_damaged_table_entry_is_refused(stopped, tmp_path):
    d, out, w = stopped["dev"]
    data = bytearray((d / "kangaroo.work").read_bytes())
    data[WF.HEADER + 32 * 3 + 8 + 2] ^= 0x04                          # one bit of d of table entry 3
    work = tmp_path / "saved.work"
    work.write_bytes(bytes(data))
    r = run_host(job(KEY48, LO48, BITS48) + ["-wl", str(work), "-kdpdev"] + SMALL, tmp_path)
    assert r.returncode not in (0, 3), r.stdout[-1500:] + r.stderr[-800:]
    assert "Recovery file is damaged: table entry 3 does not match its offset" in r.stderr, r.stderr[-800:]
    assert "table (GPU memory)" not in r.stdout and "Job time" not in r.stdout      # nothing was loaded, nothing walked
    assert work.read_bytes() == bytes(data) and not (tmp_path / "kangaroo.work").exists()
