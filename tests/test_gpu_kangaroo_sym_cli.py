"""GPU: bsgs_mi355x -kangaroo -ksym end to end (host_kangaroo.cpp): planted keys across the range and at both of its ends, the puzzle-64 vector,
two engines on one GPU, and a search stopped by -ksteps and carried to the key by -wl.  At most two GPU processes at a time: pytest and one host."""
import os
import re
import subprocess

import pytest

import kangaroo_sym_workfile as WF2
from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
PUB_PUZZLE64 = "03100611c54dfef604163b8358f7b7fac13ce478e02cb224ae16d45526b25d9d4d"
KEY_PUZZLE64 = 0xF7051F27B09112D4


def run_host(args, cwd, timeout=300):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-ksym", "-dir", str(cwd)] + args, capture_output=True, text=True, timeout=timeout)


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def job(key, lo, hi):
    return ["-pb", compressed(mul(key)), "-pk", "%x" % lo, "-pke", "%x" % hi]


def check_win(tmp_path, key, out):
    with open(os.path.join(tmp_path, "win.txt"), "rb") as f:
        lines = f.read().decode().split("\r\n")
    assert lines[0] == "KEY[1]: 0x%064x" % key
    assert lines[1] == " " * 3 + "Pub: " + compressed(mul(key))
    assert "KEY[1]: 0x%064x" % key in out
    assert "symmetric walk" in out and re.search(r"Symmetric walk: \d+ cycles retired", out)


def solve_cli(tmp_path, key, lo, hi, extra=()):
    r = run_host(job(key, lo, hi) + ["-kseed", "0x%x" % (key & 0xFFFF)] + list(extra), tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    check_win(tmp_path, key, r.stdout)
    return r.stdout


# the planted keys of test_gpu_kangaroo.py::test_cli_planted_keys, and a key at each end of a range (k'' = -W/2 and W/2 - 1: the ends of the symmetric interval)
@pytest.mark.parametrize("bits, where", [(40, "low"), (40, "high"), (48, "mid"), (56, "low"), (56, "high"), (64, "mid"), (44, "first"), (44, "last")])
def test_cli_planted_keys(tmp_path, bits, where):
    lo = 0x3 << 100 | (0x5A << bits)
    W = 1 << bits
    k = lo + {"low": 0, "first": 0, "high": W - 1, "last": W - 1, "mid": W // 3}[where]
    solve_cli(tmp_path, k, lo, lo + W - 1)


def test_cli_puzzle64(tmp_path):
    r = run_host(["-pb", PUB_PUZZLE64, "-pk", "8000000000000000", "-pke", "ffffffffffffffff", "-kseed", "64"], tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(os.path.join(tmp_path, "win.txt"), "rb").read().decode().split("\r\n")[0] == "KEY[1]: 0x%064x" % KEY_PUZZLE64


def test_cli_two_engines_share_one_table(tmp_path):
    lo = 0x77 << 60
    out = solve_cli(tmp_path, lo + 0x123456789ABC, lo, lo + (1 << 52) - 1, ["-d", "0,0"])
    assert "2 engine(s)" in out
    counts = [int(ln.split(": ")[1].split()[0]) for ln in out.split("\n") if ln.startswith("Engine ")]
    assert len(counts) == 2 and all(c > 0 for c in counts), out[-1500:]


def test_cli_ksteps_then_wl_to_the_key(tmp_path):
    """a third of the expected steps, saved as a version-2 work file whose herd carries the walk's flags; -wl -ksym continues to the key; plain mode refuses it"""
    lo = 0xABC << 64
    key = lo + 0x2F3A9C4D5E6B7
    args = job(key, lo, lo + (1 << 52) - 1)
    seed = 0x5151
    for seed in range(0x5151, 0x5159):
        for f in os.listdir(tmp_path):
            os.remove(os.path.join(tmp_path, f))
        plan = run_host(args + ["-kseed", hex(seed), "-ksteps", "1"], tmp_path)
        assert plan.returncode in (0, 3), plan.stdout[-2000:] + plan.stderr[-1000:]
        expected = 2.0 ** float(re.search(r"Expected steps: 2\^([0-9.]+)", plan.stdout).group(1))
        r1 = run_host(args + ["-kseed", hex(seed), "-ksteps", str(int(expected / 6))], tmp_path)
        if r1.returncode == 3:
            break
        assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-1000:]          # found before the budget: another seed
    assert r1.returncode == 3
    work = os.path.join(tmp_path, "kangaroo.work")
    w = WF2.parse(open(work, "rb").read())
    assert (w["version"], w["jumps"], w["engines"]) == (2, 1024, 1) and w["steps"] >= expected / 6 and w["jumpscale"] > 0
    flags = [s[3] for s in w["herds"][0]]
    live = [f for f in flags if not f & 0x80000000]
    assert live and all(f & 0x100 for f in live) and any(f & 2 for f in live)                 # last index valid everywhere, NEG on some wild ones
    assert all(s[1] & 1 == 0 for s in w["herds"][0] if not s[3] & 0x80000000)                # every live kangaroo stands on its class representative
    plain = subprocess.run([EXE, "-kangaroo", "-dir", str(tmp_path)] + args + ["-wl", work], capture_output=True, text=True, timeout=60)
    assert plain.returncode not in (0, 3) and "this host reads version 1" in plain.stderr
    r2 = run_host(args + ["-wl", work], tmp_path)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-1000:]
    assert "Resumed: %d steps" % w["steps"] in r2.stdout
    check_win(tmp_path, key, r2.stdout)
    assert not os.path.exists(work)


def test_cli_without_ksym_rejects_its_options(tmp_path):
    pub = compressed(mul(1 << 30))
    for extra in (["-kjumps", "1024"], ["-kjumpscale", "2"]):
        r = subprocess.run([EXE, "-kangaroo", "-dir", str(tmp_path), "-pb", pub] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, extra
