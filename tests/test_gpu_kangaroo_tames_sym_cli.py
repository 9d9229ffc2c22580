"""GPU: bsgs_mi355x -kangaroo -ktamesgen -kwalk sym / -ktamessym end to end, at the shape of tests/test_gpu_kangaroo_tames_cli.py -- a version-2 table of
16384 distinguished points of one 36-bit range made once with the symmetric walk, eight planted keys (two of them within 2^20 = W / 2^16 of either end of the
range) found with it on one engine and on two, win.txt exact; its steps against those of the plain walk's table on the same keys and herd; a table with one
flipped bit stopped before any step; and each kind of table refused by the other walk."""
import os
import re
import subprocess

import pytest

import kangaroo_model as K
from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
LO, W = 1 << 35, 1 << 36
SEED = "0x7a3e5"
# the bound of the step ratio against the plain walk's table: the model's mean for exactly this shape over 24 seeds, 0.5953 +- 0.0544
# (tools/kangaroo_tames_sym_ratio.py, profiles/r21a_kangaroo_tames_sym_model_ratio.log), and the midpoint between it and 1, "no gain"
MODEL_MEAN, MODEL_SE = 0.5953, 0.0544
RATIO_BOUND = (MODEL_MEAN + 1.0) / 2
SYM_BYTES = 128 + 8 * 1024 + 24 * 16384
MEAN_JUMP = (1 << 32) // 90                                          # tests/kangaroo_tames_sym_model.py plan(W, 16384, 6, 512): E / (2 isqrt(2048))


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def run_host(args, cwd, timeout=300):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-dir", str(cwd), "-pk", "%x" % LO, "-pke", "%x" % (LO + W - 1)] + args, capture_output=True, text=True, timeout=timeout)


def planted():
    """the keys of tests/test_gpu_kangaroo_tames_cli.py"""
    rng = K.Stream(836)
    ks = [LO + 1 + rng.u64() % ((1 << 20) - 1), LO + W - 1 - rng.u64() % ((1 << 20) - 1)]      # within 2^20 of either end
    while len(ks) < 8:
        k = LO + 1 + rng.u128() % (W - 1)
        if k not in ks:
            ks.append(k)
    return ks[2:5] + ks[:1] + ks[5:] + ks[1:2]


def job_steps(out):
    return float(re.search(r"Job time [0-9.]+s, ([0-9.e+]+) kangaroo steps", out).group(1))


def win_blocks(cwd):
    lines = (cwd / "win.txt").read_bytes().decode().split("\r\n")
    return {int(ln[4:ln.index("]")]): int(ln.split("0x")[1], 16) for ln in lines if ln.startswith("KEY[")}, lines


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """the table of the symmetric walk, generated once: (its directory, the generator's output)"""
    d = tmp_path_factory.mktemp("tames_sym")
    r = run_host(["-ktamesgen", "kangaroo.tames", "-kwalk", "sym", "-ktn", "16384", "-dp", "6", "-kn", "512", "-kseed", SEED], d)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return d, r.stdout


@pytest.fixture(scope="module")
def made_plain(tmp_path_factory):
    """the plain walk's table of the same range, size and herd"""
    d = tmp_path_factory.mktemp("tames_plain")
    r = run_host(["-ktamesgen", "kangaroo.tames", "-ktn", "16384", "-dp", "6", "-kn", "512", "-kseed", SEED], d)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return d, r.stdout


def search(tmp_path, table_dir, flag="-ktamessym", extra=()):
    ks = planted()
    (tmp_path / "keys.txt").write_text("\n".join(compressed(mul(k)) for k in ks) + "\n")
    r = run_host([flag, str(table_dir / "kangaroo.tames"), "-infile", str(tmp_path / "keys.txt"), "-kn", "512", "-kseed", SEED] + list(extra), tmp_path)
    return ks, r


def test_generate_and_selftest(made):
    d, out = made
    assert sorted(os.listdir(d)) == ["kangaroo.tames"] and os.path.getsize(d / "kangaroo.tames") == SYM_BYTES
    assert "Plan: symmetric walk, 1024 jump points, jump scale 1, mean jump m = %d, tame starts reach E = 0x%064x past the half range, -dp 6" % (MEAN_JUMP, 1 << 32) in out
    m = re.search(r"Tame table \S+: 16384 entries, ([0-9.e+]+) steps, (\d+) DPs, (\d+) merges, [0-9.]+s", out)
    assert m, out[-1500:]
    assert 16384 * 64 * 0.8 < float(m.group(1)) < 16384 * 64 * 2.0
    r = subprocess.run([EXE, "-selftest", "kangaroo-tames", "sym", str(d / "kangaroo.tames"), "%x" % LO, "%x" % (LO + W - 1)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:5] == ["version 2", "dp 6", "pk %064x" % LO, "pke %064x" % (LO + W - 1), "entries 16384"]
    assert "mean jump %d\njumps 1024\njump scale 1\nok" % MEAN_JUMP in r.stdout
    # the offsets are those of representatives: of either sign
    blob = (d / "kangaroo.tames").read_bytes()
    signs = [blob[128 + 8 * 1024 + 24 * i + 23] >> 7 for i in range(16384)]
    assert 4096 < sum(signs) < 12288


@pytest.mark.parametrize("engines", [1, 2])
def test_eight_planted_keys(tmp_path, made, engines):
    ks, r = search(tmp_path, made[0], extra=["-d", "0,0"] if engines == 2 else [])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "Found 8 of 8" in r.stdout and "%d engine(s)" % engines in r.stdout and "[verify] tame table: 16384 entries" in r.stdout
    assert "Kangaroo: symmetric walk (negation map), 1024 jump points, jump scale 1, from the table" in r.stdout
    blocks, lines = win_blocks(tmp_path)
    assert blocks == {i + 1: k for i, k in enumerate(ks)}
    pairs = [ln for ln in lines if ln.startswith("KEY[") or ln.startswith("   Pub:")]
    assert len(pairs) == 16
    for i in range(0, 16, 2):
        n = int(pairs[i][4:pairs[i].index("]")])
        assert pairs[i] == "KEY[%d]: 0x%064x" % (n, ks[n - 1]) and pairs[i + 1] == " " * 3 + "Pub: " + compressed(mul(ks[n - 1]))
    assert re.search(r"Job time [0-9.]+s, [0-9.e+]+ kangaroo steps, \d+ records seen \(0 dropped\), \d+ matches, 0 false matches, \d+ re-seeds", r.stdout), r.stdout[-1500:]
    assert re.search(r"Symmetric walk: \d+ cycles retired", r.stdout)
    assert not (tmp_path / "kangaroo.work").exists()


def test_steps_against_the_plain_table(tmp_path, made, made_plain):
    a = tmp_path / "sym"
    a.mkdir()
    ks, r = search(a, made[0])
    assert r.returncode == 0 and "Found 8 of 8" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    sym = job_steps(r.stdout)
    b = tmp_path / "plain"
    b.mkdir()
    ks, r = search(b, made_plain[0], flag="-ktames")
    assert r.returncode == 0 and "Found 8 of 8" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    plain = job_steps(r.stdout)
    ratio = sym / plain
    print("search steps: with the symmetric walk's table %.4e, with the plain walk's table %.4e, ratio %.3f (model %.4f +- %.4f, bound %.3f)" %
          (sym, plain, ratio, MODEL_MEAN, MODEL_SE, RATIO_BOUND))
    assert ratio < RATIO_BOUND


def test_a_flipped_bit_stops_the_run_before_any_step(tmp_path, made):
    blob = bytearray((made[0] / "kangaroo.tames").read_bytes())
    entry = 9001
    blob[128 + 8 * 1024 + 24 * entry + 8 + 5] ^= 0x10                # one bit of the entry's d
    bad = tmp_path / "bad.tames"
    bad.write_bytes(bytes(blob))
    ks = planted()
    (tmp_path / "keys.txt").write_text("\n".join(compressed(mul(k)) for k in ks) + "\n")
    r = run_host(["-ktamessym", str(bad), "-infile", str(tmp_path / "keys.txt"), "-kn", "512", "-kseed", SEED], tmp_path)
    assert r.returncode != 0 and "Tame table is damaged: entry %d does not match its offset" % entry in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-1000:]
    assert "kangaroo steps" not in r.stdout and "steps/s" not in r.stdout and "KEY[" not in r.stdout
    assert bad.read_bytes() == bytes(blob)


def test_each_table_is_refused_by_the_other_walk(tmp_path, made, made_plain):
    ks, r = search(tmp_path, made[0], flag="-ktames")
    assert r.returncode != 0 and "tame table version 2, this program reads version 1" in r.stdout + r.stderr and "kangaroo steps" not in r.stdout
    ks, r = search(tmp_path, made_plain[0])
    assert r.returncode != 0 and "tame table version 1, this program reads version 2" in r.stdout + r.stderr and "kangaroo steps" not in r.stdout
