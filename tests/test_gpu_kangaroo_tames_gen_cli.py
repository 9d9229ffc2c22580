"""GPU: bsgs_mi355x -kangaroo -ktamesgen ... -ktamesdev end to end, at the shape of tests/test_gpu_kangaroo_tames_cli.py (range 2^35 .. +2^36, 16384 entries,
dp 6, 512 kangaroos, the same seed and the same eight planted keys): the table grown in device memory is a table like any other -- the readers accept it, the
verification at the end of generation is reported, -ktames finds the keys with it in as few steps as that test asks of the host-made table; the same once
for the symmetric walk with -ktamessym; and two -d entries are refused."""
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
# the bounds of tests/test_gpu_kangaroo_tames_cli.py and tests/test_gpu_kangaroo_tames_sym_cli.py: the model's mean for this shape and the midpoint between it
# and 1.  A table grown on the device is drawn from the same distribution as one collected by the host.
RATIO_BOUND = (0.3698 + 1.0) / 2                                     # search with the plain walk's table over the plain list search
RATIO_BOUND_SYM = (0.5953 + 1.0) / 2                                 # search with the symmetric walk's table over the search with the plain walk's
GEN = ["-ktn", "16384", "-dp", "6", "-kn", "512", "-kseed", SEED]


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


def generate(tmp_path_factory, name, extra):
    d = tmp_path_factory.mktemp(name)
    r = run_host(["-ktamesgen", "kangaroo.tames"] + GEN + extra, d)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return d, r.stdout


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """the plain walk's table, grown on the device, generated once: (its directory, the generator's output)"""
    return generate(tmp_path_factory, "tames_dev", ["-ktamesdev"])


@pytest.fixture(scope="module")
def made_sym(tmp_path_factory):
    return generate(tmp_path_factory, "tames_dev_sym", ["-kwalk", "sym", "-ktamesdev"])


@pytest.fixture(scope="module")
def made_host(tmp_path_factory):
    """the plain walk's table collected by the host: what the symmetric walk's table is measured against"""
    return generate(tmp_path_factory, "tames_host", [])


def search(tmp_path, table_dir, flag):
    ks = planted()
    (tmp_path / "keys.txt").write_text("\n".join(compressed(mul(k)) for k in ks) + "\n")
    r = run_host([flag, str(table_dir / "kangaroo.tames"), "-infile", str(tmp_path / "keys.txt"), "-kn", "512", "-kseed", SEED], tmp_path)
    return ks, r


def found_all(tmp_path, ks, r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "Found 8 of 8" in r.stdout and "1 engine(s)" in r.stdout and "[verify] tame table: 16384 entries" in r.stdout
    lines = (tmp_path / "win.txt").read_bytes().decode().split("\r\n")
    pairs = [ln for ln in lines if ln.startswith("KEY[") or ln.startswith("   Pub:")]
    assert len(pairs) == 16
    seen = set()
    for i in range(0, 16, 2):
        n = int(pairs[i][4:pairs[i].index("]")])
        seen.add(n)
        assert pairs[i] == "KEY[%d]: 0x%064x" % (n, ks[n - 1]) and pairs[i + 1] == " " * 3 + "Pub: " + compressed(mul(ks[n - 1]))
    assert seen == set(range(1, 9))
    assert re.search(r"\(0 dropped\), \d+ matches, 0 false matches", r.stdout), r.stdout[-1500:]


def generated(d, out, size, selftest):
    assert sorted(os.listdir(d)) == ["kangaroo.tames"] and os.path.getsize(d / "kangaroo.tames") == size
    assert "[verify] tame table: 16384 entries" in out
    m = re.search(r"Tame table \S+: 16384 entries, ([0-9.e+]+) steps, (\d+) DPs, (\d+) merges, [0-9.]+s", out)
    assert m, out[-1500:]
    assert 16384 * 64 * 0.8 < float(m.group(1)) < 16384 * 64 * 2.0 and int(m.group(2)) >= 16384
    m = re.search(r"Table grown on the GPU: (\d+) records inserted there, (\d+) handed back over the bus \(0 dropped\)", out)
    assert m and int(m.group(2)) <= int(m.group(1)) - 16384, out[-1500:]      # every record is stored or handed back, and 16384 at least were stored
    r = subprocess.run([EXE, "-selftest", "kangaroo-tames"] + selftest + [str(d / "kangaroo.tames"), "%x" % LO, "%x" % (LO + W - 1)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "entries 16384" in r.stdout.split("\n") and "dp 6" in r.stdout.split("\n") and r.stdout.strip().endswith("ok")


def test_generate_and_selftest(made):
    generated(made[0], made[1], 624 + 24 * 16384, [])
    assert "Plan: mean jump m = 32768, tame starts reach E = 0x%064x past the range, -dp 6" % (1 << 33) in made[1]


def test_eight_planted_keys_and_the_steps(tmp_path, made):
    a = tmp_path / "tames"
    a.mkdir()
    ks, r = search(a, made[0], "-ktames")
    found_all(a, ks, r)
    tames = job_steps(r.stdout)
    b = tmp_path / "plain"
    b.mkdir()
    r = run_host(["-infile", str(a / "keys.txt"), "-kn", "512", "-kseed", SEED], b)
    assert r.returncode == 0 and "Found 8 of 8" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    plain = job_steps(r.stdout)
    print("steps: search with the table grown on the device %.4e, plain list search %.4e, ratio %.3f (bound %.3f)" % (tames, plain, tames / plain, RATIO_BOUND))
    assert tames / plain < RATIO_BOUND


def test_the_symmetric_walk(tmp_path, made_sym, made_host):
    generated(made_sym[0], made_sym[1], 128 + 8 * 1024 + 24 * 16384, ["sym"])
    a = tmp_path / "sym"
    a.mkdir()
    ks, r = search(a, made_sym[0], "-ktamessym")
    found_all(a, ks, r)
    sym = job_steps(r.stdout)
    b = tmp_path / "plain"
    b.mkdir()
    ks, r = search(b, made_host[0], "-ktames")
    assert r.returncode == 0 and "Found 8 of 8" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    plain = job_steps(r.stdout)
    print("search steps: with the symmetric walk's table grown on the device %.4e, with the plain walk's table %.4e, ratio %.3f (bound %.3f)" % (sym, plain, sym / plain, RATIO_BOUND_SYM))
    assert sym / plain < RATIO_BOUND_SYM


def test_two_devices_are_refused(tmp_path):
    r = run_host(["-ktamesgen", "kangaroo.tames", "-ktamesdev", "-d", "0,0"] + GEN, tmp_path)
    assert r.returncode == 1 and "takes one -d entry" in r.stderr and os.listdir(tmp_path) == []
