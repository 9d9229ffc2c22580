"""GPU: bsgs_mi355x -kangaroo -infile -- 16 planted keys in one 48-bit range found by one herd (one key equal to -pk, two equal to each other), two engines
on one GPU, -kcpuseed, and the point of the feature in steps: one search for the list against the sum of single-key searches."""
import os
import re
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_multi_workfile as WF
from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
LO, W = 0x3 << 100 | (0x5A << 48), 1 << 48
# the bound of the step ratio: the model's mean over 36 runs, 0.337 +- 0.016 (tools/kangaroo_multi_ratio.py), and the midpoint between it and 1
RATIO_BOUND = (0.337 + 1.0) / 2


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def run_host(args, cwd, timeout=600):
    assert os.path.exists(EXE), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([EXE, "-kangaroo", "-dir", str(cwd), "-pk", "%x" % LO, "-pke", "%x" % (LO + W - 1)] + args, capture_output=True, text=True, timeout=timeout)


def planted(n, seed):
    rng = K.Stream(seed)
    ks = []
    while len(ks) < n:
        k = LO + 1 + rng.u128() % (W - 1)
        if k not in ks:
            ks.append(k)
    return ks


def write_keys(path, ks):
    path.write_text("\n".join(compressed(mul(k)) for k in ks) + "\n")
    return ["-infile", str(path)]


def win_blocks(cwd):
    lines = (cwd / "win.txt").read_bytes().decode().split("\r\n")
    return {int(l[4:l.index("]")]): int(l.split("0x")[1], 16) for l in lines if l.startswith("KEY[")}, [l for l in lines if l.startswith("KEY[")]


def job_steps(out):
    return float(re.search(r"Job time [0-9.]+s, ([0-9.e+]+) kangaroo steps", out).group(1))


def test_cli_sixteen_keys(tmp_path):
    ks = planted(13, 48)
    ks.insert(3, LO)                                                 # the start of the range itself
    ks.insert(9, ks[5])                                              # two equal keys
    ks.append(LO + W - 1)
    assert len(ks) == 16
    r = run_host(write_keys(tmp_path / "keys.txt", ks) + ["-kseed", "16"], tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "Found 16 of 16" in r.stdout
    blocks, lines = win_blocks(tmp_path)
    assert len(lines) == 16 and blocks == {i + 1: k for i, k in enumerate(ks)}


def test_cli_two_engines_and_cpuseed(tmp_path):
    ks = planted(4, 4)
    args = write_keys(tmp_path / "keys.txt", ks) + ["-kseed", "4"]
    for extra, sub in ((["-d", "0,0"], "two"), (["-kcpuseed", "-kn", "4096", "-dp", "4"], "cpu")):
        d = tmp_path / sub
        d.mkdir()
        r = run_host(args + extra + ["-dir", str(d)], d)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert "Found 4 of 4" in r.stdout and ("2 engine(s)" in r.stdout) == (sub == "two")
        assert win_blocks(d)[0] == {i + 1: k for i, k in enumerate(ks)}


def selftest_work(path):
    r = subprocess.run([EXE, "-selftest", "kangaroo-work", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(l.split(" ", 1) for l in r.stdout.split("\n") if " " in l)


def test_cpuseed_starts_the_same_herd_as_the_gpu_seed(tmp_path):
    """one launch (-ksteps 1, saved, rc 3) from the same seed and plan: the host's comb and the kernel must leave byte-identical herds and tables"""
    ks = planted(4, 5)
    args = write_keys(tmp_path / "keys.txt", ks) + ["-kseed", "5", "-kn", "4096", "-dp", "4", "-ksteps", "1"]
    files = []
    for sub, extra in (("gpu", []), ("cpu", ["-kcpuseed"])):
        d = tmp_path / sub
        d.mkdir()
        r = run_host(args + extra + ["-dir", str(d)], d)
        assert r.returncode == 3, r.stdout[-3000:] + r.stderr[-2000:]
        files.append(WF.read(d / "kangaroo.work"))
    g, c = files
    assert g["herds"] == c["herds"] and len(g["herds"][0]) == 4096
    assert sorted(g["entries"]) == sorted(c["entries"]) and g["entries"]
    assert {s[3] >> 8 for s in g["herds"][0][2048:]} == {0, 1, 2, 3} and all(s[3] == 0 for s in g["herds"][0][:2048])


def test_resume_finds_the_rest(tmp_path):
    """the 16 keys, one launch, saved: the key equal to -pk is solved before any step, so the file holds a solved key and open ones; -wl finds the rest"""
    ks = planted(13, 48)
    ks.insert(3, LO)
    ks.insert(9, ks[5])
    ks.append(LO + W - 1)
    args = write_keys(tmp_path / "keys.txt", ks) + ["-kn", "4096", "-dp", "4"]
    r = run_host(args + ["-kseed", "9", "-ksteps", "1"], tmp_path)
    assert r.returncode == 3, r.stdout[-3000:] + r.stderr[-2000:]
    h = selftest_work(tmp_path / "kangaroo.work")
    assert h["version"] == "3" and h["keys"] == "16"
    assert 1 <= int(h["solved"]) < 16, h                              # at least one solved key and one open key, by construction
    w = WF.read(tmp_path / "kangaroo.work")
    assert w["keys"][3] == LO and w["steps"] > 0
    first = win_blocks(tmp_path)[1]
    r = run_host(args + ["-wl", "kangaroo.work"], tmp_path)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "Resumed:" in r.stdout and "Found 16 of 16" in r.stdout
    blocks, lines = win_blocks(tmp_path)
    assert len(lines) == 16 and len(set(l.split(":")[0] for l in lines)) == 16 and lines[:len(first)] == first
    assert blocks == {i + 1: k for i, k in enumerate(ks)}
    assert not (tmp_path / "kangaroo.work").exists()


def test_one_search_for_the_list_costs_fewer_steps_than_single_searches(tmp_path):
    """14 distinct keys, none equal to -pk: total steps of the one -infile run over the sum of the single-key runs (same range, -dp, -kn; seeds fixed here)"""
    ks = planted(14, 1048)
    plan = ["-kn", "4096", "-dp", "4"]
    d = tmp_path / "list"
    d.mkdir()
    r = run_host(write_keys(tmp_path / "keys.txt", ks) + plan + ["-kseed", "1000", "-dir", str(d)], d)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    multi = job_steps(r.stdout)
    single = 0.0
    for i, k in enumerate(ks):
        d = tmp_path / ("one%d" % i)
        d.mkdir()
        r = run_host(["-pb", compressed(mul(k))] + plan + ["-kseed", str(2000 + i), "-dir", str(d)], d)
        assert r.returncode == 0, (i, r.stdout[-2000:] + r.stderr[-1000:])
        single += job_steps(r.stdout)
    ratio = multi / single
    print("steps: list %.4e, %d single runs %.4e, ratio %.3f (bound %.3f)" % (multi, len(ks), single, ratio, RATIO_BOUND))
    assert ratio < RATIO_BOUND
