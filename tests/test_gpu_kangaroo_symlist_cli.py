"""GPU: bsgs_mi355x -kangaroo -infile -kwalk sym -- planted keys in one range found by one herd of the symmetric walk, saved to a version-4 work file and
continued with -wl, a herd that went wrong not saved, -kwalk sym with one key planning what -ksym plans, and the point of the feature in steps: the
symmetric list search against the plain one.  One host process at a time."""
import os
import re
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_symlist_workfile as WF
from pybsgs.ecpy import mul

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "bsgs-cuda_amd", "build")
EXE, EXE_TEST = os.path.join(BUILD, "bsgs_mi355x"), os.path.join(BUILD, "bsgs_mi355x_test")
# the bound of the step ratio: the model's mean over 36 runs, RATIO_MEAN +- RATIO_SE (tools/kangaroo_symlist_ratio.py), and the midpoint
# between it and 1 -- the construction of the plain list test's bound
RATIO_MEAN, RATIO_SE = 0.615, 0.027
RATIO_BOUND = (RATIO_MEAN + 1.0) / 2


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def run_host(args, cwd, lo, W, timeout=600, exe=EXE, env=None):
    assert os.path.exists(exe), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([exe, "-kangaroo", "-dir", str(cwd), "-pk", "%x" % lo, "-pke", "%x" % (lo + W - 1)] + args, capture_output=True, text=True,
                          timeout=timeout, env=dict(os.environ, **(env or {})))


def planted(n, seed, lo, W):
    rng = K.Stream(seed)
    ks = []
    while len(ks) < n:
        k = lo + 1 + rng.u128() % (W - 1)
        if k not in ks:
            ks.append(k)
    return ks


def write_keys(path, ks):
    path.write_text("\n".join(compressed(mul(k)) for k in ks) + "\n")
    return ["-infile", str(path), "-kwalk", "sym"]


def win_blocks(cwd):
    lines = (cwd / "win.txt").read_bytes().decode().split("\r\n")
    return {int(l[4:l.index("]")]): int(l.split("0x")[1], 16) for l in lines if l.startswith("KEY[")}, [l for l in lines if l.startswith("KEY[")]


def job_steps(out):
    return float(re.search(r"Job time [0-9.]+s, ([0-9.e+]+) kangaroo steps", out).group(1))


LO40, W40 = 0x7 << 90 | (0x3C << 40), 1 << 40


def four_keys():
    ks = planted(3, 40, LO40, W40)
    ks.insert(1, LO40 + W40 // 2)                                    # the middle of the range itself: solved before any device is opened, keeps its slot
    return ks


def test_cli_four_keys_with_the_default_plan(tmp_path):
    ks = four_keys()
    r = run_host(write_keys(tmp_path / "keys.txt", ks) + ["-kseed", "40"], tmp_path, LO40, W40)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "symmetric walk (negation map), 1024 jump points, jump scale 2" in r.stdout and "cycles retired" in r.stdout
    assert "Found 4 of 4" in r.stdout
    blocks, lines = win_blocks(tmp_path)
    assert len(lines) == 4 and blocks == {i + 1: k for i, k in enumerate(ks)}
    assert not (tmp_path / "kangaroo.work").exists()


def test_save_and_resume(tmp_path):
    """one launch, saved (rc 3): the file is version 4, its herd carries the keys beside the flags; -wl verifies herd and table, finds the rest and writes no
    solved key twice"""
    ks = four_keys()
    args = write_keys(tmp_path / "keys.txt", ks) + ["-kn", "4096", "-dp", "4"]
    r = run_host(args + ["-kseed", "9", "-ksteps", "1"], tmp_path, LO40, W40)
    assert r.returncode == 3, r.stdout[-3000:] + r.stderr[-2000:]
    w = WF.read(tmp_path / "kangaroo.work")
    assert (w["version"], w["jumps"], w["jumpscale"], len(w["keys"])) == (4, 1024, 2.0, 4)
    assert w["keys"][1] == ks[1] and w["steps"] >= 4096 * 32 and w["steps"] % 4096 == 0 and w["entries"]      # a launch is longer than twice the cycle window
    herd = w["herds"][0]
    assert len(herd) == 4096 and all(s[4] == 0 and not s[3] & K.WILD for s in herd[:2048])
    assert {s[4] for s in herd[2048:]} == {0, 2, 3} and all(s[3] & K.WILD for s in herd[2048:])          # the keys beside the flags; key 1 has no kangaroo
    assert {e[3] for e in w["entries"]} <= {0, 1, 3, 4} and any(e[4] for e in w["entries"])                                # owners; some entry of a NEG kangaroo
    first = win_blocks(tmp_path)[1]
    assert len(first) >= 1
    r = run_host(args + ["-wl", "kangaroo.work"], tmp_path, LO40, W40)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "Resumed:" in r.stdout and "Found 4 of 4" in r.stdout
    assert "[verify] herd 0: 4096 kangaroos at their offsets" in r.stdout and "[verify] table: %d entries" % len(w["entries"]) in r.stdout
    blocks, lines = win_blocks(tmp_path)
    assert len(lines) == 4 and len(set(l.split(":")[0] for l in lines)) == 4 and lines[:len(first)] == first
    assert blocks == {i + 1: k for i, k in enumerate(ks)}
    assert not (tmp_path / "kangaroo.work").exists()


def test_a_herd_that_went_wrong_is_not_saved(tmp_path):
    """the test build flips bit 0 of the offset of kangaroo 3000 (a wild one) after the first launch: the save that -ksteps asks for does not happen"""
    args = write_keys(tmp_path / "keys.txt", four_keys()) + ["-kseed", "9", "-kn", "4096", "-dp", "4", "-ksteps", "1"]
    (tmp_path / "kangaroo.work").write_bytes(b"an earlier file")
    r = run_host(args, tmp_path, LO40, W40, exe=EXE_TEST, env={"BSGS_TEST_CORRUPT_KANGAROO": "3000"})
    assert r.returncode not in (0, 3), r.stdout[-1500:] + r.stderr[-800:]
    assert "herd of engine 0 failed verification at kangaroo 3000: kangaroo.work left as it was" in r.stderr, r.stderr[-800:]
    assert (tmp_path / "kangaroo.work").read_bytes() == b"an earlier file" and not (tmp_path / "kangaroo.temp").exists()


def test_kwalk_sym_with_one_key_plans_what_ksym_plans(tmp_path):
    """the printed plan lines of -kwalk sym -pb against -ksym.  A GPU test although it checks the command line: the plan needs the device's CU count, so the
    host prints it only after it has opened one; without a GPU tests/test_kangaroo_symlist_cli.py can check no more than that both spellings are accepted"""
    pub = compressed(mul(LO40 + 0x123456789))
    outs = []
    for sub, flag in (("a", ["-ksym"]), ("b", ["-kwalk", "sym"]), ("c", ["-kwalk", "plain"])):
        d = tmp_path / sub
        d.mkdir()
        r = run_host(["-pb", pub, "-kseed", "77", "-ksteps", "1", "-dir", str(d)] + flag, d, LO40, W40)
        assert r.returncode in (0, 3), r.stdout[-1500:] + r.stderr[-800:]
        outs.append([l for l in r.stdout.split("\n") if l.startswith(("Kangaroo", "Expected steps"))])
    assert outs[0] == outs[1] and len(outs[0]) >= 4 and any("symmetric walk (negation map), 1024 jump points, jump scale 2" in l for l in outs[0])
    assert outs[2] != outs[0] and not any("symmetric" in l for l in outs[2])


def test_the_symmetric_list_search_costs_fewer_steps_than_the_plain_one(tmp_path):
    """16 planted keys in [2^47, 2^47 + 2^48): the same -kseed, -kn and -dp with -kwalk sym and with the plain walk"""
    lo, W = 1 << 47, 1 << 48
    ks = planted(16, 4748, lo, W)
    plan = ["-kn", "4096", "-dp", "4", "-kseed", "1000"]
    steps = []
    for sub, walk in (("sym", "sym"), ("plain", "plain")):
        d = tmp_path / sub
        d.mkdir()
        r = run_host(write_keys(tmp_path / "keys.txt", ks)[:2] + ["-kwalk", walk] + plan + ["-dir", str(d)], d, lo, W)
        assert r.returncode == 0 and "Found 16 of 16" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
        assert win_blocks(d)[0] == {i + 1: k for i, k in enumerate(ks)}
        steps.append(job_steps(r.stdout))
    print("steps: symmetric %.4e, plain %.4e, ratio %.3f (bound %.3f)" % (steps[0], steps[1], steps[0] / steps[1], RATIO_BOUND))
    assert RATIO_MEAN + 3 * RATIO_SE < 1.0                           # the model's mean lies three standard errors below 1: the bound stands
    assert steps[0] <= steps[1] * RATIO_BOUND
