"""CPU: the host's side of -kangaroo -kdpshard (host/host_kangaroo.cpp, host/host_kangaroo_dptable.h), no GPU: every refusal with its one line before any
device is looked for; -kdpshard -d 0,1 passes the command line; the plan of -selftest kangaroo-dpshard-plan is what the formulas of DESIGN.md 10 give for 1,
2, 3 and 8 engines, computed here from the formulas; -selftest kangaroo-dpshard gives, for the streams of tests/test_kangaroo_dpdev_cli.py spread over two
engines, the verdict lines of -selftest kangaroo / kangaroo-sym, and a re-seed names the engine and the index there."""
import math
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_dptable_model as DM
import kangaroo_dptable_shard_model as SM
from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")

A, W, KP = 0x1F << 36, 1 << 24, 0xABCDE
PUB = mul(A + KP)
CYCLE = 4
KN = 5                                                                # kangaroos per engine in the scripted streams: 1..4 are engine 0's, 5..9 engine 1's


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def host(args, cwd=None):
    assert os.path.exists(HOST), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([HOST] + args, capture_output=True, text=True, timeout=120, cwd=cwd)


RANGE = ["-pk", "%x" % A, "-pke", "%x" % (A + W - 1)]
SEARCH = ["-kangaroo", "-kdpshard", "-pb", compressed(PUB)] + RANGE
TAMES = "-kangaroo -kdpshard cannot be combined with -ktames, -ktamessym, -ktamesgen or their flags"


@pytest.mark.parametrize("args,message", [
    (["-kdpshard", "-pb", compressed(PUB)], "-kdpshard belongs to -kangaroo"),
    (SEARCH + ["-kdpdev"], "-kangaroo -kdpshard cannot be combined with -kdpdev"),
    (SEARCH + ["-kdpdev", "-d", "0,1"], "-kangaroo -kdpshard cannot be combined with -kdpdev"),
    (["-kangaroo", "-kdpshard", "-kdpkeys", "-infile", "keys.txt"] + RANGE, "-kangaroo -kdpshard cannot be combined with -kdpkeys"),
    (["-kangaroo", "-kdpshard", "-infile", "keys.txt"] + RANGE, "-kangaroo -kdpshard cannot be combined with -infile"),
    (SEARCH + ["-ktames", "none.tames"], TAMES),
    (SEARCH + ["-ktamessym", "none.tames"], TAMES),
    (["-kangaroo", "-kdpshard", "-ktamesgen", "out.tames", "-ktn", "64"] + RANGE, TAMES),
    (["-kangaroo", "-kdpshard", "-ktamesgen", "out.tames", "-ktamesdev", "-ktn", "64"] + RANGE, TAMES),
    (SEARCH + ["-kdpn", "0"], "-kdpn must be 1..2^31"),
])
def test_refusals(tmp_path, args, message):
    r = host(args + ["-dir", str(tmp_path)] if "-kangaroo" in args else args, cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode != 0 and len([ln for ln in out.split("\n") if message in ln]) == 1, out
    assert len([ln for ln in r.stderr.split("\n") if ln.strip()]) == 1, r.stderr      # the refusal is one line
    assert "No GPU found" not in out and "[startup]" not in out and "Kangaroo range" not in out, out      # refused before any device is looked for
    assert os.listdir(tmp_path) == []


def test_two_d_entries_pass_the_command_line(tmp_path):
    """what follows depends on the machine (no GPU ends the run there), but it is no refusal: -kdpshard takes several engines, and -kdpn belongs to it"""
    r = host(SEARCH + ["-d", "0,1", "-kdpn", "65536", "-ksteps", "1", "-dir", str(tmp_path)], cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert "cannot be combined" not in out and "takes one -d entry" not in out and "belongs to" not in out and "Unknown parameter" not in out, out
    assert "Kangaroo range" in out                                    # the mode got as far as its first line
    assert "No GPU found" in out or "bsgs_dev_count" in out or "engine(s)" in out, out      # it ended where the devices are looked for, or went on
    r = host(["-h"])
    assert "-kdpshard" in r.stdout
    assert "-kdpshard" in open(os.path.join(ROOT, "README.md")).read()


def plan(width_bits, engines, cus=256, min_launch=8, dp_arg=-1, kn_arg=0, kdpn=0):
    """DESIGN.md 10, "divided over engines", the plan: capacity per engine = -kdpn or the power of two at or above 4 sqrt(W) / E within [2^16, 2^27]; dp =
    max(0, ceil(log2(4 sqrt(W) / (E capacity)))) unless -dp; then plan_herd, which divides by the engines, and plan_launch, whose bound is per engine ->
    (dp, kn, per thread, S, record buffer, capacity, engines)"""
    sq = math.sqrt(float(1 << width_bits))
    capacity = kdpn
    if not capacity:
        capacity = 1 << 16
        while capacity < (1 << 27) and capacity < 4 * sq / engines:
            capacity *= 2
    dp = dp_arg if dp_arg >= 0 else int(min(32, max(0, math.ceil(math.log2(4 * sq / (engines * capacity))))))
    kn = kn_arg or int(min(float(cus * 1024 * 16), sq / 8 / 2 ** dp / engines))
    kn = max(kn, 64)
    g = 16
    while g > 1 and kn // g < cus * 512:
        g //= 2
    kn = max(64 * g, kn // (64 * g) * (64 * g))
    expected = 2 * sq + kn * engines * 2.0 ** dp
    s = int(max(min_launch, min(1024.0, expected / (kn * engines) / 8)))
    half = float(1 << 21)
    if kn * s / 2.0 ** dp > half:
        s = int(max(min_launch, math.floor(half * 2.0 ** dp / kn)))
    while dp_arg < 0 and kn * s / 2.0 ** dp > half and dp < 32:
        dp += 1
    cap = int(min(float(1 << 22), 2 * kn * s / 2.0 ** dp + 65536))
    return dp, kn, g, s, cap, capacity, engines


@pytest.mark.parametrize("bits", [44, 64, 80, 100])
@pytest.mark.parametrize("engines", [1, 2, 3, 8])
@pytest.mark.parametrize("dp_arg,kn_arg,kdpn", [(-1, 0, 0), (9, 0, 0), (-1, 1 << 20, 1 << 20)])
def test_plan(bits, engines, dp_arg, kn_arg, kdpn):
    want = plan(bits, engines, dp_arg=dp_arg, kn_arg=kn_arg, kdpn=kdpn)
    args = ["1", "%x" % (1 << bits), "256", "8", str(dp_arg), str(kn_arg), str(kdpn)]
    r = host(["-selftest", "kangaroo-dpshard-plan"] + args + [str(engines)])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["plan"] + [str(v) for v in want], (r.stdout, want)
    dp, kn, g, s, cap, capacity, _ = want
    if not kdpn and dp_arg < 0:                                       # the expected DPs fill at most half of the E tables together
        assert 2 * math.sqrt(float(1 << bits)) / 2 ** dp <= engines * capacity / 2
    if engines == 1:                                                  # one engine: -kdpdev's plan
        one = host(["-selftest", "kangaroo-dpdev-plan"] + args)
        assert one.returncode == 0 and one.stdout.split() == r.stdout.split()[:-1]


def test_plan_selftest_refuses_engines_out_of_range():
    args = ["1", "%x" % (1 << 64), "256", "8", "-1", "0", "0"]
    for engines in ("0", "17"):
        r = host(["-selftest", "kangaroo-dpshard-plan"] + args + [engines])
        assert r.returncode == 2 and r.stdout == "" and r.stderr.strip() == "kangaroo-dpshard-plan: %s engines, a table is divided over 1..16" % engines
    r = host(["-selftest", "kangaroo-dpshard-plan"] + args + ["16"])
    assert r.returncode == 0 and r.stdout.split()[-1] == "16" and r.stderr == ""


def barrier(events):
    r = host(["-selftest", "kangaroo-barrier"] + events.split())
    assert r.returncode == 0, r.stderr
    return r.stdout.split("\n")[:-1]


def test_the_save_barrier_does_not_hang_when_a_round_is_given_up():
    """the barrier in front of the last drain before a save (SaveBarrier, host/host_kangaroo_run.h), scripted for two engines.  Nothing here may end with an
    engine that waits for good."""
    # a save round: nobody passes before both have arrived, then both pass; the next round starts from nothing
    assert barrier("open A B withdraw open B A") == ["A=- B=-", "A=wait B=-", "A=all B=all", "A=- B=-", "A=- B=-", "A=- B=wait", "A=all B=all"]
    # a signal in the middle of a round: A waits for B, which is in a launch; the saver takes its request back, then the run is stopped.  A is let go, B
    # arrives in the stop round and waits for A, which comes: both pass
    assert barrier("open A withdraw stop B A") == ["A=- B=-", "A=wait B=-", "A=given-up B=-", "A=- B=-", "A=- B=wait", "A=all B=all"]
    # the stop comes while the request still stands (-ksteps, a search given up): the same
    assert barrier("open A stop B A") == ["A=- B=-", "A=wait B=-", "A=given-up B=-", "A=- B=wait", "A=all B=all"]
    # a newer round never counts an arrival of an older one
    assert barrier("open A withdraw open B") == ["A=- B=-", "A=wait B=-", "A=given-up B=-", "A=- B=-", "A=- B=wait"]
    assert barrier("open A withdraw open B A")[-1] == "A=all B=all"
    # the stop round counts living engines: one that has passed and ended does not hold the other back, nor does one that ended before
    assert barrier("stop A exitB") == ["A=- B=-", "A=wait B=-", "A=all B=-"]
    assert barrier("stop A B exitA") == ["A=- B=-", "A=wait B=-", "A=all B=all", "A=- B=-"]
    assert host(["-selftest", "kangaroo-barrier", "open", "A", "A"]).returncode == 2      # (an engine that waits cannot arrive)


FLAGS = {"T": 0, "W": K.WILD, "N": K.WILD | DM.NEG, "D": K.DEAD, "C": K.DEAD | CYCLE}


def through_the_shards(recs):
    """the logical stream (letter, x, d, global kangaroo) as -kdpshard's collector sees it: one launch per record on the engine that owns the kangaroo,
    through the model of the divided table with the relay -> (the items of -selftest kangaroo-dpshard, the positions of the records a table stored)"""
    tables = [DM.new_table(64, 64), DM.new_table(64, 64)]
    items, silent = [], set()
    for pos, (t, x, d, kid) in enumerate(recs):
        e = kid // KN
        launches = [[], []]
        launches[e] = [(x & DM.M64, d & K.M128, FLAGS[t], kid % KN)]
        tables, backs = SM.relay(tables, launches, [0, KN])
        back = backs[0] + backs[1]
        if not back:
            silent.add(pos)
            continue
        (reason, rec, stored), = back
        assert rec[3] == kid                                          # what comes back names the kangaroo by its global id
        if reason == DM.DPT_DUPLICATE:
            (tag, sd, skid, stype), = stored
            items.append("S,%x,%x,%d,%d" % (tag, sd, skid, stype))
        items.append("%s,%x,%x,%d" % (t, x, d & K.M128, kid))
    assert all(SM.shard(tag, 2) == s for s, tb in enumerate(tables) for tag in tb["cand"])
    return items, silent


def compare(selftest, sym, recs):
    args = ["%x" % A, "%x" % (A + W - 1), compressed(PUB)]
    r = host(["-selftest", selftest] + args + ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in recs])
    assert r.returncode == 0, r.stderr
    plain = r.stdout.split("\n")[:-1]
    items, silent = through_the_shards(recs)
    assert silent and all(plain[p] == "new" for p in silent)
    r = host(["-selftest", "kangaroo-dpshard"] + (["sym"] if sym else []) + ["2", str(KN)] + args + items)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]

    def named(line):                                                  # a re-seed of the host-only search, as -kdpshard names it: engine and index
        w = line.split()
        return "reseed %d %d" % (int(w[1]) // KN, int(w[1]) % KN) if w[0] == "reseed" else line

    assert got[:-1] == [named(ln) for p, ln in enumerate(plain[:-1]) if p not in silent]
    ps, gs = plain[-1].split(), got[-1].split()
    assert ps[0] == gs[0] == "summary" and ps[2:] == gs[2:] and int(gs[1]) == int(ps[1]) - len(silent)
    return got


def test_selftest_plain_gives_the_verdicts_of_the_host_only_search():
    d1, d2, d3 = 0x123456789ABC, 0x2222222222, 0x3333333333
    x1, x2, x3 = mul(d1)[0], mul(d2)[0], mul(d3)[0]
    x0 = (mul(d3)[0] >> 64) << 64
    recs = [("T", x1, d1, 1), ("W", x1, d1 - KP, 5), ("T", x1, d2, 2), ("T", x1, d1, 1), ("W", x2, d2, 6), ("T", x2, d2 + 5, 3), ("D", x3, d3, 4),
            ("T", x0, d3, 7), ("W", x0, d3 - KP, 8), ("T", x3, d3, 9)]
    got = compare("kangaroo", False, recs)
    assert got[:-1] == ["found %064x" % (A + KP), "reseed 0 2", "repeat", "false", "reseed 0 4", "new", "found %064x" % (A + KP)]


def test_selftest_sym_gives_the_verdicts_of_the_host_only_search():
    kk = KP - W // 2
    d1, d2, d3 = 0x123456789ABC, 0x2222222222, 0x3333333333
    x1, x2, x3, x4 = mul(d1)[0], mul(d2)[0], mul(d3)[0], mul(d1 + d2)[0]
    recs = [("W", x1, d1, 1), ("N", x1, d1 + 2 * kk, 2), ("T", x2, d2, 3), ("W", x2, d2 - kk, 4), ("T", x2, d3, 5), ("W", x2, d2 - kk, 3),
            ("C", x3, d3, 6), ("D", x3, d3, 7), ("N", x4, d1, 8), ("T", x4, d2, 9)]
    got = compare("kangaroo-sym", True, recs)
    assert [ln for ln in got if ln.startswith("reseed")] == ["reseed 1 0", "reseed 1 1", "reseed 1 2", "reseed 1 4"]
    assert got[-1].split()[2:] == ["1", "4", "1"]


def test_selftest_refuses_a_kangaroo_beyond_the_engines():
    args = ["%x" % A, "%x" % (A + W - 1), compressed(PUB)]
    assert host(["-selftest", "kangaroo-dpshard", "2", str(KN)] + args + ["D,5,1,10"]).returncode == 2
    r = host(["-selftest", "kangaroo-dpshard", "2", str(KN)] + args + ["D,5,1,9"])
    assert r.returncode == 0 and r.stdout.split("\n")[0] == "reseed 1 4"
