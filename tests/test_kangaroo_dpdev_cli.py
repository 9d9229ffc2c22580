"""CPU: the host's side of -kangaroo -kdpdev (host/host_kangaroo.cpp), no GPU: every refusal of the command line with its one line before any device is
looked for; -selftest kangaroo-dpdev, plain and sym, gives for the same logical stream the verdict lines of -selftest kangaroo / kangaroo-sym (the stream goes
through the device table's model, tests/kangaroo_dptable_model.py: what the device stores is silent, a duplicate arrives with the entry it met, DEAD and tag 0
arrive alone); and the plan of -kdpdev is what the formulas of DESIGN.md 10 give, computed here from the formulas."""
import math
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_dptable_model as DM
from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")

A, W, KP = 0x1F << 36, 1 << 24, 0xABCDE
PUB = mul(A + KP)
CYCLE = 4


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def host(args, cwd=None):
    assert os.path.exists(HOST), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([HOST] + args, capture_output=True, text=True, timeout=120, cwd=cwd)


SEARCH = ["-kangaroo", "-kdpdev", "-pb", compressed(PUB), "-pk", "%x" % A, "-pke", "%x" % (A + W - 1)]


@pytest.mark.parametrize("args,message", [
    (["-kdpdev", "-pb", compressed(PUB)], "-kdpdev belongs to -kangaroo"),
    (["-kdpn", "65536", "-pb", compressed(PUB)], "-kdpn belongs to -kangaroo"),
    (["-kangaroo", "-kdpn", "65536", "-pb", compressed(PUB), "-pk", "%x" % A, "-pke", "%x" % (A + W - 1)], "-kdpn belongs to -kdpdev"),
    (["-kangaroo", "-kdpdev", "-infile", "keys.txt", "-pk", "%x" % A, "-pke", "%x" % (A + W - 1)], "-kangaroo -kdpdev cannot be combined with -infile"),
    (SEARCH + ["-ktames", "none.tames"], "-kangaroo -kdpdev cannot be combined with -ktames, -ktamessym, -ktamesgen or -ktamesmerge"),
    (SEARCH + ["-ktamessym", "none.tames"], "-kangaroo -kdpdev cannot be combined with -ktames, -ktamessym, -ktamesgen or -ktamesmerge"),
    (["-kangaroo", "-kdpdev", "-ktamesgen", "out.tames", "-ktn", "64", "-pk", "%x" % A, "-pke", "%x" % (A + W - 1)],
     "-kangaroo -kdpdev cannot be combined with -ktames, -ktamessym, -ktamesgen or -ktamesmerge"),
    (["-kangaroo", "-kdpdev", "-ktamesgen", "out.tames", "-ktamesmerge", "a.tames,b.tames", "-pk", "%x" % A, "-pke", "%x" % (A + W - 1)],
     "-kangaroo -kdpdev cannot be combined with -ktames, -ktamessym, -ktamesgen or -ktamesmerge"),
    (SEARCH + ["-d", "0,1"], "-kangaroo -kdpdev takes one -d entry"),
    (SEARCH + ["-ksym", "-d", "0,1"], "-kangaroo -kdpdev takes one -d entry"),
    (SEARCH + ["-kdpn", "0"], "-kdpn must be 1..2^31"),
])
def test_refusals(tmp_path, args, message):
    r = host(args + ["-dir", str(tmp_path)] if "-kangaroo" in args else args, cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode != 0 and len([ln for ln in out.split("\n") if message in ln]) == 1, out
    assert "No GPU found" not in out and "[startup]" not in out and "Kangaroo range" not in out, out      # refused before any device is looked for
    assert os.listdir(tmp_path) == []


FLAGS = {"T": 0, "W": K.WILD, "N": K.WILD | DM.NEG, "D": K.DEAD, "C": K.DEAD | CYCLE}


def through_the_device(recs):
    """the logical stream (letter, x, d, kangaroo) as -kdpdev's collector sees it: one launch per record through the model of the device table -> (the items of
    -selftest kangaroo-dpdev, the positions of the records the device stored: they never reach the host)"""
    table = DM.new_table(64, 64)
    items, silent = [], set()
    for pos, (t, x, d, kid) in enumerate(recs):
        table, back = DM.insert(table, [(x & DM.M64, d & K.M128, FLAGS[t], kid)])
        item = "%s,%x,%x,%d" % (t, x, d & K.M128, kid)
        if not back:
            silent.add(pos)
            continue
        (reason, _, stored), = back
        if reason == DM.DPT_DUPLICATE:
            (tag, sd, skid, stype), = stored
            items.append("S,%x,%x,%d,%d" % (tag, sd, skid, stype))
        items.append(item)
    return items, silent


def compare(selftest, sym, recs, want_lines):
    args = ["%x" % A, "%x" % (A + W - 1), compressed(PUB)]
    r = host(["-selftest", selftest] + args + ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in recs])
    assert r.returncode == 0, r.stderr
    plain = r.stdout.split("\n")[:-1]
    assert plain[:-1] == want_lines, plain                            # the host-only search says what the case is about
    items, silent = through_the_device(recs)
    assert silent and all(plain[p] == "new" for p in silent)         # what the device stores is what the host-only table answers "new" to
    r = host(["-selftest", "kangaroo-dpdev"] + (["sym"] if sym else []) + args + items)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    assert got[:-1] == [ln for p, ln in enumerate(plain[:-1]) if p not in silent]
    ps, gs = plain[-1].split(), got[-1].split()
    assert ps[0] == gs[0] == "summary" and ps[2:] == gs[2:]          # false matches, re-seeds (sym: cycles) as the host-only search counts them
    assert int(gs[1]) == int(ps[1]) - len(silent)                    # and the host's map holds only what the device could not
    return got


def test_selftest_plain_gives_the_verdicts_of_the_host_only_search():
    d1, d2, d3 = 0x123456789ABC, 0x2222222222, 0x3333333333
    x1, x2, x3 = mul(d1)[0], mul(d2)[0], mul(d3)[0]
    x0 = (mul(d3)[0] >> 64) << 64                                     # a tag of 0: the device hands such a record back and the host keeps it
    recs = [("T", x1, d1, 1), ("W", x1, d1 - KP, 5),                  # tame meets wild: found
            ("T", x1, d2, 2),                                         # same type, another kangaroo: reseed
            ("T", x1, d1, 1),                                         # its own point again: repeat
            ("W", x2, d2, 6), ("T", x2, d2 + 5, 3),                   # a pair that does not solve: false
            ("D", x3, d3, 4),                                         # dead: reseed, never stored
            ("T", x0, d3, 7), ("W", x0, d3 - KP, 8),                  # tag 0: new in the host's own map, and found there
            ("T", x3, d3, 9)]                                         # the dead record's tag is still free
    got = compare("kangaroo", False, recs, ["new", "found %064x" % (A + KP), "reseed 2", "repeat", "new", "false", "reseed 4", "new", "found %064x" % (A + KP), "new"])
    assert got[:-1] == ["found %064x" % (A + KP), "reseed 2", "repeat", "false", "reseed 4", "new", "found %064x" % (A + KP)]


def test_selftest_sym_gives_the_verdicts_of_the_host_only_search():
    mid = A + W // 2
    kk = KP - W // 2                                                  # the key counted from the middle of the range
    d1, d2, d3 = 0x123456789ABC, 0x2222222222, 0x3333333333
    x1, x2, x3, x4 = mul(d1)[0], mul(d2)[0], mul(d3)[0], mul(d1 + d2)[0]
    assert mid + kk == A + KP
    recs = [("W", x1, d1, 1), ("N", x1, d1 + 2 * kk, 2),              # wild meets wild with opposite NEG: Q + d1 G = -Q + d2 G, k'' = (d2 - d1) / 2: found
            ("T", x2, d2, 3), ("W", x2, d2 - kk, 4),                  # tame meets wild: found
            ("T", x2, d3, 5),                                         # tame meets tame: reseed
            ("W", x2, d2 - kk, 3),                                    # the kangaroo of the stored entry again: repeat
            ("C", x3, d3, 6), ("D", x3, d3, 7),                       # a cycle's record and a dead one: reseed, never stored
            ("N", x4, d1, 8), ("T", x4, d2, 9)]                       # a pair that does not solve: counted as false and re-seeded
    got = compare("kangaroo-sym", True, recs, ["new", "found %064x" % (A + KP), "new", "found %064x" % (A + KP), "reseed 5", "repeat", "reseed 6", "reseed 7", "new", "reseed 9"])
    assert got[-1].split()[2:] == ["1", "4", "1"]                     # one candidate pair that did not verify, four re-seeds, one cycle


def test_selftest_refuses_a_pair_of_different_tags():
    args = ["%x" % A, "%x" % (A + W - 1), compressed(PUB)]
    assert host(["-selftest", "kangaroo-dpdev"] + args + ["S,5,1,1,0", "W,6,2,2"]).returncode == 2
    assert host(["-selftest", "kangaroo-dpdev"] + args + ["S,5,1,1,3", "W,5,2,2"]).returncode == 2      # type 3 belongs to the symmetric walk
    assert host(["-selftest", "kangaroo-dpdev"] + args + ["S,5,1,1,0"]).returncode == 2                 # a stored entry without its record
    r = host(["-selftest", "kangaroo-dpdev", "sym"] + args + ["S,5,1,1,3", "W,5,2,2"])
    assert r.returncode == 0 and r.stdout.split("\n")[0] == "reseed 2"


def plan(width_bits, cus, min_launch, dp_arg=-1, kn_arg=0, kdpn=0):
    """DESIGN.md 10, "the table of distinguished points in device memory": capacity, dp, then the herd by the existing rule (plan_herd), the launch length and
    its bound, the record buffer -> (dp, kn, per thread, S, record buffer, capacity)"""
    sq = math.sqrt(float(1 << width_bits))
    capacity = kdpn
    if not capacity:
        capacity = 1 << 16
        while capacity < (1 << 27) and capacity < 4 * sq:
            capacity *= 2
    dp = dp_arg if dp_arg >= 0 else int(min(32, max(0, math.ceil(math.log2(4 * sq / capacity)))))
    kn = kn_arg or int(min(float(cus * 1024 * 16), sq / 8 / 2 ** dp))
    kn = max(kn, 64)
    g = 16
    while g > 1 and kn // g < cus * 512:
        g //= 2
    kn = max(64 * g, kn // (64 * g) * (64 * g))
    expected = 2 * sq + kn * 2.0 ** dp
    s = int(max(min_launch, min(1024.0, expected / kn / 8)))
    half = float(1 << 21)                                             # half of the largest record buffer
    if kn * s / 2.0 ** dp > half:
        s = int(max(min_launch, math.floor(half * 2.0 ** dp / kn)))   # first the launch gives way, down to the mode's floor ...
    while dp_arg < 0 and kn * s / 2.0 ** dp > half and dp < 32:
        dp += 1                                                       # ... then dp, unless the command line fixed it
    cap = int(min(float(1 << 22), 2 * kn * s / 2.0 ** dp + 65536))
    return dp, kn, g, s, cap, capacity


@pytest.mark.parametrize("bits", [40, 63, 64, 80])
@pytest.mark.parametrize("min_launch,dp_arg,kn_arg,kdpn", [(8, -1, 0, 0), (32, -1, 0, 0), (8, 12, 0, 0), (8, -1, 1 << 20, 0), (8, -1, 0, 1 << 20), (32, 3, 1 << 22, 1 << 24)])
def test_plan(bits, min_launch, dp_arg, kn_arg, kdpn):
    want = plan(bits, 256, min_launch, dp_arg, kn_arg, kdpn)
    r = host(["-selftest", "kangaroo-dpdev-plan", "1", "%x" % (1 << bits), "256", str(min_launch), str(dp_arg), str(kn_arg), str(kdpn)])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["plan"] + [str(v) for v in want], (r.stdout, want)
    dp, kn, g, s, cap, capacity = want
    assert kn * s / 2 ** dp <= (1 << 21) or dp_arg >= 0 or dp == 32   # the records a launch is expected to write fill at most half the record buffer
    if not kdpn and dp_arg < 0:
        assert 2 * math.sqrt(float(1 << bits)) / 2 ** dp <= capacity / 2      # and the expected DPs half of the capacity


@pytest.mark.parametrize("bits,figures", [(64, (7, 4194304, 16, 64, 1 << 22, 1 << 27)), (40, (0, 131072, 1, 8, 2 * (1 << 20) + 65536, 1 << 22))])
def test_plan_figures(bits, figures):
    """the figures DESIGN.md 10 quotes, from the host: a 64-bit range walks the full herd at dp 7 with a table of 2^27 entries; a 40-bit range needs no DP
    condition at all"""
    r = host(["-selftest", "kangaroo-dpdev-plan", "1", "%x" % (1 << bits), "256", "8", "-1", "0", "0"])
    assert r.returncode == 0 and r.stdout.split() == ["plan"] + [str(v) for v in figures], r.stdout + r.stderr
    assert plan(bits, 256, 8) == figures


def test_without_d_the_search_takes_one_gpu(tmp_path):
    """-kdpdev is one engine with one table: a command line without -d, which otherwise means every GPU of the machine, names GPU #0 before any device is
    looked for (what follows depends on the machine: no GPU ends the run, one GPU walks the 20-bit range)"""
    two_g = mul(2)
    r = host(["-kangaroo", "-kdpdev", "-pb", compressed(two_g), "-pk", "1", "-pke", "%x" % (1 << 20), "-ksteps", "1", "-dir", str(tmp_path)])
    out = r.stdout + r.stderr
    lines = out.split("\n")
    assert "Kangaroo -kdpdev: no -d given, one engine on GPU #0" in lines, out
    assert "engine(s)" not in out or "Kangaroo: 1 engine(s) x " in out, out
    r = host(["-kangaroo", "-kdpdev", "-d", "0", "-pb", compressed(two_g), "-pk", "1", "-pke", "%x" % (1 << 20), "-ksteps", "1", "-dir", str(tmp_path)])
    assert "no -d given" not in r.stdout + r.stderr
