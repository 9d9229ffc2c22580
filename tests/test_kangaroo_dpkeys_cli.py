"""CPU: the host's side of -kangaroo -infile -kdpkeys (host/host_kangaroo_list.h and the two list tables), no GPU: every refusal of the command line with its
one line before any device is looked for; -selftest kangaroo-dpkeys, plain and sym, gives for every row of the two list rules the event lines of
-selftest kangaroo-multi / kangaroo-symlist on the same logical stream -- the stream goes through the model of the keyed device table
(tests/kangaroo_dptable_keys_model.py), every second tag by way of the host's own map as a full device table would send it: what the device stores is silent,
a duplicate arrives behind the entry it met, DEAD records arrive alone --; and the plan of -kdpkeys is what the formulas of DESIGN.md 10 give."""
import hashlib
import math
import os
import struct
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_dptable_model as DM
import kangaroo_dptable_keys_model as KM
import test_kangaroo_multi_model as TM
import test_kangaroo_symlist_model as TS
from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
A, W, PUBS = TM.A, TM.W, TM.PUBS
assert (TS.A, TS.W, TS.PUBS) == (A, W, PUBS)
CYCLE = 4
RANGE = ["-pk", "%x" % A, "-pke", "%x" % (A + W - 1)]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def host(args, cwd=None):
    assert os.path.exists(HOST), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([HOST] + args, capture_output=True, text=True, timeout=120, cwd=cwd)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------------------------
LIST = ["-kangaroo", "-kdpkeys", "-infile", "keys.txt"] + RANGE


@pytest.mark.parametrize("args,message", [
    (["-kdpkeys", "-infile", "keys.txt"], "-kdpkeys belongs to -kangaroo"),
    (["-kangaroo", "-kdpkeys"] + RANGE, "-kangaroo -kdpkeys needs -infile"),
    (["-kangaroo", "-kdpkeys", "-pb", compressed(PUBS[0])] + RANGE, "-kangaroo -kdpkeys cannot be combined with -pb"),
    (LIST + ["-pb", compressed(PUBS[0])], "-kangaroo -kdpkeys cannot be combined with -pb"),
    (LIST + ["-kdpdev"], "-kangaroo -kdpkeys cannot be combined with -kdpdev"),
    (LIST + ["-kwalk", "sym", "-kdpdev"], "-kangaroo -kdpkeys cannot be combined with -kdpdev"),
    (LIST + ["-ktames", "none.tames"], "-kangaroo -kdpkeys cannot be combined with -ktames, -ktamessym, -ktamesgen"),
    (LIST + ["-ktamessym", "none.tames"], "-kangaroo -kdpkeys cannot be combined with -ktames, -ktamessym, -ktamesgen"),
    (LIST + ["-ktamesgen", "out.tames", "-ktn", "64"], "-kangaroo -kdpkeys cannot be combined with -ktames, -ktamessym, -ktamesgen"),
    (LIST + ["-ktamesdev"], "-kangaroo -kdpkeys cannot be combined with -ktames, -ktamessym, -ktamesgen"),
    (LIST + ["-d", "0,1"], "-kangaroo -kdpkeys takes one -d entry"),
    (LIST + ["-kwalk", "sym", "-d", "0,1"], "-kangaroo -kdpkeys takes one -d entry"),
    (LIST + ["-kdpn", "0"], "-kdpn must be 1..2^31"),
    # what the tests of -kdpdev pin stays: the refusal of a list is one line that now names the flag a list takes, and -kdpn alone belongs to neither
    (["-kangaroo", "-kdpdev", "-infile", "keys.txt"] + RANGE, "-kangaroo -kdpdev cannot be combined with -infile"),
    (["-kangaroo", "-kdpn", "65536", "-infile", "keys.txt"] + RANGE, "-kdpn belongs to -kdpdev or -kdpkeys"),
])
def test_refusals(tmp_path, args, message):
    r = host(args + ["-dir", str(tmp_path)] if "-kangaroo" in args else args, cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode != 0 and len([ln for ln in out.split("\n") if message in ln]) == 1, out
    assert "No GPU found" not in out and "[startup]" not in out and "Kangaroo range" not in out, out      # refused before any device is looked for
    assert os.listdir(tmp_path) == []


def test_the_refusal_of_a_list_with_kdpdev_names_kdpkeys():
    r = host(["-kangaroo", "-kdpdev", "-infile", "keys.txt"] + RANGE)
    (line,) = [ln for ln in (r.stdout + r.stderr).split("\n") if "-kangaroo -kdpdev cannot be combined with -infile" in ln]
    assert "-kdpkeys" in line


def write_work_v3(path, pubs, lo, hi, engines, herd=64, per_thread=1, dp=0, seed=5):
    """a version-3 work file of `engines` engines with an empty table and herds of zero states (DESIGN.md 10 states the layout; the reader is
    tests/kangaroo_multi_workfile.py): enough for the checks that come before any device is looked for"""
    text = "".join(compressed(p) for p in pubs) + "%064x%064x" % (lo, hi) + "dp%dkn%dg%de%ds%dkeys%d" % (dp, herd, per_thread, engines, seed, len(pubs))
    b = b"KANGWORK" + struct.pack("<IIQII", 3, engines, herd, dp, per_thread) + struct.pack("<7Q", seed, 1, 0, 0, 0, 0, 0) + struct.pack("<dQ", 0.0, 0)
    b += hashlib.sha1(text.encode()).hexdigest().encode()
    b += struct.pack("<I", len(pubs)) + b"\0" * len(pubs) + struct.pack("<3Q", 0, 0, 0)
    b += (b"\0" * (96 * herd) + struct.pack("<I", 0)) * engines
    with open(path, "wb") as f:
        f.write(b)


def test_a_work_file_of_more_than_one_engine_is_refused(tmp_path):
    keys = tmp_path / "keys.txt"
    keys.write_text("".join(compressed(p) + "\n" for p in PUBS))
    for engines in (1, 2):
        write_work_v3(str(tmp_path / ("e%d.work" % engines)), PUBS, A, A + W - 1, engines)
        r = host(["-selftest", "kangaroo-work", str(tmp_path / ("e%d.work" % engines)), "%x" % A, "%x" % (A + W - 1), ",".join(compressed(p) for p in PUBS)])
        assert r.returncode == 0 and "fingerprint-check ok" in r.stdout, r.stdout + r.stderr      # the file is one this list and range made
    r = host(["-kangaroo", "-kdpkeys", "-infile", str(keys), "-wl", str(tmp_path / "e2.work"), "-dir", str(tmp_path)] + RANGE)
    out = r.stdout + r.stderr
    assert r.returncode != 0 and len([ln for ln in out.split("\n") if "Recovery file was made with other settings" in ln]) == 1, out
    assert "No GPU found" not in out and "[startup]" not in out and "engine(s)" not in out, out      # refused before any device is looked for


# ---- the rule: -selftest kangaroo-dpkeys against the host-only tables --------------------------------------------------------------------------------------------
def through_the_device(recs, sym):
    """the logical stream (letter[key], x, d, kangaroo) as -kdpkeys' collector sees it.  The tags take turns by their first appearance: those of even turn live
    in the model of the device table (one launch per record), those of odd turn find no slot there and live in the host's own map, as FULL hand-backs do
    -> (the items of -selftest kangaroo-dpkeys, the positions of the records the device stored: they never reach the host)"""
    table = DM.new_table(64, 64)
    items, silent, turn = [], set(), {}
    for pos, (t, x, d, kid) in enumerate(recs):
        item = "%s,%x,%x,%d" % (t, x, d & K.M128, kid)
        fl = {"T": 0, "W": K.WILD, "N": K.WILD | KM.NEG, "D": K.DEAD, "C": K.DEAD | CYCLE}[t[0]]
        key = int(t[1:]) if t[0] in "WN" else 0
        tag = x & DM.M64
        if not fl & K.DEAD and turn.setdefault(tag, len(turn)) % 2:
            items.append(item)                                        # FULL: handed back alone, into the host's map
            continue
        rec = (tag, d & K.M128, fl, kid, key) if sym else (tag, d & K.M128, fl | key << KM.KEY_SHIFT, kid, 0)
        table, back = KM.insert(table, [rec], sym)
        if not back:
            silent.add(pos)
            continue
        (reason, _, stored, word), = back
        assert KM.decode_reserved(word) == (reason, key)
        if reason == KM.DPT_DUPLICATE:
            (stag, sd, skid, owner), = stored
            items.append("S,%x,%x,%d,%d" % (stag, sd, skid, owner))
        items.append(item)
    return items, silent


def compare(sym, pubs, recs):
    args = ["%x" % A, "%x" % (A + W - 1), ",".join(compressed(p) for p in pubs)]
    r = host(["-selftest", "kangaroo-symlist" if sym else "kangaroo-multi"] + args + ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in recs])
    assert r.returncode == 0, r.stderr
    plain = r.stdout.split("\n")[:-1]
    # which output lines belong to which record: a record's first line is its verdict, "found" lines of a chain and "reseed" behind a link follow it
    items, silent = through_the_device(recs, sym)
    r = host(["-selftest", "kangaroo-dpkeys"] + (["sym"] if sym else []) + args + items)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    # the records the device stored are exactly those the host-only table answers "new" to and nothing else; the other lines are equal, in order
    want = list(plain[:-1])
    news = [k for k, ln in enumerate(want) if ln == "new"]
    model = (TS if sym else TM).model_lines(pubs, recs)[0]
    assert model == plain                                             # (the host-only selftest is the model's)
    per_record = lines_per_record(sym, pubs, recs)
    drop = set()
    for pos in silent:
        assert per_record[pos] == ["new"]
        drop.add(sum(len(per_record[q]) for q in range(pos)))
    assert drop <= set(news)
    assert got[:-1] == [ln for k, ln in enumerate(want) if k not in drop], (got, want, items)
    ps, gs = plain[-1].split(), got[-1].split()
    assert ps[0] == gs[0] == "summary" and ps[2:] == gs[2:]          # false matches, re-seeds, links kept and resolved, keys solved (sym: cycles)
    assert int(gs[1]) == int(ps[1]) - len(silent)                    # and the host's map holds only what the device did not take
    return items, silent, got


def lines_per_record(sym, pubs, recs):
    """the model's event lines record by record"""
    mod = TS if sym else TM
    out, before = [], 0
    for n in range(1, len(recs) + 1):
        lines = mod.model_lines(pubs, recs[:n])[0][:-1]
        out.append(lines[before:])
        before = len(lines)
    return out


PLAIN_ROWS = ["tame_wild", "wild_tame", "negative_offset", "same_type", "false_match", "link_then_second", "link_then_first", "chain", "false_link",
              "solved_acts_as_tame"]
SYM_ROWS = ["tame_wild_plus", "tame_wild_minus", "neg_wild_tame_plus", "neg_wild_tame_minus", "tame_neg_wild_minus", "same_key_plus", "same_key_minus",
            "same_key_cancel", "earlier_life_link", "earlier_life_solves", "earlier_life_same_type", "same_type", "false_match", "link_then_second",
            "link_then_first", "link_minus_then_second", "link_minus_then_first", "chain", "false_link", "solved_acts_as_tame"]


@pytest.mark.parametrize("row", PLAIN_ROWS)
def test_plain_rule_rows(row):
    """tame/wild found, false match, same-key wild/wild, a link in either order, a chain of two, a solved key acting as tame, DEAD, repeat"""
    items, silent, got = compare(False, PUBS, TM.streams()[row])
    assert silent


@pytest.mark.parametrize("row", SYM_ROWS)
def test_symmetric_rule_rows(row):
    """the same rows with both signs, the own-kangaroo cycle row ("repeat" with its re-seed), DEAD with CYCLE"""
    items, silent, got = compare(True, PUBS, TS.streams()[row])
    assert silent


def test_the_rows_cover_both_routes_and_the_own_kangaroo_cycle():
    routes = set()
    for sym, mod, rows in ((False, TM, PLAIN_ROWS), (True, TS, SYM_ROWS)):
        for row in rows:
            recs = mod.streams()[row]
            items, silent = through_the_device(recs, sym)
            tags = {}
            for t, x, d, kid in recs:
                if t[0] not in "DC":
                    tags.setdefault(x & DM.M64, []).append(t)
            for k, (tag, ts) in enumerate(tags.items()):
                if len(ts) > 1:
                    routes.add((sym, "host" if k % 2 else "device"))
    assert routes == {(False, "host"), (False, "device"), (True, "host"), (True, "device")}
    # the symmetric list's own-kangaroo row through a pair: the stored entry is the kangaroo's own record
    w = TS.wild(2, 1, 5, 2)
    items, silent, got = compare(True, PUBS, [w, w])
    assert items[0].startswith("S,") and got[:-1] == ["repeat", "reseed 2"] and got[-1].split()[-1] == "1"
    c = ("C", mul(11)[0], 3, 7)
    items, silent, got = compare(True, PUBS, [w, c, ("D", mul(9)[0], 1, 6)])
    assert items == ["%s,%x,%x,%d" % (t, x, d, kid) for t, x, d, kid in (c, ("D", mul(9)[0], 1, 6))] and got[:-1] == ["reseed 7", "reseed 6"]


def test_selftest_refuses_what_is_no_pair():
    args = ["%x" % A, "%x" % (A + W - 1), ",".join(compressed(p) for p in PUBS)]
    assert host(["-selftest", "kangaroo-dpkeys"] + args + ["S,5,1,1,0", "W0,6,2,2"]).returncode == 2          # another tag
    assert host(["-selftest", "kangaroo-dpkeys"] + args + ["S,5,1,1,0"]).returncode == 2                      # a stored entry without its record
    assert host(["-selftest", "kangaroo-dpkeys"] + args + ["S,5,1,1,0", "D,5,2,2"]).returncode == 2           # a DEAD record comes back alone
    for sym in ([], ["sym"]):                                                                                  # an owner beyond the list: that table is damaged
        r = host(["-selftest", "kangaroo-dpkeys"] + sym + args + ["S,5,1,1,5", "W0,5,2,2"])
        assert r.returncode == 2 and len([ln for ln in r.stderr.split("\n") if "the table is damaged" in ln]) == 1, r.stderr
        r = host(["-selftest", "kangaroo-dpkeys"] + sym + args + ["S,5,1,1,4", "W0,5,2,2"])
        assert r.returncode == 0 and r.stdout.split("\n")[0] == "link 3 0", r.stdout
    r = host(["-selftest", "kangaroo-dpkeys"] + args + ["S,5,1,1,%d" % (1 | 1 << 31), "W0,5,2,2"])          # NEG belongs to the symmetric list
    assert r.returncode == 2
    r = host(["-selftest", "kangaroo-dpkeys", "sym"] + args + ["S,5,1,1,%d" % (1 | 1 << 31), "W0,5,2,2"])
    assert r.returncode == 0 and r.stdout.split("\n")[:2] == ["false", "reseed 2"], r.stdout


# ---- the plan --------------------------------------------------------------------------------------------------------------------------------------------------
def plan(width_bits, L, cus, min_launch, dp_arg=-1, kn_arg=0, kdpn=0):
    """DESIGN.md 10, "the table of a key list in device memory": capacity and dp as -kdpdev's with sqrt(L W) in the place of sqrt(W); then the herd by the
    existing rule from sqrt(W) (plan_herd), the launch length and its bound, the record buffer -> (dp, kn, per thread, S, record buffer, capacity)"""
    sq = math.sqrt(float(1 << width_bits))
    sql = math.sqrt(float(L) * float(1 << width_bits))
    capacity = kdpn
    if not capacity:
        capacity = 1 << 16
        while capacity < (1 << 27) and capacity < 4 * sql:
            capacity *= 2
    dp = dp_arg if dp_arg >= 0 else int(min(32, max(0, math.ceil(math.log2(4 * sql / capacity)))))
    kn = kn_arg or int(min(float(cus * 1024 * 16), sq / 8 / 2 ** dp))
    kn = max(kn, 64)
    g = 16
    while g > 1 and kn // g < cus * 512:
        g //= 2
    kn = max(64 * g, kn // (64 * g) * (64 * g))
    expected = 2 * sq + kn * 2.0 ** dp
    s = int(max(min_launch, min(1024.0, expected / kn / 8)))
    half = float(1 << 21)
    if kn * s / 2.0 ** dp > half:
        s = int(max(min_launch, math.floor(half * 2.0 ** dp / kn)))
    while dp_arg < 0 and kn * s / 2.0 ** dp > half and dp < 32:
        dp += 1
    cap = int(min(float(1 << 22), 2 * kn * s / 2.0 ** dp + 65536))
    return dp, kn, g, s, cap, capacity


@pytest.mark.parametrize("bits", [40, 64, 80])
@pytest.mark.parametrize("L", [1, 16, 1000])
@pytest.mark.parametrize("min_launch,dp_arg,kn_arg,kdpn", [(8, -1, 0, 0), (32, -1, 0, 0), (8, 12, 0, 0), (8, -1, 0, 1 << 20), (32, 3, 1 << 22, 1 << 24)])
def test_plan(bits, L, min_launch, dp_arg, kn_arg, kdpn):
    want = plan(bits, L, 256, min_launch, dp_arg, kn_arg, kdpn)
    r = host(["-selftest", "kangaroo-dpkeys-plan", "1", "%x" % (1 << bits), "256", str(min_launch), str(dp_arg), str(kn_arg), str(kdpn), str(L)])
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["plan"] + [str(v) for v in want], (r.stdout, want)
    dp, kn, g, s, cap, capacity = want
    if not kdpn and dp_arg < 0:
        assert 2 * math.sqrt(float(L) * float(1 << bits)) / 2 ** dp <= capacity / 2      # the 2 sqrt(L W) / 2^dp expected DPs fill at most half the capacity
    if L == 1:                                                        # one open key: -kdpdev's plan
        one = host(["-selftest", "kangaroo-dpdev-plan", "1", "%x" % (1 << bits), "256", str(min_launch), str(dp_arg), str(kn_arg), str(kdpn)])
        assert one.stdout == r.stdout


def test_plan_figures():
    """the figures DESIGN.md 10 quotes for config 4's shape, 1000 keys in a 64-bit range: dp 12, 131072 kangaroos, a table of 2^27 entries"""
    r = host(["-selftest", "kangaroo-dpkeys-plan", "1", "%x" % (1 << 64), "256", "8", "-1", "0", "0", "1000"])
    assert r.returncode == 0 and r.stdout.split() == ["plan", "12", "131072", "1", "1024", "131072", str(1 << 27)], r.stdout + r.stderr
    assert plan(64, 1000, 256, 8) == (12, 131072, 1, 1024, 131072, 1 << 27)


def test_without_d_the_search_takes_one_gpu(tmp_path):
    keys = tmp_path / "keys.txt"
    keys.write_text(compressed(mul(2)) + "\n" + compressed(mul(3)) + "\n")
    r = host(["-kangaroo", "-kdpkeys", "-infile", str(keys), "-pk", "1", "-pke", "%x" % (1 << 20), "-ksteps", "1", "-dir", str(tmp_path)])
    out = r.stdout + r.stderr
    assert "Kangaroo -kdpkeys: no -d given, one engine on GPU #0" in out.split("\n"), out
    assert "engine(s)" not in out or "Kangaroo: 1 engine(s) x " in out, out
