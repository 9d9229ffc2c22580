"""CPU: the host's side of -ktamesgen -ktamesdev (host/host_kangaroo_tames.cpp): the two refusals, both before any device is looked for, and the rule of
the handed-back records line for line against the model (-selftest kangaroo-tames-gen, tests/kangaroo_tames_gen_model.py); the model's own slot formula and
insert on small cases."""
import os
import subprocess
from collections import Counter

import kangaroo_model as K
import kangaroo_tames_gen_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
RANGE = ["-pk", "800000000", "-pke", "fffffffff"]


def host(args, cwd=None):
    assert os.path.exists(HOST), "host binary missing: run __graft_entry__.build()"
    return subprocess.run([HOST] + args, capture_output=True, text=True, timeout=120, cwd=cwd)


def test_refused_without_ktamesgen(tmp_path):
    for extra in ([], ["-pb", "02" + "%064x" % 1], ["-ktames", "x.tames", "-pb", "02" + "%064x" % 1]):
        r = host(["-kangaroo", "-dir", str(tmp_path), "-ktamesdev"] + RANGE + extra)
        assert r.returncode == 1 and r.stderr.strip().split("\n") == ["-ktamesdev belongs to -ktamesgen (the table that grows in GPU memory is the one being made)"], r.stderr
        assert "GPU #" not in r.stdout and os.listdir(tmp_path) == []


def test_refused_with_more_than_one_device(tmp_path):
    for walk in ([], ["-kwalk", "sym"]):
        r = host(["-kangaroo", "-dir", str(tmp_path), "-ktamesgen", "t.tames", "-ktn", "64", "-ktamesdev", "-d", "0,0"] + RANGE + walk)
        assert r.returncode == 1, r.stdout
        assert r.stderr.strip().split("\n") == ["-kangaroo -ktamesgen -ktamesdev takes one -d entry (a table grown on several GPUs would have to be merged)"], r.stderr
        assert "GPU #" not in r.stdout and os.listdir(tmp_path) == []


def test_the_help_names_the_flag():
    r = host(["-h"])
    assert "-ktamesdev" in r.stdout and "full herd" in r.stdout


def test_slots():
    assert GM.n_slots(1, 1) == 128 and GM.n_slots(63, 1) == 128 and GM.n_slots(64, 1) == 256
    assert GM.n_slots(64, 1024) == 4096 and GM.n_slots(1024, 1024) == 4096 and GM.n_slots(1025, 1024) == 8192
    assert GM.n_slots(1 << 26, 1 << 22) == 1 << 28 and GM.n_slots(1 << 31, 1 << 26) == 1 << 33


def test_model_insert():
    t = GM.new_table(64, 64)
    assert t["slots"] == 256
    a, b, c = GM.chain_tags(255, 256, 3)                              # one home slot, the last: the chain wraps
    t, back = GM.insert(t, [(a, 1, 0), (b, 2, 0), (a, 3, 0), (0, 4, 0), (c, 5, K.DEAD), (c, 6, 0)])
    assert back == Counter({(a, GM.GEN_DUPLICATE): 1, (0, GM.GEN_TAG_ZERO): 1, (c, GM.GEN_DEAD): 1})
    assert t["cand"] == {a: {1, 3}, b: {2}, c: {6}} and GM.entries(t) == 3
    assert [i for i, v in enumerate(t["tags"]) if v] == [0, 1, 255]
    t, back = GM.insert(t, [(a, 9, 0)])                              # a tag of an earlier launch: the stored d is not in question any more
    assert back == Counter({(a, GM.GEN_DUPLICATE): 1}) and t["cand"][a] == {1, 3}


def script():
    """T = 6: two launches' hand-backs -- a duplicate, a tag-zero pair, a dead record, a FULL one -- then the launch at which T is reached, and what comes after"""
    return 6, [("E", 2), ("U", 0xABCDEF, 17, 3), ("Z", 0, 5, 1), ("D", 0x99, (1 << 128) - 9, 4), ("E", 4), ("Z", 0, 6, 2), ("F", 1, 1, 7), ("U", 0x77, 1, 0),
               ("E", 5), ("D", 0x55, 2, 6), ("U", 0x66, 3, 5)]


def test_selftest_against_the_model():
    T, items = script()
    rule = GM.GenRule(T)
    reason = {"D": GM.GEN_DEAD, "U": GM.GEN_DUPLICATE, "Z": GM.GEN_TAG_ZERO, "F": GM.GEN_FULL}
    want, args = [], []
    for it in items:
        if it[0] == "E":
            want += rule.entries(it[1])
            args.append("E,%d" % it[1])
        else:
            want += rule.record(reason[it[0]], it[1], it[2], it[3])
            args.append("%s,%x,%x,%d" % it)
    want.append(rule.summary())
    # the script is what it is meant to be: the table is done at the third E (5 on the device, 1 held), and the records behind it are not looked at
    assert want == ["entries 2", "merge 3", "held 1", "reseed 4", "entries 5", "merge 2", "dropped", "merge 0", "entries 6", "done", "ignored", "ignored",
                    "summary 4 3 1 1 1"]
    r = host(["-selftest", "kangaroo-tames-gen", str(T)] + args)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().split("\n") == want


def test_selftest_refuses_a_bad_script():
    assert host(["-selftest", "kangaroo-tames-gen"]).returncode == 2
    assert host(["-selftest", "kangaroo-tames-gen", "4", "Q,1,1,1"]).returncode == 2
    assert host(["-selftest", "kangaroo-tames-gen", "0", "E,1"]).returncode == 2
