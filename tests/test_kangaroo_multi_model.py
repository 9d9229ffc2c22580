"""CPU: the many-keys rule of kangaroo mode (include/bsgs_hip.h "Kangaroo, many keys") on the model (tests/kangaroo_multi_model.py) -- every row of the
collision table on hand-made streams, links resolved in either order and a chain of two, a false link, a solved key's old entry acting as a tame one, the
assignment of wild kangaroos, the model solver on planted keys -- and the host's table (bsgs_mi355x -selftest kangaroo-multi) on the same streams."""
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_multi_model as M
from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")

A, W = 0x1F << 36, 1 << 24
KP = [0xABCDE, 0x12345, 0xF00D, 0x3C3C3C]                       # k_k - a of the four keys
PUBS = [mul(A + k) for k in KP]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def tame(d, kid):
    """a record of a tame kangaroo at offset d: the point d*G"""
    return ("T", mul(d)[0], d, kid)


def wild(k, d, kid):
    """a record of a wild kangaroo of key k at offset d: the point Q_k + d*G = (k'_k + d)*G"""
    return ("W%d" % k, mul(KP[k] + d)[0], d, kid)


def streams():
    s = {}
    s["tame_wild"] = [tame(0x5000, 1), wild(2, 7, 9), wild(1, 0x5000 - KP[1], 2)]
    s["wild_tame"] = [wild(1, 0x5000 - KP[1], 2), tame(0x5000, 1)]
    s["negative_offset"] = [wild(0, -0x100, 2), tame(KP[0] - 0x100, 1)]
    t = tame(0x6000, 1)
    s["same_type"] = [t, t, ("T", t[1], 0x6005, 3), wild(0, 5, 4), wild(0, 5, 4), ("W0", wild(0, 5, 4)[1], 6, 6), ("D", mul(9)[0], 1, 5)]
    s["false_match"] = [t, ("W1", t[1], 0x6001, 2), ("W2", t[1], 0x6000 - KP[2] + W, 3)]
    # wild of 0 and wild of 1 on one point: (k'_0 + e0) = (k'_1 + e1); then key 1 is solved: key 0 follows through the link
    e0 = 0x777
    e1 = KP[0] + e0 - KP[1]
    link01 = [wild(0, e0, 1), wild(1, e1, 2)]
    s["link_then_second"] = link01 + [tame(0x5000, 3), wild(1, 0x5000 - KP[1], 4)]
    s["link_then_first"] = link01 + [tame(0x5000, 3), wild(0, 0x5000 - KP[0], 4)]
    # a chain: 0 -- 1 and 1 -- 2, then key 2 is solved: 2, 1, 0
    f1 = -0x4321
    f2 = KP[1] + f1 - KP[2]
    s["chain"] = link01 + [wild(2, f2, 5), wild(1, f1, 6), tame(0x5000, 3), wild(2, 0x5000 - KP[2], 4)]
    # a link whose x agree in the low 64 bits only by accident: dropped and counted when one end is solved, the other key stays open
    w0 = wild(0, e0, 1)
    s["false_link"] = [w0, ("W1", w0[1], e1 + 1, 2), tame(0x5000, 3), wild(1, 0x5000 - KP[1], 4), wild(0, 0x5000 - KP[0], 7)]
    # key 0 is solved; its OLD entry then solves key 1 as a tame one, and a NEW record of its kangaroo solves key 2 against a stored wild entry
    g2 = 0x2222
    s["solved_acts_as_tame"] = [wild(0, e0, 1), wild(2, g2, 8), tame(0x5000, 3), wild(0, 0x5000 - KP[0], 4), wild(1, e1, 2), wild(0, KP[2] + g2 - KP[0], 1),
                                wild(0, 0x999, 11), wild(0, 0x999, 12)]
    return s


def model_lines(pubs, records):
    t = M.MultiTable(A, W, pubs)
    out = []
    for k, p in enumerate(pubs):
        if p == mul(A):
            t.presolve(k, A)
            out.append("presolved %d" % k)
    for typ, x, d, kid in records:
        fl = 0 if typ == "T" else K.DEAD if typ == "D" else M.wild_flags(int(typ[1:]))
        for e in t.add(x, d & K.M128, kid, fl):
            out.append("found %d %064x" % e[1:] if e[0] == "found" else " ".join(str(v) for v in e))
    out.append("summary %d %d %d %d %d %d" % (len(t.map), t.false_matches, t.reseeds, t.links_kept, t.links_resolved, t.solved()))
    return out, t


def found(k):
    return "found %d %064x" % (k, A + KP[k])


def test_rule_rows():
    S = streams()
    assert model_lines(PUBS, S["tame_wild"])[0] == ["new", "new", found(1), "summary 2 0 0 0 0 1"]
    assert model_lines(PUBS, S["wild_tame"])[0] == ["new", found(1), "summary 1 0 0 0 0 1"]
    assert model_lines(PUBS, S["negative_offset"])[0] == ["new", found(0), "summary 1 0 0 0 0 1"]
    assert model_lines(PUBS, S["same_type"])[0] == ["new", "repeat", "reseed 3", "new", "repeat", "reseed 6", "reseed 5", "summary 2 0 3 0 0 0"]
    assert model_lines(PUBS, S["false_match"])[0] == ["new", "false", "false", "summary 1 2 0 0 0 0"]


def test_links_in_either_order_and_a_chain():
    S = streams()
    assert model_lines(PUBS, S["link_then_second"])[0] == ["new", "link 0 1", "reseed 2", "new", found(1), found(0), "summary 2 0 1 1 1 2"]
    assert model_lines(PUBS, S["link_then_first"])[0] == ["new", "link 0 1", "reseed 2", "new", found(0), found(1), "summary 2 0 1 1 1 2"]
    assert model_lines(PUBS, S["chain"])[0] == ["new", "link 0 1", "reseed 2", "new", "link 2 1", "reseed 6", "new", found(2), found(1), found(0),
                                                "summary 3 0 2 2 2 3"]
    lines, t = model_lines(PUBS, S["false_link"])
    assert lines == ["new", "link 0 1", "reseed 2", "new", found(1), found(0), "summary 2 1 1 1 0 2"]
    assert t.links == []


def test_a_solved_keys_entries_act_as_tame():
    lines, t = model_lines(PUBS, streams()["solved_acts_as_tame"])
    # the last two records: wild kangaroos of the solved key 0 count as tame, so the second of them follows the first and is re-seeded
    assert lines == ["new", "new", "new", found(0), found(1), found(2), "new", "reseed 12", "summary 4 0 1 0 0 3"]
    assert t.keys == [A + KP[0], A + KP[1], A + KP[2], None]


def test_a_key_equal_to_the_start_of_the_range_is_solved_up_front():
    pubs = [PUBS[0], mul(A), PUBS[1]]
    lines, t = model_lines(pubs, [tame(0x5000, 1), ("W2", mul(0x5000)[0], 0x5000 - KP[1], 2)])
    assert lines == ["presolved 1", "new", "found 2 %064x" % (A + KP[1]), "summary 1 0 0 0 0 2"]


def test_assignment():
    asg = M.Assigner(5, {1}, 10)                                  # keys 0 2 3 4 open, ten wild kangaroos
    assert asg.key == [0, 2, 3, 4, 0, 2, 3, 4, 0, 2]
    assert asg.count == [3, 0, 3, 2, 2]
    solved = [False, True, False, False, False]
    assert asg.reseed(4, solved) == 0 and asg.count == [3, 0, 3, 2, 2]          # its key is open: kept
    solved[0] = True
    assert asg.reseed(0, solved) == 3                             # fewest kangaroos: 3 and 4 with two each, the lower position
    assert asg.reseed(4, solved) == 4
    assert asg.reseed(8, solved) == 2                             # now 2, 3, 4 have three each
    assert asg.count == [0, 0, 4, 3, 3]
    # a list longer than the wild herd: the keys without kangaroos get them as others are solved
    asg = M.Assigner(6, set(), 3)
    assert asg.key == [0, 1, 2] and asg.count == [1, 1, 1, 0, 0, 0]
    solved = [True, False, False, False, False, False]
    assert asg.reseed(0, solved) == 3
    solved = [True] * 6
    assert asg.reseed(1, solved) is None


@pytest.mark.parametrize("bits, seed", [(20, 1), (20, 2), (20, 3), (22, 4), (22, 5), (24, 6)])
def test_model_solver_finds_eight_planted_keys(bits, seed):
    Wd = 1 << bits
    a = (0xBEEF << 44) + seed
    rng = K.Stream(900 + seed)
    ks = [a + 1 + rng.u128() % (Wd - 1) for _ in range(7)]
    ks.insert(seed % 8, a)                                        # one key is the start of the range itself
    pubs = [mul(k) for k in ks]
    keys, steps, table = M.solve_multi(pubs, a, a + Wd - 1, seed=seed, n=16)
    assert keys == ks
    assert steps < 8 * 2 * 2 * Wd ** 0.5 + 8 * 16 * 64           # well under eight single searches at twice their expectation


def host_lines(pubs, records):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    args = ["%x" % A, "%x" % (A + W - 1), ",".join(compressed(p) for p in pubs)] + ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in records]
    r = subprocess.run([HOST, "-selftest", "kangaroo-multi"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.split("\n")[:-1]


@pytest.mark.parametrize("name", sorted(streams()))
def test_host_selftest_agrees_with_model(name):
    recs = streams()[name]
    assert host_lines(PUBS, recs) == model_lines(PUBS, recs)[0]


def test_host_selftest_presolves_the_start_of_the_range():
    pubs = [PUBS[0], mul(A), PUBS[1]]
    recs = [tame(0x5000, 1), ("W2", mul(0x5000)[0], 0x5000 - KP[1], 2)]
    assert host_lines(pubs, recs) == model_lines(pubs, recs)[0]


def test_host_selftest_refuses_a_key_outside_the_list():
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    head = [HOST, "-selftest", "kangaroo-multi", "%x" % A, "%x" % (A + W - 1), compressed(PUBS[0])]
    r = subprocess.run(head + ["W0,5,5,1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split("\n")[0] == "new", r.stderr
    r = subprocess.run(head + ["W1,5,5,1"], capture_output=True, text=True, timeout=60)       # key 1 of a list of one
    assert r.returncode == 2 and r.stdout == ""
