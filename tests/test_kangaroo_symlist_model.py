"""CPU: the rule of the symmetric list search (include/bsgs_hip.h "Kangaroo, many keys, symmetric walk") on the model (tests/kangaroo_symlist_model.py) --
every row of the collision table with both signs eps on hand-made streams, a link resolved from either end, a chain of two, a false link, a solved key's old
entry acting as a tame one with sigma = -1, dead and cycle records, the model solver on planted keys -- and the host's table
(bsgs_mi355x -selftest kangaroo-symlist) on the same streams."""
import os
import subprocess
import sys

import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
import kangaroo_symlist_model as SL
from pybsgs.ecpy import N, mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")

A, W = 0x1F << 36, 1 << 24
MID = A + W // 2
KP = [0xABCDE, 0x12345, 0xF00D, 0x3C3C3C]                       # k_k - a of the four keys
KPP = [k - W // 2 for k in KP]                                  # k''_k = k_k - (a + W/2): three negative, one positive
PUBS = [mul(A + k) for k in KP]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def tame(d, kid):
    """a record of a tame kangaroo at offset d: the point d*G (d of either sign)"""
    return ("T", mul(d % N)[0], d, kid)


def wild(k, sg, d, kid):
    """a record of a wild kangaroo of key k at offset d, sigma = sg: the point sg*Q_k + d*G = (sg*k''_k + d)*G"""
    return ("%s%d" % ("W" if sg > 0 else "N", k), mul((sg * KPP[k] + d) % N)[0], d, kid)


E0, F1, G2 = 0x777, -0x4321, 0x2222
E1 = KPP[0] + E0 - KPP[1]                                       # k''_0 + E0 == k''_1 + E1: eps = +1
E1M = KPP[1] - KPP[0] - E0                                      # -k''_1 + E1M == -(k''_0 + E0): a NEG kangaroo of key 1, eps = -1
F2M = KPP[2] - KPP[1] - F1                                      # -k''_2 + F2M == -(k''_1 + F1)


def streams():
    s = {}
    t = tame(0x5000, 1)
    # tame against wild, sigma = +1 and -1, eps = +1 and -1, either one stored first
    s["tame_wild_plus"] = [t, wild(2, 1, 7, 9), wild(1, 1, 0x5000 - KPP[1], 2)]
    s["tame_wild_minus"] = [t, wild(1, 1, -0x5000 - KPP[1], 2)]
    s["neg_wild_tame_plus"] = [wild(2, -1, 0x5000 + KPP[2], 3), t]
    s["neg_wild_tame_minus"] = [wild(2, -1, -0x5000 + KPP[2], 3), t]
    s["tame_neg_wild_minus"] = [t, wild(3, -1, -0x5000 + KPP[3], 4)]
    # wild against wild of the same key: the divisor 2 with either eps, and signs that cancel (equal x by accident: nothing verifies)
    s["same_key_plus"] = [wild(0, 1, 0x10, 1), wild(0, -1, 2 * KPP[0] + 0x10, 2)]
    s["same_key_minus"] = [wild(0, 1, 0x10, 1), wild(0, 1, -2 * KPP[0] - 0x10, 2)]
    w0 = wild(0, 1, 0x10, 1)
    s["same_key_cancel"] = [w0, ("W0", w0[1], 0x11, 2), ("N0", w0[1], -0x10, 3)]
    # a kangaroo's number outlives a re-seed: on a point of its earlier life it is compared like any other -- another key: a link; the same key with the
    # other sign: solved; the same type with another offset: re-seeded, no cycle counted
    s["earlier_life_link"] = [wild(0, 1, E0, 1), wild(1, 1, E1, 1), t, wild(1, 1, 0x5000 - KPP[1], 4)]
    s["earlier_life_solves"] = [wild(0, 1, 0x10, 1), wild(0, -1, 2 * KPP[0] + 0x10, 1)]
    s["earlier_life_same_type"] = [tame(0x6000, 1), tame(-0x6000, 1), wild(2, 1, 5, 2), wild(2, 1, 5, 2)]
    t6 = tame(0x6000, 1)
    s["same_type"] = [t6, t6, ("T", t6[1], 0x6005, 3), tame(-0x6000, 4), wild(0, 1, 5, 5), wild(0, 1, 5, 5), ("D", mul(9)[0], 1, 6), ("C", mul(11)[0], 3, 7)]
    s["false_match"] = [t6, ("W1", t6[1], 0x6001, 2), ("N2", t6[1], 0x6000 - KPP[2] + W, 3)]
    # links: eps = +1 (two W) and eps = -1 (W and N), each resolved from either end
    link01 = [wild(0, 1, E0, 1), wild(1, 1, E1, 2)]
    link01m = [wild(0, 1, E0, 1), wild(1, -1, E1M, 2)]
    solve0, solve1, solve2 = wild(0, 1, 0x5000 - KPP[0], 4), wild(1, 1, 0x5000 - KPP[1], 4), wild(2, 1, 0x5000 - KPP[2], 4)
    t3 = tame(0x5000, 3)
    s["link_then_second"] = link01 + [t3, solve1]
    s["link_then_first"] = link01 + [t3, solve0]
    s["link_minus_then_second"] = link01m + [t3, solve1]
    s["link_minus_then_first"] = link01m + [t3, solve0]
    # a chain: 0 -- 1 (eps +1) and 2 -- 1 (eps -1), then key 2 is solved: 2, 1, 0
    s["chain"] = link01 + [wild(2, -1, F2M, 5), wild(1, 1, F1, 6), t3, solve2]
    # a link whose x agree in the low 64 bits only by accident: dropped and counted when one end is solved, the other key stays open until its own record
    s["false_link"] = [link01[0], ("W1", link01[0][1], E1 + 1, 2), t3, solve1, wild(0, 1, 0x5000 - KPP[0], 7)]
    # key 0 is solved; its OLD entry, of a NEG kangaroo (sigma = -1), then solves key 1 as a tame one; a NEW record of a NEG kangaroo of key 0 solves key 2
    # against a stored wild entry; two more records of key 0, sigma +1 and -1 on one point, are tame and tame
    old = wild(0, -1, E0, 1)
    s["solved_acts_as_tame"] = [old, wild(2, 1, G2, 8), t3, solve0, wild(1, 1, -KPP[0] + E0 - KPP[1], 2), wild(0, -1, KPP[0] + KPP[2] + G2, 1),
                                wild(0, 1, 0x999, 11), wild(0, -1, 2 * KPP[0] + 0x999, 12)]
    return s


def model_lines(pubs, records):
    t = SL.SymListTable(A, W, pubs)
    out = []
    for k, p in enumerate(pubs):
        if p == mul(MID):
            t.presolve(k, MID)
            out.append("presolved %d" % k)
    for typ, x, d, kid in records:
        fl = {"T": 0, "D": K.DEAD, "C": K.DEAD | S.CYCLE, "W": K.WILD, "N": K.WILD | S.NEG}[typ[0]]
        for e in t.add(x, d & K.M128, kid, fl, int(typ[1:]) if typ[0] in "WN" else 0):
            out.append("found %d %064x" % e[1:] if e[0] == "found" else " ".join(str(v) for v in e))
    out.append("summary %d %d %d %d %d %d %d" % (len(t.map), t.false_matches, t.reseeds, t.links_kept, t.links_resolved, t.solved(), t.cycles))
    return out, t


def found(k):
    return "found %d %064x" % (k, A + KP[k])


def test_tame_and_wild_with_both_signs():
    st = streams()
    assert model_lines(PUBS, st["tame_wild_plus"])[0] == ["new", "new", found(1), "summary 2 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["tame_wild_minus"])[0] == ["new", found(1), "summary 1 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["neg_wild_tame_plus"])[0] == ["new", found(2), "summary 1 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["neg_wild_tame_minus"])[0] == ["new", found(2), "summary 1 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["tame_neg_wild_minus"])[0] == ["new", found(3), "summary 1 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["false_match"])[0] == ["new", "false", "reseed 2", "false", "reseed 3", "summary 1 2 2 0 0 0 0"]


def test_same_key_same_type_dead_and_cycle_records():
    st = streams()
    assert model_lines(PUBS, st["same_key_plus"])[0] == ["new", found(0), "summary 1 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["same_key_minus"])[0] == ["new", found(0), "summary 1 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["same_key_cancel"])[0] == ["new", "false", "reseed 2", "false", "reseed 3", "summary 1 2 2 0 0 0 0"]
    # a kangaroo on its own point again runs a long cycle: re-seeded and counted; tame and tame re-seeds whatever the sign (d and -d stand on one x); a dead
    # record re-seeds, a cycle's dead record is counted as well
    assert model_lines(PUBS, st["same_type"])[0] == ["new", "repeat", "reseed 1", "reseed 3", "reseed 4", "new", "repeat", "reseed 5", "reseed 6", "reseed 7", "summary 2 0 6 0 0 0 3"]


def test_a_kangaroo_on_a_point_of_its_earlier_life_is_compared_like_any_other():
    st = streams()
    assert model_lines(PUBS, st["earlier_life_link"])[0] == ["new", "link 0 1", "reseed 1", "new", found(1), found(0), "summary 2 0 1 1 1 2 0"]
    assert model_lines(PUBS, st["earlier_life_solves"])[0] == ["new", found(0), "summary 1 0 0 0 0 1 0"]
    assert model_lines(PUBS, st["earlier_life_same_type"])[0] == ["new", "reseed 1", "new", "repeat", "reseed 2", "summary 2 0 2 0 0 0 1"]


def test_links_with_both_signs_in_either_order_a_chain_and_a_false_link():
    st = streams()
    head = ["new", "link 0 1", "reseed 2", "new"]
    for name in ("link_then_second", "link_minus_then_second"):
        assert model_lines(PUBS, st[name])[0] == head + [found(1), found(0), "summary 2 0 1 1 1 2 0"], name
    for name in ("link_then_first", "link_minus_then_first"):
        assert model_lines(PUBS, st[name])[0] == head + [found(0), found(1), "summary 2 0 1 1 1 2 0"], name
    assert model_lines(PUBS, st["chain"])[0] == ["new", "link 0 1", "reseed 2", "new", "link 2 1", "reseed 6", "new", found(2), found(1), found(0),
                                                 "summary 3 0 2 2 2 3 0"]
    lines, t = model_lines(PUBS, st["false_link"])
    assert lines == head + [found(1), found(0), "summary 2 1 1 1 0 2 0"]
    assert t.links == []


def test_a_solved_keys_entries_act_as_tame_with_sigma_minus_one():
    lines, t = model_lines(PUBS, streams()["solved_acts_as_tame"])
    assert lines == ["new", "new", "new", found(0), found(1), found(2), "new", "reseed 12", "summary 4 0 1 0 0 3 0"]
    assert t.keys == [A + KP[0], A + KP[1], A + KP[2], None]


def test_a_key_in_the_middle_of_the_range_is_solved_up_front():
    pubs = [PUBS[0], mul(MID), PUBS[1]]
    lines, t = model_lines(pubs, [tame(0x5000, 1), ("W2", mul(0x5000)[0], 0x5000 - KPP[1], 2)])
    assert lines == ["presolved 1", "new", "found 2 %064x" % (A + KP[1]), "summary 1 0 0 0 0 2 0"]


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_model_solver_finds_four_planted_keys(seed):
    Wd = 1 << 20
    a = (0xBEEF << 44) + seed
    rng = K.Stream(700 + seed)
    ks = [a + rng.u128() % Wd for _ in range(3)]
    ks.insert(seed % 4, a + Wd // 2 if seed == 2 else a + rng.u128() % Wd)          # once: a key that is the middle of the range itself
    keys, steps, table = SL.solve_symlist([mul(k) for k in ks], a, a + Wd - 1, seed=seed, n=16)
    assert keys == ks
    assert steps < 4 * 2 * 2 * Wd ** 0.5 + 4 * 16 * 64                              # well under four single searches of the plain walk at twice their expectation


def test_step_ratio_tool_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kangaroo_symlist_ratio.py"), "--keys", "3", "--bits", "16", "--seeds", "2", "--jobs", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "ratio" in r.stdout


def host_lines(pubs, records, selftest="kangaroo-symlist", extra=(), env=None):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    args = ["%x" % A, "%x" % (A + W - 1), ",".join(compressed(p) for p in pubs)] + list(extra) + ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in records]
    r = subprocess.run([HOST, "-selftest", selftest] + args, capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return r.stdout.split("\n")[:-1]


@pytest.mark.parametrize("name", sorted(streams()))
def test_host_selftest_agrees_with_model(name):
    recs = streams()[name]
    assert host_lines(PUBS, recs) == model_lines(PUBS, recs)[0]


def test_host_selftest_presolves_the_middle_of_the_range():
    pubs = [PUBS[0], mul(MID), PUBS[1]]
    recs = [tame(0x5000, 1), ("W2", mul(0x5000)[0], 0x5000 - KPP[1], 2)]
    assert host_lines(pubs, recs) == model_lines(pubs, recs)[0]


def test_host_selftest_refuses_a_key_outside_the_list():
    head = [HOST, "-selftest", "kangaroo-symlist", "%x" % A, "%x" % (A + W - 1), compressed(PUBS[0])]
    r = subprocess.run(head + ["N0,5,5,1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split("\n")[0] == "new", r.stderr
    for rec in ("W1,5,5,1", "N1,5,5,1", "T1,5,5,1"):
        r = subprocess.run(head + [rec], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", rec
