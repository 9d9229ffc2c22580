"""CPU: the symmetric kangaroo model (tests/kangaroo_sym_model.py) -- the properties of its step, the cycle check on a hand-built 2-cycle, its solver on planted
keys with both kinds of ending -- and the host's symmetric table (bsgs_mi355x -selftest kangaroo-sym) against the model's verdicts on scripted record streams."""
import os
import subprocess

import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
from pybsgs.ecpy import N, P, add, mul, neg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


def some_states(n, Q):
    rng = K.Stream(5)
    out = []
    for i in range(n):
        wild = i % 2 == 1
        d = S.herd_offset(rng, 1 << 40, wild)
        p = K.start(Q, d, wild)
        out.append((p[0], p[1], d & K.M128, K.WILD if wild else 0))
    return out


@pytest.mark.parametrize("R", [64, 1024])
def test_step_properties(R):
    scalars, jumps = S.jump_table(K.Stream(3), 1 << 30, R)
    Q = mul(0xDEADBEEF12345)
    states = some_states(24, Q)
    assert any(s[1] & 1 for s in states) and any(not s[1] & 1 for s in states)          # starts of both parities
    for st in states:
        last = None
        for n in range(40):
            x, y, d, fl = st
            new, kind = S.step(st, jumps, scalars)
            assert kind == "add" and new[1] & 1 == 0                                     # after any step y is even
            # the point is sigma Q + d G
            sg, dd = S.sigma(new[3]), K.signed128(new[2])
            want = add(mul(dd % N), Q if sg == 1 else neg(Q) if sg == -1 else None)
            assert (new[0], new[1]) == want
            j = (new[3] >> S.LAST_SHIFT) & 0xFFF
            assert new[3] & S.LAST_VALID and j != last                                   # never the same jump twice running
            if last is not None and x & (R - 1) == last:
                assert j == (last + 1) & (R - 1)
            last = j
            # the negated state steps to the same state
            mirror = (x, P - y, (-d) & K.M128, fl ^ S.NEG if fl & K.WILD else fl)
            assert S.step(mirror, jumps, scalars)[0] == new
            st = new


def equal_x_table(even):
    """a 64-point table with a point J_j whose own x selects it and whose y has the wanted parity -> (scalars, jumps, j)"""
    for seed in range(1, 8000):
        scalars, jumps = S.jump_table(K.Stream(seed), 1 << 20, 64)
        for j, p in enumerate(jumps):
            if p[0] & 63 == j and (p[1] & 1 == 0) == even:
                return scalars, jumps, j
    raise AssertionError("no such table")


def test_equal_x_cases_on_the_representative():
    """standing on the class of J_j: a doubling when J_j.y is even (the representative IS J_j), infinity when it is odd (the representative is -J_j)"""
    scalars, jumps, j = equal_x_table(True)
    jx, jy = jumps[j]
    two = mul(2 * scalars[j])
    for st in ((jx, jy, scalars[j], 0), (jx, P - jy, (-scalars[j]) & K.M128, 0)):
        new, kind = S.step(st, jumps, scalars)
        assert kind == "double" and new[0] == two[0] and new[1] & 1 == 0
        assert K.signed128(new[2]) == (2 * scalars[j] if two[1] & 1 == 0 else -2 * scalars[j])
    # with j as the last index the rule moves on to j + 1: an ordinary addition
    new, kind = S.step((jx, jy, 5, S.LAST_VALID | (j << S.LAST_SHIFT)), jumps, scalars)
    assert kind == "add" and (new[3] >> S.LAST_SHIFT) & 0xFFF == (j + 1) & 63
    scalars, jumps, j = equal_x_table(False)
    jx, jy = jumps[j]
    for st in ((jx, jy, 5, K.WILD), (jx, P - jy, 5, K.WILD | S.NEG)):
        new, kind = S.step(st, jumps, scalars)
        assert kind == "dies" and new == st[:3] + (st[3] | K.DEAD,)
        assert S.step(new, jumps, scalars) == (new, "dead")


@pytest.mark.parametrize("R, steps", [(64, 40), (1024, 64), (1024, 17)])
def test_hand_built_cycle_is_retired_within_one_launch(R, steps):
    scalars, jumps, st, a, b = S.short_cycle_case(17, R)
    assert a != b and scalars[a] == scalars[b]
    # without a check it would go round for ever
    s = st
    for n in range(6):
        s, _ = S.step(s, jumps, scalars)
        assert s[:3] == st[:3] if n % 2 else s[:3] != st[:3]
    hist = {0: []}
    final, recs = S.walk([st], jumps, scalars, steps, 32, history=hist)
    assert len(recs) == 1
    x, d, kid, fl, at = recs[0]
    assert fl & K.DEAD and fl & S.CYCLE and kid == 0
    assert at == steps - S.WINDOW + 1 and at >= steps - S.WINDOW                          # two steps after the mark of step S - 1 - C, never before S - C
    assert final[0][3] & K.DEAD and final[0][:3] == (x, hist[0][at][1], d) and x == hist[0][steps - 1 - S.WINDOW][0]
    assert all(h == final[0] for h in hist[0][at:])                                      # it rests
    # a launch of at most C steps has no check
    final, recs = S.walk([st], jumps, scalars, S.WINDOW, 32)
    assert not recs and not final[0][3] & K.DEAD


def test_solver_finds_planted_keys_with_both_endings():
    a = 0x5A5A5 << 40
    W = 1 << 20
    endings = {}
    for n in range(40):
        kp = [0, W - 1, W // 2, W // 2 - 1][n] if n < 4 else (n * 0x9E3779B1) % W
        key, steps, ending, table = S.solve(mul(a + kp), a, a + W - 1, seed=100 + n, n=16)
        assert key == a + kp, (n, kp, key, steps)
        endings[ending] = endings.get(ending, 0) + 1
    assert endings.get("tame-wild", 0) > 0 and endings.get("wild-wild", 0) > 0, endings


def scripted_streams():
    """(name, a, W, pub, records): records as -selftest kangaroo-sym takes them, (type letter T | W | N | D | C, x, d, kangaroo)"""
    a, W = 0x1F << 36, 1 << 24
    mid = a + W // 2
    kp = 0xABCDE
    pub = mul(a + kp)
    Q = add(pub, neg(mul(mid)))
    kk = a + kp - mid                                                 # k'': Q = kk G

    def pt(sg, d):
        return add(mul(d % N), Q if sg == 1 else neg(Q) if sg == -1 else None)

    # tame d_t G == Q + d_w G
    d_w = -(W // 5)
    x_tw = pt(1, d_w)[0]
    tame_wild = [("T", x_tw, kk + d_w, 1), ("W", mul(0x77)[0], 3, 9), ("W", x_tw, d_w, 2)]
    tame_wild_rev = [("W", x_tw, d_w, 2), ("T", x_tw, kk + d_w, 1)]
    # tame d G == -(-Q + e G): the tame one met the mirror image
    tame_neg = [("N", pt(-1, 12345)[0], 12345, 4), ("T", pt(-1, 12345)[0], kk - 12345, 5)]
    tame_neg_mirror = [("T", pt(-1, 999)[0], -(kk - 999), 5), ("N", pt(-1, 999)[0], 999, 4)]
    # wild-wild with opposite sigma: Q + d1 G == -Q + d2 G, d2 - d1 = 2 kk; and through the mirror image, Q + d1 G == -(-Q + d2 G)... the same point class
    d1 = 777
    wild_wild = [("W", pt(1, d1)[0], d1, 6), ("N", pt(1, d1)[0], d1 + 2 * kk, 7)]
    wild_wild_rev = [("N", pt(1, -d1)[0], -d1 + 2 * kk, 7), ("T", mul(31)[0], 31, 1), ("W", pt(1, -d1)[0], -d1, 6)]
    # same kangaroo twice, same type twice, a candidate that does not verify, deaths and cycles
    other = [("T", x_tw, kk + d_w, 1), ("T", x_tw, kk + d_w, 1), ("T", x_tw, 5, 3), ("W", mul(5)[0], 5, 4), ("W", mul(5)[0], 9, 6), ("N", mul(5)[0], 11, 8),
             ("D", mul(9)[0], 1, 5), ("C", mul(10)[0], 2, 5), ("C", mul(10)[0], 2, 6), ("W", x_tw, d_w + 1, 2)]
    names = ["tame_wild", "tame_wild_rev", "tame_neg", "tame_neg_mirror", "wild_wild", "wild_wild_rev", "other"]
    return [(n, a, W, pub, r) for n, r in zip(names, [tame_wild, tame_wild_rev, tame_neg, tame_neg_mirror, wild_wild, wild_wild_rev, other])]


TYPES = {"T": 0, "W": K.WILD, "N": K.WILD | S.NEG, "D": K.DEAD, "C": K.DEAD | S.CYCLE}


def model_verdicts(a, W, pub, records):
    t = S.SymTable(a, W, pub)
    out = []
    for typ, x, d, kid in records:
        v, key = t.add(x, d & K.M128, kid, TYPES[typ])
        out.append("found %064x" % key if v == "found" else "reseed %d" % kid if v == "reseed" else v)
    out.append("summary %d %d %d %d" % (len(t.map), t.false_matches, t.reseeds, t.cycles))
    return out


@pytest.mark.parametrize("name", [s[0] for s in scripted_streams()])
def test_host_selftest_agrees_with_model(name):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    _, a, W, pub, recs = next(s for s in scripted_streams() if s[0] == name)
    want = model_verdicts(a, W, pub, recs)
    args = ["%x" % a, "%x" % (a + W - 1), compressed(pub)] + ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in recs]
    r = subprocess.run([HOST, "-selftest", "kangaroo-sym"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:-1] == want
    if name != "other":
        assert want[-2] == "found %064x" % (a + 0xABCDE), want
    else:
        assert want[:-1] == ["new", "repeat", "reseed 3", "new", "reseed 6", "reseed 8", "reseed 5", "reseed 5", "reseed 6", "reseed 2"]
        assert want[-1] == "summary 2 3 7 2"      # stored, candidates that did not verify, re-seeds, cycles
