"""CPU: the kangaroo model (tests/kangaroo_model.py) solves planted keys and re-seeds followers, and the host's table of distinguished points
(bsgs_mi355x -selftest kangaroo) gives the model's verdicts on scripted record streams."""
import os
import subprocess

import pytest

import kangaroo_model as K
from pybsgs.ecpy import mul, neg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")


def compressed(p):
    return ("03" if p[1] & 1 else "02") + "%064x" % p[0]


@pytest.mark.parametrize("bits, where", [(20, "low"), (20, "high"), (21, "mid"), (22, "mid"), (24, "mid")])
def test_model_solves_planted_keys(bits, where):
    a = 0x5A5A5 << 40
    W = 1 << bits
    kp = {"low": 0, "high": W - 1, "mid": (W * 7) // 11}[where]
    key, steps = K.solve(mul(a + kp), a, a + W - 1, seed=bits * 7 + len(where), n=16)
    assert key == a + kp, (key, steps)


def test_step_equal_x_cases():
    """x == J_j.x: a doubling when y == J_j.y, death (one record, state kept) when y == -J_j.y"""
    # a jump table with a point whose own x selects it (about one table in three)
    seed = next(s for s in range(1, 2000) if any(p[0] & 63 == j for j, p in enumerate(K.jump_table(K.Stream(s), 1 << 20)[1])))
    scalars, jumps = K.jump_table(K.Stream(seed), 1 << 20)
    j = next(j for j in range(K.NJ) if jumps[j][0] & 63 == j)
    jx, jy = jumps[j]
    st, kind = K.step((jx, jy, 5, 0), jumps, scalars)
    assert kind == "double" and (st[0], st[1]) == mul(2 * scalars[j]) and st[2] == 5 + scalars[j]
    st, kind = K.step((jx, neg(jumps[j])[1], 5, K.WILD), jumps, scalars)
    assert kind == "dies" and st == (jx, neg(jumps[j])[1], 5, K.WILD | K.DEAD)
    assert K.step(st, jumps, scalars) == (st, "dead")


def test_walk_records_dps_and_deaths():
    scalars, jumps = K.jump_table(K.Stream(11), 1 << 30)
    states = [(p[0], p[1], d, 0) for d, p in ((d, mul(d)) for d in range(1, 9))]
    final, recs = K.walk(states, jumps, scalars, 20, 2)
    assert all(K.is_dp(x, 2) for x, *_ in recs) and recs
    for x, d, kid, fl, s in recs:
        assert 0 <= s < 20 and 0 <= kid < 8
    for i, (x, y, d, fl) in enumerate(final):
        assert (x, y) == mul(d)                              # tame kangaroos stay at d*G


def test_same_type_collision_is_reseeded():
    a, W = 1 << 40, 1 << 22
    pub = mul(a + 12345)
    t = K.DPTable(a, W, pub)
    x = mul(777)[0]
    assert t.add(x, 777, 1, 0) == ("new", None)
    assert t.add(x, 777, 1, 0) == ("repeat", None)
    assert t.add(x, 777, 2, 0) == ("reseed", None)       # tame follows tame
    y = mul(999)[0]
    assert t.add(y, 5, 3, K.WILD) == ("new", None)
    assert t.add(y, 9, 4, K.WILD) == ("reseed", None)    # wild follows wild
    assert t.reseeds == 2


def test_walked_followers_are_reseeded():
    """two tame kangaroos on the same point walk the same path: the table re-seeds the later one at its first DP"""
    a, W = 1 << 32, 1 << 20
    scalars, jumps = K.jump_table(K.Stream(5), 64)
    p = mul(1000)
    _, recs = K.walk([(p[0], p[1], 1000, 0), (p[0], p[1], 1000, 0)], jumps, scalars, 40, 1)
    t = K.DPTable(a, W, mul(a + 1))
    verdicts = [(kid, t.add(x, d, kid, fl)[0]) for x, d, kid, fl, _ in recs]
    assert verdicts and verdicts[0] == (0, "new") and verdicts[1] == (1, "reseed")


def scripted_streams():
    """(name, a, W, pub, records) -- records as the host's selftest takes them: (type letter, x, d mod 2^128, kangaroo)"""
    a, W = 0x1F << 36, 1 << 24
    kp = 0xABCDE
    pub = mul(a + kp)
    # a tame / wild collision: tame at d_T*G, wild at Q + d_W*G with d_T = k' + d_W
    d_w = -(W // 3)
    d_t = kp + d_w
    xt = mul(d_t)[0]
    collide = [("T", xt, d_t, 1), ("W", mul(0x77)[0], 0x77 - kp, 9), ("W", xt, d_w, 2)]
    # the wild record first, then the tame one
    collide_rev = [("W", xt, d_w, 2), ("T", xt, d_t, 1)]
    # same type: the later kangaroo is re-seeded, its own repeat is not
    same = [("T", xt, d_t, 1), ("T", xt, d_t, 1), ("T", xt, d_t + 5, 3), ("W", mul(5)[0], 5, 4), ("W", mul(5)[0], 5, 6)]
    # a false match: x equal in the key, difference out of range or not solving; then a death
    false = [("T", xt, d_t, 1), ("W", xt, d_t + 1, 2), ("W", mul(3)[0], 3, 7), ("T", mul(3)[0], 3 + W, 8), ("D", mul(9)[0], 1, 5)]
    return [("collide", a, W, pub, collide), ("collide_rev", a, W, pub, collide_rev), ("same", a, W, pub, same), ("false", a, W, pub, false)]


def model_verdicts(a, W, pub, records):
    t = K.DPTable(a, W, pub)
    out = []
    for typ, x, d, kid in records:
        v, key = t.add(x, d, kid, {"T": 0, "W": K.WILD, "D": K.DEAD}[typ])
        out.append("found %064x" % key if v == "found" else "reseed %d" % kid if v == "reseed" else v)
    out.append("summary %d %d %d" % (len(t.map), t.false_matches, t.reseeds))
    return out


@pytest.mark.parametrize("name", ["collide", "collide_rev", "same", "false"])
def test_host_selftest_agrees_with_model(name):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    _, a, W, pub, recs = next(s for s in scripted_streams() if s[0] == name)
    want = model_verdicts(a, W, pub, recs)
    args = ["%x" % a, "%x" % (a + W - 1), compressed(pub)] + ["%s,%x,%x,%d" % (t, x, d & K.M128, kid) for t, x, d, kid in recs]
    r = subprocess.run([HOST, "-selftest", "kangaroo"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:-1] == want
    if name.startswith("collide"):
        assert ("found %064x" % (a + 0xABCDE)) in want


def test_host_rejects_kangaroo_flag_combinations_without_a_gpu():
    """refused at the command line, before any device is looked for"""
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    for extra in (["-w", "30"], ["-htsz", "25"], ["-infile", "x.txt"], ["-wl", "currentwork.txt"], ["-onlygen"]):
        r = subprocess.run([HOST, "-kangaroo"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, extra
    r = subprocess.run([HOST, "-kangaroo", "-wl", "c.txt"], capture_output=True, text=True, timeout=60)
    assert "not supported" in r.stderr
