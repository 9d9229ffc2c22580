"""GPU: the 128-bit distance word of both kangaroo walks (csrc/kangaroo.hip) away from zero, and the DP mask at the ends of what kangaroo_alloc accepts.

The walks advance d with a four-word carry chain and the symmetric walk negates it with a four-word borrow chain; the other walk tests seed |d| < 2^44, so
words 2 and 3 never see a carry there.  Here an ordinary herd gets chosen slots' d overwritten -- the models carry d without relating it to the point, so any
value is allowed -- and states and the full record list must equal the models'.  The crafted distinguished points of the dp = 32 tests are built by the
chord formulas alone (see crafted_dp_states); the test of that construction needs no GPU."""
import random

import pytest

import kangaroo_model as K
import kangaroo_sym_model as S
from pybsgs.ecpy import P, add, mul, neg

M128 = K.M128
GEOMETRIES = [(2048, 8), (1024, 16)]                       # blocks of 256 threads (one inversion per block) / of 64 (one per thread)


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


def herd(model, seed, W, Q, n):
    rng = K.Stream(seed)
    out = []
    for i in range(n):
        wild = i >= n // 2
        d = model.herd_offset(rng, W, wild)
        p = K.start(Q, d, wild)
        out.append((p[0], p[1], d & M128, K.WILD if wild else 0))
    return out


def rec_key(r):
    return (r["x"], r["d"], r["kangaroo"], r["flags"], r["step"])


def distances(sj):
    """the values the carry and borrow chains should meet, for a slot whose first jump adds sj: each v as it is (the addition sees it), v - sj (the addition
    ends on it, and the symmetric walk negates THAT when the step lands on odd y) and -v (a start of odd y negates first: the addition then sees v)"""
    base = [0, (1 << 64) - 1, (1 << 64) - sj, (1 << 96) - 1, (1 << 96) - sj, (1 << 127) - 1, (1 << 128) - 1, (1 << 128) - sj, 1 << 127, (1 << 127) - sj,
            1 << 32, 1 << 64, 1 << 96, 5 << 32, 7 << 64, 9 << 96, (1 << 127) | (1 << 96), ((1 << 64) - 1) << 64, ((1 << 96) - 1) << 32]
    return [u & M128 for v in base for u in (v, v - sj, -v)]


N_DIST = len(distances(1))


def run_and_compare(dev, model, states, jumps, scalars, launches, dp):
    n = len(states)
    dev.kangaroo_upload(0, states)
    assert dev.kangaroo_download(0, n) == states
    model_recs, gpu_recs = [], []
    for k, launch in enumerate(launches):
        states, recs = model.walk(states, jumps, scalars, launch, dp)
        model_recs += [r[:4] + (k, r[4]) for r in recs]
        got, dropped, _ = dev.kangaroo_run(launch)
        assert dropped == 0
        gpu_recs += [rec_key(r)[:4] + (k, r["step"]) for r in got]
        down = dev.kangaroo_download(0, n)
        bad = [i for i in range(n) if down[i] != states[i]]
        assert not bad, (k, len(bad), bad[:4], [hex(v) for v in down[bad[0]]], [hex(v) for v in states[bad[0]]])
    assert sorted(gpu_recs) == sorted(model_recs)
    return states, model_recs


# ---------------------------------------------------------------------------------------------------------------- the distance word
@pytest.mark.gpu
@pytest.mark.parametrize("n, per_thread", GEOMETRIES)
def test_plain_walk_carries_d_through_all_four_words(dev, n, per_thread):
    W = 1 << 40
    Q = mul(0x1234567890ABCDEF1234)
    scalars, jumps = K.jump_table(K.Stream(78), n * (W ** 0.5) / 4)
    states = herd(K, 2000 + n, W, Q, n)
    placed = {}
    for k in range(N_DIST):                                                     # one value per slot, the slots 11 apart: tame and wild, every wave, many threads
        slot = 1 + 11 * k
        x, y, _, fl = states[slot]
        placed[slot] = distances(scalars[x & 63])[k]
        states[slot] = (x, y, placed[slot], fl)
    dev.kangaroo_setup(jumps, scalars, 0, n, per_thread, 1 << 16)
    vals = set(placed.values())
    assert {0, (1 << 64) - 1, (1 << 96) - 1, (1 << 127) - 1, (1 << 128) - 1, 1 << 127, 1 << 32, 1 << 64, 1 << 96} <= vals and len(placed) == N_DIST and 11 * N_DIST < n
    # carries into word 2 and into word 3, and the wrap to zero, really happen in the first step
    first = {i: K.step(states[i], jumps, scalars)[0][2] for i in placed}
    assert any(placed[i] < 1 << 64 <= first[i] for i in placed) and any(placed[i] < 1 << 96 <= first[i] for i in placed)
    assert any(first[i] < placed[i] for i in placed)
    final, recs = run_and_compare(dev, K, states, jumps, scalars, [1, 1, 6], 0)
    assert len(recs) == 8 * n                                                   # dp = 0: every step of every kangaroo is a record, d included


@pytest.mark.gpu
@pytest.mark.parametrize("n, per_thread", GEOMETRIES)
def test_symmetric_walk_negates_d_through_all_four_words(dev, n, per_thread):
    """every value on a slot whose start has odd y (negated before the step) and on a slot whose first step lands on odd y (negated after it): the borrow chain
    meets 0 and 2^127 (their own negatives), values with one, two and three zero low words, and all ones"""
    R = 64
    W = 1 << 40
    a = 0x123456789 << 40
    Q = add(mul(a + 0x9876543210), neg(mul(a + W // 2)))
    scalars, jumps = S.jump_table(K.Stream(79), n * (W ** 0.5) / 4, R)
    states = herd(S, 3000 + n, W, Q, n)

    def lands_odd(st):
        x, y, _, _ = st
        return y & 1 == 0 and add((x, y), jumps[S.jump_index(x, 0, R)])[1] & 1 == 1

    odd_start = [i for i in range(n) if states[i][1] & 1]
    odd_landing = [i for i in range(n) if lands_odd(states[i])]
    placed = {}
    for slots in (odd_start, odd_landing):
        spread = slots[::3]                                                     # over the whole herd: tame and wild
        assert len(spread) >= N_DIST
        for k in range(N_DIST):
            i = spread[k]
            x, y, _, fl = states[i]
            placed[i] = distances(scalars[S.jump_index(x, 0, R)])[k]
            states[i] = (x, y, placed[i], fl)
        done = {placed[i] for i in spread[:N_DIST]}
        assert {0, 1 << 127, (1 << 128) - 1, 1 << 32, 1 << 64, 1 << 96, (1 << 64) - 1, (1 << 127) - 1} <= done
    dev.kangaroo_setup_sym(jumps, scalars, 0, n, per_thread, 1 << 17)
    # the negation really runs on 0, on 2^127 and on values with zero low words: before the step (odd start) and after it (odd landing, d = v - s_j)
    negated_before = {placed[i] for i in placed if i in set(odd_start)}
    negated_after = {(placed[i] + scalars[S.jump_index(states[i][0], 0, R)]) & M128 for i in placed if i in set(odd_landing)}
    for seen in (negated_before, negated_after):
        assert {0, 1 << 127, 1 << 32, 1 << 64, 1 << 96} <= seen
    final, recs = run_and_compare(dev, S, states, jumps, scalars, [1, 1, 1, S.WINDOW + 3], 0)
    assert all(s[1] & 1 == 0 for s in final)


# ---------------------------------------------------------------------------------------------------------------- the DP mask at its ends
@pytest.mark.gpu
@pytest.mark.parametrize("n, per_thread", GEOMETRIES)
@pytest.mark.parametrize("sym", [False, True])
def test_dp_1(dev, n, per_thread, sym):
    model = S if sym else K
    W = 1 << 36
    Q = mul(0xABCDEF0123)
    if sym:
        scalars, jumps = S.jump_table(K.Stream(80), 1 << 30, 64)
        dev.kangaroo_setup_sym(jumps, scalars, 1, n, per_thread, 1 << 16)
    else:
        scalars, jumps = K.jump_table(K.Stream(80), 1 << 30)
        dev.kangaroo_setup(jumps, scalars, 1, n, per_thread, 1 << 16)
    final, recs = run_and_compare(dev, model, herd(model, 81, W, Q, n), jumps, scalars, [1, 7], 1)
    assert all(r[0] >> 255 == 0 for r in recs) and n * 8 * 0.4 < len(recs) < n * 8 * 0.6
    assert any(r[0] >> 254 for r in recs)                                       # bit 254 is not part of the mask


def crafted_dp_states(model, jumps, scalars, targets, seed):
    """For each target x3 a state whose NEXT step lands exactly on x = x3: no search finds an x with 32 zero top bits, so it is built.  In the add case the
    kernels and the models apply the plain chord formulas, which never use the curve constant: for ANY (x3, y3) and a jump J_j the predecessor
    chord((x3, y3), -J_j) steps back onto (x3, y3) -- the line through the predecessor and J_j is the mirror image of the line through (x3, y3) and -J_j, slope -lambda, and x3, y3 drop out of the formulas again.
    It is kept when the walk's index rule picks that same j for it (and, in the symmetric walk, when its y is even: it is its class's representative);
    otherwise y3 varies.  The models' add (pybsgs.ecpy.add) takes off-curve input as it is, so no helper of the test's own is needed.
    -> [(state, j)] with d a fixed pattern and no flags"""
    rnd = random.Random(seed)
    R = len(jumps)
    out = []
    for x3 in targets:
        found = None
        for _ in range(400):
            y3 = rnd.randrange(1, P)
            for j in range(R):
                pred = add((x3, y3), neg(jumps[j]))
                if pred is None or pred[0] == jumps[j][0]:
                    continue
                if model is S and (pred[1] & 1 or S.jump_index(pred[0], 0, R) != j):
                    continue
                if model is K and pred[0] & (K.NJ - 1) != j:
                    continue
                found = (pred, j, y3)
                break
            if found:
                break
        assert found, hex(x3)
        pred, j, y3 = found
        assert add(pred, jumps[j]) == (x3, y3)
        out.append(((pred[0], pred[1], (0xD15 << 100) + len(out), 0), j))
    return out


TARGETS_IN = [(1 << 224) - 1, 5, 1 << 223, 0x1234 << 200, (1 << 224) - (1 << 32)]      # 32 zero top bits
TARGETS_OUT = [1 << 224, (1 << 224) + 5, 1 << 255]                                    # one bit inside the mask


@pytest.mark.parametrize("sym", [False, True])
def test_crafted_predecessors_step_onto_their_targets(sym):
    """no GPU: the models accept the crafted (off-curve) states and return the targets, DP or not by the top 32 bits alone"""
    model = S if sym else K
    scalars, jumps = S.jump_table(K.Stream(82), 1 << 30, 64)
    crafted = crafted_dp_states(model, jumps, scalars, TARGETS_IN + TARGETS_OUT, 83)
    for (st, j), x3 in zip(crafted, TARGETS_IN + TARGETS_OUT):
        new, kind = model.step(st, jumps, scalars)
        assert kind == "add" and new[0] == x3 and new[2] in ((st[2] + scalars[j]) & M128, -(st[2] + scalars[j]) & M128)
        assert K.is_dp(new[0], 32) == (x3 in TARGETS_IN)
    _, recs = model.walk([st for st, _ in crafted], jumps, scalars, 1, 32)
    assert [r[2] for r in recs] == list(range(len(TARGETS_IN)))


@pytest.mark.gpu
@pytest.mark.parametrize("n, per_thread", GEOMETRIES)
@pytest.mark.parametrize("sym", [False, True])
def test_dp_32(dev, n, per_thread, sym):
    """exactly the crafted slots produce records at dp = 32, on the step that lands them on x < 2^224; the near misses (x = 2^224, ...) and the rest of the herd
    produce none; every state equals the model's"""
    model = S if sym else K
    scalars, jumps = S.jump_table(K.Stream(82), 1 << 30, 64)
    if sym:
        dev.kangaroo_setup_sym(jumps, scalars, 32, n, per_thread, 1 << 12)
    else:
        dev.kangaroo_setup(jumps, scalars, 32, n, per_thread, 1 << 12)
    states = herd(model, 84, 1 << 36, mul(0x5555555555), n)
    crafted = crafted_dp_states(model, jumps, scalars, TARGETS_IN + TARGETS_OUT, 83)
    slots = [3 + 67 * k for k in range(len(crafted))]                          # several waves and threads; 3 + 67 * 7 < 1024
    for i, (st, _) in zip(slots, crafted):
        states[i] = st
    final, recs = run_and_compare(dev, model, states, jumps, scalars, [1, 3], 32)
    want = slots[:len(TARGETS_IN)]
    assert sorted((r[2], r[0], r[4], r[5]) for r in recs) == sorted((i, x3, 0, 0) for i, x3 in zip(want, TARGETS_IN))
    for i, (st, j) in zip(want, crafted):
        assert [r[1] for r in recs if r[2] == i] == [model.step(st, jumps, scalars)[0][2]]
