"""GPU: the representation contract of csrc/fp256.hip.h, through bsgs_selftest_fe3, bit-exact against Python integers.

The contract ("almost reduced"): every result is below 2^256 and congruent to the true value; fe_add wants ONE canonical operand, fe_sub a canonical
subtrahend, fe_neg a canonical non-zero value; fe_canon and fe_is_p exist because p is a legal encoding of 0.  `raw=True` returns a result as the device
function left it -- what a kernel branches on -- and the canonical form is checked against the integers.  Also here: fe_sqr_add2 on every branch of its
fold's carry accounting (the cases of tests/fe_fold_model.py), fe_sqr on the carry patterns fe_mul is tested with, and fe_inv_block lane by lane."""
import random

import pytest

import fe_fold_model as M

pytestmark = pytest.mark.gpu

P = M.P
KP = M.KP                                                   # 2^256 - p = 2^32 + 977
TOP = 1 << 256
PATTERNS = [2**256 - 1, 2**256 - 2**32, int("ffffffff00000000" * 4, 16), int("00000000ffffffff" * 4, 16),
            int("ffffffff" * 8, 16) - 977, P - 1, P, P + 1, 2**256 - 0x1000003D1 - 1]        # test_gpu_parity.test_fe_mul_carry_patterns


@pytest.fixture(scope="module")
def dev():
    import pybsgs
    d = pybsgs.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def F():
    import pybsgs
    return pybsgs


def canon(v):
    return v - P if v >= P else v


def above_p(rnd, n):
    """n values of [p, 2^256): both ends, then random ones"""
    return ([P, P + 1, TOP - 1, TOP - 2, P + 977, P + (1 << 32)] + [P + rnd.randrange(KP) for _ in range(n)])[:n]


def check(dev, op, a, b, c, want, what):
    """the canonicalised result equals `want`; the raw one is congruent to it (and below 2^256: it has 32 bytes).  -> the raw results"""
    got = dev.selftest_fe3(op, a, b, c)
    bad = [k for k in range(len(a)) if got[k] != want[k]]
    assert not bad, (what, len(bad), [hex(v) for v in (a[bad[0]], (b or a)[bad[0]], (c or a)[bad[0]], got[bad[0]], want[bad[0]])])
    raw = dev.selftest_fe3(op, a, b, c, raw=True)
    bad = [k for k in range(len(a)) if raw[k] % P != want[k]]
    assert not bad, (what + " raw", len(bad), hex(a[bad[0]]), hex(raw[bad[0]]))
    return raw


# ---------------------------------------------------------------------------------------------------------------- fe_sqr_add2
def test_sqr_add2_on_every_branch_of_the_fold(dev, F):
    """the generator's cases (every event of the ADD2 carry accounting: tests/test_fe_fold_model.py) and 4000 random triples, a, c1, c2 over the whole of
    [0, 2^256): the canonical result is (a*a + c1 + c2) % P, the raw one is congruent -- and is the word-for-word model's, bit for bit"""
    cases, counts = M.cases()
    assert all(counts[e] for e in M.EVENTS), counts
    rnd = random.Random(20)
    cases = cases + [(rnd.randrange(TOP), rnd.randrange(TOP), rnd.randrange(TOP)) for _ in range(4000)]
    a, c1, c2 = ([t[k] for t in cases] for k in range(3))
    want = [(x * x + y + z) % P for x, y, z in cases]
    raw = check(dev, F.FE3_SQR_ADD2, a, c1, c2, want, "fe_sqr_add2")
    model = [M.sqr_add2(x, y, z)[0] for x, y, z in cases]
    bad = [k for k in range(len(cases)) if raw[k] != model[k]]
    assert not bad, (len(bad), [hex(v) for v in cases[bad[0]]], hex(raw[bad[0]]), hex(model[bad[0]]))


# ---------------------------------------------------------------------------------------------------------------- fe_sqr, fe_mul
def test_sqr_carry_patterns_single_words_and_single_bits(dev, F):
    """fe_sqr512 is generated code of its own (gen_fp256.py): the pattern list fe_mul is tested with, every single all-ones word, every single bit, pairs
    of words (one cross product alone), and the squares of the mul test's products"""
    words = [0xFFFFFFFF << (32 * k) for k in range(8)]
    a = PATTERNS + words + [1 << i for i in range(256)]
    a += [x | y for i, x in enumerate(words) for y in words[i + 1:]]
    a += [(1 << i) | (1 << j) for i in range(31, 256, 32) for j in range(0, 256, 32)]
    a += [x * y % TOP for x in PATTERNS for y in PATTERNS]
    rnd = random.Random(21)
    a += [rnd.randrange(TOP) for _ in range(2000)]
    want = [x * x % P for x in a]
    check(dev, F.FE3_SQR, a, None, None, want, "fe_sqr")
    assert dev.selftest_fe3(F.FE3_MUL, a, a) == want                                      # sqr(a) == mul(a, a) on the device
    assert dev.selftest_fe(1, a, a) == want


def test_sqr_and_mul_on_operands_in_p_to_2_256(dev, F):
    rnd = random.Random(22)
    hi = above_p(rnd, 300)
    other = [rnd.randrange(TOP) for _ in range(150)] + above_p(rnd, 150)
    rnd.shuffle(other)
    check(dev, F.FE3_SQR, hi, None, None, [x * x % P for x in hi], "fe_sqr above p")
    check(dev, F.FE3_MUL, hi, other, None, [x * y % P for x, y in zip(hi, other)], "fe_mul above p")
    check(dev, F.FE3_MUL, other, hi, None, [x * y % P for x, y in zip(hi, other)], "fe_mul above p, swapped")
    assert dev.selftest_fe3(F.FE3_SQR, hi) == dev.selftest_fe3(F.FE3_MUL, hi, hi)


# ---------------------------------------------------------------------------------------------------------------- operand classes of the contract
def test_add_with_one_operand_above_p(dev, F):
    """a in [p, 2^256), b canonical, in both orders: sums exactly p, 2^256 - 1 and 2^256, sums just past them, and carries out of 2^256 whose folded K
    ripples past word 1 (into word 2 only, and through every word up to 7)"""
    rnd = random.Random(23)
    a, b = [], []
    for x in above_p(rnd, 40):
        k = x - P
        for y in (0, 1, KP - 1 - k, KP - k, KP - k + 1, P - 1, P - 2, rnd.randrange(P),        # x + y = p + k, ..., 2^256 - 1, 2^256, 2^256 + 1
                  (rnd.randrange(1 << 190) << 64) | ((1 << 64) - 1),                            # the wrapped sum's low 64 bits + K overflow: ripple into word 2
                  (0x7FFFFFFF << 224) | ((1 << 224) - 1),                                       # ... through words 2..6 into word 7
                  (1 << 224) - 1, (1 << 64) - 1, (1 << 64) - 1 - k):
            if 0 <= y < P:
                a.append(x)
                b.append(y)
    assert (P, 0) in zip(a, b)                                                                  # the sum that lands exactly on p
    assert any(x + y == TOP - 1 for x, y in zip(a, b)) and any(x + y == TOP for x, y in zip(a, b))
    assert any(x + y >= TOP and ((x + y - TOP) & ((1 << 64) - 1)) + KP >= 1 << 64 for x, y in zip(a, b))
    want = [(x + y) % P for x, y in zip(a, b)]
    raw = check(dev, F.FE3_ADD, a, b, None, want, "fe_add")
    assert raw == [x + y if x + y < TOP else x + y - TOP + KP for x, y in zip(a, b)]            # one wrap, never two
    assert check(dev, F.FE3_ADD, b, a, None, want, "fe_add swapped") == raw


def test_sub_with_the_minuend_above_p_and_rippling_borrows(dev, F):
    """minuend in [p, 2^256), canonical subtrahend: no borrow can occur, differences congruent to 0 come out as p or 0.  And the borrow path with an almost
    reduced minuend below the subtrahend: the K-correction rippling past word 1, into word 2 only and through every word up to 7"""
    rnd = random.Random(24)
    a, b = [], []
    for x in above_p(rnd, 40):
        for y in (0, 1, x - P, max(x - P - 1, 0), x - P + 1, P - 1, rnd.randrange(P), rnd.randrange(KP)):
            a.append(x)
            b.append(y)
    assert any(x - y == P for x, y in zip(a, b))
    for delta in (0, 1, 976, 977, KP - 1, KP, KP + 1):                                          # below K: the correction borrows past word 1
        for j in range(2, 8):                                                                   # (x - y) mod 2^256 = 2^(32 j) + delta: the borrow runs through words 2..j
            x = rnd.randrange(1 << 32)
            a.append(x)
            b.append(x + TOP - (1 << (32 * j)) - delta)
        a.append(7)
        b.append(7 + (3 << 64) - delta)                                                         # words 2..7 all ones after the wrap: one step of ripple
    assert all(y < P for y in b)
    assert any(x < y and ((x - y) % TOP & ((1 << 64) - 1)) < KP for x, y in zip(a, b))
    want = [(x - y) % P for x, y in zip(a, b)]
    raw = check(dev, F.FE3_SUB, a, b, None, want, "fe_sub")
    assert raw == [x - y if x >= y else x - y + TOP - KP for x, y in zip(a, b)]


def test_neg(dev, F):
    rnd = random.Random(25)
    a = [1, 2, P - 1, P - 2, 1 << 32, (1 << 32) - 1, 0xFFFFFC2F, 0xFFFFFC30, (1 << 64) - 1, 1 << 255] + [rnd.randrange(1, P) for _ in range(500)]
    assert dev.selftest_fe3(F.FE3_NEG, a, raw=True) == [P - x for x in a]


def test_canon(dev, F):
    """p - 1, p, p + 1, 2^256 - 1; words 2..7 all ones with the low words on either side of the threshold; one of words 2..7 not all ones (below p whatever
    the low words are); random values"""
    hi = TOP - (1 << 64)
    thr = P & ((1 << 64) - 1)
    a = [0, 1, P - 1, P, P + 1, TOP - 1, TOP - 2]
    a += [hi | lo for lo in (0, 1, thr - 1, thr, thr + 1, (1 << 64) - 1, 0xFFFFFFFE00000000, 0xFFFFFFFEFFFFFC2E, 0xFFFFFFFEFFFFFC30, 0xFFFFFFFDFFFFFFFF,
                             0xFFFFFFFF00000000, 0xFFFFFFFFFFFFFC2E, 0x00000000FFFFFC2F, 0xFFFFFFFE00000000 | 0xFFFFFC2F)]
    for k in range(2, 8):
        for bit in (0, 15, 31):
            for lo in (thr, (1 << 64) - 1, 0):
                a.append(((TOP - 1) ^ (1 << (32 * k + bit))) & ~((1 << 64) - 1) | lo)
        a.append((hi & ~(0xFFFFFFFF << (32 * k))) | thr)
    rnd = random.Random(26)
    a += [rnd.randrange(TOP) for _ in range(300)] + above_p(rnd, 100)
    assert sum(1 for v in a if v >= P) > 100 and sum(1 for v in a if v >> 64 == hi >> 64 and v < P) >= 6
    assert dev.selftest_fe3(F.FE3_CANON, a, raw=True) == [canon(v) for v in a]


def test_inv(dev, F):
    """1, p - 1, values in [p, 2^256) and 0: fe_inv(0) is 0 = 0^(p-2) (and so is fe_inv(p)); the walks rely on no element BEING 0, not on a fault"""
    rnd = random.Random(27)
    a = [0, P, 1, P - 1, 2, P + 1, P + 2, TOP - 1] + above_p(rnd, 40) + [rnd.randrange(TOP) for _ in range(200)]
    want = [pow(v % P, P - 2, P) for v in a]
    assert want[:4] == [0, 0, 1, P - 1]
    check(dev, F.FE3_INV, a, None, None, want, "fe_inv")
    assert dev.selftest_fe(4, a, a) == want


# ---------------------------------------------------------------------------------------------------------------- raw results that kernels branch on
def test_equal_x_detection_sees_exactly_p(dev, F):
    """the tile kernels' fe_is_p(Px + (p - Gx)): fe_add(x, p - x) is exactly p for canonical x != 0, and fe_is_p says so -- and says no one off"""
    rnd = random.Random(28)
    x = [1, 2, P - 1, P - 2, 977, 1 << 32, KP, (1 << 64) - 1, 1 << 255] + [rnd.randrange(1, P) for _ in range(1000)]
    n = [P - v for v in x]
    assert dev.selftest_fe3(F.FE3_NEG, x, raw=True) == n
    assert dev.selftest_fe3(F.FE3_ADD, x, n, raw=True) == [P] * len(x)
    assert dev.selftest_fe3(F.FE3_ADD_IS_P, x, n) == [1] * len(x)
    assert dev.selftest_fe3(F.FE3_ADD_IS_P, n, x) == [1] * len(x)
    near = [(v + 1) % P for v in n]                                                              # x + (p - x + 1) = p + 1; for x = 1 the second operand wraps to 0
    assert dev.selftest_fe3(F.FE3_ADD_IS_P, x, near) == [0] * len(x)
    assert dev.selftest_fe3(F.FE3_ADD_IS_P, x, [v - 1 for v in n]) == [0] * len(x)


def test_is_p_is_false_next_to_p(dev, F):
    a = [P] + [P ^ (1 << i) for i in range(256)] + [P - 1, P + 1, P - 2, P + 2, 0, TOP - 1, P & ((1 << 64) - 1), P - (P & 0xFFFFFFFF)]
    assert dev.selftest_fe3(F.FE3_IS_P, a) == [1] + [0] * (len(a) - 1)


def test_equal_point_detection_sees_exactly_zero(dev, F):
    """kang_element's fe_is_zero(J.x - x): fe_sub(x, x) is exactly 0 -- also for x in [p, 2^256) -- and fe_is_zero says so; p is NOT zero to it"""
    rnd = random.Random(29)
    x = [0, 1, P - 1, P, TOP - 1] + [rnd.randrange(P) for _ in range(500)] + above_p(rnd, 20)
    assert dev.selftest_fe3(F.FE3_SUB, x, x, raw=True) == [0] * len(x)
    assert dev.selftest_fe3(F.FE3_SUB_IS_ZERO, x, x) == [1] * len(x)
    y = [v ^ (1 << rnd.randrange(256)) for v in x]
    ok = [k for k in range(len(x)) if y[k] < P]                                                  # fe_sub wants a canonical subtrahend
    assert len(ok) > 400
    assert dev.selftest_fe3(F.FE3_SUB_IS_ZERO, [x[k] for k in ok], [y[k] for k in ok]) == [0] * len(ok)
    a = [0] + [1 << i for i in range(256)] + [P, TOP - 1, KP]
    assert dev.selftest_fe3(F.FE3_IS_ZERO, a) == [1] + [0] * (len(a) - 1)
    # x - y with x = y + p (the difference is congruent to 0): the raw result is p, which fe_is_zero does not take for zero
    small = [rnd.randrange(KP) for _ in range(50)]
    assert dev.selftest_fe3(F.FE3_SUB, [P + v for v in small], small, raw=True) == [P] * 50
    assert dev.selftest_fe3(F.FE3_SUB_IS_ZERO, [P + v for v in small], small) == [0] * 50


def test_eq_is_true_on_identical_words_only(dev, F):
    """fe_eq compares words, not residues: fe_eq(0, p) is FALSE, which is why its callers canonicalise first (the cycle check compares two fe_canon results,
    kang_element two canonical y).  Asserted so that nobody turns it into a comparison mod p behind their backs."""
    rnd = random.Random(30)
    x = [0, P, TOP - 1, 1] + [rnd.randrange(TOP) for _ in range(60)]
    assert dev.selftest_fe3(F.FE3_EQ, x, x) == [1] * len(x)
    a = [v for v in x[:8] for i in range(256)]
    b = [v ^ (1 << i) for v in x[:8] for i in range(256)]
    assert dev.selftest_fe3(F.FE3_EQ, a, b) == [0] * len(a)
    pairs = [(0, P), (P, 0), (1, P + 1), (KP - 1, TOP - 1)]
    assert all((u - v) % P == 0 for u, v in pairs)
    assert dev.selftest_fe3(F.FE3_EQ, [u for u, _ in pairs], [v for _, v in pairs]) == [0] * len(pairs)


# ---------------------------------------------------------------------------------------------------------------- fe_inv_block
def block_inputs(rnd, W, blocks):
    """one element per thread, blocks of 64 * W: block b has leader b & (W - 1) and scenario b // W, so every scenario meets every leader.
    0: random canonical values; 1: the wave lane % W of each lane position holds a value of [p, 2^256) (never p itself: that is 0), lanes 0..7 hold them in
    every wave; 2: all waves of a lane position hold the same value; 3: wave lane % W holds 1, the next wave p - 1, the others random; then 0 again"""
    out = []
    for b in range(blocks):
        scen = (b // W) % 4
        blk = [[rnd.randrange(1, P) for _ in range(64)] for _ in range(W)]
        for lane in range(64):
            if scen == 1:
                for w in range(W):
                    if w == lane % W or lane < 8:
                        blk[w][lane] = P + 1 + rnd.randrange(KP - 1)
            elif scen == 2:
                for w in range(1, W):
                    blk[w][lane] = blk[0][lane]
            elif scen == 3:
                blk[lane % W][lane] = 1
                blk[(lane + 1) % W][lane] = P - 1
        out += [v for wave in blk for v in wave]
    return out


@pytest.mark.parametrize("name, W", [("FE3_INV_BLOCK_KANG", 4), ("FE3_INV_BLOCK_SEED", 4), ("FE3_INV_BLOCK_TILE", 4), ("FE3_INV_BLOCK2_TILE", 2),
                                     ("FE3_INV_BLOCK2_TILE_PAIR128", 2)])
def test_inv_block_gives_every_lane_its_own_inverse(dev, F, name, W):
    """fe_inv_block<REGION, W> with the REGION of each of its callers, 20 blocks (every leader five times): each thread gets the inverse of ITS element --
    the values of a lane position's waves are distinct in scenarios 0, 1 and 3, so a neighbour's inverse cannot pass"""
    op = getattr(F, name)
    rnd = random.Random(31 + op)
    x = block_inputs(rnd, W, 20)
    assert len(x) == 20 * 64 * W
    want = [pow(v % P, -1, P) for v in x]
    got = dev.selftest_fe3(op, x)
    bad = [k for k in range(len(x)) if got[k] != want[k]]
    assert not bad, (name, len(bad), "first at block %d wave %d lane %d" % (bad[0] // (64 * W), bad[0] // 64 % W, bad[0] % 64))
    raw = dev.selftest_fe3(op, x, raw=True)
    assert [v % P for v in raw] == want
    # a wave's result is not another wave's: where the inputs differ, so do the results
    for k in range(0, len(x), 64 * W):
        for lane in range(64):
            col = [(x[k + 64 * w + lane] % P, got[k + 64 * w + lane]) for w in range(W)]
            assert len(set(col)) == len(set(v for v, _ in col))


def test_inv_block_refuses_partial_blocks_and_unknown_ops(dev, F):
    with pytest.raises(F.BsgsError):
        dev.selftest_fe3(F.FE3_INV_BLOCK_KANG, [1] * 200)
    with pytest.raises(F.BsgsError):
        dev.selftest_fe3(F.FE3_INV_BLOCK2_TILE, [1] * 192)
    for op in (-1, 13, 15, 21):
        with pytest.raises(F.BsgsError):
            dev.selftest_fe3(op, [1] * 64)
