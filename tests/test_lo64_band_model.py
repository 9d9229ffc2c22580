"""The low-64-bit squaring (fe_sqr_add2_lo64) computes only the product columns 0, 1 and 6..9 of lambda^2 and bounds the carry of columns 2..5 into word 7
(fp256.hip.h, DESIGN_HISTORY.md 1).  A Python-int model of it, step by step as the device runs it, against (lambda^2 + c1 + c2) mod p: random and crafted
cases, and the bounds the derivation rests on.  No GPU."""
import random

from lo64_band_model import (B, DELTA_BOUND, DROP_MAX, M32, P, crafted_lambdas, craft_rest_lo, craft_w7, limbs, lo64, true_rest, want, win69, win_exact)


def _check(lam, c1, c2):
    """the fast key equals the exact one unless the lane is flagged; the bounds of the derivation hold.  Returns the slow flag"""
    x, slow, rest, w7 = lo64(lam, c1, c2)
    a = limbs(lam)
    S = lam * lam
    words = [(S >> (32 * k)) & M32 for k in range(10)]
    band = win_exact(lam)
    assert win69(a) == band
    # columns 0 and 1 give words 0 and 1; lo2 + drop puts 0..6 into word 7 of the band
    lo2 = a[0] * a[0] + ((2 * a[0] * a[1]) << 32)
    assert words[0] | (words[1] << 32) == lo2 & ((1 << 64) - 1)
    e = (words[7] - band[0]) % B
    assert e <= 6
    if w7 < B - 8:
        assert words[7] == band[0] + e and words[8:10] == band[1:3]
    th = (a[7] * a[7] + ((a[6] * a[7]) >> 31)) >> 32
    if th < 0xFFFFF000 and w7 < B - 8:
        delta = true_rest(lam, c1, c2) - rest
        assert 0 <= delta < DELTA_BOUND, delta
    if not slow:
        assert x == want(lam, c1, c2), hex(lam)
    return slow


def test_drop_bound_is_exact():
    """lo2 + drop with every limb all ones: the bound the carry into word 7 rests on (< 6 B^7, so at most 6 with the band's own words 0..6)"""
    assert DROP_MAX == sum((B - 1) ** 2 * (k + 1) * B ** k for k in range(6))
    assert 5 * B ** 7 < DROP_MAX < 6 * B ** 7
    lam = (1 << 192) - 1
    S = lam * lam
    a = limbs(lam)
    band_lo = sum(2 * a[i] * a[j] * B ** (i + j) for i in range(8) for j in range(i + 1, 8) if i + j <= 5) + sum(a[i] ** 2 * B ** (2 * i) for i in range(3))
    assert band_lo == DROP_MAX and S % B ** 10 == (DROP_MAX + sum(2 * a[i] * a[j] * B ** (i + j) for i in range(8) for j in range(i + 1, 8) if 6 <= i + j <= 9)
                                                   + a[3] ** 2 * B ** 6 + a[4] ** 2 * B ** 8) % B ** 10


def test_random_cases():
    rnd = random.Random(20261015)
    slow = 0
    for _ in range(20000):
        lam, c1, c2 = rnd.randrange(1 << 256), rnd.randrange(P), rnd.randrange(P)
        slow += _check(lam, c1, c2)
    assert slow <= 2                                     # ~2^-19 of the lanes


def test_crafted_lambdas():
    rnd = random.Random(7)
    for label, lams in crafted_lambdas(rnd):
        for lam in lams:
            c1, c2 = rnd.randrange(P), rnd.randrange(P)
            slow = _check(lam, c1, c2)
            w7 = win69(limbs(lam))[0]
            if label == "w7_near_wrap":
                assert w7 >= B - 8 and slow
            if label == "w7_below_wrap":
                assert B - 17 <= w7 < B - 8


def test_w7_near_wrap_needs_the_exact_path():
    """w7' within 8 of wrapping with the largest drop: the dropped carry does move words 8, 9 for some of them, so the fast words would be wrong; every
    such lane is flagged"""
    rnd = random.Random(11)
    moved = 0
    for _ in range(400):
        lam = craft_w7(rnd, B - 1 - rnd.randrange(8), low_ones=True)
        S = lam * lam
        moved += [(S >> (32 * k)) & M32 for k in (8, 9)] != win_exact(lam)[1:]
        assert _check(lam, rnd.randrange(P), rnd.randrange(P))
    assert moved > 0


def test_rest_at_the_4096_edge():
    """lo32(Rest) just below 2^32 - 4096 stays on the fast path and is exact; at and above it the lane takes the exact path"""
    rnd = random.Random(13)
    for lam in [rnd.randrange(1 << 256) for _ in range(200)] + [(1 << 256) - 2, (1 << 192) - 1, P - 1]:
        c2 = rnd.randrange(P)
        for target, expect_slow in ((0xFFFFEFFF, False), (0xFFFFEFFF - 1967, False), (0xFFFFF000, True), (0xFFFFFFFF, True)):
            c1 = craft_rest_lo(lam, c2, target, rnd)
            assert c1 < P
            x, slow, rest, w7 = lo64(lam, c1, c2)
            assert rest & M32 == target
            th = ((limbs(lam)[7] ** 2 + ((limbs(lam)[6] * limbs(lam)[7]) >> 31)) >> 32)
            if th < 0xFFFFF000 and w7 < B - 8:
                assert slow == expect_slow
            _check(lam, c1, c2)

