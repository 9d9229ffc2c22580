"""Python-int model of fe_sqr_add2_lo64 (csrc/fp256.hip.h) with the banded square fe_sqr_win69 (csrc/gen_fp256.py), step by step as the device
computes it, and the crafted lambdas the CPU and GPU tests of the low-64-bit squaring share.  TEST INFRASTRUCTURE: no product code is called.

    S = a^2 mod B^10 = lo2 + drop + win   (B = 2^32; column k = the products a_i a_j with i + j = k)
    lo2 = columns 0, 1   drop = columns 2..5 (never computed)   win = columns 6..9 (13 cross products doubled, a3^2, a4^2)
"""
import random

B = 1 << 32
M32 = B - 1
M64 = (1 << 64) - 1
P = (1 << 256) - (1 << 32) - 977
K977 = 977
DROP_MAX = sum((B - 1) ** 2 * B ** (i + j) for i in range(6) for j in range(6) if i + j <= 5)   # lo2 + drop, every limb all ones
DELTA_BOUND = 1968                                                                               # 0 <= floor(T / B^7) - Rest < DELTA_BOUND


def limbs(x):
    return [(x >> (32 * i)) & M32 for i in range(8)]


def win69(a):
    """(w7', w8', w9'): fe_sqr_win69 as generated -- Comba columns 6, 7 with carry counts, 8 and 9 wrapping mod 2^64, the 1-bit funnel doubling and the
    diagonal squares a3^2, a4^2 by one carry chain over words 6..9"""
    acc, x = 0, {}
    for k in range(6, 10):
        s = acc + sum(a[i] * a[k - i] for i in range(8) if 0 <= k - i <= 7 and i < k - i)
        if k >= 8:
            s &= M64                                      # no carry count: only words 8 and 9 are read
        x[k] = s & M32
        acc = s >> 32
    d3, d4 = a[3] * a[3], a[4] * a[4]
    c = ((x[6] << 1) & M32) + (d3 & M32) >> 32
    r = []
    for k, dw in ((7, d3 >> 32), (8, d4 & M32), (9, d4 >> 32)):
        s = (((x[k] << 1) | (x[k - 1] >> 31)) & M32) + dw + c
        r.append(s & M32)
        c = s >> 32
    return r


def win_exact(lam):
    """words 7..9 of the band, straight from its definition (the model above must agree)"""
    a = limbs(lam)
    w = sum(2 * a[i] * a[j] * B ** (i + j) for i in range(8) for j in range(i + 1, 8) if 6 <= i + j <= 9) + a[3] ** 2 * B ** 6 + a[4] ** 2 * B ** 8
    return [(w >> (32 * k)) & M32 for k in (7, 8, 9)]


def lo64(lam, c1, c2):
    """fe_sqr_add2_lo64 with the addends of fe_lo64_prepare: returns (x, slow, rest, w7')"""
    a = limbs(lam)
    c_lo = ((c1 & M64) + (c2 & M64)) & M64
    c_w7 = (c1 >> 224) + (c2 >> 224)
    w7, w8, w9 = win69(a)
    top64 = (a[7] * a[7] + ((a[6] * a[7]) >> 31)) & M64
    th = top64 >> 32
    rest = th * K977 + top64 + w7 + c_w7
    slow = (rest & M32) >= 0xFFFFF000 or th >= 0xFFFFF000 or w7 >= 0xFFFFFFF8
    if not slow:
        assert rest <= M64                                # the device's 64-bit sum does not wrap
    rest &= M64
    W8 = rest >> 32
    lo = (a[0] * a[0] + c_lo) & M64
    lo = (lo + w8 * K977) & M64
    lo = (lo + W8 * K977) & M64
    lo = (lo + (((w8 + w9 * K977 + W8 + ((a[0] * a[1]) << 1)) & M32) << 32)) & M64
    return lo, slow, rest, w7


def want(lam, c1, c2):
    """what the probe must read: bits 0..63 of the canonical lam^2 + c1 + c2 mod p"""
    return ((lam * lam + c1 + c2) % P) & M64


def true_rest(lam, c1, c2):
    """floor(T / B^7), T = L + K H + c1 + c2 with lam^2 = L + H 2^256: what Rest under-estimates"""
    S = lam * lam
    L, H = S & ((1 << 256) - 1), S >> 256
    return (L + ((1 << 32) + K977) * H + c1 + c2) >> 224


def craft_w7(rnd, target, low_ones=False):
    """a lambda whose w7' is `target`: a7 enters word 7 of the band only through 2 a0 a7 (column 7; its high half is in column 8), so with a0 odd
    w7' = base + 2 a0 a7 mod B reaches every target of base's parity.  low_ones: limbs 0..5 all ones (the largest drop)"""
    while True:
        a = [rnd.randrange(B) for _ in range(8)]
        if low_ones:
            a[:6] = [M32] * 6
        a[0] |= 1
        a[7] = 0
        base = win69(a)[0]
        d = (target - base) % B
        if d & 1:
            continue
        a[7] = ((d >> 1) * pow(a[0], -1, B)) % (B >> 1)
        if rnd.random() < 0.5:
            a[7] += B >> 1
        lam = sum(v << (32 * i) for i, v in enumerate(a))
        assert win69(a)[0] == target
        return lam


def craft_rest_lo(lam, c2, target, rnd):
    """an addend c1 < p with lo32(Rest) = target for (lam, c1, c2): only word 7 of c1 enters Rest"""
    c1 = rnd.randrange(1 << 224) | (rnd.randrange(B - 1) << 192)       # word 6 < 2^32 - 1: c1 < p whatever word 7 is
    _, _, rest, _ = lo64(lam, c1, c2)
    w = (target - rest) % B
    return c1 | (w << 224)


def low_six_ones(rnd):
    """the largest drop: limbs 0..5 all ones"""
    return (rnd.randrange(B * B) << 192) | ((1 << 192) - 1)


def crafted_lambdas(rnd):
    """(label, lambdas) of the crafted classes"""
    return [
        ("low_six_ones", [low_six_ones(rnd) for _ in range(64)] + [(1 << 192) - 1, (1 << 256) - 1]),
        ("w7_near_wrap", [craft_w7(rnd, B - k) for k in range(1, 9) for _ in range(8)]),          # w7' >= 2^32 - 8: always the exact path
        ("w7_below_wrap", [craft_w7(rnd, B - k) for k in (9, 10, 16, 17) for _ in range(8)]),     # just outside the new condition
        ("non_canonical", [(1 << 256) - 1 - k for k in range(16)] + [P + k for k in range(16)] + [rnd.randrange(P, 1 << 256) for _ in range(32)]),
    ]
