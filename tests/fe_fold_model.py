"""Python-int model of fe_sqr_add2 (csrc/fp256.hip.h): the 512-bit square, then fe_reduce512_t<true> of the default build word for word -- the three
8-word carry chains with their count `top`, the eight multiply-add columns, the join, the 33-bit overflow word W8 = l + h 2^32, fold 2 and the rarely
taken fold 3 -- with the events a case takes, and the case generator the CPU and GPU tests share.  TEST INFRASTRUCTURE: no product code is called.

    a^2 = L + H 2^256,   T = L + 977 H + (H << 32) + c1 + c2 = t + W8 2^256,   r = t + W8 (2^32 + 977)  (fold 2),   r -= p once more on a carry (fold 3)
"""
import random

B = 1 << 32
M32 = B - 1
P = (1 << 256) - (1 << 32) - 977
K977 = 977
KP = B + K977                                             # 2^256 - p

# every event of the ADD2 path: the carry count of the three chains, the 33-bit word 8 before the join, both values of the high bit of W8, fold 3 and the
# ripple into word 2 inside it
EVENTS = ("top0", "top1", "top2", "top3", "w15_33bit", "h0", "h1", "fold3", "fold3_ripple")


def limbs(x, n=8):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def value(words):
    return sum(v << (32 * i) for i, v in enumerate(words))


def addc(a, b, c):
    s = a + b + c
    return s & M32, s >> 32


def reduce512_add2(w, c1, c2):
    """fe_reduce512_t<true>(r, w, c1, c2): w = 16 words, c1 and c2 = 8 words each -> (8 result words, set of events)"""
    ev = set()
    # L + (H << 32): word k of the shifted copy is w[7 + k]; w[15] moves to word 8
    s = [w[0]] + [0] * 7
    cb = 0
    for k in range(1, 8):
        s[k], cb = addc(w[k], w[7 + k], cb)
    top = cb
    for c in (c1, c2):
        cb = 0
        for k in range(8):
            s[k], cb = addc(s[k], c[k], cb)
        top += cb
    ev.add("top%d" % top)
    A = [w[8 + k] * K977 + s[k] for k in range(8)]
    assert all(v < 1 << 64 for v in A)
    w15 = w[15] + top                                     # word 8 before the join: < 2^32 + 3
    if w15 >> 32:
        ev.add("w15_33bit")
    # the join: lo(A[k]) + hi(A[k - 1])
    t = [A[0] & M32] + [0] * 7
    c = 0
    for k in range(1, 8):
        t[k], c = addc(A[k] & M32, A[k - 1] >> 32, c)
    l, co = addc(w15 & M32, A[7] >> 32, c)
    h = co + (w15 >> 32)
    assert h in (0, 1)                                    # W8 = l + h 2^32 <= 2^32 + 2^11
    ev.add("h%d" % h)
    # fold 2: W8 K = l 977 + (l + h 977) 2^32 + h 2^64
    B0 = l * K977 + t[0]
    B1 = h * K977 + t[1] + l
    assert B0 < 1 << 64 and B1 < 1 << 64
    r = [0] * 8
    r[0] = B0 & M32
    r[1], c = addc(B1 & M32, B0 >> 32, 0)
    assert (B1 >> 32) + h <= M32
    r[2], c = addc(t[2], (B1 >> 32) + h, c)
    for k in range(3, 8):
        r[k], c = addc(t[k], 0, c)
    if c:                                                 # fold 3: a carry out of 2^256 leaves a value < 2^67; wrap it once more
        ev.add("fold3")
        assert r[2] < 8 and not any(r[3:])
        x = r[0] + K977
        r[0] = x & M32
        x = (x >> 32) + r[1] + 1
        r[1] = x & M32
        if x >> 32:
            ev.add("fold3_ripple")
        r[2] = (r[2] + (x >> 32)) & M32
    return r, ev


def sqr_add2(a, c1, c2):
    """fe_sqr_add2(r, a, c1, c2) for any a, c1, c2 below 2^256 -> (r, events)"""
    r, ev = reduce512_add2(limbs(a * a, 16), limbs(c1), limbs(c2))
    return value(r), ev


SPECIALS = [0, 1, P - 1, P, P + 1, (1 << 256) - 1, (1 << 256) - (1 << 32), int("ffffffff00000000" * 4, 16), int("00000000ffffffff" * 4, 16),
            (1 << 256) - KP - 1, (1 << 224) - 1, (1 << 256) - (1 << 224)]


def aimed_addends(a, r_target):
    """c1, c2 below 2^256 that make fold 2 of fe_sqr_add2(a, c1, c2) end on 2^256 + r_target (fold 3 then leaves r_target + K), or None when no pair does:
    T = L + K H + c1 + c2 must be t + W8 2^256 with t + W8 K = 2^256 + r_target"""
    L, H = (a * a) & ((1 << 256) - 1), (a * a) >> 256
    t0 = L + KP * H
    for w8 in range(t0 >> 256, (t0 >> 256) + 3):
        t = (1 << 256) + r_target - w8 * KP
        need = (w8 << 256) + t - t0
        if 0 <= t < 1 << 256 and 0 <= need <= 2 * ((1 << 256) - 1):
            c1 = min(need, (1 << 256) - 1)
            return c1, need - c1
    return None


def cases(seed=1, randoms=2000):
    """-> (list of (a, c1, c2), dict event -> number of cases that take it).  The special operands cubed, `randoms` random triples over the full range, and
    for every special a the addends aimed at the ripple inside fold 3 (word 1 all ones after fold 2: one case in 2^32 of those that reach fold 3 at all)."""
    out = [(a, c1, c2) for a in SPECIALS for c1 in SPECIALS for c2 in SPECIALS]
    rnd = random.Random(seed)
    out += [(rnd.randrange(1 << 256), rnd.randrange(1 << 256), rnd.randrange(1 << 256)) for _ in range(randoms)]
    for a in SPECIALS + [rnd.randrange(1 << 255, 1 << 256) for _ in range(8)]:
        for r_target in ((1 << 64) - 1, (1 << 64) - B, (1 << 64) - K977, (1 << 64) - K977 - 1, (0xFFFFFFFF << 32) | rnd.randrange(B), 0, B - K977):
            c = aimed_addends(a, r_target)
            if c:
                out.append((a, c[0], c[1]))
    counts = dict.fromkeys(EVENTS, 0)
    for a, c1, c2 in out:
        for e in sqr_add2(a, c1, c2)[1]:
            counts[e] += 1
    return out, counts
