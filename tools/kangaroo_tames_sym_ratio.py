#!/usr/bin/env python3
"""The step ratio of a search with a tame table of the symmetric walk (-ktamesgen -kwalk sym, -ktamessym) against the search with the plain walk's table
(-ktamesgen / -ktames) on the same keys and herd, on a CPU model.

   tools/kangaroo_tames_sym_ratio.py [--bits 36] [--ktn 16384] [--dp 6] [--kn 512] [--keys 8] [--seeds 24] [--jobs 8] [--jumps 1024]
                                     [--grid]  (the planning grid: E = W / 2^e and m = E / 2^s over a few e and s instead of the defaults)

prints one line per (width, seed) -- steps of both generations and of both searches, keys found, aged kangaroos, cycles -- and the mean ratio symmetric /
plain with its standard error: the figure tests/test_gpu_kangaroo_tames_sym_cli.py takes its bound from.

The model walks on the EXPONENTS, as tools/kangaroo_tames_ratio.py does (its generate and search are the plain table's side here).  For the symmetric walk a
kangaroo is the signed integer e of its representative e*G: a 64-bit hash of |e| stands for x, one more hash bit of |e| for "y is even", so the
representative of the class {e, -e} is a pseudo-random one of the two.  A step adds the jump chosen by x & (R - 1) with the last-index rule, then takes the
representative, d and sigma following it.  The cycle check is per launch of 32 steps with its window of 16.  Planning defaults: tests/kangaroo_tames_sym_model.py
plan; tame starts in [1, ceil(W/2) + E), wild starts at k'' + u with u in [-U, U); merged, dead and aged kangaroos start afresh; the list search's Assigner."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bsgs-cuda_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import kangaroo_model as K                  # noqa: E402
import kangaroo_multi_model as M            # noqa: E402
import kangaroo_tames_sym_model as TS       # noqa: E402
import kangaroo_tames_ratio as PLAIN        # noqa: E402

hash64 = PLAIN.hash64
LAUNCH, WINDOW = 32, 16


def rep(e, salt):
    """the representative of the class {e, -e}: the sign a hash bit of |e| names"""
    a = abs(e)
    return a if hash64(a, salt ^ 0x51ED) & 1 else -a


class Herd:
    """n kangaroos of the symmetric walk on exponents: e (representative), d, sigma (0 tame), last jump index, and the launch's cycle check"""

    def __init__(self, n, s, salt):
        self.n, self.s, self.R, self.salt = n, s, len(s), salt
        self.e, self.d, self.sg, self.last, self.mark = [0] * n, [0] * n, [0] * n, [-1] * n, [None] * n
        self.t = 0

    def put(self, i, e, d, sg):
        self.e[i], self.d[i], self.sg[i], self.last[i], self.mark[i] = e, d, sg, -1, None

    def step(self, i):
        """-> (x, cycle): the hash of the new class, and whether the cycle check retires the kangaroo"""
        e, d, sg = self.e[i], self.d[i], self.sg[i]
        r = rep(e, self.salt)
        if r != e:
            e, d, sg = -e, -d, -sg
        j = hash64(abs(e), self.salt) & (self.R - 1)
        if j == self.last[i]:
            j = (j + 1) & (self.R - 1)
        e, d = e + self.s[j], d + self.s[j]
        if rep(e, self.salt) != e:
            e, d, sg = -e, -d, -sg
        self.e[i], self.d[i], self.sg[i], self.last[i] = e, d, sg, j
        x = hash64(abs(e), self.salt)
        t = self.t % LAUNCH
        if t == LAUNCH - 1 - WINDOW:
            self.mark[i] = x
        elif t > LAUNCH - 1 - WINDOW and self.mark[i] == x:
            return x, True
        if t == LAUNCH - 1:
            self.mark[i] = None
        return x, False


def generate(W, T, dp, n, seed, salt, R, m, E):
    """-> ({hash: d}, scalars, steps, merges, cycles); the table is short of T entries when the host's bound of 50 times the expected steps ended it (the trails
    have saturated the range)"""
    rng = K.Stream(seed)
    span = max(1, int(2 * m) - 1)
    s = [1 + rng.u64() % span for _ in range(R)]
    top = (W + 1) // 2 + E - 1
    h = Herd(n, s, salt)
    for i in range(n):
        t = 1 + rng.u128() % top
        h.put(i, t, t, 0)
    table, steps, merges, cycles, shift = {}, 0, 0, 0, 64 - dp
    while len(table) < T and steps <= 50 * 2 * (T << dp):
        steps += n
        for i in range(n):
            x, cyc = h.step(i)
            again = cyc
            if not cyc and x >> shift == 0 and len(table) < T:
                if x in table:
                    merges += 1
                    again = True
                else:
                    table[x] = h.d[i]
            if again:
                cycles += cyc
                t = 1 + rng.u128() % top
                h.put(i, t, t, 0)
        h.t += 1
    return table, s, steps, merges, cycles


def search(table, s, W, T, dp, n, kpp, seed, salt, U, A):
    """all kangaroos wild, shared over the keys kpp (offsets from the middle of the range) -> (steps, keys found, aged, cycles)"""
    rng = K.Stream(seed ^ 0x5EA5C4)
    L = len(kpp)
    solved = [False] * L
    asg = M.Assigner(L, set(), n)
    h = Herd(n, s, salt)
    age = [0] * n

    def fresh(i):
        u = rng.u128() % (2 * U) - U
        h.put(i, kpp[asg.key[i]] + u, u, 1)
        age[i] = 0

    for i in range(n):
        fresh(i)
    steps = aged = cycles = 0
    shift = 64 - dp
    per = W // (T << dp)
    give_up = 20 * (L * per + n * (per + (1 << dp)))
    while not all(solved) and steps < give_up:
        steps += n
        for i in range(n):
            k = asg.key[i]
            if solved[k]:
                k = asg.reseed(i, solved)
                if k is None:
                    continue
                fresh(i)
            x, cyc = h.step(i)
            age[i] += 1
            if cyc:
                cycles += 1
                fresh(i)
            elif x >> shift == 0 and x in table and any(h.sg[i] * (eps * table[x] - h.d[i]) == kpp[k] for eps in (1, -1)):
                solved[k] = True
            elif age[i] > A:
                aged += 1
                fresh(i)
        h.t += 1
    return steps, sum(solved), aged, cycles


def one(job):
    bits, seed, L, n, T, dp, R, eshift, mshift = job
    W = 1 << bits
    rng = K.Stream(7000 * bits + seed)                                 # the keys of tools/kangaroo_tames_ratio.py for this width and seed
    edge = max(2, W >> 16)
    kp = [1 + rng.u64() % (edge - 1), W - 1 - rng.u64() % (edge - 1)]      # within W / 2^16 of either end
    while len(kp) < L:
        k = 1 + rng.u128() % (W - 1)
        if k not in kp:
            kp.append(k)
    salt = hash64(seed, bits)
    m, E, U, A = TS.plan(W, T, dp, n)
    if eshift is not None:
        E = W >> eshift
        m = max(2, E >> mshift)
        U = max(1, min(1 << 32, E // 4))
    table, s, gen, merges, gcyc = generate(W, T, dp, n, seed, salt, R, m, E)
    if len(table) < T:                                                 # as the host: nothing written, nothing to search with
        steps, found, aged, cyc = 0, -1, 0, 0
    else:
        steps, found, aged, cyc = search(table, s, W, T, dp, n, [k - W // 2 for k in kp], seed, salt, U, A)
    ptable, ps, pgen, _ = PLAIN.generate(W, T, dp, n, seed, salt)
    psteps, pfound, paged = PLAIN.search(ptable, ps, W, T, dp, n, kp, seed, salt)
    return bits, seed, eshift, mshift, gen, merges, gcyc, steps, found, aged, cyc, pgen, psteps, pfound, paged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="36")
    ap.add_argument("--ktn", type=int, default=16384)
    ap.add_argument("--dp", type=int, default=6)
    ap.add_argument("--kn", type=int, default=512)
    ap.add_argument("--keys", type=int, default=8)
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--jumps", type=int, default=1024)
    ap.add_argument("--grid", action="store_true")
    a = ap.parse_args()
    shapes = [(e, s) for e in (3, 4, 5, 6) for s in (6, 10, 14)] if a.grid else [(None, None)]
    jobs = [(int(b), s, a.keys, a.kn, a.ktn, a.dp, a.jumps, e, ms) for b in a.bits.split(",") for e, ms in shapes for s in range(1, a.seeds + 1)]
    with multiprocessing.Pool(a.jobs) as pool:
        rows = pool.map(one, jobs, chunksize=1)
    for bits in sorted({r[0] for r in rows}):
        for e, ms in shapes:
            ratios, missed = [], 0
            for _, seed, _, _, gen, merges, gcyc, steps, found, aged, cyc, pgen, psteps, pfound, paged in [r for r in rows if r[0] == bits and r[2:4] == (e, ms)]:
                if found < 0:
                    print("width 2^%d seed %2d: symmetric generation gave up after %d steps (%d merges, %d cycles): the trails have saturated the range" % (bits, seed, gen, merges, gcyc))
                    missed += a.keys
                    continue
                ratios.append(steps / psteps)
                missed += a.keys - found
                print("width 2^%d seed %2d: symmetric generation %9d steps (%d merges, %d cycles), search %8d steps (%d of %d keys, %d aged, %d cycles); plain table "
                      "generation %9d steps, search %8d steps (%d keys, %d aged); ratio %.3f" % (bits, seed, gen, merges, gcyc, steps, found, a.keys, aged, cyc, pgen, psteps, pfound, paged, ratios[-1]))
            if not ratios:
                print("width 2^%d, -ktn %d -dp %d -kn %d -kjumps %d: no table was made" % (bits, a.ktn, a.dp, a.kn, a.jumps))
                continue
            m = sum(ratios) / len(ratios)
            se = (sum((r - m) ** 2 for r in ratios) / (len(ratios) - 1) / len(ratios)) ** 0.5 if len(ratios) > 1 else 0.0
            what = "defaults" if e is None else "E = W / 2^%d, m = E / 2^%d" % (e, ms)
            print("width 2^%d, -ktn %d -dp %d -kn %d -kjumps %d, %d keys, %s: mean ratio %.4f, standard error %.4f, %d runs, %d keys missed" %
                  (bits, a.ktn, a.dp, a.kn, a.jumps, a.keys, what, m, se, len(ratios), missed))


if __name__ == "__main__":
    main()
