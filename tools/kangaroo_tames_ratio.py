#!/usr/bin/env python3
"""The step ratio of a search with a tame table (-ktamesgen, -ktames) against the plain search of the same key list (-kangaroo -infile), on a CPU model.

   tools/kangaroo_tames_ratio.py [--bits 36] [--ktn 16384] [--dp 6] [--kn 512] [--keys 8] [--seeds 24] [--jobs 8]

prints one line per (width, seed) -- steps of the generation, of the search with the table, of the plain list search, and search / plain -- and the mean
ratio with its standard error: the figures DESIGN.md 10 quotes and tests/test_gpu_kangaroo_tames_cli.py takes its bound from.

The model walks on the EXPONENTS: a kangaroo is the integer p of its point p*G, and a 64-bit hash of p stands for the point's x (jump index = hash & 63,
distinguished = top dp bits of the hash zero).  Step counts of a kangaroo search depend on x only through these two pseudo-random functions of the point,
so the counts are those of the walk on the curve in distribution; a shape of 2^36 keys and 512 kangaroos, 24 seeds, takes a minute this way and days on
tests/kangaroo_model.py's curve arithmetic.  Everything else is the rule as the tests' models state it: the planning defaults (tests/kangaroo_tames_model.py
plan), tame starts in [1, W + E), wild starts at k + u with u in [0, U), re-seeding of merged, dead and aged kangaroos, the list search's Assigner, and for
the plain search tests/kangaroo_multi_model.py's MultiTable itself (its candidates are verified on the curve).  Two of the planted keys lie within
W / 2^16 of either end of the range."""
import argparse
import math
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bsgs-cuda_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import kangaroo_model as K                  # noqa: E402
import kangaroo_multi_model as M            # noqa: E402
import kangaroo_tames_model as TM           # noqa: E402
from pybsgs.ecpy import mul                  # noqa: E402

M64 = (1 << 64) - 1


def hash64(p, salt):
    """stands for the x of the point p*G"""
    v = ((p ^ salt) * 0x9E3779B97F4A7C15) & M64
    v = ((v ^ (v >> 32)) * 0xBF58476D1CE4E5B9) & M64
    v = ((v ^ (v >> 29)) * 0x94D049BB133111EB) & M64
    return v ^ (v >> 32)


def scalars_of(rng, mean):
    span = max(1, int(2 * mean) - 1)
    return [1 + rng.u64() % span for _ in range(64)]


def generate(W, T, dp, n, seed, salt):
    """-> ({hash: d}, scalars, steps, merges)"""
    m, E, _, _ = TM.plan(W, T, dp)
    rng = K.Stream(seed)
    s = scalars_of(rng, m)
    pos = [1 + rng.u128() % (W + E - 1) for _ in range(n)]
    table, steps, merges, shift = {}, 0, 0, 64 - dp
    while len(table) < T:
        steps += n
        for i in range(n):
            p = pos[i] + s[hash64(pos[i], salt) & 63]
            x = hash64(p, salt)
            if x >> shift == 0 and len(table) < T:
                if x in table:
                    merges += 1
                    p = 1 + rng.u128() % (W + E - 1)
                else:
                    table[x] = p
            pos[i] = p
    return table, s, steps, merges


def search(table, s, W, T, dp, n, kp, seed, salt):
    """all kangaroos wild, shared over the keys kp (offsets from the start of the range) -> (steps, keys found, re-seeds of aged kangaroos)"""
    _, _, U, A = TM.plan(W, T, dp)
    rng = K.Stream(seed ^ 0x5EA5C4)
    L = len(kp)
    solved = [False] * L
    asg = M.Assigner(L, set(), n)
    d = [rng.u128() % U for _ in range(n)]
    age = [0] * n
    steps = aged = 0
    shift = 64 - dp
    give_up = 20 * (L * (W // (T << dp)) + n * (W // (T << dp) + (1 << dp)))      # the host's bound: every kangaroo may have to cross a gap between trails first
    while not all(solved) and steps < give_up:
        steps += n
        for i in range(n):
            k = asg.key[i]
            if solved[k]:
                k = asg.reseed(i, solved)
                if k is None:
                    continue
                d[i], age[i] = rng.u128() % U, 0
            p = kp[k] + d[i]
            dn = d[i] + s[hash64(p, salt) & 63]
            d[i] = dn
            age[i] += 1
            x = hash64(kp[k] + dn, salt)
            if x >> shift == 0 and x in table and table[x] - dn == kp[k]:
                solved[k] = True
            elif age[i] > A:
                aged += 1
                d[i], age[i] = rng.u128() % U, 0
    return steps, sum(solved), aged


def plain(a, W, kp, pubs, n, seed, salt):
    """the list search as tests/kangaroo_multi_model.py solve_multi runs it (half the herd tame, wild kangaroos shared out by the Assigner), at the dp the
    host chooses for this width -> (steps, keys found)"""
    L = len(kp)
    sq = W ** 0.5
    dp = max(0, min(32, math.ceil(math.log2(2.0 * sq / 33554432.0))))      # the host's default (plan_herd): the expected DPs within 2^25 host entries
    rng = K.Stream(seed)
    s = scalars_of(rng, max(1.0, n * sq / 4))
    table = M.MultiTable(a, W, pubs)
    asg = M.Assigner(L, set(), n - n // 2)
    pos, d, fl = [0] * n, [0] * n, [0] * n
    shift = 64 - dp

    def solved_list():
        return [k is not None for k in table.keys]

    def fresh(i):
        wild = i >= n // 2
        key = asg.reseed(i - n // 2, solved_list()) if wild else 0
        if wild and key is None:
            fl[i] = K.DEAD
            return
        d[i] = K.herd_offset(rng, W, wild)
        pos[i] = kp[key] + d[i] if wild else d[i]
        fl[i] = M.wild_flags(key) if wild else 0

    for i in range(n):
        fresh(i)
    steps = 0
    limit = int(40 * L * (2 * sq + n * (1 << dp)))
    while table.solved() < L and steps < limit:
        steps += n
        for i in range(n):
            if fl[i] & K.DEAD:
                continue
            j = hash64(pos[i], salt) & 63
            pos[i] += s[j]
            d[i] += s[j]
            x = hash64(pos[i], salt)
            if dp == 0 or x >> shift == 0:
                for e in table.add(x, d[i] & K.M128, i, fl[i]):
                    if e[0] == "reseed":
                        fresh(e[1])
                    elif e[0] == "found":
                        for w, kk in enumerate(asg.key):
                            if kk == e[1]:
                                fresh(n // 2 + w)
    return steps, table.solved()


def one(job):
    bits, seed, L, n, T, dp = job
    W = 1 << bits
    a = 1 << (bits - 1)
    rng = K.Stream(7000 * bits + seed)
    edge = max(2, W >> 16)
    kp = [1 + rng.u64() % (edge - 1), W - 1 - rng.u64() % (edge - 1)]      # within W / 2^16 of either end
    while len(kp) < L:
        k = 1 + rng.u128() % (W - 1)
        if k not in kp:
            kp.append(k)
    salt = hash64(seed, bits)
    table, s, gen_steps, merges = generate(W, T, dp, n, seed, salt)
    tames_steps, found, aged = search(table, s, W, T, dp, n, kp, seed, salt)
    pubs = [mul(a + k) for k in kp]
    plain_steps, plain_found = plain(a, W, kp, pubs, n, seed, salt)
    return bits, seed, gen_steps, merges, tames_steps, found, aged, plain_steps, plain_found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="36")
    ap.add_argument("--ktn", type=int, default=16384)
    ap.add_argument("--dp", type=int, default=6)
    ap.add_argument("--kn", type=int, default=512)
    ap.add_argument("--keys", type=int, default=8)
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    jobs = [(int(b), s, a.keys, a.kn, a.ktn, a.dp) for b in a.bits.split(",") for s in range(1, a.seeds + 1)]
    with multiprocessing.Pool(a.jobs) as pool:
        rows = pool.map(one, jobs, chunksize=1)
    for bits in sorted({r[0] for r in rows}):
        ratios = []
        for _, seed, gen_steps, merges, tames_steps, found, aged, plain_steps, plain_found in [r for r in rows if r[0] == bits]:
            ratios.append(tames_steps / plain_steps)
            print("width 2^%d seed %2d: generation %9d steps (%d merges), search %8d steps (%d of %d keys, %d aged), plain list search %9d steps (%d keys), ratio %.3f" %
                  (bits, seed, gen_steps, merges, tames_steps, found, a.keys, aged, plain_steps, plain_found, ratios[-1]))
        m = sum(ratios) / len(ratios)
        se = (sum((r - m) ** 2 for r in ratios) / (len(ratios) - 1) / len(ratios)) ** 0.5 if len(ratios) > 1 else 0.0
        print("width 2^%d, -ktn %d -dp %d -kn %d, %d keys: mean ratio %.4f, standard error %.4f, %d runs" % (bits, a.ktn, a.dp, a.kn, a.keys, m, se, len(ratios)))


if __name__ == "__main__":
    main()
