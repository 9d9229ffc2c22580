#!/usr/bin/env python3
"""The step ratio of the symmetric list search against the plain list search, on the CPU models (tests/kangaroo_symlist_model.py solve_symlist against
tests/kangaroo_multi_model.py solve_multi; no GPU): L planted keys in one range, the same keys, number of kangaroos and dp in both.
   tools/kangaroo_symlist_ratio.py [--keys 16] [--bits 20,22,24] [--seeds 12] [--jobs 8]
prints one line per (width, seed) and the mean ratio with its standard error: the figure DESIGN.md 10 quotes and tests/test_gpu_kangaroo_symlist_cli.py
takes its bound from.  The grid is that of tools/kangaroo_multi_ratio.py."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bsgs-cuda_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import kangaroo_model as K                  # noqa: E402
import kangaroo_multi_model as M            # noqa: E402
import kangaroo_symlist_model as SL         # noqa: E402
from pybsgs.ecpy import mul                  # noqa: E402


def one(job):
    bits, seed, L, n = job
    W = 1 << bits
    a = (0x5EED << 40) + seed * 977
    rng = K.Stream(1000 * bits + seed)
    ks = []
    while len(ks) < L:
        k = a + 1 + rng.u128() % (W - 1)      # distinct keys, none equal to a (kangaroo_multi_ratio.py's draw)
        if k not in ks:
            ks.append(k)
    pubs = [mul(k) for k in ks]
    dp = 0
    while n * (1 << (dp + 1)) <= (W ** 0.5) / 8:
        dp += 1
    keys, plain, _ = M.solve_multi(pubs, a, a + W - 1, seed=seed, n=n, dp=dp)
    assert keys == ks, (bits, seed)
    keys, sym, _ = SL.solve_symlist(pubs, a, a + W - 1, seed=seed, n=n, dp=dp)
    assert keys == ks, (bits, seed)
    return bits, seed, sym, plain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--bits", default="20,22,24")
    ap.add_argument("--seeds", type=int, default=12)
    ap.add_argument("--kangaroos", type=int, default=16)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    jobs = [(int(b), s, a.keys, a.kangaroos) for b in a.bits.split(",") for s in range(1, a.seeds + 1)]
    with multiprocessing.Pool(a.jobs) as pool:
        rows = pool.map(one, jobs)
    ratios = []
    for bits, seed, sym, plain in rows:
        ratios.append(sym / plain)
        print("width 2^%d seed %2d: %8d steps with the symmetric walk, %8d with the plain walk, ratio %.3f" % (bits, seed, sym, plain, ratios[-1]))
    m = sum(ratios) / len(ratios)
    se = (sum((r - m) ** 2 for r in ratios) / (len(ratios) - 1) / len(ratios)) ** 0.5
    print("mean ratio %.4f, standard error %.4f, %d runs" % (m, se, len(ratios)))


if __name__ == "__main__":
    main()
