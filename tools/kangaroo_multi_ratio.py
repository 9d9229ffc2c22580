#!/usr/bin/env python3
"""The step ratio of kangaroo mode with a key list, on the CPU model (tests/kangaroo_multi_model.py; no GPU): L planted keys in one range solved by ONE
run of solve_multi against the sum of L single-key runs of tests/kangaroo_model.py solve (same range, same number of kangaroos, same dp).
   tools/kangaroo_multi_ratio.py [--keys 16] [--bits 20,22,24] [--seeds 12] [--jobs 8]
prints one line per (width, seed) and the mean ratio with its standard error: the figure DESIGN.md 10 quotes and tests/test_gpu_kangaroo_multi_cli.py
takes its bound from."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bsgs-cuda_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import kangaroo_model as K                  # noqa: E402
import kangaroo_multi_model as M            # noqa: E402
from pybsgs.ecpy import mul                  # noqa: E402


def one(job):
    bits, seed, L, n = job
    W = 1 << bits
    a = (0x5EED << 40) + seed * 977
    rng = K.Stream(1000 * bits + seed)
    ks = []
    while len(ks) < L:
        k = a + 1 + rng.u128() % (W - 1)      # distinct keys, none equal to a
        if k not in ks:
            ks.append(k)
    pubs = [mul(k) for k in ks]
    dp = 0
    while n * (1 << (dp + 1)) <= (W ** 0.5) / 8:
        dp += 1
    keys, multi, _ = M.solve_multi(pubs, a, a + W - 1, seed=seed, n=n, dp=dp)
    assert keys == ks, (bits, seed)
    single = 0
    for i, (k, p) in enumerate(zip(ks, pubs)):
        got, steps = K.solve(p, a, a + W - 1, seed=seed * 100 + i, n=n, dp=dp)
        assert got == k, (bits, seed, i)
        single += steps
    return bits, seed, multi, single


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
    for bits, seed, multi, single in rows:
        ratios.append(multi / single)
        print("width 2^%d seed %2d: %8d steps for the list, %8d for %d single runs, ratio %.3f" % (bits, seed, multi, single, a.keys, ratios[-1]))
    m = sum(ratios) / len(ratios)
    se = (sum((r - m) ** 2 for r in ratios) / (len(ratios) - 1) / len(ratios)) ** 0.5
    print("mean ratio %.4f, standard error %.4f, %d runs" % (m, se, len(ratios)))


if __name__ == "__main__":
    main()
