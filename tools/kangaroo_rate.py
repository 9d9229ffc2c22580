#!/usr/bin/env python3
"""Kangaroo walk rate on one GPU: a full herd (16 kangaroos per thread, four waves per SIMD on every CU) at seeded starts, warm-up launches, then timed
launches between device synchronisations.  Prints one JSON line: steps/s, ms per launch, bytes per step from the layout, the kernel's VGPR count.

    tools/kangaroo_rate.py [--steps 256] [--launches 8] [--warmup 2] [--dp 16] [--per-thread 16] [--sym [--jumps 1024] [--keys]] [--tames N] [--tamesgen N] [--dptable N [--keys]] [--dpshard E] [--no-vgprs] [--out FILE]
    tools/kangaroo_rate.py --tamesload N | --tamessort N [--reps 3] [--out FILE]

--sym times the symmetric walk (bsgs_kangaroo_setup_sym: the negation map, its jump table in device memory, the cycle check of every launch); with --keys
the herd of bsgs_kangaroo_setup_sym_keys, whose kernel entry point reads a kangaroo's key when it writes a record (keys 0..15 dealt out over the herd).

--tames N installs a tame table of N entries (bsgs_kangaroo_tames_install; tags that no record meets, so every lookup ends in a miss, as all but a handful
do in a search) and times bsgs_kangaroo_run_tames and bsgs_kangaroo_run in turn, launch by launch: the difference of their kernel times is the match.
With --sym --keys the table is that of the keyed herd (bsgs_kangaroo_tames_install_keys, bsgs_kangaroo_run_tames_keys: the search of -ktamessym).

--tamesgen N begins a growing tame table of capacity N (bsgs_kangaroo_tames_gen_begin) under an all-tame herd of pairwise different starts (seeded on the
GPU: repeated starts would make every record a duplicate) and times bsgs_kangaroo_run_tames_gen and bsgs_kangaroo_run in turn, launch by launch, in one
process: the difference of their kernel times is the insert.  Plain walk, or with --sym the symmetric one (the generators of -ktamesgen -ktamesdev).

--dptable N begins a distinguished-point table of capacity N in device memory (bsgs_kangaroo_dptable_begin) under a herd of pairwise different starts, half
tame and half wild (seeded on the GPU), and times bsgs_kangaroo_run_dptable and bsgs_kangaroo_run in turn, launch by launch, in one process: the difference
of their kernel times is insert + resolve.  Plain walk, or with --sym the symmetric one: the search of -kdpdev.  Choose --steps and --dp so that a launch
writes at most 2^22 records (a full herd at --dp 7: --steps 64).  With --keys the table is the one for a key list (bsgs_kangaroo_dptable_begin_keys,
bsgs_kangaroo_run_dptable_keys: the search of -infile -kdpkeys) under a herd that serves 16 keys -- that of bsgs_kangaroo_setup with a key list, or with
--sym that of bsgs_kangaroo_setup_sym_keys -- seeded by bsgs_kangaroo_seed_keys, the wild half dealt out over the keys: the walk alone and walk + keyed
insert + resolve, alternating in one process.

--dpshard E (plain walk or --sym) opens TWO engines on the one GPU, each with a full herd of the same starts and a table of 2^27 entries: one begun by
bsgs_kangaroo_dptable_begin, one by bsgs_kangaroo_dptable_begin_shard as shard 0 of E.  Launch by launch, in one process, it times bsgs_kangaroo_run_dptable
(the --dptable leg) against bsgs_kangaroo_run_dptable_shard, which routes (E - 1) / E of its records out, followed by what an engine of a sharded search does
with its inbox: bsgs_kangaroo_dptable_insert_shard of as many records as were routed, the routed ones themselves with their shard bits rewritten to this
shard's (wall time: upload, insert, resolve).  Reports ms per launch of each and the bytes relayed.

--tamesload N times bsgs_kangaroo_tames_gen_load of N synthetic entries (pairwise different tags, 24 bytes each from pageable host memory) into a fresh growing
table of capacity N, --reps times.  --tamessort N loads such a table once and times bsgs_kangaroo_tames_gen_read_sorted of all N entries (harvest, radix sort,
gather and the copy to the host) against bsgs_kangaroo_tames_gen_read (harvest and copy, unsorted), in turn.  Both run under the smallest herd; no walk.

The starts are 65536 distinct points P0 + i*G, repeated over the herd (the walk's cost does not depend on which point a kangaroo stands on; repeats only
make their DPs coincide)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bsgs-cuda_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pybsgs                                     # noqa: E402
from pybsgs.ecpy import G, add, mul, splitmix64   # noqa: E402

# bytes of HBM traffic per kangaroo step (csrc/kangaroo.hip): pass 1 reads x (32) and flags (4) and writes the running product (32); pass 2 reads x, flags, the
# previous running product, y and d (32 + 4 + 32 + 32 + 16) and writes x, y, d (80).  DP records (64 bytes each, 2^-dp of the steps) come on top.
BYTES_PER_STEP = 32 + 4 + 32 + (32 + 4 + 32 + 32 + 16) + 80
# the symmetric walk writes the flags back every step (4) and, per launch of S steps, writes the mark once and reads it 16 times (32 * 17 / S, added in main);
# its jump points (72 bytes per step and pass) come from the 72 KiB table, which stays in L2
BYTES_PER_STEP_SYM = BYTES_PER_STEP + 4


def vgprs(sym=False, keys=False):
    try:
        import spill_report
        for r in spill_report.report(tus=["kangaroo"]):
            if ("kangaroo_sym_keys_kernel<true>" if keys else "kangaroo_sym_kernel<true>" if sym else "kangaroo_kernel<true>") in r["kernel"]:
                return r["vgprs"]
    except (SystemExit, Exception):
        return None


def table_legs(a):
    """--tamesload / --tamessort: the load into and the sorted read of a growing tame table, without a walk"""
    import numpy as np
    n = a.tamesload or a.tamessort
    dev = pybsgs.Device(0)
    L = dev.L
    scal = [(0x9E3779B97F4A7C15 * (j + 1)) % (1 << 62) + 1 for j in range(64)]
    dev.kangaroo_setup([mul(s) for s in scal], scal, 16, 64, 1, 64)
    tags = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)      # an odd multiplier: pairwise different, none zero
    d = np.empty((n, 2), dtype=np.uint64)
    d[:, 0] = tags ^ np.uint64(0x5555555555555555)
    d[:, 1] = np.arange(n, dtype=np.uint64)
    counts = [C.c_uint64() for _ in range(5)]
    u64p = C.POINTER(C.c_uint64)

    def load():
        t0 = time.perf_counter()
        pybsgs._chk(L.bsgs_kangaroo_tames_gen_load(dev.h, tags.ctypes.data, d.ctypes.data, n, *[C.byref(c) for c in counts]))
        s = time.perf_counter() - t0
        assert [c.value for c in counts] == [n, 0, 0, 0, n], [c.value for c in counts]
        return s

    res = {"gpu": dev.name(), "entries": n, "slots": 1 << max(7, (2 * (n + 64) - 1).bit_length()), "bytes_per_entry": 24}
    if a.tamesload:
        begin, secs = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pybsgs._chk(L.bsgs_kangaroo_tames_gen_begin(dev.h, n))
            begin.append(time.perf_counter() - t0)
            secs.append(load())
        res.update({"what": "load of synthetic entries into a growing tame table (bsgs_kangaroo_tames_gen_load), pageable host memory", "begin_s_each": begin, "load_s_each": secs,
                    "load_s": min(secs), "entries_per_s": n / min(secs), "host_GBps": 24 * n / min(secs) / 1e9})
    else:
        pybsgs._chk(L.bsgs_kangaroo_tames_gen_begin(dev.h, n))
        load()
        xs, ds, cnt = np.empty(n, dtype=np.uint64), np.empty((n, 2), dtype=np.uint64), C.c_uint64()
        srt, plain = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pybsgs._chk(L.bsgs_kangaroo_tames_gen_read(dev.h, xs.ctypes.data_as(u64p), ds.ctypes.data, n, C.byref(cnt)))
            plain.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            pybsgs._chk(L.bsgs_kangaroo_tames_gen_read_sorted(dev.h, xs.ctypes.data, ds.ctypes.data, n, C.byref(cnt)))
            srt.append(time.perf_counter() - t0)
        assert cnt.value == n and bool(np.all(xs[1:] > xs[:-1])) and bool(np.all(ds[:, 0] == xs ^ np.uint64(0x5555555555555555)))
        t0 = time.perf_counter()
        np.argsort(xs[::-1].copy(), kind="stable")                    # one host thread sorting the tags alone, for scale
        host_sort = time.perf_counter() - t0
        res.update({"what": "sorted read of a growing tame table (bsgs_kangaroo_tames_gen_read_sorted: harvest, radix sort on the device, gather, copy) against the unsorted read",
                    "read_sorted_s_each": srt, "read_unsorted_s_each": plain, "read_sorted_s": min(srt), "read_unsorted_s": min(plain), "sort_on_device_s": min(srt) - min(plain),
                    "entries_per_s": n / min(srt), "numpy_argsort_of_the_tags_s": host_sort, "checked": "ascending, each d with its tag"})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    dev.close()


def shard_legs(a):
    """--dpshard E: the unsharded and the sharded table under the same walk, on two engines of one GPU, alternating"""
    import numpy as np
    REC = np.dtype([("x", "<u8", (4,)), ("d", "<u8", (2,)), ("kangaroo", "<u4"), ("flags", "<u4"), ("step", "<u4"), ("reserved", "<u4")])
    E, cap, capacity = a.dpshard, 1 << 22, 1 << 27
    devs = [pybsgs.Device(0), pybsgs.Device(0)]
    L = devs[0].L
    cus = C.c_int()
    pybsgs._chk(L.bsgs_dev_cu_count(devs[0].h, C.byref(cus)))
    n = cus.value * 1024 * a.per_thread
    scal = [splitmix64(j)[1] % (1 << 62) + 1 for j in range(a.jumps if a.sym else 64)]
    jumps = [mul(s) for s in scal]
    d = np.random.RandomState(7).randint(1, 1 << 62, size=(n, 2), dtype=np.uint64)
    d[:, 1] &= np.uint64((1 << 36) - 1)                              # offsets below 2^100, pairwise different but for a 2^-62 chance
    flags = (C.c_uint32 * n)(*([0] * (n // 2) + [pybsgs.KANGAROO_WILD] * (n - n // 2)))
    q = mul(0xD15C0 << 70)
    begin_s = []
    for k, dev in enumerate(devs):
        (dev.kangaroo_setup_sym if a.sym else dev.kangaroo_setup)(jumps, scal, a.dp, n, a.per_thread, cap)
        pybsgs._chk(L.bsgs_kangaroo_seed(dev.h, pybsgs.le32(q[0]) + pybsgs.le32(q[1]), None, 0, n, d.tobytes(), flags, None, None))
        t0 = time.perf_counter()
        if k == 0:
            dev.kangaroo_dptable_begin(capacity)
        else:
            dev.kangaroo_dptable_begin_shard(capacity, 0, E, 0)
        begin_s.append(time.perf_counter() - t0)
    recs, routed = (pybsgs.KangarooRecord * (2 * cap))(), np.zeros(cap, REC)
    back = (pybsgs.KangarooRecord * (2 * cap))()
    cnt, seen, n_entries, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
    counts = (C.c_uint32 * 16)()
    rp = routed.ctypes.data_as(C.POINTER(pybsgs.KangarooRecord))

    def launch_one():
        pybsgs._chk(L.bsgs_kangaroo_run_dptable(devs[0].h, a.steps, recs, 2 * cap, C.byref(cnt), C.byref(seen), C.byref(n_entries), C.byref(dropped), C.byref(ms)))
        return ms.value, seen.value, dropped.value

    def launch_shard():
        pybsgs._chk(L.bsgs_kangaroo_run_dptable_shard(devs[1].h, a.steps, recs, 2 * cap, C.byref(cnt), rp, cap, counts, C.byref(seen), C.byref(n_entries), C.byref(dropped),
                                                      C.byref(ms)))
        kernel, total, dr, m = ms.value, seen.value, dropped.value, sum(counts)
        # the inbox of a sharded search: as many records as went out, bound for this shard.  The routed records with their shard bits divided by E name shard 0
        routed["x"][:m, 0] = (routed["x"][:m, 0] & np.uint64((1 << 48) - 1)) | ((routed["x"][:m, 0] >> np.uint64(48)) // np.uint64(E) << np.uint64(48))
        t0 = time.perf_counter()
        pybsgs._chk(L.bsgs_kangaroo_dptable_insert_shard(devs[1].h, rp, m, back, 2 * cap, C.byref(cnt), None, 0, counts, C.byref(n_entries), C.byref(dropped)))
        inbox = (time.perf_counter() - t0) * 1e3
        assert sum(counts) == 0, "an inbox record was routed again"
        return kernel, inbox, total, m, dr + dropped.value

    for _ in range(a.warmup):
        launch_one()
        launch_shard()
    one, shard, inbox, nrec, nrouted, dr = [], [], [], 0, 0, 0
    for _ in range(a.launches):
        k, r, x = launch_one()
        one.append(k)
        dr += x
        k, i, r, m, x = launch_shard()
        shard.append(k)
        inbox.append(i)
        nrec += r
        nrouted += m
        dr += x
    mean = lambda v: sum(v) / len(v)
    res = {"what": "kangaroo walk with the distinguished-point table in device memory: one table against shard 0 of %d with its inbox, two engines on one GPU, full herds, half tame "
                   "half wild" % E + (", symmetric walk" if a.sym else ""),
           "gpu": devs[0].name(), "shards": E, "kangaroos": n, "per_thread": a.per_thread, "steps_per_launch": a.steps, "dp": a.dp, "launches": a.launches, "capacity": capacity,
           "begin_s": begin_s, "ms_per_launch_walk_insert_resolve": mean(one), "ms_per_launch_walk_shard_insert_scatter_resolve": mean(shard), "ms_inbox_insert_wall": mean(inbox),
           "ms_shard_minus_one": mean(shard) - mean(one), "ms_one_each": one, "ms_shard_each": shard, "ms_inbox_each": inbox,
           "records_per_launch": nrec / a.launches, "records_routed_per_launch": nrouted / a.launches, "routed_share": nrouted / max(1, nrec),
           "bytes_relayed_per_launch": 2 * 64 * nrouted / a.launches, "dropped": dr,
           "steps_per_s_kernel_one": n * a.steps / (mean(one) / 1e3), "steps_per_s_shard_with_inbox": n * a.steps / ((mean(shard) + mean(inbox)) / 1e3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for dev in devs:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dp", type=int, default=16)
    ap.add_argument("--per-thread", type=int, default=16)
    ap.add_argument("--sym", action="store_true")
    ap.add_argument("--jumps", type=int, default=1024)
    ap.add_argument("--keys", action="store_true")
    ap.add_argument("--tames", type=int, default=0)
    ap.add_argument("--tamesgen", type=int, default=0)
    ap.add_argument("--dptable", type=int, default=0)
    ap.add_argument("--dpshard", type=int, default=0)
    ap.add_argument("--tamesload", type=int, default=0)
    ap.add_argument("--tamessort", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-vgprs", action="store_true", help="do not compile the walk's unit for its VGPR count")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.keys and not a.sym and not a.dptable:
        ap.error("--keys goes with --sym, or with --dptable")
    if a.tamesgen and (a.keys or a.tames):
        ap.error("--tamesgen goes with the plain walk or --sym alone")
    if a.dptable and (a.tames or a.tamesgen):
        ap.error("--dptable goes with the plain walk or --sym, alone or with --keys")
    if a.dpshard and (a.keys or a.tames or a.tamesgen or a.dptable or not 1 <= a.dpshard <= pybsgs.KANGAROO_DPT_MAX_SHARDS):
        ap.error("--dpshard 1..16 goes with the plain walk or --sym alone")
    if a.tamesload or a.tamessort:
        return table_legs(a)
    if a.dpshard:
        return shard_legs(a)
    dev = pybsgs.Device(0)
    L = dev.L
    cus = C.c_int()
    pybsgs._chk(L.bsgs_dev_cu_count(dev.h, C.byref(cus)))
    n = cus.value * 1024 * a.per_thread
    scal = [(0x9E3779B97F4A7C15 * (j + 1)) % (1 << 62) + 1 for j in range(64)]
    if a.sym:
        # scalars without additive structure: multiples of one constant satisfy s_a + s_b = s_c + s_d all over and would fill the walk with fruitless cycles
        scal = [splitmix64(j)[1] % (1 << 62) + 1 for j in range(a.jumps)]
        (dev.kangaroo_setup_sym_keys if a.keys else dev.kangaroo_setup_sym)([mul(s) for s in scal], scal, a.dp, n, a.per_thread, 1 << 22)      # (--keys: the list's herd)
    else:
        dev.kangaroo_setup([mul(s) for s in scal], scal, a.dp, n, a.per_thread, 1 << 22)
    distinct = 65536
    p = mul(0xC0FFEE << 60)
    one = []
    for i in range(distinct):
        one.append(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little") + (i & 0xFFFFFFFF).to_bytes(16, "little") + (i & 1).to_bytes(4, "little") +
                   ((i >> 1) & 15 if a.keys and i & 1 else 0).to_bytes(4, "little") + bytes(8))
        p = add(p, G)
    blob = b"".join(one) * (n // distinct)
    arr = (pybsgs.KangarooState * n).from_buffer_copy(blob)
    pybsgs._chk(L.bsgs_kangaroo_upload(dev.h, 0, n, arr))
    recs = (pybsgs.KangarooRecord * (1 << 22))()
    cnt, dropped, ms = C.c_uint32(), C.c_uint64(), C.c_float()

    def launch():
        pybsgs._chk(L.bsgs_kangaroo_run(dev.h, a.steps, recs, 1 << 22, C.byref(cnt), C.byref(dropped), C.byref(ms)))
        return ms.value, cnt.value + dropped.value

    if a.tamesgen:
        import numpy as np
        d = np.random.RandomState(7).randint(1, 1 << 62, size=(n, 2), dtype=np.uint64)
        d[:, 1] &= np.uint64((1 << 36) - 1)                          # tame offsets below 2^100, pairwise different but for a 2^-62 chance
        flags = (C.c_uint32 * n)()
        pybsgs._chk(L.bsgs_kangaroo_seed(dev.h, None, None, 0, n, d.tobytes(), flags, None, None))
        t0 = time.perf_counter()
        pybsgs._chk(L.bsgs_kangaroo_tames_gen_begin(dev.h, a.tamesgen))
        begin_s = time.perf_counter() - t0
        seen, n_entries = C.c_uint64(), C.c_uint64()

        def launch_gen():
            pybsgs._chk(L.bsgs_kangaroo_run_tames_gen(dev.h, a.steps, recs, 1 << 22, C.byref(cnt), C.byref(seen), C.byref(n_entries), C.byref(dropped), C.byref(ms)))
            return ms.value, seen.value, cnt.value

        for _ in range(a.warmup):
            launch()
            launch_gen()
        plain, both, nrec, back, dr = [], [], 0, 0, 0
        for _ in range(a.launches):
            plain.append(launch()[0])
            k, r, m = launch_gen()
            both.append(k)
            nrec += r
            back += m
            dr += dropped.value
        ins = (sum(both) - sum(plain)) / len(both)
        res = {"what": "kangaroo walk with the tame table grown on the device, one engine, full herd, all tame" + (", symmetric walk" if a.sym else ""), "gpu": dev.name(), "kangaroos": n,
               "per_thread": a.per_thread, "steps_per_launch": a.steps, "dp": a.dp, "launches": a.launches, "capacity": a.tamesgen, "begin_s": begin_s,
               "ms_per_launch_walk": sum(plain) / len(plain), "ms_per_launch_walk_and_insert": sum(both) / len(both), "ms_insert": ins, "insert_share": ins / (sum(both) / len(both)),
               "ms_walk_each": plain, "ms_walk_and_insert_each": both,
               "records_per_launch": nrec / a.launches, "records_handed_back_per_launch": back / a.launches, "dropped": dr, "entries": n_entries.value,
               "steps_per_s_kernel_walk": n * a.steps / (sum(plain) / len(plain) / 1e3), "steps_per_s_kernel_walk_and_insert": n * a.steps / (sum(both) / len(both) / 1e3)}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        dev.close()
        return

    if a.dptable:
        import numpy as np
        d = np.random.RandomState(7).randint(1, 1 << 62, size=(n, 2), dtype=np.uint64)
        d[:, 1] &= np.uint64((1 << 36) - 1)                          # offsets below 2^100, pairwise different but for a 2^-62 chance
        flags = (C.c_uint32 * n)(*([0] * (n // 2) + [pybsgs.KANGAROO_WILD] * (n - n // 2)))
        q = mul(0xD15C0 << 70)
        if a.keys:                                                    # sixteen keys, the wild half dealt out over them
            dev.kangaroo_set_keys([add(q, mul(k + 1)) for k in range(16)])
            key = (C.c_uint32 * n)(*([0] * (n // 2) + [k & 15 for k in range(n - n // 2)]))
            pybsgs._chk(L.bsgs_kangaroo_seed_keys(dev.h, None, 0, n, d.tobytes(), flags, key, None, None))
        else:
            pybsgs._chk(L.bsgs_kangaroo_seed(dev.h, pybsgs.le32(q[0]) + pybsgs.le32(q[1]), None, 0, n, d.tobytes(), flags, None, None))
        t0 = time.perf_counter()
        pybsgs._chk((L.bsgs_kangaroo_dptable_begin_keys if a.keys else L.bsgs_kangaroo_dptable_begin)(dev.h, a.dptable))
        begin_s = time.perf_counter() - t0
        seen, n_entries = C.c_uint64(), C.c_uint64()
        run_dpt = L.bsgs_kangaroo_run_dptable_keys if a.keys else L.bsgs_kangaroo_run_dptable

        def launch_dpt():
            pybsgs._chk(run_dpt(dev.h, a.steps, recs, 1 << 22, C.byref(cnt), C.byref(seen), C.byref(n_entries), C.byref(dropped), C.byref(ms)))
            return ms.value, seen.value, cnt.value

        for _ in range(a.warmup):
            launch()
            launch_dpt()
        plain, both, nrec, back, dr = [], [], 0, 0, 0
        for _ in range(a.launches):
            plain.append(launch()[0])
            k, r, m = launch_dpt()
            both.append(k)
            nrec += r
            back += m
            dr += dropped.value
        ins = (sum(both) - sum(plain)) / len(both)
        res = {"what": "kangaroo walk with the distinguished-point table in device memory, one engine, full herd, half tame half wild" + (", symmetric walk" if a.sym else "") +
               (", the table for a key list (16 keys)" if a.keys else ""),
               "gpu": dev.name(), "kangaroos": n, "per_thread": a.per_thread, "steps_per_launch": a.steps, "dp": a.dp, "launches": a.launches, "capacity": a.dptable,
               "slots": 1 << max(7, (2 * (a.dptable + (1 << 22)) - 1).bit_length()), "begin_s": begin_s,
               "ms_per_launch_walk": sum(plain) / len(plain), "ms_per_launch_walk_insert_resolve": sum(both) / len(both), "ms_insert_resolve": ins,
               "insert_resolve_share": ins / (sum(both) / len(both)), "ms_walk_each": plain, "ms_walk_insert_resolve_each": both,
               "records_per_launch": nrec / a.launches, "records_handed_back_per_launch": back / a.launches, "dropped": dr, "entries": n_entries.value,
               "steps_per_s_kernel_walk": n * a.steps / (sum(plain) / len(plain) / 1e3), "steps_per_s_kernel_walk_insert_resolve": n * a.steps / (sum(both) / len(both) / 1e3)}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        dev.close()
        return

    if a.tames:
        import numpy as np
        t0 = time.perf_counter()
        tags = np.arange(1, a.tames + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)      # an odd multiplier: pairwise different
        pybsgs._chk((L.bsgs_kangaroo_tames_install_keys if a.keys else L.bsgs_kangaroo_tames_install)(dev.h, tags.ctypes.data_as(C.POINTER(C.c_uint64)), a.tames))
        install_s = time.perf_counter() - t0
        seen = C.c_uint64()
        entries = (C.c_uint32 * (1 << 22))()

        def launch_tames():
            if a.keys:
                pybsgs._chk(L.bsgs_kangaroo_run_tames_keys(dev.h, a.steps, recs, entries, 1 << 22, C.byref(cnt), C.byref(seen), C.byref(dropped), C.byref(ms)))
            else:
                pybsgs._chk(L.bsgs_kangaroo_run_tames(dev.h, a.steps, recs, 1 << 22, C.byref(cnt), C.byref(seen), C.byref(dropped), C.byref(ms)))
            return ms.value, seen.value, cnt.value

        for _ in range(a.warmup):
            launch()
            launch_tames()
        plain, both, nrec, back = [], [], 0, 0
        for _ in range(a.launches):
            plain.append(launch()[0])
            k, r, m = launch_tames()
            both.append(k)
            nrec += r
            back += m
        match = (sum(both) - sum(plain)) / len(both)
        res = {"what": "kangaroo walk with a tame table matched on the device, one engine, full herd" + (", symmetric walk" if a.sym else "") + (", a key per kangaroo" if a.keys else ""), "gpu": dev.name(), "kangaroos": n,
               "per_thread": a.per_thread, "steps_per_launch": a.steps, "dp": a.dp, "launches": a.launches, "tame_entries": a.tames, "image_bytes": 64 * max(64, 1 << (max(a.tames - 1, 1) // 2).bit_length()),
               "install_s": install_s, "ms_per_launch_walk": sum(plain) / len(plain), "ms_per_launch_walk_and_match": sum(both) / len(both), "ms_match": match,
               "match_share": match / (sum(both) / len(both)), "records_per_launch": nrec / a.launches, "records_returned_per_launch": back / a.launches,
               "steps_per_s_kernel_walk": n * a.steps / (sum(plain) / len(plain) / 1e3), "steps_per_s_kernel_walk_and_match": n * a.steps / (sum(both) / len(both) / 1e3)}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        dev.close()
        return

    for _ in range(a.warmup):
        launch()
    kms, nrec = [], 0
    t0 = time.perf_counter()
    for _ in range(a.launches):
        k, r = launch()
        kms.append(k)
        nrec += r
    wall = time.perf_counter() - t0
    steps = n * a.steps * a.launches
    bps = BYTES_PER_STEP_SYM + 32 * 17 / a.steps if a.sym else BYTES_PER_STEP
    res = {"what": "kangaroo walk rate, one engine, full herd" + (", symmetric walk, %d jump points" % a.jumps if a.sym else "") + (", a key per kangaroo" if a.keys else ""), "gpu": dev.name(), "kangaroos": n, "per_thread": a.per_thread, "steps_per_launch": a.steps, "dp": a.dp,
           "launches": a.launches, "steps_per_s": steps / wall, "steps_per_s_kernel": steps / (sum(kms) / 1e3), "ms_per_launch": sum(kms) / len(kms),
           "ms_per_launch_min": min(kms), "bytes_per_step": bps, "hbm_GBps_implied": steps * bps / (sum(kms) / 1e3) / 1e9,
           "records_per_launch": nrec / a.launches, "vgprs": None if a.no_vgprs else vgprs(a.sym, a.keys)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
