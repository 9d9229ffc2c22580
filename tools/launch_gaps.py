#!/usr/bin/env python3
"""tools/launch_gaps.py KERNEL_TRACE.csv [--csv OUT.csv]: what happens at the boundaries between tile kernels in a `rocprofv3 --kernel-trace` of bench.py.

Reads the per-dispatch start and end times of the tile kernel (giant_pair2_kernel / giant_tile_kernel) and prints, for the last `--last` dispatches (the timed
region and the end of the warm-up): per queue the gap between one kernel's end and the next one's start, and across queues how much of every kernel ran
concurrently with a kernel of the other queue and how far the ends of the two queues' kernels lie apart (launch overlap, DESIGN.md 4: boundaries that coincide
gain nothing).  --csv writes the tile-kernel rows alone (queue, start and end in microseconds from the first row, grid size): the committed record."""
import argparse
import csv
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--csv", default=None)
    ap.add_argument("--last", type=int, default=40)
    args = ap.parse_args()
    rows = []
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            if "giant_pair2_kernel" in r["Kernel_Name"] or "giant_tile_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Stream_Id"], int(r["Grid_Size_X"]), r["Kernel_Name"]))
    rows.sort()
    t0 = rows[0][0]
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["kernel", "queue", "stream", "grid_size_x", "start_us", "end_us", "duration_us"])
            for s, e, q, st, g, name in rows:
                w.writerow([name.replace("void ", "").replace("(TileArgs)", ""), q, st, g, "%.1f" % ((s - t0) / 1e3), "%.1f" % ((e - t0) / 1e3), "%.1f" % ((e - s) / 1e3)])
    rows = rows[-args.last:]
    streams = sorted({r[3] for r in rows})
    print("%d tile kernels, streams %s, grids %s" % (len(rows), streams, sorted({r[4] for r in rows})))
    for st in streams:
        mine = [r for r in rows if r[3] == st]
        gaps = [(b[0] - a[1]) / 1e3 for a, b in zip(mine, mine[1:]) if b[0] - a[1] < 20e6]        # (a collect in between: not a queued boundary)
        durs = [(r[1] - r[0]) / 1e6 for r in mine]
        if gaps:
            print("stream %s: %d kernels, duration median %.3f ms; gap end -> next start on this stream: median %.1f us, min %.1f, max %.1f (%d gaps)" % (
                st, len(mine), statistics.median(durs), statistics.median(gaps), min(gaps), max(gaps), len(gaps)))
    if len(streams) >= 2:
        a, b = ([r for r in rows if r[3] == st] for st in streams[:2])
        conc, offs = [], []
        for s, e, *_ in a:
            conc.append(sum(max(0, min(e, e2) - max(s, s2)) for s2, e2, *_ in b) / (e - s))
            offs.append(min(abs(e - e2) for _, e2, *_ in b) / 1e6)
        print("kernels of stream %s: %.0f %% of their time concurrent with a kernel of stream %s (median); distance from their end to the nearest end on the other "
              "stream: median %.2f ms, min %.2f, max %.2f" % (streams[0], 100 * statistics.median(conc), streams[1], statistics.median(offs), min(offs), max(offs)))
        starts_before_end = sum(1 for s2, e2, *_ in b if any(s < s2 < e for s, e, *_ in a))
        print("%d of %d kernels of stream %s start while a kernel of stream %s is running" % (starts_before_end, len(b), streams[1], streams[0]))
    span = (rows[-1][1] - rows[0][0]) / 1e6
    busy = sorted((r[0], r[1]) for r in rows)
    idle, end = 0, busy[0][1]
    for s, e in busy[1:]:
        if s > end and s - end < 20e6:
            idle += s - end
        end = max(end, e)
    print("no tile kernel running for %.3f ms of %.1f ms (gaps below 20 ms, i.e. without the collects)" % (idle / 1e6, span))


if __name__ == "__main__":
    main()
