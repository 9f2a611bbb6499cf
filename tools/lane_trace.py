#!/usr/bin/env python3
"""Launch boundaries of the fused loop from a `rocprofv3 --kernel-trace --output-format csv` run of bench.py.

    python tools/lane_trace.py <dir with *_kernel_trace.csv> [kernel substring, default advect_run_kernel]

Prints, for the dispatches of the fused kernel in the order they started: how many there are and on which hardware queues,
their durations, the idle time between the end of one and the start of the next (one stream), how much of the time two of
them ran at once (two lanes), and the time in which none ran between the first start and the last end.  Dispatches more
than 1 ms apart from both neighbours' pattern (re-sorts, the warm-up / timed boundary) are listed as `breaks`.
"""
import csv
import glob
import os
import sys


def load(src, needle):
    rows = []
    for f in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if needle in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)))
    rows.sort()
    return rows


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))] if v else float("nan")


def main():
    src = sys.argv[1]
    needle = sys.argv[2] if len(sys.argv) > 2 else "advect_run_kernel"
    d = load(src, needle)
    if not d:
        print("no dispatch of %s under %s" % (needle, src))
        return 1
    queues = {}
    for s, e, q, g in d:
        queues.setdefault(q, []).append((s, e, g))
    print("%d dispatches of %s on %d hardware queue(s): %s" % (len(d), needle, len(queues),
          ", ".join("queue %s: %d (grid %s)" % (q, len(v), "/".join(str(x) for x in sorted({g for _, _, g in v}))) for q, v in sorted(queues.items()))))
    dur = [(e - s) / 1e3 for s, e, _, _ in d]
    print("duration us: median %.1f  p10 %.1f  p90 %.1f  max %.1f" % (pct(dur, .5), pct(dur, .1), pct(dur, .9), max(dur)))
    # union of busy intervals: time with >= 1 and with >= 2 dispatches in flight
    ev = sorted([(s, 1) for s, _, _, _ in d] + [(e, -1) for _, e, _, _ in d])
    depth, last, t1, t2, idle = 0, ev[0][0], 0, 0, []
    for t, k in ev:
        if depth >= 1:
            t1 += t - last
        if depth >= 2:
            t2 += t - last
        if depth == 0 and t > last:
            idle.append((t - last) / 1e3)
        depth += k
        last = t
    span = (max(e for _, e, _, _ in d) - d[0][0]) / 1e3
    small = [x for x in idle if x < 1000.0]
    print("span %.1f ms: >= 1 in flight %.1f ms, >= 2 in flight %.1f ms (%.1f %% of the busy time)" % (span / 1e3, t1 / 1e6, t2 / 1e6, 100.0 * t2 / max(t1, 1)))
    print("gaps with none in flight: %d, of which %d below 1 ms: median %.2f us  p90 %.2f us  max %.2f us  sum %.1f us; breaks (>= 1 ms): %s"
          % (len(idle), len(small), pct(small, .5), pct(small, .9), max(small) if small else float("nan"), sum(small),
             " ".join("%.1fms" % (x / 1e3) for x in idle if x >= 1000.0) or "none"))
    for q, v in sorted(queues.items()):
        g = [(v[k + 1][0] - v[k][1]) / 1e3 for k in range(len(v) - 1)]
        g = [x for x in g if x < 1000.0]
        print("queue %s: end -> next start on the same queue: median %.2f us  p90 %.2f us  (%d pairs)" % (q, pct(g, .5), pct(g, .9), len(g)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
