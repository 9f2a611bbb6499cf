#!/usr/bin/env python3
"""Cost of sampling model fields along the trajectories (sitrk_sample_slot, sitrk_sample_fields) next to sitrk_fetch_record, on the
C3-shaped synthetic workload of bench.py.

    python tools/bench_sample.py [--buoys N] [--reps R] [--size S]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_sample.py --reps 5      # the kernels alone

C3 shape: 4096 x 4096 regular C-grid (4 km cells), 10^7 buoys uniform in the central 60 %, fp32 records.  After 8 records of
stepping, every call is repeated R times between HIP events on the compute stream (sitrk_timer_*), which span the whole call:
kernel, device -> host copy of the result and, for sitrk_sample_fields, the host -> device copy of the fields.  The kernels' own
times (fetch_record_kernel, cart2geo_kernel, sample_fields_kernel) come from the kernel trace of the second command; the
difference is the copies.  Prints one JSON line per call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sitrack_amd import _lib  # noqa: E402
from sitrack_amd import synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buoys", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args()
    K = 8
    t0 = time.perf_counter()
    grid = syn.make_grid(a.size, a.size, dkm=4.0, warp=0.0)
    u, v, sic = syn.make_fields(grid, K=K, seed=2024, umax=0.3, drift=0.05)
    ctx = _lib.Context(0)
    ctx.set_grid(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"])
    _, yx = syn.make_buoys(grid, a.buoys, seed=1234, frac=0.6)
    ji = syn.regular_host_cell(grid, yx).astype(np.int32)
    ctx.alloc_records(K, np.float32)
    for k in range(K):
        ctx.push_record(k, u[k], v[k], sic[k])
    ctx.set_buoys(yx, ji)
    ctx.run(0, 0, K)
    ctx.sync()
    jrec, slot = K - 1, K - 1
    fields = [np.ascontiguousarray(sic[k]) for k in range(4)]
    j0, j1, i0, i1 = ctx.box(0)
    boxes = [np.ascontiguousarray(f[j0:j1, i0:i1]) for f in fields]
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "Nj": a.size, "Ni": a.size, "buoys": len(yx),
                      "box": [j0, j1, i0, i1]}), flush=True)
    calls = [
        ("fetch_record(yx, mask)", lambda: ctx.fetch_record(jrec)),
        ("fetch_record(yx, mask, latlon)", lambda: ctx.fetch_record(jrec, latlon=True)),
        ("sample_slot(siconc)", lambda: ctx.sample_slot(slot, jrec, 'after', 'siconc')),
        ("sample_fields(1 f4, full field)", lambda: ctx.sample_fields(jrec, 'after', fields[:1])),
        ("sample_fields(4 f4, full field)", lambda: ctx.sample_fields(jrec, 'after', fields)),
        ("sample_fields(1 f4, box)", lambda: ctx.sample_fields(jrec, 'after', boxes[:1], box=(j0, j1, i0, i1))),
        ("sample_fields(4 f4, box)", lambda: ctx.sample_fields(jrec, 'after', boxes, box=(j0, j1, i0, i1))),
    ]
    for name, fn in calls:
        fn()                                              # warm-up: scratch sized, code loaded
        ev, wall = [], []
        for _ in range(a.reps):
            tw = time.perf_counter()
            ctx.timer_start()
            fn()
            ev.append(ctx.timer_stop())
            wall.append((time.perf_counter() - tw) * 1e3)
        print(json.dumps({"call": name, "reps": a.reps, "event_ms_median": round(float(np.median(ev)), 3),
                          "event_ms_min": round(float(np.min(ev)), 3), "wall_ms_median": round(float(np.median(wall)), 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
