#!/usr/bin/env python3
"""Cost of the distance to the model coastline (sitrk_coast_build / sitrk_coast_dist / sitrk_coast_dist_buoys) at the C3 size
of bench.py.

    python tools/bench_coast.py [--points N] [--reps R] [--size S] [--bin B] [--out TABLE.md]

An S x S (default 4096) mesh of 4-km cells whose land is a rim of two cells and a regular pattern of rounded islands
(sin(2 pi j / 512) sin(2 pi i / 640) > 0.6), N (default 10^7) points uniform over the central 90 % of it, queried once as host
points in random order (sitrk_coast_dist: points up, distances and segments down) and once as the cell-sorted buoy state of a
tracker (sitrk_coast_dist_buoys: only the results come down), each unbounded and with rmax = 100 km, each repeated R times.
Two clocks: sitrk_timer_* around the whole call, and the HIP events the library keeps around its query kernel
(sitrk_coast_kernel_ms).  The least a query can move is 16 bytes in and 12 out (28; 32 for the buoy state, which also reads its
perm word); what it really reads -- two bin offsets per row it walks, 36 bytes per segment it evaluates -- depends on how far
from the coast it lies and comes out of L2, so `min_bytes_frac` (28 or 32 bytes per query over kernel time against 0.6 x 8 TB/s)
says how far the kernel is from a pure stream, not how well it uses the memory system.  Prints one JSON line per variant;
--out writes the table."""
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

HBM_BOUND = 0.6 * 8e12


def land_pattern(grid):
    Nj, Ni = grid["tmask"].shape
    jj, ii = np.meshgrid(np.arange(Nj), np.arange(Ni), indexing="ij")
    grid["tmask"][np.sin(2. * np.pi * jj / 512.) * np.sin(2. * np.pi * ii / 640.) > 0.6] = 0
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--bin", type=int, default=None, help="knob coast_bin (1..64); default: the library's")
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    t0 = time.perf_counter()
    grid = land_pattern(syn.make_grid(a.size, a.size, dkm=4.0, warp=0.0))
    half = 0.5 * 0.9 * 4.0 * (a.size - 1)
    rng = np.random.default_rng(1234)
    yx = rng.uniform(-half, half, (a.points, 2))
    ctx = _lib.Context(0)
    ctx.set_grid(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"])
    if a.bin is not None:
        ctx.set_tuning(coast_bin=a.bin)
    ctx.timer_start()
    nseg, ndropped = ctx.coast_build()
    build_ms = ctx.timer_stop()
    ctx.set_buoys(yx, syn.regular_host_cell(grid, yx).astype(np.int32))
    ctx.sync()
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "mesh": [a.size, a.size], "land_cells": int((grid["tmask"] == 0).sum()),
                      "segments": nseg, "dropped": ndropped, "build_ms": round(build_ms, 2), "points": a.points,
                      "coast_bin": a.bin if a.bin is not None else "default"}), flush=True)
    variants = [("host points, unbounded", False, None), ("host points, rmax 100 km", False, 100.),
                ("buoy state, unbounded", True, None), ("buoy state, rmax 100 km", True, 100.)]
    rows = []
    for name, buoys, rmax in variants:
        run = (lambda: ctx.coast_dist_buoys(rmax)) if buoys else (lambda: ctx.coast_dist(yx, rmax))
        dist, _ = run()                                        # warm-up: scratch sized, code loaded
        call, ker = [], []
        for _ in range(a.reps):
            ctx.timer_start()
            run()
            call.append(ctx.timer_stop())
            ker.append(ctx.coast_kernel_ms())
        call_ms, ker_ms = float(np.median(call)), float(np.median(ker))
        fin = np.isfinite(dist)
        r = {"variant": name, "queries": a.points, "reps": a.reps, "call_ms": round(call_ms, 2), "kernel_ms": round(ker_ms, 3),
             "kernel_ms_min_max": [round(min(ker), 3), round(max(ker), 3)],
             "queries_per_s_call": float("%.4g" % (a.points / (call_ms * 1e-3))),
             "queries_per_s_kernel": float("%.4g" % (a.points / (ker_ms * 1e-3))),
             "answered": int(fin.sum()), "mean_dist_km": round(float(dist[fin].mean()), 2) if fin.any() else None,
             "min_bytes_frac": round(a.points * (32 if buoys else 28) / (ker_ms * 1e-3) / HBM_BOUND, 4)}
        rows.append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Distance to the model coastline at the C3 size (tools/bench_coast.py)\n\n")
            f.write("%d x %d mesh of 4-km cells, rim and island pattern: %d coast segments (index built in %.1f ms, knob coast_bin %s); "
                    "%d points uniform over the central 90 %%; medians of %d calls after one warm-up call.  `call` = HIP events around the "
                    "whole call (host points: points up, kernel, dist and seg down to pageable host memory; buoy state: kernel, dist and "
                    "seg down); `kernel` = HIP events around the query kernel.  `min bytes` = 28 (32: buoy state) bytes per query over "
                    "kernel time against 0.6 x 8 TB/s = 4.8 TB/s: the distance from a pure stream, see DESIGN.md 3.10.\n\n"
                    % (a.size, a.size, nseg, build_ms, a.bin if a.bin is not None else "default", a.points, a.reps))
            f.write("| variant | call ms | queries/s (call) | kernel ms (min .. max) | queries/s (kernel) | answered | mean dist km | min bytes frac |\n")
            f.write("|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.1f | %.3g | %.3f (%.3f .. %.3f) | %.3g | %d | %s | %.4f |\n" %
                        (r["variant"], r["call_ms"], r["queries_per_s_call"], r["kernel_ms"], r["kernel_ms_min_max"][0],
                         r["kernel_ms_min_max"][1], r["queries_per_s_kernel"], r["answered"], r["mean_dist_km"], r["min_bytes_frac"]))


if __name__ == "__main__":
    main()
