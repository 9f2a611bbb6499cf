#!/usr/bin/env python3
"""Cost of the device-resident deformation rates (sitrk_deform_mark / sitrk_deform_since_mark) at the C3 size of bench.py.

    python tools/bench_deform.py [--buoys N] [--reps R] [--size S] [--out TABLE.md]

About N (default 10^7) buoys on a jittered square lattice over the C3 extent (the central 60 % of a 4096 x 4096 mesh of 4-km
cells), cell-sorted as the tracker keeps them, marked, stepped over two records, then the roughly 2 N triangles of
lattice_cells -- once in lattice order, once with the cell list shuffled -- and the N quadrangles.  Every variant is repeated
R times.  Two clocks: sitrk_timer_* around the whole call (upload of the cells, both kernels, download of out and valid),
and the HIP events the library keeps around its two kernels (sitrk_deform_kernel_ms).  Algorithmic bytes: per cell 4 nv (its
indices) + 41 (five fp64 and one byte out) + 2 x 16 per gathered vertex; the pass over the buoys is counted at 16 + 12 per buoy
(the point written; cell, perm and a window's worth of words read), which leaves out the 16-byte position it reads: with it the
pass moves 40 bytes per buoy without windows, and `frac_points_kernel_40` prices that.  `frac` is bytes over the kernels' time
against 0.6 x 8 TB/s, the device-copy rate DESIGN.md uses as the HBM bound.  Prints one JSON line per variant; --out writes the table."""
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
from sitrack_amd.deformation import lattice_cells  # noqa: E402

HBM_BOUND = 0.6 * 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buoys", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    K = 2
    t0 = time.perf_counter()
    grid = syn.make_grid(a.size, a.size, dkm=4.0, warp=0.0)
    u, v, sic = syn.make_fields(grid, K=K, seed=2024, umax=0.3, drift=0.05)
    n1 = int(round(np.sqrt(a.buoys)))
    half = 0.5 * 0.6 * 4.0 * (a.size - 1)
    d = 2. * half / (n1 - 1)
    rng = np.random.default_rng(1234)
    ax = np.linspace(-half, half, n1)
    yx = np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2) + rng.uniform(-0.3 * d, 0.3 * d, (n1 * n1, 2))
    nP = len(yx)
    ctx = _lib.Context(0)
    ctx.set_grid(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"])
    ctx.alloc_records(K, np.float32)
    for k in range(K):
        ctx.push_record(k, u[k], v[k], sic[k])
    ctx.set_buoys(yx, syn.regular_host_cell(grid, yx).astype(np.int32))
    ctx.deform_mark(0)
    ctx.run(0, 0, K)
    ctx.sync()
    tri = lattice_cells(n1, n1, "tri")
    variants = [("triangles, lattice order", tri),
                ("triangles, shuffled", np.ascontiguousarray(tri[rng.permutation(len(tri))])),
                ("quadrangles, lattice order", lattice_cells(n1, n1, "quad"))]
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "buoys": nP, "lattice": [n1, n1], "spacing_km": round(d, 3),
                      "alive": ctx.count_alive()}), flush=True)
    rows = []
    for name, cells in variants:
        nC, nv = cells.shape
        _, _, nvalid = ctx.deform_since_mark(K - 1, cells)                  # warm-up: scratch sized, code loaded
        call, pts, cel = [], [], []
        for _ in range(a.reps):
            ctx.timer_start()
            ctx.deform_since_mark(K - 1, cells)
            call.append(ctx.timer_stop())
            p, c = ctx.deform_kernel_ms()
            pts.append(p); cel.append(c)
        call_ms, pts_ms, cel_ms = (float(np.median(x)) for x in (call, pts, cel))
        b_cells, b_pts = nC * (4 * nv + 41 + 32 * nv), nP * (16 + 12)
        r = {"variant": name, "cells": nC, "nv": nv, "valid": nvalid, "reps": a.reps, "call_ms": round(call_ms, 2),
             "points_kernel_ms": round(pts_ms, 4), "cells_kernel_ms": round(cel_ms, 4),
             "cells_per_s_call": float("%.4g" % (nC / (call_ms * 1e-3))), "cells_per_s_kernels": float("%.4g" % (nC / ((pts_ms + cel_ms) * 1e-3))),
             "algorithmic_MB_cells": round(b_cells / 1e6, 1), "algorithmic_MB_points": round(b_pts / 1e6, 1),
             "frac_cells_kernel": round(b_cells / (cel_ms * 1e-3) / HBM_BOUND, 3),
             "frac_points_kernel": round(b_pts / (pts_ms * 1e-3) / HBM_BOUND, 3),
             "frac_points_kernel_40": round(nP * 40 / (pts_ms * 1e-3) / HBM_BOUND, 3),
             "frac_kernels": round((b_cells + b_pts) / ((pts_ms + cel_ms) * 1e-3) / HBM_BOUND, 3)}
        rows.append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# sitrk_deform_since_mark at the C3 size (tools/bench_deform.py)\n\n")
            f.write("%d buoys on a %d x %d jittered lattice (%.2f km), cell-sorted, marked and stepped over %d records; medians of %d "
                    "calls.  `call` = HIP events around the whole call (cells up, two kernels, out and valid down to pageable host "
                    "memory); `points` / `cells` = HIP events around the two kernels.  Algorithmic bytes: (4 nv + 41 + 32 nv) per cell, "
                    "28 per buoy (40 with the position read, not counted).  `frac` = algorithmic bytes over kernel time against 0.6 x 8 TB/s = 4.8 TB/s.\n\n" % (nP, n1, n1, d, K, a.reps))
            f.write("| variant | cells | call ms | cells/s (call) | points ms | cells ms | cells/s (kernels) | MB points | MB cells | frac points | frac cells | frac both |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %.1f | %.3g | %.3f | %.3f | %.3g | %.0f | %.0f | %.2f | %.2f | %.2f |\n" %
                        (r["variant"], r["cells"], r["call_ms"], r["cells_per_s_call"], r["points_kernel_ms"], r["cells_kernel_ms"],
                         r["cells_per_s_kernels"], r["algorithmic_MB_points"], r["algorithmic_MB_cells"], r["frac_points_kernel"],
                         r["frac_cells_kernel"], r["frac_kernels"]))


if __name__ == "__main__":
    main()
