#!/usr/bin/env python3
"""Cost of sitrk_delaunay on a jittered lattice.

    python tools/bench_delaunay.py [--sides 1000,3163] [--reps 7] [--bins 1,2,3,4] [--scipy-side 1000] [--out TABLE.md]

For every side n: n*n points on a jittered lattice (spacing 3.11 km, jitter 0.2 spacings, shuffled indices), rmax = 1.5
spacings.  Per value of the knob `delaunay_bin`: medians of `reps` calls of the HIP-event times of the three phases
(sitrk_delaunay_kernel_ms: binning, the triangle kernel, the compaction), triangles per second of the phases, in-circle tests
per point and the share of them that took the 128-bit path (sitrk_delaunay_stats).  Algorithmic bytes per point of the two
memory-bound phases, against 0.6 x 8 TB/s = 4.8 TB/s:
    binning     16 (point) + 16 + 1 (integer coordinates, flag) + 16 + 8 (key, index) + 4 * 16 (radix sort, two passes of pairs)
                + 8 + 16 + 16 (gather) + 16 + 16 (duplicates) = 209
    compaction  per triangle: 12 (row list written by the triangle kernel is not counted here) read + 4 * 12 (radix sort) + 12 + 12
The triangle kernel is compute bound: its yardstick is in-circle tests per second.
The baseline is scipy.spatial.Delaunay (Qhull) on the same points of --scipy-side on the host, one core, wall time; it computes the
full triangulation, hull triangles included.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sitrack_amd import _lib  # noqa: E402

HBM_BOUND = 0.6 * 8e12
DKM = 3.11


def jittered(n, jitter=0.2, seed=1234):
    rng = np.random.default_rng(seed)
    ax = DKM * (np.arange(n) - 0.5 * (n - 1))
    yx = np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2) + rng.uniform(-jitter * DKM, jitter * DKM, (n * n, 2))
    return np.ascontiguousarray(yx[rng.permutation(n * n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="1000,3163")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bins", default="1,2,3,4")
    ap.add_argument("--scipy-side", type=int, default=1000, help="0: no host baseline")
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    rmax = 1.5 * DKM
    ctx = _lib.Context(0)
    rows = []
    for n in (int(v) for v in a.sides.split(",")):
        yx = jittered(n)
        nP = len(yx)
        for m in (int(v) for v in a.bins.split(",")):
            ctx.set_tuning(delaunay_bin=m)
            tris, nT, _ = ctx.delaunay(yx, rmax)                             # warm-up: scratch sized, code loaded
            ms, call = [], []
            for _ in range(a.reps):
                ctx.timer_start()
                ctx.delaunay(yx, rmax)
                call.append(ctx.timer_stop())
                ms.append(ctx.delaunay_kernel_ms())
            tests, exact = ctx.delaunay_stats()
            med = np.median(np.array(ms), axis=0)
            r = {"points": nP, "delaunay_bin": m, "triangles": nT, "reps": a.reps, "call_ms": round(float(np.median(call)), 1),
                 "bin_ms": round(float(med[0]), 3), "tri_ms": round(float(med[1]), 3), "compact_ms": round(float(med[2]), 3),
                 "tri_per_s_phases": float("%.4g" % (nT / (med.sum() * 1e-3))),
                 "incircle_per_point": round(tests / nP, 1), "incircle_per_s": float("%.4g" % (tests / (med[1] * 1e-3))),
                 "exact_share": float("%.3g" % (exact / max(tests, 1))),
                 "bin_frac": round(209. * nP / (med[0] * 1e-3) / HBM_BOUND, 3),
                 "compact_frac": round(84. * nT / (med[2] * 1e-3) / HBM_BOUND, 3)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del tris
    ctx.close()
    base = None
    if a.scipy_side:
        from scipy.spatial import Delaunay
        yx = jittered(a.scipy_side)
        t0 = time.perf_counter()
        d = Delaunay(yx)
        base = {"scipy_points": len(yx), "scipy_s": round(time.perf_counter() - t0, 2), "scipy_triangles": len(d.simplices)}
        print(json.dumps(base), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# sitrk_delaunay on a jittered lattice (tools/bench_delaunay.py)\n\n")
            f.write("n x n points, spacing %.2f km, jitter 0.2 spacings, shuffled indices, rmax = 1.5 spacings; medians of %d calls.  "
                    "`call` = HIP events around the whole call (host copies of pageable memory included); the phases = HIP events "
                    "inside the library (binning includes the host's read of the bounding box).  `frac` = algorithmic bytes over "
                    "the phase's time against 4.8 TB/s (209 B per point for binning, 84 B per triangle for compaction).\n\n" % (DKM, a.reps))
            f.write("| points | delaunay_bin | triangles | call ms | binning ms | frac | triangles ms | in-circle / point | in-circle / s | "
                    "128-bit share | compaction ms | frac | triangles/s (phases) |\n")
            f.write("|" + "---|" * 13 + "\n")
            for r in rows:
                f.write("| %d | %d | %d | %.1f | %.3f | %.3f | %.3f | %.1f | %.3g | %.3g | %.3f | %.3f | %.3g |\n" %
                        (r["points"], r["delaunay_bin"], r["triangles"], r["call_ms"], r["bin_ms"], r["bin_frac"], r["tri_ms"],
                         r["incircle_per_point"], r["incircle_per_s"], r["exact_share"], r["compact_ms"], r["compact_frac"],
                         r["tri_per_s_phases"]))
            if base:
                f.write("\nBaseline: scipy.spatial.Delaunay (Qhull, the full triangulation) on the %d points of the same lattice, host, "
                        "one core: %.2f s wall, %d triangles.\n" % (base["scipy_points"], base["scipy_s"], base["scipy_triangles"]))


if __name__ == "__main__":
    main()
