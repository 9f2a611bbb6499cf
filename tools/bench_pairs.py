#!/usr/bin/env python3
"""Cost of the pair-dispersion table (sitrk_pairs_points) against a host baseline that is not the code under test.

    python tools/bench_pairs.py [--sides 1000,3163] [--reps 5] [--edges 10:160:8] [--cpu-side 150] [--out TABLE.md]

The cloud: side x side points on a lattice of 10 km, jittered by 0.2 spacings, indices shuffled; t1 = a smooth displacement of a
few percent.  Per side one warm-up call (scratch sized, code loaded), then `reps` timed calls, medians and max - min:
    wall      around Context.pairs_points: the upload of 2 x 16 bytes per point, the kernels, 56 bytes per class down
    phases    HIP events inside the library (sitrk_pairs_kernel_ms): binning (box, keys, sort, gather, bin starts; one wait for the
              bounding box lies inside it), the pairs kernel, the table
    pairs     the contributing pairs (column 0 of the table, summed), pairs/s over the pairs kernel alone and over the wall clock
    tests     the pairs the kernel formed q0 for, all class passes together (sitrk_pairs_stats), per contributing pair
The host baseline, on cpu_side x cpu_side points of the same make (0: none): scipy's cKDTree.query_pairs within the last edge,
then the contract's terms in numpy and np.add.at per class; its seconds per pair are set next to the device's.  The two tables are
compared (counts equal) before anything is reported.  One JSON line per figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sitrack_amd as sit  # noqa: E402
from sitrack_amd import _lib  # noqa: E402

DKM = 10.0
FP64_GINST = 2.4e9 * 256 * 4 / 4.35 / 1e9                             # 4.35 cycles per wave64 fp64 instruction per SIMD


def cloud(n, jitter=0.2, seed=1234):
    rng = np.random.default_rng(seed)
    ax = DKM * (np.arange(n) - 0.5 * (n - 1))
    yx = np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2) + rng.uniform(-jitter * DKM, jitter * DKM, (n * n, 2))
    yx = np.ascontiguousarray(yx[rng.permutation(n * n)])
    y, x = yx[:, 0], yx[:, 1]
    yx1 = np.stack([y + 0.02 * (0.3 * y - 0.2 * x) + 0.4 * np.sin(x / 370.), x + 0.02 * (0.1 * y + 0.25 * x) + 0.3 * np.cos(y / 290.)], axis=1)
    return yx, np.ascontiguousarray(yx1)


def host_table(yx0, yx1, edges):
    """cKDTree.query_pairs + numpy: (table, seconds for the pairs, seconds for the terms and sums)"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    ij = cKDTree(yx0).query_pairs(float(edges[-1]) * (1. + 1e-12), output_type="ndarray")
    t1 = time.perf_counter()
    i, j = ij[:, 0], ij[:, 1]
    d0, d1 = yx0[j] - yx0[i], yx1[j] - yx1[i]
    q0 = d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]
    q1 = d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]
    E = edges * edges
    cls = np.searchsorted(E, q0, side="right") - 1
    ok = (cls >= 0) & (cls < len(edges) - 1) & (q0 > 0.)
    cls, q0, q1 = cls[ok], q0[ok], q1[ok]
    r0, r1 = np.sqrt(q0), np.sqrt(q1)
    d = (q1 - q0) / (r0 + r1)
    e = d / r0
    table = np.zeros((len(edges) - 1, _lib.PAIRS_NCOLS))
    for k, t in enumerate((np.ones_like(e), r0, e, np.abs(e), e * e, (e * e) * np.abs(e), d * d)):
        np.add.at(table[:, k], cls, t)
    return table, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="1000,3163")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--edges", default="10:160:8")
    ap.add_argument("--cpu-side", type=int, default=150, help="0: no host baseline")
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    edges = sit.pairs_arg(a.edges, "--edges")
    nc = len(edges) - 1
    ctx = _lib.Context(0)
    rows, cpu = [], None
    if a.cpu_side > 0:
        yx0, yx1 = cloud(a.cpu_side)
        want, s_pairs, s_terms = host_table(yx0, yx1, edges)
        got = ctx.pairs_points(yx0, yx1, edges)["table"]
        assert np.array_equal(got[:, 0], want[:, 0]), "the device's counts differ from the host baseline's"
        assert np.allclose(got[:, 1:], want[:, 1:], rtol=1e-9, atol=0.), "the device's sums differ from the host baseline's"
        n = float(want[:, 0].sum())
        cpu = {"what": "cpu", "points": a.cpu_side ** 2, "pairs": int(n), "query_pairs_s": round(s_pairs, 4), "terms_s": round(s_terms, 4),
               "ns_per_pair": round((s_pairs + s_terms) / n * 1e9, 3)}
        print(json.dumps(cpu), flush=True)
    for side in [int(s) for s in a.sides.split(",")]:
        yx0, yx1 = cloud(side)
        first = ctx.pairs_points(yx0, yx1, edges)                              # warm-up
        walls, phases = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = ctx.pairs_points(yx0, yx1, edges)
            walls.append((time.perf_counter() - t0) * 1e3)
            phases.append(ctx.pairs_kernel_ms())
            assert np.array_equal(r["table"].view(np.uint64), first["table"].view(np.uint64)), "two calls, other bits"
        n = float(first["table"][:, 0].sum())
        tests = ctx.pairs_stats()
        ph = np.median(np.array(phases), axis=0)
        row = {"what": "gpu", "points": side * side, "classes": nc, "pairs": int(n), "pairs_per_class": [int(x) for x in first["table"][:, 0]],
               "tests": int(tests), "tests_per_pair": round(tests / n, 3), "reps": a.reps,
               "wall_ms": round(float(np.median(walls)), 3), "wall_spread_ms": round(max(walls) - min(walls), 3),
               "bin_ms": round(float(ph[0]), 3), "pairs_ms": round(float(ph[1]), 3), "table_ms": round(float(ph[2]), 3),
               "pairs_ms_spread": round(float(np.ptp(np.array(phases)[:, 1])), 3),
               "Gpairs_per_s_kernel": round(n / ph[1] / 1e6, 3), "Gpairs_per_s_wall": round(n / np.median(walls) / 1e6, 3),
               "ns_per_pair_wall": round(float(np.median(walls)) * 1e6 / n, 4),
               "fp64_inst_per_test_at_ceiling": round(FP64_GINST * 1e9 * ph[1] * 1e-3 * 64 / tests, 1),
               "beta": [round(float(b), 4) for b in sit.dispersion_exponents(first["table"], 86400.)["beta"]]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# The pair-dispersion table (tools/bench_pairs.py)\n\n")
            f.write("Points on a jittered 10-km lattice, shuffled indices; classes `%s` (%d of them).  One warm-up call, then %d timed calls: "
                    "medians, `spread` = max - min.  `wall` = around Context.pairs_points (upload of 32 bytes per point, kernels, 56 bytes per "
                    "class down); `bin`, `pairs`, `table` = HIP events inside the library, the one wait for the bounding box inside `bin`; "
                    "`tests/pair` = pairs the kernel formed q0 for, all class passes together, per contributing pair.\n\n" % (a.edges, nc, a.reps))
            f.write("| points | pairs | tests/pair | wall ms | spread ms | bin ms | pairs ms | spread ms | table ms | Gpairs/s (kernel) | "
                    "Gpairs/s (wall) |\n|" + "---|" * 11 + "\n")
            for r in rows:
                f.write("| %d | %d | %.2f | %.2f | %.2f | %.3f | %.3f | %.3f | %.3f | %.2f | %.2f |\n"
                        % (r["points"], r["pairs"], r["tests_per_pair"], r["wall_ms"], r["wall_spread_ms"], r["bin_ms"], r["pairs_ms"],
                           r["pairs_ms_spread"], r["table_ms"], r["Gpairs_per_s_kernel"], r["Gpairs_per_s_wall"]))
            if cpu:
                f.write("\nHost baseline on %d points, %d pairs: cKDTree.query_pairs %.2f s, numpy terms and np.add.at %.2f s, %.1f ns per "
                        "pair on one core.\n" % (cpu["points"], cpu["pairs"], cpu["query_pairs_s"], cpu["terms_s"], cpu["ns_per_pair"]))


if __name__ == "__main__":
    main()
