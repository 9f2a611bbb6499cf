#!/usr/bin/env python3
"""Cost of sitrk_tri2quad at the C3 size of bench.py.

    python tools/bench_tri2quad.py [--side N] [--reps R] [--out TABLE.md]

An N x N (default 3163: 10^7 points) jittered square lattice and the 2 (N-1)^2 triangles of lattice_cells, default parameters,
once in lattice order and once with the triangle list shuffled.  The two variants are run in alternating passes, R (default 7)
each, and the medians reported.  Two clocks: sitrk_timer_* around the whole call (points and triangles up, all kernels, the
rounds' read-backs, quads and tri_quad down to pageable host memory), and the HIP events the library keeps around its four
phases (sitrk_tri2quad_kernel_ms).  Algorithmic bytes per triangle, with S = table slots / triangles:
    adjacency   12 indices + 48 points + 1 live + 48 table (3 x compare-and-swap 8 + add 8) + 16 S table cleared + 4 mate cleared
    scores      12 + 48 + 1 + 48 table probes + 84 neighbours (3 x (12 indices + 16 point)) + 36 out
    one round   68 pick (mate 4, neighbours 12, their mates 12, scores 24, indices 12, pick 4) + 12 match; an upper bound: a
                triangle that is already paired reads its mate and writes its pick, 8 + 12
    compaction  4 count + 9 emit + per quadrangle 24 indices + 64 points + 16 row + 8 tri_quad
`frac` is those bytes over the phase's time against 0.6 x 8 TB/s, the device-copy rate DESIGN.md uses as the HBM bound.  The
only other yardstick there is, labelled as such: the wall time of the numpy restatement of the contract (tests/test_tri2quad.py)
on the 257 x 257 lattice of the test suite, on one CPU core.  Prints one JSON line per variant; --out writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sitrack_amd import _lib  # noqa: E402
from sitrack_amd.deformation import lattice_cells  # noqa: E402

HBM_BOUND = 0.6 * 8e12
PHASES = ("adjacency", "scores", "rounds", "compaction")


def jittered(n, dkm=3.11, jitter=0.2, seed=1234):
    rng = np.random.default_rng(seed)
    ax = dkm * (np.arange(n) - 0.5 * (n - 1))
    return np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2) + rng.uniform(-jitter * dkm, jitter * dkm, (n * n, 2))


def slots_of(nT):
    s = 64
    while s < 6 * nT:
        s <<= 1
    return s


def cpu_yardstick():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_tri2quad import tri2quad_ref
    yx, tris = jittered(257, dkm=10.0), lattice_cells(257, 257, "tri")
    t0 = time.perf_counter()
    quads, _ = tri2quad_ref(yx, tris)
    return time.perf_counter() - t0, len(tris), len(quads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    t0 = time.perf_counter()
    n = a.side
    yx = jittered(n)
    tri = lattice_cells(n, n, "tri")
    nP, nT = len(yx), len(tri)
    rng = np.random.default_rng(99)
    variants = [("lattice order", tri), ("shuffled", np.ascontiguousarray(tri[rng.permutation(nT)]))]
    ctx = _lib.Context(0)
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "points": nP, "triangles": nT, "table_slots": slots_of(nT)}), flush=True)
    acc = {name: {"call": [], "ms": [], "nQ": 0, "rounds": 0} for name, _ in variants}
    for name, t in variants:                                                # warm-up: scratch sized, code loaded
        q, _, r = ctx.tri2quad(yx, t)
        acc[name]["nQ"], acc[name]["rounds"] = len(q), r
    for _ in range(a.reps):                                                 # alternating passes
        for name, t in variants:
            ctx.timer_start()
            ctx.tri2quad(yx, t)
            acc[name]["call"].append(ctx.timer_stop())
            acc[name]["ms"].append(ctx.tri2quad_kernel_ms())
    ctx.close()
    S = slots_of(nT) / nT
    rows = []
    for name, _ in variants:
        d = acc[name]
        ms = np.median(np.array(d["ms"]), axis=0)
        nQ, rounds = d["nQ"], d["rounds"]
        per_tri = {"adjacency": 12 + 48 + 1 + 48 + 16 * S + 4, "scores": 12 + 48 + 1 + 48 + 84 + 36, "rounds": 80. * rounds,
                   "compaction": 4 + 9 + 112. * nQ / nT}
        r = {"variant": name, "triangles": nT, "quads": nQ, "rounds": rounds, "reps": a.reps, "call_ms": round(float(np.median(d["call"])), 1),
             "kernels_ms": round(float(ms.sum()), 3)}
        for k, ph in enumerate(PHASES):
            r[ph + "_ms"] = round(float(ms[k]), 3)
            r[ph + "_B_per_tri"] = round(per_tri[ph], 1)
            r[ph + "_frac"] = round(per_tri[ph] * nT / (ms[k] * 1e-3) / HBM_BOUND, 3)
        r["copies_ms"] = round(r["call_ms"] - r["kernels_ms"], 1)
        r["copies_MB"] = round((16 * nP + 12 * nT + 16 * nQ + 4 * nT) / 1e6, 1)
        r["tri_per_s_kernels"] = float("%.4g" % (nT / (ms.sum() * 1e-3)))
        rows.append(r)
        print(json.dumps(r), flush=True)
    cpu_s, cpu_nT, cpu_nQ = cpu_yardstick()
    print(json.dumps({"cpu_restatement_257x257_s": round(cpu_s, 3), "triangles": cpu_nT, "quads": cpu_nQ}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# sitrk_tri2quad at the C3 size (tools/bench_tri2quad.py)\n\n")
            f.write("%d points on a %d x %d jittered lattice (3.11 km, jitter 0.2), %d triangles, default parameters, %d table slots; "
                    "the two variants in alternating passes, medians of %d.  `call` = HIP events around the whole call; the phases = "
                    "HIP events inside the library; `copies` = call - phases: %s MB of points and triangles up, quads and tri_quad "
                    "down, pageable host memory.  B/tri = algorithmic bytes per triangle (see the tool's docstring; the rounds' is an "
                    "upper bound), `frac` = those bytes over the phase's time against 0.6 x 8 TB/s = 4.8 TB/s.\n\n"
                    % (nP, n, n, nT, slots_of(nT), a.reps, rows[0]["copies_MB"]))
            f.write("| variant | quads | rounds | call ms | copies ms | " + " | ".join("%s ms | B/tri | frac" % p for p in PHASES) + " | triangles/s (phases) |\n")
            f.write("|" + "---|" * (6 + 3 * len(PHASES)) + "\n")
            for r in rows:
                f.write("| %s | %d | %d | %.1f | %.1f | " % (r["variant"], r["quads"], r["rounds"], r["call_ms"], r["copies_ms"]) +
                        " | ".join("%.3f | %.0f | %.2f" % (r[p + "_ms"], r[p + "_B_per_tri"], r[p + "_frac"]) for p in PHASES) +
                        " | %.3g |\n" % r["tri_per_s_kernels"])
            f.write("\nThe only other yardstick, and no more than that: the numpy restatement of the contract (tests/test_tri2quad.py, greedy "
                    "form) takes %.2f s of wall time on one CPU core for the %d triangles of the 257 x 257 lattice of the test suite (%d "
                    "quadrangles).\n" % (cpu_s, cpu_nT, cpu_nQ))


if __name__ == "__main__":
    main()
