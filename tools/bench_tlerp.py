#!/usr/bin/env python3
"""Cost of interpolating the fields in time (sitrk_run_tlerp) against sub-stepped advection without it (sitrk_run) on the
C3-shaped synthetic workload of bench.py, in one process.

    python tools/bench_tlerp.py [--buoys N] [--nsub 6,24] [--reps 7] [--out FILE.md]

C3 shape: 4096 x 4096 regular C-grid (4 km cells), 10^7 buoys uniform in the central 60 %, fp32 records of the synthetic
solid-body rotation (the fields bench.py uses), rdt = 3600 * nsub as tools/bench_substep.py.  Eight resident records; a timed
pass is `--launches` launches of six records each -- for sitrk_run_tlerp with phase 0.5 and both partners resident (6 + 2 slots),
for sitrk_run the same six records per call (one launch of advect_substep_kernel, the baseline: it is not touched by the
feature).  The buoys are re-created before every pass, so both sides step the same buoys through the same records; a pass is
preceded by one untimed launch; passes of the two sides alternate; GPU time by HIP events around the pass (sitrk_timer_*).
Prints one JSON line per nsub with every pass's time, the medians and their ratio; --out appends a markdown table."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sitrack_amd import _lib  # noqa: E402
from sitrack_amd import synthetic as syn  # noqa: E402

K, M = 8, 6


def one_pass(ctx, yx, ji, tlerp, launches):
    ctx.set_buoys(yx, ji)

    def launch(jrec):
        if tlerp:
            ctx.run_tlerp(jrec % K, jrec, M, 0.5, True, True)
        else:
            ctx.run(jrec % K, jrec, M)
    launch(1)                                            # warm-up: the same launch, untimed
    ctx.sync()
    alive0 = ctx.count_alive()
    ctx.launch_stats(reset=True)
    ctx.timer_start()
    for b in range(launches):
        launch(1 + M * (b + 1))
    ms = ctx.timer_stop()
    st = ctx.launch_stats()
    assert st == {"fused_launches": launches, "fused_records": launches * M, "step_launches": 0}, st
    return ms, 0.5 * (alive0 + ctx.count_alive())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buoys", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nsub", default="6,24")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
    ctx.sync()
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "Nj": a.size, "Ni": a.size, "buoys": len(yx)}), flush=True)
    rows = []
    for nsub in [int(x) for x in a.nsub.split(",")]:
        ctx.set_params(3600. * nsub, 1, 0.1)
        ctx.set_substeps(nsub)
        t = {False: [], True: []}
        live = {}
        for rep in range(a.reps):
            for tl in (False, True):                     # alternating: drift of the clocks hits both sides alike
                ms, live[tl] = one_pass(ctx, yx, ji, tl, a.launches)
                t[tl].append(ms)
        nrec = a.launches * M
        med = {tl: statistics.median(t[tl]) for tl in t}
        row = {"nsub": nsub, "records": nrec, "reps": a.reps,
               "run_ms": [round(x, 3) for x in t[False]], "tlerp_ms": [round(x, 3) for x in t[True]],
               "run_median_ms": round(med[False], 3), "tlerp_median_ms": round(med[True], 3),
               "run_ms_per_substep": round(med[False] / (nrec * nsub), 4), "tlerp_ms_per_substep": round(med[True] / (nrec * nsub), 4),
               "ratio": round(med[True] / med[False], 4),
               "run_particle_substeps_per_s": live[False] * nrec * nsub / (med[False] * 1e-3),
               "tlerp_particle_substeps_per_s": live[True] * nrec * nsub / (med[True] * 1e-3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("| nsub | records | sitrk_run median ms (min..max) | sitrk_run_tlerp median ms (min..max) | ratio | ms per sub-step run / tlerp |\n")
            f.write("|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %d | %d | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | %.3f | %.4f / %.4f |\n"
                        % (r["nsub"], r["records"], r["run_median_ms"], min(r["run_ms"]), max(r["run_ms"]), r["tlerp_median_ms"],
                           min(r["tlerp_ms"]), max(r["tlerp_ms"]), r["ratio"], r["run_ms_per_substep"], r["tlerp_ms_per_substep"]))


if __name__ == "__main__":
    main()
