#!/usr/bin/env python3
"""Throughput of sub-stepped advection (sitrk_set_substeps) on the C3-shaped synthetic workload of bench.py.

    python tools/bench_substep.py [--buoys N] [--records R] [--nsub 1,2,6,24]

C3 shape: 4096 x 4096 regular C-grid (4 km cells), 10^7 buoys uniform in the central 60 %, fp32 records of the synthetic
solid-body rotation (umax 0.3 m/s, the fields bench.py uses).  For every nsub the run uses rdt = 3600 * nsub, so each sub-step
has the hourly displacement of the headline run (nsub = 1 is that run: advect_run_kernel).  R records are advanced in fused
launches of up to 8 resident records after a warm-up of 8; the buoys are re-created for every nsub.  Prints one JSON line per
nsub: particle-sub-steps per second (live buoys x sub-steps / GPU time), ms per launch and per record, and the launch split
of sitrk_launch_stats."""
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
    ap.add_argument("--records", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--nsub", default="1,2,6,24")
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
    ctx.sync()
    print(json.dumps({"setup_s": round(time.perf_counter() - t0, 1), "Nj": a.size, "Ni": a.size, "buoys": len(yx)}), flush=True)
    for nsub in [int(x) for x in a.nsub.split(",")]:
        ctx.set_params(3600. * nsub, 1, 0.1)
        ctx.set_substeps(nsub)
        ctx.set_buoys(yx, ji)
        jrec = 0
        for b in range(0, a.warmup, K):
            m = min(K, a.warmup - b)
            ctx.run(jrec % K, jrec, m)
            jrec += m
        ctx.sync()
        alive0 = ctx.count_alive()
        ctx.launch_stats(reset=True)
        ctx.timer_start()
        for b in range(0, a.records, K):
            m = min(K, a.records - b)
            ctx.run(jrec % K, jrec, m)
            jrec += m
        ms = ctx.timer_stop()
        st = ctx.launch_stats()
        alive1 = ctx.count_alive()
        live = 0.5 * (alive0 + alive1)
        launches = st["fused_launches"] + st["step_launches"]
        print(json.dumps({"nsub": nsub, "rdt": 3600. * nsub, "records": a.records, "ms": round(ms, 3),
                          "ms_per_record": round(ms / a.records, 4), "ms_per_substep": round(ms / (a.records * nsub), 4),
                          "ms_per_launch": round(ms / max(1, launches), 4),
                          "particle_substeps_per_s": live * a.records * nsub / (ms * 1e-3),
                          "alive_before": alive0, "alive_after": alive1, "launch_stats": st}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
