#!/usr/bin/env python3
"""Cost of the distribution of a device-resident mesh's rates (sitrk_mesh_dist) against the path it replaces.

    python tools/bench_dist.py [--side 3163] [--reps 7] [--bins 64] [--out TABLE.md]

The cloud of tools/bench_mesh.py -- side x side points on a jittered lattice, spacing 3.11 km, shuffled indices, rmax = 1.5
spacings -- as the buoys of a tracker, one mesh, one record stepped.  Alternating passes, medians of `reps`:
    (a)   IceTracker.mesh_dist of tot: `bins` geometric bins and the six quantiles of --deform-pdf, as shipped: plain LDS adds in
          the select passes ...
    (a1)  ... and with their per-wave aggregation (the knob dist_aggregate)
    (b)   the path to the same numbers without it: IceTracker.mesh_deform in full, then on the host t2 of the status-1 cells,
          np.histogram on the squared edges and np.partition at the ranks; checked to give the same counts and bits
Wall clock around the Python call, and HIP events inside the library (sitrk_dist_kernel_ms: keys, histogram, selection;
sitrk_dist_stats: the top-digit pass alone).  `core` is what the same call spends in the pass over the buoys and the cell kernel
of sitrk_mesh_deform (sitrk_mesh_kernel_ms), which run in front of those phases.  The counting passes are set against the
device-copy rate the project quotes, 0.6 of 8 TB/s: the histogram reads 8 bytes per key once, the selection once per pass.  One
JSON line per figure."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sitrack_amd as sit  # noqa: E402
from sitrack_amd import distribution as dst  # noqa: E402
from sitrack_amd import synthetic as syn  # noqa: E402
from bench_delaunay import DKM, jittered  # noqa: E402

COPY_RATE = 0.6 * 8e12                       # bytes/s, the device-copy rate of DESIGN.md


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def host_route(full, e2, q):
    """(counts, values, m) from what mesh_deform downloads: the numbers of mesh_dist, by numpy"""
    ok = full["status"] == 1
    t2 = full["div"][ok] * full["div"][ok] + full["shr"][ok] * full["shr"][ok]
    m = len(t2)
    inner = np.histogram(t2, bins=e2)[0]
    counts = np.concatenate([[int((t2 < e2[0]).sum())], inner, [0]]).astype(np.int64)
    counts[-2] -= int((t2 == e2[-1]).sum())                       # numpy's last bin is closed, the contract's is not
    counts[-1] = m - int(counts[:-1].sum())
    ranks = [min(m - 1, int(math.floor(np.float64(t) * np.float64(m)))) for t in q]
    part = np.partition(t2, sorted(set(ranks)))
    return counts, np.array([part[k] for k in ranks]), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    rmax = 1.5 * DKM
    yx = jittered(a.side)
    nP = len(yx)
    gdkm = 12.0
    N = int(np.ceil(a.side * DKM / gdkm)) + 16
    grid = syn.make_grid(N, N, dkm=gdkm)
    u, v, sic = syn.make_fields(grid, K=1, seed=5, umax=0.6, drift=0.1)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], nslots=1)
    ctx = trk.ctx
    trk.load_record(0, u[0], v[0], sic[0])
    trk.set_buoys(yx, syn.regular_host_cell(grid, yx))
    nQ = trk.mesh(rmax, 0)["nQ"]
    trk.step(0, 0)
    jrec1 = 0
    q = np.array(dst.PDF_Q)
    full = trk.mesh_deform(jrec1)                                               # warm-up: scratch sized, code loaded
    ok = full["status"] == 1
    tot = np.sqrt(full["div"][ok] ** 2 + full["shr"][ok] ** 2)
    hi = float(tot.max()) * 1.0001                                              # the bins cover the rates of this cloud
    lo = max(float(np.quantile(tot, 0.01)), hi * 1e-6)
    edges = sit.log_edges(lo, hi, a.bins)
    e2 = dst.square_edges(edges)
    want = host_route(full, e2, q)
    del full, tot
    for agg in (0, 1):                                                          # warm-up, and the numbers against the host's
        ctx.set_tuning(dist_aggregate=agg)
        d = trk.mesh_dist(jrec1, "tot", edges=edges, q=q)
        assert d["m"] == want[2] and np.array_equal(d["counts"], want[0]), "counts differ from the host's"
        assert np.array_equal(d["t2"].view(np.uint64), want[1].view(np.uint64)), "order statistics differ from the host's"
    runs = {"a": [], "a1": []}
    wall_b, wall_down = [], []
    for _ in range(a.reps):
        w, full = timed(lambda: trk.mesh_deform(jrec1))
        w2, _ = timed(lambda: host_route(full, e2, q))
        wall_down.append(w)
        wall_b.append(w + w2)
        del full
        for k, agg in (("a", 0), ("a1", 1)):
            ctx.set_tuning(dist_aggregate=agg)
            w, d = timed(lambda: trk.mesh_dist(jrec1, "tot", edges=edges, q=q))
            core = ctx.mesh_kernel_ms(build=False)
            passes, top = ctx.dist_stats()
            runs[k].append((w, core[1] + core[2]) + ctx.dist_kernel_ms() + (top, passes))
    ctx.set_tuning(dist_aggregate=0)
    trk.close()

    bytes_down = 8 * (2 + 2 * len(q) + a.bins + 2)
    head = {"points": nP, "quadrangles": nQ, "status1": want[2], "reps": a.reps, "bins": a.bins, "quantiles": len(q),
            "b_wall_ms": round(float(np.median(wall_b)), 3), "b_download_wall_ms": round(float(np.median(wall_down)), 3),
            "b_bytes_down": 41 * nQ + 80, "a_bytes_down": bytes_down}
    print(json.dumps(head), flush=True)
    rows = []
    for k in ("a", "a1"):
        m = np.median(np.array(runs[k], dtype=np.float64), axis=0)
        w_all = [x[0] for x in runs[k]]
        passes = int(m[6])
        row = {"what": k, "wall_ms": float(m[0]), "wall_spread_ms": float(max(w_all) - min(w_all)), "core_ms": float(m[1]),
               "keys_ms": float(m[2]), "hist_ms": float(m[3]), "select_ms": float(m[4]), "top_pass_ms": float(m[5]), "passes": passes,
               "hist_bytes_per_s": 8. * nQ / (float(m[3]) * 1e-3), "select_bytes_per_s": 8. * nQ * passes / (float(m[4]) * 1e-3),
               "top_pass_bytes_per_s": 8. * nQ / (float(m[5]) * 1e-3)}
        for n in ("hist", "select", "top_pass"):
            row[n + "_of_copy_rate"] = row[n + "_bytes_per_s"] / COPY_RATE
        rows.append(row)
        print(json.dumps({kk: (round(x, 4) if isinstance(x, float) else x) for kk, x in row.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Distribution of a device-resident mesh's rates (tools/bench_dist.py)\n\n")
            f.write("%d points (jittered lattice, spacing %.2f km, shuffled indices, rmax = 1.5 spacings) as the buoys of a tracker, %d "
                    "quadrangles, %d of status 1 after one record.  `mesh_dist` of tot, %d geometric bins and %d quantiles.  Alternating "
                    "passes, medians of %d; `wall` = around the Python call, `spread` = max - min of its passes; `core` = the pass over the "
                    "buoys and the cell kernel of sitrk_mesh_deform inside the same call; keys, histogram, selection = HIP events inside "
                    "the library; `top pass` = the first of the selection's %d digit passes.  Rates: 8 bytes per key (all %d quadrangles: a "
                    "marker is read too) once for the histogram, once per pass for the selection, as a fraction of the device-copy rate "
                    "of 0.6 x 8 TB/s.\n\n" % (nP, DKM, nQ, want[2], a.bins, len(q), a.reps, rows[0]["passes"], nQ))
            f.write("(b) the route without it, re-measured in the same passes: `mesh_deform` in full %.2f ms wall, %d bytes down; with "
                    "t2, np.histogram and np.partition on the host %.2f ms wall.  The same counts and the same bits.\n\n"
                    % (head["b_download_wall_ms"], head["b_bytes_down"], head["b_wall_ms"]))
            f.write("| what | wall ms | spread ms | core ms | keys ms | histogram ms | selection ms | top pass ms | bytes down | histogram "
                    "TB/s (of copy) | selection TB/s (of copy) | top pass TB/s (of copy) |\n|" + "---|" * 12 + "\n")
            for r in rows:
                f.write("| %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %d | %.3f (%.2f) | %.3f (%.2f) | %.3f (%.2f) |\n"
                        % ("(a) mesh_dist" if r["what"] == "a" else "(a1) with the wave aggregation", r["wall_ms"], r["wall_spread_ms"],
                           r["core_ms"], r["keys_ms"], r["hist_ms"], r["select_ms"], r["top_pass_ms"], bytes_down,
                           r["hist_bytes_per_s"] / 1e12, r["hist_of_copy_rate"], r["select_bytes_per_s"] / 1e12, r["select_of_copy_rate"],
                           r["top_pass_bytes_per_s"] / 1e12, r["top_pass_of_copy_rate"]))


if __name__ == "__main__":
    main()
