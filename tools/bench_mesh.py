#!/usr/bin/env python3
"""Cost of the device-resident quadrangle meshes (sitrk_mesh_*) against the host-array chain they replace.

    python tools/bench_mesh.py [--side 3163] [--reps 7] [--out TABLE.md]

The cloud of tools/bench_delaunay.py -- side x side points on a jittered lattice, spacing 3.11 km, shuffled indices, rmax = 1.5
spacings -- as the buoys of a tracker on a regular mesh that contains it.  Alternating passes, medians of `reps`:
    (a) IceTracker.mesh                          the build: triangulation, pairing, t0 positions, nothing leaves the device
    (d) the same through the public path of the commit before: IceTracker.tris -> IceTracker.quads -> deform_mark
then one record is stepped and
    (b) IceTracker.mesh_deform in full           rates, status and stats of every cell
    (c) IceTracker.mesh_deform(full=False)       the ten sums alone, 80 bytes from the device
    (d) IceTracker.deform(jrec1, quads)          the rates through sitrk_deform_since_mark: cells up, out / valid down
Wall clock around the Python call, and HIP events inside the library (sitrk_mesh_kernel_ms; for (d) the sum of
sitrk_delaunay_kernel_ms and sitrk_tri2quad_kernel_ms, and sitrk_deform_kernel_ms).  Algorithmic bytes of the cell kernel per
quadrangle: 16 (indices) + 64 (t0 block) + 4 * 16 (t1 gathers) + 40 (five rates) + 1 (status) = 185 in full, 144 for the sums
alone, against 0.6 x 8 TB/s = 4.8 TB/s.  One JSON line per figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sitrack_amd as sit  # noqa: E402
from sitrack_amd import synthetic as syn  # noqa: E402
from bench_delaunay import DKM, HBM_BOUND, jittered  # noqa: E402

BYTES_FULL, BYTES_STATS = 185., 144.


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def med(rows):
    return [float(x) for x in np.median(np.array(rows, dtype=np.float64), axis=0)]


def spread(x):
    return float(np.max(x) - np.min(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    rmax = 1.5 * DKM
    yx = jittered(a.side)
    nP = len(yx)
    gdkm = 12.0
    N = int(np.ceil(a.side * DKM / gdkm)) + 16                                  # the mesh contains the cloud with a margin
    grid = syn.make_grid(N, N, dkm=gdkm)
    u, v, sic = syn.make_fields(grid, K=1, seed=5, umax=0.6, drift=0.1)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], nslots=1)
    ctx = trk.ctx
    trk.load_record(0, u[0], v[0], sic[0])
    trk.set_buoys(yx, syn.regular_host_cell(grid, yx))
    jrec0 = 0
    info = trk.mesh(rmax, jrec0)                                                # warm-up: scratch sized, code loaded
    quads = trk.quads(trk.tris(rmax))[0]
    assert np.array_equal(trk.mesh_cells(), quads), "the mesh differs from the host-array chain"
    wall_a, ev_a, wall_d, ev_d = [], [], [], []
    for _ in range(a.reps):
        w, _ = timed(lambda: trk.mesh(rmax, jrec0))
        wall_a.append(w)
        ev_a.append(ctx.mesh_kernel_ms(deform=False)[0])

        def chain():
            t = trk.tris(rmax)
            q = trk.quads(t)[0]
            trk.deform_mark(jrec0)
            ctx.sync()
            return q
        w, _ = timed(chain)
        wall_d.append(w)
        ev_d.append(sum(ctx.delaunay_kernel_ms()) + sum(ctx.tri2quad_kernel_ms()))
    trk.step(jrec0, 0)
    jrec1 = jrec0
    full = trk.mesh_deform(jrec1)                                               # warm-up
    ref = trk.deform(jrec1, quads)
    assert np.array_equal(full["status"] != 0, ref["valid"]) and np.array_equal(full["div"], ref["div"]), "rates differ"
    wall_b, ev_b, wall_c, ev_c, wall_e, ev_e = [], [], [], [], [], []
    for _ in range(a.reps):
        w, _ = timed(lambda: trk.mesh_deform(jrec1))
        wall_b.append(w)
        ev_b.append(ctx.mesh_kernel_ms(build=False)[1:])
        w, _ = timed(lambda: trk.mesh_deform(jrec1, full=False))
        wall_c.append(w)
        ev_c.append(ctx.mesh_kernel_ms(build=False)[1:])
        w, _ = timed(lambda: trk.deform(jrec1, quads))
        wall_e.append(w)
        ev_e.append(ctx.deform_kernel_ms())
    nQ = info["nQ"]
    eb, ec, ee = med(ev_b), med(ev_c), med(ev_e)
    rows = [
        {"what": "(a) mesh_build", "wall_ms": float(np.median(wall_a)), "wall_spread_ms": spread(wall_a), "events_ms": float(np.median(ev_a))},
        {"what": "(d) tris + quads + deform_mark", "wall_ms": float(np.median(wall_d)), "wall_spread_ms": spread(wall_d),
         "events_ms": float(np.median(ev_d))},
        {"what": "(b) mesh_deform, full", "wall_ms": float(np.median(wall_b)), "wall_spread_ms": spread(wall_b), "points_ms": eb[0],
         "cells_ms": eb[1], "stats_ms": eb[2], "cells_frac": BYTES_FULL * nQ / (eb[1] * 1e-3) / HBM_BOUND},
        {"what": "(c) mesh_deform, stats only", "wall_ms": float(np.median(wall_c)), "wall_spread_ms": spread(wall_c), "points_ms": ec[0],
         "cells_ms": ec[1], "stats_ms": ec[2], "cells_frac": BYTES_STATS * nQ / (ec[1] * 1e-3) / HBM_BOUND},
        {"what": "(d) deform (since_mark)", "wall_ms": float(np.median(wall_e)), "wall_spread_ms": spread(wall_e), "points_ms": ee[0],
         "cells_ms": ee[1]},
    ]
    head = {"points": nP, "triangles": info["nT"], "quadrangles": nQ, "rounds": info["rounds"], "reps": a.reps,
            "status_0_1_2": [int(full["stats"][k]) for k in ("n0", "n1", "n2")]}
    print(json.dumps(head), flush=True)
    for r in rows:
        print(json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in r.items()}), flush=True)
    trk.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Device-resident quadrangle meshes against the host-array chain (tools/bench_mesh.py)\n\n")
            f.write("%d points (jittered lattice, spacing %.2f km, shuffled indices, rmax = 1.5 spacings) as the buoys of a tracker: %d "
                    "triangles, %d quadrangles, %d rounds; status 0 / 1 / 2 after one record: %s.  Alternating passes, medians of %d; "
                    "`wall` = around the Python call, `spread` = max - min of its passes, the other columns = HIP events inside the "
                    "library.  `frac` = the cell kernel's algorithmic bytes (185 B per quadrangle in full, 144 B for the sums alone) "
                    "over its time against 4.8 TB/s.\n\n" % (nP, DKM, info["nT"], nQ, info["rounds"], head["status_0_1_2"], a.reps))
            f.write("| | wall ms | spread ms | device chain ms | points ms | cells ms | final sum ms | frac |\n|" + "---|" * 8 + "\n")
            for r in rows:
                cell = lambda k, fmt="%.3f": (fmt % r[k]) if k in r else ""       # noqa: E731
                f.write("| %s | %.2f | %.2f | %s | %s | %s | %s | %s |\n" % (r["what"], r["wall_ms"], r["wall_spread_ms"], cell("events_ms", "%.2f"),
                                                                          cell("points_ms"), cell("cells_ms"), cell("stats_ms"), cell("cells_frac")))


if __name__ == "__main__":
    main()
