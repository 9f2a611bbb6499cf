#!/usr/bin/env python3
"""Cost of rasterising a device-resident quadrangle mesh (sitrk_mesh_raster) against the path it replaces.

    python tools/bench_raster.py [--side 3163] [--reps 7] [--scales 0.5,1,2,4] [--out TABLE.md]

The cloud of tools/bench_mesh.py -- side x side points on a jittered lattice, spacing 3.11 km, shuffled indices, rmax = 1.5
spacings -- as the buoys of a tracker, one mesh, one record stepped.  For every pixel size d = scale x spacing the grid is
sit.raster_grid over the cloud's bounding box.  Alternating passes, medians of `reps`:
    (t0)  Context.mesh_raster, owner only, cells at their t0 positions (the mesh's contiguous 64-byte blocks)
    (t1)  the same at the current positions (four 16-byte gathers per cell)
    (t0F) owner and the five maps
    (D)   IceTracker.mesh_deform in full, the path a host-side rasteriser starts from: every rate and status comes down
Wall clock around the Python call, and HIP events inside the library (sitrk_raster_kernel_ms: the fill with the cell kernel, the
gather kernel).  Algorithmic bytes: cell kernel 4 B per pixel (fill) + 16 + 64 B per cell at t0, 16 + 4 * 16 + 1 B at t1; gather
kernel 4 B per pixel for the owner alone, 4 + 40 B with the maps; against 0.6 x 8 TB/s = 4.8 TB/s.  One more pass per d under the
knob raster_count gives the centres that passed the inside test (claims), one atomic each; the lane imbalance of
the one-cell-per-lane mapping -- 64 x the largest pixel box of a wave over the sum of its boxes -- is computed on the host from the
t0 positions with the kernel's own box arithmetic.  One JSON line per figure."""
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

B_CELL_T0, B_CELL_T1, B_FILL, B_GATHER_OWNER, B_GATHER_MAPS = 80., 81., 4., 4., 44.


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def box_pixels(P, grid):
    """pixels in the widened, clipped box of every cell P (nC,4,2): the trip count of its lane"""
    y0, x0, d, ny, nx = grid
    n = []
    for ax, o, m in ((0, y0, ny), (1, x0, nx)):
        lo, hi = P[:, :, ax].min(axis=1), P[:, :, ax].max(axis=1)
        f0 = np.maximum(np.ceil((lo - o) / d - 0.5) - 1., 0.)
        f1 = np.minimum(np.floor((hi - o) / d - 0.5) + 1., m - 1.)
        n.append(np.maximum(f1 - f0 + 1., 0.))
    return n[0] * n[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scales", default="0.5,1,2,4", help="pixel sizes in point spacings")
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    scales = [float(s) for s in a.scales.split(",")]
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
    info = trk.mesh(rmax, 0)
    nQ = info["nQ"]
    P0 = yx[trk.mesh_cells()]                                                   # t0 geometry, for the imbalance figure only
    trk.step(0, 0)
    jrec1 = 0
    full = trk.mesh_deform(jrec1)                                               # warm-up: scratch sized, code loaded
    status = full["status"]
    grids = {s: sit.raster_grid(yx[:, 0].min(), yx[:, 0].max(), yx[:, 1].min(), yx[:, 1].max(), s * DKM) for s in scales}
    for s in scales:                                                            # warm-up, and the maps against the rates
        r = trk.mesh_raster(jrec1, grids[s], at="t0")
        own = r["owner"] >= 0
        assert (status[r["owner"][own]] != 0).all() and np.array_equal(r["div"][own], full["div"][r["owner"][own]]), "maps differ from the rates"
        del r
    runs = {(s, k): [] for s in scales for k in ("t0", "t1", "t0F")}
    wall_d = []
    for _ in range(a.reps):
        w, _ = timed(lambda: trk.mesh_deform(jrec1))
        wall_d.append(w)
        for s in scales:
            for k, kw in (("t0", {"at_t1": False, "want": "owner"}), ("t1", {"at_t1": True, "want": "owner"}),
                          ("t0F", {"at_t1": False, "want": ("owner", "fields")})):
                w, r = timed(lambda: ctx.mesh_raster(0, jrec1, grids[s], **kw))
                runs[(s, k)].append((w,) + ctx.raster_kernel_ms() + (r["nowned"],))
                del r
    ctx.set_tuning(raster_count=1)
    counts = {}
    for s in scales:
        for k, at_t1 in (("t0", False), ("t1", True)):
            r = ctx.mesh_raster(0, jrec1, grids[s], at_t1=at_t1, want="owner")
            counts[(s, k)] = (ctx.raster_stats(), r["nowned"])
    ctx.set_tuning(raster_count=0)
    trk.close()

    head = {"points": nP, "quadrangles": nQ, "reps": a.reps, "status_0_1_2": [int((status == k).sum()) for k in range(3)],
            "mesh_deform_full_wall_ms": round(float(np.median(wall_d)), 3), "mesh_deform_bytes_down": 41 * nQ + 80}
    print(json.dumps(head), flush=True)
    rows = []
    for s in scales:
        g = grids[s]
        npix = g[3] * g[4]
        bp = box_pixels(P0, g)
        nw = len(bp) // 64
        per_wave = bp[:nw * 64].reshape(nw, 64)
        imbalance = float(64. * per_wave.max(axis=1).sum() / max(per_wave.sum(), 1.))
        for k in ("t0", "t1", "t0F"):
            m = np.median(np.array(runs[(s, k)], dtype=np.float64), axis=0)
            w_all = [x[0] for x in runs[(s, k)]]
            b_cells = B_FILL * npix + (B_CELL_T1 if k == "t1" else B_CELL_T0) * nQ
            b_gather = (B_GATHER_MAPS if k == "t0F" else B_GATHER_OWNER) * npix
            row = {"scale": s, "d_km": round(s * DKM, 4), "ny": g[3], "nx": g[4], "pixels": npix, "what": k, "wall_ms": float(m[0]),
                   "wall_spread_ms": float(max(w_all) - min(w_all)), "cells_ms": float(m[1]), "gather_ms": float(m[2]),
                   "cells_frac": b_cells / (m[1] * 1e-3) / HBM_BOUND, "gather_frac": b_gather / (m[2] * 1e-3) / HBM_BOUND,
                   "owned": int(m[3]), "bytes_down": int((44 if k == "t0F" else 4) * npix + 32),
                   "box_pixels_per_cell": float(bp.mean()), "wave_imbalance": imbalance}
            if (s, k) in counts:
                claims, owned = counts[(s, k)]
                row.update(claims=claims, claims_per_owned=claims / max(owned, 1))
            rows.append(row)
            print(json.dumps({kk: (round(x, 4) if isinstance(x, float) else x) for kk, x in row.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Rasterising a device-resident quadrangle mesh (tools/bench_raster.py)\n\n")
            f.write("%d points (jittered lattice, spacing %.2f km, shuffled indices, rmax = 1.5 spacings) as the buoys of a tracker, %d "
                    "quadrangles, status 0 / 1 / 2 after one record: %s.  Pixels of `scale` point spacings over the cloud's bounding box.  "
                    "Alternating passes, medians of %d; `wall` = around the Python call, `spread` = max - min of its passes, `cells` (the fill "
                    "with the cell kernel) and `gather` = HIP events inside the library, `frac` = algorithmic bytes over time against 4.8 "
                    "TB/s.  `t0` / `t1` = owner only at the stored / current positions, `t0F` = owner and the five maps.  "
                    "`mesh_deform` in full, re-measured in the same passes: %.2f ms wall, %d bytes down.\n\n"
                    % (nP, DKM, nQ, head["status_0_1_2"], a.reps, head["mesh_deform_full_wall_ms"], head["mesh_deform_bytes_down"]))
            f.write("| scale | pixels | what | wall ms | spread ms | cells ms | frac | gather ms | frac | MB down | owned | box px / cell | "
                    "wave imbalance | claims / owned |\n|" + "---|" * 14 + "\n")
            for r in rows:
                f.write("| %g | %d x %d | %s | %.2f | %.2f | %.3f | %.3f | %.3f | %.3f | %.1f | %d | %.2f | %.2f | %s |\n"
                        % (r["scale"], r["ny"], r["nx"], r["what"], r["wall_ms"], r["wall_spread_ms"], r["cells_ms"], r["cells_frac"],
                           r["gather_ms"], r["gather_frac"], r["bytes_down"] / 1e6, r["owned"], r["box_pixels_per_cell"], r["wave_imbalance"],
                           ("%.3f" % r["claims_per_owned"]) if "claims" in r else ""))


if __name__ == "__main__":
    main()
