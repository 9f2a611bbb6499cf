#!/usr/bin/env python3
"""Cost of coarse-graining a device-resident quadrangle mesh (sitrk_mesh_coarse) against the path it replaces.

    python tools/bench_coarse.py [--side 3163] [--reps 7] [--scales 1,2,4] [--out TABLE.md]

The cloud of tools/bench_mesh.py -- side x side points on a jittered lattice, spacing 3.11 km, shuffled indices, rmax = 1.5
spacings -- as the buoys of a tracker, one mesh, one record stepped.  For every pixel size d = scale x spacing the grid is
sit.raster_grid over the cloud's bounding box and nlev reaches the 1 x 1 level.  Alternating passes, medians of `reps`:
    (T)   Context.mesh_coarse, the table only: 64 bytes per level come down
    (B)   the same with the pyramid (48 bytes per box)
    (D)   IceTracker.mesh_deform in full, the path a host-side coarse-graining starts from: every rate and status comes down
          (and the gradients it would need are not among them)
Wall clock around the Python call, and HIP events inside the library (sitrk_coarse_kernel_ms: the cells' terms and keys, the
sort, level 0 with its run bounds, the levels above it, the table).  `core` is what the same call spends in the pass over the
buoys and the cell kernel of sitrk_mesh_deform (sitrk_mesh_kernel_ms), which run in front of those phases.  One JSON line per
figure."""
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
from sitrack_amd import synthetic as syn  # noqa: E402
from bench_delaunay import DKM, jittered  # noqa: E402

PHASES = ("terms", "sort", "level0", "pyramid", "table")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scales", default="1,2,4", help="pixel sizes in point spacings")
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
    nQ = trk.mesh(rmax, 0)["nQ"]
    trk.step(0, 0)
    jrec1 = 0
    full = trk.mesh_deform(jrec1)                                               # warm-up: scratch sized, code loaded
    status = full["status"]
    n1 = int((status == 1).sum())
    del full
    grids = {s: sit.raster_grid(yx[:, 0].min(), yx[:, 0].max(), yx[:, 1].min(), yx[:, 1].max(), s * DKM) for s in scales}
    nlevs = {s: int(math.ceil(math.log2(max(grids[s][3], grids[s][4])))) + 1 for s in scales}
    tables = {}
    for s in scales:                                                            # warm-up, and the counts against the statuses
        r = ctx.mesh_coarse(0, jrec1, grids[s], nlevs[s], boxes=True)
        assert r["nin"] + r["nout"] == n1 and r["levels"][0][0].sum() == r["nin"] and r["levels"][-1].shape == (6, 1, 1), "counts differ"
        assert r["levels"][-1][0, 0, 0] == r["nin"], "the top box does not hold every cell"
        tables[s] = r["table"]
        del r
    runs = {(s, k): [] for s in scales for k in ("T", "B")}
    wall_d = []
    for _ in range(a.reps):
        w, _ = timed(lambda: trk.mesh_deform(jrec1))
        wall_d.append(w)
        for s in scales:
            for k in ("T", "B"):
                w, r = timed(lambda: ctx.mesh_coarse(0, jrec1, grids[s], nlevs[s], boxes=(k == "B")))
                assert np.array_equal(r["table"].view(np.uint64), tables[s].view(np.uint64)), "two calls, other bits"
                core = ctx.mesh_kernel_ms(build=False)
                runs[(s, k)].append((w, core[1] + core[2]) + ctx.coarse_kernel_ms())
                del r
    trk.close()

    head = {"points": nP, "quadrangles": nQ, "reps": a.reps, "status_0_1_2": [int((status == k).sum()) for k in range(3)],
            "mesh_deform_full_wall_ms": round(float(np.median(wall_d)), 3), "mesh_deform_bytes_down": 41 * nQ + 80}
    print(json.dumps(head), flush=True)
    rows = []
    for s in scales:
        g = grids[s]
        shapes = ctx.coarse_level_shapes(g[3], g[4], nlevs[s])
        nbox = sum(p * q for p, q in shapes)
        beta = sit.scaling_exponents(tables[s], g[2])["beta"]
        for k in ("T", "B"):
            m = np.median(np.array(runs[(s, k)], dtype=np.float64), axis=0)
            w_all = [x[0] for x in runs[(s, k)]]
            gpu = float(m[2:].sum())
            row = {"scale": s, "d_km": round(s * DKM, 4), "ny": g[3], "nx": g[4], "pixels": g[3] * g[4], "nlev": nlevs[s], "what": k,
                   "wall_ms": float(m[0]), "wall_spread_ms": float(max(w_all) - min(w_all)), "core_ms": float(m[1]),
                   **{p + "_ms": float(x) for p, x in zip(PHASES, m[2:])}, "phases_ms": gpu, "sort_share": float(m[3]) / gpu,
                   "sort_share_with_core": float(m[3]) / (gpu + float(m[1])),
                   "bytes_down": int(64 * nlevs[s] + 24 + (48 * nbox if k == "B" else 0)), "beta": [round(float(b), 4) for b in beta]}
            rows.append(row)
            print(json.dumps({kk: (round(x, 4) if isinstance(x, float) else x) for kk, x in row.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Coarse-graining a device-resident quadrangle mesh (tools/bench_coarse.py)\n\n")
            f.write("%d points (jittered lattice, spacing %.2f km, shuffled indices, rmax = 1.5 spacings) as the buoys of a tracker, %d "
                    "quadrangles, status 0 / 1 / 2 after one record: %s.  Pixels of `scale` point spacings over the cloud's bounding box, "
                    "`nlev` up to the 1 x 1 level.  Alternating passes, medians of %d; `wall` = around the Python call, `spread` = max - min "
                    "of its passes; `core` = the pass over the buoys and the cell kernel of sitrk_mesh_deform inside the same call, the five "
                    "phases = HIP events inside the library; `sort share` = the sort over the five phases (over the phases and `core`).  "
                    "`T` = the table only, `B` = with the pyramid.  `mesh_deform` in full, re-measured in the same passes: %.2f ms wall, %d "
                    "bytes down.\n\n" % (nP, DKM, nQ, head["status_0_1_2"], a.reps, head["mesh_deform_full_wall_ms"], head["mesh_deform_bytes_down"]))
            f.write("| scale | pixels | nlev | what | wall ms | spread ms | core ms | terms ms | sort ms | level 0 ms | pyramid ms | table ms | "
                    "sort share | bytes down | beta(1..3) |\n|" + "---|" * 15 + "\n")
            for r in rows:
                f.write("| %g | %d x %d | %d | %s | %.2f | %.2f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f (%.2f) | %d | %s |\n"
                        % (r["scale"], r["ny"], r["nx"], r["nlev"], r["what"], r["wall_ms"], r["wall_spread_ms"], r["core_ms"], r["terms_ms"],
                           r["sort_ms"], r["level0_ms"], r["pyramid_ms"], r["table_ms"], r["sort_share"], r["sort_share_with_core"],
                           r["bytes_down"], ", ".join("%.3f" % b for b in r["beta"])))


if __name__ == "__main__":
    main()
