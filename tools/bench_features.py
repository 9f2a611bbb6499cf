#!/usr/bin/env python3
"""Cost of labelling the features of a device-resident mesh's deformation map (sitrk_mesh_features) against the path it replaces.

    python tools/bench_features.py [--side 3163] [--reps 7] [--scales 4,2,1,0.5] [--out TABLE.md]
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/bench_features.py --reps 1 --scales 0.5 --device-only

The cloud of tools/bench_mesh.py -- side x side points on a jittered lattice, spacing 3.11 km, shuffled indices, rmax = 1.5
spacings -- as the buoys of a tracker, one mesh, one record stepped.  For every pixel size d = scale x spacing the grid is
sit.raster_grid over the cloud's bounding box; the thresholds are the 85th and the 50th percentile of the total deformation
over the cells with a rate.  Alternating passes, medians of `reps`:
    (F)   Context.mesh_features, the table only: 96 bytes per feature and three counts come down
    (L)   the same with the labels (4 bytes per pixel)
    (H)   the path without it: Context.mesh_raster with owner and fields (44 bytes per pixel come down), the mask made on the host
          from them, and the labelling there: scipy.ndimage.label where scipy can be imported, else the run-based union-find of
          this file on the coarsest grid only.  The host path stops at the labels and the pixel counts; it makes no table.
    (S)   one synthetic mask per size through Context.label_raster: a one-pixel serpentine through every row, one component that
          crosses every tile border
Wall clock around the Python call, and HIP events inside the library (sitrk_features_kernel_ms: mask, labels, table;
sitrk_raster_kernel_ms and sitrk_mesh_kernel_ms for what runs in front of them in the same call).  Every (F) result is checked
against the host labelling of the same pass: the same number of components and active pixels, the same multiset of sizes.  One
JSON line per figure.  --device-only leaves (L) and (H) out: after the warm-up call every pass is (F) at the 85th percentile, (F) at
the 50th and (S), in that order -- the run a kernel trace is taken of, whose dispatches then read in that order."""
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
from bench_delaunay import DKM, jittered  # noqa: E402

try:
    from scipy import ndimage as ndi
except ImportError:
    ndi = None

PHASES = ("mask", "label", "table")
EIGHT = np.ones((3, 3), dtype=np.int32)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def serpentine(ny, nx):
    m = np.zeros((ny, nx), dtype=np.int8)
    m[0::2] = 1
    m[1::4, nx - 1] = 1
    m[3::4, 0] = 1
    return m


def host_sizes(mask):
    """sorted pixel counts of the 8-connected components of a mask on the host: scipy, or a union-find over the row runs"""
    if ndi is not None:
        lab, n = ndi.label(mask, structure=EIGHT)
        return np.sort(np.bincount(lab.ravel(), minlength=n + 1)[1:])
    parent, size = [], []

    def find(r):
        while parent[r] != r:
            parent[r] = parent[parent[r]]
            r = parent[r]
        return r

    above = []
    for row in mask:
        pad = np.concatenate(([False], row, [False]))
        edge = np.flatnonzero(pad[1:] != pad[:-1]).tolist()
        runs, k = [], 0
        for s, e in zip(edge[0::2], edge[1::2]):
            r = len(parent)
            parent.append(r); size.append(e - s)
            while k < len(above) and above[k][1] <= s - 1:
                k += 1
            m = k
            while m < len(above) and above[m][0] < e + 1:
                x, y = find(r), find(above[m][2])
                if x != y:
                    parent[max(x, y)] = min(x, y)
                    size[min(x, y)] += size[max(x, y)]
                m += 1
            runs.append((s, e, r))
        above = runs
    return np.sort(np.array([size[r] for r in range(len(parent)) if parent[r] == r], dtype=np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scales", default="4,2,1,0.5", help="pixel sizes in point spacings")
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    ap.add_argument("--device-only", action="store_true", help="only (F) and (S): the run for a kernel trace")
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
    rated = full["status"] != 0
    tot = np.sqrt(full["div"][rated] ** 2 + full["shr"][rated] ** 2)
    thrs = {q: float(np.percentile(tot, q)) for q in (85, 50)}
    del full, tot
    grids = {s: sit.raster_grid(yx[:, 0].min(), yx[:, 0].max(), yx[:, 1].min(), yx[:, 1].max(), s * DKM) for s in scales}
    host_scales = [s for s in scales if not a.device_only and (ndi is not None or s == max(scales))]
    for s in scales:                                                            # warm-up
        ctx.mesh_features(0, jrec1, grids[s], "tot", thrs[85], labels=True)
    runs = {(s, q, k): [] for s in scales for q in thrs for k in "FLH"}
    serp = {s: [] for s in scales}
    found = {}
    for _ in range(a.reps):
        for s in scales:
            g = grids[s]
            if s in host_scales:
                w_down, r = timed(lambda: ctx.mesh_raster(0, jrec1, g, want=("owner", "fields")))
                ras = ctx.raster_kernel_ms()
                own, fld = r["owner"], r["fields"]
            for q, thr in thrs.items():
                w, f = timed(lambda: ctx.mesh_features(0, jrec1, g, "tot", thr))
                core = ctx.mesh_kernel_ms(build=False)
                runs[(s, q, "F")].append((w, core[1] + core[2], sum(ctx.raster_kernel_ms())) + ctx.features_kernel_ms())
                found[(s, q)] = (f["nfeat"], f["ncomp"], f["nactive"], len(f["table"]))
                if a.device_only:
                    runs[(s, q, "L")].append(runs[(s, q, "F")][-1])
                    continue
                w, fl = timed(lambda: ctx.mesh_features(0, jrec1, g, "tot", thr, labels=True))
                runs[(s, q, "L")].append((w, core[1] + core[2], sum(ctx.raster_kernel_ms())) + ctx.features_kernel_ms())
                assert fl["ncomp"] == f["ncomp"] and np.array_equal(fl["table"], f["table"]), "two calls, other rows"
                del fl
                if s in host_scales:
                    w_mask, mask = timed(lambda: (own >= 0) & (fld[0] * fld[0] + fld[1] * fld[1] >= thr * thr))
                    w_lab, sizes = timed(lambda: host_sizes(mask))
                    runs[(s, q, "H")].append((w_down, w_mask, w_lab, sum(ras)))
                    assert f["nactive"] == int(mask.sum()) and f["ncomp"] == len(sizes), "the host finds other components"
                    if f["nfeat"] <= len(f["table"]):
                        assert np.array_equal(np.sort(f["table"][:, 1]), sizes), "the host finds other sizes"
                    del mask, sizes
            if s in host_scales:
                del own, fld, r
            m = serpentine(g[3], g[4])
            w, f = timed(lambda: ctx.label_raster(m, labels=False))
            assert (f["ncomp"], f["nactive"]) == (1, int(m.sum())) and f["table"][0, 1] == f["nactive"], "the serpentine is not one component"
            serp[s].append((w,) + ctx.features_kernel_ms())
            del m
    trk.close()

    head = {"points": nP, "quadrangles": nQ, "reps": a.reps, "thr_p85": thrs[85], "thr_p50": thrs[50],
            "host_labelling": "scipy.ndimage.label" if ndi is not None else "union-find over row runs (coarsest grid only)"}
    print(json.dumps(head), flush=True)
    rows = []
    for s in scales:
        g = grids[s]
        npix = g[3] * g[4]
        for q in thrs:
            nfeat, ncomp, nact, kept = found[(s, q)]
            row = {"scale": s, "ny": g[3], "nx": g[4], "pixels": npix, "percentile": q, "nfeat": nfeat, "ncomp": ncomp, "nactive": nact}
            for k in "FL":
                m = np.median(np.array(runs[(s, q, k)], dtype=np.float64), axis=0)
                w_all = [x[0] for x in runs[(s, q, k)]]
                row.update({k + "_wall_ms": float(m[0]), k + "_spread_ms": float(max(w_all) - min(w_all)), k + "_core_ms": float(m[1]),
                            k + "_raster_ms": float(m[2]), **{k + "_" + p + "_ms": float(x) for p, x in zip(PHASES, m[3:])}})
            row["F_bytes_down"] = 96 * kept + 24 + 32
            row["L_bytes_down"] = row["F_bytes_down"] + 4 * npix
            if runs[(s, q, "H")]:
                m = np.median(np.array(runs[(s, q, "H")], dtype=np.float64), axis=0)
                row.update({"H_download_wall_ms": float(m[0]), "H_mask_ms": float(m[1]), "H_label_ms": float(m[2]), "H_raster_gpu_ms": float(m[3]),
                            "H_total_ms": float(m[:3].sum()), "H_bytes_down": 44 * npix + 24, "ratio": float(m[:3].sum()) / row["F_wall_ms"]})
            rows.append(row)
            print(json.dumps({kk: (round(x, 4) if isinstance(x, float) else x) for kk, x in row.items()}), flush=True)
    srows = []
    for s in scales:
        g = grids[s]
        m = np.median(np.array(serp[s], dtype=np.float64), axis=0)
        row = {"scale": s, "ny": g[3], "nx": g[4], "pixels": g[3] * g[4], "what": "serpentine", "wall_ms": float(m[0]),
               **{p + "_ms": float(x) for p, x in zip(PHASES, m[1:])}}
        srows.append(row)
        print(json.dumps({kk: (round(x, 4) if isinstance(x, float) else x) for kk, x in row.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Labelling the features of a device-resident mesh's deformation map (tools/bench_features.py)\n\n")
            f.write("%d points (jittered lattice, spacing %.2f km, shuffled indices, rmax = 1.5 spacings) as the buoys of a tracker, %d "
                    "quadrangles, one record stepped.  Pixels of `scale` point spacings over the cloud's bounding box; `tot` thresholds at "
                    "the 85th (%.4e /s) and 50th (%.4e /s) percentile over the cells; conn 8, min_pix 1.  Alternating passes, medians of "
                    "%d.  `F` = sitrk_mesh_features, table only; `L` = with the labels; `wall` around the Python call; `core` = the pass "
                    "over the buoys and the cell kernel of sitrk_mesh_deform, `raster` = the rasteriser's two kernels, then the three phases "
                    "of sitrk_features_kernel_ms, all inside the same call.  `H` = the path without it, in the same passes: mesh_raster "
                    "with owner and fields (wall), the mask on the host, then %s with the pixel counts (no table); `ratio` = H total / F "
                    "wall.\n\n" % (nP, DKM, nQ, thrs[85], thrs[50], a.reps, head["host_labelling"]))
            f.write("| scale | pixels | pct | features | active | F wall ms | spread | core | raster | mask | label | table | F bytes down | "
                    "L wall ms | L bytes down | H download ms | H mask ms | H label ms | H total ms | H bytes down | ratio |\n|" + "---|" * 21 + "\n")
            for r in rows:
                h = ("%.1f | %.1f | %.1f | %.1f | %d | %.1f" % (r["H_download_wall_ms"], r["H_mask_ms"], r["H_label_ms"], r["H_total_ms"],
                                                                r["H_bytes_down"], r["ratio"])) if "ratio" in r else "- | - | - | - | - | -"
                f.write("| %g | %d x %d | %d | %d | %d | %.2f | %.2f | %.3f | %.3f | %.3f | %.3f | %.3f | %d | %.2f | %d | %s |\n"
                        % (r["scale"], r["ny"], r["nx"], r["percentile"], r["nfeat"], r["nactive"], r["F_wall_ms"], r["F_spread_ms"],
                           r["F_core_ms"], r["F_raster_ms"], r["F_mask_ms"], r["F_label_ms"], r["F_table_ms"], r["F_bytes_down"],
                           r["L_wall_ms"], r["L_bytes_down"], h))
            f.write("\nA one-pixel serpentine through every row -- one component across every tile border -- through sitrk_label_raster "
                    "(the mask goes up, `mask` = its upload; table only):\n\n| pixels | wall ms | upload ms | label ms | table ms |\n|---|---|---|---|---|\n")
            for r in srows:
                f.write("| %d x %d | %.2f | %.3f | %.3f | %.3f |\n" % (r["ny"], r["nx"], r["wall_ms"], r["mask_ms"], r["label_ms"], r["table_ms"]))


if __name__ == "__main__":
    main()
