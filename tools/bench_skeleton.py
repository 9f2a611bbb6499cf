#!/usr/bin/env python3
"""Cost of thinning the features of a kept map on the device (sitrk_keep_skeleton) against the route it replaces
-- the download of the map, and a host thinning behind it --, measured in the same passes, and the thinning kernel at other
batch lengths.

    python tools/bench_skeleton.py [--side 3163] [--reps 7] [--scales 4,2,1,0.5] [--batches 1,4,7,8] [--host-thin-pixels 3000000] [--out TABLE.md]

The cloud of tools/bench_mesh.py -- side x side points on a jittered lattice, spacing 3.11 km, shuffled indices, rmax = 1.5
spacings -- as the buoys of a tracker, one window of one record.  For every pixel size d = scale x spacing the grid is
sit.raster_grid over the cloud's bounding box; the thresholds are the 85th and the 50th percentile of the total deformation over
the cells with a rate; conn 8, min_pix 1.  One kept map per size and threshold (sitrk_mesh_features_keep), made once.
Alternating passes over sizes, thresholds and routes, medians of `reps` with the extremes:
    (D)   keep_skeleton, table and nodes only, at every batch length of --batches (the knob skeleton_batch; the shipped one is
          the library's default): wall clock, the three phases from HIP events, nsub, launches of the thinning kernel, bytes down
    (H)   keep_get of the map: the download, 4 bytes per pixel; and on rasters of at most --host-thin-pixels pixels the numpy
          thinning of this file behind it, once per size and threshold (its inputs are the same in every pass)
Every (D) pass is checked against the other batch lengths of the same case and, where the host thinning ran, against its table
of skeleton pixels per label.  One JSON line per figure."""
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


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def host_thin(mask, max_sub=4096):
    """Guo and Hall's two sub-iterations as include/sitrk.h states them, in numpy over shifted views; (K, nsub)"""
    S = (np.asarray(mask) != 0).astype(np.uint8)
    ny, nx = S.shape
    nsub = quiet = 0
    for k in range(max_sub):
        P = np.zeros((ny + 2, nx + 2), dtype=np.uint8)
        P[1:-1, 1:-1] = S
        v = lambda dj, di: P[1 + dj:1 + dj + ny, 1 + di:1 + di + nx]
        p2, p3, p4, p5, p6, p7, p8, p9 = v(-1, 0), v(-1, 1), v(0, 1), v(1, 1), v(1, 0), v(1, -1), v(0, -1), v(-1, -1)
        C = ((1 - p2) & (p3 | p4)) + ((1 - p4) & (p5 | p6)) + ((1 - p6) & (p7 | p8)) + ((1 - p8) & (p9 | p2))
        N = np.minimum((p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8), (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9))
        m = ((p6 | p7 | (1 - p9)) & p8) if k % 2 == 0 else ((p2 | p3 | (1 - p5)) & p4)
        gone = (S == 1) & (C == 1) & (N >= 2) & (N <= 3) & (m == 0)
        if gone.any():
            S = np.where(gone, 0, S).astype(np.uint8)
            nsub, quiet = k + 1, 0
        else:
            quiet += 1
            if quiet == 2:
                break
    return S, nsub


def launches_of(nsub, batch, max_sub=4096):
    """launches of the thinning kernel for a thinning of nsub sub-iterations: batches until two quiet sub-iterations were seen"""
    done = n = 0
    while done < max_sub and done < nsub + 2:
        done += min(batch, max_sub - done)
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scales", default="4,2,1,0.5", help="pixel sizes in point spacings")
    ap.add_argument("--batches", default="1,4,7,8", help="values of the knob skeleton_batch; the last is taken as the shipped one")
    ap.add_argument("--host-thin-pixels", type=int, default=3000000, help="largest raster the numpy thinning is run on")
    ap.add_argument("--maxfeat", type=int, default=1 << 22)
    ap.add_argument("--maxnode", type=int, default=1 << 24)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    a = ap.parse_args()
    scales = [float(s) for s in a.scales.split(",")]
    batches = [int(b) for b in a.batches.split(",")]
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
    nQ = trk.mesh(rmax, 0, slot=0)["nQ"]
    trk.step(0, 0)
    full = trk.mesh_deform(0, slot=0)
    rated = full["status"] != 0
    tot = np.sqrt(full["div"][rated] ** 2 + full["shr"][rated] ** 2)
    thrs = {q: float(np.percentile(tot, q)) for q in (85, 50)}
    del full, tot
    grids = {s: sit.raster_grid(yx[:, 0].min(), yx[:, 0].max(), yx[:, 1].min(), yx[:, 1].max(), s * DKM) for s in scales}
    cases = [(s, q) for s in scales for q in thrs]
    assert len(cases) <= sit._lib.KEEP_MAX, "one kept map per size and threshold"
    slot = {c: k for k, c in enumerate(cases)}
    print(json.dumps({"points": nP, "quadrangles": nQ, "reps": a.reps, "thr_p85": thrs[85], "thr_p50": thrs[50], "batches": batches}), flush=True)

    feats = {}
    for s, q in cases:
        f = ctx.mesh_features_keep(slot[(s, q)], 0, 0, grids[s], "tot", thrs[q])
        feats[(s, q)] = (f["nfeat"], f["nactive"])
        for b in batches:                                                      # warm-up: scratch sized, code loaded
            ctx.set_tuning(skeleton_batch=b)
            ctx.keep_skeleton(slot[(s, q)], maxfeat=a.maxfeat, maxnode=a.maxnode)
    D = {(c, b): [] for c in cases for b in batches}
    H = {c: [] for c in cases}
    host, first = {}, {}
    for rep in range(a.reps):
        for c in cases:
            for b in batches:
                ctx.set_tuning(skeleton_batch=b)
                w, r = timed(lambda: ctx.keep_skeleton(slot[c], maxfeat=a.maxfeat, maxnode=a.maxnode))
                assert r["converged"] == 1 and r["nnode"] <= a.maxnode and r["nfeat"] <= a.maxfeat, "--maxfeat or --maxnode is too small, or the thinning did not end"
                D[(c, b)].append((w,) + ctx.skeleton_kernel_ms())
                ref = first.setdefault(c, r)
                assert np.array_equal(ref["table"], r["table"]) and np.array_equal(ref["nodes"], r["nodes"]) and ref["nsub"] == r["nsub"], "the batch length changed a result"
            w_get, k = timed(lambda: ctx.keep_get(slot[c])["labels"])
            H[c].append(w_get)
            g = grids[c[0]]
            if g[3] * g[4] <= a.host_thin_pixels and c not in host:
                w_thin, (K, nsub) = timed(lambda: host_thin(k >= 0))
                host[c] = w_thin
                vals, cnt = np.unique(k[K == 1], return_counts=True)
                t = first[c]["table"]
                have = t[t[:, 2] > 0]
                same = nsub == first[c]["nsub"] and np.array_equal(have[:, 0], vals) and np.array_equal(have[:, 2], cnt)
                if not same:
                    print(json.dumps({"case": c, "host_nsub": nsub, "nsub": first[c]["nsub"], "host_nskel": int(K.sum()), "nskel": first[c]["nskel"],
                                      "host_labels": len(vals), "labels": len(have), "nfeat": first[c]["nfeat"]}), flush=True)
                assert same, "the host thins to another skeleton"
            del k
        print(json.dumps({"pass": rep}), flush=True)
    trk.close()

    rows = []
    for c in cases:
        s, q = c
        g = grids[s]
        r0 = first[c]
        row = {"scale": s, "ny": g[3], "nx": g[4], "pixels": g[3] * g[4], "percentile": q, "nfeat": feats[c][0], "nactive": feats[c][1],
               "nskel": r0["nskel"], "nnode": r0["nnode"], "nsub": r0["nsub"], "bytes_down": 56 * len(r0["table"]) + 24 * len(r0["nodes"]) + 32,
               "get_ms": float(np.median(H[c])), "get_min_ms": float(min(H[c])), "get_max_ms": float(max(H[c])), "get_bytes_down": 4 * g[3] * g[4],
               "host_thin_ms": host.get(c)}
        for b in batches:
            m = np.array(D[(c, b)], dtype=np.float64)
            md = np.median(m, axis=0)
            row.update({"b%d_wall_ms" % b: float(md[0]), "b%d_wall_min_ms" % b: float(m[:, 0].min()), "b%d_wall_max_ms" % b: float(m[:, 0].max()),
                        "b%d_thin_ms" % b: float(md[1]), "b%d_table_ms" % b: float(md[2]), "b%d_nodes_ms" % b: float(md[3]),
                        "b%d_launches" % b: launches_of(r0["nsub"], b)})
        rows.append(row)
        print(json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in row.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Thinning the features of a kept map on the device (tools/bench_skeleton.py)\n\n")
            f.write("%d points (jittered lattice, spacing %.2f km, shuffled indices, rmax = 1.5 spacings) as the buoys of a tracker, one window "
                    "on a mesh of %d quadrangles over record 0.  Pixels of `scale` point spacings over the cloud's bounding box; `tot` thresholds "
                    "at the 85th (%.4e /s) and 50th (%.4e /s) percentile; conn 8, min_pix 1; one kept map per size and threshold.  Alternating "
                    "passes, medians of %d with the extremes; `wall` around the Python call, the phases from HIP events inside the library.\n\n"
                    % (nP, DKM, nQ, thrs[85], thrs[50], a.reps))
            f.write("`keep_skeleton`: table and nodes only, at each value of the knob `skeleton_batch` (B sub-iterations per launch of the "
                    "thinning kernel).  The route it replaces: `keep_get` of the map (4 bytes per pixel down) and a numpy thinning behind it, "
                    "run once per case on the rasters of at most %d pixels.  Every pass: all batch lengths give the same table, nodes and nsub; "
                    "where the host thinning ran, its skeleton pixels per label are the table's.\n\n" % a.host_thin_pixels)
            f.write("| scale | pixels | pct | features | labelled pixels | skeleton pixels | nodes | nsub | bytes down | "
                    + " | ".join("B=%d wall ms (min .. max) | thin | table | nodes | launches" % b for b in batches)
                    + " | keep_get ms (min .. max) | its bytes down | numpy thinning ms |\n|" + "---|" * (12 + 5 * len(batches)) + "\n")
            for r in rows:
                f.write("| %g | %d x %d | %d | %d | %d | %d | %d | %d | %d | " % (r["scale"], r["ny"], r["nx"], r["percentile"], r["nfeat"], r["nactive"],
                                                                              r["nskel"], r["nnode"], r["nsub"], r["bytes_down"])
                        + " | ".join("%.2f (%.2f .. %.2f) | %.3f | %.3f | %.3f | %d" % tuple(r["b%d_%s" % (b, n)] for n in
                                     ("wall_ms", "wall_min_ms", "wall_max_ms", "thin_ms", "table_ms", "nodes_ms", "launches")) for b in batches)
                        + " | %.2f (%.2f .. %.2f) | %d | %s |\n" % (r["get_ms"], r["get_min_ms"], r["get_max_ms"], r["get_bytes_down"],
                                                                   "%.0f" % r["host_thin_ms"] if r["host_thin_ms"] is not None else "not run"))


if __name__ == "__main__":
    main()
