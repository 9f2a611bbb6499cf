#!/usr/bin/env python3
"""Cost of linking the features of two windows on the device (sitrk_mesh_features_keep, sitrk_mesh_features_advect,
sitrk_features_match) against the host path it replaces, measured in the same passes.

    python tools/bench_track.py [--side 3163] [--reps 7] [--scales 4,2,1,0.5] [--host-reach-pixels 3000000] [--out TABLE.md]

The cloud of tools/bench_mesh.py -- side x side points on a jittered lattice, spacing 3.11 km, shuffled indices, rmax = 1.5
spacings -- as the buoys of a tracker.  Two windows of one record each: mesh 0 is built in front of record 0, mesh 1 in front of
record 1.  For every pixel size d = scale x spacing the grid is sit.raster_grid over the cloud's bounding box; the thresholds are
the 85th and the 50th percentile of the total deformation of window 0 over the cells with a rate; conn 8, min_pix 1.
Behind record 0, alternating passes over sizes and thresholds, medians of `reps`:
    (DA)  mesh_features_keep of window 0 (table only) and mesh_features_advect: 96 bytes per feature, five counts come down
    (HA)  the host path: mesh_raster owners at t0 and t1, mesh_features(labels=True), cellfeat / M in numpy (features.advect_labels)
Behind record 1, the carried maps of (DA) still in their slots:
    (DB)  mesh_features_keep of window 1 (table only) and features_match at reach 0, 1 and 2: 24 bytes per pair come down
    (HB)  the host path at reach 0: mesh_features(labels=True) of window 1 and np.unique over the pixels where both maps have a label
Every (DA) pass is checked against the map of (HA) of the same pass, every (DB) pass at reach 0 against the pairs of (HB) of the
same pass.  At reach 1 and 2 the host restatement (np.unique over up to 25 shifted copies) is computed once per size and threshold
-- the inputs of every pass are the same -- on the rasters of at most --host-reach-pixels pixels, and every pass is checked
against it; above that size the passes are checked against each other and against reach 0, which they must contain.  Wall clock
around the Python calls and HIP events inside the library.  One JSON line per figure."""
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
from sitrack_amd import features as ft  # noqa: E402
from sitrack_amd import synthetic as syn  # noqa: E402
from bench_delaunay import DKM, jittered  # noqa: E402

REACHES = (0, 1, 2)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def host_overlap(A, B):
    """rows (a, b, count) of the pixels where both maps have a label, ascending"""
    both = (A >= 0) & (B >= 0)
    key, cnt = np.unique(A[both].astype(np.int64) * A.size + B[both], return_counts=True)
    return np.stack([key // A.size, key % A.size, cnt], axis=1), int(both.sum())


def host_match(A, B, reach):
    """the contract of sitrk_features_match at shift (0, 0), in numpy"""
    ny, nx = A.shape
    jj, ii = np.nonzero(A >= 0)
    keys = []
    for s in range(-reach, reach + 1):
        for t in range(-reach, reach + 1):
            j, i = jj + s, ii + t
            ok = (j >= 0) & (j < ny) & (i >= 0) & (i < nx)
            b = B[j[ok], i[ok]].astype(np.int64)
            keys.append(((jj[ok] * nx + ii[ok]) * A.size + b)[b >= 0])
    pb = np.unique(np.concatenate(keys))
    p, b = pb // A.size, pb % A.size
    key, cnt = np.unique(A.ravel()[p].astype(np.int64) * A.size + b, return_counts=True)
    return np.stack([key // A.size, key % A.size, cnt], axis=1), len(np.unique(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scales", default="4,2,1,0.5", help="pixel sizes in point spacings")
    ap.add_argument("--host-reach-pixels", type=int, default=3000000, help="largest raster the host restatement at reach 1 and 2 is made on")
    ap.add_argument("--maxpair", type=int, default=1 << 24)
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
    nQ0 = trk.mesh(rmax, 0, slot=0)["nQ"]
    trk.step(0, 0)
    full = trk.mesh_deform(0, slot=0)                                           # warm-up: scratch sized, code loaded
    rated = full["status"] != 0
    tot = np.sqrt(full["div"][rated] ** 2 + full["shr"][rated] ** 2)
    thrs = {q: float(np.percentile(tot, q)) for q in (85, 50)}
    del full, tot
    grids = {s: sit.raster_grid(yx[:, 0].min(), yx[:, 0].max(), yx[:, 1].min(), yx[:, 1].max(), s * DKM) for s in scales}
    cases = [(s, q) for s in scales for q in thrs]
    assert len(cases) + 2 <= sit._lib.KEEP_MAX, "one kept map per size and threshold, and two more"
    slotP = {c: k for k, c in enumerate(cases)}                                 # the carried maps of window 0
    slot0, slotF = len(cases), len(cases) + 1                                   # the map of window 0 and of window 1 of the case at hand
    print(json.dumps({"points": nP, "quadrangles": nQ0, "reps": a.reps, "thr_p85": thrs[85], "thr_p50": thrs[50]}), flush=True)

    # ---- behind record 0: keep and advect, and the host path to the same map
    A = {c: [] for c in cases}
    carried, found = {}, {}
    for s, q in cases:                                                          # warm-up
        ctx.mesh_features_keep(slot0, 0, 0, grids[s], "tot", thrs[q])
        ctx.mesh_features_advect(slot0, slotP[(s, q)], 0, 0, grids[s])
    for rep in range(a.reps):
        for s, q in cases:
            g, thr, P = grids[s], thrs[q], slotP[(s, q)]
            w_keep, f = timed(lambda: ctx.mesh_features_keep(slot0, 0, 0, g, "tot", thr))
            keep_ev = sum(ctx.features_kernel_ms()) + sum(ctx.raster_kernel_ms())
            w_adv, (ncells, ncarried) = timed(lambda: ctx.mesh_features_advect(slot0, P, 0, 0, g))
            adv_ev = ctx.advect_kernel_ms()
            w_own, (o0, o1) = timed(lambda: (ctx.mesh_raster(0, 0, g, at_t1=False, want=("owner",))["owner"],
                                             ctx.mesh_raster(0, 0, g, at_t1=True, want=("owner",))["owner"]))
            w_lab, fl = timed(lambda: ctx.mesh_features(0, 0, g, "tot", thr, labels=True))
            w_np, (M, cellfeat) = timed(lambda: ft.advect_labels(fl["labels"], o0, o1, nQ0))
            assert np.array_equal(fl["table"], f["table"]), "keep returns another table"
            assert np.array_equal(ctx.keep_get(P)["labels"], M), "the device carries another map"
            assert (ncells, ncarried) == (int((cellfeat >= 0).sum()), int((M >= 0).sum())), "other counts"
            A[(s, q)].append((w_keep, w_adv, keep_ev, adv_ev, w_own, w_lab, w_np))
            carried[(s, q)] = M
            found[(s, q)] = (f["nfeat"], len(f["table"]), ncells, ncarried)
            del o0, o1, fl, cellfeat
        print(json.dumps({"behind_record": 0, "pass": rep}), flush=True)

    # ---- behind record 1: window 1 on a mesh of its own, and the match with what window 0 carried here
    nQ1 = trk.mesh(rmax, 1, slot=1)["nQ"]
    trk.step(1, 0)
    B = {(c, r): [] for c in cases for r in REACHES}
    HB = {c: [] for c in cases}
    want, pairs_of = {}, {}
    for s, q in cases:                                                          # warm-up
        ctx.mesh_features_keep(slotF, 1, 1, grids[s], "tot", thrs[q])
        for r in REACHES:
            ctx.features_match(slotP[(s, q)], slotF, reach=r, maxpair=a.maxpair)
    for rep in range(a.reps):
        for s, q in cases:
            g, thr, P, M = grids[s], thrs[q], slotP[(s, q)], carried[(s, q)]
            w_keep, f = timed(lambda: ctx.mesh_features_keep(slotF, 1, 1, g, "tot", thr))
            keep_ev = sum(ctx.features_kernel_ms()) + sum(ctx.raster_kernel_ms())
            got = {}
            for r in REACHES:
                w, m = timed(lambda: ctx.features_match(P, slotF, reach=r, maxpair=a.maxpair))
                assert m["npair"] <= a.maxpair, "--maxpair is too small for this table"
                B[((s, q), r)].append((w,) + ctx.match_kernel_ms())
                got[r] = m
            w_lab, fl = timed(lambda: ctx.mesh_features(1, 1, g, "tot", thr, labels=True))
            w_np, (pairs, nhit) = timed(lambda: host_overlap(M, fl["labels"]))
            HB[(s, q)].append((w_keep, w_lab, w_np, keep_ev))
            assert np.array_equal(got[0]["pairs"], pairs) and got[0]["nhit"] == nhit, "the device finds another overlap"
            if g[3] * g[4] <= a.host_reach_pixels and (s, q) not in want:
                want[(s, q)] = {r: host_match(M, fl["labels"], r) for r in (1, 2)}
            for r in (1, 2):
                if (s, q) in want:
                    assert np.array_equal(got[r]["pairs"], want[(s, q)][r][0]) and got[r]["nhit"] == want[(s, q)][r][1], "reach %d: other pairs" % r
                prev = pairs_of.setdefault(((s, q), r), got[r]["pairs"])
                assert np.array_equal(prev, got[r]["pairs"]), "two passes, other pairs"
                k0 = got[r - 1]["pairs"][:, 0] * M.size + got[r - 1]["pairs"][:, 1]
                assert np.isin(k0, got[r]["pairs"][:, 0] * M.size + got[r]["pairs"][:, 1]).all() and got[r]["nhit"] >= got[r - 1]["nhit"]
            pairs_of[((s, q), 0)] = got[0]["pairs"]
            del fl
        print(json.dumps({"behind_record": 1, "pass": rep}), flush=True)
    trk.close()

    rows = []
    for s, q in cases:
        g = grids[s]
        npix = g[3] * g[4]
        ma = np.median(np.array(A[(s, q)], dtype=np.float64), axis=0)
        mh = np.median(np.array(HB[(s, q)], dtype=np.float64), axis=0)
        nfeat, kept, ncells, ncarried = found[(s, q)]
        row = {"scale": s, "ny": g[3], "nx": g[4], "pixels": npix, "percentile": q, "nfeat": nfeat, "ncells": ncells, "ncarried": ncarried,
               "DA_keep_wall_ms": float(ma[0]), "DA_advect_wall_ms": float(ma[1]), "DA_keep_gpu_ms": float(ma[2]), "DA_advect_gpu_ms": float(ma[3]),
               "DA_bytes_down": 96 * kept + 24 + 16, "HA_owners_ms": float(ma[4]), "HA_labels_ms": float(ma[5]), "HA_numpy_ms": float(ma[6]),
               "HA_total_ms": float(ma[4:7].sum()), "HA_bytes_down": 12 * npix, "DB_keep_wall_ms": float(mh[0]), "DB_keep_wall_min_ms": float(min(x[0] for x in HB[(s, q)])),
               "DB_keep_wall_max_ms": float(max(x[0] for x in HB[(s, q)])), "DB_keep_gpu_ms": float(mh[3]), "HB_labels_ms": float(mh[1]),
               "HB_numpy_ms": float(mh[2]), "HB_total_ms": float(mh[1:3].sum()), "HB_bytes_down": 4 * npix,
               "host_checked_reach": [0] + ([1, 2] if (s, q) in want else [])}
        for r in REACHES:
            mb = np.median(np.array(B[((s, q), r)], dtype=np.float64), axis=0)
            npair = len(pairs_of[((s, q), r)])
            row.update({"r%d_wall_ms" % r: float(mb[0]), "r%d_emit_ms" % r: float(mb[1]), "r%d_sort_ms" % r: float(mb[2]),
                        "r%d_rows_ms" % r: float(mb[3]), "r%d_npair" % r: npair, "r%d_bytes_down" % r: 24 * npair + 16})
        rows.append(row)
        print(json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in row.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Linking the features of two windows on the device (tools/bench_track.py)\n\n")
            f.write("%d points (jittered lattice, spacing %.2f km, shuffled indices, rmax = 1.5 spacings) as the buoys of a tracker; window 0 "
                    "on a mesh of %d quadrangles over record 0, window 1 on a mesh of %d over record 1.  Pixels of `scale` point spacings "
                    "over the cloud's bounding box; `tot` thresholds at the 85th (%.4e /s) and 50th (%.4e /s) percentile of window 0; conn 8, "
                    "min_pix 1.  Alternating passes, medians of %d; `wall` around the Python call, `gpu` from HIP events inside the "
                    "library.\n\n" % (nP, DKM, nQ0, nQ1, thrs[85], thrs[50], a.reps))
            f.write("## Behind window 0: keep and carry\n\n`keep` = sitrk_mesh_features_keep, table only (gpu: rasteriser, mask, labels, table); "
                    "`advect` = sitrk_mesh_features_advect (gpu: its kernels behind the two rasters).  Host path in the same pass: the owners "
                    "at t0 and t1 (sitrk_mesh_raster twice), the labels (sitrk_mesh_features with labels), cellfeat / M in numpy.  Every "
                    "pass: the device's map equals the host's.\n\n")
            f.write("| scale | pixels | pct | features | cells carrying | pixels carried | keep wall ms | keep gpu ms | advect wall ms | advect gpu ms | "
                    "bytes down | host owners ms | host labels ms | host numpy ms | host total ms | host bytes down |\n|" + "---|" * 16 + "\n")
            for r in rows:
                f.write("| %g | %d x %d | %d | %d | %d | %d | %.2f | %.3f | %.2f | %.3f | %d | %.1f | %.1f | %.1f | %.1f | %d |\n"
                        % (r["scale"], r["ny"], r["nx"], r["percentile"], r["nfeat"], r["ncells"], r["ncarried"], r["DA_keep_wall_ms"],
                           r["DA_keep_gpu_ms"], r["DA_advect_wall_ms"], r["DA_advect_gpu_ms"], r["DA_bytes_down"], r["HA_owners_ms"],
                           r["HA_labels_ms"], r["HA_numpy_ms"], r["HA_total_ms"], r["HA_bytes_down"]))
            f.write("\n## Behind window 1: match\n\nsitrk_features_match of the carried map against window 1's kept map (its keep call: `keep wall`, median and extremes, and `keep gpu`: rasteriser, mask, labels, table), "
                    "per reach: wall, then the three phases from events -- keys (counts, scan, emission), sort, rows.  Host path in the same "
                    "pass, reach 0 only: the labels of window 1 come down and np.unique runs over the pixels where both maps have a label.  "
                    "Every pass at reach 0 equals the host's pairs of that pass; `host check` lists the reaches whose passes were held to a "
                    "numpy restatement.\n\n")
            f.write("| scale | pixels | pct | keep wall ms (min .. max) | keep gpu ms | " + " | ".join("r%d wall ms | r%d keys | r%d sort | r%d rows | r%d pairs" % ((r,) * 5) for r in REACHES)
                    + " | r0 bytes down | host labels ms | host unique ms | host total ms | host bytes down | host check |\n|" + "---|" * 26 + "\n")
            for r in rows:
                f.write("| %g | %d x %d | %d | %.2f (%.2f .. %.2f) | %.3f | " % (r["scale"], r["ny"], r["nx"], r["percentile"], r["DB_keep_wall_ms"],
                                                                         r["DB_keep_wall_min_ms"], r["DB_keep_wall_max_ms"], r["DB_keep_gpu_ms"])
                        + " | ".join("%.2f | %.3f | %.3f | %.3f | %d" % tuple(r["r%d_%s" % (k, n)] for n in ("wall_ms", "emit_ms", "sort_ms", "rows_ms", "npair"))
                                     for k in REACHES)
                        + " | %d | %.1f | %.1f | %.1f | %d | %s |\n" % (r["r0_bytes_down"], r["HB_labels_ms"], r["HB_numpy_ms"], r["HB_total_ms"],
                                                                       r["HB_bytes_down"], ",".join(str(x) for x in r["host_checked_reach"])))


if __name__ == "__main__":
    main()
