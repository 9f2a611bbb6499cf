#!/usr/bin/env python3
"""Time `sitrk_cancel_too_close` (overlap cleaning of a tracked cloud, CancelTooClose) on clouds of 1e7 buoys and more.

    python tools/bench_cancel_too_close.py [--grid 4096] [--dkm 1.5] [--prefix 3000]
Clouds: (1) the T-seeds of `sitrk_nemo_seed` on a 4096 x 4096 polar mesh at 1.5 km, at rd = 6 km, where every buoy is close to
another (the scan's worst case); (2) 1e7 of those seeds of which 2 % are moved next to another buoy (within ~50 m), at rd = 1 km,
so that a few percent are close.  Counts of valid records are random (1..10, fewer before krec).  Per case: wall ms of the call
(host arrays in and out), the same less the host->device copies of its input timed alone, wall ms of `sitrk_nearest_buoy`
(stage 1 and the copies of its n results), stage-1 ms (that, less its copies), the close count, and `stages23_ms`: the
cleaning's wall less the probe's (stage 1 is the same work in both), plus the probe's result copies -- the compaction, its
copy back and the host scan.  For scale, the reference restated in numpy (one Haversine row per buoy, then the sequential
scan, as util.py:520-565 does) on the first `--prefix` buoys of cloud 1, and the GPU on the same prefix.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sitrack_amd as sit                      # noqa: E402
from sitrack_amd import synthetic as syn       # noqa: E402


def haversine(plat, plon, xlat, xlon):
    to_rad = 3.141592653589793 / 180.
    a1 = np.sin(0.5 * ((xlat - plat) * to_rad))
    a2 = np.sin(0.5 * ((xlon - plon) * to_rad))
    a3 = np.cos(xlat * to_rad) * np.cos(plat * to_rad)
    return 2. * 6360. * np.arcsin(np.sqrt(a1 * a1 + a3 * a2 * a2))


def restated(la, lo, nall, nbef, rd):
    """the reference's loop restated (every buoy valid): keep mask"""
    n = len(la)
    alive = np.ones(n, dtype=bool)
    for j in range(n):
        if not alive[j]:
            continue
        d = haversine(la[j], lo[j], la, lo)
        d[j] = 9999.
        k = int(np.argmin(d))
        if d[k] < rd:
            ck = nall[k] if alive[k] else nbef[k]
            alive[j if nall[j] < ck else k] = False
    return alive


def copy_ms(n, out_bytes_per):
    """H2D of 2n doubles + n bytes and D2H of n * out_bytes_per bytes from/to pageable host memory"""
    import torch
    a = np.zeros((2, n))
    v = np.zeros(n, np.int8)
    d = torch.empty((2, n), dtype=torch.float64, device="cuda")
    dv = torch.empty(n, dtype=torch.int8, device="cuda")
    o = np.zeros(max(1, n * out_bytes_per), np.uint8)
    do = torch.zeros(len(o), dtype=torch.uint8, device="cuda")
    best = 1e30
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.copy_(torch.from_numpy(a))
        dv.copy_(torch.from_numpy(v))
        torch.cuda.synchronize()
        if out_bytes_per:
            torch.from_numpy(o).copy_(do)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def timed(f, reps=3):
    f()                                                     # scratch at its size
    best, r = 1e30, None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--dkm", type=float, default=1.5)
    ap.add_argument("--prefix", type=int, default=3000)
    a = ap.parse_args()
    N = a.grid
    ctx = sit.Context(0)
    g = syn.make_grid(N, N, dkm=a.dkm, warp=0.5)
    llT = ctx.cart2geo(np.stack([g["Yt"].ravel(), g["Xt"].ravel()], axis=1))
    latT, lonT = llT[:, 0].reshape(N, N).copy(), np.mod(llT[:, 1], 360.).reshape(N, N).copy()
    del llT, g
    ll, _, nT, _ = ctx.nemo_seed(np.ones((N, N), np.int8), latT, lonT, np.ones((N, N)))
    la1, lo1 = np.ascontiguousarray(ll[:, 0]), np.ascontiguousarray(ll[:, 1])
    rng = np.random.default_rng(5)
    n2 = min(10_000_000, len(la1))
    la2, lo2 = la1[:n2].copy(), lo1[:n2].copy()
    src, dst = rng.integers(0, n2, n2 // 50), rng.choice(n2, n2 // 50, replace=False)
    la2[dst] = np.clip(la2[src] + rng.normal(0., 3e-4, len(dst)), -90., 90.)
    lo2[dst] = np.mod(lo2[src] + rng.normal(0., 3e-4, len(dst)) / np.cos(np.radians(la2[src])), 360.)
    ctx.cancel_too_close(la1[:100_000], lo1[:100_000], None, np.ones(100_000), np.zeros(100_000), 6.)     # warm-up
    out = {"what": "sitrk_cancel_too_close", "grid": [N, N], "dkm": a.dkm, "cases": []}
    for tag, la, lo, rd in (("T-seeds", la1, lo1, 6.0), ("clustered", la2, lo2, 1.0)):
        n = len(la)
        nall = rng.integers(1, 11, n).astype(np.int32)
        nbef = (nall - rng.integers(1, 3, n)).clip(0).astype(np.int32)
        valid = np.ones(n, np.int8)
        ms, (keep, nclose) = timed(lambda: ctx.cancel_too_close(la, lo, valid, nall, nbef, rd))
        ms_nn, _ = timed(lambda: ctx.nearest_buoy(la, lo, valid, rd))
        c_in, c_nn = copy_ms(n, 0), copy_ms(n, 12)
        out["cases"].append({"cloud": tag, "n": n, "rd_km": rd, "wall_ms": round(ms, 2), "wall_ms_less_copies": round(ms - c_in, 2),
                             "copies_in_ms": round(c_in, 2), "nearest_wall_ms": round(ms_nn, 2),
                             "stage1_ms": round(ms_nn - c_nn, 2), "stages23_ms": round(ms - ms_nn + (c_nn - c_in), 2),
                             "close": int(nclose), "kept": int(keep.sum())})
        print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    m = min(a.prefix, len(la1))
    rng = np.random.default_rng(6)
    nall = rng.integers(1, 11, m).astype(np.int32)
    nbef = (nall - rng.integers(1, 3, m)).clip(0).astype(np.int32)
    for rd in (6.0,):
        t0 = time.perf_counter()
        kc = restated(la1[:m], lo1[:m], nall, nbef, rd)
        cs = time.perf_counter() - t0
        t1 = time.perf_counter()
        kg, _ = ctx.cancel_too_close(la1[:m], lo1[:m], None, nall, nbef, rd)
        gs = time.perf_counter() - t1
        out["prefix"] = {"n": m, "rd_km": rd, "restated_cpu_s": round(cs, 3), "gpu_s": round(gs, 4),
                         "identical": bool(np.array_equal(kc, kg))}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
