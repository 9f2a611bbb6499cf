#!/usr/bin/env python3
"""Time `sitrk_subsample_cloud` (seed-cloud coarsening, SubSampCloud) on seed clouds of a 4096 x 4096 polar mesh.

    python tools/bench_subsample.py [--grid 4096] [--dkm 1.5] [--prefix 100000]
Clouds: the T-seeds of `sitrk_nemo_seed` (C order) and T+F seeds, coarsened at rd = 6 and 34.5 km (the reference's -C 10
and -C 40).  Per case: wall ms of the call (host arrays in and out), the same less the host<->device copies of its input
and output timed alone, launches of the resolve kernel, kept count, and the O(n k) characterisation of the result.
For scale, the sequential greedy on the CPU (cKDTree + Python loop) on the first `--prefix` points of the T+F cloud,
with the dependency depth of that prefix (rounds of the eager rule: a point is dropped one round after its first kept
earlier neighbour, kept one round after the last of its earlier neighbours), and the GPU on the same prefix.
Prints one JSON line."""
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


def d2(a, b):
    """the contract's squared distance in fp64 (numpy does not fuse)"""
    dy = a[..., 0] - b[..., 0]
    dx = a[..., 1] - b[..., 1]
    return dy * dy + dx * dx


def characterisation_violations(yx, rd, keep):
    """O(n k) check of a keep mask without a sequential replay: it is the greedy result iff (a) no two kept points have
    d2 < r2 and (b) every dropped point has a kept earlier neighbour with d2 < r2.  Number of points that break it."""
    from scipy.spatial import cKDTree
    keep = np.asarray(keep, dtype=bool)
    n, r2, pad = len(yx), rd * rd, rd * (1.0 + 1e-9) + 1e-300
    ik = np.flatnonzero(keep)
    if n == 0 or len(ik) == 0:
        return n
    tk = cKDTree(yx[ik])
    pairs = tk.query_pairs(pad, output_type='ndarray')
    bad = int(np.count_nonzero(d2(yx[ik[pairs[:, 0]]], yx[ik[pairs[:, 1]]]) < r2)) if len(pairs) else 0
    idrop = np.flatnonzero(~keep)
    if len(idrop):
        # a correct kept set is >= rd apart, so at most 7 kept points lie within rd of any point; more than 12 means (a) has
        # already counted violations, and a truncated list can only add more
        dist, loc = tk.query(yx[idrop], k=12, distance_upper_bound=pad)
        valid = loc < len(ik)
        j = ik[np.where(valid, loc, 0)]
        ok = valid & (j < idrop[:, None]) & (d2(yx[j], yx[idrop][:, None, :]) < r2)
        bad += int(np.count_nonzero(~ok.any(axis=1)))
    return bad


def cpu_greedy_depth(yx, rd):
    """sequential greedy + dependency depth of the eager rule"""
    from scipy.spatial import cKDTree
    n = len(yx)
    r2 = rd * rd
    tree = cKDTree(yx)
    keep = np.zeros(n, dtype=bool)
    depth = np.zeros(n, dtype=np.int64)
    for i in range(n):
        nb = np.asarray(tree.query_ball_point(yx[i], rd * (1 + 1e-9)), dtype=np.int64)
        nb = nb[nb < i]
        nb = nb[d2(yx[nb], yx[i]) < r2]
        k = nb[keep[nb]]
        if len(k):
            depth[i] = depth[k].min() + 1
        else:
            keep[i] = True
            depth[i] = (depth[nb].max() + 1) if len(nb) else 1
    return keep, int(depth.max())


def copy_ms(n):
    """H2D of n (y,x) pairs and D2H of n bytes from/to pageable host memory, as the call does them"""
    import torch
    a = np.zeros((n, 2))
    b = np.zeros(n, np.int8)
    d = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    e = torch.zeros(n, dtype=torch.int8, device="cuda")
    best = 1e30
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.copy_(torch.from_numpy(a))
        torch.cuda.synchronize()
        torch.from_numpy(b).copy_(e)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--dkm", type=float, default=1.5)
    ap.add_argument("--prefix", type=int, default=100_000)
    a = ap.parse_args()
    N = a.grid
    ctx = sit.Context(0)
    g = syn.make_grid(N, N, dkm=a.dkm, warp=0.5)
    llT = ctx.cart2geo(np.stack([g["Yt"].ravel(), g["Xt"].ravel()], axis=1))
    llF = ctx.cart2geo(np.stack([g["Yf"].ravel(), g["Xf"].ravel()], axis=1))
    latT, lonT = llT[:, 0].reshape(N, N).copy(), np.mod(llT[:, 1], 360.).reshape(N, N).copy()
    latF, lonF = llF[:, 0].reshape(N, N).copy(), np.mod(llF[:, 1], 360.).reshape(N, N).copy()
    del llT, llF, g
    ones, tm = np.ones((N, N)), np.ones((N, N), np.int8)
    _, yxT, nT, _ = ctx.nemo_seed(tm, latT, lonT, ones)
    _, yxTF, nT2, nF = ctx.nemo_seed(tm, latT, lonT, ones, latF=latF, lonF=lonF)
    ctx.subsample_cloud(yxTF[:100_000], 6.0)                  # warm-up (code objects, scratch)
    out = {"what": "sitrk_subsample_cloud", "grid": [N, N], "dkm": a.dkm, "cases": []}
    for tag, yx in (("T", yxT), ("T+F", yxTF)):
        cms = copy_ms(len(yx))
        for rd in (6.0, 34.5):
            ctx.subsample_cloud(yx, rd)                        # scratch at its size
            t0 = time.perf_counter()
            keep, nl = ctx.subsample_cloud(yx, rd)
            ms = (time.perf_counter() - t0) * 1e3
            t1 = time.perf_counter()
            bad = characterisation_violations(yx, rd, keep)
            chk_s = time.perf_counter() - t1
            out["cases"].append({"cloud": tag, "n": len(yx), "rd_km": rd, "wall_ms": round(ms, 2),
                                 "wall_ms_less_copies": round(ms - cms, 2), "copies_ms": round(cms, 2), "launches": nl,
                                 "kept": int(keep.sum()), "characterisation_violations": bad, "check_s": round(chk_s, 1)})
            print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    m = min(a.prefix, len(yxTF))
    for rd in (6.0, 34.5):
        pre = yxTF[:m]
        t0 = time.perf_counter()
        kc, depth = cpu_greedy_depth(pre, rd)
        cs = time.perf_counter() - t0
        t1 = time.perf_counter()
        kg, nl = ctx.subsample_cloud(pre, rd)
        gs = time.perf_counter() - t1
        out.setdefault("prefix", []).append({"n": m, "rd_km": rd, "cpu_greedy_s": round(cs, 2), "depth": depth, "gpu_s": round(gs, 4),
                                             "gpu_launches": nl, "identical": bool(np.array_equal(kc, kg))})
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
