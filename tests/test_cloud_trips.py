"""The four point-cloud modules (sitrk_delaunay, sitrk_coast, sitrk_overlap, sitrk_subsample) start with a reduction kernel of at
most `cap` workgroups of `threads` lanes; above cap x threads elements its lanes take a second grid-stride trip.  This file ties
that size to the sources' constants (a retuned cap or thread count fails here instead of silently taking the GPU tests back into
one trip), and holds the inputs the GPU tests run past it, with the properties that make a lost or wrong second trip change the
result checked here, on the CPU.

The builders are cached: the CPU tests here and the GPU tests that import them share one copy, which nobody modifies."""
import functools
import os
import re

import numpy as np
import pytest

from test_cancel_too_close import load_generator, nearest, random_cloud, scan
from test_coast import checkerboard, coast_dist_ref, coast_segments_vec, d2_ref
from test_delaunay import delaunay_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sitrack_amd", "csrc")

TRIP = 524288                    # cap x threads of every launch below
NP_TRIP = TRIP + 4099            # the clouds' size: a second trip that is no multiple of a workgroup

# module, its thread constant, the capped kernel
LAUNCHES = [("sitrk_delaunay.hip", "kDlThreads", "dl_quant_kernel"),
            ("sitrk_coast.hip", "kCoastThreads", "coast_stats_kernel"),
            ("sitrk_overlap.hip", "kOvThreads", "unit_bbox_kernel"),
            ("sitrk_subsample.hip", "kSubThreads", "bbox_kernel")]


# ------------------------------------------------------------------------------------------------ 0. the sizes and the sources
def launch_shape(fname, tconst, kernel):
    """(cap, threads) of the one launch of `kernel` in the module, read from its text"""
    src = open(os.path.join(CSRC, fname)).read()
    m = re.findall(r"^constexpr int %s = (\d+);" % tconst, src, flags=re.M)
    assert len(m) == 1, (fname, tconst, m)
    threads = int(m[0])
    calls = re.findall(r"hipLaunchKernelGGL\(%s, dim3\((.*?)\), dim3\((\w+)\), 0, " % kernel, src)
    assert len(calls) == 1, (fname, kernel, calls)
    grid, block = calls[0]
    assert block == tconst, (fname, block)
    a = re.fullmatch(r"std::min\(nblk\((\w+)\), (\d+)u\)", grid)
    b = re.fullmatch(r"nblk\((\w+)\) < (\d+)u \? nblk\((\w+)\) : (\d+)u", grid)
    assert a or b, (fname, grid)
    if a:
        cap = int(a.group(2))
    else:
        assert b.group(1) == b.group(3) and b.group(2) == b.group(4), (fname, grid)
        cap = int(b.group(2))
    # the workgroups are counted and the lanes stride by the same constant
    assert re.search(r"inline unsigned nblk\(int64_t n\) \{ return \(unsigned\)\(\(n \+ %s - 1\) / %s\); \}" % (tconst, tconst), src), fname
    body = src[src.index("void %s(" % kernel):]
    loop = re.search(r"for \(int64_t (\w) = \(int64_t\)blockIdx\.x \* (\w+) \+ threadIdx\.x; \1 < \w+; \1 \+= \(int64_t\)gridDim\.x \* (\w+)\)", body)
    assert loop and body.index(loop.group(0)) < body.index("__syncthreads"), (fname, kernel)
    assert loop.group(2) == loop.group(3) == tconst, (fname, loop.group(0))
    return cap, threads


@pytest.mark.parametrize("fname,tconst,kernel", LAUNCHES, ids=[k for _, _, k in LAUNCHES])
def test_one_trip_of_the_capped_reduction_is_TRIP_elements(fname, tconst, kernel):
    cap, threads = launch_shape(fname, tconst, kernel)
    assert cap * threads == TRIP, "%s: %d workgroups of %d lanes; move TRIP and the GPU tests' sizes with them" % (kernel, cap, threads)
    assert TRIP < NP_TRIP < 2 * TRIP and (NP_TRIP - TRIP) % threads != 0


# ------------------------------------------------------------------------------------------------ 1. Delaunay
DL_SIDE, DL_RMAX = 138, 1.5


@functools.lru_cache(maxsize=None)
def delaunay_trip_case(seed=5):
    """(yx (NP_TRIP,2), mask, rmax, (tris, vertex) of delaunay_fast): many points, few vertices.  The 138 x 138 vertices, a jittered
    unit lattice in shuffled order, sit in slots drawn from [0, 12000) and [TRIP - 3000, NP_TRIP); every other index is a decoy
    inside the same box, three in four masked off with finite coordinates, one in four unmasked with NaN in y or inf in x."""
    rng = np.random.default_rng(seed)
    nV = DL_SIDE * DL_SIDE
    pool = np.concatenate([np.arange(12000), np.arange(TRIP - 3000, NP_TRIP)])
    slots = np.sort(rng.permutation(pool)[:nV])
    j, i = np.meshgrid(np.arange(DL_SIDE, dtype=np.float64), np.arange(DL_SIDE, dtype=np.float64), indexing="ij")
    lat = np.stack([j.ravel(), i.ravel()], axis=1) + rng.uniform(-0.3, 0.3, (nV, 2))
    yx = rng.uniform(0., DL_SIDE - 1., (NP_TRIP, 2))                       # the decoys: anywhere on the lattice
    yx[slots] = lat[rng.permutation(nV)]
    yx += np.array([-1200., 300.])
    mask = np.ones(NP_TRIP, dtype=np.int8)
    decoy = np.ones(NP_TRIP, dtype=bool)
    decoy[slots] = False
    decoy = np.flatnonzero(decoy)
    broken = decoy[3::4]                                                   # unmasked, no position
    off = np.setdiff1d(decoy, broken)
    mask[off] = 0
    yx[broken[0::2], 0] = np.nan
    yx[broken[1::2], 1] = np.inf
    want = delaunay_fast(yx, DL_RMAX, mask)
    for a in (yx, mask) + want:
        a.setflags(write=False)
    return yx, mask, DL_RMAX, want


def test_delaunay_trip_case_needs_the_second_trip():
    yx, mask, rmax, (tris, vertex) = delaunay_trip_case()
    assert len(yx) == NP_TRIP and (vertex == 1).sum() == DL_SIDE * DL_SIDE and not (vertex == 2).any()
    decoy = vertex == 0
    assert decoy.sum() == NP_TRIP - DL_SIDE * DL_SIDE
    masked, broken = decoy & (mask == 0), decoy & (mask != 0)
    assert np.isfinite(yx[masked]).all() and not np.isfinite(yx[broken]).all(axis=1).any()
    assert np.isnan(yx[broken, 0]).sum() > 50000 and np.isinf(yx[broken, 1]).sum() > 50000
    assert abs(masked.sum() - 3 * broken.sum()) <= 3 and (broken[TRIP:]).any() and (masked[TRIP:]).any()
    # the masked decoys lie among the vertices: were the mask ignored they would be vertices of other triangles
    box = yx[vertex == 1]
    assert (yx[masked] >= box.min(axis=0)).all() and (yx[masked] <= box.max(axis=0)).all()
    hi = tris >= TRIP
    print("%d vertices, %d at indices >= TRIP; %d rows, %d all in the second trip, %d mixed" %
          ((vertex == 1).sum(), (vertex[TRIP:] == 1).sum(), len(tris), hi.all(axis=1).sum(), (hi.any(axis=1) & ~hi.all(axis=1)).sum()))
    assert (vertex[TRIP:] == 1).sum() >= 1000
    assert hi.all(axis=1).sum() >= 100
    assert (hi.any(axis=1) & ~hi.all(axis=1)).sum() >= 1000
    first = mask.copy()
    first[TRIP:] = 0
    lost, _ = delaunay_fast(yx, rmax, first)                               # what a kernel that never took the second trip would see
    print("%d rows without the second trip's vertices" % len(lost))
    assert len(lost) != len(tris)


# ------------------------------------------------------------------------------------------------ 2. coast
CO_N, CO_D, CO_JS, CO_STEEP = 520, 4.0, 514, 30.0
CO_Y0, CO_X0 = -1000., 500.


@functools.lru_cache(maxsize=None)
def coast_trip_grid():
    """(Yf, Xf, tmask): 520 x 520 F-points, x spacing d = 4 km, rows d apart up to row JS = 514 and 30 d above it, offset by
    (-1000, 500) km; a checkerboard of land and sea, so every interior edge is a coast segment.  The only long segments are the
    k = 0 edges above row JS, which come last in id order."""
    row = np.arange(CO_N, dtype=np.float64)
    y = CO_D * np.minimum(row, CO_JS) + CO_STEEP * CO_D * np.maximum(row - CO_JS, 0.) + CO_Y0
    x = CO_D * row + CO_X0
    Yf, Xf = (np.ascontiguousarray(a) for a in np.broadcast_arrays(y[:, None], x[None, :]))
    tmask = checkerboard(CO_N, CO_N)
    for a in (Yf, Xf, tmask):
        a.setflags(write=False)
    return Yf, Xf, tmask


@functools.lru_cache(maxsize=None)
def coast_trip_segments():
    ids, ab, nd = coast_segments_vec(*coast_trip_grid())
    ids.setflags(write=False)
    ab.setflags(write=False)
    return ids, ab, nd


def seg_length(ab):
    e = ab[:, 1] - ab[:, 0]
    return np.hypot(e[:, 0], e[:, 1])


CO_DESIGNED, CO_DENSE = 48, 16


@functools.lru_cache(maxsize=None)
def coast_trip_queries(seed=13):
    """(yx (72,2), designed, dense): index ranges of the two kinds the tests speak of.  Few, because the brute force they are held
    to reads every one of the 538 722 segments for each.

    designed: 0.3 d above row JS and 0.1 d right of an F-column.  The nearest segment is the long k = 0 segment that starts at
    that F-point, 0.4 km away, whose midpoint (what the index bins it by) is 58.8 km away; the nearest short one is the row's
    k = 1 segment, 1.2 km away.  A search radius from a `pad` that saw the first trip's segments only (about 2 km) stops short.
    dense: vertices and interiors of segments of the first trip, and points beside them, in the part of the grid with even spacing.
    the rest: on and beside the long segments, far points on two sides, one NaN, one inf."""
    rng = np.random.default_rng(seed)
    ids, ab, _ = coast_trip_segments()
    Yf, Xf, _ = coast_trip_grid()
    cols = np.sort(rng.choice(CO_N - 1, CO_DESIGNED, replace=False))
    cols[0], cols[-1] = 0, CO_N - 2                                        # the first and the last column that has a k = 0 edge
    designed = np.stack([Yf[CO_JS, cols] + 0.3 * CO_D, Xf[CO_JS, cols] + 0.1 * CO_D], axis=1)
    k = rng.integers(0, TRIP - 8 * CO_N, CO_DENSE)                          # four rows below the first segment of the second trip
    t = rng.integers(0, 8, CO_DENSE)[:, None] / 8.                          # 0: the vertex a
    dense = ab[k, 0] + t * (ab[k, 1] - ab[k, 0])
    dense[::3] += rng.choice([-1.3, 1.3], (len(dense[::3]), 2))             # off the segments, inside a cell
    long_ = np.flatnonzero(seg_length(ab) > 1.5 * CO_D)
    k = rng.choice(long_, 4, replace=False)
    on_long = ab[k, 0] + np.array([[0.], [0.25], [0.625], [1.]]) * (ab[k, 1] - ab[k, 0])
    on_long[::2, 1] += rng.uniform(-1.9, 1.9, 2)                            # beside them: nearer than the next column
    y0, y1, x0, x1 = Yf.min(), Yf.max(), Xf.min(), Xf.max()
    L = 10. * max(y1 - y0, x1 - x0)
    far = np.array([[rng.uniform(y0, y1), x1 + L], [y0 - L, rng.uniform(x0, x1)]])
    yx = np.ascontiguousarray(np.concatenate([designed, dense, on_long, far, [[np.nan, 0.], [0., np.inf]]]))
    yx.setflags(write=False)
    return yx, slice(0, CO_DESIGNED), slice(CO_DESIGNED, CO_DESIGNED + CO_DENSE)


COAST_BATCH = 8                  # queries per batch of the brute force: one temporary of 8 x 538 722 doubles is 34 MB


def test_coast_trip_grid_hides_its_longest_segments_in_the_second_trip():
    ids, ab, nd = coast_trip_segments()
    nseg = len(ids)
    assert nd == 0 and nseg == 2 * (CO_N - 1) ** 2 and nseg > TRIP and np.all(np.diff(ids) > 0)
    length = seg_length(ab)
    long_ = np.flatnonzero(length > 1.5 * CO_D)
    print("%d segments, %d in the second trip; %d longer than 1.5 d, the first at position %d" % (nseg, nseg - TRIP, len(long_), long_[0]))
    assert len(long_) == 5 * (CO_N - 1) and long_.min() >= TRIP
    assert length[long_].min() == CO_STEEP * CO_D and length[:TRIP].max() == CO_D
    assert COAST_BATCH * nseg * 8 <= 256 << 20


def test_coast_trip_queries_are_answered_by_the_second_trip():
    ids, ab, _ = coast_trip_segments()
    yx, designed, dense = coast_trip_queries()
    assert len(yx) <= 128 and designed.stop - designed.start >= 48 and dense.stop - dense.start >= 16
    is_long = seg_length(ab) > 1.5 * CO_D
    q = yx[designed]
    for b in range(0, len(q), COAST_BATCH):
        d2 = d2_ref(q[b:b + COAST_BATCH], ab)
        k = np.argmin(d2, axis=1)
        best = d2[np.arange(len(k)), k]
        assert is_long[k].all() and (k >= TRIP).all()
        assert (np.sqrt(best) < 0.11 * CO_D).all()
        mid = 0.5 * (ab[k, 0] + ab[k, 1]) - q[b:b + COAST_BATCH]
        assert (np.hypot(mid[:, 0], mid[:, 1]) > 14. * CO_D).all()        # far beyond any radius the first trip's 4 km would give
        short = np.sqrt(np.where(is_long[None, :], np.inf, d2).min(axis=1))
        assert (short > 0.29 * CO_D).all() and (short >= 2. * np.sqrt(best)).all()
    # the dense ones are answered by the first trip
    _, seg, dist = coast_dist_ref(yx[dense], ids, ab, batch=COAST_BATCH)
    assert (np.searchsorted(ids, seg) < TRIP).all() and (dist <= 0.5 * CO_D).all() and (dist == 0.).sum() >= 8 and (dist > 0.).sum() >= 4


# ------------------------------------------------------------------------------------------------ 3. overlap
OV_VALID, OV_RD = 4000, 5.0


@functools.lru_cache(maxsize=None)
def cancel_trip_case(seed=77):
    """(la, lo, valid, nall, nbef, rd, alive, nclose, close, nn): NP_TRIP buoys of which about 4000 are valid, a third of them at
    indices >= TRIP, clustered so that most have another within rd; the invalid ones hold fill or NaN.  alive and nclose restate
    sitrk_cancel_too_close: the reference's nearest neighbours on the valid subset (which keeps index order, so its first minimum
    is the lowest index), mapped back, and its scan over the full index space."""
    gen = load_generator()
    rng = np.random.default_rng(seed)
    n, rd = NP_TRIP, OV_RD
    nhi = OV_VALID // 3
    sub = np.sort(np.concatenate([rng.choice(TRIP, OV_VALID - nhi, replace=False), TRIP + rng.choice(n - TRIP, nhi, replace=False)]))
    for _ in range(20):
        la_s, lo_s = random_cloud(rng, len(sub), rd, nclust=len(sub) // 60)
        if gen.ulp_safe(la_s, lo_s, rd):
            break
    else:
        raise RuntimeError("no ulp-safe draw")
    valid = np.zeros(n, dtype=np.int8)
    valid[sub] = 1
    bad = np.arange(n)
    la = np.where(bad % 2, -9999., np.nan)
    lo = np.where(bad % 3, -9999., np.nan)
    la[sub], lo[sub] = la_s, lo_s
    nall = rng.integers(1, 6, n).astype(np.int32)
    nbef = np.minimum(nall, rng.integers(0, 3, n)).astype(np.int32)
    nn_s, d_s = nearest(la_s, lo_s)
    nn = np.full(n, -1, dtype=np.int64)
    dmin = np.full(n, np.inf)
    nn[sub], dmin[sub] = sub[nn_s], d_s
    alive = scan(nn, dmin, valid, nall, nbef, rd)
    close = (valid != 0) & (dmin < rd)
    out = (la, lo, valid, nall, nbef, rd, alive, int(close.sum()))
    for a in out[:5] + (alive,):
        a.setflags(write=False)
    return out + (close, np.where(close, nn, -1))


def test_cancel_trip_case_has_close_buoys_on_both_sides_of_the_trip():
    la, lo, valid, nall, nbef, rd, alive, nclose, close, nn = cancel_trip_case()
    nv = int((valid != 0).sum())
    print("%d valid, %d at indices >= TRIP; %d close (%d >= TRIP); %d kept" % (nv, (valid[TRIP:] != 0).sum(), nclose, close[TRIP:].sum(), alive.sum()))
    assert len(la) == NP_TRIP and 3500 <= nv <= 4500 and 0.3 * nv <= (valid[TRIP:] != 0).sum() <= 0.4 * nv
    assert nclose > 0.6 * nv and close[TRIP:].sum() >= 500 and close[:TRIP].sum() >= 500
    inv = valid == 0
    assert np.isnan(la[inv]).any() and (la[inv] == -9999.).any() and np.isnan(lo[inv]).any() and np.isfinite(la[~inv]).all()
    # buoys are dropped on both sides, and none that was not close
    dropped = (valid != 0) & ~alive
    assert (nn[close] >= 0).all() and (close[nn[close]]).all() and ((nn[close] >= TRIP) != (np.flatnonzero(close) >= TRIP)).sum() >= 100
    assert dropped[TRIP:].sum() >= 100 and dropped[:TRIP].sum() >= 100 and not (dropped & ~close).any() and not alive[inv].any()
