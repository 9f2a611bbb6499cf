"""Coarse-grained deformation of buoy cells (sitrk_coarse_cells, sitrk_mesh_coarse; include/sitrk.h): the numpy
restatement the GPU tests compare against, its self-checks, the binding, scaling_exponents and the command line's parser.

coarse_ref() is written from the contract in the header alone.  numpy's elementwise fp64 + - * / round once per operation and
never fuse, the terms of a pixel are added one cell at a time in a Python loop over ascending cell index, and a level is formed
from padded slices as (c00 + c01) + (c10 + c11): the restatement of `boxes`, nin, nout and the two counting columns of the table
is exact.  Columns 2..7 of its table are math.fsum of the terms, the exactly rounded sum; a device sum in any order of n terms
lies within (n - 1) 2^-53 sum|t| of it (tests/test_gpu_coarse.py)."""
import math
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import coarse as co
from sitrack_amd import driver as drv
from test_mesh import ccw_quads, exact_lattice
from test_raster import JITTER_GRIDS, JITTER_INNER, jitter_case, lattice_case, split_quads
from test_tri2quad import chain_constants, up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sitrk_coarse_cells", "sitrk_mesh_coarse", "sitrk_coarse_kernel_ms")
TIE_GRID = (-1504., 1996., 8., 14, 16)                               # every centroid of the exact lattice on a pixel corner
ONE_PIXEL = (-1600., 1900., 1000., 1, 1)
DAY = 86400.


def cell_terms(yx0, yx1, cells, T, mask0=None, mask1=None):
    """(terms (5, nC) = a, a*u_x, a*u_y, a*v_x, a*v_y; valid (nC,) bool) of the sitrk_deform_cells contract, in its order"""
    yx0, yx1 = np.asarray(yx0, dtype=np.float64), np.asarray(yx1, dtype=np.float64)
    cells = np.asarray(cells)
    nC, nv = cells.shape
    T = np.float64(T)
    y, x, Y, X = yx0[cells, 0], yx0[cells, 1], yx1[cells, 0], yx1[cells, 1]
    ok = np.isfinite(y).all(1) & np.isfinite(x).all(1) & np.isfinite(Y).all(1) & np.isfinite(X).all(1)
    if mask0 is not None:
        ok &= (np.asarray(mask0)[cells] != 0).all(1)
    if mask1 is not None:
        ok &= (np.asarray(mask1)[cells] != 0).all(1)
    with np.errstate(all="ignore"):
        dx, dy = x - x[:, :1], y - y[:, :1]
        u, v = (X - x) / T, (Y - y) / T
        A2, Suy, Sux, Svy, Svx = (np.zeros(nC) for _ in range(5))
        for k in range(nv):
            q = (k + 1) % nv
            A2 = A2 + (dx[:, k] * dy[:, q] - dx[:, q] * dy[:, k])
            Suy = Suy + (u[:, q] + u[:, k]) * (dy[:, q] - dy[:, k]); Sux = Sux + (u[:, q] + u[:, k]) * (dx[:, q] - dx[:, k])
            Svy = Svy + (v[:, q] + v[:, k]) * (dy[:, q] - dy[:, k]); Svx = Svx + (v[:, q] + v[:, k]) * (dx[:, q] - dx[:, k])
        ok &= (A2 != 0.0) & np.isfinite(A2)
        ux, uy, vx, vy = Suy / A2, -(Sux / A2), Svy / A2, -(Svx / A2)
        a = 0.5 * np.abs(A2)
        return np.stack([a, a * ux, a * uy, a * vx, a * vy]), ok


def centroid_pixels(yx0, cells, grid):
    """(inside (nC,) bool, j, i) of the t0 centroids on the grid"""
    y0, x0, d, ny, nx = grid
    y0, x0, d = np.float64(y0), np.float64(x0), np.float64(d)
    P = np.asarray(yx0, dtype=np.float64)[np.asarray(cells)]
    with np.errstate(all="ignore"):
        if P.shape[1] == 4:
            cy = 0.25 * ((P[:, 0, 0] + P[:, 1, 0]) + (P[:, 2, 0] + P[:, 3, 0]))
            cx = 0.25 * ((P[:, 0, 1] + P[:, 1, 1]) + (P[:, 2, 1] + P[:, 3, 1]))
        else:
            cy = ((P[:, 0, 0] + P[:, 1, 0]) + P[:, 2, 0]) / 3.0
            cx = ((P[:, 0, 1] + P[:, 1, 1]) + P[:, 2, 1]) / 3.0
        fy, fx = (cy - y0) / d, (cx - x0) / d
        inside = (fy >= 0.) & (fy < np.float64(ny)) & (fx >= 0.) & (fx < np.float64(nx))
    j = np.where(inside, np.floor(np.where(inside, fy, 0.)), 0).astype(np.int64)
    i = np.where(inside, np.floor(np.where(inside, fx, 0.)), 0).astype(np.int64)
    return inside, j, i, fy, fx


def level_up(lev):
    """(6, ceil(ny/2), ceil(nx/2)) from (6, ny, nx): (c00 + c01) + (c10 + c11), a child beyond the edge +0.0"""
    _, ny, nx = lev.shape
    pad = np.zeros((6, ny + ny % 2, nx + nx % 2))
    pad[:, :ny, :nx] = lev
    return (pad[:, 0::2, 0::2] + pad[:, 0::2, 1::2]) + (pad[:, 1::2, 0::2] + pad[:, 1::2, 1::2])


def box_terms(lev, side, fmin):
    """(some (ny,nx) bool, filled (ny,nx) bool, terms (6, nfilled)) of one level: A, A*div, A*shr, A*tot, (A*tot)*tot, ..."""
    n, A = lev[0], lev[1]
    some = n >= 1.
    filled = some & (A > 0.) & (A >= np.float64(fmin) * (np.float64(side) * np.float64(side)))
    A = A[filled]
    UX, UY, VX, VY = (lev[k][filled] / A for k in (2, 3, 4, 5))
    div, e1, e2 = UX + VY, UX - VY, UY + VX
    shr = np.sqrt(e1 * e1 + e2 * e2)
    tot = np.sqrt(div * div + shr * shr)
    m1 = A * tot
    m2 = m1 * tot
    return some, filled, np.stack([A, A * div, A * shr, m1, m2, m2 * tot])


def table_ref(levels, d, fmin):
    """the table of a pyramid: the counting columns exact, the six sums exactly rounded (math.fsum)"""
    table = np.zeros((len(levels), 8))
    for l, lev in enumerate(levels):
        some, filled, t = box_terms(lev, np.float64(d) * 2. ** l, fmin)
        table[l, 0], table[l, 1] = some.sum(), filled.sum()
        table[l, 2:] = [math.fsum(row) for row in t]
    return table


def coarse_ref(yx0, yx1, cells, T, grid, nlev, fmin=0.5, mask0=None, mask1=None, use=None):
    """the contract of sitrk_coarse_cells: {"levels": [(6, ny_l, nx_l)], "table", "nin", "nout"}"""
    cells = np.asarray(cells)
    ny, nx = grid[3:]
    lev0 = np.zeros((6, ny, nx))
    nin = nout = 0
    if len(cells):
        t, ok = cell_terms(yx0, yx1, cells, T, mask0, mask1)
        if use is not None:
            ok = ok & (np.asarray(use) != 0)
        inside, j, i, _, _ = centroid_pixels(yx0, cells, grid)
        nin, nout = int((ok & inside).sum()), int((ok & ~inside).sum())
        for c in np.flatnonzero(ok & inside):                         # ascending cell index, S = S + t
            lev0[0, j[c], i[c]] += 1.
            lev0[1:, j[c], i[c]] = lev0[1:, j[c], i[c]] + t[:, c]
    levels = [lev0]
    for _ in range(1, nlev):
        levels.append(level_up(levels[-1]))
    return {"levels": levels, "table": table_ref(levels, grid[2], fmin), "nin": nin, "nout": nout}


def shapes(r):
    return [lev.shape[1:] for lev in r["levels"]]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# uniform strain on the exact lattice: powers of two, so that every operation of the contract is exact
STRAIN_T = 65536.
STRAIN = dict(vy=2. ** -22, vx=2. ** -23, uy=-2. ** -23, ux=2. ** -21)


def strain_move(yx0):
    y, x = yx0[:, 0], yx0[:, 1]
    return np.stack([y + STRAIN_T * (STRAIN["vy"] * y + STRAIN["vx"] * x), x + STRAIN_T * (STRAIN["uy"] * y + STRAIN["ux"] * x)], axis=1)


def smooth_move(yx0, T=DAY):
    """a smooth velocity field that is not linear in space: strains of about 1e-6 /s that change over 100-200 km"""
    y, x = yx0[:, 0], yx0[:, 1]
    u = 1.1e-4 * np.sin(x / 150.) * np.cos(y / 210.) + 2e-8 * (y + 1500.)
    v = 0.9e-4 * np.cos(x / 170.) * np.sin(y / 130.) - 3e-8 * (x - 2000.)
    return np.stack([y + T * v, x + T * u], axis=1)


_CASES = {}


def jitter_coarse(key):
    """coarse_ref of jitter_case() under smooth_move, computed once: key = "18.4" | "inner" | "one" | "perm" (18.4 km, the rows in
    the fixed random order jitter_perm())"""
    if key not in _CASES:
        yx, quads, _ = jitter_case()
        yx1 = smooth_move(yx)
        grid, nlev, rows = {"18.4": (JITTER_GRIDS[18.4], 6, quads), "perm": (JITTER_GRIDS[18.4], 6, quads[jitter_perm()]),
                            "inner": (JITTER_INNER, 4, quads), "one": (ONE_PIXEL, 2, quads)}[key]
        _CASES[key] = coarse_ref(yx, yx1, rows, DAY, grid, nlev)
    return _CASES[key]


def jitter_perm():
    return np.random.default_rng(11).permutation(1225)


# The case that takes the rows-of-partials reductions of sitrk_coarse.hip into a second trip (tests/test_gpu_coarse.py): a
# jittered lattice of 301 x 291 points 8 km apart, 87 000 quadrangles in a fixed random order, on 300 x 290 pixels of 7.6 km whose
# origin lies inside the mesh, so that cells fall outside on all four sides.
BIG_LATTICE = (301, 291)
BIG_GRID = (-1469.7, 2025.7, 7.6, 300, 290)
BIG_NLEV = 4


def big_case():
    """(yx, yx1, quads): the lattice moved by smooth_move, its quadrangles in a fixed random order"""
    if "big" not in _CASES:
        ny, nx = BIG_LATTICE
        yx = exact_lattice(ny, nx, 8.0) + np.random.default_rng(1).uniform(-2., 2., (ny * nx, 2))
        quads = ccw_quads(ny, nx)
        _CASES["big"] = (yx, smooth_move(yx), np.ascontiguousarray(quads[np.random.default_rng(11).permutation(len(quads))]))
    return _CASES["big"]


def big_use():
    """a `use` mask over the quadrangles of big_case() that switches off one contributing cell inside the grid in every trip
    of coarse_count_kernel's loop over the rows of counts, and one outside the grid in the last trip: (use (nC,) int8, the
    cells switched off, their trips)"""
    T = chain_constants()["kCoThreads"]
    yx, yx1, quads = big_case()
    _, ok = cell_terms(yx, yx1, quads, DAY)
    inside = centroid_pixels(yx, quads, BIG_GRID)[0]
    trip = np.arange(len(quads)) // (T * T)                               # row = cell // T, trip = row // T
    off = [int(np.flatnonzero(ok & inside & (trip == k))[7]) for k in range(trip.max() + 1)]
    off.append(int(np.flatnonzero(ok & ~inside & (trip == trip.max()))[3]))
    use = np.ones(len(quads), dtype=np.int8)
    use[off] = 0
    return use, off, trip[off].tolist()


def big_coarse(key):
    """coarse_ref of big_case(), computed once and left unchanged: key = "quads" | "tris" (split_quads: twice the cells) | "use"
    (the quadrangles under big_use())"""
    if "big " + key not in _CASES:
        yx, yx1, quads = big_case()
        cells = split_quads(quads) if key == "tris" else quads
        _CASES["big " + key] = coarse_ref(yx, yx1, cells, DAY, BIG_GRID, BIG_NLEV, use=big_use()[0] if key == "use" else None)
    return _CASES["big " + key]


def sort_end_bit(npix):
    """the number of key bits coarse_run sorts on: the keys run 0 .. npix"""
    end_bit = 1
    while end_bit < 32 and (1 << end_bit) <= npix:
        end_bit += 1
    return end_bit


def late_share(lev, side, fmin, first_pixel):
    """Of one level of a pyramid: [(|exactly rounded sum of the column's terms over the filled boxes of index >= first_pixel|,
    the bound (n + 16) 2^-53 fsum|t| of tests/test_gpu_coarse.py over all filled boxes)] for the six moments, and the number of
    such boxes with a cell and filled."""
    some, filled, t = box_terms(lev, side, fmin)
    late = np.flatnonzero(filled.ravel()) >= first_pixel                  # box_terms keeps the filled boxes in ascending index
    n = int(filled.sum())
    return ([(abs(math.fsum(row[late])), (n + 16) * 2. ** -53 * math.fsum(np.abs(row))) for row in t],
            int(some.ravel()[first_pixel:].sum()), int(late.sum()))


# ------------------------------------------------------------------------------------------------ the restatement's self-checks
def test_centroids_on_pixel_corners_go_to_the_upper_pixel():
    yx, quads, _, _ = lattice_case()
    assert len(quads) == 143
    inside, j, i, fy, fx = centroid_pixels(yx, quads, TIE_GRID)
    assert inside.all() and (fy == np.floor(fy)).all() and (fx == np.floor(fx)).all()      # all 143 exactly on pixel corners
    assert fy.min() == 1. and fy.max() == 11. and fx.min() == 1. and fx.max() == 13.
    assert np.array_equal(j, fy.astype(int)) and np.array_equal(i, fx.astype(int))
    r = coarse_ref(yx, strain_move(yx), quads, STRAIN_T, TIE_GRID, 5)
    assert shapes(r) == [(14, 16), (7, 8), (4, 4), (2, 2), (1, 1)] and (r["nin"], r["nout"]) == (143, 0)
    n0 = r["levels"][0][0]
    assert n0[0, 0] == 0. and n0[1, 1] == 1. and n0.sum() == 143. and n0.max() == 1. and (n0[1:12, 1:14] == 1.).all()
    for lev in r["levels"]:
        assert lev[0].sum() == 143.
    assert r["levels"][4][0, 0, 0] == 143. and r["levels"][4][1, 0, 0] == 143. * 64.
    # either orientation of the rows: the same bits
    mixed = quads.copy()
    mixed[::3] = mixed[::3, ::-1]
    rm = coarse_ref(yx, strain_move(yx), mixed, STRAIN_T, TIE_GRID, 5)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(r["levels"], rm["levels"]))


def test_uniform_strain_is_returned_exactly_at_every_level():
    """Every operation of the contract is exact here (coordinates are multiples of 8 below 4096, the gradients times T powers of
    two), so every nonempty box returns the four imposed gradients bit for bit.  beta: every filled box has the same tot, so each
    level's mean is tot^q (1 + e) with |e| below (n + 4) 2^-53 <= 2e-14 for n <= 143 boxes; the slope of log(mean) over levels at
    least log 2 apart is then below 1e-13 in magnitude."""
    yx, quads, _, _ = lattice_case()
    r = coarse_ref(yx, strain_move(yx), quads, STRAIN_T, TIE_GRID, 5)
    for lev in r["levels"]:
        some = lev[0] >= 1.
        assert some.any()
        for k, name in ((2, "ux"), (3, "uy"), (4, "vx"), (5, "vy")):
            assert (lev[k][some] / lev[1][some] == STRAIN[name]).all(), name
        assert (lev[1][some] == 64. * lev[0][some]).all()
    t = r["table"]
    assert t[:, 0].tolist() == [143., 42., 12., 4., 1.] and t[0, 1] == 143. and t[0, 2] == 143. * 64.
    assert t[:, 1].tolist() == [143., 41., 11., 2., 1.]               # a box must be half covered: 9152 of 16384 km^2 at the top
    s = sit.scaling_exponents(t, 8., min_boxes=1)
    print("filled", t[:, 1], "beta", s["beta"])
    assert s["used"].sum() >= 3 and (np.abs(s["beta"]) < 1e-13).all()
    div, e1, e2 = STRAIN["ux"] + STRAIN["vy"], STRAIN["ux"] - STRAIN["vy"], STRAIN["uy"] + STRAIN["vx"]
    tot = math.sqrt(div * div + (e1 * e1 + e2 * e2))
    assert abs(t[0, 5] / t[0, 2] - tot) <= 4 * np.spacing(tot) and t[0, 3] == 143. * 64. * div
    assert np.array_equal(s["L_km"], 8. * 2. ** np.arange(5)) and s["L_eff_km"][0] == 8.


def test_jittered_mesh_under_a_smooth_field_odd_edges_and_the_order_of_the_rows():
    yx, quads, _ = jitter_case()
    r = jitter_coarse("18.4")
    assert shapes(r) == [(19, 17), (10, 9), (5, 5), (3, 3), (2, 2), (1, 1)]          # odd edges at every level
    assert (r["nin"], r["nout"]) == (1225, 0)
    n0 = r["levels"][0][0]
    print("cells per pixel: max %d, empty pixels %d" % (n0.max(), (n0 == 0).sum()))
    assert n0.sum() == 1225. and n0.max() == 9.
    t = r["table"]
    assert all(lev[0].sum() == 1225. for lev in r["levels"]) and t[5, 0] == 1.
    assert (t[:, 1] >= 1.).sum() >= 4 and (t[:, 5] > 0.).sum() >= 4
    # the same cells in another order: other bits at level 0, because S = S + t runs in ascending index of the rows given
    p = jitter_coarse("perm")
    assert np.array_equal(p["levels"][0][0], n0) and (p["nin"], p["nout"]) == (1225, 0)
    differ = int((bits(p["levels"][0]) != bits(r["levels"][0])).sum())
    print("level-0 values whose bits differ after the permutation: %d" % differ)
    assert differ >= 50
    assert np.allclose(p["levels"][0], r["levels"][0], rtol=1e-12, atol=0.)
    # the top box holds the area of the whole mesh (half the cross product of a quadrangle's diagonals)
    p, q = yx[quads[:, 2]] - yx[quads[:, 0]], yx[quads[:, 3]] - yx[quads[:, 1]]
    assert abs(r["levels"][5][1, 0, 0] - 0.5 * np.abs(p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]).sum()) < 1e-6


def test_clipping_and_a_single_pixel():
    r = jitter_coarse("inner")
    assert shapes(r) == [(9, 7), (5, 4), (3, 2), (2, 1)] and (r["nin"], r["nout"]) == (24, 1201)
    assert r["levels"][0][0].sum() == 24.
    one = jitter_coarse("one")
    assert shapes(one) == [(1, 1), (1, 1)] and (one["nin"], one["nout"]) == (1225, 0)
    assert one["levels"][0][0, 0, 0] == 1225.
    assert all(np.array_equal(bits(one["levels"][0]), bits(lev)) for lev in one["levels"])     # 1 x 1 stays 1 x 1
    assert one["table"][:, 0].tolist() == [1., 1.] and (one["table"][:, 1:] == 0.).all()          # 78400 km^2 < half of 10^6
    yx, quads, _ = jitter_case()
    assert coarse_ref(yx, smooth_move(yx), quads, DAY, ONE_PIXEL, 1, fmin=0.05)["table"][0, 1] == 1.


def test_masks_use_and_degenerate_cells_do_not_contribute():
    yx, quads, _, _ = lattice_case()
    yx1 = strain_move(yx)
    use = np.ones(143, dtype=np.int8)
    use[[3, 70]] = 0
    m0 = np.ones(len(yx), dtype=np.int8)
    m0[quads[10, 2]] = 0
    r = coarse_ref(yx, yx1, quads, STRAIN_T, TIE_GRID, 2, use=use, mask0=m0)
    hit = (quads == quads[10, 2]).any(axis=1)
    assert r["nin"] == 143 - 2 - hit.sum() and r["levels"][0][0].sum() == r["nin"]
    flat = quads.copy()
    flat[20] = flat[20, [0, 1, 1, 0]]
    assert coarse_ref(yx, yx1, flat, STRAIN_T, TIE_GRID, 1)["nin"] == 142
    empty = coarse_ref(yx, yx1, quads[:0], STRAIN_T, TIE_GRID, 3)
    assert (empty["nin"], empty["nout"]) == (0, 0) and (empty["table"] == 0.).all() and all((lev == 0.).all() for lev in empty["levels"])


def big_sizes():
    """what the kernels of sitrk_coarse.hip see of big_case(), from the constants of the source: rows of partials per level, rows
    of counts for the quadrangles and the triangles, and the trips of the loops over them"""
    T = chain_constants()["kCoThreads"]
    shp = _lib.Context.coarse_level_shapes(BIG_GRID[3], BIG_GRID[4], BIG_NLEV)
    rows = [up(a * b, T) for a, b in shp]
    nQ = (BIG_LATTICE[0] - 1) * (BIG_LATTICE[1] - 1)
    return {"T": T, "shapes": shp, "rows": rows, "trips": [up(r, T) for r in rows], "count_rows": (up(nQ, T), up(2 * nQ, T)),
            "count_trips": (up(up(nQ, T), T), up(up(2 * nQ, T), T)), "end_bit": sort_end_bit(BIG_GRID[3] * BIG_GRID[4])}


def check_big_sizes(s):
    """the size conditions of the case, asserted before a device is asked anything"""
    T = s["T"]
    assert s["rows"][0] > T + 64 and s["trips"][0] == 2                   # level 0: a second trip, of more than one wave of lanes
    assert s["rows"][1] > 64 and s["trips"][1] == 1                       # level 1: block_sum gets sums from more than one wave
    assert min(s["count_rows"]) > T + 64 and s["count_trips"] == (2, 3)
    assert s["end_bit"] >= 17 and BIG_NLEV >= 3 and BIG_GRID[3] * BIG_GRID[4] > T * T


def test_big_case_takes_every_reduction_loop_of_the_chain_into_a_second_trip():
    """The size conditions of tests/test_gpu_coarse.py's case of more than 256 rows, from coarse_ref and the constants read from
    sitrk_coarse.hip, without a device.  coarse_ref's loop over the cells is linear: 0.36 s for the 87 000 quadrangles, 0.84 s for
    the 174 000 triangles, measured on the CPU of the development machine; the three pyramids of the case are computed once."""
    s = big_sizes()
    T = s["T"]
    print(s)
    check_big_sizes(s)
    assert s["shapes"] == [(300, 290), (150, 145), (75, 73), (38, 37)] and s["rows"] == [340, 85, 22, 6] and s["end_bit"] == 17
    yx, yx1, quads = big_case()
    assert len(quads) == 87000 and s["count_rows"] == (340, 680)
    r = big_coarse("quads")
    assert r["nin"] + r["nout"] == 87000 and r["nout"] > 1000 and r["nin"] > 70000
    n0 = r["levels"][0][0]
    print("nin %d, nout %d, cells per pixel up to %d, %d empty pixels" % (r["nin"], r["nout"], n0.max(), (n0 == 0).sum()))
    assert n0.max() >= 3 and (n0 == 0).sum() > 1000
    # a pixel's run is not contiguous before the sort: the keys of the cells, in the order given, fall as often as they rise
    inside, j, i, _, _ = centroid_pixels(yx, quads, BIG_GRID)
    key = np.where(inside, j * BIG_GRID[4] + i, BIG_GRID[3] * BIG_GRID[4])
    assert (np.diff(key) < 0).sum() > 40000 and key[inside].max() >= 1 << 16      # keys that need the 17th bit
    # rows of the second trip (level 0: pixels from T*T on) and lanes of the second wave (level 1: boxes from 64 T on) carry
    # boxes with cells, filled boxes, and a share of every moment far above the bound the device's sum is held to
    for l, first in ((0, T * T), (1, 64 * T)):
        share, nsome, nfilled = late_share(r["levels"][l], BIG_GRID[2] * 2. ** l, 0.5, first)
        print("level %d, boxes from %d on: %d with a cell, %d filled; share / bound of the six moments: %s" %
              (l, first, nsome, nfilled, ", ".join("%.3g" % (a / b) for a, b in share)))
        assert nsome > 1000 and nfilled > 1000 and all(a > 1e3 * b for a, b in share)
    assert r["table"][0, 0] == (n0 >= 1.).sum() and r["table"][0, 1] < r["table"][0, 0]
    # the triangles: twice the cells, each with a centroid of its own
    t = big_coarse("tris")
    assert t["nin"] + t["nout"] == 174000 and t["nout"] > 2000 and t["levels"][0][0].sum() == t["nin"]
    # the use mask: one contributing cell less in every trip of the loop over the rows of counts
    use, off, trips = big_use()
    assert trips == [0, 1, 1] and (use == 0).sum() == 3
    u = big_coarse("use")
    assert (u["nin"], u["nout"]) == (r["nin"] - 2, r["nout"] - 1) and u["levels"][0][0].sum() == r["nin"] - 2


# ------------------------------------------------------------------------------------------------ the binding
def test_symbols_are_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert "int %s(sitrk_t *h" % name in txt and name in _lib._SIGNATURES and hasattr(L, name)
    assert "#define SITRK_COARSE_MAXLEV 16" in txt and "#define SITRK_COARSE_NCOLS 8" in txt
    assert _lib.COARSE_MAXLEV == 16 and _lib.COARSE_NCOLS == 8 == len(_lib.COARSE_COLS)
    for name in ("coarse_cells", "mesh_coarse", "coarse_kernel_ms"):
        assert callable(getattr(_lib.Context, name))
    assert callable(sit.IceTracker.mesh_coarse) and callable(sit.CoarseCells) and callable(sit.scaling_exponents)
    assert _lib.Context.coarse_level_shapes(19, 17, 6) == [(19, 17), (10, 9), (5, 5), (3, 3), (2, 2), (1, 1)]


def test_python_argument_checks_come_before_any_device_work(monkeypatch):
    def untouched(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr("sitrack_amd.tracking.default_context", untouched)
    yx, quads = exact_lattice(3, 3, 8.0), ccw_quads(3, 3)
    G = TIE_GRID
    for args, kw in (((yx, yx, quads[:, :2], 1., G, 3), {}), ((yx, yx, quads.astype(float), 1., G, 3), {}), ((yx[:, 0], yx, quads, 1., G, 3), {}),
                     ((yx, yx[:4], quads, 1., G, 3), {}), ((yx, yx, quads, 0., G, 3), {}), ((yx, yx, quads, np.nan, G, 3), {}),
                     ((yx, yx, quads, 1., G, 3), {"use": np.ones(3)}), ((yx, yx, quads, 1., G, 3), {"mask0": np.ones(3)}),
                     ((yx, yx, quads, 1., G, 3), {"mask1": np.ones(8)}), ((yx, yx, quads, 1., (0., 0., -1., 4, 4), 3), {}),
                     ((yx, yx, quads, 1., (0., 0., 1., 2 ** 12, 2 ** 12 + 1), 3), {}), ((yx, yx, quads, 1., G, 0), {}),
                     ((yx, yx, quads, 1., G, 17), {}), ((yx, yx, quads, 1., G, 2.5), {}), ((yx, yx, quads, 1., G, 3), {"fmin": -0.1}),
                     ((yx, yx, quads, 1., G, 3), {"fmin": np.inf}), ((yx, yx, quads, 1., G, 3), {"fmin": "x"})):
        with pytest.raises(ValueError, match="CoarseCells"):
            sit.CoarseCells(*args, **kw)
    # the tracker's method refuses before it reaches its context
    trk = object.__new__(sit.IceTracker)
    for kw in ({"grid": (0., 0., 0., 4, 4)}, {"nlev": 0}, {"nlev": 17}, {"fmin": np.nan}, {"grid": (0., 0., 1., 2 ** 13, 2 ** 12)}):
        with pytest.raises(ValueError, match="mesh_coarse"):
            sit.IceTracker.mesh_coarse(trk, 5, kw.get("grid", G), kw.get("nlev", 3), fmin=kw.get("fmin", 0.5))
    assert co.check_levels((0., 0., 1., 2 ** 12, 2 ** 12), 16, 0., "") == (0., 0., 1., 2 ** 12, 2 ** 12)


# ------------------------------------------------------------------------------------------------ scaling_exponents
def test_scaling_exponents_on_a_table_with_a_known_slope():
    nlev, d = 7, 3.5
    L = d * 2. ** np.arange(nlev)
    beta = np.array([0.15, 0.42, 0.81])
    t = np.zeros((nlev, 8))
    t[:, 1] = [4096, 1024, 256, 64, 16, 4, 1]
    t[:, 0] = t[:, 1] + 3
    t[:, 2] = t[:, 1] * L * L * 0.9
    for q in range(3):
        t[:, 5 + q] = t[:, 2] * 2e-7 ** (q + 1) * L ** -beta[q]
    s = sit.scaling_exponents(t, d)
    assert s["used"].tolist() == [True] * 5 + [False] * 2 and np.allclose(s["beta"], beta, rtol=0., atol=1e-12)
    assert np.array_equal(s["L_km"], L) and np.allclose(s["L_eff_km"], L * math.sqrt(0.9), rtol=1e-15)
    # only the levels with enough filled boxes take part: spoil the two coarsest
    t[5:, 5:] *= 7.
    assert np.allclose(sit.scaling_exponents(t, d)["beta"], beta, rtol=0., atol=1e-12)
    assert not np.allclose(sit.scaling_exponents(t, d, min_boxes=1)["beta"], beta, rtol=0., atol=1e-3)
    # fewer than two levels: NaN; an empty level is never used
    assert np.isnan(sit.scaling_exponents(t, d, min_boxes=2000)["beta"]).all()
    z = np.zeros((3, 8))
    s = sit.scaling_exponents(z, d, min_boxes=0)
    assert np.isnan(s["beta"]).all() and not s["used"].any() and np.isnan(s["L_eff_km"]).all()
    for bad in ((np.zeros((3, 7)), 1.), (np.zeros(8), 1.), (z, 0.), (z, np.nan)):
        with pytest.raises(ValueError, match="scaling_exponents"):
            sit.scaling_exponents(*bad)


# ------------------------------------------------------------------------------------------------ the command line
def test_deform_coarse_flag_parser_and_its_refusals(capsys):
    base = ["-i", "a", "-m", "b", "-s", "c"]
    both = base + ["--deform", "10", "--deform-grid", "12.5"]
    assert drv.parse_args(base).deform_coarse is None and drv.parse_args(both).deform_coarse is None
    assert drv.parse_args(both + ["--deform-coarse", "4"]).deform_coarse == (4, 0.5)
    assert drv.parse_args(both + ["--deform-coarse", "16@0"]).deform_coarse == (16, 0.)
    assert drv.parse_args(both + ["--deform-coarse", "1@2.5e-1"]).deform_coarse == (1, 0.25)
    for bad in ("", "0", "17", "-2", "2.5", "x", "4@", "4@-1", "4@nan", "4@inf", "@0.5", "4@0.5@1", "4,5"):
        with pytest.raises(SystemExit):
            drv.parse_args(both + ["--deform-coarse", bad])
    capsys.readouterr()
    for argv in (base + ["--deform", "10", "--deform-coarse", "4"], base + ["--deform-coarse", "4"]):
        with pytest.raises(SystemExit):
            drv.parse_args(argv)
        assert "--deform-grid" in capsys.readouterr().err
    assert co.coarse_arg("5@0.75") == (5, 0.75)
    with pytest.raises(ValueError, match="--coarse"):
        co.coarse_arg("0")


def test_tool_refuses_coarse_without_grid(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    with pytest.raises(SystemExit, match="--coarse.*--grid"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--coarse", "4"])
    with pytest.raises(SystemExit, match="NLEV"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--grid", "5", "--coarse", "40"])
