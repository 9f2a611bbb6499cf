"""Coarse-grained deformation of buoy cells on the MI355X (sitrk_coarse_cells, sitrk_mesh_coarse, IceTracker.mesh_coarse,
--deform-coarse) against coarse_ref() of tests/test_coarse.py, the numpy restatement of the contract in include/sitrk.h.

The level sums have only + - * / in a pinned order: every comparison of `boxes`, nin, nout and the two counting columns of the
table is bit equality.  There is no tolerance on them anywhere.

Bound of the moments (columns 2..7), that of check_stats in tests/test_gpu_mesh.py: any summation order of n terms is within
(n - 1) 2^-53 sum|t| of the exact sum, and a term rebuilt in numpy from the device's own `boxes` differs from the device's by at
most nine half-ulps -- the four quotients, div, e1, e2 and the sums of squares are + - * / on the same bits and equal, then three
products and two uses of a square root that is within one ulp: |S - fsum(t)| <= (n + 16) 2^-53 fsum|t|, n = the level's filled
boxes."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv
from test_coarse import (BIG_GRID, BIG_NLEV, DAY, ONE_PIXEL, STRAIN_T, TIE_GRID, big_case, big_coarse, big_sizes, big_use, bits, box_terms,
                         check_big_sizes, coarse_ref, jitter_coarse, jitter_perm, late_share, smooth_move, strain_move)
from test_driver import make_case
from test_gpu_mesh import JREC0, K, RDT, advance, start
from test_raster import JITTER_GRIDS, JITTER_INNER, jitter_case, lattice_case, split_quads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = ("div", "shr", "vor", "area0", "area1")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_bits(got, want, what, fmin=0.5, d=None):
    """boxes, nin, nout and the counting columns bit for bit; then the moments of `got` against its own boxes"""
    assert (got["nin"], got["nout"]) == (want["nin"], want["nout"]), what
    assert len(got["levels"]) == len(want["levels"]), what
    for l, (a, b) in enumerate(zip(got["levels"], want["levels"])):
        assert a.shape == b.shape, (what, l)
        bad = np.argwhere(bits(a) != bits(b))
        assert bad.size == 0, "%s level %d: %d values differ, first %s: %r != %r" % (what, l, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])
    assert got["table"].shape == want["table"].shape and np.array_equal(got["table"][:, :2], want["table"][:, :2]), what
    if d is not None:
        check_moments(got, d, fmin, what)


def check_moments(r, d, fmin, what):
    """columns 2..7 of the device's table against math.fsum of the terms rebuilt from the device's own boxes (module docstring)"""
    for l, lev in enumerate(r["levels"]):
        some, filled, t = box_terms(lev, np.float64(d) * 2. ** l, fmin)
        n = int(filled.sum())
        assert (r["table"][l, 0], r["table"][l, 1]) == (some.sum(), n), (what, l)
        for k, row in enumerate(t):
            S, ref, mag = r["table"][l, 2 + k], math.fsum(row), math.fsum(np.abs(row))
            print("%s level %d: %-9s device %.17g  fsum %.17g  |diff| %.3g  bound %.3g" % (what, l, _lib.COARSE_COLS[2 + k], S, ref, abs(S - ref),
                                                                                        (n + 16) * 2. ** -53 * mag))
            assert abs(S - ref) <= (n + 16) * 2. ** -53 * mag, (what, l, _lib.COARSE_COLS[2 + k])
        if n == 0:
            assert (r["table"][l, 1:] == 0.).all(), (what, l)


# ------------------------------------------------------------------------------------------------ 1. ties and the uniform strain
def test_centroids_on_pixel_corners_and_the_uniform_strain(ctx):
    yx, quads, _, _ = lattice_case()
    yx1 = strain_move(yx)
    want = coarse_ref(yx, yx1, quads, STRAIN_T, TIE_GRID, 5)
    got = ctx.coarse_cells(yx, yx1, quads, STRAIN_T, TIE_GRID, 5, boxes=True)
    same_bits(got, want, "lattice", d=8.)
    assert got["levels"][0][0, 0, 0] == 0. and got["levels"][0][0, 1, 1] == 1. and got["table"][:, 0].tolist() == [143., 42., 12., 4., 1.]
    mixed = quads.copy()
    mixed[::3] = mixed[::3, ::-1]                                     # either orientation of the rows
    same_bits(ctx.coarse_cells(yx, yx1, mixed, STRAIN_T, TIE_GRID, 5, boxes=True), want, "lattice, mixed orientation", d=8.)
    same_bits(ctx.coarse_cells(yx, yx1, quads[:, ::-1], STRAIN_T, TIE_GRID, 5, boxes=True), want, "lattice, clockwise", d=8.)
    named = sit.CoarseCells(yx, yx1, quads, STRAIN_T, TIE_GRID, 5, boxes=True, ctx=ctx)
    assert sorted(named) == ["levels", "nin", "nout", "table"] and sorted(named["levels"][0]) == sorted(_lib.COARSE_VALUES)
    assert all(np.array_equal(bits(named["levels"][l][n]), bits(want["levels"][l][k])) for l in range(5) for k, n in enumerate(_lib.COARSE_VALUES))
    assert sit.CoarseCells(yx, yx1, quads, STRAIN_T, TIE_GRID, 5, ctx=ctx)["levels"] is None
    s = sit.scaling_exponents(got["table"], 8., min_boxes=1)
    assert (np.abs(s["beta"]) < 1e-13).all()                          # derived in tests/test_coarse.py
    ms = ctx.coarse_kernel_ms()
    assert len(ms) == 5 and all(x >= 0. for x in ms) and ms[0] > 0. and ms[2] > 0.


# ------------------------------------------------------------------------------------------------ 2. several workgroups, odd edges, order
def test_jittered_mesh_in_order_permuted_twice_and_as_triangles(ctx):
    yx, quads, _ = jitter_case()
    yx1 = smooth_move(yx)
    grid = JITTER_GRIDS[18.4]
    want = jitter_coarse("18.4")
    got = ctx.coarse_cells(yx, yx1, quads, DAY, grid, 6, boxes=True)
    same_bits(got, want, "jitter", d=18.4)
    assert [lev.shape[1:] for lev in got["levels"]] == [(19, 17), (10, 9), (5, 5), (3, 3), (2, 2), (1, 1)] and got["levels"][0][0].max() == 9.
    # a fixed random order of the rows: the bits of the restatement run on that order, which are other bits
    perm = jitter_perm()
    want_p = jitter_coarse("perm")
    got_p = ctx.coarse_cells(yx, yx1, quads[perm], DAY, grid, 6, boxes=True)
    same_bits(got_p, want_p, "jitter, permuted", d=18.4)
    assert (bits(got_p["levels"][0]) != bits(got["levels"][0])).sum() >= 50
    # two calls in a row: the same bits, the table's sums included
    again = ctx.coarse_cells(yx, yx1, quads, DAY, grid, 6, boxes=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again["levels"], got["levels"]))
    assert np.array_equal(bits(again["table"]), bits(got["table"]))
    assert np.array_equal(bits(ctx.coarse_cells(yx, yx1, quads, DAY, grid, 6)["table"]), bits(got["table"]))      # without the pyramid
    # the same cells as 2450 triangles
    tris = split_quads(quads)
    want_t = coarse_ref(yx, yx1, tris, DAY, grid, 6)
    assert want_t["nin"] == 2450
    same_bits(ctx.coarse_cells(yx, yx1, tris, DAY, grid, 6, boxes=True), want_t, "triangles", d=18.4)


# ------------------------------------------------------------------------------------------------ 2b. more than 256 rows of partials
def test_more_than_256_rows_of_partials_and_of_counts(ctx):
    """The loops of coarse_table_kernel and coarse_count_kernel -- lane i takes the rows i, i + kCoThreads, ... -- past their
    first trip, and sort_pairs_u32 on 17 key bits: big_case() of tests/test_coarse.py, 87 000 quadrangles of a 301 x 291 jittered
    lattice in a fixed random order on 300 x 290 pixels of 7.6 km and four levels.  Level 0 has 340 rows of partials (two trips, 84
    lanes in the second), level 1 has 85 (lanes of two waves hold sums when block_sum starts), the terms kernel writes 340 rows
    of counts for the quadrangles and 680 for the triangles (two and three trips).  tests/test_coarse.py proves these sizes, and
    that the boxes behind the first trip are filled, from the restatement alone; it also gives the restatement's CPU times.

    What a wrong second trip breaks.  coarse_table_kernel: a dropped trip loses the 19 117 pixels with a cell from number
    kCoThreads^2 on -- the two counting columns of level 0, compared as integers, are short by that, and each moment by a share
    of more than 1e9 times its bound; a wrong stride takes rows twice or not at all, the same two assertions.  coarse_count_kernel:
    nin and nout are exact against the restatement, and the `use` mask takes one contributing cell out of every trip, so a trip
    that is dropped or counted twice cannot cancel against it.  The sort: a key bit above the 16th left out merges the runs of
    pixels p and p + 65536 -- `boxes` then differ in bits at level 0."""
    s = big_sizes()
    check_big_sizes(s)                                                    # before the device is asked anything
    yx, yx1, quads = big_case()
    d = BIG_GRID[2]
    want = big_coarse("quads")
    assert want["nout"] > 0 and s["end_bit"] >= 17
    for l, first in ((0, s["T"] ** 2), (1, 64 * s["T"])):                 # rows of the second trip, lanes of the second wave
        share, nsome, nfilled = late_share(want["levels"][l], d * 2. ** l, 0.5, first)
        assert nsome > 0 and nfilled > 0 and all(a > 1e3 * b for a, b in share), l
    got =ctx.coarse_cells(yx, yx1, quads, DAY, BIG_GRID, BIG_NLEV, boxes=True)
    same_bits(got, want, "87000 quadrangles", d=d)
    # without `boxes`: the same launches, the same table
    assert np.array_equal(bits(ctx.coarse_cells(yx, yx1, quads, DAY, BIG_GRID, BIG_NLEV)["table"]), bits(got["table"]))
    # the same cells as 174 000 triangles: three trips over the rows of counts
    same_bits(ctx.coarse_cells(yx, yx1, split_quads(quads), DAY, BIG_GRID, BIG_NLEV, boxes=True), big_coarse("tris"), "174000 triangles", d=d)
    # one contributing cell switched off in every trip of the count loop
    use, off, trips = big_use()
    assert trips == [0, 1, 1]
    masked = ctx.coarse_cells(yx, yx1, quads, DAY, BIG_GRID, BIG_NLEV, use=use, boxes=True)
    same_bits(masked, big_coarse("use"), "87000 quadrangles, three switched off", d=d)
    assert (masked["nin"], masked["nout"]) == (got["nin"] - 2, got["nout"] - 1)


# ------------------------------------------------------------------------------------------------ 3., 4. one long run; clipping
def test_a_single_pixel_and_a_grid_inside_the_mesh(ctx):
    yx, quads, _ = jitter_case()
    yx1 = smooth_move(yx)
    one = ctx.coarse_cells(yx, yx1, quads, DAY, ONE_PIXEL, 2, boxes=True)                # a run of 1225 cells, five workgroups of cells
    same_bits(one, jitter_coarse("one"), "one pixel", d=1000.)
    assert one["levels"][0][0, 0, 0] == 1225. and (one["table"][:, 1:] == 0.).all()
    inner = ctx.coarse_cells(yx, yx1, quads, DAY, JITTER_INNER, 4, boxes=True)
    same_bits(inner, jitter_coarse("inner"), "inner", d=JITTER_INNER[2])
    assert (inner["nin"], inner["nout"]) == (24, 1201)


# ------------------------------------------------------------------------------------------------ 5. cells that do not contribute
def test_use_masks_and_degenerate_cells_do_not_contribute(ctx):
    yx, quads, _ = jitter_case()
    yx0, yx1 = yx.copy(), smooth_move(yx)
    grid = JITTER_GRIDS[18.4]
    rng = np.random.default_rng(5)
    use = (rng.random(1225) < 0.6).astype(np.int8)
    cells = quads.copy()
    cells[100] = cells[100, [0, 1, 1, 0]]                             # no area
    yx0[quads[300, 2], 0] = np.nan                                    # a NaN vertex at t0
    yx1[quads[500, 1], 1] = np.inf                                    # an infinite vertex at t1
    m0, m1 = np.ones(len(yx), dtype=np.int8), np.ones(len(yx), dtype=np.int8)
    m0[quads[700, 0]] = 0
    m1[quads[900, 3]] = 0
    use[[100, 300, 500, 700, 900]] = 1
    want = coarse_ref(yx0, yx1, cells, DAY, grid, 6, use=use, mask0=m0, mask1=m1)
    hit = (cells == quads[300, 2]).any(axis=1) | (cells == quads[500, 1]).any(axis=1) | (cells == quads[700, 0]).any(axis=1) | \
        (cells == quads[900, 3]).any(axis=1)
    hit[100] = True
    assert want["nin"] == (use != 0).sum() - (hit & (use != 0)).sum() and (hit & (use != 0)).sum() >= 9 and want["nout"] == 0
    got = ctx.coarse_cells(yx0, yx1, cells, DAY, grid, 6, use=use, mask0=m0, mask1=m1, boxes=True)
    same_bits(got, want, "use and masks", d=18.4)
    # the use mask alone equals the rows it keeps... in the same order
    only = ctx.coarse_cells(yx, smooth_move(yx), quads, DAY, grid, 6, use=use, boxes=True)
    kept = ctx.coarse_cells(yx, smooth_move(yx), quads[use != 0], DAY, grid, 6, boxes=True)
    same_bits(only, kept, "use = the rows kept")
    none = ctx.coarse_cells(yx, yx1, quads, DAY, grid, 3, use=np.zeros(1225), boxes=True)
    assert (none["nin"], none["nout"]) == (0, 0) and (none["table"] == 0.).all() and all((lev == 0.).all() for lev in none["levels"])


# ------------------------------------------------------------------------------------------------ 6. fmin
@pytest.mark.parametrize("fmin", [0., 0.5, 4.])
def test_fmin_decides_which_boxes_are_filled(ctx, fmin):
    yx, quads, _ = jitter_case()
    yx1 = smooth_move(yx)
    got = ctx.coarse_cells(yx, yx1, quads, DAY, JITTER_GRIDS[18.4], 6, fmin=fmin, boxes=True)
    want = jitter_coarse("18.4")                                      # the pyramid does not depend on fmin
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got["levels"], want["levels"]))
    check_moments(got, 18.4, fmin, "fmin %g" % fmin)
    t = got["table"]
    assert np.array_equal(t[:, 0], want["table"][:, 0])
    if fmin == 4.:
        assert (t[:, 1:] == 0.).all()                                 # no box holds four times its own area
    elif fmin == 0.:
        assert np.array_equal(t[:, 1], [((lev[0] >= 1.) & (lev[1] > 0.)).sum() for lev in got["levels"]]) and np.array_equal(t[:, 1], t[:, 0])
    else:
        assert np.array_equal(t[:, 1], want["table"][:, 1]) and (t[:, 1] < t[:, 0]).any() and (t[:, 1] > 0.).sum() >= 4


# ------------------------------------------------------------------------------------------------ 7. no cells, levels beyond 1 x 1
def test_no_cells_and_levels_beyond_the_top(ctx):
    yx, quads, _, _ = lattice_case()
    yx1 = strain_move(yx)
    r = ctx.coarse_cells(yx, yx1, quads[:0], STRAIN_T, TIE_GRID, 3, boxes=True)
    assert (r["nin"], r["nout"]) == (0, 0) and (r["table"] == 0.).all() and [lev.shape for lev in r["levels"]] == [(6, 14, 16), (6, 7, 8), (6, 4, 4)]
    assert all((bits(lev) == 0).all() for lev in r["levels"])       # +0.0
    r = ctx.coarse_cells(np.zeros((0, 2)), np.zeros((0, 2)), quads[:0], STRAIN_T, TIE_GRID, 1, boxes=True)
    assert (r["table"] == 0.).all() and r["table"].shape == (1, 8)
    # nlev beyond the 1 x 1 level: the top box repeats, its side goes on doubling
    want = coarse_ref(yx, yx1, quads, STRAIN_T, TIE_GRID, 8)
    got = ctx.coarse_cells(yx, yx1, quads, STRAIN_T, TIE_GRID, 8, boxes=True)
    same_bits(got, want, "8 levels", d=8.)
    assert [lev.shape[1:] for lev in got["levels"]][4:] == [(1, 1)] * 4 and got["table"][4:, 0].tolist() == [1.] * 4
    assert got["table"][4:, 1].tolist() == [1., 0., 0., 0.]
    same_bits(ctx.coarse_cells(yx, yx1, quads, STRAIN_T, TIE_GRID, 16, boxes=True), coarse_ref(yx, yx1, quads, STRAIN_T, TIE_GRID, 16), "16 levels", d=8.)
    same_bits(ctx.coarse_cells(yx, yx1, quads, STRAIN_T, TIE_GRID, 1, boxes=True), coarse_ref(yx, yx1, quads, STRAIN_T, TIE_GRID, 1), "1 level", d=8.)


# ------------------------------------------------------------------------------------------------ 8. errors
def test_every_error_of_the_contract_leaves_the_handle_usable(ctx):
    yx, quads, _, _ = lattice_case()
    yx = np.ascontiguousarray(yx)
    yx1 = np.ascontiguousarray(strain_move(yx))
    lib, h, p = ctx._L, ctx._h, _lib._ptr
    table = np.full((3, 8), 77.)
    nin, nout = _lib._i64(0), _lib._i64(0)

    def call(nP=len(yx), a=yx, b=yx1, nC=143, nv=4, cells=quads, T=STRAIN_T, y0=-1504., x0=1996., d=8., ny=14, nx=16, nlev=3, fmin=0.5, tab=table):
        return lib.sitrk_coarse_cells(h, nP, p(a), p(b), None, None, nC, nv, p(cells), None, T, y0, x0, d, ny, nx, nlev, fmin, None, p(tab),
                                      C.byref(nin), C.byref(nout))

    for kw, msg in (({"nv": 5}, b"nv must be"), ({"nC": -1}, b"nC must be"), ({"nP": -1}, b"nP must be"), ({"T": 0.}, b"T must be"),
                    ({"T": np.inf}, b"T must be"), ({"y0": np.nan}, b"finite"), ({"x0": np.inf}, b"finite"), ({"d": 0.}, b"d_km"),
                    ({"d": np.nan}, b"d_km"), ({"ny": 0}, b"ny and nx"), ({"nx": -3}, b"ny and nx"), ({"ny": 2 ** 12, "nx": 2 ** 12 + 1}, b"2^24"),
                    ({"nlev": 0}, b"nlev"), ({"nlev": 17}, b"nlev"), ({"fmin": -1e-3}, b"fmin"), ({"fmin": np.nan}, b"fmin"),
                    ({"fmin": np.inf}, b"fmin"), ({"tab": None}, b"null table"), ({"cells": None}, b"null array"), ({"a": None}, b"null array")):
        assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
    assert (table == 77.).all()
    assert call(nP=0) == -2 and b"outside [0, 0)" in lib.sitrk_last_error(h)
    assert call() == 0 and table[0, 0] == 143. and nin.value == 143
    # a vertex index outside the points: IndexError with the count, never dereferenced, and the handle goes on
    bad = quads.copy()
    bad[5, 2] = len(yx)
    bad[77, 0] = -1
    bad[140, 3] = 2 ** 31 - 1
    with pytest.raises(IndexError, match="3 cell\\(s\\) have a vertex index outside \\[0, %d\\)" % len(yx)):
        ctx.coarse_cells(yx, yx1, bad, STRAIN_T, TIE_GRID, 3)
    with pytest.raises(IndexError, match="2 cell"):                   # both halves of quadrangle 5 hold its third vertex
        ctx.coarse_cells(yx, yx1, split_quads(bad)[:20], STRAIN_T, TIE_GRID, 3)
    same_bits(ctx.coarse_cells(yx, yx1, quads, STRAIN_T, TIE_GRID, 5, boxes=True), coarse_ref(yx, yx1, quads, STRAIN_T, TIE_GRID, 5), "after the errors")
    with pytest.raises(ValueError, match="grid"):
        ctx.coarse_cells(yx, yx1, quads, STRAIN_T, (0., 0., 1., 4), 3)
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.SitrkError, match="no coarse-graining call"):
            fresh.coarse_kernel_ms()
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            fresh.mesh_coarse(0, 3, TIE_GRID, 3)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 10. the mesh path
def test_mesh_coarse_equals_coarse_cells_on_the_fetched_positions():
    trk = start()
    try:
        ctx = trk.ctx
        s0 = ctx.fetch()
        trk.mesh(3.5, JREC0)
        trk.mesh(7., JREC0, slot=1)
        cells, cells1 = trk.mesh_cells(), trk.mesh_cells(1)
        jrec1 = advance(trk, JREC0, 3, 3)
        s1 = ctx.fetch()
        T = (jrec1 - JREC0 + 1) * RDT
        before, before1 = trk.mesh_deform(jrec1), trk.mesh_deform(jrec1, slot=1)
        st = before["status"]
        assert min((st == k).sum() for k in range(3)) >= 5 and len(cells) > 256
        lo, hi = s0["yx"].min(axis=0), s0["yx"].max(axis=0)
        grid = sit.raster_grid(lo[0] + 9., hi[0] + 3., lo[1] - 2., hi[1] - 11., 3.1)        # the mesh reaches beyond it on two sides
        owner_before = trk.mesh_raster(jrec1, grid, fields=False)["owner"]
        nlev = 6
        got = trk.mesh_coarse(jrec1, grid, nlev, boxes=True)
        raw = ctx.mesh_coarse(0, jrec1, grid, nlev, boxes=True)
        host = ctx.coarse_cells(s0["yx"], s1["yx"], cells, T, grid, nlev, mask0=s0["alive"], mask1=s1["alive"], use=(st == 1), boxes=True)
        want = coarse_ref(s0["yx"], s1["yx"], cells, T, grid, nlev, mask0=s0["alive"], mask1=s1["alive"], use=(st == 1))
        same_bits(raw, host, "mesh against coarse_cells")
        assert np.array_equal(bits(raw["table"]), bits(host["table"]))                         # the same launches: the same sums
        same_bits(raw, want, "mesh against the restatement", d=grid[2])
        assert sorted(got["levels"][0]) == sorted(_lib.COARSE_VALUES) and np.array_equal(bits(got["table"]), bits(raw["table"]))
        assert all(np.array_equal(bits(got["levels"][l][n]), bits(raw["levels"][l][k])) for l in range(nlev) for k, n in enumerate(_lib.COARSE_VALUES))
        assert raw["nout"] > 0 and raw["nin"] > 100 and raw["nin"] + raw["nout"] == before["stats"]["n1"] == (st == 1).sum()
        assert raw["levels"][0][0].sum() == before["stats"]["n1"] - raw["nout"]
        assert trk.mesh_coarse(jrec1, grid, nlev)["levels"] is None
        assert np.array_equal(bits(trk.mesh_coarse(jrec1, grid, nlev)["table"]), bits(raw["table"]))      # two calls: the same bits
        ms = ctx.coarse_kernel_ms()
        assert all(x >= 0. for x in ms) and ms[0] > 0.
        # mesh_deform and mesh_raster return what they returned before, the other slot and the tracker are where they were
        for slot, was in ((0, before), (1, before1)):
            after = trk.mesh_deform(jrec1, slot=slot)
            assert np.array_equal(after["status"], was["status"]) and all(np.array_equal(bits(after[n]), bits(was[n])) for n in RATES)
            assert [np.float64(after["stats"][n]).view(np.uint64) for n in _lib.MESH_STATS] == \
                   [np.float64(was["stats"][n]).view(np.uint64) for n in _lib.MESH_STATS]
        assert np.array_equal(trk.mesh_raster(jrec1, grid, fields=False)["owner"], owner_before)
        assert np.array_equal(trk.mesh_cells(), cells) and np.array_equal(trk.mesh_cells(1), cells1)
        assert np.array_equal(bits(ctx.fetch()["yx"]), bits(s1["yx"]))
        # the second slot, coarse-grained on its own
        st1 = before1["status"]
        raw1 = ctx.mesh_coarse(1, jrec1, grid, 4, fmin=0.25, boxes=True)
        same_bits(raw1, coarse_ref(s0["yx"], s1["yx"], cells1, T, grid, 4, fmin=0.25, mask0=s0["alive"], mask1=s1["alive"], use=(st1 == 1)),
                  "slot 1", fmin=0.25, d=grid[2])
    finally:
        trk.close()


def test_mesh_coarse_errors_and_the_empty_mesh():
    trk = start()
    try:
        ctx = trk.ctx
        lib, h, p = ctx._L, ctx._h, _lib._ptr
        grid = (-70., -50., 5., 20, 21)
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_coarse(JREC0, grid, 3)
        assert trk.mesh(0.01, JREC0, slot=2)["nQ"] == 0                # an empty mesh: zeros
        ctx.run(JREC0 % K, JREC0, 1)
        r = trk.mesh_coarse(JREC0, grid, 3, slot=2, boxes=True)
        assert (r["nin"], r["nout"]) == (0, 0) and (r["table"] == 0.).all() and r["table"].shape == (3, 8)
        assert [lev["n"].shape for lev in r["levels"]] == [(20, 21), (10, 11), (5, 6)] and all((lev[n] == 0.).all() for lev in r["levels"] for n in lev)
        assert trk.mesh(3.5, JREC0 + 1)["nQ"] > 256
        ctx.run((JREC0 + 1) % K, JREC0 + 1, 1)
        table = np.full((3, 8), 77.)
        n = _lib._i64(0)

        def call(mesh=0, jrec1=JREC0 + 1, y0=-70., x0=-50., d=5., ny=20, nx=21, nlev=3, fmin=0.5, tab=table):
            return lib.sitrk_mesh_coarse(h, mesh, jrec1, y0, x0, d, ny, nx, nlev, fmin, None, p(tab), C.byref(n), None)

        for kw, msg in (({"mesh": 8}, b"mesh must be in 0..7"), ({"mesh": 1}, b"mesh 1 is empty"), ({"jrec1": JREC0}, b"before the mesh's t0"),
                        ({"d": 0.}, b"d_km"), ({"y0": np.nan}, b"finite"), ({"ny": 0}, b"ny and nx"), ({"ny": 2 ** 13, "nx": 2 ** 12}, b"2^24"),
                        ({"nlev": 0}, b"nlev"), ({"nlev": 17}, b"nlev"), ({"fmin": -1.}, b"fmin"), ({"fmin": np.nan}, b"fmin"), ({"tab": None}, b"null table")):
            assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
        assert (table == 77.).all()
        assert call() == 0 and table[0, 0] > 0. and n.value > 0
        ctx.run((JREC0 + 2) % K, JREC0 + 2, 1)                          # the handle goes on
        assert np.isfinite(ctx.fetch()["yx"]).all()
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ 11. command line
def test_cli_deform_coarse_flag(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200)
    replay = {}

    class Replaying(sit.IceTracker):
        """the driver's tracker in a run WITHOUT the flag: every mesh_raster is followed by a mesh_coarse of the test's own"""
        def mesh_raster(self, jrec1, grid, slot=0, at="t0", fields=True):
            got = super().mesh_raster(jrec1, grid, slot=slot, at=at, fields=fields)
            replay[(slot, jrec1)] = (super().mesh_coarse(jrec1, grid, 4, slot=slot), super().mesh_deform(jrec1, slot=slot), grid)
            return got

    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F", "--deform", "30", "--deform-window", "5", "--deform-grid", "10"]
    out = drv.main(argv + ["--deform-coarse", "4"])
    log = capsys.readouterr().out
    with np.load(out["files"][2]) as z:
        d = {k: z[k] for k in z.files}
    monkeypatch.setattr(drv, "IceTracker", Replaying)
    plain = drv.main(argv)                                            # an independent run, without the flag
    assert "--deform-coarse" not in capsys.readouterr().out
    with np.load(plain["files"][2]) as z:
        e = {k: z[k] for k in z.files}
    new = ["coarse"] + ["m0_w%d_coarse" % w for w in range(3)]
    assert sorted(d) == sorted(list(e) + new) and not any("coarse" in k for k in e)
    for k in e:                                                       # everything else is what it was
        assert np.array_equal(d[k], e[k]), k
    assert d["coarse"].tolist() == [4., 0.5] and len(replay) == 3
    kstrt = out["kstrt"]
    for w, jrec1 in enumerate((kstrt + 4, kstrt + 9, kstrt + 13)):
        tab = d["m0_w%d_coarse" % w]
        mine, deform, grid = replay[(0, jrec1)]
        assert tuple(d["grid"]) == tuple(grid) and tab.shape == (4, 8) and tab.dtype == np.float64
        assert np.array_equal(bits(tab), bits(mine["table"])), w
        assert tab[0, 0] > 10. and tab[0, 2] > 0. and mine["nin"] + mine["nout"] == deform["stats"]["n1"]
        beta = sit.scaling_exponents(tab, d["grid"][2])["beta"]
        line = [ln for ln in log.splitlines() if "--deform-coarse window %d mesh 0" % w in ln]
        assert len(line) == 1 and "beta(1..3) = " + ", ".join("%.4f" % b for b in beta) in line[0], line
    # tools/deformation.py --grid --coarse on the written series: the table of sit.CoarseCells on the file's positions
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    t, ids, _, yx_all, mk = ncio.LoadNCdata(out["files"][0], krec=-1, lmask=True)
    index_of = {int(v): k for k, v in enumerate(ids)}
    cells = np.array([[index_of[int(v)] for v in row] for row in d["m0_w0_cells"]], dtype=np.int32).reshape(-1, 4)
    fc, fout = str(tmp_path / "cells.npy"), str(tmp_path / "curve.npz")
    np.save(fc, d["m0_w0_cells"])
    assert tool.main(["-i", out["files"][0], "-c", fc, "-k", "0", "-K", "5", "--grid", "7.5", "--coarse", "3@0.25", "-o", fout]) == 0
    assert "--coarse 3 levels, fmin 0.25" in capsys.readouterr().out
    with np.load(fout) as z:
        m = {k: z[k] for k in z.files}
    yx0, yx5 = yx_all[0].astype(np.float64), yx_all[5].astype(np.float64)
    g = sit.raster_grid(yx0[:, 0].min(), yx0[:, 0].max(), yx0[:, 1].min(), yx0[:, 1].max(), 7.5)
    assert (mk[0] == 1).all() and tuple(m["grid"]) == g and m["coarse"].tolist() == [3., 0.25] and m["coarse_table"].shape == (3, 8)
    mine = sit.CoarseCells(yx0, yx5, cells, float(t[5] - t[0]), g, 3, fmin=0.25, mask1=mk[5])
    assert np.array_equal(bits(m["coarse_table"]), bits(mine["table"]))
    assert mine["nin"] + mine["nout"] == m["valid"].sum() >= 50 and m["coarse_table"][0, 0] >= 10.
    assert np.array_equal(m["beta"], sit.scaling_exponents(mine["table"], 7.5)["beta"], equal_nan=True)
