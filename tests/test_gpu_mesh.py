"""Device-resident quadrangle meshes on the MI355X (sitrk_mesh_*, IceTracker.mesh*, --deform) against the host-array chain they
replace -- sitrk_delaunay -> sitrk_tri2quad -> sitrk_deform_mark / sitrk_deform_since_mark -- and against the numpy restatements
of tests/test_delaunay.py, tests/test_tri2quad.py and tests/test_mesh.py.

The base case is tracked_case() of tests/test_gpu_deform.py: 600 buoys on a jittered 3.5-km lattice, two records stepped, the
mesh built with rmax_km = 3.5, six more records with a re-sort after the third.  Its sizes put more than one 1024-triangle
compaction block and more than one workgroup of the cell kernel (hence more than one row of partial sums) into every test; that,
and cells of all three statuses, is asserted from the restatements, not assumed.

Bound of the sums (test 3): any summation order of n1 terms is within (n1 - 1) 2^-53 sum|t| of the exact sum, and a term rebuilt
in numpy from the device's own `out` differs from the device's by at most nine half-ulps (three products and three uses of a
square root that is within one ulp): |S - fsum(t)| <= (n1 + 16) 2^-53 fsum|t|."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv
from sitrack_amd import synthetic as syn
from test_delaunay import delaunay_fast
from test_deform import FILL
from test_driver import make_case
from test_gpu_deform import bits, same_as, tracked_case
from test_mesh import mesh_deform_ref, stat_terms
from test_coarse import coarse_ref
from test_tri2quad import chain_constants, tri2quad_ref, tri2quad_rounds, up

pytestmark = pytest.mark.gpu
K, KSTRT, RDT = 8, 3, 3600.
JREC0 = KSTRT + 2
RATES = ("div", "shr", "vor", "area0", "area1")


def cloud(ny=25, nx=24):
    """tracked_case(), or a larger cloud of the same make"""
    grid, u, v, sic, yx, ji = tracked_case()
    if (ny, nx) != (25, 24):
        j, i = np.meshgrid(np.arange(ny) - 0.5 * (ny - 1), np.arange(nx) - 0.5 * (nx - 1), indexing="ij")
        yx = np.stack([-20. + 3.5 * j.ravel(), 3.5 * i.ravel()], axis=1) + np.random.default_rng(3).uniform(-0.8, 0.8, (ny * nx, 2))
        ji = syn.regular_host_cell(grid, yx)
    return grid, u, v, sic, yx, ji


DENSE_N, DENSE_KM = 340, 0.5


def dense_cloud(n=DENSE_N, spacing=DENSE_KM):
    """cloud()'s make at another scale: n x n points `spacing` km apart about the same centre, jittered by the same fraction of
    the spacing.  The mesh is then built with rmax_km = spacing.  340 x 340 at 0.5 km are 115 600 buoys on 170 km of the 256-km
    domain, some 10 000 of them on the block of land."""
    grid, u, v, sic, _, _ = tracked_case()
    j, i = np.meshgrid(np.arange(n) - 0.5 * (n - 1), np.arange(n) - 0.5 * (n - 1), indexing="ij")
    jit = 0.8 / 3.5 * spacing
    yx = np.stack([-20. + spacing * j.ravel(), spacing * i.ravel()], axis=1) + np.random.default_rng(3).uniform(-jit, jit, (n * n, 2))
    return grid, u, v, sic, yx, syn.regular_host_cell(grid, yx)


def start(ny=25, nx=24, first=None, last=None, case=None):
    """a tracker on the case, two records stepped from KSTRT: the next record is JREC0"""
    grid, u, v, sic, yx, ji = case or cloud(ny, nx)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=RDT, nslots=K)
    for k in range(K):
        trk.load_record(k, u[k], v[k], sic[k])
    trk.set_buoys(yx, ji, first, last)
    trk.ctx.set_resort(0)
    trk.ctx.run(KSTRT % K, KSTRT, 2)
    return trk


def advance(trk, jrec0, n_before_sort, n_after_sort):
    """records jrec0 .. with a re-sort in between; returns the last record stepped"""
    trk.ctx.run(jrec0 % K, jrec0, n_before_sort)
    trk.ctx.sort_buoys()
    if n_after_sort:
        trk.ctx.run((jrec0 + n_before_sort) % K, jrec0 + n_before_sort, n_after_sort)
    return jrec0 + n_before_sort + n_after_sort - 1


def host_chain(ctx, s, rmax, mask=None):
    """the host-array chain on fetched positions: (tris, quads, rounds)"""
    m = (s["alive"] != 0) if mask is None else ((s["alive"] != 0) & (np.asarray(mask) != 0))
    tris, nT, _ = ctx.delaunay(s["yx"], rmax, mask=m)
    quads, _, rounds = ctx.tri2quad(s["yx"], tris, mask=m)
    return tris, quads, rounds


def same_rates(r, o2, v2, what):
    """mesh_deform's dict against (out, valid) of sitrk_deform_since_mark: + - * / bit-equal, shr within one ulp, status != 0 = valid"""
    assert np.array_equal(r["status"] != 0, v2), what
    for row, name in enumerate(RATES):
        if name == "shr":
            d = np.abs(r[name][v2] - o2[row][v2])
            assert (d <= np.spacing(np.abs(o2[row][v2]))).all() and (r[name][~v2] == FILL).all(), (what, name)
        else:
            assert np.array_equal(bits(r[name]), bits(o2[row])), (what, name)


def check_stats(r, what):
    """status and stats consistent with out: counts exact, FILL where status is 0, every sum within the derived bound of the
    exactly rounded sum of the terms rebuilt from the device's own out"""
    out = np.stack([r[n] for n in RATES])
    st, stats = r["status"], np.array([r["stats"][n] for n in _lib.MESH_STATS])
    assert [stats[k] for k in range(3)] == [(st == k).sum() for k in range(3)], what
    assert (out[:, st == 0] == FILL).all() and (out[:, st != 0] != FILL).all(), what
    n1 = int((st == 1).sum())
    for k, t in enumerate(stat_terms(out, st)):
        S, ref, mag = stats[3 + k], math.fsum(t), math.fsum(np.abs(t))
        print("%s: %-10s device %.17g  fsum %.17g  |diff| %.3g  bound %.3g" % (what, _lib.MESH_STATS[3 + k], S, ref, abs(S - ref),
                                                                          (n1 + 16) * 2. ** -53 * mag))
        assert abs(S - ref) <= (n1 + 16) * 2. ** -53 * mag, (what, _lib.MESH_STATS[3 + k])


# ------------------------------------------------------------------------------------------------ 1. build
def test_build_equals_the_host_array_chain():
    trk = start()
    try:
        ctx = trk.ctx
        s = ctx.fetch()
        r = trk.mesh(3.5, JREC0)
        cells = trk.mesh_cells()
        tris, quads, rounds = host_chain(ctx, s, 3.5)
        assert cells.dtype == np.int32 and cells.shape == quads.shape and np.array_equal(cells, quads)
        assert r == {"nT": len(tris), "nQ": len(quads), "rounds": rounds}
        # ... and the restatements
        rt, _ = delaunay_fast(s["yx"], 3.5, s["alive"])
        rq, _, rr = tri2quad_rounds(s["yx"], rt, s["alive"])
        assert len(rt) > 1024 and len(rq) > 256                      # two compaction blocks, two workgroups of the cell kernel
        assert np.array_equal(rq, tri2quad_ref(s["yx"], rt, s["alive"])[0])
        assert np.array_equal(cells, rq) and r == {"nT": len(rt), "nQ": len(rq), "rounds": rr}
        assert np.array_equal(trk.mesh_cells(), cells) and np.array_equal(ctx.fetch()["yx"], s["yx"])      # nothing was moved
        ms = ctx.mesh_kernel_ms(deform=False)
        assert ms[0] > 0. and ms[1:] == (None, None, None)
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ 2. deform = deform_since_mark
@pytest.mark.parametrize("windows", [False, True])
def test_deform_equals_deform_since_mark(windows):
    nP = 600
    first = last = None
    if windows:
        rng = np.random.default_rng(8)
        first = np.full(nP, KSTRT, dtype=np.int64)
        last = np.full(nP, KSTRT + 20, dtype=np.int64)
        w = rng.permutation(nP)
        first[w[:15]] = KSTRT + 3                              # start inside the span
        last[w[15:30]] = KSTRT + 5                             # stop inside it
        last[w[30:40]] = KSTRT + 7                             # stop with its last record: valid
    trk = start(first=first, last=last)
    try:
        ctx = trk.ctx
        trk.deform_mark(JREC0)
        r0 = trk.mesh(3.5, JREC0)
        cells = trk.mesh_cells()
        assert r0["nQ"] == len(cells) > 256
        jrec1 = advance(trk, JREC0, 3, 3)
        assert jrec1 == KSTRT + 7
        r = trk.mesh_deform(jrec1)
        o2, v2, nvalid = ctx.deform_since_mark(jrec1, cells)
        assert 0 < nvalid < len(cells)
        same_rates(r, o2, v2, "windows" if windows else "plain")
        check_stats(r, "windows" if windows else "plain")
        if windows:                                              # vertices that fall out of the span take their cells with them
            s1 = ctx.fetch()
            out_of_span = (s1["alive"] == 1) & ~((first <= JREC0) & (last >= jrec1))
            hit = out_of_span[cells].any(axis=1)
            assert hit.sum() >= 5 and (r["status"][hit] == 0).all()
            assert (r["status"][(last[cells] == KSTRT + 7).any(axis=1) & ~hit] != 0).any()
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ 3. status and stats
def test_status_and_stats_equal_the_restatement():
    trk = start()
    try:
        ctx = trk.ctx
        s0 = ctx.fetch()
        trk.mesh(3.5, JREC0)
        cells = trk.mesh_cells()
        jrec1 = advance(trk, JREC0, 3, 3)
        s1 = ctx.fetch()
        T = (jrec1 - JREC0 + 1) * RDT
        ro, rs, rstats = mesh_deform_ref(s0["yx"], s1["yx"], cells, T, s0["alive"], s1["alive"])
        assert min((rs == k).sum() for k in range(3)) >= 5           # cells of all three statuses
        r = trk.mesh_deform(jrec1)
        assert r["status"].dtype == np.int8 and np.array_equal(r["status"], rs)
        same_as((np.stack([r[n] for n in RATES]), r["status"] != 0), (ro, rs != 0), "mesh")
        assert [r["stats"][n] for n in ("n0", "n1", "n2")] == rstats[:3].tolist()
        check_stats(r, "base case")
        # against the restatement's own sums too: its terms differ from the device's by the same nine half-ulps at most
        n1 = int((rs == 1).sum())
        for k, t in enumerate(stat_terms(ro, rs)):
            assert abs(r["stats"][_lib.MESH_STATS[3 + k]] - rstats[3 + k]) <= (n1 + 16) * 2. ** -53 * math.fsum(np.abs(t)), k
        # two calls in a row return the same bits; the stats alone are the same bits
        again = trk.mesh_deform(jrec1)
        for n in RATES:
            assert np.array_equal(bits(again[n]), bits(r[n])), n
        assert np.array_equal(again["status"], r["status"])
        as_bits = lambda d: [np.float64(d[n]).view(np.uint64) for n in _lib.MESH_STATS]      # noqa: E731
        assert as_bits(again["stats"]) == as_bits(r["stats"])
        only = trk.mesh_deform(jrec1, full=False)
        assert sorted(only) == sorted(_lib.MESH_STATS) and as_bits(only) == as_bits(r["stats"])
        raw = ctx.mesh_deform(0, jrec1, want="status")
        assert sorted(raw) == ["status"] and np.array_equal(raw["status"], rs)
        ms = ctx.mesh_kernel_ms()
        assert all(x >= 0. for x in ms) and ms[2] > 0.
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ 4. several meshes, the mask
def test_several_meshes_and_the_mask():
    trk = start()
    try:
        ctx = trk.ctx
        trk.mesh(3.5, JREC0, slot=0)
        cells0 = trk.mesh_cells(0)
        jrec1 = advance(trk, JREC0, 3, 3)
        r0 = trk.mesh_deform(jrec1, slot=0)
        # slot 1: every other lattice row and column, a wider bound, built later
        mask = np.zeros((25, 24), dtype=np.int8)
        mask[::2, ::2] = 1
        mask = mask.ravel()
        s = ctx.fetch()
        trk.deform_mark(jrec1 + 1)
        r1 = trk.mesh(7., jrec1 + 1, slot=1, mask=mask)
        cells1 = trk.mesh_cells(1)
        tris, quads, rounds = host_chain(ctx, s, 7., mask)
        assert r1 == {"nT": len(tris), "nQ": len(quads), "rounds": rounds} and np.array_equal(cells1, quads)
        rt, _ = delaunay_fast(s["yx"], 7., (s["alive"] != 0) & (mask != 0))
        assert np.array_equal(cells1, tri2quad_ref(s["yx"], rt, (s["alive"] != 0) & (mask != 0))[0]) and len(cells1) >= 50
        assert (mask[cells1] == 1).all() and (s["alive"][cells1] == 1).all()
        # slot 0 is as it was
        assert np.array_equal(trk.mesh_cells(0), cells0)
        again = trk.mesh_deform(jrec1, slot=0)
        for n in RATES:
            assert np.array_equal(bits(again[n]), bits(r0[n])), n
        assert np.array_equal(again["status"], r0["status"]) and again["stats"] == r0["stats"]
        # slot 1 over three more records
        jrec2 = advance(trk, jrec1 + 1, 1, 2)
        r = trk.mesh_deform(jrec2, slot=1)
        o2, v2, _ = ctx.deform_since_mark(jrec2, cells1)
        same_rates(r, o2, v2, "slot 1")
        check_stats(r, "slot 1")
        trk.mesh_free(1)
        with pytest.raises(_lib.SitrkError, match="mesh 1 is empty"):
            trk.mesh_deform(jrec2, slot=1)
        assert np.array_equal(trk.mesh_cells(0), cells0)
    finally:
        trk.close()


def test_a_mesh_of_more_than_1024_quadrangles():
    trk = start(40, 40)
    try:
        ctx = trk.ctx
        s = ctx.fetch()
        trk.deform_mark(JREC0)
        r = trk.mesh(3.5, JREC0)
        cells = trk.mesh_cells()
        tris, quads, rounds = host_chain(ctx, s, 3.5)
        assert r == {"nT": len(tris), "nQ": len(quads), "rounds": rounds} and np.array_equal(cells, quads)
        rt, _ = delaunay_fast(s["yx"], 3.5, s["alive"])
        rq, _ = tri2quad_ref(s["yx"], rt, s["alive"])
        assert len(rq) > 1024 and np.array_equal(cells, rq)
        jrec1 = advance(trk, JREC0, 3, 3)
        res = trk.mesh_deform(jrec1)
        o2, v2, _ = ctx.deform_since_mark(jrec1, cells)
        same_rates(res, o2, v2, "40 x 40")
        check_stats(res, "40 x 40")
        s1 = ctx.fetch()
        _, rs, _ = mesh_deform_ref(s["yx"], s1["yx"], cells, (jrec1 - JREC0 + 1) * RDT, s["alive"], s1["alive"])
        assert np.array_equal(res["status"], rs)
    finally:
        trk.close()


def late_terms(terms, index, first, n):
    """[(|exactly rounded sum of the terms of the cells of index >= first|, the bound (n + 16) 2^-53 fsum|t| over all terms)] of
    the rows of `terms`, whose columns belong to the cells `index`"""
    late = np.asarray(index) >= first
    return [(abs(math.fsum(t[late])), (n + 16) * 2. ** -53 * math.fsum(np.abs(t))) for t in terms]


def test_a_mesh_of_more_than_256_rows_of_partial_sums():
    """mesh_sum_kernel -- lane l takes the rows l, l + kMeshThreads, ... of mesh_cells_kernel's partial sums -- past its first
    trip, and with it the SRC = 1 path of coarse_terms_kernel and coarse_count_kernel past 256 rows of counts: dense_cloud(), 340 x
    340 buoys 0.5 km apart, gives a mesh of more than 70 000 quadrangles, more than 273 rows.  The cells are held to the
    host-array chain on the same handle (the numpy Delaunay restatement is pinned past its caps by tests/test_cloud_trips.py),
    status, counts and rates to mesh_deform_ref on the fetched positions (0.1 s at this size), the sums to check_stats' bound.

    What a wrong second trip breaks: a dropped trip loses the cells from number kMeshThreads^2 on -- n0, n1 and n2, compared as
    integers, are short by them, and each of the seven sums by a share that is asserted to be more than 1000 times its bound; a
    wrong stride takes rows twice or not at all, the same assertions.  For sitrk_mesh_coarse nin + nout must equal n1."""
    from test_gpu_coarse import same_bits                             # that module imports this one
    c = chain_constants()
    T = c["kMeshThreads"]
    assert 70000 >= T * T + 16 * T and up(up(70001, T), T) == 2 and c["kCoThreads"] * (c["kCoThreads"] + 16) <= 70000
    trk = start(case=dense_cloud())
    try:
        ctx = trk.ctx
        s0 = ctx.fetch()
        trk.deform_mark(JREC0)
        r = trk.mesh(DENSE_KM, JREC0)
        assert r["nQ"] > 70000, r                                     # the device's count: more than kMeshThreads + 16 rows
        cells = trk.mesh_cells()
        tris, quads, rounds = host_chain(ctx, s0, DENSE_KM)
        assert r == {"nT": len(tris), "nQ": len(quads), "rounds": rounds} and np.array_equal(cells, quads)
        jrec1 = advance(trk, JREC0, 3, 3)
        s1 = ctx.fetch()
        Tsec = (jrec1 - JREC0 + 1) * RDT
        ro, rs, rstats = mesh_deform_ref(s0["yx"], s1["yx"], cells, Tsec, s0["alive"], s1["alive"])
        counts = [int((rs == k).sum()) for k in range(3)]
        late = [int((rs[T * T:] == k).sum()) for k in range(3)]
        print("nQ %d in %d rows; status 0/1/2: %r, of the cells from %d on: %r" % (len(cells), up(len(cells), T), counts, T * T, late))
        assert min(counts) >= 5 and late[1] >= 100                       # all three statuses; status 1 in the second trip
        n1 = counts[1]
        share = late_terms(stat_terms(ro, rs), np.flatnonzero(rs == 1), T * T, n1)
        assert all(a > 1e3 * b for a, b in share), share
        res = trk.mesh_deform(jrec1)
        assert res["status"].dtype == np.int8 and np.array_equal(res["status"], rs)
        assert [res["stats"][n] for n in ("n0", "n1", "n2")] == rstats[:3].tolist() == counts
        same_as((np.stack([res[n] for n in RATES]), res["status"] != 0), (ro, rs != 0), "dense mesh")
        check_stats(res, "dense mesh")
        o2, v2, _ = ctx.deform_since_mark(jrec1, cells)
        same_rates(res, o2, v2, "dense mesh")
        # two calls in a row and the stats alone: the same bits
        as_bits = lambda d: [np.float64(d[n]).view(np.uint64) for n in _lib.MESH_STATS]      # noqa: E731
        again = trk.mesh_deform(jrec1)
        assert np.array_equal(again["status"], res["status"]) and all(np.array_equal(bits(again[n]), bits(res[n])) for n in RATES)
        assert as_bits(again["stats"]) == as_bits(res["stats"])
        only = trk.mesh_deform(jrec1, full=False)
        assert sorted(only) == sorted(_lib.MESH_STATS) and as_bits(only) == as_bits(res["stats"])
        # sitrk_mesh_coarse on this mesh = sitrk_coarse_cells on the fetched positions = the restatement
        lo, hi = s0["yx"].min(axis=0), s0["yx"].max(axis=0)
        grid = sit.raster_grid(lo[0] + 9., hi[0] + 3., lo[1] - 2., hi[1] - 11., 0.45)        # the mesh reaches beyond it on two sides
        nlev = 4
        assert grid[3] * grid[4] > c["kCoThreads"] ** 2
        raw = ctx.mesh_coarse(0, jrec1, grid, nlev, boxes=True)
        host = ctx.coarse_cells(s0["yx"], s1["yx"], cells, Tsec, grid, nlev, mask0=s0["alive"], mask1=s1["alive"], use=(rs == 1), boxes=True)
        want = coarse_ref(s0["yx"], s1["yx"], cells, Tsec, grid, nlev, mask0=s0["alive"], mask1=s1["alive"], use=(rs == 1))
        same_bits(raw, host, "dense mesh against coarse_cells")
        assert np.array_equal(bits(raw["table"]), bits(host["table"]))                         # the same launches: the same sums
        same_bits(raw, want, "dense mesh against the restatement", d=grid[2])
        assert raw["nout"] > 0 and raw["nin"] > 100 and raw["nin"] + raw["nout"] == n1 and up(len(cells), c["kCoThreads"]) > c["kCoThreads"]
        assert np.array_equal(bits(ctx.mesh_coarse(0, jrec1, grid, nlev)["table"]), bits(raw["table"]))
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ 5. mesh_mark
def test_mesh_mark_takes_the_positions_again():
    trk = start()
    try:
        ctx = trk.ctx
        s0 = ctx.fetch()
        trk.mesh(3.5, JREC0)
        cells = trk.mesh_cells()
        jrec1 = advance(trk, JREC0, 3, 3)
        trk.mesh_deform(jrec1)
        jrec0b = jrec1 + 1
        trk.mesh_mark(jrec0b)
        trk.deform_mark(jrec0b)
        s0b = ctx.fetch()
        jrec1b = advance(trk, jrec0b, 1, 2)
        s1b = ctx.fetch()
        r = trk.mesh_deform(jrec1b)
        o2, v2, _ = ctx.deform_since_mark(jrec1b, cells)
        same_rates(r, o2, v2, "re-marked")
        check_stats(r, "re-marked")
        assert np.array_equal(trk.mesh_cells(), cells) and v2.any()
        Tb = (jrec1b - jrec0b + 1) * RDT
        _, rs, _ = mesh_deform_ref(s0b["yx"], s1b["yx"], cells, Tb, s0b["alive"], s1b["alive"])
        assert np.array_equal(r["status"], rs)
        dead_at_mark = (s0b["alive"] == 0)[cells].any(axis=1)
        assert dead_at_mark.any() and (r["status"][dead_at_mark] == 0).all()       # NaN at t0: invalid from then on
        stale, sv, _ = ctx.deform_cells(s0["yx"], s1b["yx"], cells, Tb, s0["alive"], s1b["alive"])
        assert not np.array_equal(bits(stale[0]), bits(r["div"]))
        with pytest.raises(_lib.SitrkError, match="before the mesh's t0"):
            trk.mesh_deform(jrec1)
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ 6. empty and error paths
def test_empty_and_error_paths_leave_the_handle_usable():
    trk = start()
    try:
        ctx = trk.ctx
        lib, h, p = ctx._L, ctx._h, _lib._ptr
        nxt = [JREC0]

        def still_works():
            ctx.run(nxt[0] % K, nxt[0], 1)
            nxt[0] += 1
            assert np.isfinite(ctx.fetch()["yx"]).all()

        # an empty mesh
        assert trk.mesh(0.01, JREC0, slot=2) == {"nT": 0, "nQ": 0, "rounds": 0}
        cells = trk.mesh_cells(2)
        assert cells.shape == (0, 4) and cells.dtype == np.int32
        still_works()
        r = trk.mesh_deform(nxt[0] - 1, slot=2)
        assert all(r[n].shape == (0,) for n in RATES) and r["status"].shape == (0,) and set(r["stats"].values()) == {0.}
        trk.mesh_mark(nxt[0], slot=2)
        # the slot number
        nT, nQ, rounds = _lib._i64(0), _lib._i64(0), _lib._int(0)
        out, status, stats = np.empty((5, 4)), np.empty(4, dtype=np.int8), np.empty(10)
        for bad in (-1, 8):
            assert lib.sitrk_mesh_build(h, bad, JREC0, 3.5, None, 0.5, -0.5, 0.5, 0., float("inf"), C.byref(nT), C.byref(nQ), C.byref(rounds)) == -1
            assert b"mesh must be in 0..7" in lib.sitrk_last_error(h)
            assert lib.sitrk_mesh_deform(h, bad, JREC0, p(out), p(status), p(stats)) == -1
            assert lib.sitrk_mesh_cells(h, bad, 0, None, C.byref(nQ)) == -1 and lib.sitrk_mesh_mark(h, bad, JREC0) == -1
            assert lib.sitrk_mesh_free(h, bad) == -1
            still_works()
        # the checks of the two calls it stands for, before any device work
        for rmax in (0., -1., 501., float("nan")):
            with pytest.raises(_lib.SitrkError, match="rmax_km"):
                ctx.mesh_build(0, JREC0, rmax)
        with pytest.raises(_lib.SitrkError, match="cos_lo"):
            ctx.mesh_build(0, JREC0, 3.5, cos_lo=-0.5, cos_hi=0.5)
        with pytest.raises(_lib.SitrkError, match="ratio_min"):
            ctx.mesh_build(0, JREC0, 3.5, ratio_min=1.5)
        with pytest.raises(_lib.SitrkError, match="area_min"):
            ctx.mesh_build(0, JREC0, 3.5, area_min=2., area_max=1.)
        with pytest.raises(ValueError, match="`rmax_km`"):
            trk.mesh(float("nan"), JREC0)
        with pytest.raises(ValueError, match="`mask`"):
            trk.mesh(3.5, JREC0, mask=np.ones(5))
        still_works()
        # a slot never built, a freed slot
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_deform(nxt[0] - 1)
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_cells()
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_mark(nxt[0])
        still_works()
        j0 = nxt[0]
        assert trk.mesh(3.5, j0)["nQ"] > 256
        with pytest.raises(_lib.SitrkError, match="before the mesh's t0"):
            trk.mesh_deform(j0 - 1)
        assert lib.sitrk_mesh_deform(h, 0, j0, None, None, None) == -1 and b"all null" in lib.sitrk_last_error(h)
        still_works()
        assert trk.mesh_deform(j0)["stats"]["n1"] > 0
        nq = _lib._i64(0)                                             # cap < nQ: only the count
        assert lib.sitrk_mesh_cells(h, 0, 3, p(np.full((3, 4), -7, dtype=np.int32)), C.byref(nq)) == 0 and nq.value > 256
        trk.mesh_free(0)
        trk.mesh_free(0)                                              # freeing an empty slot is no error
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_deform(j0)
        still_works()
        # set_buoys empties every slot
        trk.mesh(3.5, nxt[0], slot=5)
        grid, u, v, sic, yx, ji = cloud()
        trk.set_buoys(yx, ji)
        for slot in range(_lib.MESH_MAX):
            with pytest.raises(_lib.SitrkError, match="mesh %d is empty" % slot):
                trk.mesh_cells(slot)
        ctx.run(KSTRT % K, KSTRT, 1)
        assert np.isfinite(ctx.fetch()["yx"]).all()
    finally:
        trk.close()
    # a context without buoys
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.mesh_build(0, 3, 3.5)
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.mesh_deform(0, 3)
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.mesh_cells(0)
        assert ctx._L.sitrk_mesh_free(ctx._h, 0) == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 7. command line
def test_cli_deform_flag(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200)
    RMAX, RD, NWIN = 15., 18., 5
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F"]
    plain = drv.main(argv)
    t, ids, _, yx_plain, mk_plain = ncio.LoadNCdata(plain["files"][0], krec=-1, lmask=True)
    capsys.readouterr()
    out = drv.main(argv + ["--deform", "%g,%g@%g" % (RMAX, 2 * RMAX, RD), "--deform-window", str(NWIN)])
    log = capsys.readouterr().out
    Nt, kstrt = out["Nt"], out["kstrt"]
    assert Nt == 14 and len(out["files"]) == 3 and out["files"][:2] == plain["files"]
    fd = out["files"][2]
    assert fd == './npz/NEMO-SI3_TEST4_EXP01_deformation_nemoTsi3_idlSeed_19961215h00_19961215h14.npz' and os.path.exists(fd)
    # the positions of the series are what they were without the flag
    _, ids2, _, yx2, mk2 = ncio.LoadNCdata(out["files"][0], krec=-1, lmask=True)
    assert np.array_equal(ids2, ids) and np.array_equal(mk2, mk_plain) and np.array_equal(bits(yx2), bits(yx_plain))
    assert np.array_equal(out["vJIt"], plain["vJIt"]) and np.array_equal(out["iAlive"], plain["iAlive"])
    with np.load(fd) as z:
        d = {k: z[k] for k in z.files}
    wins = [(kstrt, kstrt + 4), (kstrt + 5, kstrt + 9), (kstrt + 10, kstrt + 13)]                # the last one is shorter
    per = ("cells", "div", "shr", "vor", "area0", "area1", "status", "stats")
    assert sorted(d) == sorted(["meshes", "windows", "time0", "time1"] + ["m%d_w%d_%s" % (m, w, n) for m in range(2) for w in range(3) for n in per])
    assert np.array_equal(d["meshes"], [[RMAX, 0.], [2 * RMAX, RD]]) and np.array_equal(d["windows"], wins)
    assert np.array_equal(d["time0"], [t[w[0] - kstrt] for w in wins]) and np.array_equal(d["time1"], [t[w[1] - kstrt + 1] for w in wins])
    for m in range(2):
        for w in range(3):
            pre = "m%d_w%d_" % (m, w)
            nQ = len(d[pre + "cells"])
            assert d[pre + "cells"].dtype == np.int64 and d[pre + "cells"].shape == (nQ, 4) and np.isin(d[pre + "cells"], ids).all()
            assert all(d[pre + n].dtype == np.float64 and d[pre + n].shape == (nQ,) for n in RATES)
            assert d[pre + "status"].dtype == np.int8 and d[pre + "stats"].shape == (_lib.MESH_NSTATS,)
            r = {n: d[pre + n] for n in RATES}
            r["status"] = d[pre + "status"]
            r["stats"] = dict(zip(_lib.MESH_STATS, d[pre + "stats"]))
            check_stats(r, pre)
            assert ("--deform window %d mesh %d: nQ = %d, status 0/1/2 = %d/%d/%d" % ((w, m, nQ) + tuple(d[pre + "stats"][:3]))) in log
    # window 0, mesh 0: the seeds are f4 values, so record 0 of the series holds the t0 positions exactly
    yx0 = yx_plain[0]
    assert (mk_plain[0] == 1).all()
    rt, _ = delaunay_fast(yx0, RMAX)
    rq, _ = tri2quad_ref(yx0, rt)
    assert len(rq) >= 50
    index_of = {int(v): k for k, v in enumerate(ids)}
    cells = np.array([[index_of[int(v)] for v in row] for row in d["m0_w0_cells"]], dtype=np.int32).reshape(-1, 4)
    assert np.array_equal(cells, rq)
    # ... and its rates against sit.DeformCells on the file's f4 positions of record 5: every t1 coordinate is off by at most
    # e = half an f4 ulp at its size, the bound of tests/test_gpu_deform.py's f4 caveat with nv = 4
    yx1, T = yx_plain[NWIN], NWIN * RDT
    m1 = (mk_plain[NWIN] == 1) & (mk_plain[NWIN + 1] == 1)             # stepped at the window's last record and alive behind it
    want = sit.DeformCells(yx0, yx1, cells, T, mask1=m1)
    st = d["m0_w0_status"]
    assert np.array_equal(st != 0, want["valid"]) and (st == 1).sum() >= 10
    v = want["valid"]
    e = 0.5 * float(np.spacing(np.float32(np.abs(yx1[m1]).max())))
    y0, x0 = yx0[cells[v], 0], yx0[cells[v], 1]
    uu, vv = (yx1[cells[v], 1] - x0) / T, (yx1[cells[v], 0] - y0) / T
    ext = np.maximum(np.ptp(y0, axis=1), np.ptp(x0, axis=1))
    U = np.maximum(np.ptp(uu, axis=1), np.ptp(vv, axis=1))
    A2 = 2. * want["area0"][v]
    grad = np.abs(want["div"][v]) + np.abs(want["vor"][v]) + want["shr"][v]
    dN = 1.01 * 4 * 4 * e * (ext / T + U)
    dA2 = 1.01 * 8 * 4 * ext * e
    bound = 4. * (dN + grad * dA2) / (A2 - dA2)
    for n in ("div", "shr", "vor"):
        dd = np.abs(d["m0_w0_" + n][v] - want[n][v])
        print("--deform vs the f4 file: %s differs by up to %.3g 1/s (%.3g of the bound), strain %.3g 1/s" %
              (n, dd.max(), (dd / bound).max(), np.abs(want[n][v]).max()))
        assert (dd <= bound).all(), n
    assert np.array_equal(bits(d["m0_w0_area0"][v]), bits(want["area0"][v]))        # t0 is exact in the file
    # the coarsened mesh: its vertices keep their distance
    c1 = np.array([[index_of[int(v_)] for v_ in row] for row in d["m1_w0_cells"]], dtype=np.int64).reshape(-1, 4)
    used = np.unique(c1)
    if len(used) > 1:
        dist = np.hypot(yx0[used, None, 0] - yx0[None, used, 0], yx0[used, None, 1] - yx0[None, used, 1])
        assert dist[np.triu_indices(len(used), 1)].min() >= RD


@pytest.mark.parametrize("extra", [[], ["--nsub", "2", "--tinterp", "centre"]], ids=["plain", "nsub-tinterp"])
def test_cli_deform_flag_without_F(tmp_path, monkeypatch, capsys, extra):
    """2-D-time mode (fused batches, record windows), also sub-stepped with the fields blended in time: the run itself is what it
    was without the flag, the batches are cut at the windows, and every (mesh, window) is consistent in itself"""
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200, two_d_time=True)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4"] + extra
    plain = drv.main(argv)
    out = drv.main(argv + ["--deform", "15", "--deform-window", "6"])
    assert np.array_equal(out["vJIt"], plain["vJIt"]) and np.array_equal(out["iAlive"], plain["iAlive"])
    assert out["files"][:-1] == plain["files"] and "_deformation_" in out["files"][-1]
    for fa, fb in zip(out["files"][:-1], plain["files"]):
        a_, b_ = ncio.LoadNCdata(fa, krec=-1, lmask=True), ncio.LoadNCdata(fb, krec=-1, lmask=True)
        assert np.array_equal(bits(a_[3]), bits(b_[3])) and np.array_equal(a_[4], b_[4])
    Nt, kstrt = out["Nt"], out["kstrt"]
    with np.load(out["files"][-1]) as z:
        d = {k: z[k] for k in z.files}
    wins = [(kstrt + j, kstrt + min(j + 6, Nt) - 1) for j in range(0, Nt, 6)]
    assert np.array_equal(d["windows"], wins) and len(wins) == 3 and wins[-1][1] - wins[-1][0] + 1 == 2
    assert np.array_equal(d["meshes"], [[15., 0.]])
    n_valid = 0
    for w in range(len(wins)):
        pre = "m0_w%d_" % w
        r = {n: d[pre + n] for n in RATES}
        r["status"] = d[pre + "status"]
        r["stats"] = dict(zip(_lib.MESH_STATS, d[pre + "stats"]))
        assert len(d[pre + "cells"]) == len(r["status"]) >= (50 if w == 0 else 1)     # the same cloud as with -F at its start
        check_stats(r, pre)
        n_valid += int((r["status"] != 0).sum())
    assert n_valid > 0
