"""Buoy cells rasterised onto a regular grid on the MI355X (sitrk_raster_cells, sitrk_mesh_raster, IceTracker.mesh_raster,
--deform-grid, tools/deformation.py --grid) against raster_ref() of tests/test_raster.py, the numpy restatement of the contract in
include/sitrk.h.  The contract has only + - * and comparisons: every comparison here is array_equal on `owner` and bit-equality
on the fields.  There is no tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv
from test_deform import FILL
from test_driver import make_case
from test_gpu_deform import bits
from test_gpu_mesh import JREC0, K, KSTRT, RATES, advance, start
from test_mesh import ccw_quads, exact_lattice
from test_raster import (JITTER_COUNTS, JITTER_GRIDS, JITTER_INNER, LATTICE_GRID, jitter_case, lattice_case, raster_inside, raster_ref,
                         split_quads)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1. ties on the exact lattice
def test_ties_on_the_exact_lattice_go_to_the_lowest_index_in_any_order(ctx):
    yx, quads, want, inside = lattice_case()
    assert (inside.sum(axis=0) >= 2).sum() == 426                     # the tied centres of tests/test_raster.py
    owner, nowned = ctx.raster_cells(yx, quads, LATTICE_GRID)
    assert owner.dtype == np.int32 and owner.shape == (30, 34) and np.array_equal(owner, want) and nowned == 621
    assert np.array_equal(sit.RasterCells(yx, quads, LATTICE_GRID, ctx=ctx), want)
    # the rows in a fixed random order: the owner is the lowest index of the permuted rows, whatever lane gets there first
    perm = np.random.default_rng(7).permutation(len(quads))
    want_p = raster_ref(yx[quads[perm]], None, LATTICE_GRID)
    assert not np.array_equal(perm[want_p[want_p >= 0]], want[want >= 0])          # the ties do go to other cells
    owner_p, nowned_p = ctx.raster_cells(yx, quads[perm], LATTICE_GRID)
    assert np.array_equal(owner_p, want_p) and nowned_p == 621
    # either orientation
    mixed = quads.copy()
    mixed[::3] = mixed[::3, ::-1]
    assert np.array_equal(ctx.raster_cells(yx, mixed, LATTICE_GRID)[0], want)
    ms = ctx.raster_kernel_ms()
    assert ms[0] > 0. and ms[1] > 0.


# ------------------------------------------------------------------------------------------------ 2. several workgroups, odd sizes, clipping
@pytest.mark.parametrize("d", [2.96, 8.0, 18.4, "inner"])
def test_jittered_lattice_on_rasters_of_odd_sizes(ctx, d):
    yx, quads, owners = jitter_case()
    grid = JITTER_INNER if d == "inner" else JITTER_GRIDS[d]
    want = owners[d]
    own = want[want >= 0]
    # the restatement's own counts: a degenerate input cannot pass silently
    if d == 2.96:
        assert len(own) > 0.8 * want.size and len(np.unique(own)) == 1225
    if d == 18.4:
        assert len(np.unique(own)) < 1225 / 4
    if d != "inner":
        assert (len(own), len(np.unique(own))) == JITTER_COUNTS[d]
    else:
        assert want.shape == (9, 7) and (want >= 0).all()
    owner, nowned = ctx.raster_cells(yx, quads, grid)
    bad = np.argwhere(owner != want)
    assert bad.size == 0, "d = %s: %d pixels differ, first %s: got %d want %d" % (d, len(bad), bad[0], owner[tuple(bad[0])], want[tuple(bad[0])])
    assert nowned == len(own)


def test_the_same_cells_as_triangles(ctx):
    yx, quads, owners = jitter_case()
    tris = split_quads(quads)
    assert tris.shape == (2450, 3)
    grid = JITTER_GRIDS[2.96]
    want = raster_ref(yx[tris], None, grid)
    assert np.array_equal(want >= 0, owners[2.96] >= 0) and len(np.unique(want[want >= 0])) > 1225      # both halves own
    owner, nowned = ctx.raster_cells(yx, tris, grid)
    assert np.array_equal(owner, want) and nowned == JITTER_COUNTS[2.96][0]
    flip = tris.copy()
    flip[1::2] = flip[1::2, ::-1]
    assert np.array_equal(ctx.raster_cells(yx, flip, grid)[0], want)


def test_a_raster_of_more_pixels_than_one_trip_of_the_gather_kernel(ctx):
    """the gather kernel runs at most 2048 workgroups of 256 lanes: above 524288 pixels its lanes take a second trip, and lanes of
    the last trip fall behind the raster's end"""
    yx, quads = exact_lattice(4, 4, 8.0), ccw_quads(4, 4)
    grid = (-1510.03, 1990.07, 0.05, 751, 719)
    assert 2048 * 256 < grid[3] * grid[4] < 2 * 2048 * 256 and (grid[3] * grid[4]) % 256 != 0
    want = raster_ref(yx[quads], None, grid)
    assert len(np.unique(want[want >= 0])) == 9 and 0.3 * want.size < (want >= 0).sum() < want.size
    owner, nowned = ctx.raster_cells(yx, quads, grid)
    assert np.array_equal(owner, want) and nowned == (want >= 0).sum()


# ------------------------------------------------------------------------------------------------ 3. errors and edges
def test_draw_mask_nan_vertex_and_no_cells(ctx):
    yx, quads, owners = jitter_case()
    grid = JITTER_GRIDS[8.0]
    draw = (np.random.default_rng(11).uniform(size=len(quads)) < 0.6).astype(np.int8)
    want = raster_ref(yx[quads], draw, grid)
    assert 0 < (want >= 0).sum() < (owners[8.0] >= 0).sum() and (draw[want[want >= 0]] == 1).all()
    owner, nowned = ctx.raster_cells(yx, quads, grid, draw=draw)
    assert np.array_equal(owner, want) and nowned == (want >= 0).sum()
    # a NaN vertex takes its four cells out; an infinite one too
    bad = yx.copy()
    bad[36 * 10 + 10, 0] = np.nan
    bad[36 * 20 + 25, 1] = np.inf
    want = raster_ref(bad[quads], None, grid)
    hit = ~np.isfinite(bad[quads]).all(axis=(1, 2))
    assert hit.sum() == 8 and not np.isin(want, np.flatnonzero(hit)).any() and np.isin(owners[8.0], np.flatnonzero(hit)).any()
    assert np.array_equal(ctx.raster_cells(bad, quads, grid)[0], want)
    # a cell without area
    flat = quads.copy()
    flat[100] = [5, 6, 6, 5]
    assert np.array_equal(ctx.raster_cells(yx, flat, grid)[0], raster_ref(yx[flat], None, grid))
    # no cells, no points
    owner, nowned = ctx.raster_cells(yx, np.zeros((0, 4), dtype=np.int32), grid)
    assert owner.shape == (37, 41) and (owner == -1).all() and nowned == 0
    owner, nowned = ctx.raster_cells(np.zeros((0, 2)), np.zeros((0, 3), dtype=np.int32), (0., 0., 1., 1, 1))
    assert owner.tolist() == [[-1]] and nowned == 0
    # one pixel
    g1 = (-1400., 2100., 300., 1, 1)
    assert np.array_equal(ctx.raster_cells(yx, quads, g1)[0], raster_ref(yx[quads], None, g1))


def test_bad_index_and_bad_grids_leave_the_handle_usable(ctx):
    yx, quads, owners = jitter_case()
    grid = JITTER_GRIDS[18.4]
    for v in (-1, len(yx), 2 ** 31 - 1):
        c = quads.copy()
        c[[3, 700], [1, 2]] = v
        with pytest.raises(IndexError, match=r"2 cell\(s\) have a vertex index outside \[0, 1296\)"):
            ctx.raster_cells(yx, c, grid)
        assert np.array_equal(ctx.raster_cells(yx, quads, grid)[0], owners[18.4])
    with pytest.raises(IndexError):
        ctx.raster_cells(np.zeros((0, 2)), quads, grid)
    lib, h, p = ctx._L, ctx._h, _lib._ptr
    yxc, qc = np.ascontiguousarray(yx), np.ascontiguousarray(quads)
    own = np.full((19, 17), 77, dtype=np.int32)
    n = _lib._i64(5)

    def call(y0=-1508.3, x0=1988.9, d=18.4, ny=19, nx=17, nv=4, owner=own):
        return lib.sitrk_raster_cells(h, len(yxc), p(yxc), len(qc), nv, p(qc), None, y0, x0, d, ny, nx, p(owner), C.byref(n))

    for kw in ({"y0": np.nan}, {"x0": np.inf}, {"d": 0.}, {"d": -1.}, {"d": np.nan}, {"d": np.inf}, {"ny": 0}, {"nx": -3},
               {"ny": 2 ** 14, "nx": 2 ** 14 + 1}, {"nv": 5}, {"nv": 2}, {"owner": None}):
        assert call(**kw) == -1, kw
        assert lib.sitrk_last_error(h)
    assert (own == 77).all()                                          # refused before any device work
    assert call() == 0 and np.array_equal(own, owners[18.4]) and n.value == 238
    with pytest.raises(ValueError, match="grid"):
        sit.RasterCells(yx, quads, (0., 0., 1., 0, 4), ctx=ctx)


def test_a_tracker_on_the_same_handle_is_untouched():
    yx, quads, owners = jitter_case()
    states = []
    for with_raster in (False, True):
        trk = start()
        try:
            if with_raster:
                assert np.array_equal(trk.ctx.raster_cells(yx, quads, JITTER_GRIDS[2.96])[0], owners[2.96])
                with pytest.raises(IndexError):
                    trk.ctx.raster_cells(yx[:100], quads, JITTER_GRIDS[8.0])
            advance(trk, JREC0, 2, 1)
            states.append(trk.ctx.fetch())
        finally:
            trk.close()
    a, b = states
    assert np.array_equal(bits(a["yx"]), bits(b["yx"])) and np.array_equal(a["alive"], b["alive"]) and np.array_equal(a["jiT"], b["jiT"])


# ------------------------------------------------------------------------------------------------ 4. the mesh path
def test_mesh_raster_at_t0_and_at_t1():
    nP = 1600
    first = np.full(nP, KSTRT, dtype=np.int64)
    last = np.full(nP, KSTRT + 20, dtype=np.int64)
    gone = np.random.default_rng(8).permutation(nP)[:12]
    last[gone] = KSTRT + 5                                            # these stop inside the span: their cells are of status 0
    trk = start(40, 40, first=first, last=last)
    try:
        ctx = trk.ctx
        s0 = ctx.fetch()
        assert trk.mesh(3.5, JREC0)["nQ"] > 1024
        cells = trk.mesh_cells()
        jrec1 = advance(trk, JREC0, 3, 3)
        s1 = ctx.fetch()
        before = trk.mesh_deform(jrec1)
        st = before["status"]
        out = np.stack([before[n] for n in RATES])
        assert min((st == k).sum() for k in range(3)) >= 1 and (st[np.isin(cells, gone).any(axis=1)] == 0).all()
        lo, hi = s0["yx"].min(axis=0), s0["yx"].max(axis=0)
        grid = (lo[0] - 5.3, lo[1] - 4.1, 1.9, int((hi[0] - lo[0] + 11.) / 1.9), int((hi[1] - lo[1] + 9.) / 1.9))
        for at, P, draw in (("t0", s0["yx"][cells], st != 0), ("t1", s1["yx"][cells], st == 1)):
            want = raster_ref(P, draw, grid)
            assert (want >= 0).sum() > 0.5 * want.size and (want == -1).any(), at
            r = trk.mesh_raster(jrec1, grid, at=at)
            bad = np.argwhere(r["owner"] != want)
            assert bad.size == 0, "%s: %d pixels differ, first %s" % (at, len(bad), bad[0])
            own = want >= 0
            assert not np.isin(want[own], np.flatnonzero(st == 0)).any()           # a status-0 cell owns nothing
            if at == "t1":
                assert (st[want[own]] == 1).all()
            else:
                assert (st[want[own]] == 2).any()
            for k, n in enumerate(RATES):
                f = np.where(own, out[k][np.where(own, want, 0)], FILL)
                assert r[n].shape == want.shape and np.array_equal(bits(r[n]), bits(f)), (at, n)
            again = trk.mesh_raster(jrec1, grid, at=at)                        # two calls: the same bits
            assert np.array_equal(again["owner"], r["owner"]) and all(np.array_equal(bits(again[n]), bits(r[n])) for n in RATES)
            only = trk.mesh_raster(jrec1, grid, at=at, fields=False)
            assert sorted(only) == ["owner"] and np.array_equal(only["owner"], want)
            raw = ctx.mesh_raster(0, jrec1, grid, at_t1=(at == "t1"), want="fields")
            assert sorted(raw) == ["fields", "nowned"] and raw["nowned"] == own.sum() and np.array_equal(bits(raw["fields"][0]), bits(r["div"]))
        assert not np.array_equal(trk.mesh_raster(jrec1, grid, at="t0")["owner"], trk.mesh_raster(jrec1, grid, at="t1")["owner"])
        # sitrk_mesh_deform returns what it returned before the raster calls, the tracker is where it was
        after = trk.mesh_deform(jrec1)
        assert np.array_equal(after["status"], st) and all(np.array_equal(bits(after[n]), bits(before[n])) for n in RATES)
        assert [np.float64(after["stats"][n]).view(np.uint64) for n in _lib.MESH_STATS] == \
               [np.float64(before["stats"][n]).view(np.uint64) for n in _lib.MESH_STATS]
        assert np.array_equal(bits(ctx.fetch()["yx"]), bits(s1["yx"])) and np.array_equal(trk.mesh_cells(), cells)
        ms = ctx.raster_kernel_ms()
        assert ms[0] > 0. and ms[1] > 0.
        # the measurement knob changes no result
        ctx.set_tuning(raster_count=1)
        counted = trk.mesh_raster(jrec1, grid, at="t0")
        claims = ctx.raster_stats()
        ctx.set_tuning(raster_count=0)
        want = raster_ref(s0["yx"][cells], st != 0, grid)
        inside = raster_inside(s0["yx"][cells], st != 0, grid)
        assert np.array_equal(counted["owner"], want) and claims == inside.sum() >= (want >= 0).sum() > 0
    finally:
        trk.close()


def test_mesh_raster_errors_and_the_empty_mesh():
    trk = start()
    try:
        ctx = trk.ctx
        lib, h, p = ctx._L, ctx._h, _lib._ptr
        grid = (-70., -50., 5., 20, 21)
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_raster(JREC0, grid)
        assert trk.mesh(0.01, JREC0, slot=2)["nQ"] == 0                # an empty mesh: -1 and FILL everywhere
        ctx.run(JREC0 % K, JREC0, 1)
        r = trk.mesh_raster(JREC0, grid, slot=2)
        assert (r["owner"] == -1).all() and r["owner"].shape == (20, 21) and all((r[n] == FILL).all() for n in RATES)
        assert trk.mesh(3.5, JREC0 + 1)["nQ"] > 256
        ctx.run((JREC0 + 1) % K, JREC0 + 1, 1)
        own = np.full((20, 21), 77, dtype=np.int32)
        n = _lib._i64(0)

        def call(mesh=0, jrec1=JREC0 + 1, at=0, y0=-70., x0=-50., d=5., ny=20, nx=21, owner=own, fields=None):
            return lib.sitrk_mesh_raster(h, mesh, jrec1, at, y0, x0, d, ny, nx, p(owner), p(fields), C.byref(n))

        for kw, msg in (({"mesh": 8}, b"mesh must be in 0..7"), ({"mesh": 1}, b"mesh 1 is empty"), ({"jrec1": JREC0}, b"before the mesh's t0"),
                        ({"at": 2}, b"at_t1"), ({"at": -1}, b"at_t1"), ({"d": 0.}, b"d_km"), ({"y0": np.nan}, b"finite"), ({"ny": 0}, b"ny and nx"),
                        ({"ny": 2 ** 15, "nx": 2 ** 15}, b"2^28"), ({"owner": None}, b"both null")):
            assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
        assert (own == 77).all()
        assert call() == 0 and (own >= 0).any() and n.value == (own >= 0).sum()
        for bad, pat in (({"at": "t2"}, "`at`"), ({"grid": (0., 0., 1., 0, 4)}, "`grid`")):
            with pytest.raises(ValueError, match=pat):
                trk.mesh_raster(JREC0 + 1, bad.get("grid", grid), at=bad.get("at", "t0"))
        ctx.run((JREC0 + 2) % K, JREC0 + 2, 1)                          # the handle goes on
        assert np.isfinite(ctx.fetch()["yx"]).all()
    finally:
        trk.close()
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.mesh_raster(0, 3, (0., 0., 1., 4, 4))
        with pytest.raises(_lib.SitrkError, match="no raster call"):
            ctx.raster_kernel_ms()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. command line
def test_cli_deform_grid_flag_and_the_tool(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200)
    replay = {}

    class Replaying(sit.IceTracker):
        """the driver's tracker; every mesh_raster is followed by a mesh_deform and a mesh_raster of the test's own on the same state"""
        def mesh_raster(self, jrec1, grid, slot=0, at="t0", fields=True):
            got = super().mesh_raster(jrec1, grid, slot=slot, at=at, fields=fields)
            assert sorted(got) == ["owner"] and not fields           # no second copy of the rates comes down
            replay[(slot, jrec1)] = (super().mesh_deform(jrec1, slot=slot), super().mesh_raster(jrec1, grid, slot=slot, at=at), grid, at)
            return got

    monkeypatch.setattr(drv, "IceTracker", Replaying)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F", "--deform", "30", "--deform-window", "5"]
    outs = {}
    for at in ("t0", "t1"):
        replay.clear()
        out = drv.main(argv + ["--deform-grid", "10" if at == "t0" else "10@t1"])
        capsys.readouterr()
        with np.load(out["files"][2]) as z:
            d = {k: z[k] for k in z.files}
        outs[at] = d
        kstrt = out["kstrt"]
        wins = [(kstrt, kstrt + 4), (kstrt + 5, kstrt + 9), (kstrt + 10, kstrt + 13)]
        per = ("cells", "div", "shr", "vor", "area0", "area1", "status", "stats", "owner")
        assert sorted(d) == sorted(["meshes", "windows", "time0", "time1", "grid", "grid_at"] + ["m0_w%d_%s" % (w, n) for w in range(3) for n in per])
        assert d["grid"].shape == (5,) and d["grid"][2] == 10. and str(d["grid_at"]) == at and len(replay) == 3
        assert d["grid"][0] % 10. == 0. and d["grid"][1] % 10. == 0.
        ny, nx = int(d["grid"][3]), int(d["grid"][4])
        for w, (_, jrec1) in enumerate(wins):
            pre = "m0_w%d_" % w
            owner = d[pre + "owner"]
            r, ras, grid, at_ = replay[(0, jrec1)]
            assert tuple(d["grid"]) == tuple(grid) and at_ == at
            assert owner.dtype == np.int32 and owner.shape == (ny, nx) and np.array_equal(owner, ras["owner"])
            own = owner >= 0
            assert own.any() and (d[pre + "status"][owner[own]] != 0).all() and owner.max() < len(d[pre + "status"])
            for n in RATES:                                          # the map is out[:, owner] on the host
                assert np.array_equal(bits(d[pre + n]), bits(r[n]))
                assert np.array_equal(bits(ras[n]), bits(np.where(own, d[pre + n][np.where(own, owner, 0)], FILL))), (at, w, n)
    # window 0 at t0: the seeds are f4 values, so record 0 of the series holds the t0 positions exactly
    d = outs["t0"]
    t, ids, _, yx_all, mk = ncio.LoadNCdata(out["files"][0], krec=-1, lmask=True)
    index_of = {int(v): k for k, v in enumerate(ids)}
    cells = np.array([[index_of[int(v)] for v in row] for row in d["m0_w0_cells"]], dtype=np.int32).reshape(-1, 4)
    assert len(cells) >= 50 and (mk[0] == 1).all()
    grid = tuple(d["grid"][:3]) + (int(d["grid"][3]), int(d["grid"][4]))
    assert np.array_equal(d["m0_w0_owner"], raster_ref(yx_all[0][cells], d["m0_w0_status"] != 0, grid))
    assert not np.array_equal(outs["t1"]["m0_w0_owner"], d["m0_w0_owner"])
    # tools/deformation.py --grid on the written series: a map equal to sit.RasterCells on the file's positions
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    fc, fout = str(tmp_path / "cells.npy"), str(tmp_path / "map.npz")
    np.save(fc, d["m0_w0_cells"])
    assert tool.main(["-i", out["files"][0], "-c", fc, "-k", "0", "-K", "5", "--grid", "7.5", "-o", fout]) == 0
    assert "--grid 7.5 km" in capsys.readouterr().out
    with np.load(fout) as z:
        m = {k: z[k] for k in z.files}
    yx0 = yx_all[0].astype(np.float64)
    g = sit.raster_grid(yx0[:, 0].min(), yx0[:, 0].max(), yx0[:, 1].min(), yx0[:, 1].max(), 7.5)
    assert tuple(m["grid"]) == g and m["owner"].dtype == np.int32 and m["owner"].shape == g[3:]
    assert np.array_equal(m["owner"], sit.RasterCells(yx0, cells, g, draw=m["valid"]))
    assert np.array_equal(m["owner"], raster_ref(yx0[cells], m["valid"], g)) and 0 < (m["owner"] >= 0).sum()
