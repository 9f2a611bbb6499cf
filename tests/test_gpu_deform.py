"""Deformation rates of buoy cells on the MI355X (sitrk_deform_cells, sitrk_deform_mark, sitrk_deform_since_mark,
tools/deformation.py) against the numpy restatement of the contract in tests/test_deform.py: validity equal everywhere, div,
vor and the areas equal as bit patterns (only + - * /), shr within one ulp (the device's sqrt)."""
import os
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio
from sitrack_amd import synthetic as syn
from test_deform import (DAY3, FILL, both_orientations, check_linear_field, deform_ref, jittered_lattice, linear_move, track_file)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


_LAT = {}


def lattice_case():
    """33 x 33 jittered lattice near (-2900, 3000) km moved by the linear field of test_deform over three days; 1024 quads and
    2048 triangles, every third cell reversed, 8 cells of each kind with a repeated vertex (A2 == 0), 20 buoys masked at t0 and
    20 others at t1, one unmasked buoy with a NaN coordinate; the restatement's answer, computed once"""
    if not _LAT:
        yx0 = jittered_lattice(33, 33, -2900., 3000., seed=11)
        yx1 = linear_move(yx0, DAY3)
        rng = np.random.default_rng(12)
        pick = rng.permutation(33 * 33)
        m0 = np.ones(33 * 33, dtype=np.int8); m0[pick[:20]] = 0
        m1 = np.ones(33 * 33, dtype=np.int8); m1[pick[20:40]] = 0
        yx1n = yx1.copy()
        yx1n[pick[40], 0] = np.nan
        cells = {}
        for kind in ("quad", "tri"):
            c = sit.lattice_cells(33, 33, kind).copy()
            c[::3] = c[::3, ::-1]
            flat = rng.choice(len(c), 8, replace=False)
            c[flat, 1] = c[flat, 0]
            c[flat, 2:] = c[flat, :1]                           # a, a, a(, a): no area
            cells[kind] = c
        _LAT.update(yx0=yx0, yx1=yx1, yx1n=yx1n, m0=m0, m1=m1, cells=cells,
                    ref={k: deform_ref(yx0, yx1n, c, DAY3, m0, m1) for k, c in cells.items()})
    return _LAT


def same_as(got, want, what):
    """(out, valid) pairs: validity equal, + - * / results bit-equal, shr within one ulp, fill exact"""
    (o, v), (ro, rv) = got, want
    assert o.shape == ro.shape and np.array_equal(v, rv), what
    for row, name in ((0, "div"), (2, "vor"), (3, "area0"), (4, "area1")):
        bad = np.flatnonzero(bits(o[row]) != bits(ro[row]))
        assert bad.size == 0, "%s: %s differs in %d of %d cells, first %d: got %r want %r" % (what, name, bad.size, o.shape[1], bad[0],
                                                                                            o[row, bad[0]], ro[row, bad[0]])
    d = np.abs(o[1][rv] - ro[1][rv])
    nbit = int((bits(o[1]) != bits(ro[1])).sum())
    print("%s: shr differs from numpy's sqrt in %d of %d valid cells" % (what, nbit, int(rv.sum())))
    assert (d <= np.spacing(np.abs(ro[1][rv]))).all(), what
    assert (o[:, ~rv] == FILL).all(), what


@pytest.mark.parametrize("kind", ["quad", "tri"])
def test_deform_cells_equals_the_restatement(ctx, kind):
    L = lattice_case()
    c = L["cells"][kind]
    assert c.shape == ({"quad": 1024, "tri": 2048}[kind], {"quad": 4, "tri": 3}[kind])
    out, valid, nvalid = ctx.deform_cells(L["yx0"], L["yx1n"], c, DAY3, L["m0"], L["m1"])
    ro, rv = L["ref"][kind]
    assert 0 < (~rv).sum() < len(c) // 2 and nvalid == int(rv.sum())
    same_as((out, valid), (ro, rv), kind)
    # the linear field, all buoys valid: the tolerance of the CPU test
    clean = sit.lattice_cells(33, 33, kind).copy()
    clean[::3] = clean[::3, ::-1]
    out, valid, nvalid = ctx.deform_cells(L["yx0"], L["yx1"], clean, DAY3)
    assert nvalid == len(clean)
    check_linear_field(out, valid)
    r = sit.DeformCells(L["yx0"], L["yx1"], clean, DAY3, ctx=ctx)
    assert np.array_equal(r["div"], out[0]) and np.array_equal(r["tot"], np.sqrt(out[0] * out[0] + out[1] * out[1])) and r["valid"].all()


# ----------------------------------------------------------------------------------------------- device-resident path
def tracked_case():
    grid = syn.make_grid(64, 64, dkm=4.0)
    tm = grid["tmask"].copy()
    tm[39:46, 18:40] = 0                                                          # a coast the flow pushes buoys onto
    grid["tmask"] = tm
    u, v, sic = syn.make_fields(grid, K=8, seed=5, umax=1.2, drift=0.4)
    j, i = np.meshgrid(np.arange(25) - 12., np.arange(24) - 11.5, indexing="ij")
    rng = np.random.default_rng(3)
    yx = np.stack([-20. + 3.5 * j.ravel(), 3.5 * i.ravel()], axis=1) + rng.uniform(-0.8, 0.8, (600, 2))
    return grid, u, v, sic, yx, syn.regular_host_cell(grid, yx)


@pytest.mark.parametrize("nsub", [1, 2])
def test_since_mark_equals_deform_cells_on_fetched_positions(nsub):
    grid, u, v, sic, yx, ji = tracked_case()
    nP, K, kstrt, rdt = len(yx), 8, 3, 3600.
    rng = np.random.default_rng(8)
    first = np.full(nP, kstrt, dtype=np.int64)
    last = np.full(nP, kstrt + 20, dtype=np.int64)
    w = rng.permutation(nP)
    first[w[:15]] = kstrt + 3                              # start inside the first span
    last[w[15:30]] = kstrt + 5                             # stop inside it
    last[w[30:40]] = kstrt + 7                             # stop with its last record: valid
    cells = {"tri": both_orientations(sit.lattice_cells(25, 24, "tri")), "quad": both_orientations(sit.lattice_cells(25, 24, "quad"))}
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=rdt, nslots=K, nsub=nsub)
    try:
        ctx = trk.ctx
        for k in range(K):
            trk.load_record(k, u[k], v[k], sic[k])
        trk.set_buoys(yx, ji, first, last)
        ctx.set_resort(0)
        ctx.run(kstrt % K, kstrt, 2)
        jrec0 = kstrt + 2

        def span(jrec0, n_before_sort, n_after_sort):
            """mark, step, re-sort, step; (jrec1, masks, positions at the mark and now)"""
            trk.deform_mark(jrec0)
            s0 = ctx.fetch()
            ctx.run(jrec0 % K, jrec0, n_before_sort)
            ctx.sort_buoys()
            ctx.run((jrec0 + n_before_sort) % K, jrec0 + n_before_sort, n_after_sort)
            jrec1 = jrec0 + n_before_sort + n_after_sort - 1
            s1 = ctx.fetch()
            m1 = (s1["alive"] == 1) & (first <= jrec0) & (last >= jrec1)
            return jrec1, s0, s1, m1

        jrec1, s0, s1, m1 = span(jrec0, 3, 3)
        assert jrec1 == kstrt + 7
        died = (s0["alive"] == 1) & (s1["alive"] == 0)
        assert died.sum() >= 5 and (s1["alive"] == 1).sum() > nP // 2 and not m1[w[:30]].any() and m1[w[30:40]].any()
        T = (jrec1 - jrec0 + 1) * rdt
        for kind, c in cells.items():
            got = trk.deform(jrec1, c)
            ro, rv, nvalid = ctx.deform_cells(s0["yx"], s1["yx"], c, T, s0["alive"], m1)
            assert 0 < nvalid < len(c)
            for row, name in enumerate(("div", "shr", "vor", "area0", "area1")):
                assert np.array_equal(bits(got[name]), bits(ro[row])), (kind, name)
            assert np.array_equal(got["valid"], rv), kind
            o2, v2, n2 = ctx.deform_since_mark(jrec1, c)
            assert n2 == nvalid and np.array_equal(bits(o2), bits(ro)) and np.array_equal(v2, rv)
            same_as((ro, rv), deform_ref(s0["yx"], s1["yx"], c, T, s0["alive"], m1), "tracked " + kind)
        # a mark re-taken later replaces the first
        jrec0b = jrec1 + 1
        jrec1b, s0b, s1b, m1b = span(jrec0b, 1, 2)
        Tb = (jrec1b - jrec0b + 1) * rdt
        c = cells["tri"]
        o2, v2, _ = ctx.deform_since_mark(jrec1b, c)
        ro, rv, _ = ctx.deform_cells(s0b["yx"], s1b["yx"], c, Tb, s0b["alive"], m1b)
        assert np.array_equal(bits(o2), bits(ro)) and np.array_equal(v2, rv) and rv.any()
        stale, _, _ = ctx.deform_cells(s0["yx"], s1b["yx"], c, Tb, s0["alive"], m1b)
        assert not np.array_equal(bits(stale), bits(o2))
    finally:
        trk.close()


# ----------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_handle_usable():
    L = lattice_case()
    nP = len(L["yx0"])
    good = sit.lattice_cells(33, 33, "tri")
    ctx = _lib.Context(0)
    try:
        want, _, _ = ctx.deform_cells(L["yx0"], L["yx1"], good, DAY3)
        for bad_index, n_bad in ((nP, 1), (-1, 3)):
            c = good.copy()
            c[np.arange(n_bad) * 17 + 5, 1] = bad_index
            with pytest.raises(IndexError, match=r"sitrk_deform_cells: %d cell\(s\) have a vertex index outside \[0, %d\)" % (n_bad, nP)):
                ctx.deform_cells(L["yx0"], L["yx1"], c, DAY3)
            again, _, _ = ctx.deform_cells(L["yx0"], L["yx1"], good, DAY3)
            assert np.array_equal(bits(again), bits(want))
        big = good.astype(np.int64)
        big[7, 2] = 2 ** 40                                                   # does not fit int32: out of range all the same
        with pytest.raises(IndexError, match=r"1 cell\(s\)"):
            ctx.deform_cells(L["yx0"], L["yx1"], big, DAY3)
        # nv = 2, T <= 0 and missing pointers through the raw ABI
        lib, h = ctx._L, ctx._h
        c2 = np.zeros((4, 2), dtype=np.int32)
        out, valid = np.empty((5, 4)), np.empty(4, dtype=np.int8)
        p = _lib._ptr
        assert lib.sitrk_deform_cells(h, nP, p(L["yx0"]), p(L["yx1"]), None, None, 4, 2, p(c2), DAY3, p(out), p(valid), None) == -1
        assert b"nv must be 3" in lib.sitrk_last_error(h)
        c3 = np.ascontiguousarray(good[:4])
        for T in (0., -5., float("nan"), float("inf")):
            assert lib.sitrk_deform_cells(h, nP, p(L["yx0"]), p(L["yx1"]), None, None, 4, 3, p(c3), T, p(out), p(valid), None) == -1
        assert lib.sitrk_deform_cells(h, nP, p(L["yx0"]), None, None, None, 4, 3, p(c3), DAY3, p(out), p(valid), None) == -1
        assert lib.sitrk_deform_cells(h, nP, p(L["yx0"]), p(L["yx1"]), None, None, 4, 3, p(c3), DAY3, None, p(valid), None) == -1
        # nC = 0
        out0, valid0, n0 = ctx.deform_cells(L["yx0"], L["yx1"], np.zeros((0, 3), dtype=np.int32), DAY3)
        assert out0.shape == (5, 0) and valid0.shape == (0,) and n0 == 0
        # since_mark: no buoys, no mark, a mark cancelled by set_buoys, jrec1 < jrec0
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.deform_since_mark(3, good)
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.deform_mark(3)
        grid, u, v, sic, yx, ji = tracked_case()
        ctx.set_grid(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"])
        ctx.set_buoys(yx, ji)
        tri = sit.lattice_cells(25, 24, "tri")
        with pytest.raises(_lib.SitrkError, match="no mark"):
            ctx.deform_since_mark(3, tri)
        ctx.deform_mark(3)
        with pytest.raises(_lib.SitrkError, match="before the mark"):
            ctx.deform_since_mark(2, tri)
        out, valid, n = ctx.deform_since_mark(3, tri)                         # nothing stepped: no motion, every cell valid
        assert n == len(tri) and valid.all() and (out[:3] == 0.).all() and np.array_equal(out[3], out[4])
        out0, _, n0 = ctx.deform_since_mark(3, tri[:0])
        assert out0.shape == (5, 0) and n0 == 0
        c = tri.copy(); c[9, 0] = len(yx)
        with pytest.raises(IndexError, match=r"sitrk_deform_since_mark: 1 cell\(s\)"):
            ctx.deform_since_mark(3, c)
        ctx.set_buoys(yx, ji)
        with pytest.raises(_lib.SitrkError, match="no mark"):
            ctx.deform_since_mark(3, tri)
    finally:
        ctx.close()


# ----------------------------------------------------------------------------------------------- command line
def test_tool_end_to_end_and_the_f4_caveat(tmp_path, ctx, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    L = lattice_case()
    nP = len(L["yx0"])
    ids = (5000 + 7 * np.random.default_rng(2).permutation(nP)).astype(np.int64)
    msk = np.stack([L["m0"], L["m1"]])
    fin = track_file(tmp_path / "trk.nc", L["yx0"], L["yx1"], ids, mask=msk)
    cells = sit.lattice_cells(33, 33, "tri").copy()
    cells[::3] = cells[::3, ::-1]
    fc = str(tmp_path / "cells.npy")
    np.save(fc, ids[cells])
    fout = str(tmp_path / "out.npz")
    assert tool.main(["-i", fin, "-c", fc, "-o", fout]) == 0
    assert "f4 km" in capsys.readouterr().out
    with ncio._Reader(fin) as f:
        y, x = np.asarray(f.var("y_pos")), np.asarray(f.var("x_pos"))
        assert y.dtype.newbyteorder("=") == np.float32
    f0 = np.stack([y[0], x[0]], axis=1).astype(np.float64)
    f1 = np.stack([y[1], x[1]], axis=1).astype(np.float64)
    want = sit.DeformCells(f0, f1, cells, DAY3, mask0=L["m0"], mask1=L["m1"], ctx=ctx)
    with np.load(fout) as z:
        got = {k: z[k] for k in z.files}
    assert sorted(got) == sorted(["div", "shr", "vor", "tot", "area0", "area1", "valid", "cells", "time0", "time1"])
    assert np.array_equal(got["cells"], ids[cells]) and int(got["time1"]) - int(got["time0"]) == int(DAY3)
    for k in ("div", "shr", "vor", "tot", "area0", "area1"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["valid"], want["valid"]) and 0 < got["valid"].sum() < len(cells)
    # the caveat: the f4 file against the fp64 positions.  Every coordinate moves by at most e = half an f4 ulp at its size.
    # With L the cell's extent, U the spread of its vertices' velocities and A2 its doubled area: a velocity gradient is N / A2
    # with N = sum (u_k' + u_k)(y_k' - y_k), where a uniform velocity drops out of the closed contour; each velocity moves by
    # 2e/T and each coordinate difference by 2e, so |dN| <= 4 nv e (L/T + U) and |dA2| <= 8 nv L e (second order: + 1 %);
    # d(gradient) <= (|dN| + |gradient| |dA2|) / (|A2| - |dA2|), and div, vor, shr combine two gradients: <= 4 d(gradient)
    exact = sit.DeformCells(L["yx0"], L["yx1"], cells, DAY3, mask0=L["m0"], mask1=L["m1"], ctx=ctx)
    assert np.array_equal(exact["valid"], want["valid"])
    v = want["valid"]
    e = 0.5 * float(np.spacing(np.float32(max(np.abs(L["yx0"]).max(), np.abs(L["yx1"]).max()))))
    y0, x0 = L["yx0"][cells[v], 0], L["yx0"][cells[v], 1]
    uu, vv = (L["yx1"][cells[v], 1] - x0) / DAY3, (L["yx1"][cells[v], 0] - y0) / DAY3
    ext = np.maximum(np.ptp(y0, axis=1), np.ptp(x0, axis=1))
    U = np.maximum(np.ptp(uu, axis=1), np.ptp(vv, axis=1))
    A2 = 2. * exact["area0"][v]
    grad = np.abs(exact["div"][v]) + np.abs(exact["vor"][v]) + exact["shr"][v]             # above every single gradient
    dN = 1.01 * 4 * 3 * e * (ext / DAY3 + U)
    dA2 = 1.01 * 8 * 3 * ext * e
    bound = 4. * (dN + grad * dA2) / (A2 - dA2)
    for k in ("div", "shr", "vor"):
        d = np.abs(want[k][v] - exact[k][v])
        print("f4 file vs fp64: %s differs by up to %.3g 1/s (%.3g of the bound), strain %.3g 1/s" %
              (k, d.max(), (d / bound).max(), np.abs(exact[k][v]).max()))
        assert (d <= bound).all(), k
        assert d.max() > 1e-12                                                # the rounding of the file is visible
