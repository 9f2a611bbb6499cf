"""Bounded Delaunay triangulation on the MI355X (sitrk_delaunay, sitrk_delaunay_buoys, sit.DelaunayTris, IceTracker.tris) against
the restatements of the contract in tests/test_delaunay.py: tris, nT and vertex equal as integers in every case, row for row."""
import itertools

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from test_deform import DAY3, check_linear_field, jittered_lattice, linear_move
from test_gpu_deform import tracked_case
from test_delaunay import UNIT, cocircular_points, delaunay_fast, delaunay_literal, delaunay_ref, lattice_case, quantise
from test_cloud_trips import NP_TRIP, TRIP, delaunay_trip_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_as(ctx, yx, rmax, mask=None, ref=delaunay_ref, want=None):
    """the device against a restatement: rows, their number and the vertex flags as integers; returns (tris, vertex)"""
    tris, nT, vertex = ctx.delaunay(yx, rmax, mask=mask)
    rt, rv = ref(yx, rmax, mask) if want is None else want
    assert tris.dtype == np.int32 and vertex.dtype == np.int8 and tris.shape == (nT, 3)
    assert np.array_equal(vertex, rv), np.flatnonzero(vertex != rv)[:8]
    assert nT == len(rt), (nT, len(rt))
    assert np.array_equal(tris, rt), np.flatnonzero((tris != rt).any(axis=1))[:8]
    return tris, vertex


def test_smallest_inputs(ctx):
    for n in (0, 1, 2):
        t, v = same_as(ctx, np.arange(2. * n).reshape(n, 2), 5., ref=delaunay_literal)
        assert t.shape == (0, 3) and v.tolist() == [1] * n
    tri = np.array([[0., 0.], [0., 4.], [3., 0.]])                     # y up, x right: 0 -> 1 -> 2 is counter-clockwise
    t, _ = same_as(ctx, tri, 5., ref=delaunay_literal)
    assert t.tolist() == [[0, 1, 2]]
    t, _ = same_as(ctx, tri[::-1].copy(), 5., ref=delaunay_literal)
    assert t.tolist() == [[0, 2, 1]]
    t, _ = same_as(ctx, tri[[0, 2, 1]], 5., ref=delaunay_literal)
    assert t.tolist() == [[0, 2, 1]]
    t, _ = same_as(ctx, np.array([[0., 0.], [1., 2.], [2., 4.]]), 5., ref=delaunay_literal)
    assert len(t) == 0                                                  # collinear
    # the circumradius of the 3-4-5 triangle is 2.5 km
    assert len(same_as(ctx, tri, 2.5 * (1. - 1e-9), ref=delaunay_literal)[0]) == 0
    assert len(same_as(ctx, tri, 2.5 * (1. + 1e-9), ref=delaunay_literal)[0]) == 1
    # a masked point, a NaN point and a duplicate
    yx = np.array([[0., 0.], [0., 4.], [3., 0.], [3., 4.], [0., 4.], [1., 1.], [np.nan, 2.], [1.5, 2.5]])
    mask = np.array([1, 1, 1, 1, 1, 0, 1, 1], dtype=np.int8)
    t, v = same_as(ctx, yx, 5., mask, ref=delaunay_literal)
    assert v.tolist() == [1, 1, 1, 1, 2, 0, 0, 1] and len(t) == 4 and not np.isin(t, [4, 5, 6]).any()


def test_unit_square_in_all_24_index_orders(ctx):
    sq = np.array([[0., 0.], [0., 1.], [1., 1.], [1., 0.]])
    for perm in itertools.permutations(range(4)):
        yx = sq[list(perm)]
        t, _ = same_as(ctx, yx, 1., ref=delaunay_literal)
        assert len(t) == 2 and (t[:, 0] == 0).all(), perm              # the fan from the lowest index


@pytest.fixture(scope="module")
def uniform_case():
    rng = np.random.default_rng(11)
    yx = np.rint(rng.uniform(0., 100., (2000, 2)) * UNIT) / UNIT         # on the 2^-20 km lattice: an offset of whole km is exact
    return yx, {r: delaunay_ref(yx, r) for r in (3., 5., 50.)}


@pytest.mark.parametrize("rmax", [3., 5., 50.])
def test_uniform_cloud_and_its_translate(ctx, uniform_case, rmax):
    yx, refs = uniform_case
    t, v = same_as(ctx, yx, rmax, want=refs[rmax])
    print("rmax %g km: %d triangles of 2000 points" % (rmax, len(t)))
    assert len(refs[3.][0]) < len(refs[5.][0]) < len(refs[50.][0]) < 2 * 2000 - 5
    far = yx + np.array([4000., -3000.])
    assert np.array_equal(np.rint(far * UNIT) - np.rint(yx * UNIT), np.broadcast_to([4000. * UNIT, -3000. * UNIT], yx.shape))
    t2, v2 = same_as(ctx, far, rmax, want=(t, v))


def test_exact_lattice_is_independent_of_the_bin_side(ctx):
    yx, mask = lattice_case(40, 50, spacing_km=4.0, seed=2, nmask=30)
    want = {f: delaunay_ref(yx, f * 4.0, mask) for f in (1.0, 0.6)}
    assert len(want[0.6][0]) == 0 and 2 * 39 * 49 - 4 * 30 * 2 <= len(want[1.0][0]) < 2 * 39 * 49
    try:
        for knob in (1, 2, 3, 4):
            ctx.set_tuning(delaunay_bin=knob)
            for f in (1.0, 0.6):
                same_as(ctx, yx, f * 4.0, mask, want=want[f])
        for bad in (0, 5):
            with pytest.raises(_lib.SitrkError, match="delaunay_bin must be 1..4"):
                ctx.set_tuning(delaunay_bin=bad)
    finally:
        ctx.set_tuning(delaunay_bin=3)


def test_cocircular_and_nearly_cocircular_points(ctx):
    k = 1500000                                                          # coordinates of about 2^28 units around the centre
    shift = (2 ** 40 + 12345, -2 ** 41 + 777)
    P = cocircular_points(k=k, shift=shift)
    n = len(P)
    assert n >= 12 and 2 ** 27 < np.abs(P - np.array(shift)).max() < 2 ** 29
    P = P[np.random.default_rng(6).permutation(n)]
    yx = P / UNIT
    Y, X, _ = quantise(yx)
    assert Y == P[:, 0].tolist() and X == P[:, 1].tolist()                # quantisation is the identity
    t, v = same_as(ctx, yx, 500.)
    assert len(t) == n - 2 and (t[:, 0] == 0).all()                      # the fan from the lowest index
    tests, exact = ctx.delaunay_stats()
    print("%d cocircular points: %d in-circle tests, %d through the 128-bit path" % (n, tests, exact))
    assert exact >= n - 3
    rng = np.random.default_rng(7)
    for trial in range(6):                                               # single points one unit off the circle
        Q = P.copy()
        j = rng.choice(n, 1 + trial % 3, replace=False)
        Q[j] += rng.choice([-1, 1], (len(j), 2))
        t, v = same_as(ctx, Q / UNIT, 500.)
        assert n - 2 - 4 * len(j) <= len(t) <= n - 2


@pytest.fixture(scope="module")
def large_case():
    rng = np.random.default_rng(21)
    side = 540
    j, i = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
    lat = np.stack([j.ravel(), i.ravel()], axis=1) + rng.uniform(-0.3, 0.3, (side * side, 2))
    clusters = [c + rng.uniform(0., 0.5, (5000, 2)) for c in (np.array([100.2, 200.4]), np.array([400.6, 50.1]))]
    sparse = 10. * np.stack(np.meshgrid(np.arange(20.), np.arange(20.), indexing="ij"), axis=-1).reshape(-1, 2) + \
        np.array([0., 600.]) + rng.uniform(-1., 1., (400, 2))
    yx = np.concatenate([lat] + clusters + [sparse])
    yx = yx[rng.permutation(len(yx))] + np.array([-1200., 300.])
    mask = np.ones(len(yx), dtype=np.int8)
    for y0, x0 in ((-1000., 400.), (-800., 700.), (-1100.5, 520.25)):    # holes
        mask[(np.abs(yx[:, 0] - y0) < 12.) & (np.abs(yx[:, 1] - x0) < 9.)] = 0
    rmax = 1.5
    return yx, mask, rmax, delaunay_fast(yx, rmax, mask)


def test_large_cloud_with_clusters_holes_and_a_sparse_region(ctx, large_case):
    yx, mask, rmax, want = large_case
    assert len(yx) > 300000 and (mask == 0).sum() > 1000
    t, v = same_as(ctx, yx, rmax, mask, want=want)
    bin_ms, tri_ms, compact_ms = ctx.delaunay_kernel_ms()
    tests, exact = ctx.delaunay_stats()
    print("%d points, %d triangles: binning %.2f ms, triangles %.2f ms, compaction %.2f ms; %d in-circle tests, %d exact" %
          (len(yx), len(t), bin_ms, tri_ms, compact_ms, tests, exact))
    assert len(t) > 1024 * 256 and tests > 0                             # more than one scan block, many workgroups
    # the sparse region has vertices and no triangle
    sparse = np.flatnonzero(yx[:, 1] > 300. + 560.)
    assert len(sparse) == 400 and (v[sparse] == 1).all() and not np.isin(t, sparse).any()


def test_vertices_on_both_sides_of_the_quantise_kernels_trip(ctx):
    """nP past one trip of dl_quant_kernel's capped grid, few vertices: the second trip's points need their xy and vertex bytes and
    their part in nv, the bounding box and the mask (tests/test_cloud_trips.py checks what the input holds)"""
    yx, mask, rmax, want = delaunay_trip_case()
    t, v = same_as(ctx, yx, rmax, mask, want=want)
    assert len(yx) == NP_TRIP and (v[TRIP:] == 1).sum() >= 1000 and (t >= TRIP).all(axis=1).sum() >= 100


def test_out_of_range_index_in_the_second_trip():
    rng = np.random.default_rng(12)
    yx = rng.uniform(0., 30., (NP_TRIP, 2))
    small = rng.uniform(0., 30., (200, 2))
    want = delaunay_ref(small, 4.)
    ctx = _lib.Context(0)
    try:
        yx[[TRIP + 1234, TRIP + 77], 1] = 2.0 ** 31
        with pytest.raises(_lib.SitrkError, match=r"beyond 2\^30 km at index %d$" % (TRIP + 77)):
            ctx.delaunay(yx, 4.)
        yx[5, 0] = -2.0 ** 31
        with pytest.raises(_lib.SitrkError, match=r"beyond 2\^30 km at index 5$"):
            ctx.delaunay(yx, 4.)
        m = np.ones(NP_TRIP, dtype=np.int8)
        m[5] = 0
        with pytest.raises(_lib.SitrkError, match=r"beyond 2\^30 km at index %d$" % (TRIP + 77)):
            ctx.delaunay(yx, 4., mask=m)
        same_as(ctx, small, 4., want=want)
    finally:
        ctx.close()


def test_device_resident_buoys():
    grid, u, v, sic, yx, ji = tracked_case()
    K, rmax = 8, 4.0
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=3600., nslots=K)
    try:
        c = trk.ctx
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            c.delaunay_buoys(rmax)
        for k in range(K):
            trk.load_record(k, u[k], v[k], sic[k])
        trk.set_buoys(yx, ji)
        c.set_resort(0)
        c.run(0, 0, 2)
        trk.deform_mark(2)
        s0 = c.fetch()
        c.run(2, 2, 6)
        s = c.fetch()
        alive = s["alive"] == 1
        assert 5 <= (~alive).sum() < len(yx) // 2
        tris = trk.tris(rmax)
        want, wv = delaunay_ref(s["yx"], rmax, alive)
        assert np.array_equal(tris, want) and len(want) > 500
        host = sit.DelaunayTris(s["yx"], rmax, mask=alive, ctx=c, return_vertex=True)
        assert np.array_equal(host[0], want) and np.array_equal(host[1], wv)
        got = c.delaunay_buoys(rmax)
        assert np.array_equal(got[0], want) and got[1] == len(want) and np.array_equal(got[2], wv)
        c.sort_buoys()                                                   # a re-sort in between changes nothing
        assert np.array_equal(trk.tris(rmax), want)
        # the rows go into quads() and deform() as they are
        quads, tri_quad = trk.quads(tris, angles=(40., 140.), ratio_min=0.3)
        assert len(quads) > 100 and (tri_quad >= -1).all()
        m1 = alive & (s0["alive"] == 1)
        for cells in (tris, quads):
            d = trk.deform(7, cells)
            ro, rv, nvalid = c.deform_cells(s0["yx"], s["yx"], cells, 6 * 3600., s0["alive"], m1)
            assert nvalid == len(cells) and d["valid"].all() and np.array_equal(d["div"], ro[0]) and np.array_equal(d["area1"], ro[4])
        s2 = c.fetch()
        for k in s:
            assert np.array_equal(s2[k], s[k], equal_nan=True), k        # nothing of the tracker moved
    finally:
        trk.close()


def test_round_trip_reproduces_a_linear_field(ctx):
    yx0 = jittered_lattice(30, 30, -1500., 2000.)
    tris = sit.DelaunayTris(yx0, 12., ctx=ctx)
    assert np.array_equal(tris, delaunay_fast(yx0, 12.)[0]) and len(tris) > 1500
    quads, _ = sit.Tri2Quad(yx0, tris, angles=(40., 140.), ratio_min=0.3, ctx=ctx)
    assert len(quads) > 400
    for cells in (tris, quads):
        r = sit.DeformCells(yx0, linear_move(yx0, DAY3), cells, DAY3, ctx=ctx)
        check_linear_field(np.stack([r["div"], r["shr"], r["vor"]]), r["valid"])


def test_tool_triangulates_a_record_on_the_device(tmp_path, ctx):
    import os
    import sys
    from test_deform import track_file
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import generate_quad_mesh as tool
    from sitrack_amd import ncio
    yx0 = jittered_lattice(14, 13, -1500., 2000.)
    ids = 1000 + 3 * np.random.default_rng(4).permutation(len(yx0))
    msk = np.ones((2, len(yx0)), dtype=np.int8)
    msk[0, [20, 21, 34, 90]] = 0
    fin = track_file(tmp_path / "trk.nc", yx0, linear_move(yx0, DAY3), ids, mask=msk)
    fout = str(tmp_path / "cells.npy")
    assert tool.main(["-i", fin, "-t", "gpu", "--rmax", "12", "--angles", "40,140", "--ratio", "0.3", "-o", fout]) == 0
    with ncio._Reader(fin) as f:
        yx, ok = tool._record(f, 0, True)
    assert not ok[[20, 21, 34, 90]].any() and ok.sum() == len(yx0) - 4
    tris = sit.DelaunayTris(yx, 12., mask=ok, ctx=ctx)
    assert np.array_equal(tris, delaunay_fast(yx, 12., ok)[0]) and len(tris) > 250
    quads, _ = sit.Tri2Quad(yx, tris, mask=ok, angles=(40., 140.), ratio_min=0.3, ctx=ctx)
    cells = np.load(fout)
    assert len(quads) > 60 and np.array_equal(cells, ids[quads])
    with pytest.raises(SystemExit, match="--rmax"):
        tool.main(["-i", fin, "-t", "gpu", "--rmax", "501", "-o", fout])
    with pytest.raises(SystemExit, match="--rmax goes with"):
        tool.main(["-i", fin, "-t", "auto", "--rmax", "5", "-o", fout])


def test_errors_leave_the_handle_usable():
    rng = np.random.default_rng(9)
    yx = rng.uniform(0., 30., (200, 2))
    ctx = _lib.Context(0)
    try:
        want = delaunay_ref(yx, 4.)
        same_as(ctx, yx, 4., want=want)
        for bad in (float("nan"), 0., -1., 501., float("inf")):
            with pytest.raises(_lib.SitrkError, match=r"rmax_km must be finite and in \(0, 500\]"):
                ctx.delaunay(yx, bad)
            with pytest.raises(ValueError, match="`rmax_km`"):
                sit.DelaunayTris(yx, bad, ctx=ctx)
        far = yx.copy()
        far[[17, 5], 1] = 2.0 ** 31
        with pytest.raises(_lib.SitrkError, match=r"beyond 2\^30 km at index 5"):
            ctx.delaunay(far, 4.)
        m = np.ones(200, dtype=np.int8)
        m[[5, 17]] = 0
        same_as(ctx, far, 4., m, want=delaunay_ref(far, 4., m))          # masked: no error
        # too little room: only nT (and the flags) come back
        nT = len(want[0])
        t, n, v = ctx.delaunay(yx, 4., cap=nT - 1)
        assert t is None and n == nT and np.array_equal(v, want[1])
        lib, h, p = ctx._L, ctx._h, _lib._ptr
        rows = np.full((nT, 3), -7, dtype=np.int32)
        cnt = _lib._i64(0)
        assert lib.sitrk_delaunay(h, 200, p(yx), None, 4., nT - 1, p(rows), _lib.C.byref(cnt), None) == 0
        assert cnt.value == nT and (rows == -7).all()
        assert lib.sitrk_delaunay(h, 200, p(yx), None, 4., nT, p(rows), _lib.C.byref(cnt), None) == 0
        assert cnt.value == nT and np.array_equal(rows, want[0])
        # missing pointers
        assert lib.sitrk_delaunay(h, 200, None, None, 4., nT, p(rows), _lib.C.byref(cnt), None) == -1
        assert lib.sitrk_delaunay(h, 200, p(yx), None, 4., nT, None, _lib.C.byref(cnt), None) == -1
        assert lib.sitrk_delaunay(h, 200, p(yx), None, 4., nT, p(rows), None, None) == -1
        assert lib.sitrk_delaunay(h, 200, p(yx), None, 4., 0, None, _lib.C.byref(cnt), None) == 0 and cnt.value == nT
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.delaunay_buoys(4.)
        same_as(ctx, yx, 4., want=want)
    finally:
        ctx.close()
