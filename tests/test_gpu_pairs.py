"""Dispersion of buoy pairs on the MI355X (sitrk_pairs_*, sit.PairDispersion, IceTracker.pairs*, --pairs) against pairs_ref() of
tests/test_pairs.py, the numpy restatement of the contract in include/sitrk.h.

The class of a pair is decided by + - * and comparisons alone: column 0 of the table and npts are compared as integers, with no
tolerance anywhere.

Bound of the sums (columns 1..6), the rule of check_stats in tests/test_gpu_mesh.py: any summation order of n terms is within
(n - 1) 2^-53 sum|t| of the exact sum, and a term t rebuilt in numpy differs from the device's by at most c half-ulps, so
    |S - fsum(t)| <= (n + c) 2^-53 fsum|t|.
c per column, with u = 2^-53 (one half-ulp, relative), "sqrt within one ulp, everything else the same bits": q0, q1 and q1 - q0 are
+ - * on the same bits and equal.  numpy's sqrt is correctly rounded and the device's within one ulp of the exact root, so a root
differs by at most one ulp = 2u.
    r0                     2u                                            c = 2
    r0 + r1                both addends positive and off by <= 2u, the two roundings of the sum u each: 4u
    d = (q1 - q0)/(r0+r1)  the same numerator, 4u from the divisor, the two roundings of the quotient u each: 6u
    e = d/r0               6u + 2u + the two roundings: 10u              c = 10   (sum e and sum |e|)
    e*e                    2 * 10u + the two roundings: 22u              c = 22
    (e*e)*|e|              22u + 10u + the two roundings: 34u            c = 34
    d*d                    2 * 6u + the two roundings: 14u               c = 14
These are first-order counts; what is left of the n - 1 -> n step covers the terms of second order."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv
from test_driver import make_case
from test_gpu_mesh import JREC0, K, KSTRT, RDT, advance, start
from test_pairs import LAT_EDGES, LAT_NX, LAT_NY, bits, jitter_cloud, lattice, lattice_counts, pairs_ref, smooth_move

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_ULPS = (2, 10, 10, 22, 34, 14)                                  # columns 1..6, derived in the module docstring


def kernel_constant(name):
    """a constexpr of sitrack_amd/csrc/sitrk_pairs.hip"""
    src = open(os.path.join(ROOT, "sitrack_amd", "csrc", "sitrk_pairs.hip")).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9.]+)\s*;" % name, src)
    assert m, name
    return float(m.group(1))


TILE, BIN_FRAC = int(kernel_constant("kPairsTile")), kernel_constant("kPairsBinFrac")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def check(got, ref, what):
    """counts as integers; every sum within the derived bound of the exactly rounded sum of the restatement's terms"""
    assert got["npts"] == ref["npts"], what
    assert got["table"].shape == ref["table"].shape and np.array_equal(got["table"][:, 0], ref["table"][:, 0]), \
        (what, got["table"][:, 0], ref["table"][:, 0])
    for c, t in enumerate(ref["terms"]):
        n = t.shape[1]
        for k in range(6):
            S, want, mag = got["table"][c, 1 + k], math.fsum(t[k]), math.fsum(np.abs(t[k]))
            bound = (n + HALF_ULPS[k]) * 2. ** -53 * mag
            print("%s class %d: %-10s device %.17g  fsum %.17g  |diff| %.3g  bound %.3g" % (what, c, _lib.PAIRS_COLS[1 + k], S, want, abs(S - want),
                                                                                         bound))
            assert abs(S - want) <= bound, (what, c, _lib.PAIRS_COLS[1 + k])
        if n == 0:
            assert (got["table"][c] == 0.).all(), (what, c)


def chunks_of(yx, R):
    """the home chunks the documented grid gives the points yx: bins of side R / kPairsBinFrac from the cloud's lower corner, a row of
    bins with n points cut into ceil(n / kPairsTile) chunks; and the most points in one bin"""
    side = R / BIN_FRAC
    b = np.floor((yx - yx.min(axis=0)) / side).astype(np.int64)
    assert b.max() < 8000 and (b[:, 0].max() + 1) * (b[:, 1].max() + 1) <= max(4096, 8 * len(yx))     # the side is not widened
    rows = np.bincount(b[:, 0])
    return int(np.ceil(rows / TILE).sum()), int(np.bincount(b[:, 0] * (b[:, 1].max() + 1) + b[:, 1]).max())


# ------------------------------------------------------------------------------------------------ 1. the lattice
def test_lattice_with_edges_on_exact_separations(ctx):
    yx = lattice()
    yx1 = smooth_move(yx)
    assert len(yx) % 64 != 0
    got = sit.PairDispersion(yx, yx1, LAT_EDGES, ctx=ctx)
    assert sorted(got) == ["npts", "table"] and got["table"].dtype == np.float64
    check(got, pairs_ref(yx, yx1, LAT_EDGES), "lattice")
    assert got["table"][:, 0].tolist() == [lattice_counts(LAT_NY, LAT_NX, (c + 1) ** 2, (c + 2) ** 2) for c in range(3)]
    # edges[0] > 0 cuts the pairs 8 and 11.3 km apart out; [12, 16) and [16.5, 17.5) hold no separation of the lattice; 16 km
    # exactly, q0 == E_1, opens class 1
    edges = (12., 16., 16.5, 17.5, 24.)
    ref = pairs_ref(yx, yx1, edges)
    assert ref["table"][:, 0].tolist() == [0., lattice_counts(LAT_NY, LAT_NX, 4, 5), 0., lattice_counts(LAT_NY, LAT_NX, 5, 9)]
    check(ctx.pairs_points(yx, yx1, edges), ref, "lattice, cut")
    ms = ctx.pairs_kernel_ms()
    assert len(ms) == 3 and all(x >= 0. for x in ms) and ms[1] > 0.
    assert ctx.pairs_stats() >= ref["table"][:, 0].sum()


# ------------------------------------------------------------------------------------------------ 2. many bins both ways
@pytest.mark.parametrize("name", ["geometric", "linear", "one class", "sixteen classes"])
def test_jittered_cloud_over_many_bins(ctx, name):
    yx = jitter_cloud()                                               # 1480 points on 400 x 370 km
    yx1 = smooth_move(yx)
    edges = {"geometric": sit.pair_edges(10., 80., 6), "linear": np.arange(0., 61., 10.), "one class": (15., 45.),
             "sixteen classes": sit.pair_edges(4., 64., 16)}[name]
    nchunks, _ = chunks_of(yx, float(edges[-1]))
    assert nchunks >= 20
    ref = pairs_ref(yx, yx1, edges)
    assert ref["table"][:, 0].min() > 0 or name == "sixteen classes"
    got = ctx.pairs_points(yx, yx1, edges)
    check(got, ref, name)
    assert np.array_equal(bits(ctx.pairs_points(yx, yx1, edges)["table"]), bits(got["table"]))       # two calls: the same bits


# ------------------------------------------------------------------------------------------------ 3. second trips
def test_a_crowded_bin_and_more_rows_of_partials_than_the_table_kernel_has_lanes(ctx):
    """pairs_kernel streams a run of points kPairsTile at a time and cuts a row's points into home chunks of kPairsTile: 3 kPairsTile
    points inside one bin next to sparse ones take both loops past their first trip.  pairs_table_kernel's lane i sums the rows i,
    i + kPairsTile, ...: a strip of more than 2 kPairsTile rows of bins takes it to a third trip.  A dropped trip loses pairs, and the
    counts are compared as integers."""
    rng = np.random.default_rng(5)
    R = 8.
    side = R / BIN_FRAC
    sparse = np.stack([rng.uniform(0., 400., 2000), rng.uniform(0., 12., 2000)], axis=1)
    sparse[0] = 0.                                                    # the grid's lower corner
    blob = np.array([60 * side, 2 * side]) + rng.uniform(0.05 * side, 0.95 * side, (3 * TILE, 2))
    yx = np.concatenate([sparse, blob])[rng.permutation(2000 + 3 * TILE)]
    nchunks, crowd = chunks_of(yx, R)
    assert nchunks > 2 * TILE and crowd >= 3 * TILE
    yx1 = smooth_move(yx, 0.01)
    edges = (0.05, 0.5, 1., 2., 4., 8.)
    ref = pairs_ref(yx, yx1, edges)
    assert ref["table"][:, 0].min() >= 1000
    check(ctx.pairs_points(yx, yx1, edges), ref, "crowded bin")


# ------------------------------------------------------------------------------------------------ 4. the bin cap, one bin
def test_two_far_clusters_and_edges_wider_than_the_cloud(ctx):
    rng = np.random.default_rng(6)
    a = rng.uniform(0., 20., (300, 2))
    yx = np.concatenate([a, a[::-1] * 0.9 + 5000.])                   # 5000 km apart both ways: 10^8 bins of 0.5 km, far above the cap
    yx1 = smooth_move(yx, 0.002)
    edges = (0.25, 0.5, 1., 2.)
    ref = pairs_ref(yx, yx1, edges)
    assert ref["table"][:, 0].min() >= 50
    check(ctx.pairs_points(yx, yx1, edges), ref, "two clusters")
    wide = (0., 1e5)                                                  # one bin, every pair
    got = ctx.pairs_points(yx, yx1, wide)
    check(got, pairs_ref(yx, yx1, wide), "one bin")
    assert got["table"][0, 0] == 600 * 599 // 2


# ------------------------------------------------------------------------------------------------ 5. validity
def test_validity_coincident_points_and_tiny_clouds(ctx):
    yx = jitter_cloud(12)
    yx1 = smooth_move(yx)
    n = len(yx)
    yx[7] = yx[100]                                                   # q0 == 0 is excluded, even with edges[0] == 0
    yx0b, yx1b = yx.copy(), yx1.copy()
    yx0b[3, 1], yx0b[40, 0], yx1b[11, 0], yx1b[90, 1] = np.nan, -np.inf, np.inf, np.nan
    rng = np.random.default_rng(2)
    m0, m1 = (rng.uniform(size=n) > 0.1).astype(np.int8), rng.uniform(size=n) > 0.1
    edges = (0., 12., 30., 60.)
    for what, args, kw in (("coincident", (yx, yx1), {}), ("not finite", (yx0b, yx1b), {}), ("masks", (yx, yx1), {"mask0": m0, "mask1": m1}),
                           ("all of it", (yx0b, yx1b), {"mask0": m0, "mask1": m1})):
        ref = pairs_ref(*args, edges, **kw)
        got = ctx.pairs_points(*args, edges, **kw)
        check(got, ref, what)
        assert np.array_equal(bits(sit.PairDispersion(*args, edges, ctx=ctx, **kw)["table"]), bits(got["table"])), what
    assert ctx.pairs_points(yx, yx1, (0., 1e4))["table"][0, 0] == pairs_ref(yx, yx1, (0., 1e4))["table"][0, 0] == n * (n - 1) // 2 - 1
    for k in (0, 1, 2):
        got = ctx.pairs_points(yx[:k], yx1[:k], edges)
        assert got["npts"] == k and got["table"].shape == (3, 7)
        check(got, pairs_ref(yx[:k], yx1[:k], edges), "nP = %d" % k)
    assert ctx.pairs_points(yx[:2], yx1[:2], edges)["table"][:, 0].sum() == 1.
    none = ctx.pairs_points(yx, yx1, edges, mask0=np.zeros(n))
    assert none["npts"] == 0 and (none["table"] == 0.).all()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_refusals_leave_the_handle_and_a_tracker_on_it_as_they_were():
    trk, twin = start(), start()
    try:
        ctx = trk.ctx
        L, h = ctx._L, ctx._h
        yx = np.ascontiguousarray(jitter_cloud(8))
        yx1 = np.ascontiguousarray(smooth_move(yx))
        n = len(yx)
        table = np.full((16, 7), 7.)
        npts = C.c_int64(-5)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731

        def call(nP=n, a=yx, b=yx1, nc=2, edges=(1., 20., 40.), tab=table):
            e = np.array(edges, dtype=np.float64)
            return L.sitrk_pairs_points(h, nP, None if a is None else p(a), None if b is None else p(b), None, None, nc,
                                        None if edges is None else p(e), None if tab is None else p(tab), C.byref(npts))
        before = ctx.fetch()
        for kw, word in (({"nc": 0}, "nc must be"), ({"nc": 17, "edges": tuple(range(1, 19))}, "nc must be"), ({"edges": (1., 1., 2.)}, "increase"),
                         ({"edges": (2., 1., 3.)}, "increase"), ({"edges": (-1., 1., 3.)}, ">= 0"), ({"edges": (1., math.nan, 3.)}, "finite"),
                         ({"edges": (1., 2., math.inf)}, "finite"), ({"edges": None}, "null"), ({"tab": None}, "null"), ({"a": None}, "null"),
                         ({"b": None}, "null"), ({"nP": -1}, "nP")):
            assert call(**kw) == -1, kw
            assert word in L.sitrk_last_error(h).decode(), (kw, L.sitrk_last_error(h).decode())
        assert (table == 7.).all() and npts.value == -5               # refused before anything was written
        assert L.sitrk_pairs_since_mark(h, JREC0, 2, p(np.array([1., 2., 3.])), p(table), None) == -1 and b"no mark" in L.sitrk_last_error(h)
        assert L.sitrk_pairs_mark(None, 0, None) == -1
        trk.pairs_mark(JREC0)
        assert L.sitrk_pairs_since_mark(h, JREC0 - 1, 2, p(np.array([1., 2., 3.])), p(table), None) == -1 and b"before the mark" in L.sitrk_last_error(h)
        assert L.sitrk_pairs_since_mark(h, JREC0, 2, p(np.array([3., 2., 3.])), p(table), None) == -1
        # the handle works, and neither the refusals nor a table on host arrays touched the tracker's state
        check(ctx.pairs_points(yx, yx1, (1., 20., 40.)), pairs_ref(yx, yx1, (1., 20., 40.)), "after the refusals")
        after = ctx.fetch()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        j1 = advance(trk, JREC0, 2, 1)
        advance(twin, JREC0, 2, 1)
        a, b = ctx.fetch(), twin.ctx.fetch()
        assert np.array_equal(bits(a["yx"]), bits(b["yx"])) and all(np.array_equal(a[k], b[k]) for k in ("jiT", "alive", "kill_rec"))
        assert trk.pairs(j1, (1., 20., 40.))["npts"] > 0
        empty = _lib.Context(0)
        try:
            assert empty._L.sitrk_pairs_mark(empty._h, 0, None) == -1 and b"no buoys" in empty._L.sitrk_last_error(empty._h)
            assert empty._L.sitrk_pairs_since_mark(empty._h, 0, 2, p(np.array([1., 2., 3.])), p(table), None) == -1
            assert b"no buoys" in empty._L.sitrk_last_error(empty._h)
            with pytest.raises(_lib.SitrkError, match="no pair-dispersion call"):
                empty.pairs_kernel_ms()
            empty.pairs_free()
        finally:
            empty.close()
    finally:
        trk.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 7. a tracker
def test_tracker_tables_equal_the_host_arrays_in_every_bit():
    nP = 600
    rng = np.random.default_rng(8)
    first = np.full(nP, KSTRT, dtype=np.int64)
    last = np.full(nP, KSTRT + 20, dtype=np.int64)
    w = rng.permutation(nP)
    first[w[:15]] = KSTRT + 3                                         # start inside the span
    last[w[15:30]] = KSTRT + 5                                        # stop inside it
    last[w[30:40]] = KSTRT + 7                                        # stop with its last record: valid
    mask = (rng.uniform(size=nP) > 0.15).astype(np.int8)
    edges = sit.pair_edges(3., 40., 6)
    trk, twin = start(first=first, last=last), start(first=first, last=last)
    try:
        ctx = trk.ctx
        for t in (trk, twin):
            t.deform_mark(JREC0)
            t.mesh(3.5, JREC0)
        s0 = ctx.fetch()
        trk.pairs_mark(JREC0, mask)
        v0 = (s0["alive"] != 0) & (mask != 0)
        assert 0 < v0.sum() < (s0["alive"] != 0).sum()

        def host(sa, va, sb, jrec0, jrec1):
            vb = (sb["alive"] != 0) & (first <= jrec0) & (last >= jrec1)
            return ctx.pairs_points(sa["yx"], sb["yx"], edges, mask0=va, mask1=vb), vb

        def same(r, want, jrec0, jrec1, what):
            assert r["npts"] == want["npts"] and np.array_equal(bits(r["table"]), bits(want["table"])), what
            assert r["T"] == (jrec1 - jrec0 + 1) * RDT and sorted(r) == ["T", "npts", "table"], what

        ctx.run(JREC0 % K, JREC0, 2)
        j1 = JREC0 + 1
        r1 = trk.pairs(j1, edges)
        s1 = ctx.fetch()
        want1, v1 = host(s0, v0, s1, JREC0, j1)
        same(r1, want1, JREC0, j1, "two records")
        check(r1, pairs_ref(s0["yx"], s1["yx"], edges, v0, v1), "two records")
        assert r1["table"][:, 0].min() > 100 and r1["npts"] == (v0 & v1).sum() < v0.sum()
        ctx.sort_buoys()                                              # a re-sort between the calls changes nothing
        assert np.array_equal(bits(trk.pairs(j1, edges)["table"]), bits(r1["table"]))
        j2 = advance(trk, j1 + 1, 2, 2)                               # ... and the same t0, a longer T
        assert j2 == KSTRT + 7
        s2 = ctx.fetch()
        r2 = trk.pairs(j2, edges)
        want2, v2 = host(s0, v0, s2, JREC0, j2)
        same(r2, want2, JREC0, j2, "six records")
        out_of_span = (s2["alive"] != 0) & ~((first <= JREC0) & (last >= j2))
        assert out_of_span.sum() >= 20 and (s2["alive"] == 0).sum() > (s0["alive"] == 0).sum() and r2["npts"] < r1["npts"]
        # deform_mark and the mesh of the same handle are where a tracker without any of this has them
        twin.ctx.run(JREC0 % K, JREC0, 2)
        advance(twin, j1 + 1, 2, 2)
        a, b = trk.mesh_deform(j2), twin.mesh_deform(j2)
        assert np.array_equal(a["status"], b["status"]) and all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("div", "shr", "vor", "area0", "area1"))
        cells = trk.mesh_cells()
        da, db = ctx.deform_since_mark(j2, cells), twin.ctx.deform_since_mark(j2, cells)
        assert np.array_equal(bits(da[0]), bits(db[0])) and np.array_equal(da[1], db[1])
        assert np.array_equal(bits(s2["yx"]), bits(twin.ctx.fetch()["yx"]))
        # a second mark replaces the first
        trk.pairs_mark(j2 + 1)
        ctx.run((j2 + 1) % K, j2 + 1, 1)
        s3 = ctx.fetch()
        want3, _ = host(s2, s2["alive"] != 0, s3, j2 + 1, j2 + 1)
        same(trk.pairs(j2 + 1, edges), want3, j2 + 1, j2 + 1, "second mark")
        # pairs_free and set_buoys cancel it
        trk.pairs_free()
        with pytest.raises(ValueError, match="no mark"):
            trk.pairs(j2 + 1, edges)
        with pytest.raises(_lib.SitrkError, match="no mark"):
            ctx.pairs_since_mark(j2 + 1, edges)
        trk.pairs_mark(j2 + 2)
        trk.set_buoys(s3["yx"], s3["jiT"])
        with pytest.raises(ValueError, match="no mark"):
            trk.pairs(j2 + 2, edges)
        with pytest.raises(_lib.SitrkError, match="no mark"):
            ctx.pairs_since_mark(j2 + 2, edges)
    finally:
        trk.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 8. command line
def test_cli_pairs_flag(tmp_path, monkeypatch, capsys):
    """The series file holds f4 positions.  The seeds are f4 values, so record 0 holds the t0 of window 0 exactly: its counts and
    npts equal the restatement's on the file's positions as integers and sum r0 within the bound above.  A t1 coordinate of the file
    is off by at most eps = half an f4 ulp at its size, a separation r1 by at most dr = 2 sqrt(2) eps, so d by dr and e by de = dr/r0:
    the other sums are held to n terms of dr or de to first order, with the higher orders written out."""
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=300)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F"]
    plain = drv.main(argv)
    t, ids, _, yx_plain, mk_plain = ncio.LoadNCdata(plain["files"][0], krec=-1, lmask=True)
    capsys.readouterr()
    spec, NWIN, EVERY = "20:160:4", 5, 2
    edges = sit.pairs_arg(spec)
    out = drv.main(argv + ["--pairs", spec, "--pairs-window", str(NWIN), "--pairs-every", str(EVERY)])
    log = capsys.readouterr().out
    Nt, kstrt = out["Nt"], out["kstrt"]
    assert Nt == 14 and len(out["files"]) == 3 and out["files"][:2] == plain["files"]
    fp = out["files"][2]
    assert fp == './npz/NEMO-SI3_TEST4_EXP01_pairs_nemoTsi3_idlSeed_19961215h00_19961215h14.npz' and os.path.exists(fp)
    _, ids2, _, yx2, mk2 = ncio.LoadNCdata(out["files"][0], krec=-1, lmask=True)
    assert np.array_equal(ids2, ids) and np.array_equal(mk2, mk_plain) and np.array_equal(bits(yx2), bits(yx_plain))
    assert np.array_equal(out["vJIt"], plain["vJIt"]) and np.array_equal(out["iAlive"], plain["iAlive"])
    with np.load(fp) as z:
        d = {k: z[k] for k in z.files}
    wins = drv.pair_windows(Nt, kstrt, NWIN, EVERY)
    assert [len(w[1]) for w in wins] == [3, 3, 2]
    assert sorted(d) == sorted(["edges", "windows", "time0"] + ["w%d_%s" % (k, n) for k in range(3) for n in ("jrec1", "T", "pairs", "npts")])
    assert np.array_equal(d["edges"], edges) and np.array_equal(d["windows"], [(w[0], w[1][-1]) for w in wins])
    assert np.array_equal(d["time0"], [t[w[0] - kstrt] for w in wins])
    for k, (j0, js) in enumerate(wins):
        pre = "w%d_" % k
        assert np.array_equal(d[pre + "jrec1"], js) and np.array_equal(d[pre + "T"], [(j - j0 + 1) * 3600. for j in js])
        assert d[pre + "pairs"].shape == (len(js), 4, 7) and d[pre + "pairs"].dtype == np.float64 and d[pre + "npts"].shape == (len(js),)
        assert (np.diff(d[pre + "npts"]) <= 0).all() and d[pre + "npts"][0] <= len(ids)
        for q, j in enumerate(js):
            line = "--pairs window %d record %d (T = %g s): %d points, pairs per class %s" % (
                k, j, (j - j0 + 1) * 3600., d[pre + "npts"][q], ' '.join('%d' % n for n in d[pre + "pairs"][q, :, 0]))
            assert line in log, line
    # window 0 against the restatement on the file's positions
    assert (mk_plain[0] == 1).all()
    yx0 = yx_plain[0]
    for q, j in enumerate(wins[0][1]):
        k1 = j - kstrt + 1                                            # the record of the series behind the step of j
        m1 = (mk_plain[k1] == 1) & (mk_plain[k1 + 1] == 1)            # stepped at j and alive behind it
        yx1 = yx_plain[k1]
        ref = pairs_ref(yx0, yx1, edges, mask1=m1)
        tab = d["w0_pairs"][q]
        assert d["w0_npts"][q] == ref["npts"] and np.array_equal(tab[:, 0], ref["table"][:, 0]) and tab[:, 0].min() >= 10
        dr = 2. * math.sqrt(2.) * 0.5 * float(np.spacing(np.float32(np.abs(yx1[m1]).max())))
        for cl, tt in enumerate(ref["terms"]):
            n = tt.shape[1]
            r0, e, dd = tt[0], np.abs(tt[1]), np.sqrt(tt[5])
            de = dr / r0
            slack = [0., de, de, 2. * e * de + de * de, 3. * e * e * de + 3. * e * de * de + de ** 3, 2. * dd * dr + dr * dr]
            for col in range(6):
                want, mag = math.fsum(tt[col]), math.fsum(np.abs(tt[col]))
                bound = (n + HALF_ULPS[col]) * 2. ** -53 * mag + 1.001 * math.fsum(np.broadcast_to(slack[col], (n,)))
                print("window 0 table %d class %d: %-10s file %.17g  fsum %.17g  |diff| %.3g  bound %.3g" % (q, cl, _lib.PAIRS_COLS[1 + col],
                                                                                                      tab[cl, 1 + col], want, abs(tab[cl, 1 + col] - want), bound))
                assert abs(tab[cl, 1 + col] - want) <= bound, (q, cl, col)
    # next to --deform: both files, the same tables, the same trajectories
    both = drv.main(argv + ["--pairs", spec, "--pairs-window", str(NWIN), "--pairs-every", str(EVERY), "--deform", "15", "--deform-window", "7"])
    assert len(both["files"]) == 4 and "_deformation_" in both["files"][2] and both["files"][3] == fp
    assert np.array_equal(both["vJIt"], plain["vJIt"]) and np.array_equal(both["iAlive"], plain["iAlive"])
    with np.load(fp) as z:
        assert sorted(z.files) == sorted(d) and all(z[k].tobytes() == d[k].tobytes() for k in d)
