"""Features of a map on the GPU (sitrk_label_raster / sitrk_mesh_features) against the restatement of
tests/test_features.py.  All integer: every comparison is array_equal, there is no tolerance anywhere.  The rasters are the
smallest at which each phase can go wrong -- one pixel, one row, a tile less and more than a tile, partial tiles on both rims
with three merge levels, many tiles long and less than one high -- and the masks the worst cases for propagation: a one-pixel
serpentine through every row, a comb, a spiral, diagonals that are dust at conn 4, and random masks near the two percolation
thresholds.  Those rasters all fit one grid-stride trip and spans of the least length; the tests on TRIP2, SPAN5 and DEEP
(tests/test_features.py) take the same masks, and two combs that mesh, to the sizes at which the host gives the kernels several
trips, longer spans, merge borders of more than one trip and seven merge levels both ways."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import driver as drv
from test_driver import make_case
from test_features import (DEEP, SPAN5, TRIP2, bars, bars_expected, checkerboard, comb, diagonals, full_row, interleaved_combs,
                           interleaved_labels, label_ref, random_mask, same_result, serpentine, spiral, table_ref)
from test_gpu_mesh import JREC0, K, advance, start

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = getattr(_lib, "LABEL_TILE", 64)
SHAPES = [(1, 1), (1, 300), (T - 1, T + 1), (67, 131), (200, 333), (3, 8 * T + 5)]
RATES = ("div", "shr", "vor")


@pytest.fixture(scope="module")
def ctx():
    c = sit.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def want_labels(kind, ny, nx, conn):
    lab = label_ref(make_mask(kind, ny, nx), conn)
    lab.setflags(write=False)
    return lab


def border_cut(ny, nx):
    """a pixel on a tile border where the comb's tooth and the spiral's first winding run straight, or None on a raster too small"""
    if nx <= T:
        return None, None
    tooth = (ny // 2, T) if ny >= 3 else None                         # column T is even: a tooth, cut half way down
    wind = (0, T) if ny < 3 else (ny - 1, T - 1)                       # the first winding: along row 0, back along the last row
    return tooth, wind


@functools.lru_cache(maxsize=None)
def make_mask(kind, ny, nx):
    tooth, wind = border_cut(ny, nx)
    if kind == "all":
        m = np.ones((ny, nx), dtype=np.int8)
    elif kind == "none":
        m = np.zeros((ny, nx), dtype=np.int8)
    elif kind == "corner":
        m = np.zeros((ny, nx), dtype=np.int8)
        m[-1, -1] = 1
    elif kind == "checker":
        m = checkerboard(ny, nx)
    elif kind == "serpentine":
        m = serpentine(ny, nx)
    elif kind == "comb":
        m = comb(ny, nx)
    elif kind == "comb_cut":
        m = comb(ny, nx, cut=tooth)
    elif kind == "spiral":
        m = spiral(ny, nx)
    elif kind == "spiral_cut":
        m = spiral(ny, nx, cut=wind)
    elif kind == "diagonals":
        m = diagonals(ny, nx)
    elif kind == "interleaved":
        m = interleaved_combs(ny, nx)
    else:
        density, seed = kind
        m = random_mask(ny, nx, density, seed)
    m.setflags(write=False)
    return m


SIMPLE = ("all", "none", "corner", "checker")
WINDING = ("serpentine", "comb", "comb_cut", "spiral", "spiral_cut", "diagonals")
RANDOM = tuple((d, s) for d in (0.41, 0.59) for s in (1, 2, 3))


def check_case(ctx, kind, ny, nx, conn):
    """one mask and connectivity through every form of the call"""
    m, want = make_mask(kind, ny, nx), want_labels(kind, ny, nx, conn)
    what = (kind, ny, nx, conn)
    got = ctx.label_raster(m, conn=conn)
    tab = same_result(got, want, what=what)
    again = ctx.label_raster(m, conn=conn)                             # two calls: the same bits
    assert np.array_equal(again["labels"], got["labels"]) and np.array_equal(again["table"], got["table"]), what
    same_result(ctx.label_raster(m, conn=conn, min_pix=2, labels=False), want, min_pix=2, what=what)
    largest = int(tab[:, 1].max()) if len(tab) else 0
    none = ctx.label_raster(m, conn=conn, min_pix=largest + 1, labels=False)
    assert none["labels"] is None and none["nfeat"] == 0 and none["table"].shape == (0, 12) and none["ncomp"] == got["ncomp"], what
    assert (none["ncomp"] > 0) == bool(m.any())
    if len(tab) > 1:                                                   # truncated: the first rows, and nfeat still all of them
        same_result(ctx.label_raster(m, conn=conn, maxfeat=len(tab) // 2), want, maxfeat=len(tab) // 2, what=what)
        same_result(ctx.label_raster(m, conn=conn, maxfeat=0, labels=False), want, maxfeat=0, what=what)
    return tab


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_simple_masks(ctx, ny, nx):
    for kind in SIMPLE:
        for conn in (4, 8):
            tab = check_case(ctx, kind, ny, nx, conn)
            if kind == "all":
                assert tab[0, [0, 1, 11]].tolist() == [0, ny * nx, 2 * (ny + nx)]
            if kind == "corner":
                assert tab.tolist() == [[ny * nx - 1, 1, ny - 1, ny - 1, nx - 1, nx - 1, ny - 1, nx - 1, (ny - 1) ** 2, (nx - 1) ** 2,
                                         (ny - 1) * (nx - 1), 4]]
            if kind == "checker" and ny > 1:                           # every pixel alone, against one component through every corner
                assert len(tab) == ((ny * nx + 1) // 2 if conn == 4 else 1)


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_winding_masks(ctx, ny, nx):
    tooth, wind = border_cut(ny, nx)
    for kind in WINDING:
        if (kind == "comb_cut" and tooth is None) or (kind == "spiral_cut" and wind is None):
            continue
        for conn in (4, 8):
            tab = check_case(ctx, kind, ny, nx, conn)
            if kind in ("serpentine", "comb", "spiral"):
                assert len(tab) == 1 and tab[0, 1] == make_mask(kind, ny, nx).sum()
            if kind in ("comb_cut", "spiral_cut"):                     # one pixel out at a tile border: two components
                assert len(tab) == 2 and make_mask(kind, ny, nx).sum() == make_mask(kind[:-4], ny, nx).sum() - 1


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_random_masks_near_the_percolation_thresholds(ctx, ny, nx):
    for kind in RANDOM:
        for conn in (4, 8):
            tab = check_case(ctx, kind, ny, nx, conn)
            if (ny, nx) == (200, 333) and (kind[0], conn) in ((0.41, 8), (0.59, 4)):
                lab = want_labels(kind, ny, nx, conn)
                big = tab[np.argmax(tab[:, 1])]
                tiles = {(j // T, i // T) for j, i in zip(*np.nonzero(lab == big[0]))}
                assert len(tab) > 100 and len(tiles) > 4, (kind, conn, len(tab), len(tiles))


# ------------------------------------------------------------------------------------------------ rasters of a production size
# TRIP2 and SPAN5 (tests/test_features.py, where a CPU test holds them to the constants of the source) are past the sizes at
# which the host gives the kernels more than one grid-stride trip, spans of more than kLbMinTrips pieces and merge borders of
# more than one trip; the shapes above are all below them.  The same check_case, the same restatement, array_equal only.
LARGE = (TRIP2, SPAN5)


@pytest.mark.parametrize("density,conn", [(0.41, 8), (0.59, 4)])
@pytest.mark.parametrize("ny,nx", LARGE)
def test_random_masks_on_large_rasters(ctx, ny, nx, density, conn):
    """near the percolation threshold of the connectivity: tens of thousands of components, the largest over most of the raster"""
    kind = (density, 1)
    tab = check_case(ctx, kind, ny, nx, conn)
    lab = want_labels(kind, ny, nx, conn)
    big = tab[np.argmax(tab[:, 1])]
    jj, ii = np.nonzero(lab == big[0])
    tiles = len(np.unique((jj // T) * (nx // T + 1) + ii // T))
    # 10 000 components and 100 tiles at SPAN5, as measured on the restatement with room to spare (29 021 and 61 327 components,
    # 347 and 206 tiles); both scale with the area, and TRIP2 has a quarter of it
    scale = (ny * nx) / (SPAN5[0] * SPAN5[1])
    assert len(tab) > 10000 * scale and tiles > 100 * scale, (kind, conn, len(tab), tiles)


# (the comb has a million runs at SPAN5, and its restatement takes too long there: it runs at TRIP2)
WINDING_LARGE = [(s, k) for s in LARGE for k in ("serpentine", "spiral", "interleaved")] + [(TRIP2, "comb"), (TRIP2, "comb_cut")]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape,kind", WINDING_LARGE, ids=["%dx%d-%s" % (s + (k,)) for s, k in WINDING_LARGE])
def test_winding_masks_on_large_rasters(ctx, shape, kind, conn):
    """one component through every tile -- the longest parent chains the merge can leave --, and two that alternate along every
    row, so that in every piece of every span the flatten and table kernels choose which of two rows stays in registers"""
    ny, nx = shape
    tab = check_case(ctx, kind, ny, nx, conn)
    if kind == "interleaved":
        lab, sizes = interleaved_labels(ny, nx)
        assert np.array_equal(want_labels(kind, ny, nx, conn), lab) and tab[:, :2].tolist() == [[0, sizes[0]], [2 * nx + 2, sizes[1]]]
    elif kind == "comb_cut":
        assert len(tab) == 2 and make_mask(kind, ny, nx).sum() == make_mask("comb", ny, nx).sum() - 1
    else:
        assert len(tab) == 1 and tab[0, 1] == make_mask(kind, ny, nx).sum() and tab[0, 2:6].tolist() == [0, ny - 1, 0, nx - 1]


def test_closed_form_masks_on_the_deepest_raster(ctx):
    """DEEP: spans of 33 pieces that end inside a row, seven merge levels both ways, 33 grid-stride trips.  Expected values in
    closed form (their formulas are checked against the restatement on small rasters in tests/test_features.py)"""
    ny, nx = DEEP
    whole = np.ones((ny, nx), dtype=np.int8)
    striped = bars(ny, nx)
    labels, table = bars_expected(ny, nx)
    assert len(table) == 1367 and table[-1, 1] == nx and striped.sum() == table[:, 1].sum()      # the last bar is one row
    for conn in (4, 8):
        got = ctx.label_raster(whole, conn=conn)
        assert got["table"].tolist() == [full_row(ny, nx)] and (got["nfeat"], got["ncomp"], got["nactive"]) == (1, 1, ny * nx), conn
        assert got["labels"].dtype == np.int32 and not got["labels"].any(), conn
        got = ctx.label_raster(striped, conn=conn)
        assert got["table"].dtype == np.int64 and np.array_equal(got["table"], table), conn
        assert (got["nfeat"], got["ncomp"], got["nactive"]) == (len(table), len(table), int(table[:, 1].sum())), conn
        assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], labels), conn
        bare = ctx.label_raster(striped, conn=conn, min_pix=nx + 1, maxfeat=1000, labels=False)   # without the short bar, truncated
        assert bare["labels"] is None and np.array_equal(bare["table"], table[:1000]), conn
        assert (bare["nfeat"], bare["ncomp"], bare["nactive"]) == (len(table) - 1, len(table), int(table[:, 1].sum())), conn


def test_longest_sides(ctx):
    """32768 pixels a side are labelled -- nine merge levels along one column --, one more is refused"""
    m = np.ones((32768, 1), dtype=np.int8)
    m[5::64] = 0
    for mask in (m, m.T.copy()):
        for conn in (4, 8):
            same_result(ctx.label_raster(mask, conn=conn), label_ref(mask, conn))
    whole = ctx.label_raster(np.ones((32768, 1), dtype=np.int8))
    assert whole["table"].tolist() == [[0, 32768, 0, 32767, 0, 0, 32767 * 32768 // 2, 0, 32767 * 32768 * 65535 // 6, 0, 0, 2 * 32769]]
    for shape in ((32769, 1), (1, 32769)):
        with pytest.raises(_lib.SitrkError, match="1..32768"):
            ctx.label_raster(np.ones(shape, dtype=np.int8))
    assert ctx.label_raster(np.ones((2, 2)))["ncomp"] == 1


def test_argument_errors_leave_the_handle_usable(ctx):
    lib, h, p = ctx._L, ctx._h, _lib._ptr
    mask = np.ones((4, 5), dtype=np.int8)
    table = np.full((3, 12), 77, dtype=np.int64)
    lab = np.full((4, 5), 55, dtype=np.int32)
    n = [_lib._i64(7) for _ in range(3)]

    def call(ny=4, nx=5, m=mask, conn=8, min_pix=1, maxfeat=3, tab=table):
        return lib.sitrk_label_raster(h, ny, nx, p(m), conn, min_pix, maxfeat, p(lab), p(tab), *[C.byref(x) for x in n])

    for kw, msg in (({"conn": 5}, b"conn must be 4"), ({"conn": 0}, b"conn"), ({"ny": 0}, b"ny and nx"), ({"nx": 32769}, b"1..32768"),
                    ({"ny": 32768, "nx": 8193}, b"2^28"), ({"min_pix": 0}, b"min_pix"), ({"maxfeat": -1}, b"maxfeat"), ({"tab": None}, b"null table"),
                    ({"m": None}, b"null mask")):
        assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
    assert (table == 77).all() and (lab == 55).all() and [x.value for x in n] == [7, 7, 7]
    assert call() == 0 and table[0].tolist()[:2] == [0, 20] and (table[1:] == 77).all() and (lab == 0).all()
    assert [x.value for x in n] == [1, 1, 20]
    assert call(maxfeat=0, tab=None) == 0 and [x.value for x in n] == [1, 1, 20]
    assert lib.sitrk_label_raster(h, 4, 5, p(mask), 4, 1, 0, None, None, None, None, None) == 0       # every output is optional
    ms = ctx.features_kernel_ms()
    assert len(ms) == 3 and all(x >= 0. for x in ms) and ms[1] > 0.
    fresh = sit.Context(0)
    try:
        with pytest.raises(_lib.SitrkError, match="no labelling call"):
            fresh.features_kernel_ms()
    finally:
        fresh.close()
    r = sit.LabelRaster(checkerboard(5, 7), conn=4, min_pix=1, ctx=ctx)
    assert r["ncomp"] == 18 and sit.feature_table(r["table"], (0., 0., 2., 5, 7))["area_km2"].tolist() == [4.] * 18


# ------------------------------------------------------------------------------------------------ the mesh path
def expected_mask(owner, rates, what, sgn, thr):
    own = owner >= 0
    at = np.maximum(owner, 0)
    with np.errstate(invalid="ignore"):
        if what == "tot":
            hit = rates["div"][at] * rates["div"][at] + rates["shr"][at] * rates["shr"][at] >= thr * thr
        else:
            hit = sgn * rates[what][at] >= thr
    return own & hit


def test_mesh_features_equal_labelling_the_map_of_mesh_raster_and_mesh_deform():
    trk = start()
    try:
        ctx = trk.ctx
        s0 = ctx.fetch()
        trk.mesh(3.5, JREC0)
        jrec1 = advance(trk, JREC0, 3, 3)
        rates = trk.mesh_deform(jrec1)
        lo, hi = s0["yx"].min(axis=0), s0["yx"].max(axis=0)
        grid = sit.raster_grid(lo[0] + 9., hi[0] + 3., lo[1] - 2., hi[1] - 11., 0.9)        # the mesh reaches beyond it on two sides
        assert grid[3] > T and grid[4] > T
        state = ctx.fetch()
        for at in ("t0", "t1"):
            owner = trk.mesh_raster(jrec1, grid, at=at, fields=False)["owner"]
            owned = owner >= 0
            assert 0.3 < owned.mean() < 1.
            for what in RATES + ("tot",):
                for sgn in ((1,) if what == "tot" else (1, -1)):
                    if what == "tot":
                        f = rates["div"][owner[owned]] ** 2 + rates["shr"][owner[owned]] ** 2
                        thr = float(np.sqrt(np.median(f)))
                    else:
                        thr = float(np.median(sgn * rates[what][owner[owned]]))
                    mask = expected_mask(owner, rates, what, sgn, thr)
                    assert 0.3 < mask.sum() / owned.sum() < 0.7, (at, what, sgn)              # about half of the owned pixels pass
                    for conn in (4, 8):
                        want = label_ref(mask, conn)
                        got = trk.mesh_features(jrec1, grid, what=what, thr=thr, sgn=sgn, conn=conn, at=at, labels=True)
                        tab = same_result(got, want, what=(at, what, sgn, conn))
                        assert len(tab) > 3
                    bare = trk.mesh_features(jrec1, grid, what=what, thr=thr, sgn=sgn, conn=8, min_pix=3, maxfeat=2, at=at)
                    same_result(bare, want, min_pix=3, maxfeat=2, what=(at, what, sgn, "bare"))
                    host = ctx.label_raster(mask, conn=8)                                     # ... and the host-mask entry point agrees
                    assert np.array_equal(host["labels"], want) and np.array_equal(host["table"], tab)
        ms = ctx.features_kernel_ms()
        assert all(x >= 0. for x in ms) and ms[1] > 0.
        # the mesh, its rates and the tracker are where they were
        after = trk.mesh_deform(jrec1)
        assert np.array_equal(after["status"], rates["status"]) and all(np.array_equal(after[n].view(np.uint64), rates[n].view(np.uint64)) for n in RATES)
        assert np.array_equal(ctx.fetch()["yx"].view(np.uint64), state["yx"].view(np.uint64))
    finally:
        trk.close()


def test_mesh_features_errors_and_the_empty_mesh():
    trk = start()
    try:
        ctx = trk.ctx
        lib, h, p = ctx._L, ctx._h, _lib._ptr
        grid = (-70., -50., 5., 20, 21)
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_features(JREC0, grid, thr=0.)
        assert trk.mesh(0.01, JREC0, slot=2)["nQ"] == 0                # an empty mesh: nothing is active
        ctx.run(JREC0 % K, JREC0, 1)
        r = trk.mesh_features(JREC0, grid, what="div", thr=-1., slot=2, labels=True)
        assert (r["nfeat"], r["ncomp"], r["nactive"]) == (0, 0, 0) and (r["labels"] == -1).all() and r["table"].shape == (0, 12)
        assert trk.mesh(3.5, JREC0 + 1)["nQ"] > 256
        ctx.run((JREC0 + 1) % K, JREC0 + 1, 1)
        table = np.full((3, 12), 77, dtype=np.int64)
        n = _lib._i64(0)

        def call(mesh=0, jrec1=JREC0 + 1, at=0, y0=-70., x0=-50., d=5., ny=20, nx=21, what=3, sgn=1, thr=0., conn=8, min_pix=1, maxfeat=3,
                 tab=table):
            return lib.sitrk_mesh_features(h, mesh, jrec1, at, y0, x0, d, ny, nx, what, sgn, thr, conn, min_pix, maxfeat, None, p(tab),
                                           C.byref(n), None, None)

        for kw, msg in (({"mesh": 8}, b"mesh must be in 0..7"), ({"mesh": 1}, b"mesh 1 is empty"), ({"jrec1": JREC0}, b"before the mesh's t0"),
                        ({"at": 2}, b"at_t1"), ({"d": 0.}, b"d_km"), ({"y0": np.nan}, b"finite"), ({"ny": 0}, b"ny and nx"),
                        ({"nx": 32769}, b"1..32768"), ({"conn": 5}, b"conn"), ({"min_pix": 0}, b"min_pix"), ({"maxfeat": -2}, b"maxfeat"),
                        ({"tab": None}, b"null table"), ({"what": 4}, b"what must be"), ({"what": -1}, b"what must be"),
                        ({"what": 3, "sgn": -1}, b"sgn = +1"), ({"what": 3, "thr": -1e-9}, b"thr >= 0"), ({"sgn": 0}, b"sgn must be"),
                        ({"what": 0, "sgn": 2}, b"sgn must be"), ({"thr": np.nan}, b"thr must be finite"), ({"thr": np.inf}, b"thr must be finite")):
            assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
        assert (table == 77).all()
        assert call() == 0 and n.value >= 1 and table[0, 1] > 10          # thr 0 on tot: every owned pixel
        ctx.run((JREC0 + 2) % K, JREC0 + 2, 1)                          # the handle goes on
        assert np.isfinite(ctx.fetch()["yx"]).all()
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ command line
def test_cli_deform_features_flag(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F", "--deform", "30", "--deform-window", "5", "--deform-grid", "4"]
    plain = drv.main(argv)                                            # without the flag: the file every run wrote before
    assert "--deform-features" not in capsys.readouterr().out
    with np.load(plain["files"][2]) as z:
        e = {k: z[k] for k in z.files}
    own = e["m0_w0_owner"]
    tot2 = e["m0_w0_div"] ** 2 + e["m0_w0_shr"] ** 2
    thr = float(np.sqrt(np.median(tot2[own[own >= 0]])))
    out = drv.main(argv + ["--deform-features", "tot@%r@2@4" % thr])
    log = capsys.readouterr().out
    with np.load(out["files"][2]) as z:
        d = {k: z[k] for k in z.files}
    new = ["features"] + ["m0_w%d_features%s" % (w, s) for w in range(3) for s in ("", "_counts")]
    assert sorted(d) == sorted(list(e) + new) and not any("features" in k for k in e)
    for k in e:                                                       # everything else is what it was
        assert np.array_equal(d[k], e[k]), k
    assert d["features"].tolist() == [3., 1., thr, 2., 4.]
    grid = tuple(d["grid"][:3]) + (int(d["grid"][3]), int(d["grid"][4]))
    for w in range(3):
        pre = "m0_w%d_" % w
        rates = {n: d[pre + n] for n in RATES}
        want = label_ref(expected_mask(d[pre + "owner"], rates, "tot", 1, thr), 4)
        tab, ncomp, nact = table_ref(want, 2)
        assert d[pre + "features"].dtype == np.int64 and np.array_equal(d[pre + "features"], tab), w
        assert d[pre + "features_counts"].tolist() == [len(tab), ncomp, nact] and ncomp >= len(tab) > 0
        line = [ln for ln in log.splitlines() if "--deform-features window %d mesh 0" % w in ln]
        longest = sit.feature_table(tab, grid)["length_km"].max()
        assert len(line) == 1 and "%d features" % len(tab) in line[0] and "longest %.3f km" % longest in line[0], line
    # tools/deformation.py --grid --features on the written series: the mask from its own owners and rates
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    fc, fout = str(tmp_path / "cells.npy"), str(tmp_path / "feat.npz")
    np.save(fc, d["m0_w0_cells"])
    assert tool.main(["-i", out["files"][0], "-c", fc, "-k", "0", "-K", "5", "--grid", "3", "--features", "conv@0@1@8", "-o", fout]) == 0
    assert "--features conv@0@1@8" in capsys.readouterr().out
    with np.load(fout) as z:
        m = {k: z[k] for k in z.files}
    want = label_ref(expected_mask(m["owner"], {"div": m["div"]}, "div", -1, 0.), 8)
    tab, ncomp, nact = table_ref(want)
    assert np.array_equal(m["features"], tab) and m["features_counts"].tolist() == [len(tab), ncomp, nact] and 0 < nact < (m["owner"] >= 0).sum()
    assert m["features_arg"].tolist() == [0., -1., 0., 1., 8.]
