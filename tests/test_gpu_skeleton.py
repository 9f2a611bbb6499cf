"""Skeletons of a label map on the GPU (sitrk_skeleton_raster / sitrk_keep_skeleton) against the restatement of
tests/test_skeleton.py.  All integer: every comparison is array_equal, there is no tolerance anywhere.  The rasters and the maps
are those of tests/test_gpu_track.py; the shapes behind them are the ones where the batching of the thinning kernel can go wrong
-- more sub-iterations than a launch runs, several tiles, a tile corner in the middle of a shape, runs that end inside a batch
-- and TRIP2 of tests/test_features.py, where every grid-stride kernel of sitrk_skeleton.hip takes a second trip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import driver as drv
from sitrack_amd import features as ft
from test_driver import make_case
from test_features import TRIP2, checkerboard, comb, label_ref, random_mask, serpentine
from test_gpu_mesh import JREC0, advance, start
from test_skeleton import kernel_constants, labels_of, nodes_ref, one, plus, skeleton_ref, skeleton_table_ref, thin_ref
from test_track import kept_ref, permuted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONST = kernel_constants()
B, TILE = CONST["kSkBatch"], CONST["kSkTile"]
SHAPES = [(1, 1), (1, 300), (63, 65), (67, 131), (200, 333), (3, 517)]
COUNTS = ("nfeat", "nnode", "nskel", "nsub", "converged")


@pytest.fixture(scope="module")
def ctx():
    c = sit.Context(0)
    yield c
    c.close()


MAPS = {"random 0.41/8": lambda ny, nx: label_ref(random_mask(ny, nx, 0.41, 1), 8),
        "random 0.59/4": lambda ny, nx: label_ref(random_mask(ny, nx, 0.59, 2), 4),
        "full": lambda ny, nx: label_ref(np.ones((ny, nx), dtype=np.int8), 4),
        "empty": lambda ny, nx: np.full((ny, nx), -1, dtype=np.int32),
        "checkerboard": lambda ny, nx: label_ref(checkerboard(ny, nx), 4),
        "serpentine": lambda ny, nx: label_ref(serpentine(ny, nx), 4),
        "comb": lambda ny, nx: label_ref(comb(ny, nx), 8),
        "not canonical": lambda ny, nx: permuted(label_ref(random_mask(ny, nx, 0.59, 2), 4), 12)}


def want(name, ny, nx, max_sub=4096):
    return skeleton_ref((name, ny, nx), lambda: MAPS[name](ny, nx), max_sub)


def same(got, ref, what, skel=True, maxfeat=None, maxnode=None):
    """a result dict of the binding against the restatement"""
    for n in COUNTS:
        assert got[n] == ref[n], (what, n, got[n], ref[n])
    tab = ref["table"] if maxfeat is None else ref["table"][:maxfeat]
    nod = ref["nodes"] if maxnode is None else ref["nodes"][:maxnode]
    assert got["table"].dtype == np.int64 and got["table"].shape == tab.shape and np.array_equal(got["table"], tab), what
    assert got["nodes"].dtype == np.int64 and got["nodes"].shape == nod.shape and np.array_equal(got["nodes"], nod), what
    if skel:
        assert got["skel"].dtype == np.int8 and np.array_equal(got["skel"], ref["skel"]), what
    else:
        assert got["skel"] is None, what


# ------------------------------------------------------------------------------------------------ both entry points
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_skeleton_equals_the_restatement(ctx, ny, nx):
    for name in MAPS:
        ref = want(name, ny, nx)
        assert ref["converged"] == 1
        same(ctx.skeleton_raster(ref["labels"]), ref, (name, ny, nx, "raster"))
        ctx.keep_put(2, ref["labels"], conn=4, min_pix=3)
        same(ctx.keep_skeleton(2, skel=True), ref, (name, ny, nx, "keep"))
        same(ctx.keep_skeleton(2), ref, (name, ny, nx, "keep, no skeleton"), skel=False)
        k = ctx.keep_get(2)                                            # the kept slot is what it was
        assert (k["shape"], k["conn"], k["min_pix"]) == ((ny, nx), 4, 3) and np.array_equal(k["labels"], ref["labels"]), name
    ctx.keep_free(2)
    if (ny, nx) == (200, 333):
        assert want("random 0.59/4", ny, nx)["nnode"] > 1000 and want("random 0.59/4", ny, nx)["nsub"] > 4
        assert want("full", ny, nx)["nsub"] > 2 * B and len(want("not canonical", ny, nx)["table"]) > 500


def test_forms_of_the_call(ctx):
    ny, nx = 67, 131
    ref = want("random 0.59/4", ny, nx)
    lab = ref["labels"]
    nf, nn = ref["nfeat"], ref["nnode"]
    assert nf > 30 and nn > 60
    lib, h, p = ctx._L, ctx._h, _lib._ptr
    ctx.keep_put(5, lab)
    i64, cint = _lib._i64, C.c_int

    def raster(max_sub, maxfeat, maxnode, skel, table, nodes, *counts):
        return lib.sitrk_skeleton_raster(h, ny, nx, p(lab), max_sub, maxfeat, maxnode, p(skel), p(table), p(nodes), *counts)

    def keep(max_sub, maxfeat, maxnode, skel, table, nodes, *counts):
        return lib.sitrk_keep_skeleton(h, 5, max_sub, maxfeat, maxnode, p(skel), p(table), p(nodes), *counts)

    for call in (raster, keep):
        # truncation: the first rows only, the rest of the arrays untouched; the counts say how many there are
        cf, cn = nf // 3, nn // 3
        tab, nod = np.full((cf + 3, 7), 77, dtype=np.int64), np.full((cn + 3, 3), 77, dtype=np.int64)
        c = [i64(-5), i64(-5), i64(-5), cint(-5), cint(-5)]
        assert call(4096, cf, cn, None, tab, nod, *[C.byref(x) for x in c]) == 0
        assert np.array_equal(tab[:cf], ref["table"][:cf]) and (tab[cf:] == 77).all()
        assert np.array_equal(nod[:cn], ref["nodes"][:cn]) and (nod[cn:] == 77).all()
        assert [x.value for x in c] == [ref[n] for n in COUNTS]
        # more room than rows
        tab, nod = np.full((nf + 3, 7), 77, dtype=np.int64), np.full((nn + 3, 3), 77, dtype=np.int64)
        assert call(4096, nf + 3, nn + 3, None, tab, nod, None, None, None, None, None) == 0   # every count is optional
        assert np.array_equal(tab[:nf], ref["table"]) and (tab[nf:] == 77).all()
        assert np.array_equal(nod[:nn], ref["nodes"]) and (nod[nn:] == 77).all()
        # nothing but the counts and the skeleton
        sk = np.full((ny, nx), 77, dtype=np.int8)
        c = [i64(-5), i64(-5), i64(-5), cint(-5), cint(-5)]
        assert call(4096, 0, 0, sk, None, None, *[C.byref(x) for x in c]) == 0
        assert np.array_equal(sk, ref["skel"]) and [x.value for x in c] == [ref[n] for n in COUNTS]
    one_, two = ctx.keep_skeleton(5, skel=True), ctx.keep_skeleton(5, skel=True)           # the same bits
    assert all(np.array_equal(one_[n], two[n]) for n in ("table", "nodes", "skel")) and all(one_[n] == two[n] for n in COUNTS)
    same(ctx.skeleton_raster(lab, maxfeat=2, maxnode=1), ref, "binding, truncated", maxfeat=2, maxnode=1)
    ms = ctx.skeleton_kernel_ms()
    assert len(ms) == 3 and all(x >= 0. for x in ms) and ms[0] > 0.
    r = sit.SkeletonRaster(lab, ctx=ctx)                               # the host entry points: a label map, and a mask labelled first
    same(r, ref, "SkeletonRaster(labels)")
    mask = lab >= 0
    for m in (mask, mask.astype(np.int8)):
        r = sit.SkeletonRaster(m, conn=4, ctx=ctx)
        assert np.array_equal(r["labels"], lab)
        same(r, ref, "SkeletonRaster(mask)")
    r8 = sit.SkeletonRaster(mask, conn=8, ctx=ctx)                      # other labels, the same skeleton
    assert np.array_equal(r8["skel"], ref["skel"]) and np.array_equal(r8["labels"], label_ref(mask, 8)) and r8["nfeat"] < nf
    ctx.keep_free(5)


def test_errors_come_before_any_device_work(ctx):
    ny, nx = 5, 9
    lab = np.zeros((ny, nx), dtype=np.int32)
    lib, h, p = ctx._L, ctx._h, _lib._ptr
    ctx.keep_put(6, lab)
    tab, nod = np.full((4, 7), 77, dtype=np.int64), np.full((4, 3), 77, dtype=np.int64)
    n = _lib._i64(7)

    def raster(ny=ny, nx=nx, map=lab, max_sub=8, maxfeat=4, maxnode=4, table=tab, nodes=nod):
        return lib.sitrk_skeleton_raster(h, ny, nx, p(map), max_sub, maxfeat, maxnode, None, p(table), p(nodes), C.byref(n), None, None, None, None)

    def keep(slot=6, max_sub=8, maxfeat=4, maxnode=4, table=tab, nodes=nod):
        return lib.sitrk_keep_skeleton(h, slot, max_sub, maxfeat, maxnode, None, p(table), p(nodes), C.byref(n), None, None, None, None)

    for call in (raster, keep):
        for kw, msg in (({"max_sub": 0}, b"max_sub must be in 1..1048576"), ({"max_sub": (1 << 20) + 1}, b"max_sub"), ({"maxfeat": -1}, b"maxfeat"),
                        ({"maxnode": -1}, b"maxnode"), ({"table": None}, b"null table"), ({"nodes": None}, b"null nodes")):
            assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
    for kw, msg in (({"ny": 0}, b"ny and nx must be in 1..32768"), ({"nx": 32769}, b"1..32768"), ({"ny": 32768, "nx": 32768}, b"2^28"),
                    ({"map": None}, b"null map")):
        assert raster(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
    for kw, msg in (({"slot": 16}, b"keep must be in 0..15"), ({"slot": -1}, b"keep must be in"), ({"slot": 7}, b"kept map 7 is empty")):
        assert keep(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
    assert (tab == 77).all() and (nod == 77).all() and n.value == 7
    assert raster(max_sub=1 << 20) == 0 and n.value == 1
    for v, at in ((ny * nx, (0, 0)), (-2, (4, 8))):                    # a value out of range: counted, SITRK_EINDEX
        bad = lab.copy()
        bad[at] = v
        assert raster(map=bad) == -2 and b"1 value(s) of the map lie outside [-1, 45)" in lib.sitrk_last_error(h)
        with pytest.raises(IndexError, match=r"1 value\(s\)"):
            ctx.skeleton_raster(bad)
    with pytest.raises(_lib.SitrkError, match="skeleton_batch must be 1..%d" % CONST["kSkHalo"]):
        ctx.set_tuning(skeleton_batch=CONST["kSkHalo"] + 1)
    fresh = sit.Context(0)
    try:
        with pytest.raises(_lib.SitrkError, match="no skeleton call"):
            fresh.skeleton_kernel_ms()
        with pytest.raises(_lib.SitrkError, match="kept map 0 is empty"):
            fresh.keep_skeleton(0)
    finally:
        fresh.close()
    ctx.keep_free(6)


# ------------------------------------------------------------------------------------------------ where the batching can go wrong
def plus_across_a_corner():
    m = np.zeros((130, 135), dtype=np.int8)
    p33 = plus(33)                                                     # 113 x 113, its centre at (56, 56): at (64, 64) of the raster
    m[8:8 + p33.shape[0], 8:8 + p33.shape[1]] = p33
    assert m[TILE - 1:TILE + 1, TILE - 1:TILE + 1].all()
    return one(m)


BATCH_MAPS = {"block 65x130": lambda: one(np.ones((65, 130), dtype=np.int8)), "block 130x130": lambda: one(np.ones((130, 130), dtype=np.int8)),
              "plus 33 across a tile corner": plus_across_a_corner}
CUTS = sorted({1, 2, 3, B - 1, B, B + 1, 2 * B + 1, 4096} - {0})


@pytest.mark.parametrize("name", list(BATCH_MAPS))
def test_every_cut_of_a_long_thinning_equals_the_restatement(ctx, name):
    full = skeleton_ref(name, BATCH_MAPS[name])
    assert full["nsub"] > 2 * B + 1 and full["converged"] == 1 and TILE == 64
    lab = full["labels"]
    ctx.keep_put(1, lab)
    for cut in CUTS:
        ref = skeleton_ref(name, BATCH_MAPS[name], cut)
        if cut < 4096:
            assert ref["nsub"] == cut and ref["converged"] == 0          # the run ends inside a batch, or at its end, still thinning
        same(ctx.skeleton_raster(lab, max_sub=cut), ref, (name, cut, "raster"))
        same(ctx.keep_skeleton(1, max_sub=cut, skel=True), ref, (name, cut, "keep"))
    # the last sub-iterations that say so: nsub + 1 has not seen one quiet sub-iteration of each kind, nsub + 2 has
    for cut, conv in ((full["nsub"], 0), (full["nsub"] + 1, 0), (full["nsub"] + 2, 1)):
        got = ctx.keep_skeleton(1, max_sub=cut, skel=True)
        assert (got["nsub"], got["converged"]) == (full["nsub"], conv) and np.array_equal(got["skel"], full["skel"]), (name, cut)
    ctx.keep_free(1)


def test_the_batch_length_never_changes_a_result(ctx):
    name = "plus 33 across a tile corner"
    lab = skeleton_ref(name, BATCH_MAPS[name])["labels"]
    try:
        for batch in range(1, CONST["kSkHalo"] + 1):
            ctx.set_tuning(skeleton_batch=batch)
            for cut in (2 * B + 1, 4096):
                same(ctx.skeleton_raster(lab, max_sub=cut), skeleton_ref(name, BATCH_MAPS[name], cut), (name, batch, cut))
    finally:
        ctx.set_tuning(skeleton_batch=B)


def test_empty_map_and_the_smallest_max_sub(ctx):
    empty = np.full((5, 7), -1, dtype=np.int32)
    for cut, conv in ((1, 0), (2, 1), (4096, 1)):
        got = ctx.skeleton_raster(empty, max_sub=cut)
        assert (got["nsub"], got["converged"], got["nskel"], got["nfeat"], got["nnode"]) == (0, conv, 0, 0, 0)
        assert not got["skel"].any() and got["table"].shape == (0, 7) and got["nodes"].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ a second trip of every strided kernel
def test_a_raster_of_two_trips(ctx):
    ny, nx = TRIP2
    npix = ny * nx
    up = lambda a, b: -(-a // b)
    blocks = max(1, min(up(npix, CONST["kSkThreads"]), CONST["kSkBlocks"]))
    assert up(npix, blocks * CONST["kSkThreads"]) == 2                 # skel_init_kernel, skel_class_kernel
    pieces = up(npix, 64)
    wtrips = max(up(pieces, CONST["kSkSpanWaves"]), CONST["kSkMinTrips"])
    assert wtrips >= 2 and up(pieces, wtrips) > 1000                   # skel_count_kernel, skel_table_kernel
    mk = lambda: labels_of(random_mask(ny, nx, 0.6, 7), 8)
    ref = skeleton_ref(("trip2", ny, nx), mk)
    assert ref["converged"] == 1 and ref["nfeat"] > 100 and ref["nnode"] > 10000 and ref["nsub"] > B
    same(ctx.skeleton_raster(ref["labels"]), ref, "TRIP2 raster")
    ctx.keep_put(0, ref["labels"])
    same(ctx.keep_skeleton(0), ref, "TRIP2 keep", skel=False)
    ctx.keep_free(0)
    first = blocks * CONST["kSkThreads"]                               # bad values at the ends of both trips are all counted
    bad = ref["labels"].copy().reshape(-1)
    bad[[0, first - 1, first, npix - 1]] = (npix, -2, npix + 7, -2 ** 31)
    with pytest.raises(IndexError, match=r"4 value\(s\) of the map lie outside \[-1, %d\)" % npix):
        ctx.skeleton_raster(bad.reshape(ny, nx))


# ------------------------------------------------------------------------------------------------ the mesh path
def test_keep_skeleton_of_a_mesh_follows_its_feature_table():
    trk = start()
    try:
        s0 = trk.ctx.fetch()
        assert trk.mesh(3.5, JREC0)["nQ"] > 256
        jrec1 = advance(trk, JREC0, 3, 3)
        lo, hi = s0["yx"].min(axis=0), s0["yx"].max(axis=0)
        grid = sit.raster_grid(lo[0] + 9., hi[0] + 3., lo[1] - 2., hi[1] - 11., 0.9)
        rates = trk.mesh_deform(jrec1)
        owner = trk.mesh_raster(jrec1, grid, fields=False)["owner"]
        own = owner[owner >= 0]
        thr = float(np.sqrt(np.median(rates["div"][own] ** 2 + rates["shr"][own] ** 2)))
        for min_pix in (1, 5):
            f = trk.mesh_features(jrec1, grid, what="tot", thr=thr, conn=4, min_pix=min_pix, labels=True, keep=3)
            assert f["nfeat"] > 3
            kept = kept_ref(f["labels"], min_pix)
            K, nsub, conv = thin_ref(kept, 4096)
            ref = {"skel": K, "nsub": nsub, "converged": conv, "nskel": int(K.sum()), "table": skeleton_table_ref(kept, K),
                   "nodes": nodes_ref(kept, K)}
            ref["nfeat"], ref["nnode"] = len(ref["table"]), len(ref["nodes"])
            got = trk.features_skeleton(3, skel=True)
            same(got, ref, ("mesh", min_pix))
            assert np.array_equal(got["table"][:, :2], f["table"][:, :2]) and got["nfeat"] == f["nfeat"]
            assert np.array_equal(trk.ctx.keep_get(3)["labels"], kept)
            s = sit.skeleton_table(got["table"], grid)
            assert s["length_km"].max() > 0. and np.array_equal(s["npix"], f["table"][:, 1])
            assert sit.node_yx(got["nodes"], grid).shape == (got["nnode"], 2)
        with pytest.raises(ValueError, match="max_sub"):
            trk.features_skeleton(3, max_sub=0)
        with pytest.raises(ValueError, match="keep"):
            trk.features_skeleton(16)
    finally:
        trk.ctx.close()


# ------------------------------------------------------------------------------------------------ command line
def test_cli_deform_skeleton_flag(tmp_path, monkeypatch, capsys, ctx):
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F", "--deform", "30", "--deform-window", "5", "--deform-grid", "10"]
    plain = drv.main(argv)
    with np.load(plain["files"][2]) as z:
        own, tot2 = z["m0_w0_owner"], z["m0_w0_div"] ** 2 + z["m0_w0_shr"] ** 2
    thr = float(np.sqrt(np.median(tot2[own[own >= 0]])))
    feat = argv + ["--deform-features", "tot@%r@2" % thr]
    capsys.readouterr()
    with np.load(drv.main(feat)["files"][2]) as z:                     # without the flag: the file every run wrote before
        e = {k: z[k] for k in z.files}
    assert "--deform-skeleton" not in capsys.readouterr().out and not any("skeleton" in k for k in e)
    with np.load(drv.main(feat + ["--deform-skeleton"])["files"][2]) as z:
        d = {k: z[k] for k in z.files}
    log = capsys.readouterr().out
    with np.load(drv.main(feat + ["--deform-skeleton", "3", "--deform-track"])["files"][2]) as z:
        t = {k: z[k] for k in z.files}
    log3 = capsys.readouterr().out
    new = ["skeleton"] + ["m0_w%d_%s" % (w, s) for w in range(3) for s in ("skeleton", "skeleton_nodes", "skeleton_counts")]
    assert sorted(d) == sorted(list(e) + new) and all(np.array_equal(d[k], e[k], equal_nan=(e[k].dtype.kind == "f")) for k in e)
    assert d["skeleton"].tolist() == [4096] and t["skeleton"].tolist() == [3] and "m0_w1_pairs" in t
    for w in range(3):
        pre = "m0_w%d_" % w
        o = d[pre + "owner"]
        at = np.maximum(o, 0)
        with np.errstate(invalid="ignore"):
            mask = (o >= 0) & (d[pre + "div"][at] * d[pre + "div"][at] + d[pre + "shr"][at] * d[pre + "shr"][at] >= thr * thr)
        lab = ft.kept_labels(sit.LabelRaster(mask, conn=8, min_pix=2, ctx=ctx)["labels"], 2)
        for run, max_sub in ((d, 4096), (t, 3)):
            py = ctx.skeleton_raster(lab, max_sub=max_sub, skel=False)      # the Python call on the same map, and the restatement
            K, nsub, conv = thin_ref(lab, max_sub)
            assert np.array_equal(run[pre + "skeleton"], py["table"]) and np.array_equal(py["table"], skeleton_table_ref(lab, K))
            assert np.array_equal(run[pre + "skeleton_nodes"], py["nodes"]) and np.array_equal(py["nodes"], nodes_ref(lab, K))
            assert run[pre + "skeleton_counts"].tolist() == [py[n] for n in COUNTS] == [len(py["table"]), len(py["nodes"]), int(K.sum()), nsub, conv]
            assert run[pre + "skeleton"].dtype == np.int64 and run[pre + "skeleton_nodes"].dtype == np.int64
            assert np.array_equal(run[pre + "skeleton"][:, :2], run[pre + "features"][:, :2]) and len(py["table"]) > 0
        line = [ln for ln in log.splitlines() if "--deform-skeleton window %d mesh 0" % w in ln and "WARNING" not in ln]
        assert len(line) == 1 and "longest" in line[0] and "sub-iterations" in line[0], line
    assert "WARNING --deform-skeleton" not in log
    assert ("WARNING --deform-skeleton" in log3) == any(t["m0_w%d_skeleton_counts" % w][4] == 0 for w in range(3))
    with pytest.raises(_lib.SitrkError, match="is empty"):              # without --deform-track the driver's slot is free again
        ctx.keep_get(_lib.KEEP_MAX - 1)
    # the tool on the series file: its own map through sitrk_skeleton_raster
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    fc, fout = str(tmp_path / "cells.npy"), str(tmp_path / "skel.npz")
    np.save(fc, d["m0_w0_cells"])
    assert tool.main(["-i", plain["files"][0], "-c", fc, "-k", "0", "-K", "5", "--grid", "6", "--features", "tot@%r@2" % thr, "--skeleton", "-o", fout]) == 0
    assert "--skeleton 4096:" in capsys.readouterr().out
    with np.load(fout) as z:
        m = {k: z[k] for k in z.files}
    assert m["skeleton_arg"].tolist() == [4096] and m["skeleton"].shape == (len(m["features"]), 7) and m["skeleton_counts"][4] == 1
    assert np.array_equal(m["skeleton"][:, :2], m["features"][:, :2]) and m["skeleton_nodes"].shape == (m["skeleton_counts"][1], 3)
