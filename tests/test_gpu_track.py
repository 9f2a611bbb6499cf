"""Features from window to window on the GPU (sitrk_mesh_features_keep / sitrk_keep_* / sitrk_mesh_features_advect /
sitrk_features_match) against the restatements of tests/test_track.py.  All integer: every comparison is
array_equal, there is no tolerance anywhere.  The rasters are those of tests/test_gpu_features.py -- one pixel, one row, around a
tile, partial tiles, many tiles long --, the maps the labels of its masks, and the mesh that of tests/test_gpu_mesh.py.  Every
kernel launched through `Strided` takes one trip on those; the tests on TRIP2 and SPAN5 (tests/test_features.py) give it two and
five, and sort keys of 40 and 44 bits."""
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
from test_features import (SPAN5, TRIP2, checkerboard, comb, kernel_constants, label_ref, launch_shape, random_mask, same_result,
                           serpentine, table_ref)
from test_gpu_features import want_labels
from test_gpu_mesh import JREC0, K, advance, start
from test_track import advect_ref, kept_ref, match_ref, permuted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = getattr(_lib, "LABEL_TILE", 64)
SHAPES = [(1, 1), (1, 300), (T - 1, T + 1), (67, 131), (200, 333), (3, 8 * T + 5)]
REACHES = (0, 1, 2)


@pytest.fixture(scope="module")
def ctx():
    c = sit.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def maps(ny, nx):
    """the pairs (name, A, B) of one raster; B is None for a self-match"""
    lo, hi = label_ref(random_mask(ny, nx, 0.41, 1), 8), label_ref(random_mask(ny, nx, 0.59, 2), 4)
    none = np.full((ny, nx), -1, dtype=np.int32)
    out = [("random 0.41/8 against 0.59/4", lo, hi), ("random 0.59/4 against 0.41/8", hi, lo),
           ("all against checkerboard", label_ref(np.ones((ny, nx), dtype=np.int8), 4), label_ref(checkerboard(ny, nx), 4)),
           ("serpentine against comb", label_ref(serpentine(ny, nx), 4), label_ref(comb(ny, nx), 8)),
           ("empty against random", none, hi), ("random against empty", lo, none),
           ("not canonical", permuted(lo, 11), permuted(hi, 12)), ("self", hi, None)]
    for _, a, b in out:
        a.setflags(write=False)
        if b is not None:
            b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_match(ny, nx, k, reach, dj, di):
    _, a, b = maps(ny, nx)[k]
    return match_ref(a, a if b is None else b, reach, dj, di)


# ------------------------------------------------------------------------------------------------ match
@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_match_equals_the_restatement(ctx, ny, nx, reach):
    for k, (name, a, b) in enumerate(maps(ny, nx)):
        ctx.keep_put(0, a)
        if b is not None:
            ctx.keep_put(1, b)
        sa, sb = 0, (0 if b is None else 1)
        for dj, di in ((0, 0), (1, -2), (-ny, 0)):
            what = (name, ny, nx, reach, dj, di)
            pairs, nhit = want_match(ny, nx, k, reach, dj, di)
            got = ctx.features_match(sa, sb, reach=reach, dj=dj, di=di)
            assert got["pairs"].dtype == np.int64 and got["pairs"].shape == pairs.shape and np.array_equal(got["pairs"], pairs), what
            assert (got["npair"], got["nhit"]) == (len(pairs), nhit), what
            if (dj, di) == (-ny, 0) and reach == 0:                    # everything outside the raster (with a reach the last rows
                assert got["npair"] == 0 and got["nhit"] == 0, what    # of A still see the first rows of B: the restatement says so)
        if name == "all against checkerboard" and ny * nx > 1:         # one feature of A into many of B
            pairs, _ = want_match(ny, nx, k, reach, 0, 0)
            assert (pairs[:, 0] == 0).all() and len(pairs) == (ny * nx + 1) // 2
        if name == "self" and reach == 0:
            tab, _, nact = table_ref(a)
            pairs, nhit = want_match(ny, nx, k, 0, 0, 0)
            assert np.array_equal(pairs, np.stack([tab[:, 0], tab[:, 0], tab[:, 1]], axis=1)) and nhit == nact
    if (ny, nx) == (200, 333):                                         # the random maps meet in many pairs over many workgroups
        assert len(want_match(ny, nx, 0, reach, 0, 0)[0]) > 1000


def test_match_forms_of_the_call(ctx):
    ny, nx = 67, 131
    _, a, b = maps(ny, nx)[0]
    ctx.keep_put(4, a, conn=8, min_pix=1)
    ctx.keep_put(9, b, conn=4, min_pix=3)
    lib, h, p = ctx._L, ctx._h, _lib._ptr
    for reach in REACHES:
        pairs, nhit = match_ref(a, b, reach, 1, -2)
        assert len(pairs) > 40
        np_, nh = _lib._i64(-5), _lib._i64(-5)
        assert lib.sitrk_features_match(h, 4, 9, 1, -2, reach, 0, None, C.byref(np_), C.byref(nh)) == 0     # maxpair 0, pairs NULL
        assert (np_.value, nh.value) == (len(pairs), nhit)
        assert lib.sitrk_features_match(h, 4, 9, 1, -2, reach, 0, None, None, None) == 0                       # every output is optional
        buf = np.full((len(pairs) + 3, 3), 77, dtype=np.int64)
        cut = len(pairs) // 3
        assert lib.sitrk_features_match(h, 4, 9, 1, -2, reach, cut, p(buf), C.byref(np_), C.byref(nh)) == 0 # truncated: the first rows only
        assert np.array_equal(buf[:cut], pairs[:cut]) and (buf[cut:] == 77).all() and (np_.value, nh.value) == (len(pairs), nhit)
        assert lib.sitrk_features_match(h, 4, 9, 1, -2, reach, len(buf), p(buf), C.byref(np_), None) == 0
        assert np.array_equal(buf[:len(pairs)], pairs) and (buf[len(pairs):] == 77).all()
        one, two = ctx.features_match(4, 9, reach=reach, dj=1, di=-2), ctx.features_match(4, 9, reach=reach, dj=1, di=-2)
        assert np.array_equal(one["pairs"], two["pairs"]) and (one["npair"], one["nhit"]) == (two["npair"], two["nhit"])   # the same bits
    fwd, back = ctx.features_match(4, 9, dj=1, di=-2), ctx.features_match(9, 4, dj=-1, di=2)                  # swapped at reach 0
    sw = back["pairs"][np.lexsort((back["pairs"][:, 0], back["pairs"][:, 1]))]
    assert np.array_equal(sw[:, [1, 0, 2]], fwd["pairs"]) and fwd["nhit"] == back["nhit"]
    ms = ctx.match_kernel_ms()
    assert len(ms) == 3 and all(x >= 0. for x in ms) and ms[0] > 0.
    # refusals, before any device work: the slots are what they were
    ctx.keep_put(5, np.zeros((4, 5), dtype=np.int32))
    buf = np.full((4, 3), 77, dtype=np.int64)
    n = _lib._i64(7)

    def call(ka=4, kb=9, dj=0, di=0, reach=0, maxpair=4, out=buf):
        return lib.sitrk_features_match(h, ka, kb, dj, di, reach, maxpair, p(out), C.byref(n), None)

    for kw, msg in (({"ka": 16}, b"keepA must be in 0..15"), ({"kb": -1}, b"keepB must be in"), ({"ka": 6}, b"kept map 6 is empty"),
                    ({"kb": 5}, b"kept map 5 is 4 x 5"), ({"reach": 3}, b"reach must be in 0..2"), ({"reach": -1}, b"reach"),
                    ({"dj": 32769}, b"shift"), ({"di": -32769}, b"shift"), ({"maxpair": -1}, b"maxpair"), ({"out": None}, b"null pairs")):
        assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
    assert (buf == 77).all() and n.value == 7
    assert call(dj=32768, di=-32768) == 0 and n.value == 0
    fresh = sit.Context(0)
    try:
        with pytest.raises(_lib.SitrkError, match="no sitrk_features_match"):
            fresh.match_kernel_ms()
        with pytest.raises(_lib.SitrkError, match="kept map 0 is empty"):
            fresh.keep_get(0)
    finally:
        fresh.close()
    r = sit.MatchLabels(a, b, reach=1, dj=1, di=-2, ctx=ctx)          # the host-map entry point: its two slots are free again
    pairs, nhit = match_ref(a, b, 1, 1, -2)
    assert np.array_equal(r["pairs"], pairs) and (r["npair"], r["nhit"]) == (len(pairs), nhit)
    for slot in (_lib.KEEP_MAX - 2, _lib.KEEP_MAX - 1):
        with pytest.raises(_lib.SitrkError, match="is empty"):
            ctx.keep_get(slot)
    for slot in (4, 5, 9):
        ctx.keep_free(slot)


# ------------------------------------------------------------------------------------------------ match, on large rasters
# TRIP2 and SPAN5 of tests/test_features.py: more than one trip of every kernel that `Strided` launches, and keys of 40 and 44
# bits where the rasters above stop at 34.  The maps are the labels of the random masks of tests/test_gpu_features.py (from its
# cache: each is restated once for both files) and copies under other names, whose values use all of [0, npix) and so every bit
# of the nb that the keys are packed and unpacked with.
@functools.lru_cache(maxsize=None)
def large_maps(ny, nx):
    lo, hi = want_labels((0.41, 1), ny, nx, 8), want_labels((0.59, 1), ny, nx, 4)
    out = [("random 0.41/8 against 0.59/4", lo, hi), ("not canonical", permuted(lo, 11), permuted(hi, 12))]
    for _, a, b in out:
        a.setflags(write=False)
        b.setflags(write=False)
    assert max(int(m.max()).bit_length() for m in out[1][1:]) == (ny * nx - 1).bit_length()           # the top bit is used
    return out


@functools.lru_cache(maxsize=None)
def want_large_match(ny, nx, k, reach, dj, di):
    _, a, b = large_maps(ny, nx)[k]
    return match_ref(a, b, reach, dj, di)


def check_match(ctx, ny, nx, k, reach, dj, di):
    """slots 0 and 1 hold the maps k of the raster: one call against the restatement; returns its pairs"""
    pairs, nhit = want_large_match(ny, nx, k, reach, dj, di)
    got = ctx.features_match(0, 1, reach=reach, dj=dj, di=di)
    what = (ny, nx, k, reach, dj, di, got["npair"], len(pairs), got["nhit"], nhit)
    assert got["pairs"].dtype == np.int64 and got["pairs"].shape == pairs.shape and np.array_equal(got["pairs"], pairs), what
    assert (got["npair"], got["nhit"]) == (len(pairs), nhit), what
    return pairs


@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("k", [0, 1])
def test_match_on_a_raster_of_two_trips(ctx, k, reach):
    ny, nx = TRIP2
    _, a, b = large_maps(ny, nx)[k]
    ctx.keep_put(0, a)
    ctx.keep_put(1, b)
    for dj, di in ((0, 0), (1, -2), (-ny, 0)):
        pairs = check_match(ctx, ny, nx, k, reach, dj, di)
        if dj == -ny:                                                  # outside the raster, but for the last rows of A within the reach
            assert (len(pairs) == 0) == (reach == 0), (k, reach, len(pairs))
        else:
            assert len(pairs) > 10000, (k, reach, dj, di, len(pairs))
    ctx.keep_free(0)
    ctx.keep_free(1)


@pytest.mark.parametrize("reach", [0, 2])
@pytest.mark.parametrize("k", [0, 1])
def test_match_on_a_raster_of_five_trips(ctx, k, reach):
    ny, nx = SPAN5
    _, a, b = large_maps(ny, nx)[k]
    ctx.keep_put(0, a)
    ctx.keep_put(1, b)
    pairs = check_match(ctx, ny, nx, k, reach, 1, -2)
    assert len(pairs) > 50000 and pairs[:, 2].sum() > 500000, (k, reach, len(pairs))      # tens of thousands of rows from 10^5..10^6 keys
    if k == 1:
        assert int(pairs[:, :2].max()).bit_length() == (ny * nx - 1).bit_length()
    if reach == 2:                                                     # truncated: the first rows only, the rest of the buffer untouched
        lib, h, p = ctx._L, ctx._h, _lib._ptr
        nhit = want_large_match(ny, nx, k, reach, 1, -2)[1]
        cut = len(pairs) // 3
        buf = np.full((cut + 3, 3), 77, dtype=np.int64)
        np_, nh = _lib._i64(-5), _lib._i64(-5)
        assert lib.sitrk_features_match(h, 0, 1, 1, -2, reach, cut, p(buf), C.byref(np_), C.byref(nh)) == 0
        assert np.array_equal(buf[:cut], pairs[:cut]) and (buf[cut:] == 77).all() and (np_.value, nh.value) == (len(pairs), nhit)
    ctx.keep_free(0)
    ctx.keep_free(1)


def test_keep_put_counts_the_bad_values_of_every_trip(ctx):
    """keep_range_kernel carries a wave's count from trip to trip: values outside [-1, npix) at the first and the last pixel of each
    of the two trips of TRIP2 are all counted, and the slot stays what it was"""
    ny, nx = TRIP2
    npix = ny * nx
    good = large_maps(ny, nx)[1][1]
    ctx.keep_put(2, good, conn=4, min_pix=3)
    c = kernel_constants()
    first = c["kTrThreads"] * c["kTrBlocks"]                           # the first pixel of the second trip
    assert first < npix - 1 < 2 * first
    for where, values in (((0, first - 1, first, npix - 1), (npix, -2, npix + 7, -2 ** 31)), ((first,), (npix,)), ((npix - 1,), (2 ** 31 - 1,))):
        bad = good.copy().reshape(-1)
        bad[list(where)] = values
        with pytest.raises(IndexError, match=r"%d value\(s\) of the map lie outside \[-1, %d\)" % (len(where), npix)):
            ctx.keep_put(2, bad.reshape(ny, nx))
    edge = good.copy().reshape(-1)                                     # the largest and the smallest value that pass, at the same pixels
    edge[[0, first - 1, first, npix - 1]] = (npix - 1, -1, npix - 1, -1)
    ctx.keep_put(3, edge.reshape(ny, nx))
    assert np.array_equal(ctx.keep_get(3)["labels"].reshape(-1), edge)
    k = ctx.keep_get(2)
    assert (k["shape"], k["conn"], k["min_pix"]) == ((ny, nx), 4, 3) and np.array_equal(k["labels"], good)
    ctx.keep_free(2)
    ctx.keep_free(3)


def test_self_match_on_a_raster_of_five_trips(ctx):
    ny, nx = SPAN5
    for k, (_, _, b) in enumerate(large_maps(ny, nx)):                 # the labels at conn 4, and the same partition under other names
        ctx.keep_put(0, b)
        tab, _, nact = table_ref(b)
        got = ctx.features_match(0, 0)
        assert len(tab) > 50000 and got["npair"] == len(tab) and got["nhit"] == nact, k
        assert np.array_equal(got["pairs"], np.stack([tab[:, 0], tab[:, 0], tab[:, 1]], axis=1)), k
    ctx.keep_free(0)


# ------------------------------------------------------------------------------------------------ keep
def refined(grid, more_than):
    """the grid over the extent of `grid` with pixels small enough for more than `more_than` of them, both sides odd"""
    y0, x0, d, ny, nx = grid
    f = 1.01 * float(np.sqrt(more_than / (ny * nx)))
    fine = (y0, x0, d / f, int(np.ceil(ny * f)) | 1, int(np.ceil(nx * f)) | 1)
    assert fine[3] * fine[4] > more_than and fine[3] % 2 == 1 and fine[4] % 2 == 1 and fine[3] != fine[4]
    return fine


def mesh_case():
    """the tracker of the mesh tests with a mesh of more than 256 cells advanced six records, a grid finer than its cells that
    it reaches beyond on two sides, and the threshold that half of the owned pixels pass, from the device's own rates"""
    trk = start()
    s0 = trk.ctx.fetch()
    assert trk.mesh(3.5, JREC0)["nQ"] > 256
    jrec1 = advance(trk, JREC0, 3, 3)
    lo, hi = s0["yx"].min(axis=0), s0["yx"].max(axis=0)
    grid = sit.raster_grid(lo[0] + 9., hi[0] + 3., lo[1] - 2., hi[1] - 11., 0.9)
    return trk, jrec1, grid, half_threshold(trk, jrec1, grid)


def half_threshold(trk, jrec1, grid, slot=0):
    rates = trk.mesh_deform(jrec1, slot=slot)
    owner = trk.mesh_raster(jrec1, grid, slot=slot, fields=False)["owner"]
    own = owner[owner >= 0]
    return float(np.sqrt(np.median(rates["div"][own] ** 2 + rates["shr"][own] ** 2)))


def test_keep_is_mesh_features_plus_the_kept_map():
    trk, jrec1, grid, thr = mesh_case()
    try:
        ctx = trk.ctx
        assert grid[3] > T and grid[4] > T
        for min_pix, maxfeat in ((1, 65536), (5, 65536), (5, 2), (1, 0)):
            kw = dict(what="tot", thr=thr, conn=4, min_pix=min_pix, maxfeat=maxfeat, labels=True)
            want = trk.mesh_features(jrec1, grid, **kw)
            got = trk.mesh_features(jrec1, grid, keep=3, **kw)
            assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["table"], want["table"]), (min_pix, maxfeat)
            assert all(got[n] == want[n] for n in ("nfeat", "ncomp", "nactive")) and want["ncomp"] >= want["nfeat"] > 3
            assert len(want["table"]) == min(maxfeat, want["nfeat"])
            k = ctx.keep_get(3)
            assert (k["shape"], k["conn"], k["min_pix"]) == ((grid[3], grid[4]), 4, min_pix) and k["labels"].dtype == np.int32
            assert np.array_equal(k["labels"], kept_ref(want["labels"], min_pix)), (min_pix, maxfeat)     # a truncated table: the same map
        # a min_pix that drops half of the components, from the table itself; and the call without the labels
        whole = trk.mesh_features(jrec1, grid, what="tot", thr=thr, conn=4, labels=True)
        cut = int(np.sort(whole["table"][:, 1])[len(whole["table"]) // 2]) + 1
        assert 1 < cut <= whole["table"][:, 1].max()
        bare = trk.mesh_features(jrec1, grid, what="tot", thr=thr, conn=4, min_pix=cut, keep=3)
        kept5 = ctx.keep_get(3)["labels"]
        assert bare["labels"] is None and 0 < bare["nfeat"] < whole["nfeat"] and ctx.keep_get(3, labels=False)["labels"] is None
        assert np.array_equal(kept5, kept_ref(whole["labels"], cut)) and ctx.keep_get(3, labels=False)["min_pix"] == cut
        assert 0 < (kept5 >= 0).sum() < (whole["labels"] >= 0).sum()

        # a call that fails leaves the slot as it was
        lib, h = ctx._L, ctx._h
        with pytest.raises(_lib.SitrkError, match="before the mesh's t0"):
            trk.mesh_features(JREC0 - 1, grid, thr=thr, keep=3)
        with pytest.raises(_lib.SitrkError, match="mesh 1 is empty"):
            trk.mesh_features(jrec1, grid, thr=thr, keep=3, slot=1)
        with pytest.raises(_lib.SitrkError, match="keep must be in 0..15"):
            ctx.mesh_features_keep(16, 0, jrec1, grid, 3, thr)
        with pytest.raises(_lib.SitrkError, match="1..32768"):
            ctx.mesh_features_keep(3, 0, jrec1, (0., 0., 1., 1, 32769), 3, thr)
        bad = np.zeros((3, 4), dtype=np.int32)
        for v in (12, -2):
            bad[1, 2] = v
            with pytest.raises(IndexError, match=r"1 value\(s\) of the map lie outside \[-1, 12\)"):
                ctx.keep_put(3, bad)
        for kw, msg in (({"conn": 5}, "conn must be 4"), ({"min_pix": 0}, "min_pix")):
            with pytest.raises(_lib.SitrkError, match=msg):
                ctx.keep_put(3, np.zeros((3, 4), dtype=np.int32), **kw)
        assert lib.sitrk_keep_put(h, 3, 3, 4, None, 8, 1) == -1 and b"null map" in lib.sitrk_last_error(h)
        with pytest.raises(_lib.SitrkError, match="kept map 3 is %d x %d" % (grid[3], grid[4])):
            trk.features_advect(jrec1, tuple(grid[:4]) + (grid[4] + 1,), 3, 3)
        k = ctx.keep_get(3)
        assert (k["shape"], k["conn"], k["min_pix"]) == ((grid[3], grid[4]), 4, cut) and np.array_equal(k["labels"], kept5)

        # a round trip, with values that no labelling gives
        rng = np.random.default_rng(9)
        odd = rng.integers(-1, 7 * 9, (7, 9)).astype(np.int32)
        ctx.keep_put(12, odd, conn=8, min_pix=2)
        back = ctx.keep_get(12)
        assert np.array_equal(back["labels"], odd) and (back["shape"], back["conn"], back["min_pix"]) == ((7, 9), 8, 2)

        # the kept maps survive stepping, a re-sort, a rebuilt mesh, the transient scratch of other calls, and new buoys
        state = ctx.fetch()
        nxt = advance(trk, jrec1 + 1, 1, 1)
        assert trk.mesh(3.5, nxt + 1)["nQ"] > 256
        ctx.run((nxt + 1) % K, nxt + 1, 1)
        trk.mesh_coarse(nxt + 1, (grid[0], grid[1], 4., 20, 20), 3)
        assert sit.LabelRaster(checkerboard(300, 300), ctx=ctx)["ncomp"] == 1
        assert sit.MatchLabels(odd, odd, ctx=ctx)["nhit"] == (odd >= 0).sum()
        alive = state["alive"] != 0
        trk.set_buoys(state["yx"][alive][:50], state["jiT"][alive][:50])
        assert np.array_equal(ctx.keep_get(3)["labels"], kept5) and np.array_equal(ctx.keep_get(12)["labels"], odd)

        ctx.keep_free(3)
        ctx.keep_free(3)                                               # an empty slot may be freed
        with pytest.raises(_lib.SitrkError, match="kept map 3 is empty"):
            ctx.keep_get(3)
        with pytest.raises(_lib.SitrkError, match="keep must be in 0..15"):
            ctx.keep_free(16)
        assert np.array_equal(ctx.keep_get(12)["labels"], odd)
    finally:
        trk.close()


def test_keep_on_a_raster_of_long_spans():
    """the mesh path on more than 2^21 pixels: label_mask_kernel, the label pipeline with spans of five pieces on real rates, and
    keep_labels_kernel"""
    trk, jrec1, coarse, thr = mesh_case()
    try:
        ctx = trk.ctx
        grid = refined(coarse, SPAN5[0] * SPAN5[1])
        c = kernel_constants()
        shape = launch_shape(grid[3], grid[4], c)
        assert shape["wtrips"] > c["kLbMinTrips"] and shape["flag"][0] > 2 and shape["npix"] % 64 != 0, shape
        kw = dict(what="tot", thr=thr, conn=4, labels=True)
        want = trk.mesh_features(jrec1, grid, **kw)
        got = trk.mesh_features(jrec1, grid, keep=3, **kw)
        assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["table"], want["table"])
        assert all(got[n] == want[n] for n in ("nfeat", "ncomp", "nactive")) and want["ncomp"] == want["nfeat"] > 3
        owner = trk.mesh_raster(jrec1, grid, fields=False)["owner"]
        assert 0.3 < want["nactive"] / (owner >= 0).sum() < 0.7         # about half of the owned pixels pass
        same_result(want, label_ref(want["labels"] >= 0, 4), what="the labels of the device's own mask")
        k = ctx.keep_get(3)
        assert (k["shape"], k["conn"], k["min_pix"]) == ((grid[3], grid[4]), 4, 1) and np.array_equal(k["labels"], want["labels"])
        # a min_pix that drops half of the components, from the table itself
        cut = int(np.sort(want["table"][:, 1])[len(want["table"]) // 2]) + 1
        assert 1 < cut <= want["table"][:, 1].max()
        bare = trk.mesh_features(jrec1, grid, what="tot", thr=thr, conn=4, min_pix=cut, keep=3)
        kept = ctx.keep_get(3)
        assert bare["labels"] is None and 0 < bare["nfeat"] < want["nfeat"] and kept["min_pix"] == cut
        assert np.array_equal(kept["labels"], kept_ref(want["labels"], cut)) and 0 < (kept["labels"] >= 0).sum() < want["nactive"]
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ advect
def test_advect_on_a_raster_of_two_trips():
    trk, jrec1, coarse, thr = mesh_case()
    try:
        ctx = trk.ctx
        nQ = len(trk.mesh_cells())
        grid = refined(coarse, TRIP2[0] * TRIP2[1])
        shape = launch_shape(grid[3], grid[4], kernel_constants())
        assert shape["strided"][0] >= 2 and shape["npix"] % 64 != 0, shape
        o0 =trk.mesh_raster(jrec1, grid, at="t0", fields=False)["owner"]
        o1 = trk.mesh_raster(jrec1, grid, at="t1", fields=False)["owner"]
        assert (o0 >= 0).any() and (o1 >= 0).any() and not np.array_equal(o0, o1)
        f = trk.mesh_features(jrec1, grid, what="tot", thr=thr, min_pix=2, labels=True, keep=0)
        L = ctx.keep_get(0)["labels"]
        assert np.array_equal(L, kept_ref(f["labels"], 2)) and (L >= 0).any()
        odd = np.random.default_rng(3).integers(-1, L.size, L.shape).astype(np.int32)       # any values of [-1, npix)
        ctx.keep_put(7, odd, conn=4, min_pix=1)
        for src, dst, m in ((0, 1, L), (7, 8, odd)):
            M, ncells, ncarried = advect_ref(m, o0, o1, nQ)
            assert trk.features_advect(jrec1, grid, src, dst) == {"ncells": ncells, "ncarried": ncarried}
            assert np.array_equal(ctx.keep_get(dst)["labels"], M) and np.array_equal(ctx.keep_get(src)["labels"], m)
            assert ncells > 50 and ncarried > 10000 and not np.array_equal(M, m)
    finally:
        trk.close()


def test_advect_equals_the_restatement_on_the_downloaded_owners():
    trk, jrec1, fine, thr = mesh_case()
    try:
        ctx = trk.ctx
        nQ = len(trk.mesh_cells())
        coarse = sit.raster_grid(fine[0], fine[0] + fine[2] * fine[3], fine[1], fine[1] + fine[2] * fine[4], 6.)
        for grid in (fine, coarse):                                    # pixels finer and coarser than the cells of 3.5 km
            o0 = trk.mesh_raster(jrec1, grid, at="t0", fields=False)["owner"]
            o1 = trk.mesh_raster(jrec1, grid, at="t1", fields=False)["owner"]
            assert (o0 >= 0).any() and (o1 >= 0).any() and not np.array_equal(o0, o1)
            f = trk.mesh_features(jrec1, grid, what="tot", thr=thr, min_pix=2, labels=True, keep=0)
            L = ctx.keep_get(0)["labels"]
            assert np.array_equal(L, kept_ref(f["labels"], 2)) and (L >= 0).any()
            M, ncells, ncarried = advect_ref(L, o0, o1, nQ)
            r = trk.features_advect(jrec1, grid, 0, 1)
            got = ctx.keep_get(1)
            assert np.array_equal(got["labels"], M) and (r["ncells"], r["ncarried"]) == (ncells, ncarried) and ncells > 0
            assert (got["shape"], got["conn"], got["min_pix"]) == (L.shape, 8, 2)
            if grid is fine:
                assert ncarried > 100 and not np.array_equal(M, L)
            assert np.array_equal(ctx.keep_get(0)["labels"], L)        # the source is what it was
            again = trk.features_advect(jrec1, grid, 0, 0)             # ... until it is the destination
            assert again == r and np.array_equal(ctx.keep_get(0)["labels"], M)
            # a map that was not made from this mesh: any values of [-1, npix)
            odd = np.random.default_rng(3).integers(-1, L.size, L.shape).astype(np.int32)
            ctx.keep_put(7, odd, conn=4, min_pix=1)
            M, ncells, ncarried = advect_ref(odd, o0, o1, nQ)
            assert trk.features_advect(jrec1, grid, 7, 8) == {"ncells": ncells, "ncarried": ncarried}
            assert np.array_equal(ctx.keep_get(8)["labels"], M) and ctx.keep_get(8)["conn"] == 4
        assert ctx.advect_kernel_ms() > 0.
        # an empty mesh carries nothing
        assert trk.mesh(0.01, jrec1 + 1, slot=2)["nQ"] == 0
        ctx.run((jrec1 + 1) % K, jrec1 + 1, 1)
        assert trk.features_advect(jrec1 + 1, coarse, 7, 8, slot=2) == {"ncells": 0, "ncarried": 0}
        assert (ctx.keep_get(8)["labels"] == -1).all() and ctx.keep_get(8)["shape"] == odd.shape
        # refusals leave both slots as they were
        lib, h = ctx._L, ctx._h
        n = _lib._i64(7)

        def call(frm=7, to=8, mesh=0, jrec=jrec1 + 1, y0=coarse[0], d=coarse[2], ny=coarse[3], nx=coarse[4]):
            return lib.sitrk_mesh_features_advect(h, frm, to, mesh, jrec, y0, coarse[1], d, ny, nx, C.byref(n), None)

        for kw, msg in (({"frm": 16}, b"keep_from must be in 0..15"), ({"to": -1}, b"keep_to must be in"), ({"frm": 12}, b"kept map 12 is empty"),
                        ({"mesh": 8}, b"mesh must be in 0..7"), ({"mesh": 5}, b"mesh 5 is empty"), ({"jrec": JREC0 - 1}, b"before the mesh's t0"),
                        ({"d": 0.}, b"d_km"), ({"y0": np.nan}, b"finite"), ({"ny": 0}, b"ny and nx"), ({"nx": coarse[4] + 1}, b"kept map 7 is")):
            assert call(**kw) == -1 and msg in lib.sitrk_last_error(h), kw
        assert n.value == 7 and np.array_equal(ctx.keep_get(7)["labels"], odd) and (ctx.keep_get(8)["labels"] == -1).all()
        assert lib.sitrk_mesh_features_advect(h, 7, 8, 0, jrec1 + 1, *coarse, None, None) == 0                # both counts are optional
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ the chain
def test_two_windows_through_the_api():
    trk, jrec1, grid, thr = mesh_case()
    try:
        ctx = trk.ctx
        nQ = len(trk.mesh_cells())
        o0 = trk.mesh_raster(jrec1, grid, at="t0", fields=False)["owner"]
        o1 = trk.mesh_raster(jrec1, grid, at="t1", fields=False)["owner"]
        f0 = trk.mesh_features(jrec1, grid, what="tot", thr=thr, min_pix=3, labels=True, keep=0)
        r = trk.features_advect(jrec1, grid, 0, 1)
        M, ncells, ncarried = advect_ref(kept_ref(f0["labels"], 3), o0, o1, nQ)
        assert (r["ncells"], r["ncarried"]) == (ncells, ncarried)
        assert trk.mesh(3.5, jrec1 + 1)["nQ"] > 256                    # the next window: a new mesh from the cloud as it is now
        jrec2 = advance(trk, jrec1 + 1, 2, 2)
        thr2 = half_threshold(trk, jrec2, grid)
        f1 = trk.mesh_features(jrec2, grid, what="tot", thr=thr2, min_pix=3, labels=True, keep=0)
        assert np.array_equal(ctx.keep_get(1)["labels"], M)
        B = kept_ref(f1["labels"], 3)
        assert np.array_equal(ctx.keep_get(0)["labels"], B)
        pairs, nhit = match_ref(M, B, 1)
        got = trk.features_match(1, 0, reach=1)
        assert nhit > 0 and len(pairs) > 3
        assert np.array_equal(got["pairs"], pairs) and (got["npair"], got["nhit"]) == (len(pairs), nhit)
        link = sit.link_features(got["pairs"], f0["table"], f1["table"])
        track, age = sit.feature_tracks([link], [len(f0["table"]), len(f1["table"])])
        assert link["dropped"] == 0 and (link["parent"] >= 0).any() and age[1].max() == 1 and np.isin(track[1][age[1] == 1], track[0]).all()
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ command line
def test_cli_deform_track_flag(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F", "--deform", "30", "--deform-window", "5", "--deform-grid", "10"]
    plain = drv.main(argv)
    with np.load(plain["files"][2]) as z:
        own, tot2 = z["m0_w0_owner"], z["m0_w0_div"] ** 2 + z["m0_w0_shr"] ** 2
    thr = float(np.sqrt(np.median(tot2[own[own >= 0]])))
    feat = argv + ["--deform-features", "tot@%r" % thr]
    capsys.readouterr()
    with np.load(drv.main(feat)["files"][2]) as z:                     # without the flag: the file every run wrote before
        e = {k: z[k] for k in z.files}
    assert "--deform-track" not in capsys.readouterr().out and not any(("track" in k or "pairs" in k or k.endswith("_age")) for k in e)
    with np.load(drv.main(feat + ["--deform-track"])["files"][2]) as z:
        d = {k: z[k] for k in z.files}
    log = capsys.readouterr().out
    new = ["track"] + ["m0_w%d_%s" % (w, s) for w in range(3) for s in ("track", "age")] + \
          ["m0_w%d_%s" % (w, s) for w in (1, 2) for s in ("pairs", "pairs_counts")]
    assert sorted(d) == sorted(list(e) + new)
    for k in e:                                                       # everything else is what it was
        assert np.array_equal(d[k], e[k]), k
    assert d["track"].tolist() == [1]
    links = []
    for w in range(3):
        pre = "m0_w%d_" % w
        rows = len(d[pre + "features"])
        assert d[pre + "track"].shape == d[pre + "age"].shape == (rows,) and d[pre + "track"].dtype == np.int64 and rows > 0
        if w:
            pairs = d[pre + "pairs"]
            assert pairs.dtype == np.int64 and pairs.shape == (d[pre + "pairs_counts"][0], 3) and d[pre + "pairs_counts"][1] > 0
            assert np.isin(pairs[:, 0], d["m0_w%d_features" % (w - 1)][:, 0]).all() and np.isin(pairs[:, 1], d[pre + "features"][:, 0]).all()
            assert (pairs[:, 2] >= 1).all() and (np.diff(pairs[:, 0] * (1 << 32) + pairs[:, 1]) > 0).all()
            links.append(sit.link_features(pairs, d["m0_w%d_features" % (w - 1)], d[pre + "features"]))
            line = [ln for ln in log.splitlines() if "--deform-track window %d mesh 0" % w in ln]
            assert len(line) == 1 and "continued" in line[0] and "split" in line[0], line
    track, age = sit.feature_tracks(links, [len(d["m0_w%d_features" % w]) for w in range(3)])
    for w in range(3):
        assert np.array_equal(d["m0_w%d_track" % w], track[w]) and np.array_equal(d["m0_w%d_age" % w], age[w])
    assert max(a.max() for a in age) >= 1                              # a track goes on across a window
    assert np.isin(track[1], track[0]).any() or np.isin(track[2], track[1]).any()
    # tools/deformation.py --track on the written series, for the cells of the first window
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    fc, fout = str(tmp_path / "cells.npy"), str(tmp_path / "trk.npz")
    np.save(fc, d["m0_w0_cells"])
    assert tool.main(["-i", plain["files"][0], "-c", fc, "-k", "0", "-K", "5", "--grid", "6", "--features", "tot@%r@2" % thr, "--track", "-o", fout]) == 0
    assert "--track 1: records 0 -> 5 against 5 -> 10" in capsys.readouterr().out
    with np.load(fout) as z:
        m = {k: z[k] for k in z.files}
    assert m["track_arg"].tolist() == [1, 10] and m["pairs"].shape == (m["pairs_counts"][0], 3)
    assert m["parent"].shape == (len(m["next_features"]),) and m["child"].shape == (len(m["features"]),)
    link = sit.link_features(m["pairs"], m["features"], m["next_features"])
    assert np.array_equal(link["parent"], m["parent"]) and np.array_equal(link["child"], m["child"]) and link["dropped"] == 0
