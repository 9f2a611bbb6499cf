"""Distribution of values on the MI355X (sitrk_dist_values, sitrk_mesh_dist, IceTracker.mesh_dist, --deform-pdf, --deform-features
WHAT@pNN) against dist_ref() of tests/test_dist.py, the numpy restatement of the contract in include/sitrk.h.

Counts, comparisons and a selection on the bits of the values: every comparison of counts, values, ranks, m and nnan is bit
equality.  There is no tolerance anywhere in this file."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import distribution as dst
from sitrack_amd import driver as drv
from test_dist import (EDGE_EDGES, bits, dist_ref, edge_values, pass_families, pass_targets, same_dist, tie_q, trips_case)
from test_driver import make_case
from test_gpu_mesh import JREC0, K, advance, start

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def both_ways(ctx, x, edges=None, q=None, use=None):
    """the call with and without the per-wave aggregation of the select passes: the same bits, checked against the restatement"""
    ref = dist_ref(x, edges, q, use)
    try:
        for agg in (0, 1):
            ctx.set_tuning(dist_aggregate=agg)
            same_dist(ctx.dist_values(x, edges=edges, q=q, use=use), ref)
    finally:
        ctx.set_tuning(dist_aggregate=0)
    return ref


# ------------------------------------------------------------------------------------------------ 1. edge values
def test_edge_values(ctx):
    x, use = edge_values()
    q = tie_q(x, use)
    ref = both_ways(ctx, x, EDGE_EDGES, q, use)
    assert ref["nnan"] > 0 and ref["values"][0] == -np.inf and ref["values"][1] == np.inf
    both_ways(ctx, x, EDGE_EDGES, tie_q(x))                            # without `use`
    got = sit.ValueDistribution(x, EDGE_EDGES, q, use, ctx=ctx)        # the public function, and twice the same bits
    same_dist(got, ref)
    same_dist(sit.ValueDistribution(x, EDGE_EDGES, q, use, ctx=ctx), got)
    assert np.array_equal(got["edges"], EDGE_EDGES) and np.array_equal(got["q"], q)


def test_degenerate_samples(ctx):
    q3 = np.array([0., 0.5, 1.])
    both_ways(ctx, np.full(700, -2.5e-7), [-1., -2.5e-7, 0.], np.linspace(0., 1., 16))    # all equal, nq = 16
    both_ways(ctx, np.array([3.25]), [0., 5.], q3)                     # n = 1
    both_ways(ctx, np.array([-0.0]), [-1., 0., 1.], q3)
    # m = 0: no value at all, and every value excluded or a NaN
    for x, use in ((np.zeros(0), None), (np.arange(300.), np.zeros(300, dtype=np.int8)), (np.full(70, np.nan), None)):
        r = ctx.dist_values(x, edges=[0., 1.], q=q3, use=use)
        same_dist(r, dist_ref(x, [0., 1.], q3, use))
        assert r["m"] == 0 and np.isnan(r["values"]).all() and (r["ranks"] == -1).all() and (r["counts"] == 0).all()
    # nb = 0, 1, 1024; nq = 0 and 16
    x = np.random.default_rng(4).standard_normal(5000)
    r = ctx.dist_values(x, q=q3)
    assert r["counts"] is None
    same_dist(r, dist_ref(x, None, q3))
    r = ctx.dist_values(x, edges=[-0.5, 0.5])
    assert r["values"].shape == (0,) and r["ranks"].shape == (0,)
    same_dist(r, dist_ref(x, [-0.5, 0.5]))
    both_ways(ctx, x, sit.lin_edges(-3., 3., 1024), np.linspace(0., 1., 16))
    both_ways(ctx, x, sit.lin_edges(-3., 3., 1023), np.array([0.29]))
    x[::7] = x[3]                                                      # values exactly on edges of a fine histogram
    e = np.sort(np.unique(x))[::11][:1025]
    both_ways(ctx, x, e, q3)


def test_refusals_before_any_device_work(ctx):
    lib, h, p = ctx._L, ctx._h, _lib._ptr
    x = np.arange(8.)
    counts, qval, qrank = np.zeros(1026, dtype=np.int64), np.zeros(16), np.zeros(16, dtype=np.int64)
    m, nn = _lib._i64(0), _lib._i64(0)

    def call(n=8, nb=2, edges=(0., 1., 2.), nq=1, q=(0.5,), xs=x, cnt=counts):
        e = None if edges is None else np.array(edges, dtype=np.float64)
        qq = None if q is None else np.array(q, dtype=np.float64)
        return lib.sitrk_dist_values(h, n, p(xs), None, nb, p(e), p(cnt), nq, p(qq), p(qval), p(qrank), C.byref(m), C.byref(nn))

    assert call() == 0
    for kw, text in (({"edges": (0., 0., 1.)}, b"increase strictly"), ({"edges": (0., 2., 1.)}, b"increase strictly"),
                     ({"edges": (0., math.inf, 1.)}, b"not finite"), ({"edges": (math.nan, 0., 1.)}, b"not finite"),
                     ({"q": (1.5,)}, b"not in [0, 1]"), ({"q": (-1e-9,)}, b"not in [0, 1]"), ({"q": (math.nan,)}, b"not in [0, 1]"),
                     ({"nb": -1}, b"nb must be"), ({"nb": 1025}, b"nb must be"), ({"nq": 17}, b"nq must be"), ({"nq": -1}, b"nq must be"),
                     ({"edges": None}, b"null edges"), ({"cnt": None}, b"null edges"), ({"q": None}, b"null q"),
                     ({"n": -1}, b"n must be"), ({"xs": None}, b"null array")):
        assert call(**kw) == -1 and text in lib.sitrk_last_error(h), kw
    assert call() == 0
    with pytest.raises(_lib.SitrkError, match="dist_aggregate must be 0 or 1"):
        ctx.set_tuning(dist_aggregate=2)


# ------------------------------------------------------------------------------------------------ 2. every pass decides
def test_every_pass_of_the_select_decides(ctx):
    x, fam = pass_families()
    q = pass_targets(x, fam)
    ref = both_ways(ctx, x, None, q)
    assert len(set(bits(ref["values"]).tolist())) == 16
    # the same families shuffled: no wave is uniform any more, the result is the same
    perm = np.random.default_rng(9).permutation(x.shape[0])
    same_dist(ctx.dist_values(x[perm], q=q), ref)
    # ... and negated: the keys' bytes are the complements, every pass still decides
    both_ways(ctx, -x, None, q)


# ------------------------------------------------------------------------------------------------ 3. past the first trip
def test_past_the_first_trip(ctx):
    x, edges, q, info = trips_case()
    ref = both_ways(ctx, x, edges, q)
    assert ref["m"] + ref["nnan"] == info["n"]
    # the timers of the last call
    ms = ctx.dist_kernel_ms()
    assert len(ms) == 3 and all(t >= 0. for t in ms)


# ------------------------------------------------------------------------------------------------ 4. the mesh form
def sample_of(r, what, sgn):
    """the restatement's input from what mesh_deform downloads"""
    if what == "tot":
        return r["div"] * r["div"] + r["shr"] * r["shr"]
    f = r[what]
    return f if sgn > 0 else -f if sgn < 0 else np.abs(f)


def test_mesh_dist_equals_the_restatement_on_what_mesh_deform_downloads():
    trk = start()
    try:
        assert trk.mesh(3.5, JREC0)["nQ"] > 256
        jrec1 = advance(trk, JREC0, 2, 2)
        r = trk.mesh_deform(jrec1)
        use = (r["status"] == 1).astype(np.int8)
        assert 0 < use.sum() < len(use)
        q = np.array([0., 0.5, 0.85, 0.99, 1.])
        before = (trk.mesh_deform(jrec1), trk.ctx.fetch())
        for what in ("div", "shr", "vor", "tot"):
            for sgn in ((1,) if what == "tot" else (1, -1, 0)):
                x = sample_of(r, what, sgn)
                lo, hi = float(x[use != 0].min()), float(x[use != 0].max())
                edges = np.linspace(lo, hi, 12)[1:-1]                  # some cells below, some at or above
                got = trk.ctx.mesh_dist(0, jrec1, what, sgn=sgn, edges=edges, q=q)
                same_dist(got, dist_ref(x, edges, q, use))
                assert got["counts"].sum() == got["m"] == int(r["stats"]["n1"]) and got["nnan"] == 0
        # the tracker's method: the edges of tot are squared on the way in, the values are the roots of the selected t2
        t2 = sample_of(r, "tot", 1)
        e = np.linspace(0., math.sqrt(float(t2[use != 0].max())), 9)[1:]
        got = trk.mesh_dist(jrec1, "tot", edges=e, q=q)
        ref = dist_ref(t2, e * e, q, use)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(bits(got["t2"]), bits(ref["values"]))
        assert np.array_equal(bits(got["values"]), bits(np.sqrt(ref["values"]))) and np.array_equal(got["edges"], e)
        same_dist(trk.mesh_dist(jrec1, "div", sgn=-1, edges=[-1e-6, 0., 1e-6], q=q), dist_ref(-r["div"], [-1e-6, 0., 1e-6], q, use))
        # nothing of the tracker has moved
        after = (trk.mesh_deform(jrec1), trk.ctx.fetch())
        for n in ("div", "shr", "vor", "area0", "area1", "status"):
            assert np.array_equal(before[0][n], after[0][n], equal_nan=True)
        assert before[0]["stats"] == after[0]["stats"] and np.array_equal(bits(before[1]["yx"]), bits(after[1]["yx"]))
    finally:
        trk.close()


def test_mesh_dist_leaves_the_other_readings_as_they_were():
    trk = start()
    try:
        trk.mesh(3.5, JREC0)
        jrec1 = advance(trk, JREC0, 2, 1)
        s = trk.ctx.fetch()
        lo, hi = s["yx"][s["alive"] != 0].min(axis=0), s["yx"][s["alive"] != 0].max(axis=0)
        grid = sit.raster_grid(lo[0], hi[0], lo[1], hi[1], 1.1)

        def readings():
            d = trk.mesh_deform(jrec1)
            f = trk.mesh_features(jrec1, grid, what="tot", thr=1e-7, labels=True)
            c = trk.mesh_coarse(jrec1, grid, 4)
            return ([bits(d[n]) for n in ("div", "shr", "vor", "area0", "area1")] + [d["status"], f["table"], f["labels"], bits(c["table"])],
                    (d["stats"], f["nfeat"], f["ncomp"], f["nactive"], c["nin"], c["nout"]))

        a = readings()
        d = trk.mesh_dist(jrec1, "tot", edges=sit.log_edges(1e-9, 1e-4, 32), q=dst.PDF_Q)
        assert d["m"] > 0
        b = readings()
        assert all(np.array_equal(u, v) for u, v in zip(a[0], b[0])) and a[1] == b[1]
    finally:
        trk.close()


def test_mesh_dist_errors_and_the_empty_mesh():
    trk = start()
    try:
        q = [0.5]
        with pytest.raises(_lib.SitrkError, match="mesh 0 is empty"):
            trk.mesh_dist(JREC0, "tot", q=q)
        assert trk.mesh(0.01, JREC0, slot=2)["nQ"] == 0                # an empty mesh: zeros, m = 0
        trk.ctx.run(JREC0 % K, JREC0, 1)
        r = trk.mesh_dist(JREC0, "div", edges=[-1., 0., 1.], q=[0., 1.], slot=2)
        assert r["m"] == 0 and r["nnan"] == 0 and (r["counts"] == 0).all() and np.isnan(r["values"]).all() and (r["ranks"] == -1).all()
        assert trk.mesh(3.5, JREC0 + 1)["nQ"] > 256
        with pytest.raises(_lib.SitrkError, match="before the mesh's t0"):
            trk.mesh_dist(JREC0, "tot", q=q)
        for kw, text in (({"what": 4}, "what must be"), ({"what": -1}, "what must be"), ({"sgn": 2}, "sgn must be"),
                         ({"what": 3, "sgn": -1}, "needs sgn"), ({"what": 3, "sgn": 0}, "needs sgn"), ({"mesh": 8}, "mesh must be")):
            a = {"mesh": 0, "what": 0, "sgn": 1}
            a.update(kw)
            with pytest.raises(_lib.SitrkError, match=text):
                trk.ctx.mesh_dist(a["mesh"], JREC0 + 1, a["what"], sgn=a["sgn"], q=q)
        with pytest.raises(_lib.SitrkError, match="increase strictly"):
            trk.ctx.mesh_dist(0, JREC0 + 1, 0, edges=np.array([1., 0.]))
        with pytest.raises(_lib.SitrkError, match=r"not in \[0, 1\]"):
            trk.ctx.mesh_dist(0, JREC0 + 1, 0, q=np.array([2.]))
        for kw in ({"what": "curl"}, {"sgn": 2}, {"what": "tot", "sgn": -1}, {"edges": [1., 0.]}, {"q": [2.]},
                   {"what": "tot", "edges": [-1., 1.]}):
            with pytest.raises(ValueError):
                trk.mesh_dist(JREC0 + 1, **kw)
        trk.ctx.run((JREC0 + 1) % K, JREC0 + 1, 1)                     # the handle is still usable
        assert trk.mesh_dist(JREC0 + 1, "tot", q=q)["m"] > 0
    finally:
        trk.close()
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            c.mesh_dist(0, 3, 0, q=np.array([0.5]))
        with pytest.raises(_lib.SitrkError, match="no distribution call"):
            c.dist_kernel_ms()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 5. the threshold
def test_features_at_a_percentile_equal_features_at_that_number():
    trk = start()
    try:
        trk.mesh(3.5, JREC0)
        jrec1 = advance(trk, JREC0, 2, 2)
        s = trk.ctx.fetch()
        lo, hi = s["yx"][s["alive"] != 0].min(axis=0), s["yx"][s["alive"] != 0].max(axis=0)
        grid = sit.raster_grid(lo[0], hi[0], lo[1], hi[1], 0.9)
        r = trk.mesh_deform(jrec1)
        ok = r["status"] == 1
        for what, sgn, q in (("tot", 1, 0.85), ("div", -1, 0.5), ("shr", 1, 0.9)):
            d = trk.mesh_dist(jrec1, what, sgn=sgn, q=[q])
            sel = d["t2"][0] if what == "tot" else d["values"][0]
            thr = sit.percentile_threshold(what, sel)
            x = sample_of(r, what, sgn)
            assert sel in x[ok]                                        # bit for bit the rate of one cell ...
            # ... and that cell and every status-1 cell at or above it pass the test of mesh_features at thr
            passed = (x >= thr * thr) if what == "tot" else (x >= thr)
            assert passed[ok & (x >= sel)].all() and passed[ok].sum() >= d["m"] - d["ranks"][0]
            # the number a user would type in comes from the downloaded arrays alone: the restatement's order statistic, then the
            # threshold.  It is the device's, and the features at it are those of a mask made in numpy from mesh_raster's owners
            typed = sit.percentile_threshold(what, dist_ref(x, None, [q], ok)["values"][0])
            assert typed == thr
            got = trk.mesh_features(jrec1, grid, what=what, thr=typed, sgn=sgn, labels=True)
            own = trk.mesh_raster(jrec1, grid, fields=False)["owner"]
            mask = (own >= 0) & passed[np.maximum(own, 0)]
            assert got["nactive"] == int(mask.sum()) > 0 and np.array_equal(got["labels"] >= 0, mask)
    finally:
        trk.close()


# ------------------------------------------------------------------------------------------------ 6. driver and tool
PDF = "tot@1e-9:1e-4:32,div@-1e-5:1e-5:20@lin"


def test_cli_deform_pdf_and_percentile_features(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), nP=1200)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "-F", "--deform", "30", "--deform-window", "5", "--deform-grid", "4"]
    plain = drv.main(argv)                                            # the parent's flags: the file every run wrote before
    log = capsys.readouterr().out
    assert "--deform-pdf" not in log and "percentile" not in log
    with np.load(plain["files"][2]) as z:
        e = {k: z[k] for k in z.files}
    assert not any("pdf" in k or "_q_" in k or "features" in k for k in e)
    out = drv.main(argv + ["--deform-pdf", PDF, "--deform-features", "tot@p85"])
    log = capsys.readouterr().out
    with np.load(out["files"][2]) as z:
        d = {k: z[k] for k in z.files}
    nw = len(d["windows"])
    new = (["features", "features_pct", "pdf_q", "pdf_tot_edges", "pdf_div_edges"]
           + ["m0_w%d_%s" % (w, s) for w in range(nw) for s in ("features", "features_counts", "features_thr", "pdf_tot", "q_tot", "pdf_div", "q_div")])
    assert sorted(d) == sorted(list(e) + new)
    for k in e:                                                       # everything else is what it was
        assert np.array_equal(d[k], e[k]), k
    assert np.array_equal(d["pdf_q"], dst.PDF_Q) and d["features_pct"].tolist() == [85.]
    assert np.array_equal(d["pdf_tot_edges"], sit.log_edges(1e-9, 1e-4, 32)) and np.array_equal(d["pdf_div_edges"], sit.lin_edges(-1e-5, 1e-5, 20))
    assert d["features"][0] == 3. and d["features"][1] == 1. and math.isnan(d["features"][2]) and d["features"][3:].tolist() == [1., 8.]
    grid = tuple(d["grid"][:3]) + (int(d["grid"][3]), int(d["grid"][4]))
    for w in range(nw):
        pre = "m0_w%d_" % w
        use = (d[pre + "status"] == 1).astype(np.int8)
        t2 = d[pre + "div"] * d[pre + "div"] + d[pre + "shr"] * d[pre + "shr"]
        et = d["pdf_tot_edges"]
        ref = dist_ref(t2, et * et, dst.PDF_Q, use)
        assert d[pre + "pdf_tot"].shape == (34,) and d[pre + "pdf_tot"].dtype == np.int64 and np.array_equal(d[pre + "pdf_tot"], ref["counts"])
        assert d[pre + "q_tot"].shape == (6,) and np.array_equal(bits(d[pre + "q_tot"]), bits(np.sqrt(ref["values"])))
        ref = dist_ref(d[pre + "div"], d["pdf_div_edges"], dst.PDF_Q, use)
        assert d[pre + "pdf_div"].shape == (22,) and np.array_equal(d[pre + "pdf_div"], ref["counts"])
        assert np.array_equal(bits(d[pre + "q_div"]), bits(ref["values"])) and ref["m"] == int(d[pre + "stats"][1]) > 0
        thr = sit.percentile_threshold("tot", dist_ref(t2, None, [0.85], use)["values"][0])
        assert d[pre + "features_thr"].shape == () and float(d[pre + "features_thr"]) == thr
        assert ("--deform-features window %d mesh 0: percentile 85 of tot" % w) in log and ("THR = %r /s" % thr) in log
        assert len([ln for ln in log.splitlines() if "--deform-pdf window %d mesh 0 " % w in ln]) == 2
    # the features at the resolved number, typed in: the same tables
    typed = drv.main(argv + ["--deform-features", "tot@%r" % float(d["m0_w0_features_thr"])])
    capsys.readouterr()
    with np.load(typed["files"][2]) as z:
        assert np.array_equal(z["m0_w0_features"], d["m0_w0_features"]) and np.array_equal(z["m0_w0_features_counts"], d["m0_w0_features_counts"])
    assert len(d["m0_w0_features"]) > 0
    # tools/deformation.py --pdf and --features WHAT@pNN on the written series: sit.ValueDistribution on its per-cell arrays
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    fc, fout = str(tmp_path / "cells.npy"), str(tmp_path / "pdf.npz")
    np.save(fc, d["m0_w0_cells"])
    assert tool.main(["-i", out["files"][0], "-c", fc, "-k", "0", "-K", "5", "--grid", "3", "--pdf", PDF + ",avor@1e-9:1e-4:8",
                      "--features", "conv@p50@1@8", "-o", fout]) == 0
    assert "--pdf tot:" in capsys.readouterr().out
    with np.load(fout) as z:
        m = {k: z[k] for k in z.files}
    use = m["valid"].astype(np.int8)
    ref = dist_ref(m["div"] * m["div"] + m["shr"] * m["shr"], m["pdf_tot_edges"] * m["pdf_tot_edges"], dst.PDF_Q, use)
    assert np.array_equal(m["pdf_tot"], ref["counts"]) and np.array_equal(bits(m["q_tot"]), bits(np.sqrt(ref["values"])))
    ref = dist_ref(np.abs(m["vor"]), m["pdf_avor_edges"], dst.PDF_Q, use)
    assert np.array_equal(m["pdf_avor"], ref["counts"]) and np.array_equal(bits(m["q_avor"]), bits(ref["values"]))
    assert float(m["features_thr"]) == dist_ref(-m["div"], None, [0.5], use)["values"][0] and float(m["features_pct"]) == 50.
    assert m["features_arg"].tolist() == [0., -1., float(m["features_thr"]), 1., 8.] and m["features_counts"][2] > 0
