"""Dispersion of buoy pairs without a GPU: pairs_ref(), the numpy restatement of the contract of sitrk_pairs_points in
include/sitrk.h; the host helpers of sitrack_amd/dispersion.py on hand-made tables; every refusal the Python side makes before
any device work; and the analytic anchors of the contract, checked on the restatement itself.

pairs_ref() is a brute force over all i < j in blocks of rows: q0 and q1 exactly as the contract writes them (numpy evaluates one
rounded operation per symbol and fuses nothing), the class by comparisons against E_c = edges[c]*edges[c], the terms per class
kept as arrays and every sum taken with math.fsum, the exactly rounded sum.  tests/test_gpu_pairs.py compares the device with it."""
import math
import types

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, dispersion
from sitrack_amd import driver as drv

TERMS = ("r0", "e", "abs_e", "e2", "abs_e3", "d2")              # columns 1..6 of the table


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def pairs_ref(yx0, yx1, edges_km, mask0=None, mask1=None, block=256):
    """{"table" (nc,7), "npts", "terms": per class a (6, n_c) array of the terms of columns 1..6, "ij": per class (n_c, 2)}"""
    yx0 = np.asarray(yx0, dtype=np.float64).reshape(-1, 2)
    yx1 = np.asarray(yx1, dtype=np.float64).reshape(-1, 2)
    e = np.asarray(edges_km, dtype=np.float64)
    nc = len(e) - 1
    E = e * e
    ok = np.isfinite(yx0).all(axis=1) & np.isfinite(yx1).all(axis=1)
    if mask0 is not None:
        ok &= np.asarray(mask0) != 0
    if mask1 is not None:
        ok &= np.asarray(mask1) != 0
    idx = np.flatnonzero(ok)
    a, b = yx0[idx], yx1[idx]
    n = len(idx)
    terms = [[] for _ in range(nc)]
    ij = [[] for _ in range(nc)]
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        dy = a[None, :, 0] - a[i0:i1, None, 0]
        dx = a[None, :, 1] - a[i0:i1, None, 1]
        q0 = dy * dy + dx * dx
        dy = b[None, :, 0] - b[i0:i1, None, 0]
        dx = b[None, :, 1] - b[i0:i1, None, 1]
        q1 = dy * dy + dx * dx
        later = np.arange(n)[None, :] > np.arange(i0, i1)[:, None]
        for c in range(nc):
            sel = later & (E[c] <= q0) & (q0 < E[c + 1]) & (q0 > 0.)
            if not sel.any():
                continue
            s0, s1 = q0[sel], q1[sel]
            r0, r1 = np.sqrt(s0), np.sqrt(s1)
            d = (s1 - s0) / (r0 + r1)
            s = d / r0
            terms[c].append(np.stack([r0, s, np.abs(s), s * s, (s * s) * np.abs(s), d * d]))
            w = np.argwhere(sel)
            ij[c].append(np.stack([idx[w[:, 0] + i0], idx[w[:, 1]]], axis=1))
    table = np.zeros((nc, _lib.PAIRS_NCOLS))
    for c in range(nc):
        terms[c] = np.concatenate(terms[c], axis=1) if terms[c] else np.zeros((6, 0))
        ij[c] = np.concatenate(ij[c]) if ij[c] else np.zeros((0, 2), dtype=np.int64)
        table[c, 0] = terms[c].shape[1]
        table[c, 1:] = [math.fsum(row) for row in terms[c]]
    return {"table": table, "npts": int(n), "terms": terms, "ij": ij}


# ------------------------------------------------------------------------------------------------ shared cases
LAT_NY, LAT_NX, LAT_KM = 13, 11, 8.
LAT_EDGES = (8., 16., 24., 32.)


def lattice(ny=LAT_NY, nx=LAT_NX, km=LAT_KM):
    """ny x nx points `km` apart, integers: every q0 is exact"""
    j, i = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return np.stack([-40. + km * j.ravel(), 16. + km * i.ravel()], axis=1)


def lattice_counts(ny, nx, lo2, hi2):
    """pairs of an ny x nx unit lattice with lo2 <= a^2 + b^2 < hi2: an offset (a, b), a > 0 or a == 0 and b > 0, occurs
    (ny - a)*(nx - |b|) times"""
    n = 0
    for a in range(ny):
        for b in range(-(nx - 1), nx):
            if (a > 0 or b > 0) and lo2 <= a * a + b * b < hi2:
                n += (ny - a) * (nx - abs(b))
    return n


def smooth_move(yx, amp=0.03):
    """a smooth, slightly non-linear displacement of a few percent"""
    y, x = yx[:, 0], yx[:, 1]
    return np.stack([y + amp * (0.3 * y - 0.2 * x) + 0.4 * np.sin(x / 37.), x + amp * (0.1 * y + 0.25 * x) + 0.3 * np.cos(y / 29.)], axis=1)


def jitter_cloud(n_side=40, km=10., seed=11):
    j, i = np.meshgrid(np.arange(n_side, dtype=np.float64), np.arange(n_side - 3, dtype=np.float64), indexing="ij")
    yx = np.stack([-150. + km * j.ravel(), -2000. + km * i.ravel()], axis=1)
    return yx + np.random.default_rng(seed).uniform(-0.3 * km, 0.3 * km, yx.shape)


# ------------------------------------------------------------------------------------------------ the contract's anchors
def test_lattice_counts_are_the_closed_form_and_ties_go_to_the_upper_class():
    yx = lattice()
    r = pairs_ref(yx, smooth_move(yx), LAT_EDGES)
    assert r["npts"] == LAT_NY * LAT_NX
    want = [lattice_counts(LAT_NY, LAT_NX, (c + 1) ** 2, (c + 2) ** 2) for c in range(3)]
    assert r["table"][:, 0].tolist() == want and min(want) > 0
    # r0 == 8 exactly (q0 == E_0) is in class 0, r0 == 16 exactly (q0 == E_1) in class 1
    r0 = [t[0] for t in r["terms"]]
    assert (r0[0] == 8.).sum() == (LAT_NY - 1) * LAT_NX + LAT_NY * (LAT_NX - 1) and r0[0].min() == 8.
    assert (r0[1] == 16.).sum() == (LAT_NY - 2) * LAT_NX + LAT_NY * (LAT_NX - 2) and r0[1].min() == 16. and r0[0].max() < 16.
    # every pair once, i < j
    ij = np.concatenate(r["ij"])
    assert (ij[:, 0] < ij[:, 1]).all() and len(np.unique(ij[:, 0] * 1000 + ij[:, 1])) == len(ij)


def test_a_dilation_strains_every_pair_alike():
    yx = jitter_cloud(14)
    a = 0.0125
    r = pairs_ref(yx, (1. + a) * yx, dispersion.pair_edges(10., 80., 6))
    for c, t in enumerate(r["terms"]):
        assert t.shape[1] > 50 and np.abs(t[1] - a).max() <= 1e-12, c
    cur = sit.dispersion_curve(r["table"], 3600.)
    assert np.allclose(cur["mean"] * 3600., a, rtol=0, atol=1e-12) and np.allclose(cur["rate"][:, 0] * 3600., a, rtol=0, atol=1e-12)
    assert np.allclose(cur["d2"], a * a * np.array([math.fsum(t[0] ** 2) / t.shape[1] for t in r["terms"]]), rtol=1e-9)
    # no scale dependence: all three exponents vanish
    assert np.abs(sit.dispersion_exponents(r["table"], 3600.)["beta"]).max() < 1e-10


def test_a_rigid_motion_strains_no_pair():
    yx = jitter_cloud(14)
    th = 0.3
    rot = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    r = pairs_ref(yx, yx @ rot.T + np.array([12.5, -3.25]), dispersion.pair_edges(10., 80., 6))
    # coordinates of 2000 km, rounded to 2^-53 of that: a separation is off by some 1e-12 km, of at least 10 km
    assert all(t.shape[1] > 50 and np.abs(t[1]).max() < 1e-12 for t in r["terms"])


def test_validity_and_coincident_points():
    yx = lattice(4, 5)
    yx1 = smooth_move(yx)
    yx[7] = yx[6]                                                     # q0 == 0: excluded, even with edges[0] == 0
    full = pairs_ref(yx, yx1, (0., 8., 100.))
    assert full["npts"] == 20 and full["table"][:, 0].sum() == 20 * 19 // 2 - 1
    bad0, bad1 = yx.copy(), yx1.copy()
    bad0[3, 1] = np.nan
    bad1[11, 0] = np.inf
    m0 = np.ones(20, dtype=np.int8)
    m0[0] = 0
    r = pairs_ref(bad0, bad1, (0., 8., 100.), mask0=m0, mask1=np.arange(20) != 19)
    assert r["npts"] == 16 and r["table"][:, 0].sum() == 16 * 15 // 2 - 1
    assert not np.isin(np.concatenate(r["ij"]), [0, 3, 11, 19]).any()
    assert pairs_ref(yx[:1], yx1[:1], (0., 8.))["table"].tolist() == [[0.] * 7] and pairs_ref(yx[:0], yx1[:0], (0., 8.))["npts"] == 0


# ------------------------------------------------------------------------------------------------ the host helpers
def hand_table():
    t = np.zeros((4, 7))
    L = np.array([10., 20., 40., 80.])
    n = np.array([100., 50., 20., 0.])
    m = 1e-6 * L ** -0.5                                            # <|e|> falls like L^-0.5, <e^2> like L^-1.2, <|e|^3> like L^-2
    t[:, 0], t[:, 1], t[:, 2] = n, n * L, n * 0.25 * m
    t[:, 3], t[:, 4], t[:, 5], t[:, 6] = n * m, n * 1e-12 * L ** -1.2, n * 1e-18 * L ** -2., n * 3.
    return t, L, n


def test_curve_and_exponents_of_a_hand_made_table():
    t, L, n = hand_table()
    T = 86400.
    c = sit.dispersion_curve(t, T)
    assert sorted(c) == ["L_km", "d2", "mean", "n", "rate"] and c["rate"].shape == (4, 3)
    assert np.allclose(c["L_km"][:3], L[:3], rtol=1e-15) and np.allclose(c["d2"][:3], 3.) and np.array_equal(c["n"], n)
    assert np.allclose(c["rate"][:3, 0], 1e-6 * L[:3] ** -0.5 / T, rtol=1e-14) and np.allclose(c["mean"][:3], 0.25 * c["rate"][:3, 0])
    assert np.allclose(c["rate"][:3, 1], 1e-12 * L[:3] ** -1.2 / T ** 2, rtol=1e-14)
    # the class without a pair: NaN everywhere but its count
    assert c["n"][3] == 0. and all(np.isnan(c[k][3]).all() for k in ("L_km", "rate", "mean", "d2"))
    s = sit.dispersion_exponents(t, T, min_pairs=10)
    assert sorted(s) == ["L_km", "beta", "used"] and s["used"].tolist() == [True, True, True, False]
    assert np.allclose(s["beta"], [0.5, 1.2, 2.], rtol=0, atol=1e-12)
    # min_pairs drops the thin classes; fewer than two classes left: NaN
    s = sit.dispersion_exponents(t, T, min_pairs=30)
    assert s["used"].tolist() == [True, True, False, False] and np.allclose(s["beta"], [0.5, 1.2, 2.], rtol=0, atol=1e-12)
    assert np.isnan(sit.dispersion_exponents(t, T, min_pairs=60)["beta"]).all()
    for bad in (np.zeros((4, 6)), np.zeros(7)):
        with pytest.raises(ValueError, match="table"):
            sit.dispersion_curve(bad, T)
    for bad in (0., -1., math.nan, "x"):
        with pytest.raises(ValueError, match="`T`"):
            sit.dispersion_exponents(t, bad)


def test_pair_edges_and_pairs_arg():
    e = sit.pair_edges(10., 160., 8)
    assert e.shape == (9,) and e[0] == 10. and e[8] == 160. and np.allclose(e[1:] / e[:-1], 2. ** 0.5, rtol=1e-14)
    assert np.array_equal(sit.pairs_arg("10:160:8"), e) and np.array_equal(sit.pairs_arg(" 0,8,16.5 "), [0., 8., 16.5])
    assert sit.pairs_arg("5:6:1").tolist() == [5., 6.] and len(sit.pairs_arg("1:2:16")) == 17
    for bad in ("", "10", "10:160", "10:160:8:2", "10:160:0", "10:160:17", "10:160:2.5", "0:160:4", "160:10:4", "a:160:4", "inf:160:4",
                "1,1", "2,1", "-1,2", "1,nan", "1,inf", "1,2,x", ",".join(str(k) for k in range(18))):
        with pytest.raises(ValueError, match="--pairs"):
            sit.pairs_arg(bad)
    with pytest.raises(ValueError, match="--other"):
        sit.pairs_arg("1", "--other")
    for bad in ((10., 160., 0), (10., 160., 17), (10., 160., 2.5), (0., 160., 4), (-1., 160., 4), (160., 10., 4), (10., math.inf, 4), ("a", 1., 2)):
        with pytest.raises(ValueError, match="pair_edges"):
            sit.pair_edges(*bad)


# ------------------------------------------------------------------------------------------------ refusals before any device work
class NoDevice:
    """stands in for a Context: any call on it is a failure of the test"""
    nP = 20

    def __getattr__(self, name):
        raise AssertionError("the device was asked for %s" % name)


def test_pair_dispersion_refuses_before_any_device_work():
    yx = lattice(4, 5)
    ctx = NoDevice()
    ok = (0., 8., 16.)
    for args, kw, word in (((yx[:, 0], yx[:, 0], ok), {}, "yx0"), ((yx, yx[:5], ok), {}, "yx0"), ((np.zeros((20, 3)), np.zeros((20, 3)), ok), {}, "yx0"),
                           ((yx, yx, ok), {"mask0": np.ones(19)}, "mask0"), ((yx, yx, ok), {"mask1": np.ones((20, 1))}, "mask1"),
                           ((yx, yx, (8.,)), {}, "edges_km"), ((yx, yx, 8.), {}, "edges_km"), ((yx, yx, list(range(18))), {}, "edges_km"),
                           ((yx, yx, (8., 8.)), {}, "increase"), ((yx, yx, (8., 4.)), {}, "increase"), ((yx, yx, (-1., 4.)), {}, "increase"),
                           ((yx, yx, (1., math.nan)), {}, "finite"), ((yx, yx, (1., math.inf)), {}, "finite"), ((yx, yx, "abc"), {}, "edges_km"),
                           ((yx, yx, ((1., 2.), (3., 4.))), {}, "edges_km")):
        with pytest.raises(ValueError, match=word):
            sit.PairDispersion(*args, ctx=ctx, **kw)


def fake_tracker(jrec0=None):
    trk = object.__new__(sit.IceTracker)
    trk.ctx = NoDevice()
    trk._rdt = 3600.
    trk._pairs_jrec0 = jrec0
    return trk


def test_tracker_pairs_refuse_before_any_device_work():
    trk = fake_tracker()
    for bad in (1.5, "x", None):
        with pytest.raises(ValueError, match="jrec0"):
            trk.pairs_mark(bad)
    with pytest.raises(ValueError, match="mask"):
        trk.pairs_mark(3, mask=np.ones(19))
    with pytest.raises(ValueError, match="no mark"):
        trk.pairs(5, (1., 2.))
    trk = fake_tracker(jrec0=5)
    for bad in ((2., 1.), (1.,), (-1., 1.), (1., math.nan), list(range(18))):
        with pytest.raises(ValueError, match="edges_km"):
            trk.pairs(6, bad)
    for bad in (4, 5.5, "x"):
        with pytest.raises(ValueError, match="jrec1"):
            trk.pairs(bad, (1., 2.))


def test_driver_pairs_flags_are_checked_by_the_parser(capsys):
    base = ["-i", "a.nc", "-m", "b.nc", "-s", "c.nc"]
    a = drv.parse_args(base + ["--pairs", "10:160:8@25", "--pairs-window", "6", "--pairs-every", "2"])
    assert np.array_equal(a.pairs[0], sit.pair_edges(10., 160., 8)) and a.pairs[1] == 25. and (a.pairs_window, a.pairs_every) == (6, 2)
    a = drv.parse_args(base + ["--pairs", "1,2,4"])
    assert a.pairs[0].tolist() == [1., 2., 4.] and a.pairs[1] == 0. and (a.pairs_window, a.pairs_every) == (0, 0)
    assert drv.parse_args(base).pairs is None
    for extra, word in ((["--pairs", "10:160"], "--pairs"), (["--pairs", "2,1"], "--pairs"), (["--pairs", "1,2@0"], "RD_KM"),
                        (["--pairs", "1,2@x"], "RD_KM"), (["--pairs", "1,2@3@4"], "--pairs"), (["--pairs-window", "4"], "--pairs-window"),
                        (["--pairs-every", "2"], "--pairs-every"), (["--pairs", "1,2", "--pairs-window", "-1"], "--pairs-window"),
                        (["--pairs", "1,2", "--pairs-every", "-2"], "--pairs-every"), (["--pairs", "1,2", "--pairs-every", "x"], "--pairs-every")):
        with pytest.raises(SystemExit):
            drv.parse_args(base + extra)
        assert word in capsys.readouterr().err, extra


def test_pair_windows_and_their_records():
    # 14 records from 3, windows of 5, a table every 2 records and at the window's end
    w = drv.pair_windows(14, 3, 5, 2)
    assert w == [(3, [4, 6, 7]), (8, [9, 11, 12]), (13, [14, 16])]
    assert drv.pair_windows(14, 3, 0, 0) == [(3, [16])] and drv.pair_windows(14, 3, 0, 5) == [(3, [7, 12, 16])]
    assert drv.pair_windows(6, 0, 3, 3) == [(0, [2]), (3, [5])]
    assert sorted({j for _, js in w for j in js}) == drv.pair_cuts(w)
