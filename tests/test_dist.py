"""Distribution of values (sitrk_dist_values, sitrk_mesh_dist): dist_ref(), the numpy restatement of the contract
in include/sitrk.h; the builders of the inputs that tests/test_gpu_dist.py gives the device, each with the proof that it tests
what it claims; and the host side -- edges, densities, the tail's slope, the threshold of a percentile, the command line.

The contract is counts, comparisons and a selection on the bits of the values: every comparison of a device result with
dist_ref() is bit equality, and there is no tolerance anywhere except in the slope of a fitted line (test_tail_exponent_...),
where it is derived from the rounding of the counts."""
import math
import os
import re

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import distribution as dst
from sitrack_amd import driver as drv
from sitrack_amd import features as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sitrack_amd", "csrc", "sitrk_dist.hip")
TOP = np.uint64(1) << np.uint64(63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the restatement
def key_of(v):
    """the monotone 64-bit key of fp64 values: b ^ (b >> 63 ? ~0 : 1 << 63)"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, b ^ ALL, b ^ TOP)


def value_of(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k >> np.uint64(63)) != 0, k ^ TOP, k ^ ALL).view(np.float64)


def rank_of(q, m):
    """k = min(m - 1, (int64)floor(q * (double)m)), one rounded product; -1 for an empty sample"""
    if m == 0:
        return -1
    return min(m - 1, int(math.floor(np.float64(q) * np.float64(m))))


def dist_ref(x, edges=None, q=None, use=None):
    x = np.asarray(x, dtype=np.float64).ravel()
    inn = np.ones(x.shape, dtype=bool) if use is None else np.asarray(use).ravel() != 0
    nan = inn & np.isnan(x)
    v = x[inn & ~nan] + 0.0                                            # -0.0 -> +0.0
    m = int(v.shape[0])
    counts = None
    if edges is not None:
        e = np.asarray(edges, dtype=np.float64)
        counts = np.bincount(np.searchsorted(e, v, side="right"), minlength=e.shape[0] + 1).astype(np.int64)
    qq = np.zeros(0) if q is None else np.asarray(q, dtype=np.float64)
    keys = np.sort(key_of(v))
    ranks = np.array([rank_of(t, m) for t in qq], dtype=np.int64)
    values = np.array([value_of(keys[k:k + 1])[0] if k >= 0 else np.nan for k in ranks], dtype=np.float64)
    return {"counts": counts, "values": values, "ranks": ranks, "m": m, "nnan": int(nan.sum())}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_dist(got, ref):
    """bit equality of everything a distribution call returns"""
    assert got["m"] == ref["m"] and got["nnan"] == ref["nnan"], (got["m"], ref["m"], got["nnan"], ref["nnan"])
    if ref["counts"] is None:
        assert got["counts"] is None
    else:
        assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], ref["counts"])
        assert int(got["counts"].sum()) == ref["m"]
    assert np.array_equal(got["ranks"], ref["ranks"])
    assert np.array_equal(bits(got["values"]), bits(ref["values"])), (got["values"], ref["values"])


def constants():
    """the launch constants of sitrk_dist.hip, read from the source text"""
    text = open(SRC).read()
    out = {}
    for name in ("kDistThreads", "kDistWide", "kDistMaxBlocks", "kDistUnroll", "kDistRowLanes", "kDistSumCols", "kDistSumRows", "kDistDigits"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


# ------------------------------------------------------------------------------------------------ 1. edge values
EDGE_EDGES = np.array([-np.finfo(np.float64).max, -1.5, -0.0, 5e-324, 1.0, 1.0 + 2.0 ** -52, 7.25, np.finfo(np.float64).max])


def edge_values():
    """about 1000 values: both zeros, denormals, both infinities, NaNs of both signs, negative numbers, long runs of duplicates,
    values exactly on the edges of EDGE_EDGES, and a `use` with zeros (some of them on NaNs and on values that would matter)"""
    rng = np.random.default_rng(21)
    tiny = np.array([5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308])
    nans = np.array([np.nan, -np.nan, np.uint64(0x7FF0000000000001).view(np.float64), np.uint64(0xFFFFFFFFFFFFFFFF).view(np.float64)])
    x = np.concatenate([np.array([0.0, -0.0] * 20), np.tile(tiny, 5), np.array([np.inf, -np.inf] * 4), np.tile(nans, 6),
                        -np.abs(rng.standard_normal(150)) * 3.0, np.full(200, 1.0), np.full(120, -1.5), np.tile(EDGE_EDGES, 4),
                        rng.standard_normal(300) * 1e-6, rng.uniform(0., 9., 100)])
    x = x[rng.permutation(x.shape[0])]
    use = (rng.uniform(size=x.shape[0]) > 0.2).astype(np.int8)
    return x, use


# q = 0 and 1, plain ones, and four that land on the two sides of the ties of the runs of 1.0 and -1.5 (filled by tie_q)
def tie_q(x, use=None):
    """quantiles whose ranks are the first and the last position of a run of duplicates and the positions next to it"""
    ref = dist_ref(x, use=use)
    inn = np.ones(x.shape, bool) if use is None else use != 0
    v = np.sort(x[inn & ~np.isnan(x)] + 0.0)
    m = ref["m"]
    qs = [0.0, 1.0, 0.5, 0.85]
    for dup in (1.0, -1.5):
        a, b = int(np.searchsorted(v, dup, "left")), int(np.searchsorted(v, dup, "right"))
        assert b - a > 50
        for pos in (a - 1, a, b - 1, b):
            qs.append((pos + 0.5) / m)
    return np.array(qs)


def test_restatement_on_the_edge_values():
    x, use = edge_values()
    assert 900 <= x.shape[0] <= 1100 and (use == 0).sum() > 100
    assert np.isnan(x[use == 0]).any() and np.isnan(x[use != 0]).any()
    q = tie_q(x, use)
    r = dist_ref(x, EDGE_EDGES, q, use)
    assert r["nnan"] == int(np.isnan(x[use != 0]).sum()) and r["m"] == int((use != 0).sum()) - r["nnan"]
    assert r["counts"].sum() == r["m"] and (r["counts"] > 0).all()
    # the zeros: -0.0 is an edge and both zeros count as at or above it; the selected zero is +0.0
    v = np.sort(x[(use != 0) & ~np.isnan(x)])
    assert r["values"][0] == -np.inf and r["values"][1] == np.inf
    for k, val in zip(r["ranks"], r["values"]):
        assert val == v[k] and not (val == 0. and np.signbit(val))
    # the two sides of a tie: rank a - 1 is below the run, a and b - 1 in it, b above it
    t = r["values"][4:8]
    assert t[0] < 1.0 and t[1] == 1.0 and t[2] == 1.0 and t[3] > 1.0
    # the order of the keys is the order of the values
    k = key_of(v + 0.0)
    assert (np.diff(k.astype(object)) >= 0).all() and np.array_equal(bits(value_of(k)), bits(v + 0.0))
    # an empty sample
    e = dist_ref(np.array([np.nan, 1.0]), [0., 1.], [0., 0.5, 1.], use=np.array([1, 0]))
    assert e["m"] == 0 and e["nnan"] == 1 and np.isnan(e["values"]).all() and (e["ranks"] == -1).all() and (e["counts"] == 0).all()


def test_rank_formula_is_one_product():
    assert rank_of(1.0, 10) == 9 and rank_of(0.0, 10) == 0 and rank_of(0.85, 20) == 17 and rank_of(0.5, 1) == 0 and rank_of(0.3, 0) == -1
    # 0.29 * 100 rounds to 28.999999999999996: the rank is 28, what the device's one product gives too
    assert rank_of(0.29, 100) == 28


# ------------------------------------------------------------------------------------------------ 2. every pass decides
BASE_KEY = 0xBE98D4B5A6C7E8F1            # the key of +3.7e-7-ish: byte 1 = 0x98 keeps every variant of bytes 0 and 1 finite
FAMILY_N = 3000


def byte_of(keys, p):
    return (np.asarray(keys, dtype=np.uint64) >> np.uint64(56 - 8 * p)) & np.uint64(255)


def pass_families():
    """Eight families of FAMILY_N keys: the members of family p are BASE_KEY with byte p (0 = the top one, the digit of pass p)
    replaced, so they differ from each other ONLY in byte p.  Family 7 takes all 256 values of its byte, in turn, so that a wave
    of it is uniform in the digits of passes 0..6 and spread in pass 7; family 0 takes 200 values of the top byte at random, so
    that a wave of it is not uniform in the top pass.  Returns (x, fam): the values family after family, and each one's family."""
    rng = np.random.default_rng(8)
    keys, fam = [], []
    for p in range(8):
        if p == 7:
            d = np.arange(FAMILY_N) % 256
        elif p == 0:
            d = rng.choice(np.r_[1:0x7F, 0x80:0xFF], 200, replace=False)[rng.integers(0, 200, FAMILY_N)]
        else:
            d = rng.integers(0, 256, FAMILY_N)
        sh = np.uint64(56 - 8 * p)
        k = (np.uint64(BASE_KEY) & ~(np.uint64(255) << sh)) | (d.astype(np.uint64) << sh)
        keys.append(k)
        fam.append(np.full(FAMILY_N, p))
    keys, fam = np.concatenate(keys), np.concatenate(fam)
    x = value_of(keys)
    assert np.isfinite(x).all() and np.array_equal(key_of(x), keys)
    return x, fam


def pass_targets(x, fam):
    """sixteen quantiles, two per family: the sorted positions of two members of family p whose byte p differs"""
    keys = key_of(x)
    order = np.argsort(keys, kind="stable")
    m = x.shape[0]
    q = []
    for p in range(8):
        pos = np.where(fam[order] == p)[0]
        b = byte_of(keys[order][pos], p)
        first = pos[0]
        other = pos[np.where(b != b[0])[0][-1]]
        q += [(first + 0.5) / m, (other + 0.5) / m]
    return np.array(q)


def first_difference(a, b):
    """the pass at which the prefixes of two keys diverge"""
    for p in range(8):
        if byte_of(a, p) != byte_of(b, p):
            return p
    return 8


def test_pass_families_make_every_pass_decide():
    x, fam = pass_families()
    q = pass_targets(x, fam)
    r = dist_ref(x, q=q)
    tk = key_of(r["values"])
    assert len(q) == 16 and len(set(tk.tolist())) == 16
    # the two targets of family p share bytes 0 .. p-1 and part at pass p: every one of the eight passes separates a pair
    assert [first_difference(tk[2 * p], tk[2 * p + 1]) for p in range(8)] == list(range(8))
    # ... and a target of family p parts from one of family g > p no later than pass p
    for p in range(8):
        for g in range(p + 1, 8):
            assert first_difference(tk[2 * p + 1], tk[2 * g + 1]) <= p
    # within a family only byte p varies
    k = key_of(x)
    for p in range(8):
        for o in range(8):
            nvals = len(np.unique(byte_of(k[fam == p], o)))
            assert (nvals > 1) == (o == p), (p, o, nvals)
    assert len(np.unique(byte_of(k[fam == 7], 7))) == 256
    # the waves: 64 consecutive values.  Some are uniform in the top digit (the aggregated add), some are not (the plain adds)
    top = byte_of(k, 0)[: (k.shape[0] // 64) * 64].reshape(-1, 64)
    uniform = (top == top[:, :1]).all(axis=1)
    assert uniform.sum() > 100 and (~uniform).sum() > 20
    # ... and in the last pass the waves of family 7 match a target's prefix with 64 different digits
    w7 = byte_of(k[fam == 7][:64], 7)
    assert len(np.unique(w7)) == 64


# ------------------------------------------------------------------------------------------------ 3. past the first trip
def trips_case():
    """(x, edges, q, info): a few times cap x threads of the capped count launches plus a remainder that is no multiple of a
    workgroup.  The values of the first round of trips lie in [0, 1); those behind them -- reached only by later trips -- in
    [-3, -2) and [2, 3), in bins nothing else falls in, and the quantiles near 0 and 1 select among them."""
    c = constants()
    per_trip = c["kDistMaxBlocks"] * c["kDistWide"]
    n = c["kDistUnroll"] * per_trip + 3 * c["kDistThreads"] + 9
    rng = np.random.default_rng(3)
    x = rng.uniform(0., 1., n)
    late = n - c["kDistUnroll"] * per_trip                            # the elements of the second round of the unrolled loop
    x[per_trip:2 * per_trip:7] = rng.uniform(2., 3., len(x[per_trip:2 * per_trip:7]))      # the second trip of the first round
    x[n - late:] = np.where(np.arange(late) % 2 == 0, rng.uniform(-3., -2., late), rng.uniform(2., 3., late))
    x[5::1001] = np.nan
    edges = np.array([-3., -2.5, -2., 0., 0.25, 0.5, 0.75, 1., 2., 2.5, 3.])
    q = np.array([0.0, 1e-4, 3e-4, 0.5, 0.9, 0.999, 0.9999, 1.0])
    return x, edges, q, {"n": n, "per_trip": per_trip, "late": late, "c": c}


def test_trips_case_goes_past_the_first_trip():
    x, edges, q, info = trips_case()
    c, n = info["c"], info["n"]
    assert 2e5 < n < 2e6
    # the capped launches: cap workgroups, more than one round of the unrolled trips, a last workgroup that is not full
    blocks = min(-(-n // c["kDistWide"]), c["kDistMaxBlocks"])
    trips = -(-n // (blocks * c["kDistWide"]))
    assert blocks == c["kDistMaxBlocks"] and trips == c["kDistUnroll"] + 1 and n % c["kDistThreads"] != 0 and n % c["kDistWide"] != 0
    # the rows of partials: m / nnan (one per workgroup of the key kernel, kDistThreads lanes read them), the histogram's (one per
    # workgroup of the count launch, kDistSumRows side by side), the pick kernel's (kDistRowLanes side by side, kDistUnroll in flight)
    key_rows = -(-n // c["kDistThreads"])
    assert -(-key_rows // c["kDistThreads"]) >= 2
    assert -(-blocks // c["kDistSumRows"]) >= 2
    assert -(-blocks // (c["kDistRowLanes"] * c["kDistUnroll"])) >= 2
    full = dist_ref(x, edges, q)
    assert full["nnan"] > 100

    def differs(sub):
        r = dist_ref(x[sub], edges, q)
        return (np.where(r["counts"] != full["counts"])[0].tolist(),
                np.where(bits(r["values"]) != bits(full["values"]))[0].tolist(), r)

    idx = np.arange(n)
    # the first trip alone, and the first round of the unrolled loop alone: bins -- some of them empty -- and values differ
    for first in (idx < info["per_trip"], idx < c["kDistUnroll"] * info["per_trip"]):
        bins, vals, r = differs(first)
        assert bins and vals and r["m"] != full["m"] and r["nnan"] != full["nnan"]
        assert (r["counts"][[1, 2, 9, 10]] == 0).all() or (r["counts"][[1, 2]] == 0).all()
        assert (full["counts"][[1, 2, 9, 10]] > 0).all()
    # the values selected near the two ends are ones only the last round reaches
    last_round = x[c["kDistUnroll"] * info["per_trip"]:]
    assert full["values"][1] in last_round and full["values"][2] in last_round and full["values"][-2] >= 2.
    # the first trip of each row-summing loop alone: the rows of the first kDistThreads key workgroups, of the first kDistSumRows
    # and of the first kDistRowLanes count workgroups
    count_block = (idx // c["kDistWide"]) % c["kDistMaxBlocks"]
    for first in (idx // c["kDistThreads"] < c["kDistThreads"], count_block < c["kDistSumRows"], count_block < c["kDistRowLanes"]):
        bins, vals, r = differs(first)
        assert bins and vals and r["m"] != full["m"]


# ------------------------------------------------------------------------------------------------ 5. the threshold
@pytest.mark.parametrize("t2", [0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-18, 1.2345678e-12, 1.0, 2.0, 1e300, 1.7e308,
                                np.nextafter(1e-12, 1.0), np.nextafter(1e-12, 0.0)])
def test_threshold_of_tot_is_the_largest_double_whose_square_does_not_exceed(t2):
    thr = sit.percentile_threshold("tot", t2)
    assert math.isfinite(thr) and thr >= 0.
    assert np.float64(thr) * np.float64(thr) <= t2
    up = math.nextafter(thr, math.inf)
    assert np.float64(up) * np.float64(up) > t2
    if t2 > 1e-300:                                                    # away from the denormals it is sqrt or a neighbour
        assert abs(thr - math.sqrt(t2)) <= 2 * math.ulp(thr)


def test_threshold_of_the_other_rates_and_refusals():
    assert sit.percentile_threshold("div", -1.5e-7) == -1.5e-7 and sit.percentile_threshold("conv", 2e-7) == 2e-7
    z = sit.percentile_threshold("shr", -0.0)
    assert z == 0. and not math.copysign(1., z) < 0.
    for what, v in (("tot", -1e-9), ("tot", math.nan), ("div", math.inf), ("curl", 1.), ("tot", None)):
        with pytest.raises(ValueError):
            sit.percentile_threshold(what, v)


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_deform_pdf_flag_parser_and_its_refusals():
    base = ["-i", "a", "-m", "b", "-s", "c", "--deform", "10"]
    assert drv.parse_args(base).deform_pdf is None
    got = drv.parse_args(base + ["--deform-pdf", "tot@1e-9:1e-4:32,div@-1e-5:1e-5:20@lin"]).deform_pdf
    assert [g[0] for g in got] == ["tot", "div"]
    assert np.array_equal(got[0][1], sit.log_edges(1e-9, 1e-4, 32)) and np.array_equal(got[1][1], sit.lin_edges(-1e-5, 1e-5, 20))
    assert got[0][1].shape == (33,) and got[0][1][0] == 1e-9 and got[0][1][-1] == 1e-4
    for name in ("conv", "shr", "vor", "adiv", "avor"):
        assert drv.parse_args(base + ["--deform-pdf", name + "@1e-9:1e-4:8@log"]).deform_pdf[0][0] == name
    for bad in ("", "tot", "curl@1e-9:1e-4:8", "tot@1e-4:1e-9:8", "tot@1e-9:1e-9:8", "div@-1e-5:1e-5:8", "div@0:1e-5:8@log",
                "tot@1e-9:1e-4:0", "tot@1e-9:1e-4:1025", "tot@1e-9:1e-4:8@cube", "tot@1e-9:1e-4", "tot@1e-9:1e-4:8.5",
                "tot@1e-9:inf:8", "tot@nan:1e-4:8", "tot@1e-9:1e-4:8,tot@1e-9:1e-4:4", "tot@-1:1:8@lin"):
        with pytest.raises(SystemExit):
            drv.parse_args(base + ["--deform-pdf", bad])
    with pytest.raises(SystemExit):                                    # no mesh to take a distribution of
        drv.parse_args(["-i", "a", "-m", "b", "-s", "c", "--deform-pdf", "tot@1e-9:1e-4:8"])


def test_percentile_form_of_the_features_flag():
    both = ["-i", "a", "-m", "b", "-s", "c", "--deform", "10", "--deform-grid", "12.5"]
    # the numeric form parses to exactly the tuples it parsed to before
    assert drv.parse_args(both + ["--deform-features", "tot@1e-6"]).deform_features == ("tot", 1, 1e-6, 1, 8)
    assert drv.parse_args(both + ["--deform-features", "conv@2.5e-7@3"]).deform_features == ("div", -1, 2.5e-7, 3, 8)
    assert type(drv.parse_args(both + ["--deform-features", "div@-1e-7@2@4"]).deform_features[2]) is float
    f = drv.parse_args(both + ["--deform-features", "tot@p85"]).deform_features
    assert f == ("tot", 1, dst.Percentile(85.), 1, 8)
    assert drv.parse_args(both + ["--deform-features", "conv@p99.5@3@4"]).deform_features == ("div", -1, dst.Percentile(99.5), 3, 4)
    assert ft.features_arg("shr@p0") [2] == dst.Percentile(0.) and ft.features_arg("shr@p100")[2] == dst.Percentile(100.)
    with pytest.raises(ValueError, match=r"percentile of pNN must lie in \[0, 100\]"):       # the refusal names what is wrong
        ft.features_arg("tot@p101")
    with pytest.raises(ValueError, match="expected pNN"):
        ft.features_arg("tot@px")
    for bad in ("tot@p101", "tot@p-1", "tot@pNaN", "tot@pnan", "tot@p", "tot@px", "tot@P85", "tot@x", "tot@pinf", "tot@p85@0"):
        with pytest.raises(SystemExit):
            drv.parse_args(both + ["--deform-features", bad])
        with pytest.raises(ValueError):
            ft.features_arg(bad)
    # tracking and thinning take the percentile form as they take the numeric one
    a = drv.parse_args(both + ["--deform-features", "tot@p85", "--deform-track", "--deform-skeleton"])
    assert a.deform_track == 1 and a.deform_skeleton == ft.SKEL_DEFAULT_MAXSUB


# ------------------------------------------------------------------------------------------------ 7. edges, densities, the tail
def test_log_and_lin_edges():
    e = sit.log_edges(1e-9, 1e-4, 50)
    assert e.shape == (51,) and e[0] == 1e-9 and e[-1] == 1e-4 and (np.diff(e) > 0.).all()
    assert np.allclose(e[1:] / e[:-1], 10. ** 0.1, rtol=1e-12)
    l = sit.lin_edges(-1e-5, 1e-5, 20)
    assert l.shape == (21,) and l[0] == -1e-5 and l[-1] == 1e-5 and np.allclose(np.diff(l), 1e-6, rtol=1e-9)
    assert sit.log_edges(1., 2., 1).tolist() == [1., 2.] and sit.lin_edges(0., 1., 1024).shape == (1025,)
    for fn, args in ((sit.log_edges, (0., 1., 4)), (sit.log_edges, (-1., 1., 4)), (sit.log_edges, (2., 1., 4)), (sit.lin_edges, (1., 1., 4)),
                     (sit.lin_edges, (0., 1., 0)), (sit.lin_edges, (0., 1., 1025)), (sit.lin_edges, (0., math.inf, 4)),
                     (sit.log_edges, (1., 2., 2.5)), (sit.lin_edges, (0., math.nan, 4)), (sit.log_edges, ("a", 2., 2))):
        with pytest.raises(ValueError):
            fn(*args)


def test_pdf_from_counts():
    edges = np.array([0., 1., 3., 7.])
    counts = np.array([5, 10, 20, 10, 99], dtype=np.int64)
    p = sit.pdf_from_counts(counts, edges)
    assert np.array_equal(p, np.array([10. / 40., 20. / (40. * 2.), 10. / (40. * 4.)]))
    assert math.isclose(float((p * np.diff(edges)).sum()), 1.0, rel_tol=1e-15)
    assert np.isnan(sit.pdf_from_counts(np.array([3, 0, 0, 0, 4]), edges)).all()
    for bad in (np.array([1, 2, 3, 4]), np.array([1., 2., 3., 4., 5.]), np.array([1, -2, 3, 4, 5])):
        with pytest.raises(ValueError):
            sit.pdf_from_counts(bad, edges)


def test_tail_exponent_of_an_analytic_power_law():
    """A density p(x) = C x^-a between geometric edges of ratio r puts  N_c = K e_c^(1-a)  values into bin c, so the density of
    the bin, N_c / (N e_c (r - 1)), is proportional to e_c^-a and, at the geometric centre x_c = e_c sqrt(r), log p_c is
    -a log x_c + const EXACTLY: the fitted slope is -a up to the rounding of the counts to integers.  That rounding changes a
    count by at most 0.5, a relative error of at most d = 0.5 / (smallest count used), hence log p_c by at most -log(1 - d) (the
    common factor 1/N moves every point alike and leaves the slope alone).  A least-squares slope is sum((X_c - Xm) y_c) /
    sum((X_c - Xm)^2), so it moves by at most  -log(1 - d) * sum|X_c - Xm| / sum((X_c - Xm)^2) ; 1e-9 is added for the
    floating-point evaluation of logs and the fit."""
    a, nb = 2.4, 30
    edges = sit.log_edges(1e-8, 1e-5, nb)
    exact = 4e3 * (edges[:-1] / edges[-2]) ** (1. - a)                 # the smallest, the last, is 4000
    counts = np.concatenate([[7], np.rint(exact).astype(np.int64), [3]])
    lo = edges[4]
    t = sit.tail_exponent(counts, edges, lo, min_count=100)
    used = t["used"]
    assert used.sum() == nb - 4 and not used[:4].any()
    d = 0.5 / counts[1:-1][used].min()
    X = np.log(t["x"][used])
    tol = -math.log(1. - d) * np.abs(X - X.mean()).sum() / ((X - X.mean()) ** 2).sum() + 1e-9
    assert tol < 1e-4
    assert abs(t["slope"] + a) <= tol, (t["slope"], tol)
    # bins below lo or with too few values do not enter; fewer than two bins give NaN
    few = counts.copy(); few[10] = 50
    assert not sit.tail_exponent(few, edges, lo, min_count=100)["used"][9]
    assert math.isnan(sit.tail_exponent(counts, edges, edges[-2], min_count=100)["slope"])
    with pytest.raises(ValueError):
        sit.tail_exponent(counts, edges, 0.)
    # equidistant edges across 0 (what --deform-pdf div@-1e-5:1e-5:20@lin logs the tail of): no bin at or below 0 enters, and
    # nothing is computed for it -- no warning
    import warnings
    lin = sit.lin_edges(-1e-5, 1e-5, 20)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t = sit.tail_exponent(np.concatenate([[0], np.arange(500, 520), [0]]), lin, lin[11], min_count=1)
    assert not t["used"][:11].any() and t["used"][11:].all() and np.isnan(t["x"][:11]).all() and math.isfinite(t["slope"])


def test_value_distribution_refuses_bad_arguments_before_any_device_work():
    x = np.arange(5.)
    for kw in ({"edges": [0., 0.]}, {"edges": [1., 0.]}, {"edges": [0., math.inf]}, {"edges": [0.]}, {"edges": np.arange(1026.)},
               {"edges": [0., math.nan, 1.]}, {"q": [1.5]}, {"q": [-0.1]}, {"q": [math.nan]}, {"q": np.zeros(17)}, {"use": np.ones(4)}):
        with pytest.raises(ValueError):
            sit.ValueDistribution(x, **kw)
    with pytest.raises(ValueError):
        sit.ValueDistribution(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="ascending"):
        dst.square_edges([0., 1e-200, 2e-200])                         # both squares underflow to 0
    with pytest.raises(ValueError):
        dst.square_edges([-1., 1.])
    assert np.array_equal(dst.square_edges([0., 2., 3.]), [0., 4., 9.])
