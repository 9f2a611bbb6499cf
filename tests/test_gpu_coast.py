"""Distance to the model coastline on the GPU (sitrk_coast_*) against the numpy restatement of tests/test_coast.py.

Tolerances: segment ids and endpoints bit-equal; d2min bit-equal (only + - * /, compare and min take
part) -- recomputed from the returned segment, and dist*dist must bracket it; seg equal; dist within one ulp of numpy's sqrt;
+inf, NaN and -1 exact.  Every query of every case is compared."""
import importlib.util
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import ncio
from sitrack_amd import synthetic as syn

from test_coast import checkerboard, coast_segments_ref, coast_dist_ref, d2_ref, island_grid, messy_grid
from test_cloud_trips import COAST_BATCH, TRIP, coast_trip_grid, coast_trip_queries, coast_trip_segments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = sit.Context(0)
    yield c
    c.close()


def query_mix(g, ab, n, seed=11):
    """n queries: random in the box; 64 at 10x the domain's size outside it on all sides; on vertices; on segment interiors;
    every T-point (at warp 0 the centre of a lake or of a channel is equally far from two or four shores: exact ties) and
    points on the diagonals off segment ends; two with a NaN / inf coordinate"""
    rng = np.random.default_rng(seed)
    y0, y1, x0, x1 = g["Yf"].min(), g["Yf"].max(), g["Xf"].min(), g["Xf"].max()
    L = 10. * max(y1 - y0, x1 - x0)
    far = np.stack([rng.uniform(y0, y1, 64), rng.uniform(x0, x1, 64)], axis=1)
    far[0:16, 0] += L; far[16:32, 0] -= L; far[32:48, 1] += L; far[48:64, 1] -= L
    parts = [far, np.array([[np.nan, 0.], [0., np.inf]])]
    if len(ab):
        k = rng.integers(0, len(ab), 200)
        parts.append(ab[k, rng.integers(0, 2, 200)])                                   # vertices
        t = rng.integers(1, 8, 200)[:, None] / 8.
        parts.append(ab[k, 0] + t * (ab[k, 1] - ab[k, 0]))                              # interiors
        s = rng.choice([-3., 3., -5., 5.], (200, 2))
        parts.append(ab[k, 1] + s)                                                      # diagonals off the ends
    tp = np.stack([g["Yt"].ravel(), g["Xt"].ravel()], axis=1)
    parts.append(tp[:min(len(tp), 700)])
    m = n - sum(len(p) for p in parts)
    assert m > 0
    parts.insert(0, np.stack([rng.uniform(y0, y1, m), rng.uniform(x0, x1, m)], axis=1))
    return np.ascontiguousarray(np.concatenate(parts))


def pair_d2(yx, ab):
    """the contract's d2 of point k to segment k"""
    ey = ab[:, 1, 0] - ab[:, 0, 0]; ex = ab[:, 1, 1] - ab[:, 0, 1]
    py = yx[:, 0] - ab[:, 0, 0]; px = yx[:, 1] - ab[:, 0, 1]
    len2 = ey * ey + ex * ex
    dot = py * ey + px * ex
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(len2 > 0., dot / len2, 0.)
    t = np.where(t < 0., 0., np.where(t > 1., 1., t))
    cy = py - t * ey; cx = px - t * ex
    return cy * cy + cx * cx


def check_against(dist, seg, yx, ids, ab, rmax=None, label="", batch=512):
    """every query against the brute force over all segments"""
    d2r, segr, distr = coast_dist_ref(yx, ids, ab, rmax, batch=batch)
    assert seg.dtype == np.int32 and dist.dtype == np.float64
    assert np.array_equal(seg, segr), (label, np.flatnonzero(seg != segr)[:5])
    fin = segr >= 0
    assert np.array_equal(np.isposinf(dist), np.isposinf(distr)) and np.array_equal(np.isnan(dist), np.isnan(distr)), label
    assert np.all(np.isfinite(dist[fin])) and np.all(np.isposinf(dist[~fin]) | np.isnan(dist[~fin]))
    if fin.any():
        # d2 of the reported segment is the brute-force minimum, bit for bit ...
        d2 = pair_d2(yx[fin], ab[np.searchsorted(ids, seg[fin])])
        assert np.array_equal(d2, d2r[fin]), label
        # ... and the reported distance is its square root: within one ulp of numpy's, its neighbours' squares bracket d2
        d = dist[fin]
        ulp = np.spacing(distr[fin])
        ndiff = int((d != distr[fin]).sum())
        print("%s: %d queries, %d finite, dist differs from numpy's sqrt in %d" % (label, len(yx), int(fin.sum()), ndiff))
        assert np.all(np.abs(d - distr[fin]) <= ulp), label
        lo, hi = np.nextafter(d, 0.), np.nextafter(d, np.inf)
        assert np.all(lo * lo <= d2) and np.all(d2 <= hi * hi), label
    return d2r, segr


def build_and_check_segments(ctx, g):
    ids_r, ab_r, nd_r = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    nseg, nd = ctx.coast_build(g["Yf"], g["Xf"], g["tmask"])
    ids, ab = ctx.coast_segments()
    assert (nseg, nd) == (len(ids_r), nd_r)
    assert ids.dtype == np.int32 and np.array_equal(ids, ids_r) and np.array_equal(ab, ab_r)
    return ids_r, ab_r


# --------------------------------------------------------------------------- 1. segments
@pytest.mark.parametrize("warp", [0., 0.8])
def test_segments_match_the_restatement_whichever_way_the_grid_comes_in(ctx, warp):
    g = messy_grid(warp)
    ids_r, ab_r = build_and_check_segments(ctx, g)
    assert len(ids_r) > 60
    yx = query_mix(g, ab_r, 2000)
    dist, seg = ctx.coast_dist(yx)
    # the grid of set_grid, NULL pointers: the same bytes
    c2 = sit.Context(0)
    try:
        with pytest.raises(sit.SitrkError, match="no grid"):
            c2.coast_build()
        c2.set_grid(g["Yf"], g["Xf"], g["Yu"], g["Xu"], g["Yv"], g["Xv"], g["tmask"])
        assert c2.coast_build() == (len(ids_r), 0)
        ids2, ab2 = c2.coast_segments()
        assert ids2.tobytes() == ids_r.tobytes() and ab2.tobytes() == ab_r.tobytes()
        dist2, seg2 = c2.coast_dist(yx)
        assert dist2.tobytes() == dist.tobytes() and seg2.tobytes() == seg.tobytes()
        # a new grid drops the index that was built from the old one
        c2.set_grid(g["Yf"], g["Xf"], g["Yu"], g["Xu"], g["Yv"], g["Xv"], g["tmask"])
        with pytest.raises(sit.SitrkError, match="no coast index"):
            c2.coast_dist(yx)
    finally:
        c2.close()


def test_a_nan_f_point_drops_exactly_its_coast_segments(ctx):
    g = messy_grid(0.8)
    Yf = g["Yf"].copy()
    Yf[12, 15] = np.nan                                        # north-east vertex of the island: two coast segments end there
    ids_r, ab_r, nd_r = coast_segments_ref(Yf, g["Xf"], g["tmask"])
    ids_full, _, _ = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    assert nd_r == 2 and len(ids_r) == len(ids_full) - 2
    assert ctx.coast_build(Yf, g["Xf"], g["tmask"]) == (len(ids_r), 2)
    ids, ab = ctx.coast_segments()
    assert np.array_equal(ids, ids_r) and np.array_equal(ab, ab_r)
    yx = query_mix(g, ab_r, 2000)
    check_against(*ctx.coast_dist(yx), yx, ids_r, ab_r, label="nan F-point")


def test_calls_without_an_index_are_refused():
    c = sit.Context(0)
    try:
        for call in (lambda: c.coast_dist(np.zeros((3, 2))), c.coast_segments, c.coast_dist_buoys):
            with pytest.raises(sit.SitrkError):
                call()
        with pytest.raises(sit.SitrkError):
            c.set_tuning(coast_bin=0)
        with pytest.raises(sit.SitrkError):
            c.set_tuning(coast_bin=65)
    finally:
        c.close()


# --------------------------------------------------------------------------- 2. mixed coast
@pytest.mark.parametrize("warp", [0., 0.8])
def test_distances_mixed_coast(ctx, warp):
    g = messy_grid(warp)
    ids, ab = build_and_check_segments(ctx, g)
    yx = query_mix(g, ab, 4096)
    dist, seg = ctx.coast_dist(yx)
    d2r, segr = check_against(dist, seg, yx, ids, ab, label="mixed warp %g" % warp)
    if warp == 0.:
        d2all = d2_ref(yx[np.isfinite(yx).all(axis=1)][:3000], ab)
        assert ((d2all == d2all.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() > 100       # the mix does hold exact ties
    # seg is optional, n == 0 is valid, DistToCoast is the same call
    d_only, none = ctx.coast_dist(yx, want_seg=False)
    assert none is None and d_only.tobytes() == dist.tobytes()
    assert len(ctx.coast_dist(np.zeros((0, 2)))[0]) == 0
    assert sit.DistToCoast(yx, ctx=ctx).tobytes() == dist.tobytes()
    assert ctx.coast_kernel_ms() > 0.


# --------------------------------------------------------------------------- 3. sparse coast
def test_sparse_coast_one_land_cell_and_a_single_segment(ctx):
    g = syn.make_grid(96, 128, dkm=4., warp=0.6, rim=0)
    g["tmask"][40, 70] = 0
    ids, ab = build_and_check_segments(ctx, g)
    assert len(ids) == 4
    yx = query_mix(g, ab, 4096)
    check_against(*ctx.coast_dist(yx), yx, ids, ab, label="one land cell")
    check_against(*ctx.coast_dist(yx, 25.), yx, ids, ab, rmax=25., label="one land cell, rmax 25")
    g["tmask"][:] = 1
    g["tmask"][0, 1] = 0                                       # on the rim: only its edge towards T(1,1) is a coast
    ids, ab = build_and_check_segments(ctx, g)
    assert list(ids) == [3]
    check_against(*ctx.coast_dist(yx), yx, ids, ab, label="single segment")


@pytest.mark.parametrize("value", [0, 1])
def test_no_coast(ctx, value):
    g = syn.make_grid(24, 28, dkm=4., warp=0.5, rim=0)
    g["tmask"][:] = value
    assert ctx.coast_build(g["Yf"], g["Xf"], g["tmask"]) == (0, 0)
    ids, ab = ctx.coast_segments()
    assert len(ids) == 0 and ab.shape == (0, 2, 2)
    yx = query_mix(g, ab, 1000)
    yx = yx[np.isfinite(yx).all(axis=1)]
    for rmax in (None, 12.):
        dist, seg = ctx.coast_dist(yx, rmax)
        assert np.all(np.isposinf(dist)) and np.all(seg == -1)


# --------------------------------------------------------------------------- 4. dense coast
def test_dense_coast_checkerboard(ctx):
    g = syn.make_grid(24, 28, dkm=4., warp=0.8, rim=0)
    g["tmask"][:] = checkerboard(24, 28)
    ids, ab = build_and_check_segments(ctx, g)
    assert len(ids) == 23 * 27 * 2                              # every interior edge
    yx = query_mix(g, ab, 4096)
    check_against(*ctx.coast_dist(yx), yx, ids, ab, label="checkerboard")


def test_mid_size_random_coast(ctx):
    """about 28 000 segments: more than 100 workgroups, thousands of bins, a sort that moves every segment"""
    g = syn.make_grid(160, 176, dkm=4., warp=0.8, rim=0)
    g["tmask"][:] = (np.random.default_rng(31).random((160, 176)) >= 0.5).astype(np.int8)
    ids, ab = build_and_check_segments(ctx, g)
    assert 100 * 256 < len(ids) < 2 * 159 * 175
    yx = query_mix(g, ab, 2048)[2::4]                           # 512 of every kind the mix holds
    assert len(yx) == 512 and not np.isfinite(yx).all()
    check_against(*ctx.coast_dist(yx), yx, ids, ab, label="random coast", batch=64)
    d, s = ctx.coast_dist(yx, 12.)                              # three cells
    check_against(d, s, yx, ids, ab, rmax=12., label="random coast, rmax 12", batch=64)
    assert 25 < (s >= 0).sum() < 500


def test_coast_past_one_trip_of_the_stats_kernel(ctx):
    """more segments than one trip of coast_stats_kernel's capped grid, the longest of them known to the second trip alone: `pad`,
    and with it every query's search radius, depends on it (tests/test_cloud_trips.py checks what the input holds)"""
    Yf, Xf, tmask = coast_trip_grid()
    ids_r, ab_r, nd_r = coast_trip_segments()
    assert len(ids_r) > TRIP
    assert ctx.coast_build(Yf, Xf, tmask) == (len(ids_r), nd_r)
    ids, ab = ctx.coast_segments()
    assert ids.dtype == np.int32 and np.array_equal(ids, ids_r) and np.array_equal(ab, ab_r)
    yx, designed, dense = coast_trip_queries()
    assert len(yx) <= 128
    dist, seg = ctx.coast_dist(yx)
    d2r, segr = check_against(dist, seg, yx, ids_r, ab_r, label="past one trip", batch=COAST_BATCH)
    assert (np.searchsorted(ids_r, seg[designed]) >= TRIP).all() and (np.searchsorted(ids_r, seg[dense]) < TRIP).all()


# --------------------------------------------------------------------------- 5. long segments
def test_long_segments(ctx):
    g = messy_grid(0.8)
    for k in ("Yf", "Yt"):
        g[k] = g[k] * 0.25                                      # cells of 1 km x 40 km
    for k in ("Xf", "Xt"):
        g[k] = g[k] * 10.
    ids, ab = build_and_check_segments(ctx, g)
    e = ab[:, 1] - ab[:, 0]
    assert np.hypot(e[:, 0], e[:, 1]).max() > 35. and np.hypot(e[:, 0], e[:, 1]).min() < 1.5
    yx = query_mix(g, ab, 4096)
    check_against(*ctx.coast_dist(yx), yx, ids, ab, label="long segments")
    check_against(*ctx.coast_dist(yx, 3.), yx, ids, ab, rmax=3., label="long segments, rmax 3")


# --------------------------------------------------------------------------- 6. rmax
def test_rmax(ctx):
    g = island_grid()
    ids, ab = build_and_check_segments(ctx, g)
    east_mid = 2 * (11 * 28 + 15)
    hand = np.array([[-2., 20.], [-2., np.nextafter(20., 30.)], [-2., 19.], [4., 8.], [7., 11.]])
    dist, seg = ctx.coast_dist(hand, 12.)
    assert dist[0] == 12. and seg[0] == east_mid                # exactly at the radius: the answer stays
    assert np.isposinf(dist[1]) and seg[1] == -1
    assert dist[2] == 11. and dist[3] == 0. and seg[3] == 2 * (12 * 28 + 15) and seg[4] == 2 * (12 * 28 + 15)
    yx = np.concatenate([hand, query_mix(g, ab, 4000)])
    d_all, s_all = ctx.coast_dist(yx)
    check_against(d_all, s_all, yx, ids, ab, label="island, unbounded")
    for rmax in (12., np.nextafter(12., 0.), 1e-3, 1e6):
        d, s = ctx.coast_dist(yx, rmax)
        check_against(d, s, yx, ids, ab, rmax=rmax, label="island, rmax %r" % rmax)
        within = s >= 0
        assert d[within].tobytes() == d_all[within].tobytes() and np.array_equal(s[within], s_all[within])
    for unbounded in (0., -3., np.inf, None):
        d, s = ctx.coast_dist(yx, unbounded)
        assert d.tobytes() == d_all.tobytes() and s.tobytes() == s_all.tobytes()
    with pytest.raises(sit.SitrkError, match="NaN"):
        ctx.coast_dist(yx, float("nan"))


# --------------------------------------------------------------------------- 7. knob
def test_results_do_not_depend_on_the_bin_knob(ctx):
    g = messy_grid(0.8)
    ids_r, ab_r, _ = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    yx = query_mix(g, ab_r, 4096)
    outs = []
    try:
        for v in (1, 7, 64):
            ctx.set_tuning(coast_bin=v)
            ctx.coast_build(g["Yf"], g["Xf"], g["tmask"])
            outs.append([ctx.coast_dist(yx), ctx.coast_dist(yx, 9.)])
    finally:
        ctx.set_tuning(coast_bin=4)
    check_against(*outs[0][0], yx, ids_r, ab_r, label="coast_bin 1")
    check_against(*outs[0][1], yx, ids_r, ab_r, rmax=9., label="coast_bin 1, rmax 9")
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# --------------------------------------------------------------------------- 8. buoy state
def test_buoy_state_queries_leave_the_tracker_alone():
    g = syn.make_grid(64, 64, dkm=4.0, warp=1.0)
    g["tmask"][30:34, 20:27] = 0
    u, v, sic = syn.make_fields(g, K=4, seed=2024, umax=0.75, drift=0.25, ripple=0.12)
    _, yx = syn.make_buoys(g, 2000, seed=1234, frac=0.7)
    ids_r, ab_r, _ = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    states = []
    for ask in (True, False):
        trk = sit.IceTracker(g["Yf"], g["Xf"], g["Yu"], g["Xu"], g["Yv"], g["Xv"], g["tmask"], nslots=4)
        try:
            if ask:
                with pytest.raises(sit.SitrkError, match="no buoys"):
                    trk.dist2coast()
            found, ji, _ = sit.FindContainingCell(yx, syn.nearest_t_plane(g, yx), ctx=trk.ctx)
            trk.set_buoys(yx[found], ji[found])
            for k in range(4):
                trk.load_record(k, u[k], v[k], sic[k])
            for jrec in range(5):
                trk.step(jrec, jrec % 4)
                if jrec == 2:
                    trk.ctx.sort_buoys()
            if ask:
                before = trk.ctx.fetch()
                dist, seg = trk.dist2coast(return_seg=True)
                after = trk.ctx.fetch()
                for k in before:
                    assert before[k].tobytes() == after[k].tobytes(), k
                assert (before["alive"] == 0).any()             # dead buoys are answered too
                d_host, s_host = trk.ctx.coast_dist(before["yx"])
                assert dist.tobytes() == d_host.tobytes() and seg.tobytes() == s_host.tobytes()
                check_against(dist, seg, before["yx"], ids_r, ab_r, label="buoy state")
                check_against(*trk.dist2coast(rmax_km=12., return_seg=True), before["yx"], ids_r, ab_r, rmax=12., label="buoy state, rmax 12")
            for jrec in range(5, 10):
                trk.step(jrec, jrec % 4)
            states.append((trk.ctx.fetch(), trk.record(9)))
        finally:
            trk.close()
    (a, ra), (b, rb) = states
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes()


# --------------------------------------------------------------------------- 9. seeding tool
def _gis():
    spec = importlib.util.spec_from_file_location("gis_coast_gpu", os.path.join(ROOT, "tools", "generate_idealized_seeding.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_seeding_tool_min_dist_land_end_to_end(tmp_path, monkeypatch, capsys):
    from test_driver import make_case
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), dkm=4.0)
    gis = _gis()
    base = ["-d", "1996-12-15_00:00:00", "-m", c["mm"], "-i", c["si3"], "-k", "0", "-N", "TEST4"]
    f = gis.main(base + ["--min-dist-land", "30"])
    assert f == './nc/sitrack_seeding_nemoTsi3_19961215_00_dl30km.nc'
    # the seeds of the same inputs, and which of them the restatement keeps
    dctx = sit.default_context()
    imaskt, latT, lonT, _, _, Yf, Xf, _ = ncio.GetModelGrid(c["mm"])
    rec = ncio.ModelRecords(c["si3"])
    (ic,) = rec.fields(0, ("siconc",))
    rec.close()
    gc_all, yx_all = sit.seeding.nemoSeed(imaskt, latT, lonT, ic, ctx=dctx, return_yx=True)
    ids_r, ab_r, _ = coast_segments_ref(Yf, Xf, imaskt)
    d2r, _, _ = coast_dist_ref(yx_all, ids_r, ab_r)
    keep = d2r >= 900.
    assert 50 < keep.sum() < len(keep) - 50
    assert " * Need to remove %d points because too close to land! (30.0km)" % (~keep).sum() in capsys.readouterr().out
    _, ids, ll, yx = ncio.LoadNCdata(f, krec=0)
    ids = np.asarray(ids).astype(np.int64)
    assert np.array_equal(ids, np.flatnonzero(keep) + 1)         # exactly those, under their own IDs
    fall = './nc/all.nc'
    ncio.ncSaveCloudBuoys(fall, np.array([c["base"]], dtype='i4'), np.arange(1, len(gc_all) + 1), yx_all[None, :, 0], yx_all[None, :, 1],
                          gc_all[None, :, 0], gc_all[None, :, 1], corigin='idealized_seeding', cauthor='test')
    _, _, ll0, yx0 = ncio.LoadNCdata(fall, krec=0)
    assert np.array_equal(ll, ll0[ids - 1]) and np.array_equal(yx, yx0[ids - 1])
    # with -C 40 the coarsening sees only the kept seeds
    f40 = gis.main(base + ["--min-dist-land", "30", "-C", "40"])
    assert f40 == './nc/sitrack_seeding_nemoTsi3_19961215_00_40km_dl30km.nc'
    _, _, idx = sit.SubSampCloud(34.5, yx_all[keep], ctx=dctx)
    _, ids40, _, _ = ncio.LoadNCdata(f40, krec=0)
    assert 1 < len(idx) < keep.sum()
    assert np.array_equal(np.asarray(ids40).astype(np.int64), (np.flatnonzero(keep) + 1)[idx])
    # MaskCoastal on the seeds' lat/lon is the tool's rule
    dctx.coast_build(Yf, Xf, imaskt)
    assert np.array_equal(sit.MaskCoastal(gc_all, 30., ctx=dctx), keep.astype(np.int8))
