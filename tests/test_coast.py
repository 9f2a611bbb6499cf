"""Distance to the model coastline, CPU side: the numpy restatement of the contract of include/sitrk.h (coast segments, the
distance expression, ties, rmax) that tests/test_gpu_coast.py holds the library to, hand-checkable values of it, the
MaskCoastal rule, the C ABI's new symbols and the seeding tool's `--min-dist-land`."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, coast
from sitrack_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COAST_SYMBOLS = ["sitrk_coast_build", "sitrk_coast_segments", "sitrk_coast_dist", "sitrk_coast_dist_buoys", "sitrk_coast_kernel_ms"]


# --------------------------------------------------------------------------- the restatement
def coast_segments_ref(Yf, Xf, tmask):
    """(ids (n,) int32, ab (n,2,2) = [a|b][y,x], ndropped): the coast segments of include/sitrk.h in id order, one edge at a
    time as the header words it."""
    Nj, Ni = tmask.shape
    ids, ab, ndropped = [], [], 0
    for j in range(Nj):
        for i in range(Ni):
            for k in (0, 1):
                if k == 0:
                    if not (j >= 1 and i + 1 < Ni):
                        continue
                    other, a = (j, i + 1), (j - 1, i)
                else:
                    if not (i >= 1 and j + 1 < Nj):
                        continue
                    other, a = (j + 1, i), (j, i - 1)
                if (tmask[j, i] == 0) == (tmask[other] == 0):
                    continue
                seg = [[Yf[a], Xf[a]], [Yf[j, i], Xf[j, i]]]
                if not np.all(np.isfinite(seg)):
                    ndropped += 1
                    continue
                ids.append(2 * (j * Ni + i) + k)
                ab.append(seg)
    return np.array(ids, dtype=np.int32), np.array(ab, dtype=np.float64).reshape(-1, 2, 2), ndropped


def coast_segments_vec(Yf, Xf, tmask):
    """coast_segments_ref in whole-array numpy, for coasts too long for the loop: the same three values.  The loop form stays the
    statement of the contract; this one is trusted only through test_vectorised_segments_equal_the_loop_form."""
    Yf, Xf = np.asarray(Yf, dtype=np.float64), np.asarray(Xf, dtype=np.float64)
    land = np.asarray(tmask) == 0
    Nj, Ni = land.shape
    coast = [np.zeros((Nj, Ni), dtype=bool), np.zeros((Nj, Ni), dtype=bool)]
    coast[0][1:, :-1] = land[1:, :-1] != land[1:, 1:]         # k = 0: T(j,i) | T(j,i+1), j >= 1, from F(j-1,i)
    coast[1][:-1, 1:] = land[:-1, 1:] != land[1:, 1:]         # k = 1: T(j,i) | T(j+1,i), i >= 1, from F(j,i-1)
    ids, ab = [], []
    for k, (dj, di) in enumerate(((1, 0), (0, 1))):
        j, i = np.nonzero(coast[k])
        ids.append(2 * (j * Ni + i) + k)
        ab.append(np.stack([Yf[j - dj, i - di], Xf[j - dj, i - di], Yf[j, i], Xf[j, i]], axis=1).reshape(-1, 2, 2))
    ids, ab = np.concatenate(ids), np.concatenate(ab)
    fin = np.isfinite(ab).all(axis=(1, 2))
    order = np.argsort(ids[fin], kind="stable")
    return ids[fin][order].astype(np.int32), np.ascontiguousarray(ab[fin][order]), int((~fin).sum())


def d2_ref(yx, ab):
    """d2 of every point (n,2) to every segment (m,2,2) -> (n,m): the contract's expression, one numpy operation per symbol
    (numpy rounds each once and fuses none)"""
    ya, xa, yb, xb = (ab[None, :, 0, 0], ab[None, :, 0, 1], ab[None, :, 1, 0], ab[None, :, 1, 1])
    yp, xp = yx[:, 0, None], yx[:, 1, None]
    ey = yb - ya; ex = xb - xa; py = yp - ya; px = xp - xa
    len2 = ey * ey + ex * ex
    dot = py * ey + px * ex
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(len2 > 0., dot / len2, 0.)
    t = np.where(t < 0., 0., np.where(t > 1., 1., t))
    cy = py - t * ey; cx = px - t * ex
    return cy * cy + cx * cx


def coast_dist_ref(yx, ids, ab, rmax=None, batch=512):
    """(d2min, seg, dist) by brute force over ALL segments: the minimum, the lowest id that attains it (ids ascend, argmin takes
    the first), its numpy sqrt; rmax, no coast and non-finite queries as the header states them.  `batch` queries at a time: one
    temporary is batch x len(ids) doubles."""
    yx = np.asarray(yx, dtype=np.float64)
    n = len(yx)
    d2min = np.full(n, np.inf); seg = np.full(n, -1, dtype=np.int32)
    if len(ids) == 0:
        return d2min, seg, d2min.copy()
    ok = np.isfinite(yx).all(axis=1)
    d2min[~ok] = np.nan
    for b in range(0, n, batch):
        sl = np.flatnonzero(ok[b:b + batch]) + b
        if len(sl) == 0:
            continue
        d2 = d2_ref(yx[sl], ab)
        k = np.argmin(d2, axis=1)
        d2min[sl] = d2[np.arange(len(sl)), k]
        seg[sl] = ids[k]
    if rmax is not None and np.isfinite(rmax) and rmax > 0.:
        far = ok & (d2min > rmax * rmax)
        d2min[far] = np.inf; seg[far] = -1
    return d2min, seg, np.sqrt(d2min)


def island_grid(Nj=24, Ni=28, dkm=4., warp=0.):
    """all sea but the 3 x 4-cell island T(10..12, 12..15); at warp 0, F(j,i) = (4 (j - 11), 4 (i - 13)) km exactly"""
    g = syn.make_grid(Nj, Ni, dkm=dkm, warp=warp, rim=0)
    g["tmask"][10:13, 12:16] = 0
    return g


def messy_grid(warp):
    """24 x 28: an island, a one-cell island, land with a one-cell lake, a peninsula that reaches the rim, land along one rim row"""
    g = syn.make_grid(24, 28, dkm=4., warp=warp, rim=0)
    t = g["tmask"]
    t[10:13, 12:16] = 0
    t[4, 5] = 0
    t[16:21, 18:24] = 0; t[18, 20] = 1
    t[6:9, 0:6] = 0
    t[-1, :] = 0
    return g


def checkerboard(Nj, Ni):
    jj, ii = np.indices((Nj, Ni))
    return ((jj + ii) % 2).astype(np.int8)


# --------------------------------------------------------------------------- the restatement on hand-checkable values
def test_segments_of_the_island_by_hand():
    g = island_grid()
    ids, ab, nd = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    assert nd == 0 and len(ids) == 2 * (3 + 4) and np.all(np.diff(ids) > 0)
    # east shore of the middle row: T(11,15) | T(11,16), k = 0, from F(10,15) = (-4, 8) to F(11,15) = (0, 8)
    k = list(ids).index(2 * (11 * 28 + 15))
    assert np.array_equal(ab[k], [[-4., 8.], [0., 8.]])
    # north shore above T(12,13): T(12,13) | T(13,13), k = 1, from F(12,12) = (4, -4) to F(12,13) = (4, 0)
    k = list(ids).index(2 * (12 * 28 + 13) + 1)
    assert np.array_equal(ab[k], [[4., -4.], [4., 0.]])
    # the west shore belongs to the SEA cell T(j,11) (the edge is named after its lower-index cell)
    assert 2 * (11 * 28 + 11) in ids and 2 * (9 * 28 + 13) + 1 in ids
    # the vectorised count: every unlike pair of neighbours inside the domain
    land = g["tmask"] == 0
    assert len(ids) == (land[1:, :-1] != land[1:, 1:]).sum() + (land[:-1, 1:] != land[1:, 1:]).sum()


def test_rim_is_no_coast_and_row_zero_has_no_k0_edges():
    g = syn.make_grid(8, 9, dkm=4., warp=0., rim=0)
    g["tmask"][0, :] = 0                                       # land along one rim row
    ids, ab, _ = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    assert list(ids) == [2 * i + 1 for i in range(1, 9)]       # only the edges between row 0 and row 1, for i >= 1
    g["tmask"][:] = 0
    assert len(coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])[0]) == 0
    g["tmask"][:] = 1
    assert len(coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])[0]) == 0


def test_vectorised_segments_equal_the_loop_form():
    cases = []
    for warp in (0., 0.8):
        g = messy_grid(warp)
        cases.append((g["Yf"], g["Xf"], g["tmask"]))
    g = syn.make_grid(24, 28, dkm=4., warp=0.8, rim=0)
    cases.append((g["Yf"], g["Xf"], checkerboard(24, 28)))
    g = messy_grid(0.8)
    Yf = g["Yf"].copy()
    Yf[12, 15] = np.nan                                        # the case of the GPU test: two coast segments end there
    cases.append((Yf, g["Xf"], g["tmask"]))
    for seed, (Nj, Ni, warp, p) in enumerate([(17, 23, 0.8, 0.5), (30, 9, 0.3, 0.2), (2, 2, 0., 0.5), (2, 40, 1.0, 0.5), (33, 2, 0.6, 0.7)]):
        rng = np.random.default_rng(40 + seed)
        g = syn.make_grid(Nj, Ni, dkm=4., warp=warp, rim=0)
        Yf, Xf = g["Yf"].copy(), g["Xf"].copy()
        if seed % 2:                                           # a few F-points without a position, NaN or inf, in either array
            Yf.flat[rng.choice(Nj * Ni, 3, replace=False)] = np.nan
            Xf.flat[rng.choice(Nj * Ni, 3, replace=False)] = np.inf
        cases.append((Yf, Xf, (rng.random((Nj, Ni)) >= p).astype(np.int8)))
    dropped = 0
    for Yf, Xf, tmask in cases:
        ids, ab, nd = coast_segments_ref(Yf, Xf, tmask)
        ids_v, ab_v, nd_v = coast_segments_vec(Yf, Xf, tmask)
        assert ids_v.dtype == np.int32 and ab_v.dtype == np.float64 and ab_v.shape == (len(ids), 2, 2)
        assert np.array_equal(ids_v, ids) and np.array_equal(ab_v, ab) and nd_v == nd
        dropped += nd
    assert dropped >= 4


def test_batched_brute_force_is_the_same_brute_force():
    g = messy_grid(0.8)
    ids, ab, _ = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    rng = np.random.default_rng(3)
    yx = np.stack([rng.uniform(g["Yf"].min(), g["Yf"].max(), 700), rng.uniform(g["Xf"].min(), g["Xf"].max(), 700)], axis=1)
    yx[[5, 640]] = [[np.nan, 0.], [0., np.inf]]
    for rmax in (None, 9.):
        want = coast_dist_ref(yx, ids, ab, rmax)
        for batch in (1000, 32, 7):
            got = coast_dist_ref(yx, ids, ab, rmax, batch=batch)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_distances_by_hand():
    g = island_grid()
    ids, ab, _ = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    east_mid = 2 * (11 * 28 + 15)
    q = np.array([[-2., 20.],        # three cells east of the middle of the east shore
                  [4., 8.],          # on the island's north-east vertex F(12,15)
                  [7., 11.],         # on the diagonal off that vertex: as far from the east shore as from the north shore
                  [np.nan, 0.], [0., np.inf]])
    d2, seg, dist = coast_dist_ref(q, ids, ab)
    assert d2[0] == 144. and dist[0] == 12. and seg[0] == east_mid
    east_top, north_east = 2 * (12 * 28 + 15), 2 * (12 * 28 + 15) + 1
    assert d2[1] == 0. and seg[1] == east_top
    both = d2_ref(q[2:3], ab[[list(ids).index(east_top), list(ids).index(north_east)]])[0]
    assert both[0] == both[1] == 18. == d2[2] and seg[2] == east_top < north_east        # the lower id of the two
    assert np.isnan(dist[3]) and np.isnan(dist[4]) and seg[3] == seg[4] == -1
    # rmax: at exactly the radius the answer stays, beyond it +inf / -1
    d2r, segr, distr = coast_dist_ref(np.array([[-2., 20.], [-2., np.nextafter(20., 30.)], [-2., 19.]]), ids, ab, rmax=12.)
    assert distr[0] == 12. and segr[0] == east_mid and np.isposinf(distr[1]) and segr[1] == -1 and distr[2] == 11.
    # the library's host-side copy of the expression is the restatement
    k = np.searchsorted(ids, seg[:3])
    assert np.array_equal(coast.seg_d2(q[:3], ab[k]), d2[:3])


class _RefCtx:
    """stands in for a Context with a built index: answers from the restatement"""

    def __init__(self, g):
        self.ids, self.ab, _ = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])

    def coast_dist(self, yx, rmax_km=None, want_seg=True):
        _, seg, dist = coast_dist_ref(yx, self.ids, self.ab, rmax_km)
        return dist, seg

    def coast_segments(self):
        return self.ids, self.ab


def test_mask_coastal_rule_at_exactly_the_radius():
    ctx = _RefCtx(island_grid())
    yx = np.array([[-2., 20.], [-2., np.nextafter(20., 0.)], [-2., np.nextafter(20., 30.)], [-2., 8.], [40., 50.], [np.nan, 1.]])
    # d == r is kept (d2 >= r*r, decided on the squared distance), the next double inside is not; land itself and NaN go
    assert list(coast.mask_coastal_yx(yx, 12., ctx)) == [1, 0, 1, 0, 1, 0]
    assert coast.mask_coastal_yx(yx, 12., ctx).dtype == np.int8
    # a radius whose square rounds: 0.1 km off the shore against r = 0.1 (r*r = 0.010000000000000002 > the point's d2?)
    p = np.array([[-2., 8. + 0.1]])
    d2 = coast_dist_ref(p, ctx.ids, ctx.ab)[0][0]
    assert bool(coast.mask_coastal_yx(p, 0.1, ctx)[0]) == bool(d2 >= 0.1 * 0.1)
    for bad in (0., -5., float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sit.MaskCoastal(np.zeros((1, 2)), bad, ctx=ctx)
    assert len(coast.mask_coastal_yx(np.zeros((0, 2)), 5., ctx)) == 0


# --------------------------------------------------------------------------- C ABI
def test_coast_symbols_are_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(sitrk_[a-z0-9_]+)\s*\(", txt))
    assert set(COAST_SYMBOLS) <= declared, sorted(set(COAST_SYMBOLS) - declared)
    so = _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sitrk_[a-z0-9_]+)", out))
    assert set(COAST_SYMBOLS) <= exported, sorted(set(COAST_SYMBOLS) - exported)
    assert set(COAST_SYMBOLS) <= set(_lib._SIGNATURES)
    for name in ("coast_build", "coast_segments", "coast_dist", "coast_dist_buoys"):
        assert callable(getattr(sit.Context, name))
    assert callable(sit.DistToCoast) and callable(sit.MaskCoastal) and callable(sit.IceTracker.dist2coast)


# --------------------------------------------------------------------------- seeding tool
def _seeding_tool():
    spec = importlib.util.spec_from_file_location("gis_coast", os.path.join(ROOT, "tools", "generate_idealized_seeding.py"))
    gis = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gis)
    return gis


class _ReachedTheGpu(Exception):
    pass


def _no_gpu(*a, **k):
    raise _ReachedTheGpu()


@pytest.mark.parametrize("extra", [[], ["-C", "40"]])
def test_seeding_tool_accepts_min_dist_land(monkeypatch, extra):
    """the flag parses and passes the tool's own checks: the run gets as far as opening the GPU"""
    gis = _seeding_tool()
    monkeypatch.setattr(gis.sit, "Context", _no_gpu)
    with pytest.raises(_ReachedTheGpu):
        gis.main(["-d", "1996-12-15_00:00:00", "-m", "mesh_mask.nc", "--min-dist-land", "30"] + extra)


@pytest.mark.parametrize("km", ["0", "-5", "nan", "inf"])
def test_seeding_tool_refuses_a_bad_min_dist_land(monkeypatch, km):
    gis = _seeding_tool()
    monkeypatch.setattr(gis.sit, "Context", _no_gpu)
    with pytest.raises(SystemExit, match="min-dist-land.*finite distance > 0 km"):
        gis.main(["-d", "1996-12-15_00:00:00", "-m", "mesh_mask.nc", "--min-dist-land=" + km])


def test_seeding_tool_min_dist_land_needs_the_mesh_and_leaves_C640_refused(monkeypatch):
    gis = _seeding_tool()
    monkeypatch.setattr(gis.sit, "Context", _no_gpu)
    with pytest.raises(SystemExit, match="needs the MeshMask file"):
        gis.main(["-d", "1996-12-15_00:00:00", "--lsidfex", "1", "--min-dist-land", "30"])
    with pytest.raises(SystemExit, match="dist2coast_4deg_North.nc.*MaskCoastal"):
        gis.main(["-d", "1996-12-15_00:00:00", "-m", "mesh_mask.nc", "-C", "640", "--min-dist-land", "30"])
