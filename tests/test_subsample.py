"""Seed-cloud coarsening (SubSampCloud, sitrk_subsample_cloud), CPU side: the test-side statements of the contract and the
argument checks that come before any GPU work.  The GPU results are held against these in test_gpu_subsample.py.

Contract: d2(i,j) = (y_i-y_j)*(y_i-y_j) + (x_i-x_j)*(x_i-x_j) in fp64 (numpy does not fuse), r2 = rd*rd; point i is kept iff
no kept j < i has d2(i,j) < r2."""
import importlib.util
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

import sitrack_amd as sit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def d2(a, b):
    dy = a[..., 0] - b[..., 0]
    dx = a[..., 1] - b[..., 1]
    return dy * dy + dx * dx


def _pad(rd):
    return rd * (1.0 + 1e-9) + 1e-300      # cKDTree's own distance rounding must never hide a pair with d2 < r2


def greedy_reference(yx, rd):
    """The sequential greedy loop (gudhi's sparsify_point_set) restated: keep mask (bool)."""
    yx = np.asarray(yx, dtype=np.float64)
    n = len(yx)
    r2 = rd * rd
    keep = np.zeros(n, dtype=bool)
    dropped = np.zeros(n, dtype=bool)
    if n == 0:
        return keep
    tree = cKDTree(yx)
    for i in range(n):
        if dropped[i]:
            continue
        keep[i] = True
        nb = np.asarray(tree.query_ball_point(yx[i], _pad(rd)), dtype=np.int64)
        nb = nb[nb > i]
        dropped[nb[d2(yx[nb], yx[i]) < r2]] = True
    return keep


def characterisation_violations(yx, rd, keep):
    """O(n k) check that needs no sequential replay: keep is the greedy result iff
    (a) no two kept points have d2 < r2, and (b) every dropped point has a kept j < i with d2 < r2.
    Returns the number of points that break it (0 = correct)."""
    yx = np.asarray(yx, dtype=np.float64)
    keep = np.asarray(keep, dtype=bool)
    n = len(yx)
    if n == 0:
        return 0
    r2 = rd * rd
    ik = np.flatnonzero(keep)
    if len(ik) == 0:
        return n
    tk = cKDTree(yx[ik])
    bad = 0
    pairs = tk.query_pairs(_pad(rd), output_type='ndarray')
    if len(pairs):
        bad += int(np.count_nonzero(d2(yx[ik[pairs[:, 0]]], yx[ik[pairs[:, 1]]]) < r2))
    idrop = np.flatnonzero(~keep)
    if len(idrop):
        # kept points are >= rd apart: at most 7 of them lie within rd of any point
        kq = 12
        dist, loc = tk.query(yx[idrop], k=kq, distance_upper_bound=_pad(rd))
        assert np.all(np.isinf(dist[:, -1])), "more kept neighbours than a packing allows"
        valid = loc < len(ik)
        j = ik[np.where(valid, loc, 0)]
        ok = valid & (j < idrop[:, None]) & (d2(yx[j], yx[idrop][:, None, :]) < r2)
        bad += int(np.count_nonzero(~ok.any(axis=1)))
    return bad


def hand_cases():
    """(name, yx, rd, expected keep) -- the boundary cases of the contract"""
    cases = []
    cases.append(("exact d2 == r2: both kept", [[0., 0.], [3., 4.]], 5.0, [1, 1]))
    inside = [[0., 0.], [3., np.nextafter(4., 0.)]]
    assert d2(np.array(inside[1]), np.array(inside[0])) < 25.0
    cases.append(("one ulp inside: later dropped", inside, 5.0, [1, 0]))
    cases.append(("duplicates collapse to the first", [[1., 2.], [1., 2.], [7., 7.], [1., 2.]], 0.5, [1, 0, 1, 0]))
    cases.append(("n = 0", np.zeros((0, 2)), 1.0, []))
    cases.append(("n = 1", [[5., -3.]], 1.0, [1]))
    rng = np.random.default_rng(7)
    blob = rng.uniform(-10., 10., (50, 2))
    cases.append(("radius collapses all to point 0", blob, 100.0, [1] + [0] * 49))
    grid = np.stack(np.meshgrid(np.arange(10.) * 2.0, np.arange(10.) * 2.0, indexing="ij"), -1).reshape(-1, 2)
    cases.append(("radius below every spacing: nothing dropped", grid, 1.999, [1] * 100))
    cases.append(("chain: kept, dropped, kept", [[0., 0.], [1., 0.], [2., 0.], [3., 0.]], 1.5, [1, 0, 1, 0]))
    return cases


def fma_case(rd=6.0, seed=11, tries=200000):
    """A pair (0,0),(dy,dx) whose FMA-contracted d2 -- fma(dy,dy,dx*dx) or fma(dx,dx,dy*dy), each rounded once -- lies on
    the other side of r2 from the contract's d2.  Returns (yx, plain keep mask)."""
    from fractions import Fraction
    r2 = rd * rd
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        dy = float(rng.uniform(0.5, rd - 0.5))
        dx = float(np.sqrt(r2 - dy * dy))
        dx = float(np.nextafter(dx, 0.) if rng.random() < 0.5 else np.nextafter(dx, 10.))
        yy, xx = dy * dy, dx * dx
        plain = yy + xx
        f1 = float(Fraction(dy) * Fraction(dy) + Fraction(xx))
        f2 = float(Fraction(dx) * Fraction(dx) + Fraction(yy))
        for f in (f1, f2):
            if (plain < r2) != (f < r2):
                yx = np.array([[0., 0.], [dy, dx]])
                return yx, np.array([1, 0 if plain < r2 else 1], dtype=bool)
    raise AssertionError("no FMA-sensitive pair found")


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_greedy_statements_agree_on_hand_cases(case):
    _, yx, rd, want = case
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    want = np.asarray(want, dtype=bool)
    assert np.array_equal(greedy_reference(yx, rd), want)
    assert characterisation_violations(yx, rd, want) == 0


def test_characterisation_rejects_wrong_masks():
    rng = np.random.default_rng(3)
    yx = rng.uniform(0., 100., (3000, 2))
    k = greedy_reference(yx, 4.0)
    assert characterisation_violations(yx, 4.0, k) == 0
    for flip in (int(np.flatnonzero(k)[5]), int(np.flatnonzero(~k)[5])):
        w = k.copy()
        w[flip] = ~w[flip]
        assert characterisation_violations(yx, 4.0, w) > 0


def test_fma_case_is_found_and_stated():
    yx, want = fma_case()
    assert np.array_equal(greedy_reference(yx, 6.0), want)
    assert characterisation_violations(yx, 6.0, want) == 0


@pytest.mark.parametrize("seed,n,rd", [(1, 4000, 3.0), (2, 6000, 0.7), (3, 2000, 25.0)])
def test_greedy_statements_agree_on_random_clouds(seed, n, rd):
    rng = np.random.default_rng(seed)
    yx = rng.uniform(-50., 50., (n, 2))
    yx[::17] = yx[::17].round()                     # shared coordinate values and a few duplicates
    k = greedy_reference(yx, rd)
    assert 0 < k.sum() < n
    assert characterisation_violations(yx, rd, k) == 0


def test_subsampcloud_argument_checks_come_before_the_gpu(monkeypatch):
    from sitrack_amd import tracking

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(tracking, "default_context", no_gpu)
    pts = np.zeros((4, 2))
    for rd in (0., -1., 2000.5, float("nan")):
        with pytest.raises(ValueError, match="rd_km"):
            sit.SubSampCloud(rd, pts)
    with pytest.raises(ValueError, match="second dimension"):
        sit.SubSampCloud(10., np.zeros((4, 3)))
    with pytest.raises(ValueError, match="second dimension"):
        sit.SubSampCloud(10., np.zeros(4))


def _seeding_tool():
    spec = importlib.util.spec_from_file_location("gis_crsn", os.path.join(ROOT, "tools", "generate_idealized_seeding.py"))
    gis = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gis)
    return gis


@pytest.mark.parametrize("crsn,msg", [(640, "dist2coast_4deg_North.nc.*MaskCoastal"), (15, "do not know what `rd_ss` to pick")])
def test_seeding_tool_refuses_what_it_cannot_coarsen(monkeypatch, crsn, msg):
    gis = _seeding_tool()

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(gis.sit, "Context", no_gpu)
    with pytest.raises(SystemExit, match=msg):
        gis.main(["-d", "1996-12-15_00:00:00", "-m", "mesh_mask.nc", "-C", str(crsn)])


def test_seeding_tool_coarsening_table():
    gis = _seeding_tool()
    assert gis.coarsening(0) == (None, False)
    assert [gis.coarsening(c) for c in (10, 20, 40, 80, 160, 320)] == [
        (6.0, True), (14.6, True), (34.5, False), (74.75, False), (156., False), (315.6, False)]
