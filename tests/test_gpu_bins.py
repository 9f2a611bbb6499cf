"""bin_start_kernel of sitrack_amd/csrc/sitrk_bins.h on the MI355X: the offsets of the coast index and of the pair bins, through the
results that are read off them.  It replaced a search with a loop of its own length in the coast build, so the coast is built with
exactly 1, 2, 3, 7, 8, 9, 255, 256 and 257 segments -- lengths at and around the powers of two where the fixed trip count of
lower_bound_steps grows -- with one bin and with many mostly empty ones; and the pair bins hold 1, 2, 63, 64 and 65 valid points.

Coast: the rules of tests/test_gpu_coast.py, and tighter: seg equal, d2 of the reported segment equal to the brute-force minimum
bit for bit, and dist equal to numpy's (correctly rounded) square root of it in every bit.  Pairs: check() of tests/test_gpu_pairs.py,
counts as integers and the sums within the bound derived there."""
import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import synthetic as syn

from test_coast import coast_dist_ref, coast_segments_ref
from test_gpu_coast import check_against
from test_gpu_pairs import check
from test_pairs import jitter_cloud, pairs_ref, smooth_move

pytestmark = pytest.mark.gpu

COAST_COUNTS = (1, 2, 3, 7, 8, 9, 255, 256, 257)
NJ, NI = 36, 36


@pytest.fixture(scope="module")
def ctx():
    c = sit.Context(0)
    yield c
    c.close()


def coast_with(nseg):
    """a 36 x 36 grid whose coast has exactly nseg segments: a land cell with sea on all four sides has four, and each land cell
    of the rim row j = 0 has one, its edge towards row 1 (include/sitrk.h: no k = 0 edge at j = 0)"""
    g = syn.make_grid(NJ, NI, dkm=4., warp=0.6, rim=0)
    t = g["tmask"]
    t[:] = 1
    lone, rim = divmod(nseg, 4)
    if rim:
        t[0, 1:1 + rim] = 0
    jj, ii = np.meshgrid(np.arange(2, NJ - 2, 2), np.arange(2, NI - 2, 2), indexing="ij")      # 16 x 16 cells, none next to another
    pick = np.random.default_rng(nseg).permutation(jj.size)[:lone]
    t[jj.ravel()[pick], ii.ravel()[pick]] = 0
    return g


def coast_queries(g, ab, seed):
    """some 300 queries: in the grid's box, far outside it on all four sides, just outside the box of the segments' midpoints, on
    segment ends and interiors, and two that are not finite"""
    rng = np.random.default_rng(seed)
    y0, y1, x0, x1 = g["Yf"].min(), g["Yf"].max(), g["Xf"].min(), g["Xf"].max()
    inside = np.stack([rng.uniform(y0, y1, 150), rng.uniform(x0, x1, 150)], axis=1)
    L = 10. * max(y1 - y0, x1 - x0)
    far = np.stack([rng.uniform(y0, y1, 64), rng.uniform(x0, x1, 64)], axis=1)
    far[0:16, 0] += L; far[16:32, 0] -= L; far[32:48, 1] += L; far[48:64, 1] -= L
    mid = 0.5 * ab[:, 0] + 0.5 * ab[:, 1]
    lo, hi = mid.min(axis=0), mid.max(axis=0)
    near = np.array([[lo[0] - 1e-3, lo[1] - 1e-3], [hi[0] + 1e-3, hi[1] + 1e-3], [lo[0] - 1e-3, hi[1] + 1e-3], [hi[0] + 1e-3, lo[1] - 1e-3],
                     [np.nextafter(lo[0], -np.inf), lo[1]], [hi[0], np.nextafter(hi[1], np.inf)], [lo[0], lo[1]], [hi[0], hi[1]]])
    k = rng.integers(0, len(ab), 40)
    ends = ab[k, rng.integers(0, 2, 40)]
    inner = ab[k, 0] + rng.integers(1, 8, 40)[:, None] / 8. * (ab[k, 1] - ab[k, 0])
    bad = np.array([[np.nan, 0.], [0., np.inf]])
    return np.ascontiguousarray(np.concatenate([inside, far, near, ends, inner, bad]))


@pytest.mark.parametrize("nseg", COAST_COUNTS)
def test_coast_of_exactly_n_segments_in_one_bin_and_in_many(ctx, nseg):
    g = coast_with(nseg)
    ids_r, ab_r, nd_r = coast_segments_ref(g["Yf"], g["Xf"], g["tmask"])
    assert (len(ids_r), nd_r) == (nseg, 0)                          # the restatement agrees on what the mask was made for
    yx = coast_queries(g, ab_r, 100 + nseg)
    assert 300 <= len(yx) <= 400
    d2r, segr, distr = coast_dist_ref(yx, ids_r, ab_r)
    fin = segr >= 0
    assert fin.sum() == len(yx) - 2
    try:
        for coast_bin in (4, 1, 64):                                # the default, then bins so coarse / so fine that the grid is one bin / mostly empty
            ctx.set_tuning(coast_bin=coast_bin)
            built = ctx.coast_build(g["Yf"], g["Xf"], g["tmask"])
            ids, ab = ctx.coast_segments()
            assert len(ids) == nseg                                 # before anything else: the case is the one it is named for
            assert built == (nseg, 0) and np.array_equal(ids, ids_r) and np.array_equal(ab, ab_r)
            dist, seg = ctx.coast_dist(yx)
            label = "%d segments, coast_bin %d" % (nseg, coast_bin)
            check_against(dist, seg, yx, ids_r, ab_r, label=label)
            print("%s: dist differs from numpy's in %d of %d" % (label, int((dist[fin] != distr[fin]).sum()), int(fin.sum())))
            assert np.array_equal(seg, segr), label
            assert dist[fin].tobytes() == distr[fin].tobytes(), label
            assert np.isnan(dist[~fin]).all(), label
    finally:
        ctx.set_tuning(coast_bin=4)


@pytest.mark.parametrize("nvalid", (1, 2, 63, 64, 65))
def test_pairs_of_exactly_n_valid_points_in_one_class(ctx, nvalid):
    """80 points of which nvalid are valid, by both masks: the invalid ones sort behind the last bin, and the search runs over a
    range of exactly nvalid"""
    yx = jitter_cloud(12)[:80]
    yx1 = smooth_move(yx)
    order = np.random.default_rng(nvalid).permutation(80)
    m0, m1 = np.zeros(80, dtype=np.int8), np.ones(80, dtype=np.int8)
    m0[order[:nvalid + 5]] = 1
    m1[order[nvalid:nvalid + 5]] = 0
    edges = (8., 45.)
    ref = pairs_ref(yx, yx1, edges, mask0=m0, mask1=m1)
    assert ref["npts"] == nvalid and (nvalid < 63 or ref["table"][0, 0] > 100)
    got = ctx.pairs_points(yx, yx1, edges, mask0=m0, mask1=m1)
    assert got["npts"] == nvalid
    check(got, ref, "%d valid points" % nvalid)
