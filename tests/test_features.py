"""Features of a map (sitrk_label_raster / sitrk_mesh_features) without a GPU: the restatement of the contract
that the GPU tests compare against -- connected components by a plain union-find, the table from the labels --, its self-checks
on inputs with known answers, the masks those tests use, sit.feature_table on shapes whose length, width and orientation are
known, and the parser of --deform-features."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import driver as drv
from sitrack_amd import features as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
def label_ref(active, conn):
    """labels (ny,nx) int32 of the contract: -1 where the pixel is not active, else the lowest linear index of its component.
    A union-find over the row runs: the runs of a row that touch a run of the row above (for conn 8: or lie across a corner
    from it) are united, the root of a set being its lowest run, and the first pixel of the lowest run is the lowest index."""
    a = np.asarray(active) != 0
    assert a.ndim == 2 and conn in (4, 8)
    ny, nx = a.shape
    parent, first = [], []                                             # per run: its parent run, its first pixel's linear index

    def find(r):
        while parent[r] != r:
            parent[r] = parent[parent[r]]
            r = parent[r]
        return r

    reach = 1 if conn == 8 else 0
    above, rows = [], []
    for j in range(ny):
        row = np.concatenate(([False], a[j], [False]))
        edge = np.flatnonzero(row[1:] != row[:-1]).tolist()            # run k covers columns edge[2k] .. edge[2k+1]-1
        runs, k = [], 0
        for s, e in zip(edge[0::2], edge[1::2]):
            r = len(parent)
            parent.append(r); first.append(j * nx + s)
            while k < len(above) and above[k][1] <= s - reach:         # wholly to the left of this run and of all that follow
                k += 1
            m = k
            while m < len(above) and above[m][0] < e + reach:          # they share a column, or with corners are one apart
                x, y = find(r), find(above[m][2])
                if x != y:
                    parent[max(x, y)] = min(x, y)                      # runs are numbered in raster order: the lower run is the root
                m += 1
            runs.append((s, e, r))
        rows.append(runs)
        above = runs
    labels = np.full((ny, nx), -1, dtype=np.int32)
    for j, runs in enumerate(rows):
        for s, e, r in runs:
            labels[j, s:e] = first[find(r)]
    return labels


def table_ref(labels, min_pix=1):
    """(table (rows,12) int64 of every component with npix >= min_pix in ascending label, ncomp, nactive) from the labels alone"""
    lab = np.asarray(labels)
    ny, nx = lab.shape
    act = lab >= 0
    pad = np.zeros((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = act
    open_sides = (~pad[:-2, 1:-1]).astype(np.int64) + ~pad[2:, 1:-1] + ~pad[1:-1, :-2] + ~pad[1:-1, 2:]
    jj, ii = np.nonzero(act)
    l = lab[jj, ii].astype(np.int64)
    roots, inv = np.unique(l, return_inverse=True)
    j64, i64 = jj.astype(np.int64), ii.astype(np.int64)
    n = len(roots)

    def total(w):
        out = np.zeros(n, dtype=np.int64)
        np.add.at(out, inv, w)
        return out

    def extreme(w, fn, start):
        out = np.full(n, start, dtype=np.int64)
        fn.at(out, inv, w)
        return out

    big = 1 << 40
    t = np.stack([roots, total(np.ones_like(j64)), extreme(j64, np.minimum, big), extreme(j64, np.maximum, -1),
                  extreme(i64, np.minimum, big), extreme(i64, np.maximum, -1), total(j64), total(i64), total(j64 * j64),
                  total(i64 * i64), total(j64 * i64), total(open_sides[jj, ii])], axis=1).astype(np.int64).reshape(n, 12)
    return t[t[:, 1] >= min_pix], n, int(act.sum())


# ------------------------------------------------------------------------------------------------ the masks of the GPU tests
def checkerboard(ny, nx):
    j, i = np.indices((ny, nx))
    return ((j + i) % 2 == 0).astype(np.int8)


def serpentine(ny, nx):
    """one component, one pixel wide, through every row: the even rows whole, the odd rows one pixel at alternating ends"""
    m = np.zeros((ny, nx), dtype=np.int8)
    m[0::2] = 1
    m[1::4, nx - 1] = 1
    m[3::4, 0] = 1
    return m


def comb(ny, nx, cut=None):
    """a spine along row 0 with a tooth down every second column; cut = (j, i): that pixel of a tooth is taken out"""
    m = np.zeros((ny, nx), dtype=np.int8)
    m[0] = 1
    m[:, 0::2] = 1
    if cut is not None:
        m[cut] = 0
    return m


def spiral(ny, nx, cut=None):
    """a one-pixel-wide path from (0, 0) inwards, clockwise, one pixel between its turns: one component at conn 4 and 8"""
    m = np.zeros((ny, nx), dtype=np.int8)
    j, i, dj, di = 0, 0, 0, 1
    m[0, 0] = 1

    def free(y, x):
        return not (0 <= y < ny and 0 <= x < nx) or m[y, x] == 0

    while True:
        for _ in range(2):                                             # straight on, else one turn to the right
            y, x = j + dj, i + di
            if 0 <= y < ny and 0 <= x < nx and m[y, x] == 0 and free(y + dj, x + di):
                break
            dj, di = di, -dj
        else:
            break
        j, i = y, x
        m[j, i] = 1
    if cut is not None:
        m[cut] = 0
    return m


def diagonals(ny, nx, step=5):
    j, i = np.indices((ny, nx))
    return (((j - i) % step == 0) | ((j + i) % (2 * step + 1) == 0)).astype(np.int8)


def random_mask(ny, nx, density, seed):
    return (np.random.default_rng(seed).random((ny, nx)) < density).astype(np.int8)


def interleaved_combs(ny, nx):
    """two combs that mesh: a spine along row 0 with a tooth down every fourth column, a spine along the last row with a tooth up
    the columns half way between, every tooth two rows short of the other spine.  Two components of nearly equal size, at conn 4
    and at conn 8, whose pixels alternate along every row between the spines"""
    assert ny >= 5 and nx >= 3
    m = np.zeros((ny, nx), dtype=np.int8)
    m[0] = m[ny - 1] = 1
    m[:ny - 2, 0::4] = 1
    m[2:, 2::4] = 1
    return m


def interleaved_labels(ny, nx):
    """(labels, [npix of the upper comb, npix of the lower]) of interleaved_combs in closed form: the upper comb is component 0,
    the lower one is named by the top of its first tooth, (2, 2)"""
    assert ny >= 5 and nx >= 3
    lab = np.full((ny, nx), -1, dtype=np.int32)
    lab[0] = 0
    lab[:ny - 2, 0::4] = 0
    lab[ny - 1] = 2 * nx + 2
    lab[2:, 2::4] = 2 * nx + 2
    return lab, [nx + (ny - 3) * ((nx + 3) // 4), nx + (ny - 3) * ((nx + 1) // 4)]


def full_row(ny, nx):
    """the table row of a raster that is one component, in closed form"""
    sj, si = ny * (ny - 1) // 2, nx * (nx - 1) // 2
    return [0, ny * nx, 0, ny - 1, 0, nx - 1, nx * sj, ny * si, nx * ((ny - 1) * ny * (2 * ny - 1) // 6),
            ny * ((nx - 1) * nx * (2 * nx - 1) // 6), sj * si, 2 * (ny + nx)]


def bars(ny, nx):
    """the rows j with j % 3 != 2: bars of two whole rows, and a last one of one row where ny % 3 == 1"""
    m = np.zeros((ny, nx), dtype=np.int8)
    m[np.arange(ny) % 3 != 2] = 1
    return m


def bars_expected(ny, nx):
    """(labels, table) of bars(ny, nx) in closed form, at conn 4 and 8 alike: bar k is rows 3k .. 3k + h - 1, h = 2 or, for a
    last bar cut by the rim, 1; its label is 3k * nx and every column of its row is a polynomial in k, h, nx"""
    k = np.arange((ny + 2) // 3, dtype=np.int64)
    j0 = 3 * k
    h = np.minimum(2, ny - j0)
    sj, sjj = h * j0 + (h - 1), h * j0 * j0 + (h - 1) * (2 * j0 + 1)  # over the bar's rows: j0 (+ j0 + 1), and the squares
    si, sii = nx * (nx - 1) // 2, (nx - 1) * nx * (2 * nx - 1) // 6    # over a row's columns
    one = np.ones_like(k)
    table = np.stack([j0 * nx, h * nx, j0, j0 + h - 1, 0 * one, (nx - 1) * one, nx * sj, h * si, nx * sjj, h * sii, sj * si,
                      2 * nx + 2 * h], axis=1).astype(np.int64)
    j = np.arange(ny)
    rows = np.where(j % 3 != 2, (j // 3) * 3 * nx, -1).astype(np.int32)
    labels = np.repeat(rows[:, None], nx, axis=1)
    return labels, table


# ------------------------------------------------------------------------------------------------ rasters of a production size
# The kernels of sitrk_label.hip and sitrk_track.hip size their launches on the host from a handful of constants, and take other
# paths on a large raster than on a small one: more than one grid-stride trip, spans of more than kLbMinTrips pieces, borders of
# more than one merge trip.  The three shapes below are the smallest that reach those paths with ragged ends everywhere;
# test_the_large_shapes_reach_the_paths_they_are_for recomputes the launches from the source's own constants, so that a retuned
# constant fails a test instead of taking the coverage away.
TRIP2 = (727, 733)       # 2 grid-stride trips (the second of 8603 pixels), 4 merge levels both ways, borders of 2-3 merge trips
SPAN5 = (1461, 1459)     # spans of 5 pieces, the last wave with 2; 5 grid-stride trips; 5 merge levels; 44-bit sort keys
DEEP = (4099, 4201)      # spans of 33 pieces, shorter than a row; 7 merge levels; closed-form masks only


def kernel_constants():
    """the launch constants of the two sources, read from their text: name -> int"""
    out = {}
    for fn, names in (("sitrk_label.hip", ("kLbFlagBlocks", "kLbSpanWaves", "kLbMinTrips", "kLbThreads")),
                      ("sitrk_track.hip", ("kTrBlocks", "kTrThreads"))):
        src = open(os.path.join(ROOT, "sitrack_amd", "csrc", fn)).read()
        for name in names:
            found = re.findall(r"constexpr\s+[\w\s]+?\b%s\s*=\s*(\d+(?:\s*\*\s*\d+)*)\s*;" % name, src)
            assert len(found) == 1, (fn, name, found)
            out[name] = math.prod(int(f) for f in found[0].split("*"))
    return out


def launch_shape(ny, nx, c, tile=64):
    """what the host of label_run / Strided / sitrk_features_match derives for a raster, restated from their formulas"""
    npix = ny * nx
    up = lambda a, b: -(-a // b)

    def strided(blocks_max, threads):                                  # (trips, pixels of the last trip)
        blocks = max(1, min(up(npix, threads), blocks_max))
        trips = up(npix, blocks * threads)
        return trips, npix - (trips - 1) * blocks * threads

    def merge(n):                                                      # (levels, merge trips of the longest border) along one side
        halves = [tile << k for k in range(16) if (tile << k) < n]
        return len(halves), max([up(min(2 * h, n), c["kLbThreads"]) for h in halves], default=0)

    pieces = up(npix, 64)
    wtrips = max(up(pieces, c["kLbSpanWaves"]), c["kLbMinTrips"])
    waves = up(pieces, wtrips)
    nb = 1
    while (1 << nb) < npix:
        nb += 1
    return {"npix": npix, "flag": strided(c["kLbFlagBlocks"], c["kLbThreads"]), "strided": strided(c["kTrBlocks"], c["kTrThreads"]),
            "wtrips": wtrips, "waves": waves, "last_wave_pieces": pieces - (waves - 1) * wtrips, "last_piece_pixels": npix - (pieces - 1) * 64,
            "merge_j": merge(ny), "merge_i": merge(nx), "nb": nb}


def same_result(got, want_labels, min_pix=1, maxfeat=None, what=""):
    """a result dict of the binding against the restatement on the expected labels: labels (when returned), table, counts"""
    tab, ncomp, nact = table_ref(want_labels, min_pix)
    if got["labels"] is not None:
        assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], want_labels), what
    assert (got["nfeat"], got["ncomp"], got["nactive"]) == (len(tab), ncomp, nact), (what, got["nfeat"], got["ncomp"], got["nactive"])
    keep = tab if maxfeat is None else tab[:maxfeat]
    assert got["table"].dtype == np.int64 and got["table"].shape == keep.shape and np.array_equal(got["table"], keep), what
    return tab


# ------------------------------------------------------------------------------------------------ self-checks of the restatement
def test_checkerboard_is_dust_at_conn_4_and_one_component_at_conn_8():
    m = checkerboard(5, 7)
    l4, l8 = label_ref(m, 4), label_ref(m, 8)
    t4, n4, a4 = table_ref(l4)
    t8, n8, a8 = table_ref(l8)
    assert (n4, a4, len(t4)) == (18, 18, 18) and (t4[:, 1] == 1).all() and (t4[:, 11] == 4).all()
    assert np.array_equal(l4[m != 0], np.flatnonzero(m.ravel())) and (l4[m == 0] == -1).all()
    assert (n8, a8, len(t8)) == (1, 18, 1) and t8[0, 0] == 0 and t8[0, 1] == 18 and t8[0, 11] == 72
    assert (l8[m != 0] == 0).all() and t8[0, 2:6].tolist() == [0, 4, 0, 6]
    assert len(table_ref(l8, 19)[0]) == 0 and len(table_ref(l4, 2)[0]) == 0


@pytest.mark.parametrize("ny,nx", [(1, 1), (3, 8), (7, 5)])
def test_a_full_raster_is_one_component_with_the_rim_as_perimeter(ny, nx):
    for conn in (4, 8):
        lab = label_ref(np.ones((ny, nx)), conn)
        t, n, a = table_ref(lab)
        assert (lab == 0).all() and n == 1 and a == ny * nx
        j, i = np.indices((ny, nx))
        assert t[0].tolist() == [0, ny * nx, 0, ny - 1, 0, nx - 1, j.sum(), i.sum(), (j * j).sum(), (i * i).sum(), (j * i).sum(), 2 * (ny + nx)]
    lab = label_ref(np.zeros((ny, nx)), 8)
    assert (lab == -1).all() and table_ref(lab) [1:] == (0, 0) and table_ref(lab)[0].shape == (0, 12)


def test_concentric_rings_are_nested_components():
    n = 13
    m = np.zeros((n, n), dtype=np.int8)
    for k in (0, 2, 4, 6):
        m[k, k:n - k] = m[n - 1 - k, k:n - k] = 1
        m[k:n - k, k] = m[k:n - k, n - 1 - k] = 1
    for conn in (4, 8):
        t, ncomp, _ = table_ref(label_ref(m, conn))
        assert ncomp == 4 and t[:, 0].tolist() == [k * n + k for k in (0, 2, 4, 6)]
        for k in range(3):                                             # every ring's box lies strictly inside the one before
            assert t[k, 2] < t[k + 1, 2] and t[k, 3] > t[k + 1, 3] and t[k, 4] < t[k + 1, 4] and t[k, 5] > t[k + 1, 5]
        side = n - 2 * np.array([0, 2, 4, 6])
        assert t[:, 1].tolist() == [4 * s - 4 if s > 1 else 1 for s in side]
        assert t[:3, 11].tolist() == [2 * (4 * s - 4) for s in side[:3]] and t[3, 11] == 4


def test_u_shapes_and_corner_contacts_join_only_where_the_contract_says():
    m = np.array([[1, 0, 1, 0, 0],
                  [1, 0, 1, 0, 1],
                  [1, 1, 1, 1, 0]], dtype=np.int8)
    l4, l8 = label_ref(m, 4), label_ref(m, 8)
    assert l4[m != 0].tolist() == [0, 0, 0, 0, 9, 0, 0, 0, 0] and l8[m != 0].tolist() == [0] * 9
    # the second arm is met only in the last row: its pixels still take the first arm's index
    assert table_ref(l4)[0][:, 0].tolist() == [0, 9] and table_ref(l8)[0][0, 1] == 9


def test_the_masks_of_the_gpu_tests_are_what_they_claim():
    for ny, nx in ((1, 300), (63, 65), (67, 131), (3, 517)):
        s = serpentine(ny, nx)
        for conn in (4, 8):
            t, ncomp, nact = table_ref(label_ref(s, conn))
            assert ncomp == 1 and t[0, 1] == nact and t[0, 2:6].tolist() == [0, ny - 1, 0, nx - 1], (ny, nx)
        assert s.sum() == ((ny + 1) // 2) * nx + ny // 2               # one pixel wide: whole rows joined by single pixels
    for ny, nx in ((63, 65), (67, 131)):
        for make in (comb, spiral):
            whole = table_ref(label_ref(make(ny, nx), 4))
            assert whole[1] == 1 and whole[0][0, 1] > (ny * nx) // 3, make.__name__
        assert table_ref(label_ref(comb(ny, nx, cut=(40, 64)), 8))[1] == 2
        sp = spiral(ny, nx)
        assert sp[ny - 1, 62:65].all() and table_ref(label_ref(spiral(ny, nx, cut=(ny - 1, 63)), 8))[1] == 2
        d = diagonals(ny, nx)
        n4, n8 = table_ref(label_ref(d, 4))[1], table_ref(label_ref(d, 8))[1]
        assert n8 < 30 and n4 > 20 * n8
    # near the two percolation thresholds the components are large and tangled
    for density, conn in ((0.41, 8), (0.59, 4)):
        for seed in (1, 2, 3):
            lab = label_ref(random_mask(200, 333, density, seed), conn)
            t, ncomp, _ = table_ref(lab)
            big = t[np.argmax(t[:, 1])]
            tiles = {(j // 64, i // 64) for j, i in zip(*np.nonzero(lab == big[0]))}
            assert ncomp > 100 and len(tiles) > 4, (density, seed, ncomp, len(tiles))


def test_scipy_agrees_where_it_is_installed():
    ndi = pytest.importorskip("scipy.ndimage")
    for conn, st in ((4, None), (8, np.ones((3, 3)))):
        for m in (random_mask(40, 57, 0.5, 5), spiral(30, 41), checkerboard(9, 8)):
            lab, n = ndi.label(m, structure=st)
            mine = label_ref(m, conn)
            assert n == table_ref(mine)[1]
            for k in range(1, n + 1):
                assert len(np.unique(mine[lab == k])) == 1 and mine[lab == k][0] == np.flatnonzero((lab == k).ravel())[0]


def test_interleaved_combs_are_two_components_of_known_sizes():
    for ny, nx in ((5, 3), (6, 4), (9, 13), (31, 66), (67, 131), (40, 257)):
        m = interleaved_combs(ny, nx)
        want, sizes = interleaved_labels(ny, nx)
        assert np.array_equal(want >= 0, m != 0) and m.sum() == sum(sizes) and abs(sizes[0] - sizes[1]) <= ny - 3, (ny, nx)
        for conn in (4, 8):
            lab = label_ref(m, conn)
            t, ncomp, nact = table_ref(lab)
            assert np.array_equal(lab, want), (ny, nx, conn)
            assert ncomp == 2 and t[:, 0].tolist() == [0, 2 * nx + 2] and t[:, 1].tolist() == sizes and nact == sum(sizes), (ny, nx, conn)
            assert t[:, 2:6].tolist() == [[0, ny - 3, 0, nx - 1], [2, ny - 1, 0, nx - 1]]
        # between the spines the two alternate along every row: no two pixels of one comb follow each other
        inner = want[2:ny - 2]
        assert (inner[:, 0::4] == 0).all() and (inner[:, 2::4] == 2 * nx + 2).all() and (inner[:, 1::2] == -1).all()
    ndi = pytest.importorskip("scipy.ndimage")
    for conn, st in ((4, None), (8, np.ones((3, 3)))):
        lab, n = ndi.label(interleaved_combs(67, 131), structure=st)
        want, sizes = interleaved_labels(67, 131)
        assert n == 2 and np.array_equal(lab == 1, want == 0) and np.array_equal(lab == 2, want == 2 * 131 + 2)
        assert np.bincount(lab.ravel())[1:].tolist() == sizes


def test_closed_forms_of_the_full_raster_and_of_the_bars():
    for ny, nx in ((1, 1), (3, 8), (7, 5), (66, 131)):
        assert table_ref(label_ref(np.ones((ny, nx)), 4))[0].tolist() == [full_row(ny, nx)], (ny, nx)
    for ny, nx in ((1, 1), (2, 3), (3, 1), (6, 5), (7, 5), (8, 5), (67, 131), (130, 70)):  # ny % 3 = 0, 1, 2: no, a short, a whole last bar
        m = bars(ny, nx)
        labels, table = bars_expected(ny, nx)
        assert labels.dtype == np.int32 and table.dtype == np.int64 and table.shape == ((ny + 2) // 3, 12)
        for conn in (4, 8):
            lab = label_ref(m, conn)
            assert np.array_equal(lab, labels), (ny, nx, conn)
            t, ncomp, nact = table_ref(lab)
            assert np.array_equal(t, table) and ncomp == len(table) and nact == m.sum() == table[:, 1].sum(), (ny, nx, conn)
        assert (table[-1, 1] == nx) == (ny % 3 == 1)


def test_the_large_shapes_reach_the_paths_they_are_for():
    """TRIP2, SPAN5 and DEEP against the constants as the sources have them now.  If this fails after a constant was retuned, the
    shapes have to follow it: the GPU tests that use them would still pass, on paths they were not written for."""
    c = kernel_constants()
    assert c["kLbThreads"] % 64 == 0 and c["kTrThreads"] % 64 == 0 and _lib.LABEL_TILE == 64
    s = {name: launch_shape(ny, nx, c) for name, (ny, nx) in (("TRIP2", TRIP2), ("SPAN5", SPAN5), ("DEEP", DEEP))}
    for name, (ny, nx) in (("TRIP2", TRIP2), ("SPAN5", SPAN5), ("DEEP", DEEP)):
        v = s[name]
        assert ny % 2 == 1 and nx % 2 == 1 and ny != nx and v["npix"] % 64 != 0 and v["npix"] <= 1 << 28, (name, v)
        assert v["npix"] % c["kLbThreads"] != 0 and v["npix"] % c["kTrThreads"] != 0, (name, v)   # a ragged last workgroup
        for trips, last in (v["flag"], v["strided"]):                  # more than one grid-stride trip, the last one not whole
            assert trips >= 2 and 0 < last < v["npix"] // trips, (name, v)
        assert 1 <= v["last_wave_pieces"] < v["wtrips"] and 0 < v["last_piece_pixels"] < 64, (name, v)
        for levels, border_trips in (v["merge_j"], v["merge_i"]):      # a merge border of more than one trip, both ways
            assert levels >= 4 and border_trips >= 2, (name, v)
        assert 2 * v["nb"] > 34, (name, v)                             # wider sort keys than the small rasters have
    # TRIP2 is the raster of two trips and spans of the least length; SPAN5 and DEEP have longer spans, DEEP's shorter than a row
    assert s["TRIP2"]["flag"][0] == 2 and s["TRIP2"]["strided"][0] == 2 and s["TRIP2"]["wtrips"] == c["kLbMinTrips"]
    assert s["TRIP2"]["merge_j"][1] >= 3 and s["TRIP2"]["merge_i"][1] >= 3
    assert c["kLbMinTrips"] < s["SPAN5"]["wtrips"] < s["DEEP"]["wtrips"] and 64 * s["DEEP"]["wtrips"] < DEEP[1]
    assert s["SPAN5"]["flag"][0] > 2 and s["SPAN5"]["merge_j"][0] > s["TRIP2"]["merge_j"][0] and s["DEEP"]["merge_j"][0] > s["SPAN5"]["merge_j"][0]
    assert s["TRIP2"]["nb"] < s["SPAN5"]["nb"] < s["DEEP"]["nb"]
    # the small shapes of the GPU tests stay below every one of these thresholds: one trip, the least span
    for ny, nx in ((1, 1), (1, 300), (63, 65), (67, 131), (200, 333), (3, 517), (32768, 1)):
        v = launch_shape(ny, nx, c)
        assert v["flag"][0] == 1 and v["strided"][0] == 1 and v["wtrips"] == c["kLbMinTrips"], (ny, nx, v)
    # with the constants as they are today, the figures the three shapes were chosen for
    if (c["kLbFlagBlocks"], c["kLbSpanWaves"], c["kLbMinTrips"], c["kLbThreads"], c["kTrBlocks"], c["kTrThreads"]) == (2048, 8192, 4, 256, 2048, 256):
        assert s["TRIP2"] == {"npix": 532891, "flag": (2, 8603), "strided": (2, 8603), "wtrips": 4, "waves": 2082, "last_wave_pieces": 3,
                              "last_piece_pixels": 27, "merge_j": (4, 3), "merge_i": (4, 3), "nb": 20}
        assert s["SPAN5"] == {"npix": 2131599, "flag": (5, 34447), "strided": (5, 34447), "wtrips": 5, "waves": 6662, "last_wave_pieces": 2,
                              "last_piece_pixels": 15, "merge_j": (5, 6), "merge_i": (5, 6), "nb": 22}
        assert (s["DEEP"]["npix"], s["DEEP"]["wtrips"], s["DEEP"]["merge_j"][0], s["DEEP"]["merge_i"][0], s["DEEP"]["nb"]) == (17219899, 33, 7, 7, 25)


def test_launch_shape_is_what_the_library_computes(tmp_path):
    """launch_shape() is a restatement; the launches are sized by Strided and WaveSpans of sitrk_launch.h.  That header is plain
    C++: a small program built from it prints what it derives, for the three large shapes and at the edges of both formulas, and
    the restatement has to give the same."""
    c = kernel_constants()
    exe = str(tmp_path / "launch_shape_check")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "sitrack_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "c", "launch_shape_check.cpp")], check=True)
    up = lambda a, b: -(-a // b)
    capped = (("flag", c["kLbThreads"], c["kLbFlagBlocks"]), ("strided", c["kTrThreads"], c["kTrBlocks"]))
    counts = [ny * nx for ny, nx in (TRIP2, SPAN5, DEEP)] + [0, 1, 256, 256 * 2048, 256 * 2048 + 1]
    spans = [ny * nx for ny, nx in (TRIP2, SPAN5, DEEP)] + [1, 64, 65, 64 * 4 * 8192, 64 * 4 * 8192 + 1]
    args = []
    for n in counts:
        for _, threads, cap in capped:
            args += ["s", n, threads, cap]
    for n in spans:
        args += ["w", n, c["kLbThreads"], c["kLbSpanWaves"], c["kLbMinTrips"]]
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(got) == 2 * len(counts) + len(spans)
    it = iter(got)
    for n in counts:
        v = launch_shape(1, n, c)
        for key, threads, cap in capped:
            blocks, trips = next(it)
            want_trips, last = v[key]
            assert trips == want_trips and blocks == max(1, min(up(n, threads), cap)), (key, n, blocks, trips, v[key])
            assert n - (trips - 1) * blocks * threads == last, (key, n, blocks, trips, v[key])
    for n in spans:
        v = launch_shape(1, n, c)
        blocks, trips = next(it)
        assert trips == v["wtrips"] and blocks == up(v["waves"], c["kLbThreads"] // 64), (n, blocks, trips, v)
    # the second trip and the longer span start exactly where the formulas say
    if (c["kLbFlagBlocks"], c["kLbSpanWaves"], c["kLbMinTrips"], c["kLbThreads"], c["kTrBlocks"], c["kTrThreads"]) == (2048, 8192, 4, 256, 2048, 256):
        assert got[2 * 3:2 * 8:2] == [(1, 0), (1, 1), (1, 1), (2048, 1), (2048, 2)]
        assert got[2 * len(counts) + 3:] == [(1, 4), (1, 4), (1, 4), (2048, 4), (1639, 5)]


# ------------------------------------------------------------------------------------------------ feature_table
def test_feature_table_of_bars_and_diagonals():
    d, y0, x0 = 2.5, -40., 15.
    for n in (1, 2, 7, 300):
        bar = np.zeros((5, n + 3), dtype=np.int8)
        bar[2, 1:n + 1] = 1
        for m, want_angle in ((bar, 0.), (bar.T, math.pi / 2)):
            t, _, _ = table_ref(label_ref(m, 8))
            f = sit.feature_table(t, (y0, x0, d, m.shape[0], m.shape[1]))
            assert abs(f["length_km"][0] - n * d) <= 1e-12 * n * d and abs(f["width_km"][0] - d) <= 1e-12 * d
            assert f["area_km2"][0] == n * d * d and f["perimeter_km"][0] == (2 * n + 2) * d and f["npix"][0] == n
            if n > 1:
                assert f["angle"][0] == want_angle
            cy, cx = (2.5, 1 + n / 2.) if m is bar else (1 + n / 2., 2.5)
            assert f["y_km"][0] == y0 + cy * d and f["x_km"][0] == x0 + cx * d
    n = 9
    eye = np.eye(n, dtype=np.int8)
    for m, want in ((eye, math.pi / 4), (eye[:, ::-1], -math.pi / 4)):
        t, ncomp, _ = table_ref(label_ref(m, 8))
        f = sit.feature_table(t, (0., 0., 1., n, n))
        assert ncomp == 1 and abs(f["angle"][0] - want) <= 1e-15 and f["length_km"][0] > 5 * f["width_km"][0]
        assert table_ref(label_ref(m, 4))[1] == n
    assert all(len(v) == 0 for v in sit.feature_table(np.zeros((0, 12), dtype=np.int64), (0., 0., 1., 4, 4)).values())
    for bad in ((np.zeros((2, 11), dtype=np.int64), (0., 0., 1., 4, 4)), (np.zeros((2, 12)), (0., 0., 1., 4, 4)),
                (np.zeros((1, 12), dtype=np.int64), (0., 0., 1., 4, 4)), (np.ones((1, 12), dtype=np.int64), (0., 0., 0., 4, 4))):
        with pytest.raises(ValueError, match="feature_table"):
            sit.feature_table(*bad)


# ------------------------------------------------------------------------------------------------ the binding and the wrappers
def test_the_three_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    for name in ("sitrk_label_raster", "sitrk_mesh_features", "sitrk_features_kernel_ms"):
        assert "int %s(sitrk_t *h" % name in hdr and name in _lib._SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert "#define SITRK_FEAT_NCOLS 12" in hdr and _lib.FEAT_NCOLS == 12 == len(_lib.FEAT_COLS)
    assert "#define SITRK_LABEL_TILE %d" % _lib.LABEL_TILE in hdr
    assert _lib.FEAT_COLS[:2] == ("label", "npix") and _lib.FEAT_COLS[-1] == "perimeter"
    assert len(_lib._SIGNATURES["sitrk_label_raster"][1]) == 12 and len(_lib._SIGNATURES["sitrk_mesh_features"][1]) == 20
    for name in ("label_raster", "mesh_features", "features_kernel_ms"):
        assert callable(getattr(_lib.Context, name))
    assert sit.LabelRaster is ft.LabelRaster and sit.feature_table is ft.feature_table and callable(sit.IceTracker.mesh_features)


def test_wrappers_refuse_bad_arguments_before_any_device_work():
    ok = np.ones((4, 5))
    for args, kw in (((np.ones(5),), {}), ((np.ones((0, 5)),), {}), ((np.ones((1, 32769)),), {}), ((ok,), {"conn": 5}),
                     ((ok,), {"conn": 4.5}), ((ok,), {"min_pix": 0}), ((ok,), {"maxfeat": -1}), ((ok,), {"maxfeat": "x"})):
        with pytest.raises(ValueError, match="LabelRaster"):
            sit.LabelRaster(*args, **kw)
    trk = object.__new__(sit.IceTracker)                               # refuses before it reaches its context
    G = (0., 0., 1., 6, 7)
    for kw in ({"grid": (0., 0., 0., 4, 4)}, {"grid": (0., 0., 1., 1, 32769)}, {"what": "curl"}, {"what": 3}, {"sgn": 0}, {"thr": np.nan},
               {"thr": "x"}, {"what": "tot", "sgn": -1}, {"what": "tot", "thr": -1.}, {"conn": 6}, {"min_pix": 0}, {"maxfeat": -3},
               {"at": "t2"}):
        with pytest.raises(ValueError, match="mesh_features"):
            sit.IceTracker.mesh_features(trk, 5, kw.pop("grid", G), **kw)
    assert ft.check_test("div", -1, -2.) == (0, -1, -2.) and ft.check_test("tot", 1, 0.) == (3, 1, 0.)
    assert ft.check_label_args(32768, 8192, 4, 1, 0) == (4, 1, 0)
    with pytest.raises(ValueError, match="2\\^28"):
        ft.check_label_args(32768, 8193, 4, 1, 0)


# ------------------------------------------------------------------------------------------------ the command line
def test_deform_features_flag_parser_and_its_refusals(capsys):
    base = ["-i", "a", "-m", "b", "-s", "c"]
    both = base + ["--deform", "10", "--deform-grid", "12.5"]
    assert drv.parse_args(base).deform_features is None and drv.parse_args(both).deform_features is None
    assert drv.parse_args(both + ["--deform-features", "tot@1e-6"]).deform_features == ("tot", 1, 1e-6, 1, 8)
    assert drv.parse_args(both + ["--deform-features", "conv@2.5e-7@3"]).deform_features == ("div", -1, 2.5e-7, 3, 8)
    assert drv.parse_args(both + ["--deform-features", "div@-1e-7@2@4"]).deform_features == ("div", 1, -1e-7, 2, 4)
    assert drv.parse_args(both + ["--deform-features", "shr@0@1@8"]).deform_features == ("shr", 1, 0., 1, 8)
    assert drv.parse_args(both + ["--deform-features", "vor@-3"]).deform_features == ("vor", 1, -3., 1, 8)
    for bad in ("", "tot", "tot@", "curl@1", "@1", "tot@x", "tot@nan", "tot@inf", "tot@-1e-9", "div@1@0", "div@1@1.5", "div@1@2@6",
                "div@1@2@8@1", "div,1", "TOT@1"):
        with pytest.raises(SystemExit):
            drv.parse_args(both + ["--deform-features", bad])
    capsys.readouterr()
    for argv in (base + ["--deform", "10", "--deform-features", "tot@1e-6"], base + ["--deform-features", "tot@1e-6"]):
        with pytest.raises(SystemExit):
            drv.parse_args(argv)
        assert "--deform-grid" in capsys.readouterr().err
    assert ft.features_arg("conv@1@2@4") == ("div", -1, 1., 2, 4)
    with pytest.raises(ValueError, match="--features"):
        ft.features_arg("tot@-1", "--features")
    with pytest.raises(ValueError, match="32768 pixels a side"):
        ft.check_features_grid((0., 0., 1., 32769, 1))
    assert ft.check_features_grid((0., 0., 1., 32768, 2)) == (0., 0., 1., 32768, 2)


def test_tool_refuses_features_without_grid(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    with pytest.raises(SystemExit, match="--features.*--grid"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--features", "tot@1e-6"])
    with pytest.raises(SystemExit, match="WHAT"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--grid", "5", "--features", "curl@1"])
