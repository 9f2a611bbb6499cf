"""Buoy cells rasterised onto a regular grid (sitrk_raster_cells, sitrk_mesh_raster; include/sitrk.h): the numpy
restatement the GPU tests compare against, its self-checks, the binding, raster_grid and the command line's parser.

raster_ref() is written from the contract alone: every pixel against every cell, no bounding box, the lowest index wins by
construction (argmax over a boolean (cell, pixel) table finds the first True).  numpy's elementwise fp64 + - * round once per
operation and never fuse, so the restatement is exact."""
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import driver as drv
from sitrack_amd import raster as ras
from test_mesh import ccw_quads, exact_lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sitrk_raster_cells", "sitrk_mesh_raster", "sitrk_raster_kernel_ms")
LATTICE_GRID = (-1506., 1994., 4., 30, 34)


def centres(grid):
    """(cy (ny,), cx (nx,)): one rounded product and one rounded sum each"""
    y0, x0, d, ny, nx = grid
    y0, x0, d = np.float64(y0), np.float64(x0), np.float64(d)
    return y0 + (np.arange(ny, dtype=np.float64) + 0.5) * d, x0 + (np.arange(nx, dtype=np.float64) + 0.5) * d


def drawable(P):
    """(drawable (nC,) bool, s (nC,) = +1 | -1) of the cells P (nC, nv, 2) [y,x]: the shoelace sum of sitrk_deform_cells"""
    P = np.asarray(P, dtype=np.float64)
    nv = P.shape[1]
    with np.errstate(all="ignore"):
        dx, dy = P[:, :, 1] - P[:, :1, 1], P[:, :, 0] - P[:, :1, 0]
        A2 = np.zeros(len(P))
        for k in range(nv):
            q = (k + 1) % nv
            A2 = A2 + (dx[:, k] * dy[:, q] - dx[:, q] * dy[:, k])
    ok = np.isfinite(P).all(axis=(1, 2)) & np.isfinite(A2) & (A2 != 0.)
    return ok, np.where(A2 > 0., 1., -1.)


def raster_inside(P, draw, grid):
    """(nC, ny, nx) bool: the centre of pixel (j,i) lies IN drawn cell c"""
    P = np.asarray(P, dtype=np.float64)
    nC, nv = P.shape[:2]
    cy, cx = centres(grid)
    ok, s = drawable(P)
    if draw is not None:
        ok = ok & (np.asarray(draw) != 0)
    inside = np.zeros((nC, len(cy), len(cx)), dtype=bool)
    CY, CX = cy[None, :, None], cx[None, None, :]
    for lo in range(0, nC, 256):
        p = P[lo:lo + 256]
        acc = np.repeat(ok[lo:lo + 256, None, None], len(cy), axis=1).repeat(len(cx), axis=2)
        with np.errstate(all="ignore"):
            for k in range(nv):
                q = (k + 1) % nv
                yk, xk = p[:, k, 0, None, None], p[:, k, 1, None, None]
                ex, ey = p[:, q, 1, None, None] - xk, p[:, q, 0, None, None] - yk
                o = ex * (CY - yk) - ey * (CX - xk)
                acc &= s[lo:lo + 256, None, None] * o >= 0.
        inside[lo:lo + 256] = acc
    return inside


def raster_ref(P, draw, grid):
    """owner (ny, nx) int32 of the contract: the lowest index among the drawn cells the centre lies in, -1 for none"""
    inside = raster_inside(P, draw, grid)
    if inside.shape[0] == 0:
        return np.full(inside.shape[1:], -1, dtype=np.int32)
    return np.where(inside.any(axis=0), inside.argmax(axis=0), -1).astype(np.int32)


_CASES = {}


def lattice_case():
    """the exact lattice of tests/test_mesh.py on a grid where every second centre lies exactly on a lattice line:
    (yx, quads, owner, inside)"""
    if "lattice" not in _CASES:
        yx, quads = exact_lattice(12, 14, 8.0), ccw_quads(12, 14)
        inside = raster_inside(yx[quads], None, LATTICE_GRID)
        _CASES["lattice"] = (yx, quads, raster_ref(yx[quads], None, LATTICE_GRID), inside)
    return _CASES["lattice"]


JITTER_ORIGIN = (-1508.3, 1988.9)
JITTER_GRIDS = {2.96: JITTER_ORIGIN + (2.96, 101, 107), 8.0: JITTER_ORIGIN + (8.0, 37, 41), 18.4: JITTER_ORIGIN + (18.4, 19, 17)}
JITTER_INNER = (-1400.7, 2100.3, 5.3, 9, 7)                         # wholly inside the mesh: the mesh reaches beyond it on all sides
JITTER_COUNTS = {2.96: (8952, 1225), 8.0: (1223, 1056), 18.4: (238, 238)}      # owned pixels, distinct owners


def jitter_case():
    """36 x 36 points 8 km apart, jittered by up to a quarter of the spacing, 1225 quadrangles: (yx, quads, {d: owner})"""
    if "jitter" not in _CASES:
        yx = exact_lattice(36, 36, 8.0) + np.random.default_rng(1).uniform(-2., 2., (36 * 36, 2))
        quads = ccw_quads(36, 36)
        owners = {d: raster_ref(yx[quads], None, g) for d, g in JITTER_GRIDS.items()}
        owners["inner"] = raster_ref(yx[quads], None, JITTER_INNER)
        _CASES["jitter"] = (yx, quads, owners)
    return _CASES["jitter"]


def split_quads(quads):
    """each quadrangle (a,b,c,d) as the triangles (a,b,c), (a,c,d): rows 2q and 2q+1"""
    return np.ascontiguousarray(np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3))


# ------------------------------------------------------------------------------------------------ the restatement's self-checks
def test_restatement_on_the_exact_lattice_resolves_ties_to_the_lowest_index():
    yx, quads, owner, inside = lattice_case()
    assert len(quads) == 143 and owner.shape == (30, 34) and owner.dtype == np.int32
    claims = inside.sum(axis=0)
    print("owned %d of %d, claimed by 2: %d, by 4: %d, owners %d" % ((owner >= 0).sum(), owner.size, (claims == 2).sum(), (claims == 4).sum(),
                                                                   len(np.unique(owner[owner >= 0]))))
    assert (owner >= 0).sum() == 621 and owner.size == 1020
    assert (claims == 2).sum() == 306 and (claims == 4).sum() == 120 and set(np.unique(claims)) == {0, 1, 2, 4}
    assert np.array_equal(np.unique(owner[owner >= 0]), np.arange(143))
    for j, i in zip(*np.nonzero(claims >= 2)):
        assert owner[j, i] == np.flatnonzero(inside[:, j, i]).min()
    assert np.array_equal(owner >= 0, claims > 0)


def test_restatement_orientation_degenerate_cells_and_clipping():
    yx, quads, owner, _ = lattice_case()
    P = yx[quads]
    # clockwise rows own the same pixels
    assert np.array_equal(raster_ref(P[:, ::-1], None, LATTICE_GRID), owner)
    mixed = P.copy()
    mixed[::3] = mixed[::3, ::-1]
    assert np.array_equal(raster_ref(mixed, None, LATTICE_GRID), owner)
    # a zero-area cell, a NaN vertex, draw == 0: each owns nothing, and its pixels go to the next claimant or to nobody
    flat, nan = P.copy(), P.copy()
    flat[20, 2], flat[20, 3] = flat[20, 1], flat[20, 0]
    nan[20, 2, 1] = np.nan
    draw = np.ones(143, dtype=np.int8)
    draw[20] = 0
    want = raster_ref(np.delete(P, 20, axis=0), None, LATTICE_GRID)
    want = np.where(want >= 20, want + 1, want)
    assert (owner == 20).sum() > 0 and not (want == 20).any()
    for got in (raster_ref(flat, None, LATTICE_GRID), raster_ref(nan, None, LATTICE_GRID), raster_ref(P, draw, LATTICE_GRID)):
        assert np.array_equal(got, want)
    assert (raster_ref(P, np.zeros(143), LATTICE_GRID) == -1).all()
    # a cell wholly outside the raster owns nothing; one straddling the rim is clipped
    one = np.array([[[0., 0.], [0., 10.], [10., 10.], [10., 0.]]])
    assert (raster_ref(one, None, (20., 20., 1., 5, 5)) == -1).all() and (raster_ref(one, None, (-20., 0., 1., 5, 5)) == -1).all()
    got = raster_ref(one, None, (8., 7., 1., 5, 6))                  # centres y 8.5 .. 12.5, x 7.5 .. 12.5
    want = np.full((5, 6), -1)
    want[:2, :3] = 0
    assert np.array_equal(got, want)
    # triangles: the two halves of a quadrangle own what it owns, the diagonal going to the first half
    tri = raster_ref(yx[split_quads(quads)], None, LATTICE_GRID)
    assert np.array_equal(tri >= 0, owner >= 0) and np.array_equal(tri[tri >= 0] // 2, owner[owner >= 0])
    # no cells
    assert (raster_ref(np.zeros((0, 4, 2)), None, LATTICE_GRID) == -1).all()


def test_jittered_lattice_counts():
    yx, quads, owners = jitter_case()
    assert len(quads) == 1225
    for d, (owned, distinct) in JITTER_COUNTS.items():
        o = owners[d]
        ny, nx = JITTER_GRIDS[d][3:]
        print("d = %g: %d x %d pixels, %d owned, %d distinct owners" % (d, ny, nx, (o >= 0).sum(), len(np.unique(o[o >= 0]))))
        assert o.shape == (ny, nx) and (o >= 0).sum() == owned and len(np.unique(o[o >= 0])) == distinct
        y0, x0, dd = JITTER_GRIDS[d][:3]                             # the raster reaches beyond the mesh on all four sides
        assert y0 < yx[:, 0].min() and x0 < yx[:, 1].min() and y0 + ny * dd > yx[:, 0].max() and x0 + nx * dd > yx[:, 1].max()
    assert (owners["inner"] >= 0).all() and owners["inner"].shape == (9, 7)      # ... and the mesh beyond the inner raster


# ------------------------------------------------------------------------------------------------ the binding
def test_symbols_are_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    L = _lib.lib()
    for name in NAMES + ("sitrk_raster_stats",):
        assert "int %s(sitrk_t *h" % name in txt and name in _lib._SIGNATURES and hasattr(L, name)
    for name in ("raster_cells", "mesh_raster", "raster_kernel_ms"):
        assert callable(getattr(_lib.Context, name))
    assert callable(sit.IceTracker.mesh_raster) and callable(sit.RasterCells) and callable(sit.raster_grid)


# ------------------------------------------------------------------------------------------------ raster_grid
def test_raster_grid_arithmetic():
    assert sit.raster_grid(-1500., -1412., 2000., 2104., 4.) == (-1500., 2000., 4., 22, 26)      # a box on exact multiples of d
    assert sit.raster_grid(8., 16., -8., 8., 4.) == (8., -8., 4., 2, 4)
    assert sit.raster_grid(8., 16.000001, -8.5, 8., 4.) == (8., -12., 4., 3, 5)
    assert sit.raster_grid(1., 1., 2., 2., 0.5) == (1., 2., 0.5, 1, 1)                           # a point: one pixel
    assert sit.raster_grid(-0.1, 0.1, -0.1, 0.1, 1.) == (-1., -1., 1., 2, 2)
    rng = np.random.default_rng(4)
    for _ in range(200):
        lo = rng.uniform(-3000., 3000., 2)
        hi = lo + rng.uniform(0., 500., 2)
        d = float(rng.choice([0.37, 1., 2.96, 12.5]))
        y0, x0, dd, ny, nx = sit.raster_grid(lo[0], hi[0], lo[1], hi[1], d)
        assert dd == d and y0 == np.floor(lo[0] / d) * d and x0 == np.floor(lo[1] / d) * d
        assert ny == max(1, int(np.ceil((hi[0] - y0) / d))) and nx == max(1, int(np.ceil((hi[1] - x0) / d)))
        assert y0 <= lo[0] and x0 <= lo[1] and y0 + ny * d >= hi[0] - 1e-9 and x0 + nx * d >= hi[1] - 1e-9
        assert isinstance(ny, int) and isinstance(nx, int)
    for bad in ((0., 1., 0., 1., 0.), (0., 1., 0., 1., -1.), (0., 1., 0., 1., np.nan), (0., np.inf, 0., 1., 1.), (2., 1., 0., 1., 1.),
                (0., 1., 3., 1., 1.)):
        with pytest.raises(ValueError, match="raster_grid"):
            sit.raster_grid(*bad)
    for bad in ((0., 0., 1., 0, 5), (0., 0., 1., 5, -1), (0., 0., 0., 5, 5), (np.nan, 0., 1., 5, 5), (0., 0., 1., 2 ** 14, 2 ** 14 + 1),
                (0., 0., 1., 2.5, 5), (0., 0., 1., 5)):
        with pytest.raises(ValueError, match="grid"):
            ras.check_grid(bad)
    assert ras.check_grid((0, 0, 1, 2 ** 14, 2 ** 14)) == (0., 0., 1., 2 ** 14, 2 ** 14)


def test_python_argument_checks_come_before_any_device_work(monkeypatch):
    def untouched(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr("sitrack_amd.tracking.default_context", untouched)
    yx, quads = exact_lattice(3, 3, 8.0), ccw_quads(3, 3)
    for args, kw in (((yx, quads[:, :2], LATTICE_GRID), {}), ((yx, quads.astype(float), LATTICE_GRID), {}), ((yx[:, 0], quads, LATTICE_GRID), {}),
                     ((yx, quads, LATTICE_GRID), {"draw": np.ones(3)}), ((yx, quads, (0., 0., -1., 4, 4)), {}),
                     ((yx, quads, (0., 0., 1., 2 ** 15, 2 ** 15)), {})):
        with pytest.raises(ValueError, match="RasterCells"):
            sit.RasterCells(*args, **kw)


# ------------------------------------------------------------------------------------------------ the command line
def test_deform_grid_flag_parser_and_its_two_refusals(capsys):
    base = ["-i", "a", "-m", "b", "-s", "c"]
    assert drv.parse_args(base).deform_grid is None and drv.parse_args(base + ["--deform", "10"]).deform_grid is None
    assert drv.parse_args(base + ["--deform", "10", "--deform-grid", "12.5"]).deform_grid == (12.5, "t0")
    assert drv.parse_args(base + ["--deform", "10", "--deform-grid", "5@t0"]).deform_grid == (5., "t0")
    assert drv.parse_args(base + ["--deform", "10,20@5", "--deform-grid", "1e1@t1"]).deform_grid == (10., "t1")
    for bad in ("", "0", "-2", "nan", "inf", "5@", "5@t2", "@t0", "5@t0@t1", "x", "5,6"):
        with pytest.raises(SystemExit):
            drv.parse_args(base + ["--deform", "10", "--deform-grid", bad])
    # refusal 1: nothing to rasterise without --deform
    capsys.readouterr()
    with pytest.raises(SystemExit):
        drv.parse_args(base + ["--deform-grid", "10"])
    assert "without --deform" in capsys.readouterr().err
    # refusal 2: more than 2^28 pixels over the model's F-points
    j, i = np.meshgrid(np.arange(50.), np.arange(60.), indexing="ij")
    Yf, Xf = -1000. + 12. * j, 500. + 12. * i
    assert drv.deform_grid(Yf, Xf, 10.) == sit.raster_grid(-1000., -1000. + 12. * 49, 500., 500. + 12. * 59, 10.) == (-1000., 500., 10., 59, 71)
    with pytest.raises(ValueError, match="--deform-grid.*2\\^28"):
        drv.deform_grid(Yf, Xf, 0.03)
    Yn = Yf.copy()
    Yn[0, 0] = np.nan                                                 # a non-finite F-point takes no part
    assert drv.deform_grid(Yn, Xf, 10.) == (-1000., 500., 10., 59, 71)


def test_too_large_a_grid_is_refused_before_anything_is_computed(monkeypatch):
    j, i = np.meshgrid(np.arange(50.), np.arange(60.), indexing="ij")
    grid = (np.ones((50, 60), dtype=np.int8), None, None, None, None, -1000. + 12. * j, 500. + 12. * i, None)

    def untouched(*a, **k):
        raise AssertionError("the run went on")

    class Ctx:
        def __init__(self, *a):
            pass

    monkeypatch.setattr(drv.ncio, "SeedFileTimeInfo", lambda *a, **k: (0., 0., "s", "b", None))
    monkeypatch.setattr(drv.ncio, "ModelFileTimeInfo", lambda *a, **k: (10, np.arange(10) * 3600., 0., 9 * 3600., "C", "E"))
    monkeypatch.setattr(drv, "GetTimeSpan", lambda *a, **k: (5, 0, 5, 0., 5 * 3600.))
    monkeypatch.setattr(drv.os, "makedirs", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "Context", Ctx)
    monkeypatch.setattr(drv.ncio, "GetModelGrid", lambda *a, **k: grid)
    monkeypatch.setattr(drv.ncio, "GetModelUVGrid", lambda *a, **k: (None,) * 4)
    monkeypatch.setattr(drv.ncio, "ModelRecords", untouched)
    monkeypatch.setattr(drv, "SeedInit", untouched)
    monkeypatch.setattr(drv, "IceTracker", untouched)
    with pytest.raises(ValueError, match="--deform-grid.*2\\^28"):
        drv.main(["-i", "a", "-m", "b", "-s", "sitrack_seeding_nemoTsi3_19961215_00_HSS5.nc", "--deform", "5", "--deform-grid", "0.03"])
