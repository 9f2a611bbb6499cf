"""Deformation rates of buoy cells, host side: the numpy restatement of the contract of include/sitrk.h (the reference of
tests/test_gpu_deform.py), its linear-field property, lattice_cells, the binding and tools/deformation.py's argument errors.

Tolerance of the linear-field check, 1e-6 relative: positions near 3000 km round to ulp = 4.5e-13 km, about 4e-10 relative in
the strain of a 10-km cell at strain * T >= 2.5e-3; the double rounding of yx1 adds about 5e-10 and the division by T and the
contour sums 1-3e-9.  That leaves about two orders of margin."""
import os
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FILL = -9999.0
DAY3 = 3 * 86400.


def deform_ref(yx0, yx1, cells, T, mask0=None, mask1=None):
    """The contract of include/sitrk.h, one rounded fp64 operation per symbol, in its order: (out (5, nC), valid (nC,) bool)."""
    yx0, yx1 = np.asarray(yx0, dtype=np.float64), np.asarray(yx1, dtype=np.float64)
    cells = np.asarray(cells)
    nC, nv = cells.shape
    T = np.float64(T)
    y, x, Y, X = yx0[cells, 0], yx0[cells, 1], yx1[cells, 0], yx1[cells, 1]          # (nC, nv)
    ok = np.isfinite(y).all(1) & np.isfinite(x).all(1) & np.isfinite(Y).all(1) & np.isfinite(X).all(1)
    if mask0 is not None:
        ok &= (np.asarray(mask0)[cells] != 0).all(1)
    if mask1 is not None:
        ok &= (np.asarray(mask1)[cells] != 0).all(1)
    with np.errstate(all="ignore"):
        dx, dy = x - x[:, :1], y - y[:, :1]
        ex, ey = X - X[:, :1], Y - Y[:, :1]
        u, v = (X - x) / T, (Y - y) / T
        A2, B2, Suy, Sux, Svy, Svx = (np.zeros(nC) for _ in range(6))
        for k in range(nv):
            q = (k + 1) % nv
            A2 = A2 + (dx[:, k] * dy[:, q] - dx[:, q] * dy[:, k])
            B2 = B2 + (ex[:, k] * ey[:, q] - ex[:, q] * ey[:, k])
            Suy = Suy + (u[:, q] + u[:, k]) * (dy[:, q] - dy[:, k]); Sux = Sux + (u[:, q] + u[:, k]) * (dx[:, q] - dx[:, k])
            Svy = Svy + (v[:, q] + v[:, k]) * (dy[:, q] - dy[:, k]); Svx = Svx + (v[:, q] + v[:, k]) * (dx[:, q] - dx[:, k])
        ok &= (A2 != 0.0) & np.isfinite(A2)
        ux, uy, vx, vy = Suy / A2, -(Sux / A2), Svy / A2, -(Svx / A2)
        div, vor = ux + vy, vx - uy
        shr = np.sqrt((ux - vy) * (ux - vy) + (uy + vx) * (uy + vx))
        out = np.stack([div, shr, vor, 0.5 * np.abs(A2), 0.5 * np.abs(B2)])
    out[:, ~ok] = FILL
    return out, ok


def jittered_lattice(ny, nx, yc, xc, dkm=10.0, jitter=2.0, seed=7):
    """row-major ny x nx points, dkm apart, centred at (yc, xc) km, each moved by up to `jitter` km in y and x"""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(ny) - 0.5 * (ny - 1), np.arange(nx) - 0.5 * (nx - 1), indexing="ij")
    yx = np.stack([yc + dkm * j.ravel(), xc + dkm * i.ravel()], axis=1)
    return yx + rng.uniform(-jitter, jitter, yx.shape)


# u = a_x + u_x x + u_y y, v = a_y + v_x x + v_y y [km/s]; |gradients| in 1e-8 .. 4e-8 1/s
LIN = dict(ax=5e-5, ay=-3e-5, ux=3e-8, uy=-1e-8, vx=2e-8, vy=1.5e-8)
LIN_DIV = LIN["ux"] + LIN["vy"]
LIN_VOR = LIN["vx"] - LIN["uy"]
LIN_SHR = float(np.hypot(LIN["ux"] - LIN["vy"], LIN["uy"] + LIN["vx"]))


def linear_move(yx0, T):
    y, x = yx0[:, 0], yx0[:, 1]
    u = LIN["ax"] + LIN["ux"] * x + LIN["uy"] * y
    v = LIN["ay"] + LIN["vx"] * x + LIN["vy"] * y
    return np.stack([y + T * v, x + T * u], axis=1)


def both_orientations(cells):
    """every second cell reversed"""
    c = cells.copy()
    c[1::2] = c[1::2, ::-1]
    return c


def check_linear_field(out, valid, rtol=1e-6):
    assert valid.all()
    for name, row, want in (("div", 0, LIN_DIV), ("shr", 1, LIN_SHR), ("vor", 2, LIN_VOR)):
        err = np.abs(out[row] - want).max() / abs(want)
        print("linear field: %s max relative error %.3g" % (name, err))
        assert err <= rtol, (name, err)


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_restatement_is_exact_for_a_linear_field(kind):
    yx0 = jittered_lattice(40, 40, -1500., 2000.)
    yx1 = linear_move(yx0, DAY3)
    assert min(abs(LIN[k]) for k in ("ux", "uy", "vx", "vy")) * DAY3 >= 2.5e-3
    cells = both_orientations(sit.lattice_cells(40, 40, kind))
    out, valid = deform_ref(yx0, yx1, cells, DAY3)
    check_linear_field(out, valid)
    # orientation changes nothing but the last bits; the areas are those of the lattice
    out2, _ = deform_ref(yx0, yx1, sit.lattice_cells(40, 40, kind), DAY3)
    assert np.allclose(out, out2, rtol=1e-7, atol=0)
    assert abs(out[3].sum() - (100. * 39 * 39)) < 0.05 * 100. * 39 * 39
    assert np.allclose(out[4] / out[3], 1. + LIN_DIV * DAY3, rtol=1e-3)            # area change = divergence * T, first order


def test_restatement_flags_invalid_cells():
    yx0 = jittered_lattice(5, 5, 100., -200.)
    yx1 = linear_move(yx0, 3600.)
    cells = sit.lattice_cells(5, 5, "quad").copy()
    cells[3] = [6, 6, 7, 12]                                  # a repeated vertex that leaves an area ...
    cells[4] = [8, 8, 13, 13]                                 # ... and one that does not: A2 == 0
    yx1[0, 1] = np.nan
    m0 = np.ones(25, dtype=np.int8); m0[24] = 0
    out, valid = deform_ref(yx0, yx1, cells, 3600., mask0=m0)
    assert not valid[0] and not valid[4] and not valid[15] and valid[3] and valid.sum() == 13
    assert (out[:, ~valid] == FILL).all() and np.isfinite(out[:, valid]).all()


def test_lattice_cells_shapes_and_ranges():
    for ny, nx in ((2, 2), (3, 7), (40, 33)):
        q, t = sit.lattice_cells(ny, nx, "quad"), sit.lattice_cells(ny, nx, "tri")
        assert q.shape == ((ny - 1) * (nx - 1), 4) and t.shape == (2 * (ny - 1) * (nx - 1), 3)
        assert q.dtype == np.int32 and t.dtype == np.int32 and q.flags.c_contiguous and t.flags.c_contiguous
        for c in (q, t):
            assert c.min() == 0 and c.max() == ny * nx - 1
            assert all(len(set(r)) == c.shape[1] for r in c.tolist())
        # one orientation throughout, and the triangles tile the quadrangles
        j, i = np.meshgrid(np.arange(ny, dtype=float), np.arange(nx, dtype=float), indexing="ij")
        yx = np.stack([j.ravel(), i.ravel()], axis=1)

        def area2(c):
            y, x = yx[c, 0], yx[c, 1]
            return sum(x[:, k] * y[:, (k + 1) % c.shape[1]] - x[:, (k + 1) % c.shape[1]] * y[:, k] for k in range(c.shape[1]))
        assert (area2(q) == 2.).all() and (area2(t) == 1.).all()
        assert all(set(a) == set(b) for a, b in zip(t.reshape(-1, 6).tolist(), q.tolist()))
    with pytest.raises(ValueError):
        sit.lattice_cells(1, 5)
    with pytest.raises(ValueError):
        sit.lattice_cells(4, 4, "hex")


def test_binding_covers_the_deformation_symbols():
    for name in ("sitrk_deform_cells", "sitrk_deform_mark", "sitrk_deform_since_mark"):
        assert name in _lib._SIGNATURES
    L = _lib.lib()                                            # binds every declared symbol: the library exports them
    for name in ("sitrk_deform_cells", "sitrk_deform_mark", "sitrk_deform_since_mark"):
        assert hasattr(L, name)
    for name in ("deform_cells", "deform_mark", "deform_since_mark"):
        assert callable(getattr(_lib.Context, name))
    assert callable(sit.IceTracker.deform_mark) and callable(sit.IceTracker.deform)


def test_deformcells_refuses_bad_arguments_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(_lib, "Context", no_device)
    import sitrack_amd.tracking as trk
    monkeypatch.setattr(trk, "default_context", no_device)
    yx = np.zeros((6, 2))
    with pytest.raises(ValueError, match="cells"):
        sit.DeformCells(yx, yx, np.zeros((2, 5), dtype=np.int64), 3600.)
    with pytest.raises(ValueError, match="cells"):
        sit.DeformCells(yx, yx, np.zeros((2, 3)), 3600.)
    for T in (0., -1., np.nan, np.inf, "soon"):
        with pytest.raises(ValueError, match="`T`"):
            sit.DeformCells(yx, yx, np.zeros((2, 3), dtype=np.int64), T)
    with pytest.raises(ValueError, match="yx1"):
        sit.DeformCells(yx, yx[:5], np.zeros((2, 3), dtype=np.int64), 3600.)
    with pytest.raises(ValueError, match="mask1"):
        sit.DeformCells(yx, yx, np.zeros((2, 3), dtype=np.int64), 3600., mask1=np.ones(5))


def track_file(path, yx0, yx1, ids, t0=1000000, T=int(DAY3), mask=None):
    """a 2-record trajectory file as the tracker writes it"""
    pos = np.stack([yx0, yx1])
    zero = np.zeros(pos.shape[:2])
    msk = np.ones(pos.shape[:2], dtype=np.int8) if mask is None else mask
    ncio.ncSaveCloudBuoys(str(path), np.array([t0, t0 + T], dtype=np.int32), ids, pos[:, :, 0], pos[:, :, 1], zero, zero, mask=msk)
    return str(path)


def test_tool_argument_errors(tmp_path, monkeypatch, capsys):
    import deformation as tool
    monkeypatch.setattr(sit, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device context was asked for")))
    yx0 = jittered_lattice(4, 5, -1500., 2000.)
    ids = 100 + 3 * np.arange(20, dtype=np.int64)[::-1]
    fin = track_file(tmp_path / "trk.nc", yx0, linear_move(yx0, DAY3), ids)
    good = str(tmp_path / "cells.npy")
    np.save(good, ids[sit.lattice_cells(4, 5, "tri")])
    bad = str(tmp_path / "bad.npy")
    cells = ids[sit.lattice_cells(4, 5, "tri")].copy()
    cells[5, 1] = 101
    np.save(bad, cells)
    with pytest.raises(SystemExit, match="id_buoy 101 "):
        tool.main(["-i", fin, "-c", bad])
    for opt in ("-k", "-K"):
        with pytest.raises(SystemExit, match="%s 2 outside the 2 records" % opt):
            tool.main(["-i", fin, "-c", good, opt, "2"])
    with pytest.raises(SystemExit, match="not later"):
        tool.main(["-i", fin, "-c", good, "-k", "1", "-K", "0"])
    five = str(tmp_path / "five.npy")
    np.save(five, np.zeros((3, 5), dtype=np.int64))
    with pytest.raises(SystemExit, match=r"\(nC,3\) or \(nC,4\)"):
        tool.main(["-i", fin, "-c", five])
    monkeypatch.setitem(sys.modules, "scipy.spatial", None)               # the import of scipy.spatial fails
    with pytest.raises(SystemExit, match="-c CELLS.npy"):
        tool.main(["-i", fin, "-c", "auto"])
