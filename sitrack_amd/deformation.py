"""Deformation rates of buoy triangles and quadrangles: host side of `sitrk_deform_cells` (sitrack_amd/csrc/sitrk_deform.hip).

An extra the reference does not have: its tracking12 file is written for the deformation scripts of another project.  The
rates -- divergence, shear, vorticity -- are the line-integral (Green) estimate on each cell's t0 contour, evaluated in fp64
on the GPU; the contract (operation order, validity, fill) is in include/sitrk.h and DESIGN.md 3.9.  There is no host
version."""
import math

import numpy as np


def lattice_cells(ny, nx, kind="tri"):
    """Cells of a row-major ny x nx point lattice (point (j,i) has index j*nx + i), as an (nC, nv) int32 array:
    kind 'quad' -> the (ny-1)(nx-1) quadrangles (j,i), (j,i+1), (j+1,i+1), (j+1,i), in C order of (j,i);
    kind 'tri'  -> twice as many triangles, each quadrangle cut along (j,i)-(j+1,i+1): its lower-right half, then its
    upper-left half."""
    ny, nx = int(ny), int(nx)
    if ny < 2 or nx < 2:
        raise ValueError("lattice_cells: the lattice needs at least 2 x 2 points, got %d x %d" % (ny, nx))
    if ny * nx >= 2 ** 31 - 1:
        raise ValueError("lattice_cells: %d x %d points do not fit int32 indices" % (ny, nx))
    j, i = np.meshgrid(np.arange(ny - 1, dtype=np.int32), np.arange(nx - 1, dtype=np.int32), indexing="ij")
    a = (j * nx + i).ravel()
    b, c, d = a + 1, a + nx + 1, a + nx
    if kind == "quad":
        return np.ascontiguousarray(np.stack([a, b, c, d], axis=1))
    if kind == "tri":
        return np.ascontiguousarray(np.stack([a, b, c, a, c, d], axis=1).reshape(-1, 3))
    raise ValueError("lattice_cells: kind must be 'tri' or 'quad', got %r" % (kind,))


def _as_dict(out, valid):
    div, shr, vor, area0, area1 = out
    tot = np.full_like(div, -9999.0)
    tot[valid] = np.sqrt(div[valid] * div[valid] + shr[valid] * shr[valid])
    return {"div": div, "shr": shr, "vor": vor, "tot": tot, "area0": area0, "area1": area1, "valid": valid}


def DeformCells(yx0, yx1, cells, T, mask0=None, mask1=None, ctx=None):
    """Deformation rates [1/s] of the cells (nC, 3|4) of buoy indices between the positions yx0 and yx1 (nP,2) [y,x] km that lie
    T seconds apart; mask0 / mask1 (nP): 0 = the buoy is no valid vertex at t0 / t1.  Runs on the GPU.  Returns a dict of div,
    shr, vor, tot = sqrt(div^2 + shr^2), area0, area1 [km^2] (nC,) fp64 and valid (nC,) bool; invalid cells hold -9999.
    Raises ValueError on bad arguments before any device work, IndexError for a vertex index outside the buoys."""
    from .tracking import default_context
    cerr = 'ERROR [DeformCells()]: '
    c = np.asarray(cells)
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError(cerr + '`cells` must be an (nC, 3) or (nC, 4) array of buoy indices, got shape %s' % (c.shape,))
    if c.dtype.kind not in "iu":
        raise ValueError(cerr + '`cells` must hold integers, got %s' % c.dtype)
    try:
        t = float(T)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`T` must be a number of seconds, got %r' % (T,)) from None
    if not math.isfinite(t) or not t > 0.:
        raise ValueError(cerr + '`T` must be finite and > 0 seconds, got %r' % (T,))
    if np.ndim(yx0) != 2 or np.shape(yx0)[1] != 2 or np.shape(yx1) != np.shape(yx0):
        raise ValueError(cerr + '`yx0` and `yx1` must be (nP, 2) arrays of one shape, got %s and %s' % (np.shape(yx0), np.shape(yx1)))
    nP = np.shape(yx0)[0]
    for nm, m in (("mask0", mask0), ("mask1", mask1)):
        if m is not None and np.shape(m) != (nP,):
            raise ValueError(cerr + '`%s` must be (nP,), got %s' % (nm, np.shape(m)))
    out, valid, _ = (ctx or default_context()).deform_cells(yx0, yx1, c, t, mask0, mask1)
    return _as_dict(out, valid)
