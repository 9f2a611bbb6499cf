"""Coarse-grained deformation of buoy cells: host side of `sitrk_coarse_cells` (sitrack_amd/csrc/sitrk_coarse.hip).

An extra the reference does not have: the cells' area-weighted velocity gradients summed into the pixels of a regular grid and up
a pyramid of 2x2 boxes, and per level the moments of the total deformation of the boxes -- the spatial scaling curve
<tot^q>(L), L = d*2^l, of one mesh from one call, evaluated in fp64 on the GPU; the contract is in include/sitrk.h and
DESIGN.md 3.16.  There is no host version.  A running tracker coarse-grains its device-resident meshes with
IceTracker.mesh_coarse()."""
import math

import numpy as np

from ._lib import COARSE_MAXLEV, COARSE_NCOLS, COARSE_VALUES

MAX_PIXELS = 2 ** 24


def check_levels(grid, nlev, fmin, cerr=''):
    """the library's checks of a grid that went through raster.check_grid, of nlev and of fmin, for callers that must refuse
    before anything is computed; returns the grid"""
    if grid[3] * grid[4] > MAX_PIXELS:
        raise ValueError(cerr + '`grid`: at most 2^24 pixels can be coarse-grained, got %d x %d' % (grid[3], grid[4]))
    try:
        bad = int(nlev) != nlev
    except (TypeError, ValueError):
        bad = True
    if bad or not 1 <= int(nlev) <= COARSE_MAXLEV:
        raise ValueError(cerr + '`nlev` must be an integer in 1..%d, got %r' % (COARSE_MAXLEV, nlev))
    try:
        f = float(fmin)
    except (TypeError, ValueError):
        f = math.nan
    if not (math.isfinite(f) and f >= 0.):
        raise ValueError(cerr + '`fmin` must be finite and >= 0, got %r' % (fmin,))
    return grid


def name_levels(r):
    """the six (ny_l, nx_l) arrays of every level under their names"""
    if r["levels"] is not None:
        r["levels"] = [dict(zip(COARSE_VALUES, lev)) for lev in r["levels"]]
    return r


def coarse_arg(text, flag='--coarse'):
    """(nlev, fmin) of NLEV[@FMIN]: NLEV an integer in 1..16, FMIN finite >= 0 (default 0.5); ValueError otherwise"""
    tok = text.strip().split('@')
    if len(tok) not in (1, 2):
        raise ValueError("%s: expected NLEV or NLEV@FMIN, got %r" % (flag, text))
    try:
        nlev = int(tok[0])
        fmin = float(tok[1]) if len(tok) == 2 else 0.5
    except ValueError:
        raise ValueError("%s: expected an integer and a number in NLEV[@FMIN], got %r" % (flag, text)) from None
    if not 1 <= nlev <= COARSE_MAXLEV:
        raise ValueError("%s: NLEV must be in 1..%d, got %r" % (flag, COARSE_MAXLEV, text))
    if not (math.isfinite(fmin) and fmin >= 0.):
        raise ValueError("%s: FMIN must be finite and >= 0, got %r" % (flag, text))
    return (nlev, fmin)


def CoarseCells(yx0, yx1, cells, T, grid, nlev, fmin=0.5, mask0=None, mask1=None, use=None, boxes=False, ctx=None):
    """The cells (nC, 3|4) of indices into the points yx0, yx1 (nP, 2) [y,x] km, `T` seconds apart, coarse-grained on `nlev`
    levels over the grid (y0_km, x0_km, d_km, ny, nx) (see raster_grid): each valid cell's area0 and area0 times its four
    velocity gradients are added to the pixel its t0 centroid lies in, in ascending cell index, and every level above sums 2x2
    boxes of the one below.  Returns {"table", "nin", "nout", "levels"}: table (nlev, 8) fp64 under the names _lib.COARSE_COLS --
    per level the boxes with a cell, the FILLED boxes (those whose summed area is > 0 and >= fmin of the box's own) and over the
    filled boxes the sums of A, A*div, A*shr, A*tot, A*tot^2, A*tot^3 of the box-averaged gradients; nin / nout the contributing
    cells inside / outside the grid; levels None or, with boxes=True, per level a dict of (ny_l, nx_l) arrays n, A, AUx, AUy, AVx,
    AVy.  mask0 / mask1 (nP): 0 = invalid vertex; use (nC): 0 = the cell does not contribute.  Runs on the GPU.  Raises
    ValueError on bad arguments before any device work, IndexError for a vertex index outside the points."""
    from .raster import check_grid
    from .tracking import default_context
    cerr = 'ERROR [CoarseCells()]: '
    c = np.asarray(cells)
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError(cerr + '`cells` must be an (nC, 3) or (nC, 4) array of point indices, got shape %s' % (c.shape,))
    if c.dtype.kind not in "iu":
        raise ValueError(cerr + '`cells` must hold integers, got %s' % c.dtype)
    if np.ndim(yx0) != 2 or np.shape(yx0)[1] != 2 or np.shape(yx1) != np.shape(yx0):
        raise ValueError(cerr + '`yx0` and `yx1` must be (nP, 2) arrays of one shape, got %s, %s' % (np.shape(yx0), np.shape(yx1)))
    nP = np.shape(yx0)[0]
    for name, m, n in (("mask0", mask0, nP), ("mask1", mask1, nP), ("use", use, c.shape[0])):
        if m is not None and np.shape(m) != (n,):
            raise ValueError(cerr + '`%s` must be (%d,), got %s' % (name, n, np.shape(m)))
    try:
        T = float(T)
    except (TypeError, ValueError):
        T = math.nan
    if not (math.isfinite(T) and T > 0.):
        raise ValueError(cerr + '`T` must be finite and > 0 seconds, got %r' % (T,))
    g = check_levels(check_grid(grid, cerr), nlev, fmin, cerr)
    r = (ctx or default_context()).coarse_cells(yx0, yx1, c, T, g, int(nlev), fmin=float(fmin), mask0=mask0, mask1=mask1, use=use,
                                                boxes=boxes)
    return name_levels(r)


def scaling_exponents(table, d_km, min_boxes=10):
    """The structure-function exponents of a table of CoarseCells / mesh_coarse: {"beta": (3,), "L_km": (nlev,), "L_eff_km":
    (nlev,), "used": (nlev,) bool}.  beta[q-1], q = 1, 2, 3, is minus the least-squares slope of log(table[:, 4+q]/table[:, 2]) --
    the area-weighted mean of tot^q over the filled boxes -- against log(L_l), L_l = d_km*2^l, over the levels with at least
    `min_boxes` filled boxes and a positive mean; NaN with fewer than two such levels.  L_eff_km = sqrt(table[:, 2]/table[:, 1])
    is the side a filled box of the level really covers (NaN where there is none)."""
    t = np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != COARSE_NCOLS:
        raise ValueError('ERROR [scaling_exponents()]: `table` must be (nlev, %d), got %s' % (COARSE_NCOLS, t.shape))
    d = float(d_km)
    if not (math.isfinite(d) and d > 0.):
        raise ValueError('ERROR [scaling_exponents()]: `d_km` must be finite and > 0, got %r' % (d_km,))
    L = d * 2. ** np.arange(t.shape[0])
    with np.errstate(divide='ignore', invalid='ignore'):
        Leff = np.sqrt(t[:, 2] / t[:, 1])
        mean = t[:, 5:8] / t[:, 2:3]
    used = (t[:, 1] >= min_boxes) & (t[:, 1] >= 1) & np.all(np.isfinite(mean) & (mean > 0.), axis=1)
    beta = np.full(3, np.nan)
    if used.sum() >= 2:
        x = np.log(L[used])
        for q in range(3):
            beta[q] = -np.polyfit(x, np.log(mean[used, q]), 1)[0]
    return {"beta": beta, "L_km": L, "L_eff_km": Leff, "used": used}
