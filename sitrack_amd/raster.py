"""Buoy cells rasterised onto a regular grid: host side of `sitrk_raster_cells` (sitrack_amd/csrc/sitrk_raster.hip).

An extra the reference does not have: per pixel of a regular grid in the tracker's polar-stereographic plane the lowest-indexed
cell its centre lies in, evaluated in fp64 on the GPU; the contract (centres, inside test, owner) is in include/sitrk.h and
DESIGN.md 3.15.  There is no host version.  A running tracker rasterises its device-resident meshes with
IceTracker.mesh_raster()."""
import math

import numpy as np

MAX_PIXELS = 2 ** 28


def raster_grid(ymin, ymax, xmin, xmax, d_km):
    """The grid (y0, x0, d, ny, nx) of square pixels of side d_km whose pixels cover the box [ymin, ymax] x [xmin, xmax] km and
    whose origin is a multiple of d_km: y0 = floor(ymin/d)*d, ny = ceil((ymax - y0)/d), at least 1; likewise along x.  Two boxes
    rasterised at the same d_km share their pixel lattice."""
    cerr = 'ERROR [raster_grid()]: '
    try:
        v = [float(a) for a in (ymin, ymax, xmin, xmax, d_km)]
    except (TypeError, ValueError):
        raise ValueError(cerr + 'the five arguments must be numbers') from None
    if not all(math.isfinite(a) for a in v):
        raise ValueError(cerr + 'the box and `d_km` must be finite, got %r' % (v,))
    ymin, ymax, xmin, xmax, d = v
    if not d > 0.:
        raise ValueError(cerr + '`d_km` must be > 0, got %r' % (d_km,))
    if ymax < ymin or xmax < xmin:
        raise ValueError(cerr + 'empty box: [%g, %g] x [%g, %g]' % (ymin, ymax, xmin, xmax))
    y0, x0 = math.floor(ymin / d) * d, math.floor(xmin / d) * d
    ny, nx = max(1, math.ceil((ymax - y0) / d)), max(1, math.ceil((xmax - x0) / d))
    return (y0, x0, d, int(ny), int(nx))


def check_grid(grid, cerr=''):
    """the library's grid checks, for callers that must refuse before anything is computed; returns the grid as numbers"""
    try:
        y0, x0, d, ny, nx = grid
        y0, x0, d = float(y0), float(x0), float(d)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`grid` must be (y0_km, x0_km, d_km, ny, nx), got %r' % (grid,)) from None
    if int(ny) != ny or int(nx) != nx:
        raise ValueError(cerr + '`grid`: ny and nx must be integers, got %r, %r' % (ny, nx))
    ny, nx = int(ny), int(nx)
    if not (math.isfinite(y0) and math.isfinite(x0) and math.isfinite(d) and d > 0.):
        raise ValueError(cerr + '`grid`: y0, x0, d must be finite and d > 0, got %r' % (grid,))
    if ny < 1 or nx < 1 or ny * nx > MAX_PIXELS:
        raise ValueError(cerr + '`grid`: needs ny, nx >= 1 and ny*nx <= 2^28 pixels, got %d x %d' % (ny, nx))
    return (y0, x0, d, ny, nx)


def RasterCells(yx, cells, grid, draw=None, ctx=None):
    """owner (ny, nx) int32 of the cells (nC, 3|4) of indices into the points yx (nP,2) [y,x] km, either orientation, on the grid
    (y0_km, x0_km, d_km, ny, nx) (see raster_grid): per pixel the LOWEST index among the cells its centre lies in (the boundary
    counts as inside), -1 for none.  draw (nC): 0 = the cell is not drawn; a cell with a non-finite vertex or no area is never
    drawn.  Runs on the GPU.  Raises ValueError on bad arguments before any device work, IndexError for a vertex index outside
    the points."""
    from .tracking import default_context
    cerr = 'ERROR [RasterCells()]: '
    c = np.asarray(cells)
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError(cerr + '`cells` must be an (nC, 3) or (nC, 4) array of point indices, got shape %s' % (c.shape,))
    if c.dtype.kind not in "iu":
        raise ValueError(cerr + '`cells` must hold integers, got %s' % c.dtype)
    if np.ndim(yx) != 2 or np.shape(yx)[1] != 2:
        raise ValueError(cerr + '`yx` must be an (nP, 2) array, got %s' % (np.shape(yx),))
    if draw is not None and np.shape(draw) != (c.shape[0],):
        raise ValueError(cerr + '`draw` must be (nC,), got %s' % (np.shape(draw),))
    g = check_grid(grid, cerr)
    owner, _ = (ctx or default_context()).raster_cells(yx, c, g, draw)
    return owner
