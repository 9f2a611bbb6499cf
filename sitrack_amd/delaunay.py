"""Bounded Delaunay triangulation of a buoy cloud: host side of `sitrk_delaunay` (sitrack_amd/csrc/sitrk_delaunay.hip).

An extra the reference does not have.  Every Delaunay triangle of the cloud whose circumradius is at most `rmax_km`, decided on
the GPU by exact integer predicates on positions snapped to 2^-20 km; the rows are what `Tri2Quad` pairs and `DeformCells`
takes.  The contract (vertices, size and reach tests, empty circle, the rule for cocircular points, order of the rows) is in
include/sitrk.h and DESIGN.md 3.13.  There is no host version."""
import math

import numpy as np

RMAX_MAX_KM = 500.


def _rmax(cerr, rmax_km):
    try:
        r = float(rmax_km)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`rmax_km` must be a number in (0, %g], got %r' % (RMAX_MAX_KM, rmax_km)) from None
    if not (math.isfinite(r) and 0. < r <= RMAX_MAX_KM):
        raise ValueError(cerr + '`rmax_km` must be finite and in (0, %g], got %r' % (RMAX_MAX_KM, rmax_km))
    return r


def DelaunayTris(yx, rmax_km, mask=None, ctx=None, return_vertex=False):
    """Triangles (nT, 3) int32 of the points yx (nP, 2) [y,x] km: every Delaunay triangle whose circumradius is at most
    rmax_km.  Runs on the GPU.  mask (nP): 0 = the point is no vertex.  A row (p, q, r) is counter-clockwise (x to the right, y
    up) with p its lowest index; rows are in ascending order of (p, q).  Points that share their coordinates to 2^-20 km count
    once, at their lowest index.  With return_vertex also vertex (nP,) int8: 1 vertex, 0 masked or not finite, 2 duplicate.
    Raises ValueError on bad arguments before any device work."""
    from .tracking import default_context
    cerr = 'ERROR [DelaunayTris()]: '
    r = _rmax(cerr, rmax_km)
    if np.ndim(yx) != 2 or np.shape(yx)[1] != 2:
        raise ValueError(cerr + '`yx` must be an (nP, 2) array, got shape %s' % (np.shape(yx),))
    nP = np.shape(yx)[0]
    if mask is not None and np.shape(mask) != (nP,):
        raise ValueError(cerr + '`mask` must be (nP,), got %s' % (np.shape(mask),))
    tris, _, vertex = (ctx or default_context()).delaunay(yx, r, mask=mask)
    return (tris, vertex) if return_vertex else tris
