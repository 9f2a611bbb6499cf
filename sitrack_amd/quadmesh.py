"""Quadrangles from a triangulated buoy cloud: host side of `sitrk_tri2quad` (sitrack_amd/csrc/sitrk_quadmesh.hip).

An extra the reference does not have.  Adjacent triangles -- `DelaunayTris` of the cloud, scipy's Delaunay, or any (nT, 3) list -- are paired
into strictly convex, near-rectangular quadrangles by a deterministic greedy matching on the GPU; the quadrangles are the
cells `DeformCells` takes.  The contract (canonical form, acceptance tests, score, order) is in include/sitrk.h and
DESIGN.md 3.12.  There is no host version."""
import math

import numpy as np


def _params(cerr, tris, angles, ratio_min, area):
    """the checks every entry point makes before any device work; the library's parameters as keywords"""
    t = np.asarray(tris)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(cerr + '`tris` must be an (nT, 3) array of point indices, got shape %s' % (t.shape,))
    if t.dtype.kind not in "iu":
        raise ValueError(cerr + '`tris` must hold integers, got %s' % t.dtype)
    try:
        lo, hi = (float(a) for a in angles)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`angles` must be (smallest, largest) interior angle in degrees, got %r' % (angles,)) from None
    if not (0. <= lo <= hi <= 180.):
        raise ValueError(cerr + '`angles` must satisfy 0 <= smallest <= largest <= 180 degrees, got %r' % (angles,))
    try:
        r = float(ratio_min)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`ratio_min` must be a number in [0, 1], got %r' % (ratio_min,)) from None
    if not (0. <= r <= 1.):
        raise ValueError(cerr + '`ratio_min` must be in [0, 1], got %r' % (ratio_min,))
    try:
        amin, amax = (float(a) for a in area)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`area` must be (smallest, largest) area in km^2, got %r' % (area,)) from None
    if not (amin <= amax):
        raise ValueError(cerr + '`area` must satisfy smallest <= largest, got %r' % (area,))
    # 90 degrees is exactly 0: cos(pi/2) = 6e-17 would refuse exact rectangles
    cos_lo = 0. if lo == 90. else math.cos(math.radians(lo))
    cos_hi = 0. if hi == 90. else math.cos(math.radians(hi))
    return dict(cos_lo=cos_lo, cos_hi=cos_hi, ratio_min=r, area_min=amin, area_max=amax)


def Tri2Quad(yx, tris, mask=None, angles=(60., 120.), ratio_min=0.5, area=(0., float("inf")), ctx=None):
    """Pairs adjacent triangles `tris` (nT, 3) of the points yx (nP, 2) [y,x] km into quadrangles.  Runs on the GPU.
    mask (nP): 0 = the point is no valid vertex; angles: smallest and largest interior angle allowed [degrees]; ratio_min:
    shortest over longest side, at least; area: smallest and largest area [km^2].
    Returns quads (nQ, 4) int32 -- counter-clockwise, started at the smallest index, ordered by the smaller triangle of each
    pair -- and tri_quad (nT,) int32: the row a triangle went into, -1 where it stayed single, -2 where it is dead (a vertex
    masked or not finite, a repeated index, no area).  Raises ValueError on bad arguments before any device work, IndexError
    for a vertex index outside the points."""
    from .tracking import default_context
    cerr = 'ERROR [Tri2Quad()]: '
    kw = _params(cerr, tris, angles, ratio_min, area)
    if np.ndim(yx) != 2 or np.shape(yx)[1] != 2:
        raise ValueError(cerr + '`yx` must be an (nP, 2) array, got shape %s' % (np.shape(yx),))
    nP = np.shape(yx)[0]
    if mask is not None and np.shape(mask) != (nP,):
        raise ValueError(cerr + '`mask` must be (nP,), got %s' % (np.shape(mask),))
    quads, tri_quad, _ = (ctx or default_context()).tri2quad(yx, tris, mask=mask, **kw)
    return quads, tri_quad
