"""Distance to the model's own coastline and the coastal cleaning of a point cloud (an extra the reference does not have: its
`ldo_coastal_clean` reads a rasterised dist2coast file through mojito's `MaskCoastal`).

The coast is the set of T-cell edges between a sea cell and a land cell of the mesh handed to `Context.coast_build`; distances
are kilometres in the polar-stereographic plane the tracker works in (true at 70 N, not corrected: include/sitrk.h)."""
import numpy as np

from .tracking import default_context, Geo2CartNPSkm1D


def seg_d2(yx, ab):
    """The contract's squared distance (include/sitrk.h) of the points yx (n,2) to the segments ab (n,2,2), pairwise: numpy
    rounds every operation once and fuses none, so this equals the device's value bit for bit."""
    yx = np.asarray(yx, dtype=np.float64)
    ab = np.asarray(ab, dtype=np.float64)
    ey = ab[:, 1, 0] - ab[:, 0, 0]; ex = ab[:, 1, 1] - ab[:, 0, 1]
    py = yx[:, 0] - ab[:, 0, 0]; px = yx[:, 1] - ab[:, 0, 1]
    len2 = ey * ey + ex * ex
    dot = py * ey + px * ex
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(len2 > 0., dot / len2, 0.)
    t = np.where(t < 0., 0., np.where(t > 1., 1., t))
    cy = py - t * ey; cx = px - t * ex
    return cy * cy + cx * cx


def DistToCoast(yx, ctx=None, rmax_km=None, return_seg=False):
    """Distance [km] of the points yx (n,2) [y,x] km to the coast of the index built by `ctx.coast_build(...)`.  With
    `rmax_km`, points further than that report +inf (and segment -1); points with a non-finite coordinate report NaN.
    `return_seg`: also the id 2*(j*Ni+i)+k of the nearest segment (lowest id on ties)."""
    ctx = ctx or default_context()
    dist, seg = ctx.coast_dist(yx, rmax_km, want_seg=return_seg)
    return (dist, seg) if return_seg else dist


def MaskCoastal(pCoorGC, rMinDistLand=100., ctx=None):
    """mojito's MaskCoastal as the reference seeding tools call it, on the model's own coastline: pCoorGC (n,2) [lat,lon]
    degrees -> (n,) int8, 1 = keep.  A point is kept iff its squared distance to the coast is >= rMinDistLand**2 -- decided
    on the squared distance of the contract, no square root takes part -- so a point at exactly rMinDistLand is kept; a point
    that does not project to finite coordinates is dropped.  Needs `ctx.coast_build(...)` first."""
    ctx = ctx or default_context()
    r = float(rMinDistLand)
    if not (np.isfinite(r) and r > 0.):
        raise ValueError("MaskCoastal: rMinDistLand must be finite and > 0 km (got %r)" % (rMinDistLand,))
    g = np.asarray(pCoorGC, dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != 2:
        raise ValueError("MaskCoastal: pCoorGC must be (n,2) [lat,lon]")
    yx = Geo2CartNPSkm1D(g, ctx=ctx) if len(g) else np.zeros((0, 2))
    return mask_coastal_yx(yx, r, ctx)


def mask_coastal_yx(yx, r, ctx):
    """MaskCoastal's rule on plane coordinates yx (n,2) km: the query is bounded by rmax_km = r, so a point beyond it comes
    back as +inf and is kept; for the others the squared distance to the reported segment is recomputed and compared."""
    yx = np.ascontiguousarray(yx, dtype=np.float64)
    dist, seg = ctx.coast_dist(yx, r, want_seg=True)
    keep = np.isposinf(dist)
    near = np.flatnonzero(seg >= 0)
    if len(near):
        ids, ab = ctx.coast_segments()
        d2 = seg_d2(yx[near], ab[np.searchsorted(ids, seg[near])])
        keep[near] = d2 >= r * r
    return keep.astype(np.int8)
