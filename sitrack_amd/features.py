"""Features of a map: host side of `sitrk_label_raster` / `sitrk_mesh_features` (sitrack_amd/csrc/sitrk_label.hip).

An extra the reference does not have: the connected components of a mask on a regular grid -- the leads, ridges and linear
kinematic features of a deformation map -- labelled on the GPU, one row of twelve integers per feature coming down instead of
the map; the contract is in include/sitrk.h and DESIGN.md 3.17.  There is no host version.  A running tracker labels the map of
its device-resident meshes with IceTracker.mesh_features(); feature_table() turns the integer rows into areas, centroids,
lengths, widths and orientations."""
import math

import numpy as np

from ._lib import FEAT_COLS, FEAT_NCOLS, FEAT_WHAT

MAX_SIDE = 32768
MAX_PIXELS = 2 ** 28
# WHAT of --deform-features -> (what, sgn) of sitrk_mesh_features
FEATURE_KINDS = {"div": ("div", 1), "conv": ("div", -1), "shr": ("shr", 1), "vor": ("vor", 1), "tot": ("tot", 1)}


def _as_int(v, name, cerr):
    try:
        bad = int(v) != v
    except (TypeError, ValueError):
        bad = True
    if bad:
        raise ValueError(cerr + '`%s` must be an integer, got %r' % (name, v))
    return int(v)


def check_label_args(ny, nx, conn, min_pix, maxfeat, cerr=''):
    """the library's checks of a raster's shape, conn, min_pix and maxfeat, for callers that must refuse before anything is
    computed; returns (conn, min_pix, maxfeat) as integers"""
    if not (1 <= ny <= MAX_SIDE and 1 <= nx <= MAX_SIDE) or ny * nx > MAX_PIXELS:
        raise ValueError(cerr + 'a raster to label needs 1 <= ny, nx <= 32768 and ny*nx <= 2^28 pixels, got %d x %d' % (ny, nx))
    conn, min_pix, maxfeat = _as_int(conn, "conn", cerr), _as_int(min_pix, "min_pix", cerr), _as_int(maxfeat, "maxfeat", cerr)
    if conn not in (4, 8):
        raise ValueError(cerr + '`conn` must be 4 (edge neighbours) or 8 (edge and corner neighbours), got %r' % (conn,))
    if min_pix < 1:
        raise ValueError(cerr + '`min_pix` must be >= 1, got %r' % (min_pix,))
    if maxfeat < 0:
        raise ValueError(cerr + '`maxfeat` must be >= 0, got %r' % (maxfeat,))
    return conn, min_pix, maxfeat


def check_test(what, sgn, thr, cerr=''):
    """the library's checks of the test of sitrk_mesh_features; returns (what as 0..3, sgn, thr)"""
    if what not in FEAT_WHAT:
        raise ValueError(cerr + '`what` must be one of %s, got %r' % (", ".join(sorted(FEAT_WHAT)), what))
    if sgn not in (1, -1):
        raise ValueError(cerr + '`sgn` must be +1 or -1, got %r' % (sgn,))
    try:
        thr = float(thr)
    except (TypeError, ValueError):
        thr = math.nan
    if not math.isfinite(thr):
        raise ValueError(cerr + '`thr` must be a finite number, got %r' % (thr,))
    if what == "tot" and (sgn != 1 or thr < 0.):
        raise ValueError(cerr + 'what="tot" needs sgn = +1 and thr >= 0, got %r, %r' % (sgn, thr))
    return FEAT_WHAT[what], int(sgn), thr


def features_arg(text, flag='--deform-features'):
    """(what, sgn, thr, min_pix, conn) of WHAT@THR[@MINPIX[@CONN]]: WHAT one of div, conv (div with sgn -1), shr, vor, tot; THR
    finite (tot: >= 0), in the unit of the rates; MINPIX an integer >= 1 (default 1); CONN 4 or 8 (default 8).  ValueError
    otherwise."""
    tok = text.strip().split('@')
    if len(tok) not in (2, 3, 4):
        raise ValueError("%s: expected WHAT@THR[@MINPIX[@CONN]], got %r" % (flag, text))
    if tok[0] not in FEATURE_KINDS:
        raise ValueError("%s: WHAT must be one of %s, got %r" % (flag, ", ".join(FEATURE_KINDS), text))
    what, sgn = FEATURE_KINDS[tok[0]]
    try:
        thr = float(tok[1])
        min_pix = int(tok[2]) if len(tok) > 2 else 1
        conn = int(tok[3]) if len(tok) > 3 else 8
    except ValueError:
        raise ValueError("%s: expected a number and integers in WHAT@THR[@MINPIX[@CONN]], got %r" % (flag, text)) from None
    if not math.isfinite(thr):
        raise ValueError("%s: THR must be finite, got %r" % (flag, text))
    if what == "tot" and thr < 0.:
        raise ValueError("%s: THR of tot must be >= 0, got %r" % (flag, text))
    if min_pix < 1:
        raise ValueError("%s: MINPIX must be >= 1, got %r" % (flag, text))
    if conn not in (4, 8):
        raise ValueError("%s: CONN must be 4 or 8, got %r" % (flag, text))
    return (what, sgn, thr, min_pix, conn)


def check_features_grid(grid, flag='--deform-features'):
    """a grid that went through raster.check_grid, refused above 32768 pixels a side; returns it"""
    if grid[3] > MAX_SIDE or grid[4] > MAX_SIDE:
        raise ValueError("%s: at most 32768 pixels a side can be labelled, the grid has %d x %d" % (flag, grid[3], grid[4]))
    return grid


def LabelRaster(active, conn=8, min_pix=1, maxfeat=65536, ctx=None):
    """The connected components of the mask `active` (ny, nx) -- a pixel is active iff its value is not 0 -- for conn = 4 (edge
    neighbours) or 8 (edge and corner neighbours).  Returns {"labels", "table", "nfeat", "ncomp", "nactive"}: labels (ny, nx)
    int32, -1 for an inactive pixel, else the LOWEST linear index j*nx + i of the pixel's component; table (rows, 12) int64 under
    the names _lib.FEAT_COLS, one row per component of at least `min_pix` pixels in ascending label, at most `maxfeat` rows;
    nfeat the number of such components (above maxfeat the table is truncated), ncomp all components, nactive the active pixels.
    Runs on the GPU.  Raises ValueError on bad arguments before any device work."""
    from .tracking import default_context
    cerr = 'ERROR [LabelRaster()]: '
    a = np.asarray(active)
    if a.ndim != 2:
        raise ValueError(cerr + '`active` must be an (ny, nx) array, got shape %s' % (a.shape,))
    conn, min_pix, maxfeat = check_label_args(a.shape[0], a.shape[1], conn, min_pix, maxfeat, cerr)
    return (ctx or default_context()).label_raster(a, conn=conn, min_pix=min_pix, maxfeat=maxfeat, labels=True)


def feature_table(table, grid):
    """Per row of a table of LabelRaster / mesh_features on the grid (y0_km, x0_km, d_km, ny, nx), a dict of (rows,) arrays: label,
    npix; area_km2 = npix*d^2; y_km, x_km the centroid, y0 + (sum_j/npix + 0.5)*d and likewise along x; length_km =
    d*sqrt(12*l1) and width_km = d*sqrt(12*l2), l1 >= l2 the eigenvalues of the covariance of the pixel centres plus 1/12 per
    axis (a pixel's own extent: a bar of n x 1 pixels is n*d long and d wide); angle [rad] = 0.5*atan2(2*cji, cii - cjj), the
    direction of the long axis from the x axis, in (-pi/2, pi/2]; perimeter_km = perimeter*d; jmin, jmax, imin, imax."""
    from .raster import check_grid
    cerr = 'ERROR [feature_table()]: '
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != FEAT_NCOLS or t.dtype.kind not in "iu":
        raise ValueError(cerr + '`table` must be (rows, %d) integers, got %s %s' % (FEAT_NCOLS, t.shape, t.dtype))
    y0, x0, d, _, _ = check_grid(grid, cerr)
    c = dict(zip(FEAT_COLS, (t[:, k] for k in range(FEAT_NCOLS))))
    n = c["npix"].astype(np.float64)
    if np.any(c["npix"] < 1):
        raise ValueError(cerr + 'every row must have npix >= 1')
    mj, mi = c["sum_j"] / n, c["sum_i"] / n
    # the second moments about the centroid from integers: n*sum(j^2) - (sum j)^2 is exact in Python integers, not in fp64
    nn = [int(v) for v in c["npix"]]
    def central(sab, sa, sb):
        return np.array([(k * int(ab) - int(a) * int(b)) / (k * k) for k, ab, a, b in zip(nn, sab, sa, sb)], dtype=np.float64)
    cjj = central(c["sum_jj"], c["sum_j"], c["sum_j"]) + 1. / 12.
    cii = central(c["sum_ii"], c["sum_i"], c["sum_i"]) + 1. / 12.
    cji = central(c["sum_ji"], c["sum_j"], c["sum_i"])
    half, diff = 0.5 * (cii + cjj), 0.5 * (cii - cjj)
    root = np.hypot(diff, cji)
    l1 = half + root                                                   # >= 1/12; l2 from the determinant: half - root would cancel
    l2 = np.maximum(cii * cjj - cji * cji, 0.) / l1
    return {"label": c["label"].copy(), "npix": c["npix"].copy(), "area_km2": n * (d * d),
            "y_km": y0 + (mj + 0.5) * d, "x_km": x0 + (mi + 0.5) * d,
            "length_km": d * np.sqrt(12. * l1), "width_km": d * np.sqrt(12. * l2),
            "angle": 0.5 * np.arctan2(2. * cji, cii - cjj), "perimeter_km": c["perimeter"] * d,
            "jmin": c["jmin"].copy(), "jmax": c["jmax"].copy(), "imin": c["imin"].copy(), "imax": c["imax"].copy()}
