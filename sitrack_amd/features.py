"""Features of a map: host side of `sitrk_label_raster` / `sitrk_mesh_features` (sitrack_amd/csrc/sitrk_label.hip).

An extra the reference does not have: the connected components of a mask on a regular grid -- the leads, ridges and linear
kinematic features of a deformation map -- labelled on the GPU, one row of twelve integers per feature coming down instead of
the map; the contract is in include/sitrk.h and DESIGN.md 3.17.  There is no host version.  A running tracker labels the map of
its device-resident meshes with IceTracker.mesh_features(); feature_table() turns the integer rows into areas, centroids,
lengths, widths and orientations.

Features from window to window (sitrack_amd/csrc/sitrk_track.hip): IceTracker.mesh_features(keep=...),
features_advect() and features_match() keep, carry and compare label maps on the device; MatchLabels() compares two host maps
the same way; link_features() and feature_tracks() turn the pair tables into parents, children and tracks, on the host and in
integers.

Skeletons (sitrack_amd/csrc/sitrk_skeleton.hip): SkeletonRaster() and IceTracker.features_skeleton() thin the
features of a label map to lines one pixel wide on the device; skeleton_table() turns the integer rows into lengths along the
features, node_yx() the node list into positions."""
import math

import numpy as np

from .distribution import Percentile, percentile_arg
from ._lib import FEAT_COLS, FEAT_NCOLS, FEAT_WHAT, KEEP_MAX, MATCH_MAXREACH, MATCH_MAXSHIFT, SKEL_COLS, SKEL_MAXSUB, SKEL_NCOLS

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
    finite (tot: >= 0), in the unit of the rates, or pNN, which gives distribution.Percentile(NN), NN in [0, 100]; MINPIX an
    integer >= 1 (default 1); CONN 4 or 8 (default 8).  ValueError otherwise."""
    tok = text.strip().split('@')
    if len(tok) not in (2, 3, 4):
        raise ValueError("%s: expected WHAT@THR[@MINPIX[@CONN]], got %r" % (flag, text))
    if tok[0] not in FEATURE_KINDS:
        raise ValueError("%s: WHAT must be one of %s, got %r" % (flag, ", ".join(FEATURE_KINDS), text))
    what, sgn = FEATURE_KINDS[tok[0]]
    # pNN: the NN-th percentile of the rate over the cells, resolved on the device where the threshold is needed
    pct = percentile_arg(tok[1], flag) if tok[1][:1] == 'p' else None
    try:
        thr = pct if pct is not None else float(tok[1])
        min_pix = int(tok[2]) if len(tok) > 2 else 1
        conn = int(tok[3]) if len(tok) > 3 else 8
    except ValueError:
        raise ValueError("%s: expected a number and integers in WHAT@THR[@MINPIX[@CONN]], got %r" % (flag, text)) from None
    if not isinstance(thr, Percentile):
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


# ------------------------------------------------------------------------------------------------ features from window to window
def check_keep(keep, name="keep", cerr=''):
    """a slot of the kept maps as an integer in 0..KEEP_MAX-1"""
    k = _as_int(keep, name, cerr)
    if not 0 <= k < KEEP_MAX:
        raise ValueError(cerr + '`%s` must be in 0..%d, got %r' % (name, KEEP_MAX - 1, keep))
    return k


def check_match_args(reach, dj, di, maxpair, cerr=''):
    """the library's checks of reach, shift and maxpair of sitrk_features_match; returns them as integers"""
    reach, dj, di, maxpair = (_as_int(v, n, cerr) for v, n in ((reach, "reach"), (dj, "dj"), (di, "di"), (maxpair, "maxpair")))
    if not 0 <= reach <= MATCH_MAXREACH:
        raise ValueError(cerr + '`reach` must be in 0..%d pixels, got %r' % (MATCH_MAXREACH, reach))
    if abs(dj) > MATCH_MAXSHIFT or abs(di) > MATCH_MAXSHIFT:
        raise ValueError(cerr + 'the shift `dj`, `di` must be within +-%d pixels, got %r, %r' % (MATCH_MAXSHIFT, dj, di))
    if maxpair < 0:
        raise ValueError(cerr + '`maxpair` must be >= 0, got %r' % (maxpair,))
    return reach, dj, di, maxpair


def track_arg(text, flag='--deform-track'):
    """REACH of --deform-track [REACH]: an integer in 0..MATCH_MAXREACH.  ValueError otherwise."""
    try:
        reach = int(text)
    except (TypeError, ValueError):
        raise ValueError("%s: REACH must be an integer number of pixels, got %r" % (flag, text)) from None
    if not 0 <= reach <= MATCH_MAXREACH:
        raise ValueError("%s: REACH must be in 0..%d pixels, got %r" % (flag, MATCH_MAXREACH, text))
    return reach


def _label_map(a, name, cerr):
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype.kind not in "iu":
        raise ValueError(cerr + '`%s` must be an (ny, nx) array of integers, got %s %s' % (name, a.shape, a.dtype))
    return a


def MatchLabels(mapA, mapB, reach=0, dj=0, di=0, maxpair=1 << 20, ctx=None):
    """The features of two label maps (ny, nx) -- every value -1 or a label in [0, ny*nx), as LabelRaster gives them -- that meet:
    for every pixel p of mapA with a label a, the distinct labels b of mapB within `reach` pixels (0..2) of p shifted by (dj, di)
    count once for the pair (a, b).  Returns {"pairs": (rows, 3) int64 rows (a, b, count) in ascending (a, b), at most maxpair of
    them, "npair": all such rows, "nhit": the pixels of mapA that meet a feature of mapB}.  With reach = 0 this is the pixel
    overlap.  Runs on the GPU: two kept maps (slots KEEP_MAX-2 and KEEP_MAX-1 of the context, freed again) and
    sitrk_features_match.  Raises ValueError on bad arguments before any device work."""
    from .tracking import default_context
    cerr = 'ERROR [MatchLabels()]: '
    a, b = _label_map(mapA, "mapA", cerr), _label_map(mapB, "mapB", cerr)
    if a.shape != b.shape:
        raise ValueError(cerr + 'the two maps must have one shape, got %s and %s' % (a.shape, b.shape))
    check_label_args(a.shape[0], a.shape[1], 8, 1, 0, cerr)
    reach, dj, di, maxpair = check_match_args(reach, dj, di, maxpair, cerr)
    c = ctx or default_context()
    sa, sb = KEEP_MAX - 2, KEEP_MAX - 1
    try:
        c.keep_put(sa, a)
        c.keep_put(sb, b)
        return c.features_match(sa, sb, reach=reach, dj=dj, di=di, maxpair=maxpair)
    finally:
        c.keep_free(sa)
        c.keep_free(sb)


def kept_labels(labels, min_pix=1):
    """what sitrk_mesh_features_keep keeps of a label map: the label where the pixel's component has at least min_pix pixels,
    else -1 (host, numpy)"""
    lab = np.asarray(labels)
    act = lab >= 0
    npix = np.bincount(lab[act].astype(np.int64), minlength=max(lab.size, 1))
    return np.where(act & (npix[np.maximum(lab, 0)] >= min_pix), lab, -1).astype(np.int32)


def advect_labels(labels, owner0, owner1, ncells):
    """the host counterpart of sitrk_mesh_features_advect for maps that are on the host already (numpy): cell q takes the lowest
    label >= 0 among the pixels with owner0 == q, and gives it to the pixels with owner1 == q; -1 where there is none.  Returns
    (M (ny, nx) int32, cellfeat (ncells,) int32)."""
    lab, o0, o1 = np.asarray(labels), np.asarray(owner0), np.asarray(owner1)
    if not (lab.shape == o0.shape == o1.shape):
        raise ValueError('ERROR [advect_labels()]: the three maps must have one shape, got %s, %s, %s' % (lab.shape, o0.shape, o1.shape))
    big = np.iinfo(np.int32).max
    cellfeat = np.full(int(ncells), big, dtype=np.int32)
    use = (o0 >= 0) & (lab >= 0)
    np.minimum.at(cellfeat, o0[use], lab[use].astype(np.int32))
    cellfeat[cellfeat == big] = -1
    M = np.where(o1 >= 0, cellfeat[np.maximum(o1, 0)] if ncells else -1, -1).astype(np.int32)
    return M, cellfeat


def link_features(pairs, tableA, tableB, min_overlap=1):
    """The links between the features of two windows from the rows (a, b, count) of a match of A (the earlier map) against B and
    the two feature tables (rows, >= 1) whose column 0 is the label in ascending order.  Pairs with count < min_overlap are no
    links.  Returns a dict of int64 arrays: parent (rowsB,) the row in tableA of the A feature with the largest count into that B
    feature, ties to the lowest label, -1 for none; child (rowsA,) likewise from the A side, a row of tableB; nparents (rowsB,)
    and nchildren (rowsA,) the number of links (the merge and the split degree); and dropped: the pairs that name a label absent
    from its table (a table truncated by maxfeat), which are ignored."""
    cerr = 'ERROR [link_features()]: '
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 3 or (p.size and p.dtype.kind not in "iu"):
        raise ValueError(cerr + '`pairs` must be (rows, 3) integers, got %s %s' % (p.shape, p.dtype))
    p = p.astype(np.int64).reshape(-1, 3)
    labs = []
    for t, name in ((tableA, "tableA"), (tableB, "tableB")):
        t = np.asarray(t)
        if t.ndim != 2 or t.shape[1] < 1 or (t.size and t.dtype.kind not in "iu"):
            raise ValueError(cerr + '`%s` must be (rows, >= 1) integers, got %s %s' % (name, t.shape, t.dtype))
        lab = t[:, 0].astype(np.int64)
        if np.any(lab[1:] <= lab[:-1]):
            raise ValueError(cerr + 'the labels of `%s` must ascend strictly' % name)
        labs.append(lab)
    min_overlap = _as_int(min_overlap, "min_overlap", cerr)
    la, lb = labs

    def row_of(lab, v):
        if not len(lab):
            return np.full(len(v), -1, dtype=np.int64)
        r = np.minimum(np.searchsorted(lab, v), len(lab) - 1)
        return np.where(lab[r] == v, r, -1).astype(np.int64)

    p = p[p[:, 2] >= min_overlap]
    ra, rb = row_of(la, p[:, 0]), row_of(lb, p[:, 1])
    known = (ra >= 0) & (rb >= 0)
    dropped = int((~known).sum())
    ra, rb, cnt = ra[known], rb[known], p[known, 2]

    def best(mine, other, n):
        """per row of `mine`: the row of `other` with the largest count, the lowest on a tie; and the number of links"""
        out = np.full(n, -1, dtype=np.int64)
        order = np.lexsort((other, -cnt, mine))                        # by mine, then falling count, then rising other
        m = mine[order]
        first = np.ones(len(m), dtype=bool)
        first[1:] = m[1:] != m[:-1]
        out[m[first]] = other[order][first]
        return out, np.bincount(mine, minlength=n).astype(np.int64)

    parent, nparents = best(rb, ra, len(lb))
    child, nchildren = best(ra, rb, len(la))
    return {"parent": parent, "child": child, "nparents": nparents, "nchildren": nchildren, "dropped": dropped}


def feature_tracks(links, nrows):
    """Tracks through the windows of a series: nrows[k] = the features (table rows) of window k, links[k] = link_features() of
    window k against window k+1 (len(nrows) - 1 of them).  A feature continues the track of its parent iff it is also that
    parent's child; otherwise it starts a new track.  Track ids are handed out in window order, then row order, from 0.  Returns
    (track, age): per window an int64 array of track ids and one of ages, the windows the track has lived before this one."""
    cerr = 'ERROR [feature_tracks()]: '
    nrows = [_as_int(n, "nrows", cerr) for n in nrows]
    if len(links) != max(len(nrows) - 1, 0):
        raise ValueError(cerr + '%d windows need %d links, got %d' % (len(nrows), max(len(nrows) - 1, 0), len(links)))
    track, age, nxt = [], [], 0
    for k, n in enumerate(nrows):
        t, a = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
        if k > 0:
            par, chi = np.asarray(links[k - 1]["parent"]), np.asarray(links[k - 1]["child"])
            if len(par) != n or len(chi) != nrows[k - 1]:
                raise ValueError(cerr + 'links[%d] does not fit the rows of windows %d and %d' % (k - 1, k - 1, k))
            has = par >= 0
            cont = np.zeros(n, dtype=bool)
            cont[has] = chi[par[has]] == np.flatnonzero(has)
            t[cont] = track[k - 1][par[cont]]
            a[cont] = age[k - 1][par[cont]] + 1
        new = t < 0
        t[new] = nxt + np.arange(int(new.sum()), dtype=np.int64)
        nxt += int(new.sum())
        track.append(t)
        age.append(a)
    return track, age


def track_events(link, track_prev, track_next):
    """(continued, born, ended, merged, split) between two windows: features of the later window that continue a track, that
    start one, tracks of the earlier window that are not continued, features of the later window with more than one parent,
    features of the earlier one with more than one child"""
    cont = int(np.isin(track_next, track_prev).sum()) if len(track_prev) else 0
    return (cont, len(track_next) - cont, len(track_prev) - cont, int((np.asarray(link["nparents"]) > 1).sum()),
            int((np.asarray(link["nchildren"]) > 1).sum()))


# ------------------------------------------------------------------------------------------------ skeletons
SKEL_DEFAULT_MAXSUB = 4096


def check_skeleton_args(max_sub, maxfeat, maxnode, cerr=''):
    """the library's checks of max_sub, maxfeat and maxnode of the skeleton calls; returns them as integers"""
    max_sub, maxfeat, maxnode = (_as_int(v, n, cerr) for v, n in ((max_sub, "max_sub"), (maxfeat, "maxfeat"), (maxnode, "maxnode")))
    if not 1 <= max_sub <= SKEL_MAXSUB:
        raise ValueError(cerr + '`max_sub` must be in 1..%d sub-iterations, got %r' % (SKEL_MAXSUB, max_sub))
    if maxfeat < 0:
        raise ValueError(cerr + '`maxfeat` must be >= 0, got %r' % (maxfeat,))
    if maxnode < 0:
        raise ValueError(cerr + '`maxnode` must be >= 0, got %r' % (maxnode,))
    return max_sub, maxfeat, maxnode


def skeleton_arg(text, flag='--deform-skeleton'):
    """MAXSUB of --deform-skeleton [MAXSUB]: an integer in 1..2^20.  ValueError otherwise."""
    try:
        max_sub = int(text)
    except (TypeError, ValueError):
        raise ValueError("%s: MAXSUB must be an integer number of sub-iterations, got %r" % (flag, text)) from None
    if not 1 <= max_sub <= SKEL_MAXSUB:
        raise ValueError("%s: MAXSUB must be in 1..%d sub-iterations, got %r" % (flag, SKEL_MAXSUB, text))
    return max_sub


def SkeletonRaster(map_or_mask, conn=8, max_sub=SKEL_DEFAULT_MAXSUB, maxfeat=65536, maxnode=1 << 20, ctx=None):
    """The skeleton of the features of a raster (ny, nx).  A bool or int8 array is a mask and is labelled first with
    LabelRaster(mask, conn); an int32 array is taken as a label map, every value -1 or a label in [0, ny*nx).  The mask of the
    labelled pixels is thinned by Guo and Hall's two-sub-iteration algorithm, at most `max_sub` sub-iterations of it.  Returns
    {"table", "nodes", "nfeat", "nnode", "nskel", "nsub", "converged", "skel", "labels"}: table (rows, 7) int64 under the names
    _lib.SKEL_COLS, one row per label in ascending order, at most maxfeat rows; nodes (rows, 3) int64 rows (p, label, X) of the
    skeleton pixels that are no plain line pixel (X = 1 an end, X >= 3 a junction, X = 0 an isolated pixel) in ascending
    p = j*nx + i, at most maxnode rows; skel (ny, nx) int8; labels the map that was thinned.  converged = 0: max_sub was too
    small to see the thinning end.  Runs on the GPU.  Raises ValueError on bad arguments before any device work."""
    from .tracking import default_context
    cerr = 'ERROR [SkeletonRaster()]: '
    a = np.asarray(map_or_mask)
    if a.ndim != 2 or a.dtype not in (np.dtype(bool), np.dtype(np.int8), np.dtype(np.int32)):
        raise ValueError(cerr + 'expected an (ny, nx) mask of bool or int8, or a label map of int32, got %s %s' % (a.shape, a.dtype))
    conn, _, _ = check_label_args(a.shape[0], a.shape[1], conn, 1, 0, cerr)
    max_sub, maxfeat, maxnode = check_skeleton_args(max_sub, maxfeat, maxnode, cerr)
    c = ctx or default_context()
    if a.dtype != np.dtype(np.int32):
        a = c.label_raster(a, conn=conn, min_pix=1, maxfeat=0, labels=True)["labels"]
    r = c.skeleton_raster(a, max_sub=max_sub, maxfeat=maxfeat, maxnode=maxnode, skel=True)
    r["labels"] = a
    return r


def skeleton_table(table, grid):
    """Per row of a skeleton table on the grid (y0_km, x0_km, d_km, ny, nx), a dict of (rows,) arrays: label, npix, nskel, n_end,
    n_junc, north, ndiag and length_km = d*(north + sqrt(2)*ndiag), the length along the skeleton.  It counts LINKS, not pixels:
    a straight row of n skeleton pixels is (n - 1)*d long, an isolated pixel 0."""
    from .raster import check_grid
    cerr = 'ERROR [skeleton_table()]: '
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != SKEL_NCOLS or t.dtype.kind not in "iu":
        raise ValueError(cerr + '`table` must be (rows, %d) integers, got %s %s' % (SKEL_NCOLS, t.shape, t.dtype))
    _, _, d, _, _ = check_grid(grid, cerr)
    c = dict(zip(SKEL_COLS, (t[:, k].copy() for k in range(SKEL_NCOLS))))
    return {"label": c["label"], "npix": c["npix"], "nskel": c["nskel"], "n_end": c["nend"], "n_junc": c["njunc"],
            "north": c["north"], "ndiag": c["ndiag"], "length_km": d * (c["north"] + math.sqrt(2.) * c["ndiag"])}


def node_yx(nodes, grid):
    """(rows, 2) [y, x] km: the pixel centres of the rows (p, label, X) of a node list on the grid (y0_km, x0_km, d_km, ny, nx)"""
    from .raster import check_grid
    cerr = 'ERROR [node_yx()]: '
    n = np.asarray(nodes)
    if n.ndim != 2 or n.shape[1] != 3 or (n.size and n.dtype.kind not in "iu"):
        raise ValueError(cerr + '`nodes` must be (rows, 3) integers, got %s %s' % (n.shape, n.dtype))
    y0, x0, d, ny, nx = check_grid(grid, cerr)
    p = n[:, 0].astype(np.int64)
    if np.any((p < 0) | (p >= ny * nx)):
        raise ValueError(cerr + 'a node lies outside the %d x %d grid' % (ny, nx))
    return np.stack([y0 + (p // nx + 0.5) * d, x0 + (p % nx + 0.5) * d], axis=1)
