"""Dispersion of buoy pairs: host side of `sitrk_pairs_points` (sitrack_amd/csrc/sitrk_pairs.hip).

An extra the reference does not have: for every pair of points a distance r0 apart at t0 the strain e = (r1 - r0)/r0 of their
separation at t1, and per class of r0 the sums of e, |e|, e^2, |e|^3 and (r1 - r0)^2 -- the buoy-dispersion analysis of sea-ice
deformation (Rampal et al. 2008) with no mesh and no grid, evaluated in fp64 on the GPU; the contract is in include/sitrk.h and
DESIGN.md 3.20.  There is no host version.  A running tracker takes the tables from its device-resident positions with
IceTracker.pairs_mark() / IceTracker.pairs()."""
import math

import numpy as np

from ._lib import PAIRS_MAXCLASS, PAIRS_NCOLS


def check_edges(edges_km, cerr=''):
    """the library's checks of the class edges, for callers that must refuse before anything is computed; returns them as a
    (nc + 1,) float64 array"""
    try:
        e = np.array(edges_km, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`edges_km` must be a sequence of numbers, got %r' % (edges_km,)) from None
    if e.ndim != 1 or not 2 <= e.shape[0] <= PAIRS_MAXCLASS + 1:
        raise ValueError(cerr + '`edges_km` must hold the nc + 1 edges of 1..%d classes, got shape %s' % (PAIRS_MAXCLASS, e.shape))
    if not np.isfinite(e).all():
        raise ValueError(cerr + '`edges_km` must be finite, got %r' % (e.tolist(),))
    if not (e[0] >= 0. and (np.diff(e) > 0.).all()):
        raise ValueError(cerr + '`edges_km` must start at >= 0 and increase strictly, got %r' % (e.tolist(),))
    return e


def pair_edges(r_lo, r_hi, nc):
    """nc + 1 geometric class edges from r_lo to r_hi km: edges[c] = r_lo*(r_hi/r_lo)**(c/nc), the two ends exact"""
    try:
        lo, hi = float(r_lo), float(r_hi)
        bad = int(nc) != nc
    except (TypeError, ValueError):
        raise ValueError('ERROR [pair_edges()]: expected two numbers and an integer, got %r, %r, %r' % (r_lo, r_hi, nc)) from None
    if bad or not 1 <= int(nc) <= PAIRS_MAXCLASS:
        raise ValueError('ERROR [pair_edges()]: `nc` must be an integer in 1..%d, got %r' % (PAIRS_MAXCLASS, nc))
    if not (math.isfinite(lo) and math.isfinite(hi) and 0. < lo < hi):
        raise ValueError('ERROR [pair_edges()]: need 0 < r_lo < r_hi, both finite, got %r, %r' % (r_lo, r_hi))
    nc = int(nc)
    e = lo * (hi / lo) ** (np.arange(nc + 1) / nc)
    e[0], e[nc] = lo, hi
    return check_edges(e, 'ERROR [pair_edges()]: ')


def pairs_arg(text, flag='--pairs'):
    """the class edges of R_LO:R_HI:NC (geometric, see pair_edges) or of an explicit list e0,e1,...; ValueError otherwise"""
    t = text.strip()
    try:
        if ':' in t:
            tok = t.split(':')
            if len(tok) != 3:
                raise ValueError
            return pair_edges(float(tok[0]), float(tok[1]), int(tok[2]))
        vals = [float(x) for x in t.split(',')]
    except ValueError as err:
        raise ValueError("%s: expected R_LO:R_HI:NC or e0,e1,..., got %r%s" % (flag, text, (" (%s)" % err) if str(err) else "")) from None
    return check_edges(vals, flag + ': ')


def PairDispersion(yx0, yx1, edges_km, mask0=None, mask1=None, ctx=None):
    """Every unordered pair of valid points of yx0, yx1 (nP, 2) [y,x] km -- the same points at t0 and t1 -- whose t0 separation r0
    lies in a class [edges_km[c], edges_km[c+1]), r0 > 0: with r1 the separation at t1, d = r1 - r0 and e = d/r0.  Returns
    {"table", "npts"}: table (nc, 7) fp64 under the names _lib.PAIRS_COLS -- per class the number of pairs and the sums of r0, e,
    |e|, e^2, |e|^3 and d^2 --, npts the valid points.  mask0 / mask1 (nP): 0 = the point is not valid; a point with a coordinate
    that is not finite is not valid either.  The work is the number of pairs within edges_km[-1] of each other, about
    nP*rho*pi*edges_km[-1]^2/2, and is the caller's to bound.  Runs on the GPU.  Raises ValueError on bad arguments before any
    device work.  dispersion_curve() and dispersion_exponents() read the table."""
    from .tracking import default_context
    cerr = 'ERROR [PairDispersion()]: '
    if np.ndim(yx0) != 2 or np.shape(yx0)[1] != 2 or np.shape(yx1) != np.shape(yx0):
        raise ValueError(cerr + '`yx0` and `yx1` must be (nP, 2) arrays of one shape, got %s, %s' % (np.shape(yx0), np.shape(yx1)))
    nP = np.shape(yx0)[0]
    for name, m in (("mask0", mask0), ("mask1", mask1)):
        if m is not None and np.shape(m) != (nP,):
            raise ValueError(cerr + '`%s` must be (%d,), got %s' % (name, nP, np.shape(m)))
    e = check_edges(edges_km, cerr)
    return (ctx or default_context()).pairs_points(yx0, yx1, e, mask0=mask0, mask1=mask1)


def _table_arg(table, T, who):
    t = np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != PAIRS_NCOLS:
        raise ValueError('ERROR [%s()]: `table` must be (nc, %d), got %s' % (who, PAIRS_NCOLS, t.shape))
    try:
        T = float(T)
    except (TypeError, ValueError):
        T = math.nan
    if not (math.isfinite(T) and T > 0.):
        raise ValueError('ERROR [%s()]: `T` must be finite and > 0, got %r' % (who, T))
    return t, T


def dispersion_curve(table, T):
    """The curve of a table of PairDispersion / IceTracker.pairs over the interval T: per class {"n", "L_km" = sum r0 / n, "rate":
    (nc, 3) the means of |e|^q / T^q for q = 1, 2, 3, "mean" = <e>/T, "d2" = <d^2> [km^2], the relative dispersion}.  A class
    without a pair gives NaN."""
    t, T = _table_arg(table, T, 'dispersion_curve')
    n = t[:, 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.where(n > 0., 1. / n, np.nan)
        L = t[:, 1] * inv
        rate = np.stack([t[:, 3] * inv / T, t[:, 4] * inv / T ** 2, t[:, 5] * inv / T ** 3], axis=1)
        mean = t[:, 2] * inv / T
        d2 = t[:, 6] * inv
    return {"n": n.copy(), "L_km": L, "rate": rate, "mean": mean, "d2": d2}


def dispersion_exponents(table, T, min_pairs=10):
    """The scaling exponents of a table of PairDispersion / IceTracker.pairs: {"beta": (3,), "L_km": (nc,), "used": (nc,) bool}.
    beta[q-1], q = 1, 2, 3, is minus the least-squares slope of log <|e/T|^q> against log L_km over the classes with at least
    `min_pairs` pairs and positive means; NaN with fewer than two such classes."""
    c = dispersion_curve(table, T)
    rate, L = c["rate"], c["L_km"]
    with np.errstate(invalid='ignore'):
        used = (c["n"] >= min_pairs) & (c["n"] >= 1) & np.isfinite(L) & (L > 0.) & np.all(np.isfinite(rate) & (rate > 0.), axis=1)
    beta = np.full(3, np.nan)
    if used.sum() >= 2:
        x = np.log(L[used])
        for q in range(3):
            beta[q] = -np.polyfit(x, np.log(rate[used, q]), 1)[0]
    return {"beta": beta, "L_km": L, "used": used}
