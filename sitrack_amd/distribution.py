"""Distribution of a set of values: host side of `sitrk_dist_values` / `sitrk_mesh_dist` (sitrack_amd/csrc/sitrk_dist.hip).

An extra the reference does not have: how many values fall between explicit edges -- the PDF of sea-ice deformation rates and its
power-law tail -- and exact order statistics -- the percentile a feature threshold is stated as --, counted and selected on the
GPU; the contract is in include/sitrk.h and DESIGN.md 3.21.  The device only compares: the edges are made here (log_edges,
lin_edges), and densities, tail slopes and thresholds are read off the integers that come back (pdf_from_counts, tail_exponent,
percentile_threshold).  There is no host version.  A running tracker takes the distribution of the cells of a device-resident
mesh with IceTracker.mesh_dist()."""
import collections
import math
import struct

import numpy as np

from ._lib import DIST_MAXBINS, DIST_MAXQ

# WHAT of the command line -> (what of sitrk_mesh_dist, sgn); sgn 0 = the absolute value
DIST_KINDS = {"div": ("div", 1), "conv": ("div", -1), "shr": ("shr", 1), "vor": ("vor", 1), "tot": ("tot", 1),
              "adiv": ("div", 0), "avor": ("vor", 0)}
PDF_Q = (0.5, 0.75, 0.85, 0.9, 0.95, 0.99)      # the quantiles --deform-pdf / --pdf store next to every histogram

Percentile = collections.namedtuple("Percentile", "pct")     # the THR of WHAT@pNN: resolved per sample, on the device


def check_edges(edges, cerr=''):
    """the library's checks of bin edges, for callers that must refuse before anything is computed; returns them as a (nb + 1,)
    float64 array"""
    try:
        e = np.array(edges, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`edges` must be a sequence of numbers, got %r' % (edges,)) from None
    if e.ndim != 1 or not 2 <= e.shape[0] <= DIST_MAXBINS + 1:
        raise ValueError(cerr + '`edges` must hold the nb + 1 edges of 1..%d bins, got shape %s' % (DIST_MAXBINS, e.shape))
    if not np.isfinite(e).all():
        raise ValueError(cerr + '`edges` must be finite')
    if not (np.diff(e) > 0.).all():
        raise ValueError(cerr + '`edges` must increase strictly')
    return e


def check_q(q, cerr=''):
    """the library's checks of the quantiles: (nq,) float64, nq <= 16, each in [0, 1]"""
    try:
        v = np.array(q, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`q` must be a sequence of numbers, got %r' % (q,)) from None
    if v.ndim != 1 or v.shape[0] > DIST_MAXQ:
        raise ValueError(cerr + '`q` must hold at most %d quantiles, got shape %s' % (DIST_MAXQ, v.shape))
    if not ((v >= 0.) & (v <= 1.)).all():
        raise ValueError(cerr + 'every `q` must lie in [0, 1], got %r' % (v.tolist(),))
    return v


def _edges_args(lo, hi, nb, who):
    try:
        lo, hi = float(lo), float(hi)
        bad = int(nb) != nb
    except (TypeError, ValueError):
        raise ValueError('ERROR [%s()]: expected two numbers and an integer, got %r, %r, %r' % (who, lo, hi, nb)) from None
    if bad or not 1 <= int(nb) <= DIST_MAXBINS:
        raise ValueError('ERROR [%s()]: `nb` must be an integer in 1..%d, got %r' % (who, DIST_MAXBINS, nb))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError('ERROR [%s()]: need lo < hi, both finite, got %r, %r' % (who, lo, hi))
    return lo, hi, int(nb)


def log_edges(lo, hi, nb):
    """nb + 1 geometric bin edges from lo to hi, 0 < lo < hi: edges[c] = lo*(hi/lo)**(c/nb), the two ends exact"""
    lo, hi, nb = _edges_args(lo, hi, nb, 'log_edges')
    if not lo > 0.:
        raise ValueError('ERROR [log_edges()]: geometric edges need lo > 0, got %r' % (lo,))
    e = lo * (hi / lo) ** (np.arange(nb + 1) / nb)
    e[0], e[nb] = lo, hi
    return check_edges(e, 'ERROR [log_edges()]: ')


def lin_edges(lo, hi, nb):
    """nb + 1 equidistant bin edges from lo to hi, lo < hi: edges[c] = lo + (hi - lo)*(c/nb), the two ends exact"""
    lo, hi, nb = _edges_args(lo, hi, nb, 'lin_edges')
    e = lo + (hi - lo) * (np.arange(nb + 1) / nb)
    e[0], e[nb] = lo, hi
    return check_edges(e, 'ERROR [lin_edges()]: ')


def ValueDistribution(x, edges=None, q=None, use=None, ctx=None):
    """The distribution of the values x (n,) whose `use` (n,) is not 0 (None: all), NaNs aside.  Returns {"counts", "edges", "q",
    "values", "ranks", "m", "nnan"}: counts (nb + 2,) int64, counts[c] = the values v with exactly c of the edges (nb + 1,
    finite, strictly ascending) <= v -- counts[0] below edges[0], counts[nb + 1] at or above edges[nb] --, None without edges;
    values (nq,) = for every q in [0, 1] the value at rank min(m - 1, floor(q*m)) of the sample in ascending order, bit for bit
    one of its values (-0.0 taken as 0.0), and ranks (nq,) int64 those ranks: NaN and -1 for an empty sample; m the sample's
    size, nnan the NaNs left out.  Infinities are ordinary values.  Runs on the GPU: counts and a radix selection, no sort.
    Raises ValueError on bad arguments before any device work."""
    from .tracking import default_context
    cerr = 'ERROR [ValueDistribution()]: '
    if np.ndim(x) != 1:
        raise ValueError(cerr + '`x` must be a (n,) array, got shape %s' % (np.shape(x),))
    if use is not None and np.shape(use) != np.shape(x):
        raise ValueError(cerr + '`use` must be %s, got %s' % (np.shape(x), np.shape(use)))
    e = None if edges is None else check_edges(edges, cerr)
    v = None if q is None else check_q(q, cerr)
    return (ctx or default_context()).dist_values(x, edges=e, q=v, use=use)


def pdf_from_counts(counts, edges):
    """The density of the in-range sample: per bin c of the nb bins  counts[c + 1] / (N * (edges[c + 1] - edges[c]))  with N the
    sum of counts[1 .. nb], the values inside [edges[0], edges[nb]); the two outer counts do not enter.  (nb,) fp64; NaN when no
    value is in range."""
    cerr = 'ERROR [pdf_from_counts()]: '
    e = check_edges(edges, cerr)
    c = np.asarray(counts)
    if c.shape != (e.shape[0] + 1,) or c.dtype.kind not in "iu" or (c < 0).any():
        raise ValueError(cerr + '`counts` must be (%d,) integers >= 0, got %s %s' % (e.shape[0] + 1, c.shape, c.dtype))
    inner = c[1:-1].astype(np.float64)
    n = float(inner.sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        return inner / (n * np.diff(e)) if n > 0. else np.full(inner.shape, np.nan)


def tail_exponent(counts, edges, lo, min_count=10):
    """The exponent of the power-law tail of a histogram: {"slope", "used", "x"}.  WHAT IS FITTED: over the bins c whose lower
    edge edges[c] >= lo > 0 and that hold at least `min_count` values, the ordinary least-squares line through the points
    (log x_c, log p_c), x_c = sqrt(edges[c]*edges[c + 1]) the bin's geometric centre and p_c = pdf_from_counts(counts, edges)[c];
    `slope` is that line's slope: a density p ~ x^-a gives -a.  `used` (nb,) bool marks the bins that entered; NaN with fewer
    than two.  `x` (nb,) is NaN for a bin that does not lie above 0.  With geometric edges a pure power law gives log p_c linear in log x_c exactly, whatever the bin width."""
    cerr = 'ERROR [tail_exponent()]: '
    p = pdf_from_counts(counts, edges)
    e = check_edges(edges, cerr)
    try:
        lo = float(lo)
    except (TypeError, ValueError):
        lo = math.nan
    if not (math.isfinite(lo) and lo > 0.):
        raise ValueError(cerr + '`lo` must be finite and > 0, got %r' % (lo,))
    c = np.asarray(counts)[1:-1]
    with np.errstate(invalid='ignore'):
        used = (e[:-1] >= lo) & (c >= max(int(min_count), 1)) & np.isfinite(p) & (p > 0.)
    x = np.full(c.shape, np.nan)                             # the geometric centre exists where the bin lies above 0
    pos = e[:-1] > 0.
    x[pos] = np.sqrt(e[:-1][pos] * e[1:][pos])
    slope = math.nan
    if used.sum() >= 2:
        slope = float(np.polyfit(np.log(x[used]), np.log(p[used]), 1)[0])
    return {"slope": slope, "used": used, "x": x}


def _bits(v):
    return struct.unpack('<q', struct.pack('<d', v))[0]


def _from_bits(b):
    return struct.unpack('<d', struct.pack('<q', b))[0]


def percentile_threshold(what, value):
    """The `thr` to hand to mesh_features() so that its test passes exactly from the selected order statistic `value` of
    mesh_dist() upwards.  For "div", "shr", "vor" (and their sgn -1 / absolute forms, whose sample already is sgn*f) the test is
    sgn*f >= thr and thr is `value` itself.  For "tot" `value` is t2_k = div*div + shr*shr of the selected cell and the test is
    t2 >= thr*thr: thr is the LARGEST double with thr*thr <= t2_k (the product rounded as the device rounds it), found by
    bisection on the bits of the doubles >= 0, so thr*thr <= t2_k < nextafter(thr, inf)**2.  The
    cell at the selected rank is therefore always active.  thr*thr may lie an ulp or two below t2_k, so a cell whose t2 falls in
    [thr*thr, t2_k) -- within an ulp or two below the selected value -- is active too.  ValueError for a value that is not
    finite (mesh_features() takes finite thresholds), for "tot" also below 0."""
    cerr = 'ERROR [percentile_threshold()]: '
    if what not in DIST_KINDS:
        raise ValueError(cerr + '`what` must be one of %s, got %r' % (", ".join(DIST_KINDS), what))
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = math.nan
    if not math.isfinite(v):
        raise ValueError(cerr + '`value` must be finite, got %r' % (value,))
    if DIST_KINDS[what][0] != "tot":
        return v + 0.0
    if v < 0.:
        raise ValueError(cerr + 'the t2 of "tot" cannot be negative, got %r' % (value,))
    # the bits of the doubles >= 0 ascend with them and the rounded square never descends: 0*0 <= v, and the largest double
    # squares to inf > v.  (For a denormal t2_k many doubles above sqrt(t2_k) still square to it: no fixed number of steps from
    # sqrt would do.)
    lo, hi = 0, _bits(1.7976931348623157e308)
    while hi - lo > 1:                                       # thr(lo)^2 <= v < thr(hi)^2
        mid = (lo + hi) // 2
        if _from_bits(mid) * _from_bits(mid) <= v:
            lo = mid
        else:
            hi = mid
    return _from_bits(lo)


def percentile_arg(token, flag='--deform-features'):
    """Percentile(NN) of the token pNN, NN a number in [0, 100]; ValueError otherwise"""
    try:
        if token[:1] != 'p':
            raise ValueError
        pct = float(token[1:])
    except ValueError:
        raise ValueError("%s: expected pNN with NN a number in [0, 100], got %r" % (flag, token)) from None
    if not 0. <= pct <= 100.:                                # a NaN fails both
        raise ValueError("%s: the percentile of pNN must lie in [0, 100], got %r" % (flag, token))
    return Percentile(pct)


def pdf_arg(text, flag='--deform-pdf'):
    """[(WHAT, edges)] of WHAT@LO:HI:NB[@lin|log][,...]: WHAT one of DIST_KINDS, NB in 1..1024 bins from LO to HI, geometric
    (`log`, the default, LO > 0) or equidistant (`lin`); every WHAT at most once.  ValueError otherwise."""
    res = []
    for part in text.split(','):
        tok = part.strip().split('@')
        if len(tok) not in (2, 3) or (len(tok) == 3 and tok[2] not in ("lin", "log")):
            raise ValueError("%s: expected WHAT@LO:HI:NB[@lin|log], got %r" % (flag, part))
        if tok[0] not in DIST_KINDS:
            raise ValueError("%s: WHAT must be one of %s, got %r" % (flag, ", ".join(DIST_KINDS), part))
        if tok[0] in [r[0] for r in res]:
            raise ValueError("%s: %s is given twice" % (flag, tok[0]))
        rng = tok[1].split(':')
        try:
            if len(rng) != 3:
                raise ValueError
            lo, hi, nb = float(rng[0]), float(rng[1]), int(rng[2])
        except ValueError:
            raise ValueError("%s: expected two numbers and an integer in LO:HI:NB, got %r" % (flag, part)) from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError("%s: need LO < HI, both finite, got %r" % (flag, part))
        if not 1 <= nb <= DIST_MAXBINS:
            raise ValueError("%s: NB must be in 1..%d, got %r" % (flag, DIST_MAXBINS, part))
        log = len(tok) < 3 or tok[2] == "log"
        if log and not lo > 0.:
            raise ValueError("%s: geometric (log) edges need LO > 0, got %r" % (flag, part))
        if tok[0] == "tot" and lo < 0.:
            raise ValueError("%s: the edges of tot must be >= 0, got %r" % (flag, part))
        res.append((tok[0], log_edges(lo, hi, nb) if log else lin_edges(lo, hi, nb)))
    return res


def square_edges(edges, cerr=''):
    """the edges of a histogram of tot as the device compares them: each squared (one rounded product); they must be >= 0 and
    still strictly ascending, else ValueError"""
    e = check_edges(edges, cerr)
    if (e < 0.).any():
        raise ValueError(cerr + 'the edges of what="tot" must be >= 0')
    e2 = e * e
    if not (np.diff(e2) > 0.).all() or not np.isfinite(e2).all():
        raise ValueError(cerr + 'the edges of what="tot" must stay finite and strictly ascending when squared')
    return e2


def rate_sample(rates, what, sgn):
    """the per-cell values sitrk_mesh_dist takes its sample from, formed on the host from the arrays rates["div"], ["shr"],
    ["vor"] of a deformation call: f, -f or |f| for sgn = +1, -1, 0, or for "tot" t2 = div*div + shr*shr (one rounded
    operation per symbol)"""
    if what == "tot":
        d, s = np.asarray(rates["div"], dtype=np.float64), np.asarray(rates["shr"], dtype=np.float64)
        return d * d + s * s
    f = np.asarray(rates[what], dtype=np.float64)
    return f if sgn > 0 else -f if sgn < 0 else np.abs(f)


def rate_distribution(rates, name, edges=None, q=None, use=None, ctx=None):
    """ValueDistribution of the rate `name` (one of DIST_KINDS) over the cells of a deformation call whose `use` is not 0: the
    host-array form of IceTracker.mesh_dist, with the same handling of "tot" -- edges squared on the way in, values = the square
    roots of the selected t2, which come back as "t2" """
    cerr = 'ERROR [rate_distribution()]: '
    if name not in DIST_KINDS:
        raise ValueError(cerr + '`name` must be one of %s, got %r' % (", ".join(DIST_KINDS), name))
    what, sgn = DIST_KINDS[name]
    e = None if edges is None else check_edges(edges, cerr)
    r = ValueDistribution(rate_sample(rates, what, sgn), edges=e if e is None or what != "tot" else square_edges(e, cerr), q=q, use=use,
                          ctx=ctx)
    r["edges"] = e
    if what == "tot":
        r["t2"] = r["values"]
        r["values"] = np.array([math.sqrt(t) if t == t else t for t in r["t2"]], dtype=np.float64)
    return r
