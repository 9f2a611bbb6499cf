"""Command-line driver: the reference's `si3_part_tracker.py` surface on top of libsitrk.

Same flags and defaults (reference si3_part_tracker.py:42-73), same module constants
(`rdt = 3600`, `iUVstrategy = 1`, :31,37), same file-name logic (:115-148,510-517,565-568), same
`./seed/Initialized_buoys_<SeedName>_<CONF>.npz` cache keys (:205-255), same per-buoy record windows in
2-D-time mode (:264-318), same NetCDF outputs (:515-571) -- the per-buoy loop (:378-490) and the
per-record inverse projection (:493) run on the GPU.  Differences, all opt-in or forced:
extra flags `--device`, `--uv-strategy`, `--rdt` (model output period: the reference's constant 3600, or `auto` = the spacing
of the model file's time axis) and `--nsub` (Euler sub-steps per record, default 1); under `torchrun` (WORLD_SIZE > 1) the buoys are range-partitioned over the
ranks by latitude band and every rank reads only the box (rows x columns) of each record its own buoys can touch (box
ingest, no collective; `--full-records`: rank 0 reads, RCCL broadcast), rank 0 writes the files; errors raise instead of
`print; exit(0)`; maps need the
optional `mojito` package and are skipped without it; the full (Nt+1,nP,2) series is NEVER held in host memory (the
reference keeps it twice, si3_part_tracker.py:324-330: 320 GB at 1e7 buoys x 1000 records): with `-F` every record is
appended to the series file as it is fetched (ncio.CloudBuoysStream: O(nP) memory), `--out-stride K` writes every K-th
record only, and the always-written 2-record file keeps records 0 and Nt.

`main()` is the run itself: open_run, read_mesh / sample_vars, init_seeds / seed_windows, open_tracker, then the record loop
over plan_batches.  What the loop keeps between batches lives in one object per concern -- Partition (who owns which buoys,
re-balancing), BoxIngest (which hyperslab of a record is read), Outputs (the series and the two-record file) and, where the
run asks for them, Sampler (--sample), DeformSeries (--deform) and PairSeries (--pairs), None otherwise.
"""
import argparse
import math
import os
from datetime import datetime, timezone
from os import path
from types import SimpleNamespace

import numpy as np

from . import _lib, coarse, dispersion, distribution, features, ncio, raster
from .distributed import Comm, all_ranges
from .tracking import GetTimeSpan, IceTracker, SeedInit, tinterp_phase

rdt = 3600.          # time step [s] = model output period (reference :31); the default of --rdt
FILL = ncio.FillValue


def epoch2clock(it):
    """reference util.py:18-34 (precision 's')"""
    return datetime.fromtimestamp(int(it), timezone.utc).strftime("%Y-%m-%d_%H:%M:%S")


def clock2epoch(cdate):
    """'YYYY-MM-DD_hh:mm:ss' (reference util.py:36-40) or a bare day 'YYYY-MM-DD' / 'YYYYMMDD' (mojito's 'guess')."""
    for fmt in ("%Y-%m-%d_%H:%M:%S", "%Y-%m-%d", "%Y%m%d"):
        try:
            return int(datetime.strptime(cdate, fmt).replace(tzinfo=timezone.utc).timestamp())
        except ValueError:
            pass
    raise ValueError("cannot parse date '%s'" % cdate)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='SITRACK ICE PARTICULES TRACKER (MI355X build)')
    rq = ap.add_argument_group('required arguments')
    rq.add_argument('-i', '--fsi3', required=True, help='output file of SI3 containing ice velocities ans co')
    rq.add_argument('-m', '--fmmm', required=True, help='model `mesh_mask` file of NEMO config used in SI3 run')
    rq.add_argument('-s', '--fsdg', required=True, help='seeding file')
    ap.add_argument('-k', '--krec', type=int, default=0, help='record of seeding file to use to seed from')
    ap.add_argument('-e', '--dend', default=None, help='date at which to stop')
    ap.add_argument('-F', '--fxdt', action="store_true", help='fixed tracking time (1D time array)')
    ap.add_argument('-N', '--ncnf', default='NANUK4', help='name of the horizontak NEMO config used')
    ap.add_argument('-p', '--plot', type=int, default=0, help='how often, in terms of model records, we plot the positions on a map')
    ap.add_argument('--device', type=int, default=0, help='GPU to use (extra)')
    ap.add_argument('--uv-strategy', type=int, default=1, choices=(0, 1, 2),
                    help='iUVstrategy of the reference (0 cell mean, 1 nearest U/V point = default); 2 = linear interpolation, an extra the reference does not have')
    ap.add_argument('--slots', type=int, default=32,
                    help='model records resident on the GPU (extra): up to half of them are advanced by one fused launch '
                         'whenever no per-record output is due, while the next ones are read and uploaded')
    ap.add_argument('--rebalance', type=int, default=256,
                    help='under torchrun: every so many records the buoys are re-partitioned over the ranks by their CURRENT host '
                         'row (migration of the states between ranks), so that every rank keeps a compact latitude band to read '
                         '(extra; 0 = never; same results)')
    ap.add_argument('--out-stride', type=int, default=1,
                    help='with -F: write every so many-th record of the series only (records 0, K, 2K, ...; extra, default 1 = the '
                         'reference\'s full series); the records in between go through fused launches of up to K records')
    ap.add_argument('--full-records', action='store_true',
                    help='read and upload whole records (under torchrun: rank 0 reads, RCCL broadcast) instead of only the rows '
                         'each rank\'s buoys can touch (extra; same results)')
    ap.add_argument('--rdt', type=_rdt_arg, default=rdt,
                    help='period of the model output [s], SECONDS or `auto` = the spacing of the model file\'s time_counter (extra; '
                         'default 3600, the reference\'s constant): each record advances the buoys by that much time')
    ap.add_argument('--nsub', type=_nsub_arg, default=1,
                    help='advance every record in NSUB Euler sub-steps of rdt/NSUB, each the reference\'s full step logic (extra; '
                         'default 1 = one step per record like the reference; 1..1024): keeps a buoy within one cell per '
                         'sub-step on 6-hourly or daily output')
    ap.add_argument('--sample', type=_sample_arg, default=[],
                    help='NAME[,NAME...]: 2-D variables (time,y,x) of the SI3 file written next to the positions as NAME(time,buoy), '
                         'the raw value at each buoy\'s host T-point, no interpolation (extra; default none): `siconc` comes from '
                         'the record resident on the GPU, any other name is read from the -i file for the records that are written')
    ap.add_argument('--tinterp', choices=('off', 'centre', 'start'), default='off',
                    help='interpolate u_ice, v_ice linearly in time between consecutive records for the sub-steps of --nsub (extra; '
                         'default off = every sub-step of a record uses that record\'s fields): `centre` = records are time means '
                         'centred on their step interval (what NEMO writes), `start` = snapshots at its start.  Partners are taken '
                         'among the records the run reads; siconc and the Survive test are never interpolated')
    ap.add_argument('--deform', type=_deform_arg, default=[],
                    help='SPEC[,SPEC...], at most 8; SPEC = RMAX_KM or RMAX_KM@RD_KM: deformation rates of quadrangle meshes that live on '
                         'the GPU next to the buoys (extra; default none).  Each SPEC is one mesh: the Delaunay triangles of circumradius '
                         '<= RMAX_KM of the buoys alive at the start of a window, paired into quadrangles; @RD_KM first coarsens the '
                         'cloud to that spacing.  Several SPECs give the scales of a scaling analysis from one run.  Written to '
                         './npz/<...>_deformation_<...>.npz; one rank only')
    ap.add_argument('--deform-window', type=_deform_window_arg, default=0,
                    help='with --deform: model records per window (extra; default 0 = the whole run is one window).  Every mesh is built '
                         'anew at the start of each window and its rates are taken after the window\'s last record; a last, shorter '
                         'window is kept')
    ap.add_argument('--deform-grid', type=_deform_grid_arg, default=None,
                    help='with --deform: D_KM or D_KM@t0 or D_KM@t1: every mesh is also rasterised, after each window, onto one regular '
                         'grid of square D_KM pixels that covers the model\'s F-points in the polar-stereographic plane (extra; default '
                         'none).  Per pixel the index of the cell it lies in (-1: none), stored as m<k>_w<k>_owner next to `grid` = (y0, '
                         'x0, d, ny, nx) and `grid_at`; a map is m<k>_w<k>_div[owner] where owner >= 0.  @t0 (default): the cells where '
                         'they were at the window\'s start, @t1: where they are at its end (status 1 only).  At most 2^28 pixels')
    ap.add_argument('--deform-coarse', type=_deform_coarse_arg, default=None,
                    help='with --deform and --deform-grid: NLEV or NLEV@FMIN: every mesh is also coarse-grained, after each window, on '
                         'NLEV levels of boxes of side D_KM*2^l over that grid (extra; default none): the area-weighted velocity '
                         'gradients of its status-1 cells box-averaged on the GPU, and per level the sums of A, A*div, A*shr, A*tot^q '
                         '(q = 1, 2, 3) over the boxes filled to at least FMIN (default 0.5) of their area, stored as m<k>_w<k>_coarse '
                         '(NLEV, 8) next to `coarse` = (nlev, fmin); the scaling exponents are logged.  At most 2^24 pixels')
    ap.add_argument('--deform-features', type=_deform_features_arg, default=None, metavar='WHAT@THR[@MINPIX[@CONN]]',
                    help='with --deform and --deform-grid: after each window the map of every mesh is taken apart into its features '
                         '(extra; default none): the connected sets of pixels whose rate passes a threshold, labelled on the GPU.  WHAT '
                         'is div (div >= THR), conv (-div >= THR), shr, vor or tot (div^2 + shr^2 >= THR^2), THR in 1/s, or pNN: the NN-th '
                         'percentile (0..100) of that rate over the status-1 cells of the mesh and window, taken on the GPU, logged and '
                         'stored as m<k>_w<k>_features_thr (`features` then holds NaN for thr, `features_pct` the NN); features of '
                         'fewer than MINPIX pixels (default 1) are dropped; CONN = 4 or 8 neighbours (default 8).  Stored as '
                         'm<k>_w<k>_features (rows, 12) int64 -- label, npix, jmin, jmax, imin, imax, the sums of j, i, j^2, i^2, j*i and '
                         'the perimeter -- with m<k>_w<k>_features_counts = (nfeat, ncomp, nactive), next to `features` = (what, sgn, '
                         'thr, min_pix, conn); the feature count and the longest feature are logged.  At most 32768 pixels a side')
    ap.add_argument('--deform-pdf', type=_deform_pdf_arg, default=None, metavar='WHAT@LO:HI:NB[@lin|log][,...]',
                    help='with --deform: after each window the distribution of a rate over the status-1 cells of every mesh, counted '
                         'and selected on the GPU (extra; default none).  WHAT is div, conv (-div), shr, vor, tot, adiv (|div|) or avor '
                         '(|vor|); NB bins (1..1024) from LO to HI in 1/s, geometric (`log`, the default, LO > 0) or equidistant '
                         '(`lin`).  Stored as m<k>_w<k>_pdf_<WHAT> (NB+2) int64 -- the cells below LO, in each bin, at or above HI -- '
                         'and m<k>_w<k>_q_<WHAT>, the exact quantiles 0.5, 0.75, 0.85, 0.9, 0.95, 0.99 (each the rate of one cell), next '
                         'to pdf_<WHAT>_edges and pdf_q; the median, the 95th percentile and the slope of the tail are logged')
    ap.add_argument('--deform-track', type=_deform_track_arg, nargs='?', const=1, default=None, metavar='REACH',
                    help='with --deform-features on the t0 draw: the features of every window are linked to those of the window before '
                         '(extra; default none).  The label map of a window is kept on the GPU, carried to the window\'s end by the '
                         'cells of its own mesh, and compared there with the map of the next window, pixel by pixel and within REACH '
                         'pixels (0..2, default 1).  Stored as m<k>_w<k>_pairs (npair, 3) int64 -- the label in the window before, '
                         'the label in this one, the pixels where they meet -- with m<k>_w<k>_pairs_counts = (npair, nhit), and per '
                         'row of m<k>_w<k>_features m<k>_w<k>_track and m<k>_w<k>_age, next to `track` = (reach,); the features '
                         'continued, born, ended, merged and split are logged.  At most 8 meshes')
    ap.add_argument('--deform-skeleton', type=_deform_skeleton_arg, nargs='?', const=features.SKEL_DEFAULT_MAXSUB, default=None,
                    metavar='MAXSUB',
                    help='with --deform-features: the features of every window are thinned to their skeletons on the GPU (extra; '
                         'default none), by at most MAXSUB sub-iterations (1..2^20, default 4096) of Guo and Hall\'s algorithm on the '
                         'kept label map.  Stored as m<k>_w<k>_skeleton (rows, 7) int64 -- label, npix, skeleton pixels, ends, '
                         'junctions, orthogonal and diagonal links, one row per row of m<k>_w<k>_features --, m<k>_w<k>_skeleton_nodes '
                         '(rows, 3) int64 -- pixel, label, X of every end (X = 1), junction (X >= 3) and isolated pixel (X = 0) -- with '
                         'm<k>_w<k>_skeleton_counts = (nfeat, nnode, nskel, nsub, converged), next to `skeleton` = (max_sub,); the '
                         'feature count and the longest skeleton are logged')
    ap.add_argument('--pairs', type=_pairs_arg, default=None, metavar='R_LO:R_HI:NC|e0,e1,...[@RD_KM]',
                    help='dispersion of buoy pairs (extra; default none): for every pair of buoys r0 apart at the start of a window the '
                         'strain (r1 - r0)/r0 of their separation, summed on the GPU per class of r0 -- NC geometric classes from R_LO '
                         'to R_HI km, or the explicit edges e0,e1,... (at most 16 classes) -- from the positions that live there: '
                         'per class the pairs and the sums of r0, e, |e|, e^2, |e|^3 and (r1 - r0)^2.  @RD_KM first coarsens the alive '
                         'cloud to that spacing; the work grows with the pairs within the last edge.  Written to '
                         './npz/<...>_pairs_<...>.npz as w<k>_pairs (ntau, nc, 7) with w<k>_jrec1, w<k>_T and w<k>_npts, next to '
                         '`edges`, `windows` and `time0`; the pairs per class and the scaling exponents are logged.  One rank only')
    ap.add_argument('--pairs-window', type=_pairs_count_arg('--pairs-window'), default=None,
                    help='with --pairs: model records per window (extra; default 0 = the whole run is one window).  The t0 positions are '
                         'taken in front of each window; a last, shorter window is kept')
    ap.add_argument('--pairs-every', type=_pairs_count_arg('--pairs-every'), default=None,
                    help='with --pairs: a table after every so many records of a window and at its end, all from the window\'s own t0 '
                         '(extra; default 0 = at the window\'s end only)')
    a = ap.parse_args(argv)
    for flag, v in (('--pairs-window', a.pairs_window), ('--pairs-every', a.pairs_every)):
        if v is not None and a.pairs is None:
            ap.error("%s: there is no table to take without --pairs" % flag)
    a.pairs_window, a.pairs_every = a.pairs_window or 0, a.pairs_every or 0
    refusal = deform_track_refusal(a.deform_track, a.deform_features, a.deform_grid, len(a.deform))
    if refusal:
        ap.error(refusal)
    refusal = deform_skeleton_refusal(a.deform_skeleton, a.deform_features)
    if refusal:
        ap.error(refusal)
    if a.deform_features is not None and a.deform_grid is None:
        ap.error("--deform-features: it works on the grid of --deform-grid; give that flag too")
    if a.deform_pdf is not None and not a.deform:
        ap.error("--deform-pdf: there is no mesh to take a distribution of without --deform")
    if a.deform_grid is not None and not a.deform:
        ap.error("--deform-grid: there is no mesh to rasterise without --deform")
    if a.deform_coarse is not None and a.deform_grid is None:
        ap.error("--deform-coarse: it works on the grid of --deform-grid; give that flag too")
    return a


def _sample_arg(text):
    names = [n.strip() for n in text.split(',') if n.strip()]
    if not names or len(set(names)) != len(names):
        raise argparse.ArgumentTypeError("--sample: expected distinct variable names NAME[,NAME...], got %r" % text)
    return names


DEFORM_MAX = _lib.MESH_MAX


def _deform_arg(text):
    """--deform: [(rmax_km, rd_km or 0.)] of RMAX_KM[@RD_KM][,...]: 1..8 entries, RMAX_KM finite in (0, 500], RD_KM finite > 0"""
    err = argparse.ArgumentTypeError
    specs = []
    parts = text.split(',')
    if len(parts) > DEFORM_MAX:
        raise err("--deform: at most %d meshes, got %d" % (DEFORM_MAX, len(parts)))
    for part in parts:
        tok = part.strip().split('@')
        if len(tok) not in (1, 2) or not all(t.strip() for t in tok):
            raise err("--deform: expected RMAX_KM or RMAX_KM@RD_KM, got %r" % part)
        try:
            val = [float(t) for t in tok]
        except ValueError:
            raise err("--deform: expected numbers in RMAX_KM[@RD_KM], got %r" % part)
        if not (np.isfinite(val[0]) and 0. < val[0] <= 500.):
            raise err("--deform: RMAX_KM must be finite and in (0, 500], got %r" % part)
        if len(val) == 2 and not (np.isfinite(val[1]) and val[1] > 0.):
            raise err("--deform: RD_KM must be finite and > 0, got %r" % part)
        specs.append((val[0], val[1] if len(val) == 2 else 0.))
    return specs


def _deform_grid_arg(text):
    """--deform-grid: (d_km, "t0" | "t1") of D_KM[@t0|@t1], D_KM finite > 0"""
    err = argparse.ArgumentTypeError
    tok = text.strip().split('@')
    if len(tok) not in (1, 2) or (len(tok) == 2 and tok[1] not in ("t0", "t1")):
        raise err("--deform-grid: expected D_KM, D_KM@t0 or D_KM@t1, got %r" % text)
    try:
        d = float(tok[0])
    except ValueError:
        raise err("--deform-grid: expected a number of km in D_KM[@t0|@t1], got %r" % text)
    if not (np.isfinite(d) and d > 0.):
        raise err("--deform-grid: D_KM must be finite and > 0, got %r" % text)
    return (d, tok[1] if len(tok) == 2 else "t0")


def _deform_coarse_arg(text):
    """--deform-coarse: (nlev, fmin) of NLEV[@FMIN], NLEV in 1..16, FMIN finite >= 0 (default 0.5)"""
    try:
        return coarse.coarse_arg(text, '--deform-coarse')
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _deform_features_arg(text):
    """--deform-features: (what, sgn, thr, min_pix, conn) of WHAT@THR[@MINPIX[@CONN]]"""
    try:
        return features.features_arg(text, '--deform-features')
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _deform_pdf_arg(text):
    """--deform-pdf: [(WHAT, edges)] of WHAT@LO:HI:NB[@lin|log][,...]"""
    try:
        return distribution.pdf_arg(text, '--deform-pdf')
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _deform_track_arg(text):
    """--deform-track: REACH, an integer in 0..2"""
    try:
        return features.track_arg(text, '--deform-track')
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _deform_skeleton_arg(text):
    """--deform-skeleton: MAXSUB, an integer in 1..2^20"""
    try:
        return features.skeleton_arg(text, '--deform-skeleton')
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def deform_skeleton_refusal(skel, feat):
    """--deform-skeleton: why the flags given cannot be thinned with, or None: it thins the features of --deform-features"""
    if skel is None:
        return None
    if feat is None:
        return "--deform-skeleton: it thins the features of --deform-features; give that flag too"
    return None


def deform_track_refusal(track, feat, grid, nmesh):
    """--deform-track: why the flags given cannot be tracked with, or None: it links the features of --deform-features, compares
    maps of the t0 draw, and takes two kept maps per mesh"""
    if track is None:
        return None
    if feat is None:
        return "--deform-track: it links the features of --deform-features; give that flag too"
    if grid is not None and grid[1] == "t1":
        return "--deform-track: tracking compares the t0 draw of a window with the window before carried to that instant; --deform-grid D_KM@t1 cannot be tracked"
    if 2 * nmesh > _lib.KEEP_MAX:
        return "--deform-track: two kept maps per mesh and %d of them: at most %d meshes, got %d" % (_lib.KEEP_MAX, _lib.KEEP_MAX // 2, nmesh)
    return None


def deform_grid(xYf, xXf, d_km):
    """--deform-grid: the one grid of a run, raster_grid over the model's finite F-point coordinates; refuses more than 2^28 pixels"""
    ok = np.isfinite(xYf) & np.isfinite(xXf)
    if not ok.any():
        raise ValueError('--deform-grid: the model grid has no finite F-point')
    g = raster.raster_grid(xYf[ok].min(), xYf[ok].max(), xXf[ok].min(), xXf[ok].max(), d_km)
    if g[3] * g[4] > raster.MAX_PIXELS:
        raise ValueError('--deform-grid: %g km over the model grid is %d x %d pixels, more than 2^28: take a coarser grid' % (d_km, g[3], g[4]))
    return g


def _deform_window_arg(text):
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("--deform-window: expected an integer, got %r" % text)
    if n < 0:
        raise argparse.ArgumentTypeError("--deform-window: must be >= 0 records, got %d" % n)
    return n


def _pairs_arg(text):
    """--pairs: (edges, rd_km or 0.) of R_LO:R_HI:NC[@RD_KM] or e0,e1,...[@RD_KM], RD_KM finite > 0"""
    err = argparse.ArgumentTypeError
    tok = text.split('@')
    if len(tok) not in (1, 2):
        raise err("--pairs: expected R_LO:R_HI:NC or e0,e1,..., with @RD_KM or without, got %r" % text)
    try:
        edges = dispersion.pairs_arg(tok[0], '--pairs')
    except ValueError as e:
        raise err(str(e))
    rd = 0.
    if len(tok) == 2:
        try:
            rd = float(tok[1])
        except ValueError:
            rd = math.nan
        if not (math.isfinite(rd) and rd > 0.):
            raise err("--pairs: RD_KM must be finite and > 0, got %r" % text)
    return (edges, rd)


def _pairs_count_arg(flag):
    def parse(text):
        try:
            n = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError("%s: expected an integer, got %r" % (flag, text))
        if n < 0:
            raise argparse.ArgumentTypeError("%s: must be >= 0 records, got %d" % (flag, n))
        return n
    return parse


def pair_windows(Nt, kstrt, nwin, every):
    """--pairs-window, --pairs-every: [(jrec0, [jrec1, ...])]: the windows of deform_windows and, per window, the model records
    behind which a table is taken -- every `every`-th of the window (0: none) and its last"""
    out = []
    for j0, j1 in deform_windows(Nt, kstrt, nwin):
        at = list(range(j0 + every - 1, j1, every)) if every > 0 else []
        out.append((j0, at + [j1]))
    return out


def pair_cuts(windows):
    """the model records behind which a batch must end for --pairs"""
    return sorted({j for _, js in windows for j in js})


def deform_windows(Nt, kstrt, nwin):
    """--deform-window: the windows [(jrec0, jrec1)] of model records, nwin records each (0: the whole run), the last one
    shorter where nwin does not divide Nt"""
    nwin = Nt if nwin <= 0 else nwin
    return [(kstrt + j, kstrt + min(j + nwin, Nt) - 1) for j in range(0, Nt, nwin)]


def output_due(jrec, kstrt, Nt, lFull, stride=1, ends=()):
    """does the step of model record jrec produce a record that is written (the series' k-th, or some buoys' last)"""
    k = jrec - kstrt + 1                               # the record of the series this step produces
    return bool((lFull and (k % stride == 0 or k == Nt)) or ((not lFull) and jrec in ends))


def plan_batches(Nt, kstrt, K, lFull, stride=1, ends=(), firsts=None, cuts=None):
    """The record loop's batches [(jt, m)]: consecutive records go into one sitrk_run of up to K // 2 records, cut after every
    record whose output is due (output_due) and -- only when fields are sampled (`firsts` = the distinct first records of the
    buoys' windows) -- in front of every record some buoy starts in, where its seed is sampled before the step.  `cuts`: model
    records after each of which a batch ends as well (--deform: the last record of every window; --pairs: the records it takes a
    table behind)."""
    firsts = set(firsts) if firsts is not None else set()
    cuts = set(cuts) if cuts is not None else set()
    batches, jt = [], 0
    while jt < Nt:
        m = 1
        while m < K // 2 and jt + m < Nt and not output_due(jt + m - 1 + kstrt, kstrt, Nt, lFull, stride, ends) \
                and (jt + m + kstrt) not in firsts and (jt + m - 1 + kstrt) not in cuts:
            m += 1
        batches.append((jt, m))
        jt += m
    return batches


def tinterp_slots(K):
    """--tinterp: the slot ring (at least 3: a record and its two partners) and the `K` plan_batches is given, so that a batch
    of m records, its two partners and the look-ahead of the batch before it (m'' + m + 2 records) sit in distinct slots."""
    K = max(3, int(K))
    return K, 2 * max(1, (K - 2) // 2)


def plan_tinterp(batches, Nt, K):
    """--tinterp: what every batch (jt0, m) of plan_batches needs around its launch, as a list of dicts.
      slot0, have_prev, have_next      arguments of sitrk_run_tlerp: partners are records of the run only, so the first record
                                       has none before it and the last none behind it
      prev_slot, next_slot             the slots of records jt0 - 1 / jt0 + m (None: no such partner)
      ahead                            the record (first of the next batch = the partner behind this one) that must be uploaded
                                       IN FRONT of this batch's launch, None for the last batch
      behind                           the rest of the next batch, uploaded behind the launch, while it runs
    Record jt0 - 1 is still resident from the batch before.  ValueError where m + 2 records do not fit the ring."""
    plan = []
    for ib, (jt0, m) in enumerate(batches):
        if m + 2 > K:
            raise ValueError('--tinterp: a batch of %d records and its two partners do not fit %d slots' % (m, K))
        nxt = batches[ib + 1] if ib + 1 < len(batches) else None
        have_prev, have_next = jt0 > 0, jt0 + m < Nt
        plan.append({"jt0": jt0, "m": m, "slot0": jt0 % K, "have_prev": have_prev, "have_next": have_next,
                     "prev_slot": (jt0 - 1) % K if have_prev else None, "next_slot": (jt0 + m) % K if have_next else None,
                     "ahead": nxt[0] if nxt else None,
                     "behind": list(range(nxt[0] + 1, nxt[0] + nxt[1])) if nxt else []})
    return plan


def batch_box_age(age, m, tinterp=False):
    """The `age` Context.box_of is given for a batch of m records planned `age` records after the buoys' box was evaluated:
    its last record is age + m - 1 records away.  With --tinterp the box is one record wider: the batch's last record is the
    partner of the next batch's first one, whose sub-steps start up to nsub cells further out."""
    return age + m - 1 + (1 if tinterp else 0)


def _rdt_arg(text):
    if text == 'auto':
        return 'auto'
    try:
        val = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("--rdt: expected seconds or 'auto', got %r" % text)
    if not (np.isfinite(val) and val > 0):
        raise argparse.ArgumentTypeError("--rdt: must be > 0 seconds, got %r" % text)
    return val


def _nsub_arg(text):
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("--nsub: expected an integer, got %r" % text)
    if not 1 <= n <= 1024:
        raise argparse.ArgumentTypeError("--nsub: must be in 1..1024, got %d" % n)
    return n


def axis_spacing(ztime_model):
    """The spacing [s] of a uniform model time axis (what `--rdt auto` takes); ValueError for an axis of fewer than two
    records or with unequal spacings."""
    tm = np.asarray(ztime_model, dtype=np.float64).reshape(-1)
    if tm.size < 2:
        raise ValueError('--rdt auto: the model time axis has %d record(s); its spacing needs at least 2' % tm.size)
    d = np.diff(tm)
    if not (d[0] > 0 and np.all(d == d[0])):
        raise ValueError('--rdt auto: the model time axis is not uniform (spacings %s .. %s s); give --rdt SECONDS'
                         % (d.min(), d.max()))
    return float(d[0])


def run_rdt(arg, ztime_model, say=print):
    """The period a run uses: `auto` -> axis_spacing(); an explicit value is kept, with one warning line when the axis is
    uniform with another spacing."""
    if arg == 'auto':
        return axis_spacing(ztime_model)
    val = float(arg)
    try:
        sp = axis_spacing(ztime_model)
    except ValueError:
        return val
    if sp != val:
        say(' *** WARNING: rdt = %g s but the model time axis is uniform with a spacing of %g s (--rdt auto would take it)' % (val, sp))
    return val


_IDEALISED_KINDS = ('nemoTsi3', 'nemoTmm', 'sidfex')


def seed_name_tokens(seed_file_name):
    """The two tags the output names inherit from the seeding file's NAME (behaviour of reference
    si3_part_tracker.py:115-148): the time-bin tag and the resolution tag, each with its leading underscore.

    * idealised seeding (`sitrack_seeding_<kind>_...`, kind = nemoTsi3 / nemoTmm / sidfex): time-bin tag `_idlSeed`;
      the resolution tag is the last of the final three `_`-separated tokens that ends in `km`, if any;
    * otherwise (RGPS-style selections, `..._dt72_..._10km.nc`): the time-bin token `dt<h>` sits three places before the
      resolution token `<n>km`, which is among the last four tokens; a name without resolution token has its `dt<h>`
      third from the end and yields an empty resolution tag.  Anything else is an error, like in the reference."""
    head = seed_file_name.split('.')[0].split('_')
    if len(head) > 2 and head[2] in _IDEALISED_KINDS:
        km = next((tok for tok in reversed(head[-3:]) if tok.endswith('km')), None)
        return '_idlSeed', ('_' + km) if km else ''
    toks = seed_file_name.split('.')[-2].split('_')
    if toks[-3].startswith('dt'):                      # no resolution token at the end
        return '_' + toks[-3], ''
    for back in range(1, 5):
        res, dtbin = toks[-back], toks[-back - 3]
        if res.endswith('km') and dtbin.startswith('dt'):
            return '_' + dtbin, '_' + res
    raise ValueError('could not figure out the resolution and time-bin tags from the file name %s' % seed_file_name)


def date_tag(it):
    """'1996-12-15_00:00:00' -> '19961215h00' (reference :510-512)"""
    c = epoch2clock(it).split(':')[0]
    return c.replace('-', '').replace('_', 'h')


def _savez_deflate(fname, **arrays):
    """The `.npz` the reference writes with `np.savez_compressed` (:255) -- same members, same `np.load` -- deflated at
    level 1 in 4-MB pieces on a thread pool (independent raw-deflate blocks closed with a sync flush concatenate into one
    valid deflate stream, the way `pigz -i` does it): the cache of 10^7 seeds (1.3 GB of arrays) took 36 s of zlib at
    numpy's level 6, 9 s at level 1 on one thread.  Written as ZIP64 throughout (members of 10^8 seeds exceed 4 GB)."""
    import io
    import struct
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    from numpy.lib import format as npfmt
    PIECE = 4 << 20

    def deflate(args):
        piece, last = args
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        return co.compress(piece) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)

    central = []
    with open(fname, 'wb') as f, ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        for key, val in arrays.items():
            arr = np.asanyarray(val)
            if not arr.flags.c_contiguous:
                arr = np.ascontiguousarray(arr)                # (never for a 0-d array: it would become 1-d)
            hdr = io.BytesIO()
            npfmt.write_array_header_1_0(hdr, npfmt.header_data_from_array_1_0(arr))        # the .npy header, then the data
            head = hdr.getvalue()
            body = memoryview(arr.reshape(-1).view(np.uint8)) if arr.size else memoryview(b'')
            name = (key + '.npy').encode()
            n = len(head) + len(body)
            pieces = [(head, len(body) == 0)] + [(body[o:o + PIECE], o + PIECE >= len(body)) for o in range(0, len(body), PIECE)]
            crc_job = ex.submit(lambda: zlib.crc32(body, zlib.crc32(head)))
            blobs = list(ex.map(deflate, pieces))
            crc, csize, off = crc_job.result() & 0xffffffff, sum(len(b) for b in blobs), f.tell()
            extra = struct.pack('<HHQQ', 1, 16, n, csize)                       # zip64: sizes
            f.write(struct.pack('<IHHHHHIIIHH', 0x04034b50, 45, 0, 8, 0, 0x21, crc, 0xffffffff, 0xffffffff, len(name), len(extra)))
            f.write(name); f.write(extra)
            for b in blobs:
                f.write(b)
            central.append((name, crc, csize, n, off))
        cd_off = f.tell()
        for name, crc, csize, n, off in central:
            extra = struct.pack('<HHQQQ', 1, 24, n, csize, off)
            f.write(struct.pack('<IHHHHHHIIIHHHHHII', 0x02014b50, 45, 45, 0, 8, 0, 0x21, crc, 0xffffffff, 0xffffffff, len(name),
                                len(extra), 0, 0, 0, 0, 0xffffffff))
            f.write(name); f.write(extra)
        cd_size = f.tell() - cd_off
        z64 = f.tell()
        f.write(struct.pack('<IQHHIIQQQQ', 0x06064b50, 44, 45, 45, 0, 0, len(central), len(central), cd_size, cd_off))
        f.write(struct.pack('<IIQI', 0x07064b50, 0, z64, 1))
        f.write(struct.pack('<IHHHHIIH', 0x06054b50, 0, 0, 0xffff, 0xffff, 0xffffffff, 0xffffffff, 0))


def record_windows(zTpos, ztime_model, kstrt, kstop, iTmA, iTmB, nP, rdt=3600.):
    """Per-buoy first / last model record in 2-D-time mode (reference :264-312).

    The reference loops over the late starters / early stoppers with one `np.where` over the model time axis each
    (`idx[-1]+1`, `idx[0]-1`).  On an increasing time axis those are counts, i.e. two `searchsorted` for all buoys at
    once (10^7 buoys: 5 s -> 0.1 s); any other axis takes the reference's loop.  Same IndexError when the search
    comes back empty.  `rdt` = the model output period (reference :31, the default)."""
    z1st = np.zeros(nP, dtype=int) + kstrt
    zLst = np.zeros(nP, dtype=int) + kstop
    half = int(rdt / 2)
    tm = np.asarray(ztime_model)
    # (entries the seeding file holds as _FillValue arrive masked, like netCDF4 hands them to the reference: a masked
    # comparison is no match for np.where, so such a buoy keeps the full window)
    late = np.where(np.ma.filled(zTpos[0, :] >= iTmA + half, False))[0]
    early = np.where(np.ma.filled(zTpos[1, :] < iTmB - half, False))[0]
    if tm.ndim == 1 and (tm.size < 2 or np.all(np.diff(tm) > 0)):
        if late.size:
            cnt = np.searchsorted(tm + half, zTpos[0, late], side='left')        # how many tm+half < T
            if np.any(cnt == 0):
                raise IndexError("index -1 is out of bounds for axis 0 with size 0")
            z1st[late] = cnt
        if early.size:
            cnt = np.searchsorted(tm - half, zTpos[1, early], side='right')      # how many tm-half <= T
            if np.any(cnt == tm.size):
                raise IndexError("index 0 is out of bounds for axis 0 with size 0")
            zLst[early] = cnt - 1
        return z1st, zLst
    return _record_windows_loop(zTpos, tm, z1st, zLst, late, early, half)


def _record_windows_loop(zTpos, tm, z1st, zLst, late, early, half):
    """the reference's own form (:289-312), one search per buoy"""
    for jb in late:
        (idx,) = np.where(tm + half < zTpos[0, jb])
        z1st[jb] = idx[-1] + 1
    for jb in early:
        (idx,) = np.where(tm - half > zTpos[1, jb])
        zLst[jb] = idx[0] - 1
    return z1st, zLst


class _Clock:
    """wall-clock shares of a run (where the command line spends its time: reading, the GPU, writing)"""

    def __init__(self):
        import time
        self.now = time.perf_counter
        self.t = {}
        self.t0 = self.now()

    def add(self, key, since):
        self.t[key] = self.t.get(key, 0.0) + (self.now() - since)
        return self.now()


def _tame_malloc():
    """The command line's host memory is O(nP) by design (the series is streamed); glibc would still keep hundreds of MB of
    freed record-sized buffers in per-thread arenas (the output is deflated on up to 16 threads, each allocating and freeing
    4-MB pieces): allocations of 1 MB and more go straight to mmap (returned to the system when freed, no dynamic threshold)
    and the arenas are capped.  Best effort, Linux / glibc only; the library itself never touches the allocator."""
    try:
        import ctypes
        libc = ctypes.CDLL(None)
        libc.mallopt(-3, 1 << 20)        # M_MMAP_THRESHOLD
        libc.mallopt(-8, 4)              # M_ARENA_MAX
    except Exception:                    # noqa: BLE001
        pass


def out_file(run, kind, t0, t1, ext='nc', tail=''):
    """./<ext>/<origin>_<kind>_<seed batch><time-bin tag>_<first date>_<last date><resolution tag><tail>.<ext> (reference :510-517,565-568)"""
    return ('./' + ext + '/' + run.corgn + '_' + kind + '_' + run.SeedBatch + run.cdtbin + '_' + date_tag(t0) + '_' + date_tag(t1)
            + run.csfkm + tail + '.' + ext)


def open_run(a, comm, say):
    """Run opening: the span of model records the seeding file asks for, the period and sub-steps of a record, the tags of the
    output names; makes the output directories (rank 0).  None when no model record matches."""
    lUse2DTime = not a.fxdt
    cdtbin, csfkm = seed_name_tokens(path.basename(a.fsdg))
    idateSeedA, idateSeedB, SeedName, SeedBatch, zTpos = ncio.SeedFileTimeInfo(a.fsdg, ltime2d=lUse2DTime)
    Nt0, ztime_model, idateModA, idateModB, ModConf, ModExp = ncio.ModelFileTimeInfo(a.fsi3)
    rdt = run_rdt(a.rdt, ztime_model, say)              # the module constant's value unless --rdt says otherwise
    if rdt != 3600. or a.nsub != 1:
        say(' *** rdt = %g s per model record, %d Euler sub-step(s) of %g s each' % (rdt, a.nsub, rdt / a.nsub))

    date_stop = None
    if a.dend:
        date_stop = clock2epoch(a.dend)
    elif idateSeedB - idateSeedA >= 3600.:
        date_stop = idateSeedB                      # several records in the seeding file: replicate its time span (:168-172)
    Nt, kstrt, kstop, iTmA, iTmB = GetTimeSpan(rdt, ztime_model, idateSeedA, idateModA, idateModB, iStop=date_stop)
    if Nt < 1:
        say(' QUITTING since no matching model records!')
        return None
    say(' *** model records %d..%d (%d records): %s -> %s' % (kstrt, kstop, Nt, epoch2clock(iTmA), epoch2clock(iTmB)))
    if comm.root:
        for cd in ('seed', 'nc', 'npz'):
            os.makedirs(cd, exist_ok=True)
    return SimpleNamespace(lUse2DTime=lUse2DTime, cdtbin=cdtbin, csfkm=csfkm, SeedName=SeedName, SeedBatch=SeedBatch, zTpos=zTpos,
                           Nt0=Nt0, ztime_model=ztime_model, corgn='NEMO-SI3_' + ModConf + '_' + ModExp, rdt=rdt, nsub=a.nsub,
                           Nt=Nt, kstrt=kstrt, kstop=kstop, iTmA=iTmA, iTmB=iTmB)


def read_mesh(a, ctx):
    """The model mesh (projected on the GPU of `ctx`) and, with --deform-grid, the one grid of the run: refused here -- before
    the model records are opened or anything is computed -- if it is too large."""
    imaskt, xlatT, xlonT, xYt, xXt, xYf, xXf, xResKM = ncio.GetModelGrid(a.fmmm, ctx=ctx)
    if a.uv_strategy >= 1:
        xYv, xXv, xYu, xXu = ncio.GetModelUVGrid(a.fmmm, ctx=ctx)
    else:
        xYv, xXv, xYu, xXu = xYf, xXf, xYf, xXf     # never read by the cell-mean rule
    (Nj, Ni) = np.shape(imaskt)
    dfm_grid = deform_grid(xYf, xXf, a.deform_grid[0]) if a.deform_grid else None
    if a.deform_coarse and dfm_grid[3] * dfm_grid[4] > coarse.MAX_PIXELS:
        raise ValueError('--deform-coarse: %g km over the model grid is %d x %d pixels, more than 2^24: take a coarser --deform-grid'
                         % (dfm_grid[2], dfm_grid[3], dfm_grid[4]))
    if a.deform_features:
        features.check_features_grid(dfm_grid, '--deform-features')
    return SimpleNamespace(imaskt=imaskt, xlatT=xlatT, xlonT=xlonT, xYf=xYf, xXf=xXf, xYu=xYu, xXu=xXu, xYv=xYv, xXv=xXv,
                           xResKM=xResKM, Nj=Nj, Ni=Ni, dfm_grid=dfm_grid)


def sample_vars(names, records, cf_uv, kstrt, Nj, Ni):
    """--sample: every name must be a (time, y, x) variable of the SI3 file -- checked before anything is computed.  Returns
    the attributes the files give each variable and the type (f4 / f8) it is sampled in."""
    attrs, dtype = {}, {}
    for n in names:
        if not records.f.has_var(n):
            raise ValueError("--sample: the SI3 file %s has no variable '%s'" % (cf_uv, n))
        x0 = np.asarray(records.fields(kstrt, (n,))[0])
        if x0.shape != (Nj, Ni):
            raise ValueError("--sample: variable '%s' of %s is not a (time, y, x) field of the %d x %d mesh" % (n, cf_uv, Nj, Ni))
        attrs[n] = ncio.model_var_attrs(records.f, n)
        dtype[n] = np.dtype(np.float32) if x0.dtype.newbyteorder('=') == np.float32 else np.dtype(np.float64)
        if n in ncio.SCHEMA_VARS:
            raise ValueError("--sample: '%s' collides with a variable of the trajectory files" % n)
    return attrs, dtype


def init_seeds(a, run, mesh, records, comm, ctx, say):
    """Seeding, with the reference's intermediate cache (:205-255).  Seeds are independent: with several ranks each one
    locates its own contiguous range and the results are concatenated in rank (= seed) order."""
    cf_npz_itm = './seed/Initialized_buoys_' + run.SeedName + '_' + a.ncnf + '.npz'
    if comm.bcast_obj(path.exists(cf_npz_itm)):
        say(' *** using cached seed initialisation ' + cf_npz_itm)
        pack = None
        if comm.root:
            with np.load(cf_npz_itm) as data:
                pack = (data['xPosG0'], data['xPosC0'], data['IDs'], data['vJIt'], data['VRTCS'], data['idxKeep'])
        xPosG0, xPosC0, IDs, vJIt, VRTCS, idxK = comm.bcast_arrays(pack)          # tensors, not pickles
        nP = len(IDs)
    else:
        (xIC,) = records.fields(run.kstrt, ('siconc',))
        zt, zIDs, XseedG, XseedC = ncio.LoadNCdata(a.fsdg, krec=a.krec)
        (nP0, _) = np.shape(XseedG)
        IDs = np.array(zIDs, dtype=int)
        lo, hi = comm.range(nP0)
        kept = SeedInit(IDs[lo:hi], XseedG[lo:hi], XseedC[lo:hi], mesh.xlatT, mesh.xlonT, mesh.xYf, mesh.xXf, mesh.xResKM, mesh.imaskt,
                        xIceConc=np.asarray(xIC, dtype=np.float64), ctx=ctx)
        # every rank's kept seeds, concatenated in rank (= seed) order: tensor all-gathers
        xPosG0, xPosC0, IDs, vJIt, VRTCS, idxK = comm.allgather_rows(kept[1:6] + (lo + kept[6],))
        nP = len(IDs)
        if nP < nP0:
            say(' *** `SeedInit()` had to cancel ' + str(nP0 - nP) + ' buoys! => nP = ' + str(nP))
        if comm.root:
            _savez_deflate(cf_npz_itm, nP=nP, xPosG0=xPosG0, xPosC0=xPosC0, IDs=IDs, vJIt=vJIt, VRTCS=VRTCS, idxKeep=idxK)
    return SimpleNamespace(nP=nP, xPosG0=xPosG0, xPosC0=xPosC0, IDs=IDs, vJIt=vJIt, idxK=idxK)


def seed_windows(run, seeds, say):
    """Per-buoy first / last model record (:264-318): the whole run with -F, record_windows() of the seeding file's 2-D time
    otherwise."""
    nP = seeds.nP
    if not run.lUse2DTime:
        return np.zeros(nP, dtype=int) + run.kstrt, np.zeros(nP, dtype=int) + run.kstop
    zTpos = run.zTpos if np.ma.isMaskedArray(run.zTpos) else np.asarray(run.zTpos)
    if zTpos.shape != (2, nP) and zTpos.ndim == 2 and zTpos.shape[1] > nP and len(seeds.idxK) == nP:
        # SeedInit cancelled buoys: keep the time positions of the survivors.  (The reference has this line
        # commented out, si3_part_tracker.py:250, and then stops on the shape check of :269-272.)
        say(' *** adjusting `zTpos` to the %d buoys kept by SeedInit' % nP)
        zTpos = zTpos[:, seeds.idxK]
    if zTpos.shape != (2, nP):
        raise ValueError('wrong shape for the 2D time array `zTpos`: %s vs nP=%d' % (zTpos.shape, nP))
    return record_windows(zTpos, run.ztime_model, run.kstrt, run.kstop, run.iTmA, run.iTmB, nP, rdt=run.rdt)


def open_tracker(a, run, mesh, records, ctx):
    """The tracker on the device: `K` resident record slots of the model file's type; with --tinterp the ring and the `K_plan`
    plan_batches is given are those of tinterp_slots().  Returns (trk, K, K_plan, tphase), tphase None without --tinterp."""
    (u0,) = records.fields(run.kstrt, ('u_ice',))
    fdt = np.float64 if np.asarray(u0).dtype == np.float64 else np.float32
    K = int(max(2, min(a.slots, 64)))
    tphase = None if a.tinterp == 'off' else tinterp_phase(a.tinterp)
    K_plan = K
    if tphase is not None:
        K, K_plan = tinterp_slots(K)
    trk = IceTracker(mesh.xYf, mesh.xXf, mesh.xYu, mesh.xXu, mesh.xYv, mesh.xXv, mesh.imaskt, rdt=run.rdt, iUVstrategy=a.uv_strategy,
                     nslots=K, field_dtype=fdt, ctx=ctx, nsub=run.nsub)
    return trk, K, K_plan, tphase


def record_broadcaster(a, comm, ctx, tphase):
    """--full-records under an RCCL launch: rank 0 reads; one RCCL broadcast per record, overlapped with the stepping.  None
    for every other run."""
    if not (a.full_records and comm.multi and comm.backend == "nccl"):
        return None
    from .distributed import RecordBroadcaster
    if tphase is not None:
        raise ValueError('--tinterp is not available together with --full-records under an RCCL launch (the record broadcaster '
                         'hands a slot back before its partner has been stepped with): drop --full-records')
    return RecordBroadcaster(ctx)


def rebalance_places(rows, allh, rank, ranges):
    """Re-balancing: where the buoys of rank `rank` go.  rows: their host rows, in local order; allh (world, Nj): every rank's
    histogram of host rows; ranges: all_ranges(nP, world).  Returns newpos, each buoy's place in the new global order -- by
    (row, owning rank, local order) -- and dest, the rank whose range that place falls in."""
    hist = allh[rank]
    before_row = np.concatenate([[0], np.cumsum(allh.sum(axis=0))[:-1]])    # buoys in lower rows
    before_rank = allh[:rank].sum(axis=0)                                   # same row, lower ranks
    o = np.argsort(rows, kind='stable')
    within = np.empty(len(rows), dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(hist)[:-1]])
    within[o] = np.arange(len(rows)) - starts[rows[o]]                      # same row, this rank, local order
    newpos = before_row[rows] + before_rank[rows] + within
    ends = np.array([hi for _, hi in ranges])
    return newpos, np.searchsorted(ends, newpos, side='right')


def rebalance_due(batches, every, multi):
    """after which batches the ranks re-balance: a function of the record count alone (never after the last one)"""
    due, since = [], 0
    for (_, m) in batches:
        since += m
        due.append(multi and every > 0 and since >= every)
        if due[-1]:
            since = 0
    if due:
        due[-1] = False
    return due


class Partition:
    """Who owns which buoys.  Under torchrun every rank owns a contiguous range of the buoys ordered by host row, i.e. a
    latitude band: with box ingest each rank then reads only its own rows of every record, no collective.
      order    the caller's indices of all buoys in rank order (rank 0 keeps it up to date)
      mine     those of this rank;  range: its [lo, hi) of `order` at the start
      windows  (first, last) model record of every buoy in the caller's order, None with -F"""

    def __init__(self, comm, vJIt, nP, Nj, windows=None):
        self.comm, self.nP, self.Nj, self.windows = comm, nP, Nj, windows
        self.order = np.argsort(vJIt[:, 0], kind='stable') if comm.multi else np.arange(nP)
        self.range = comm.range(nP)
        self.mine = self.order[self.range[0]:self.range[1]]
        self.rebalances = self.migrated = 0

    def to_caller_order(self, rows):
        """rows gathered in rank order -> the caller's buoy order"""
        if rows is None or not self.comm.multi:
            return rows
        out = np.empty_like(rows)
        out[self.order] = rows
        return out

    def gather(self, rows):
        """this rank's rows -> all buoys' rows in the caller's order on rank 0, None elsewhere"""
        return self.to_caller_order(self.comm.gather_rows(rows, self.nP))

    def rebalance(self, ctx, ingest):
        """Re-partition the buoys over the ranks by their CURRENT host row (migration / re-balancing).
        Each rank fetches its buoys' state, a global histogram of host rows fixes every buoy's place in the new order
        (rebalance_places), hence its new owner; the states travel in one all-to-all of 50-byte rows and every rank
        re-creates its buoy set with their history (dead flags, kill records).  Trajectories do not depend on who steps a
        buoy; only the rows a rank has to read do: `ingest` starts over."""
        comm = self.comm
        st = ctx.fetch()
        rows = st["jiT"][:, 0].astype(np.int64)
        hist = np.bincount(rows, minlength=self.Nj).astype(np.int64)
        allh = comm.allgather_rows((hist[None, :],))[0]                        # (world, Nj)
        newpos, dest = rebalance_places(rows, allh, comm.rank, all_ranges(self.nP, comm.world))
        f8 = np.concatenate([st["yx"], newpos[:, None].astype(np.float64)], axis=1)          # positions travel exactly
        win = (self.windows[0][self.mine], self.windows[1][self.mine]) if self.windows else (np.zeros(len(rows), dtype=int),) * 2
        i8 = np.stack([self.mine.astype(np.int64), st["jiT"][:, 0].astype(np.int64), st["jiT"][:, 1].astype(np.int64),
                       st["alive"].astype(np.int64), st["kill_rec"].astype(np.int64), np.asarray(win[0], dtype=np.int64),
                       np.asarray(win[1], dtype=np.int64)], axis=1)
        self.rebalances += 1
        self.migrated += comm.sum_int(int((dest != comm.rank).sum()))
        chunks = [(f8[dest == d], i8[dest == d]) for d in range(comm.world)]
        rf8, ri8 = comm.alltoall_rows(chunks)
        k = np.argsort(rf8[:, 2], kind='stable')                               # the new order inside this rank's range
        rf8, ri8 = rf8[k], ri8[k]
        self.mine = ri8[:, 0].copy()
        ctx.set_buoys(np.ascontiguousarray(rf8[:, :2]), ri8[:, 1:3].astype(np.int32),
                      ri8[:, 5].astype(np.int32) if self.windows else None, ri8[:, 6].astype(np.int32) if self.windows else None, sort=False)
        ctx.restore_state(ri8[:, 3].astype(np.int8), ri8[:, 4].astype(np.int32))
        ctx.sort_buoys()
        allmine = comm.gather_rows(self.mine, self.nP)
        if comm.root:
            self.order = allmine
        ingest.reset()


class BoxIngest:
    """Record ingest: records jt -> slots jt % K, asynchronously.  By default only the box (rows x columns, round 4) this
    rank's buoys can touch is read from the file and uploaded: their host cells at the last evaluation, widened by one cell
    per record stepped or queued since (sitrk_buoy_box waits for the GPU: only every REEVALUATE_AFTER records).
      boxes    batch start jt0 -> (j0, j1, i0, i1), what the batch's slots hold: the box its records are sampled in.  Empty
               with --full-records (whole records; under torchrun rank 0 reads and the record is broadcast)
      bytes    read and uploaded so far"""
    REEVALUATE_AFTER = 96

    def __init__(self, ctx, records, comm, clk, kstrt, K, Nj, esz, full_records=False, tinterp=False, bcast=None):
        self.ctx, self.records, self.comm, self.clk, self.bcast = ctx, records, comm, clk, bcast
        self.kstrt, self.K, self.Nj, self.esz, self.full_records, self.tinterp = kstrt, K, Nj, esz, full_records, tinterp
        self.box, self.age, self.bytes, self.boxes = None, None, 0, {}

    def reset(self):
        """the buoys are others now (re-balancing): their box is evaluated at the next batch"""
        self.age = None

    def plan(self, jt0, m, not_queued=0):
        """the box of the batch jt0..jt0+m-1; not_queued: records planned in front of it that the GPU has not been given yet"""
        if self.full_records:
            return
        if self.age is None or self.age + m > self.REEVALUATE_AFTER:
            self.box = self.ctx.buoy_box()
            self.age = not_queued
        self.boxes[jt0] = self.ctx.box_of(*self.box, batch_box_age(self.age, m, self.tinterp))
        self.age += m

    def upload(self, jt0, m):
        """records jt0..jt0+m-1 -> slots (jt0+r) % K"""
        self.plan(jt0, m)
        self.upload_recs(jt0, range(jt0, jt0 + m))

    def upload_recs(self, jt0, jts):
        """records jts of (or, as a partner, next to) the batch that starts at jt0 -> slots jt % K, over that batch's box"""
        t_up = self.clk.now()
        ctx, records, comm, Nj = self.ctx, self.records, self.comm, self.Nj
        if not self.full_records:
            j0, j1, i0, i1 = self.boxes[jt0]
        for jt_r in jts:
            jrec, slot = jt_r + self.kstrt, jt_r % self.K
            if not self.full_records:
                if j1 > j0:
                    ctx.stage_fill(slot, j0, j1 - j0, lambda *outs: records.fields_box_into(jrec, j0, j1, i0, i1, outs), i0=i0, ncols=i1 - i0)
                    self.bytes += 3 * (j1 - j0) * (i1 - i0) * self.esz
                else:
                    ctx.commit_record_rows(slot, 0, 0)                  # no live buoy: nothing to read
            elif not comm.multi:
                ctx.stage_fill(slot, 0, Nj, lambda *outs: records.fields_rows_into(jrec, 0, Nj, outs))   # the whole record (:372-374)
            elif self.bcast is not None:
                self.bcast.deliver(slot, records.fields(jrec) if comm.root else None)
            else:
                comm.deliver_record(ctx, slot, records.fields(jrec) if comm.root else None)   # gloo rehearsal: host broadcast
        self.clk.add("read_and_stage_records_s", t_up)


class Sampler:
    """--sample: the model fields at the buoys, written next to the positions.
      firsts   the model records in front of which seeds are sampled before the step: record kstrt with -F, every distinct
               first record of the windows otherwise
      keep()   fills the two rows of the tracking12 file (rank 0)"""

    def __init__(self, names, attrs, dtype, ctx, records, part, clk, kstrt, K, Nj, Ni, z1st=None):
        self.names, self.attrs, self.dtype = list(names), attrs, dtype
        self.ctx, self.records, self.part, self.clk, self.kstrt, self.K, self.Nj, self.Ni = ctx, records, part, clk, kstrt, K, Nj, Ni
        self.firsts = set(np.unique(z1st).tolist()) if z1st is not None else {kstrt}
        self.zS = {n: np.full((2, part.nP), FILL, dtype=np.float32) for n in self.names} if part.comm.root else None

    def sample(self, jrec, box, mode):
        """The fields at this rank's buoys for model record jrec -- 'enter' before its step, 'after' behind it -- gathered into
        (nP, names) f4 in the caller's order on rank 0 (None elsewhere).  siconc comes from the resident slot; the other
        variables are read from the file for this record only, as the `box` the batch's slots hold (a buoy's cell stays
        inside it during the batch; None: whole records), and travel to the GPU through sitrk_sample_fields."""
        t_s = self.clk.now()
        names, ctx = self.names, self.ctx
        nloc = len(self.part.mine)
        rows = np.full((nloc, len(names)), FILL, dtype=np.float32)
        if nloc and (box is None or (box[1] > box[0] and box[3] > box[2])):
            for dt in (np.dtype(np.float32), np.dtype(np.float64)):
                cols = [k for k, n in enumerate(names) if n != 'siconc' and self.dtype[n] == dt]
                for b in range(0, len(cols), _lib.SAMPLE_MAX_FIELDS):
                    grp = cols[b:b + _lib.SAMPLE_MAX_FIELDS]
                    j0, j1, i0, i1 = box if box is not None else (0, self.Nj, 0, self.Ni)
                    bufs = [np.empty((j1 - j0, i1 - i0), dtype=dt) for _ in grp]
                    self.records.fields_box_into(jrec, j0, j1, i0, i1, bufs, names=[names[k] for k in grp])
                    rows[:, grp] = ctx.sample_fields(jrec, mode, bufs, box=(j0, j1, i0, i1)).T
            if 'siconc' in names:
                rows[:, names.index('siconc')] = ctx.sample_slot((jrec - self.kstrt) % self.K, jrec, mode, 'siconc')
        self.clk.add("sample_s", t_s)
        return self.part.gather(rows)

    def keep(self, row, sel, srow):
        """the sampled values srow of the buoys `sel` -> row 0 (seeds) or 1 (last positions) of the tracking12 file"""
        for kn, n in enumerate(self.names):
            self.zS[n][row, sel] = srow[sel, kn]

    def columns(self, srow):
        """a record of the series: {name: values of all buoys}"""
        return {n: srow[:, kn] for kn, n in enumerate(self.names)}

    def rows(self):
        """the tracking12 file's {name: ((2, nP) values, attributes)}"""
        return {n: (self.zS[n], self.attrs[n]) for n in self.names}


class DeformSeries:
    """--deform: quadrangle meshes that live on the GPU next to the buoys, built anew in front of every window of model
    records and their rates taken behind it.
      win      the windows [(jrec0, jrec1)];  first / last: model record -> the window it opens / closes
      out      what is kept of every (mesh, window) for the file"""

    def __init__(self, specs, window, grid, grid_at, Nt, kstrt, ctx, trk, IDs, nP, say, clk, coarse=None, feat=None, track=None,
                 skel=None, pdf=None):
        self.specs, self.grid, self.grid_at, self.coarse, self.feat, self.track = specs, grid, grid_at, coarse, feat, track
        self.pdf = pdf                                   # --deform-pdf: [(WHAT, edges)]
        self.skel = skel                                 # --deform-skeleton: max_sub
        self.links = {}                                  # --deform-track: (mesh, window) -> the links to the window before
        self.ctx, self.trk, self.IDs, self.nP, self.say, self.clk = ctx, trk, IDs, nP, say, clk
        self.win = deform_windows(Nt, kstrt, window)
        self.first, self.last = {w[0]: k for k, w in enumerate(self.win)}, {w[1]: k for k, w in enumerate(self.win)}
        self.out = {}

    def build(self, kw):
        """in front of the first record of window kw: every mesh from the cloud as it is now"""
        t_d = self.clk.now()
        ctx, trk = self.ctx, self.trk
        jrec0 = self.win[kw][0]
        keep_of = {}
        for km, (rmax, rd) in enumerate(self.specs):
            msk = None
            if rd > 0.:
                if rd not in keep_of:                    # the alive cloud, coarsened to spacing rd on the positions as they are now
                    st = ctx.fetch()
                    al = np.asarray(st["alive"]) != 0
                    keep = np.zeros(self.nP, dtype=np.int8)
                    if al.any():
                        keep[np.where(al)[0][ctx.subsample_cloud(st["yx"][al], rd)[0]]] = 1
                    keep_of[rd] = keep
                msk = keep_of[rd]
            r = trk.mesh(rmax, jrec0, slot=km, mask=msk)
            self.out["m%d_w%d_cells" % (km, kw)] = np.asarray(self.IDs)[trk.mesh_cells(km)].astype(np.int64).reshape(-1, 4)
            self.say(' *** --deform window %d mesh %d (rmax %g km%s): %d triangles -> %d quadrangles'
                     % (kw, km, rmax, ', rd %g km' % rd if rd > 0. else '', r["nT"], r["nQ"]))
        self.clk.add("deform_s", t_d)

    def take(self, kw):
        """behind the last record of window kw: the rates of every mesh since the window's start"""
        t_d = self.clk.now()
        jrec1 = self.win[kw][1]
        for km in range(len(self.specs)):
            r = self.trk.mesh_deform(jrec1, slot=km)
            pre = "m%d_w%d_" % (km, kw)
            for n in ("div", "shr", "vor", "area0", "area1"):
                self.out[pre + n] = r[n]
            self.out[pre + "status"] = r["status"]
            stt = r["stats"]
            self.out[pre + "stats"] = np.array([stt[n] for n in _lib.MESH_STATS], dtype=np.float64)
            self.say(' *** --deform window %d mesh %d: nQ = %d, status 0/1/2 = %d/%d/%d, area-weighted mean total deformation = %s'
                     % (kw, km, len(r["status"]), stt["n0"], stt["n1"], stt["n2"],
                        '%.6e /s' % (stt["area0_tot"] / stt["area0"]) if stt["area0"] > 0. else 'n/a'))
            for name, edges in self.pdf or ():           # the distribution of a rate: NB + 2 counts and six values come down
                what, sgn = distribution.DIST_KINDS[name]
                d = self.trk.mesh_dist(jrec1, what=what, sgn=sgn, edges=edges, q=distribution.PDF_Q, slot=km)
                self.out[pre + "pdf_" + name], self.out[pre + "q_" + name] = d["counts"], d["values"]
                lo = edges[0] if edges[0] > 0. else edges[edges > 0.][0] if (edges > 0.).any() else None
                self.say(' *** --deform-pdf window %d mesh %d %s: %d cells, %d below / %d at or above the edges, median %.6e /s, '
                         'p95 %.6e /s, tail slope %s' % (kw, km, name, d["m"], d["counts"][0], d["counts"][-1], d["values"][0], d["values"][4],
                                                       '%.3f' % distribution.tail_exponent(d["counts"], edges, lo)["slope"]
                                                       if lo is not None else 'n/a'))
            if self.grid is not None:                    # the map is out[:, owner] on the host: no second copy of the rates
                self.out[pre + "owner"] = self.trk.mesh_raster(jrec1, self.grid, slot=km, at=self.grid_at, fields=False)["owner"]
            if self.coarse is not None:                  # the scaling curve of this mesh and window: 64 bytes per level come down
                tab = self.trk.mesh_coarse(jrec1, self.grid, self.coarse[0], fmin=self.coarse[1], slot=km)["table"]
                self.out[pre + "coarse"] = tab
                beta = coarse.scaling_exponents(tab, self.grid[2])["beta"]
                self.say(' *** --deform-coarse window %d mesh %d: %d levels from %g km, filled boxes %s, beta(1..3) = %s'
                         % (kw, km, len(tab), self.grid[2], '/'.join('%d' % n for n in tab[:, 1]), ', '.join('%.4f' % b for b in beta)))
            if self.feat is not None:                    # the features of this mesh's map: 96 bytes per feature come down
                what, sgn, thr, min_pix, conn = self.feat
                if isinstance(thr, distribution.Percentile):           # WHAT@pNN: this mesh's and window's own threshold, 16 bytes down
                    thr = self.threshold(jrec1, km, kw, what, sgn, thr.pct)
                    self.out[pre + "features_thr"] = np.float64(thr)
                # --deform-track: kept map 2km = this window's features, 2km + 1 = those of the window before at this window's start
                # --deform-skeleton without it: the last kept map, for this call only
                slot = 2 * km if self.track is not None else _lib.KEEP_MAX - 1 if self.skel is not None else None
                f = self.trk.mesh_features(jrec1, self.grid, what=what, thr=thr, sgn=sgn, conn=conn, min_pix=min_pix, slot=km,
                                           at=self.grid_at, keep=slot)
                self.out[pre + "features"] = f["table"]
                self.out[pre + "features_counts"] = np.array([f["nfeat"], f["ncomp"], f["nactive"]], dtype=np.int64)
                ft = features.feature_table(f["table"], self.grid)
                self.say(' *** --deform-features window %d mesh %d: %d features of >= %d pixels (%d components, %d active pixels)%s, '
                         'longest %s' % (kw, km, f["nfeat"], min_pix, f["ncomp"], f["nactive"],
                                         '' if f["nfeat"] == len(f["table"]) else ', first %d kept' % len(f["table"]),
                                         '%.3f km' % ft["length_km"].max() if len(f["table"]) else 'n/a'))
                if self.skel is not None:                # this window's kept map thinned: 56 bytes per feature, 24 per node come down
                    try:
                        s = self.trk.features_skeleton(slot, max_sub=self.skel)
                    finally:
                        if self.track is None:
                            self.ctx.keep_free(slot)
                    self.out[pre + "skeleton"] = s["table"]
                    self.out[pre + "skeleton_nodes"] = s["nodes"]
                    self.out[pre + "skeleton_counts"] = np.array([s["nfeat"], s["nnode"], s["nskel"], s["nsub"], s["converged"]], dtype=np.int64)
                    sk = features.skeleton_table(s["table"], self.grid)
                    self.say(' *** --deform-skeleton window %d mesh %d: %d features, %d skeleton pixels, %d nodes%s in %d sub-iterations, '
                             'longest %s' % (kw, km, s["nfeat"], s["nskel"], s["nnode"],
                                             '' if s["nnode"] == len(s["nodes"]) else ' (first %d kept)' % len(s["nodes"]), s["nsub"],
                                             '%.3f km' % sk["length_km"].max() if len(s["table"]) else 'n/a'))
                    if not s["converged"]:
                        self.say(' *** WARNING --deform-skeleton window %d mesh %d: the thinning had not ended after %d sub-iterations; '
                                 'the skeleton is not final' % (kw, km, self.skel))
                if self.track is not None:
                    if kw > 0:                           # 24 bytes per pair of features that meet come down
                        m = self.trk.features_match(2 * km + 1, 2 * km, reach=self.track)
                        self.out[pre + "pairs"] = m["pairs"]
                        self.out[pre + "pairs_counts"] = np.array([m["npair"], m["nhit"]], dtype=np.int64)
                        self.links[(km, kw)] = features.link_features(m["pairs"], self.out["m%d_w%d_features" % (km, kw - 1)], f["table"])
                    self.trk.features_advect(jrec1, self.grid, 2 * km, 2 * km + 1, slot=km)   # ... to the start of the next window
        self.clk.add("deform_s", t_d)

    def threshold(self, jrec1, km, kw, what, sgn, pct):
        """--deform-features WHAT@pNN: the threshold at which the cell of rank floor(NN/100 * m) among the m status-1 cells of mesh
        km, and every cell above it, passes the test of mesh_features; no cell: the largest double, which nothing passes"""
        d = self.trk.mesh_dist(jrec1, what=what, sgn=sgn, q=[pct / 100.], slot=km)
        if d["m"] == 0:
            thr = float(np.finfo(np.float64).max)
        else:
            thr = distribution.percentile_threshold(what, d["t2"][0] if what == "tot" else d["values"][0])
        self.say(' *** --deform-features window %d mesh %d: percentile %g of %s over %d cells (rank %d) -> THR = %r /s'
                 % (kw, km, pct, what, d["m"], d["ranks"][0], thr))
        return thr

    def tracks(self):
        """--deform-track, behind the last window: m<k>_w<k>_track and _age of every feature, and one line per window"""
        for km in range(len(self.specs)):
            nrows = [len(self.out["m%d_w%d_features" % (km, kw)]) for kw in range(len(self.win))]
            links = [self.links[(km, kw)] for kw in range(1, len(self.win))]
            track, age = features.feature_tracks(links, nrows)
            for kw in range(len(self.win)):
                self.out["m%d_w%d_track" % (km, kw)], self.out["m%d_w%d_age" % (km, kw)] = track[kw], age[kw]
                if kw > 0:
                    self.say(' *** --deform-track window %d mesh %d: %d continued, %d born, %d ended, %d merged, %d split'
                             % ((kw, km) + features.track_events(links[kw - 1], track[kw - 1], track[kw])))

    def write(self, fname, vTime, kstrt):
        """the run's .npz; vTime: the times of records 0..Nt of the series"""
        if self.track is not None:
            self.tracks()
        pct = self.feat is not None and isinstance(self.feat[2], distribution.Percentile)
        _savez_deflate(fname, meshes=np.array(self.specs, dtype=np.float64).reshape(-1, 2),
                       windows=np.array(self.win, dtype=np.int64).reshape(-1, 2),
                       time0=np.array([vTime[w[0] - kstrt] for w in self.win], dtype=np.int64),
                       time1=np.array([vTime[w[1] - kstrt + 1] for w in self.win], dtype=np.int64), **self.out,
                       **({"grid": np.array(self.grid, dtype=np.float64), "grid_at": np.array(self.grid_at)} if self.grid else {}),
                       **({"coarse": np.array(self.coarse, dtype=np.float64)} if self.coarse else {}),
                       **({"features": np.array((_lib.FEAT_WHAT[self.feat[0]],) + tuple(self.feat[1:]), dtype=np.float64)}
                          if self.feat and not pct else {}),
                       **({"features": np.array((_lib.FEAT_WHAT[self.feat[0]], self.feat[1], np.nan) + tuple(self.feat[3:]), dtype=np.float64),
                           "features_pct": np.array([self.feat[2].pct], dtype=np.float64)} if pct else {}),
                       **({"pdf_%s_edges" % name: edges for name, edges in self.pdf} if self.pdf else {}),
                       **({"pdf_q": np.array(distribution.PDF_Q, dtype=np.float64)} if self.pdf else {}),
                       **({"track": np.array([self.track], dtype=np.int64)} if self.track is not None else {}),
                       **({"skeleton": np.array([self.skel], dtype=np.int64)} if self.skel is not None else {}))


class PairSeries:
    """--pairs: the dispersion of buoy pairs from the positions that live on the GPU: a mark in front of every window of model
    records, a table behind each record the window asks for, all from the window's own t0.
      win      [(jrec0, [jrec1, ...])];  first: model record -> the window it opens;  at: model record -> the window it belongs to"""

    def __init__(self, spec, window, every, Nt, kstrt, ctx, trk, nP, say, clk):
        self.edges, self.rd = spec
        self.ctx, self.trk, self.nP, self.say, self.clk = ctx, trk, nP, say, clk
        self.win = pair_windows(Nt, kstrt, window, every)
        self.first = {w[0]: k for k, w in enumerate(self.win)}
        self.at = {j: k for k, w in enumerate(self.win) for j in w[1]}
        self.out = {k: [] for k in range(len(self.win))}

    def mark(self, kw):
        """in front of the first record of window kw: the t0 of its pairs, the cloud as it is now"""
        t_d = self.clk.now()
        msk = None
        if self.rd > 0.:                                 # the alive cloud, coarsened to spacing rd on the positions as they are now
            st = self.ctx.fetch()
            al = np.asarray(st["alive"]) != 0
            msk = np.zeros(self.nP, dtype=np.int8)
            if al.any():
                msk[np.where(al)[0][self.ctx.subsample_cloud(st["yx"][al], self.rd)[0]]] = 1
        self.trk.pairs_mark(self.win[kw][0], msk)
        self.clk.add("pairs_s", t_d)

    def take(self, jrec1):
        """behind the step of jrec1: the table since the start of its window"""
        t_d = self.clk.now()
        kw = self.at[jrec1]
        r = self.trk.pairs(jrec1, self.edges)
        self.out[kw].append((jrec1, r["T"], r["table"], r["npts"]))
        beta = dispersion.dispersion_exponents(r["table"], r["T"])["beta"]
        self.say(' *** --pairs window %d record %d (T = %g s): %d points, pairs per class %s, beta(1..3) = %s'
                 % (kw, jrec1, r["T"], r["npts"], ' '.join('%d' % n for n in r["table"][:, 0]), ' '.join('%.3f' % b for b in beta)))
        self.clk.add("pairs_s", t_d)

    def write(self, fname, vTime, kstrt):
        members = {}
        for kw, rows in self.out.items():
            members["w%d_jrec1" % kw] = np.array([r[0] for r in rows], dtype=np.int64)
            members["w%d_T" % kw] = np.array([r[1] for r in rows], dtype=np.float64)
            members["w%d_pairs" % kw] = np.array([r[2] for r in rows], dtype=np.float64).reshape(len(rows), len(self.edges) - 1, _lib.PAIRS_NCOLS)
            members["w%d_npts" % kw] = np.array([r[3] for r in rows], dtype=np.int64)
        _savez_deflate(fname, edges=np.asarray(self.edges, dtype=np.float64),
                       windows=np.array([(w[0], w[1][-1]) for w in self.win], dtype=np.int64).reshape(-1, 2),
                       time0=np.array([vTime[w[0] - kstrt] for w in self.win], dtype=np.int64), **members)


class Outputs:
    """The files of positions.  The reference allocates the whole series -- xPosC, xPosG (Nt+1,nP,2) f8, xmask -- and writes it
    at the end (:324-330,515-519).  Here, with -F, the series file is opened at once and every record is appended when it is
    fetched: host memory stays O(nP).  Its time axis is known in advance (record times of the model file).  The always-written
    two-record `tracking12` file keeps every buoy's first and last position: rows 0 and 1 of z2XY, z2GC, zMSK (and zTim in
    2-D-time mode), held on rank 0 only.
      vTime    the times of records 0..Nt of the series (every rank)
      ends     2-D-time mode: the model records some buoy's window closes with; () with -F"""

    def __init__(self, run, seeds, z1st, zLst, records, ctx, stride=1, smp=None, root=True):
        Nt, kstrt, nP = run.Nt, run.kstrt, seeds.nP
        self.run, self.seeds, self.z1st, self.zLst, self.ctx, self.smp = run, seeds, z1st, zLst, ctx, smp
        self.lFull = not run.lUse2DTime
        self.stride = max(1, int(stride)) if self.lFull else 1
        self.vTime = vTime = np.zeros(Nt + 1, dtype=int)
        for jt in range(Nt):
            vTime[jt] = records.time(jt + kstrt) - int(run.rdt / 2.)
        vTime[Nt] = vTime[Nt - 1] + int(run.rdt)
        self.ends = () if self.lFull else set(np.unique(zLst).tolist())
        self.series, self.cf_series, self.zTim = None, None, []
        if not root:
            return
        xPosC0, xPosG0 = seeds.xPosC0, seeds.xPosG0
        if self.lFull:
            self.cf_series = out_file(run, 'tracking', vTime[0], vTime[Nt], tail='_stride%d' % self.stride if self.stride > 1 else '')
            self.series = ncio.CloudBuoysStream(self.cf_series, vTime[::self.stride], seeds.IDs, with_mask=True, corigin=run.corgn,
                                                extra_names=smp.attrs if smp else None)
            # record 0: the seeds as the seeding file gave them (:331-333; in 1-D-time mode every window opens at record 0); with
            # --sample it waits for the fields sampled in the seeds' cells, in front of the first step
            if not smp:
                self.series.put(0, xPosC0[:, 0], xPosC0[:, 1], xPosG0[:, 0], xPosG0[:, 1], np.ones(nP, dtype='i1'))
        self.z2XY, self.z2GC = np.zeros((2, nP, 2)) + FILL, np.zeros((2, nP, 2)) + FILL
        self.zMSK = np.zeros((2, nP), dtype='i1')
        self.z2XY[0], self.z2GC[0], self.zMSK[0] = xPosC0, xPosG0, 1
        if not self.lFull:
            self.zTim = np.zeros((2, nP), dtype=int) + int(FILL)
            self.zTim[0] = run.ztime_model[z1st] - int(run.rdt / 2)
            # a buoy whose window opens later has its seed position pre-written at record k0, and the reference converts
            # that row to lat/lon when it passes over record k0-1 (:493)
            late = z1st - kstrt > 0
            if np.any(late):
                self.z2GC[0, late] = ctx.cart2geo(xPosC0[late])

    def need(self, jrec):
        """does the step of model record jrec produce a record that is written"""
        return output_due(jrec, self.run.kstrt, self.run.Nt, self.lFull, self.stride, self.ends)

    def fetch(self, trk, part, jrec):
        """every rank: the record the step of jrec produced -> (pos, msk, ll) of all buoys in the caller's order on rank 0.
        One record at a time, never the series: xPosC[jt+1], xmask[jt+1] (:459-460) and, for the series, xPosG[jt+1] =
        CartNPSkm2Geo1D of that row, FillValue rows included (:493), converted on the device by the rank that owns the rows"""
        ll = None
        if self.lFull:
            pos_l, msk_l, ll_l = trk.record(jrec, latlon=True)
            ll = part.gather(ll_l)
        else:
            pos_l, msk_l = trk.record(jrec)
        return part.gather(pos_l), part.gather(msk_l), ll

    def _put(self, k, pos, ll, msk, srow):
        try:
            self.series.put(k, pos[:, 0], pos[:, 1], ll[:, 0], ll[:, 1], msk, extra=self.smp.columns(srow) if self.smp else None)
        except BaseException:
            self.series.abort()
            raise

    def seeds_sampled(self, jrec0, srow):
        """rank 0, --sample: the seeds that start at jrec0 were sampled in that record before it moves them: row 0 of the files"""
        self.smp.keep(0, np.where(self.z1st == jrec0)[0], srow)
        if self.lFull:
            self._put(0, self.seeds.xPosC0, self.seeds.xPosG0, np.ones(self.seeds.nP, dtype='i1'), srow)

    def store(self, jrec, pos, msk, ll=None, srow=None):
        """rank 0: what fetch() gave for model record jrec (and, with --sample, the fields sampled behind its step)"""
        run = self.run
        k = jrec - run.kstrt + 1                           # the record of the series
        if self.lFull:
            if k % self.stride == 0:
                self._put(k // self.stride, pos, ll, msk, srow)
            if k == run.Nt:
                self.z2XY[1], self.z2GC[1], self.zMSK[1] = pos, ll, msk
                if self.smp:
                    self.smp.keep(1, slice(None), srow)
        elif jrec in self.ends:
            sel = np.where(self.zLst == jrec)[0]
            self.z2XY[1, sel] = pos[sel]
            self.z2GC[1, sel] = self.ctx.cart2geo(pos[sel])
            self.zMSK[1, sel] = msk[sel]
            self.zTim[1, sel[msk[sel] == 1]] = int(self.vTime[k - 1] + run.rdt)
            if self.smp:
                self.smp.keep(1, sel, srow)

    def write(self):
        """closes the series and writes the tracking12 file (:509-571); returns the files and their first and last date"""
        outs, vTime = [], self.vTime
        if self.lFull:
            self.series.close()                                  # every record is in the file already
            outs.append(self.cf_series)
            zvt = np.array([vTime[0], vTime[self.run.Nt]])
        else:
            zvt = np.array([np.mean(self.zTim[0, :]), np.mean(self.zTim[1, :])])
        cf_nc_out = out_file(self.run, 'tracking12', zvt[0], zvt[1])
        ncio.ncSaveCloudBuoys(cf_nc_out, zvt, self.seeds.IDs, self.z2XY[:, :, 0], self.z2XY[:, :, 1], self.z2GC[:, :, 0], self.z2GC[:, :, 1],
                              mask=self.zMSK, xtime=self.zTim, corigin=self.run.corgn, extra=self.smp.rows() if self.smp else None)
        outs.append(cf_nc_out)
        return outs, zvt


def main(argv=None):
    a = parse_args(argv)
    _tame_malloc()
    clk = _Clock()
    comm = Comm()
    if a.deform and comm.multi:
        comm.close()
        raise ValueError('--deform: the cells of a mesh would span the ranks\' buoy ranges; run it on one rank (%d ranks here)' % comm.world)
    if a.pairs is not None and comm.multi:
        comm.close()
        raise ValueError('--pairs: the pairs would span the ranks\' buoy ranges; run it on one rank (%d ranks here)' % comm.world)
    say = print if comm.root else (lambda *args, **kw: None)
    say('\n *** SITRACK ice particule tracker, GPU build; NetCDF backend = ' + ncio.backend()
        + ('; %d ranks (%s)' % (comm.world, comm.backend) if comm.multi else ''))
    say(' *** SI3 file =>', a.fsi3, '\n *** mesh_mask =>', a.fmmm, '\n *** seeding  =>', a.fsdg, a.krec)
    run = open_run(a, comm, say)
    if run is None:
        comm.close()
        return 0
    Nt, kstrt = run.Nt, run.kstrt

    # ---- mesh, records, seeds
    ctx = _lib.Context(comm.device if comm.multi else a.device)
    tk = clk.now()
    mesh = read_mesh(a, ctx)
    records = ncio.ModelRecords(a.fsi3)
    smp_attrs, smp_dtype = sample_vars(a.sample, records, a.fsi3, kstrt, mesh.Nj, mesh.Ni)
    tk = clk.add("read_mesh_s", tk)
    seeds = init_seeds(a, run, mesh, records, comm, ctx, say)
    tk = clk.add("seed_init_and_cache_s", tk)
    z1st, zLst = seed_windows(run, seeds, say)
    windows = (z1st, zLst) if run.lUse2DTime else None
    nP = seeds.nP

    # ---- device state, and the stages that apply to this run (None: not asked for)
    part = Partition(comm, seeds.vJIt, nP, mesh.Nj, windows)
    trk, K, K_plan, tphase = open_tracker(a, run, mesh, records, ctx)
    trk.set_buoys(seeds.xPosC0[part.mine], seeds.vJIt[part.mine], z1st[part.mine] if windows else None, zLst[part.mine] if windows else None)
    smp = Sampler(a.sample, smp_attrs, smp_dtype, ctx, records, part, clk, kstrt, K, mesh.Nj, mesh.Ni, z1st if windows else None) if a.sample else None
    out = Outputs(run, seeds, z1st, zLst, records, ctx, a.out_stride, smp, comm.root)
    bcast = record_broadcaster(a, comm, ctx, tphase)
    ingest = BoxIngest(ctx, records, comm, clk, kstrt, K, mesh.Nj, ctx.field_dtype.itemsize, a.full_records, tphase is not None, bcast)
    dfm = DeformSeries(a.deform, a.deform_window, mesh.dfm_grid, a.deform_grid and a.deform_grid[1], Nt, kstrt, ctx, trk, seeds.IDs, nP,
                       say, clk, coarse=a.deform_coarse, feat=a.deform_features, track=a.deform_track,
                       skel=a.deform_skeleton, pdf=a.deform_pdf) if a.deform else None
    prs = PairSeries(a.pairs, a.pairs_window, a.pairs_every, Nt, kstrt, ctx, trk, nP, say, clk) if a.pairs is not None else None

    # ---- the record loop (:361-496).  The reference steps record by record; here consecutive records go through ONE
    #      fused launch (sitrk_run: every buoy still takes every step, only the loop nest is interchanged) whenever no
    #      per-record output is due between them -- always in the default 2-D-time mode, which writes first/last positions
    #      only (:565-571).  Records are read straight into the library's pinned staging and uploaded on its copy stream
    #      while the previous batch is stepped with; `-F` / `-p` need every record's positions: batches of one.
    batches = plan_batches(Nt, kstrt, K_plan, out.lFull, out.stride, out.ends, smp.firsts if smp and run.lUse2DTime else None,
                           cuts=(set(dfm.last) if dfm else set()) | (set(prs.at) if prs else set()) if dfm or prs else None)
    tplan = plan_tinterp(batches, Nt, K) if tphase is not None else None
    due = rebalance_due(batches, a.rebalance, comm.multi)
    tk = clk.add("setup_s", tk)
    t_loop = clk.now()
    if batches:
        ingest.upload(*batches[0])
    for ib, (jt0, m) in enumerate(batches):
        jrec0, jrecN = jt0 + kstrt, jt0 + m - 1 + kstrt
        if m == 1:
            nalive = comm.sum_int(trk.alive_count())
            say(' *** record #%d/%d  date = %s   buoys alive = %d' % (jrec0 + 1, run.Nt0, epoch2clock(out.vTime[jt0]), nalive))
        else:
            say(' *** records #%d..#%d/%d  dates = %s .. %s   (one fused launch)'
                % (jrec0 + 1, jrecN + 1, run.Nt0, epoch2clock(out.vTime[jt0]), epoch2clock(out.vTime[jt0 + m - 1])))
        t_q = clk.now()
        used = [(jt0 + r) % K for r in range(m)]
        if bcast is not None:
            bcast.before_run(used)
        if smp and jrec0 in smp.firsts:
            srow = smp.sample(jrec0, ingest.boxes.get(jt0), 'enter')
            if comm.root:
                out.seeds_sampled(jrec0, srow)
            t_q = clk.now()
        if dfm and jrec0 in dfm.first:
            dfm.build(dfm.first[jrec0])
            t_q = clk.now()
        if prs and jrec0 in prs.first:
            prs.mark(prs.first[jrec0])
            t_q = clk.now()
        if tplan is None:
            trk.run(jrec0, jt0 % K, m)
        else:
            # --tinterp: the first record of the next batch is this batch's last partner: it travels in front of the launch
            # (the GPU has not been given this batch's m records yet when its box is worked out)
            if tplan[ib]["ahead"] is not None:
                ingest.plan(*batches[ib + 1], not_queued=m)
                ingest.upload_recs(batches[ib + 1][0], [tplan[ib]["ahead"]])
                t_q = clk.now()
            trk.run(jrec0, jt0 % K, m, tinterp=tphase, have_prev=tplan[ib]["have_prev"], have_next=tplan[ib]["have_next"])
        if bcast is not None:
            bcast.after_run(used)
        clk.add("enqueue_stepping_s", t_q)
        if ib + 1 < len(batches) and not due[ib]:
            if tplan is None:
                ingest.upload(*batches[ib + 1])           # travels while the launch above runs
            else:
                ingest.upload_recs(batches[ib + 1][0], tplan[ib]["behind"])
        if dfm and jrecN in dfm.last:
            dfm.take(dfm.last[jrecN])
        if prs and jrecN in prs.at:
            prs.take(jrecN)
        t_f = clk.now()
        if out.need(jrecN):
            rec = out.fetch(trk, part, jrecN)
            srow = None
            if smp:
                t_f = clk.add("fetch_and_store_outputs_s", t_f)
                srow = smp.sample(jrecN, ingest.boxes.get(jt0), 'after')
                t_f = clk.now()
            if comm.root:
                out.store(jrecN, *rec, srow)
        clk.add("fetch_and_store_outputs_s", t_f)
        if due[ib]:
            t_r = clk.now()
            part.rebalance(ctx, ingest)
            clk.add("rebalance_s", t_r)
            ingest.upload(*batches[ib + 1])
            if tplan is not None:
                # the next batch's first partner was uploaded over the box of this rank's former buoys: once more, over the new one
                ingest.upload_recs(batches[ib + 1][0], [jt0 + m - 1])
    ctx.sync()
    if bcast is not None:
        bcast.close()
    clk.add("record_loop_s", t_loop)
    record_bytes = 3 * mesh.Nj * mesh.Ni * ctx.field_dtype.itemsize
    if not a.full_records:
        # what box ingest bought, per rank (every rank prints its own line)
        print(' *** rank %d read and uploaded %.1f MB of the %.1f MB of its %d records (box ingest: the rows x columns its own buoys can touch)'
              % (comm.rank, ingest.bytes / 1e6, record_bytes * Nt / 1e6, Nt), flush=True)
    tk = clk.now()
    records.close()
    launches = ctx.launch_stats()
    state = trk.state()
    vJIt_end, alive_end = part.gather(state["vJIt"]), part.gather(state["iAlive"])
    trk.close()
    if not comm.root:
        comm.close()
        return {"rank": comm.rank, "nP": nP, "range": part.range, "upload_bytes": ingest.bytes}

    # ---- outputs (:509-571)
    outs, zvt = out.write()
    if dfm:
        outs.append(out_file(run, 'deformation', out.vTime[0], out.vTime[Nt], ext='npz'))
        dfm.write(outs[-1], out.vTime, kstrt)
    if prs:
        outs.append(out_file(run, 'pairs', out.vTime[0], out.vTime[Nt], ext='npz'))
        prs.write(outs[-1], out.vTime, kstrt)
    if a.plot > 0:
        try:
            import mojito as mjt          # noqa: F401  optional, as in the reference (:20,587-600)
            print(' *** `mojito` found: map plotting is left to the reference tooling (positions are in ' + outs[0] + ')')
        except Exception:                 # noqa: BLE001
            print(' *** `-p`: package `mojito` not available here => no maps (positions are in ' + outs[0] + ')')
    print(' *** first and final dates in simulated trajectories:', epoch2clock(zvt[0]), epoch2clock(zvt[1]))
    for f in outs:
        print('      ===> ' + f + ' saved!')
    clk.add("write_outputs_s", tk)
    clk.t["total_s"] = clk.now() - clk.t0
    comm.close()
    return {"files": outs, "nP": nP, "IDs": seeds.IDs, "vJIt": vJIt_end, "iAlive": alive_end, "Nt": Nt, "kstrt": kstrt,
            "timing": dict(clk.t), "launches": launches, "upload_bytes": ingest.bytes, "record_bytes": record_bytes,
            "rebalances": part.rebalances, "migrated": part.migrated}
