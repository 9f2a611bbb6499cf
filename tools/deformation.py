#!/usr/bin/env python3
"""Deformation rates of buoy triangles / quadrangles between two records of a trajectory file the tracker wrote (the
2-record file or the `-F` series), on the GPU (sitrk_deform_cells; contract in include/sitrk.h).

    python tools/deformation.py -i TRACKFILE -c CELLS.npy [-k K0] [-K K1] [--pdf WHAT@LO:HI:NB[@lin|log][,...]] [--grid D_KM [--coarse NLEV[@FMIN]] [--features WHAT@THR[@MINPIX[@CONN]] [--track [REACH]] [--skeleton [MAXSUB]]]]
                                [-o OUT.npz]

CELLS.npy is an (nC, 3) or (nC, 4) integer array of `id_buoy` values, either orientation.  `-c auto` triangulates the valid
positions of record K0 (Delaunay; needs scipy).  Records default to the first and the last; the elapsed time comes from
`time`; validity from `mask` when the file has it, otherwise from the `_FillValue` of `y_pos`.  OUT (default: TRACKFILE
with `_deform.npz` for its extension) holds div, shr, vor, tot [1/s], area0, area1 [km^2], valid, cells (the ids) and
time0, time1.  `--grid D_KM` also rasterises the cells at their K0 positions onto square pixels of D_KM km over the bounding
box of the valid points (sitrk_raster_cells): OUT then holds `owner` (ny, nx) int32, per pixel the row of the
valid cell its centre lies in (the lowest on a shared edge, -1 for none), and `grid` = (y0, x0, d, ny, nx); a map is
`div[owner]` where owner >= 0.  `--coarse NLEV[@FMIN]` with it coarse-grains the valid cells on NLEV levels of boxes of side
D_KM*2^l over that grid (sitrk_coarse_cells): OUT then holds `coarse_table` (NLEV, 8) -- per level the boxes
with a cell, the boxes filled to FMIN (default 0.5) of their area and over those the sums of A, A*div, A*shr, A*tot^q, q = 1,
2, 3 --, `coarse` = (nlev, fmin) and `beta` (3,), the scaling exponents sit.scaling_exponents reads off the table.
`--features WHAT@THR[@MINPIX[@CONN]]` with --grid takes that map apart into its features (sitrk_label_raster): the
mask -- the pixels with an owner whose rate passes the threshold: WHAT = div (div >= THR), conv (-div >= THR), shr, vor or tot
(div^2 + shr^2 >= THR^2), THR in 1/s -- is made here from `owner` and the rates, and its connected components (CONN = 4 or 8
neighbours, default 8) of at least MINPIX pixels (default 1) are labelled on the GPU: OUT then holds `features` (rows, 12)
int64 -- label, npix, jmin, jmax, imin, imax, the sums of j, i, j^2, i^2, j*i, the perimeter --, `features_counts` = (nfeat,
ncomp, nactive) and `features_arg` = (what, sgn, thr, min_pix, conn).
`--track [REACH]` with --features links those features to the ones of the next window of as many records, K1 -> K2 = K1 + (K1 - K0),
for the same cells: the labels are carried to record K1 by their own cells -- a cell takes the lowest label
among the pixels it owns at K0 and gives it to the pixels it owns at K1, here in numpy --, the next window's map is drawn at K1
on the same grid, and the two are matched on the GPU within REACH pixels (0..2, default 1; sitrk_features_match).  OUT then
holds `next_features`, `pairs` (npair, 3) -- label, label in the next window, pixels where they meet --, `pairs_counts` =
(npair, nhit), `parent` per row of next_features and `child` per row of features (sit.link_features) and `track_arg` = (reach, K2).
`--skeleton [MAXSUB]` with --features thins those features to their skeletons on the GPU (sitrk_skeleton_raster),
by at most MAXSUB sub-iterations (1..2^20, default 4096): OUT then holds `skeleton` (rows, 7) int64 -- label, npix, skeleton
pixels, ends, junctions, orthogonal and diagonal links, one row per row of `features` --, `skeleton_nodes` (rows, 3) int64 --
pixel, label, X of every end, junction and isolated pixel --, `skeleton_counts` = (nfeat, nnode, nskel, nsub, converged) and
`skeleton_arg` = (max_sub,).
`--pdf WHAT@LO:HI:NB[@lin|log][,...]` takes the distribution of a rate over the valid cells on the GPU (sitrk_dist_values;
DESIGN.md 3.21): WHAT = div, conv (-div), shr, vor, tot, adiv (|div|) or avor (|vor|), NB bins (1..1024) from LO to HI, geometric
(`log`, the default, LO > 0) or equidistant.  OUT then holds `pdf_<WHAT>` (NB+2) int64 -- the cells below LO, in each bin, at or
above HI --, `q_<WHAT>`, the exact quantiles `pdf_q` = 0.5, 0.75, 0.85, 0.9, 0.95, 0.99, each the rate of one cell, and
`pdf_<WHAT>_edges`.  `--features WHAT@pNN[...]` states the threshold as the NN-th percentile of the rate over the valid cells; it
is resolved the same way (sit.percentile_threshold) and stored as `features_thr`.

Caveat: the files hold positions as f4 km.  At |x| ~ 3000 km that is 0.24 m of rounding per coordinate, 2e-5 of a 10-km
cell -- the size of the strains of interest over a few hours.  A running tracker holds the positions in fp64 on the device:
IceTracker.deform_mark() / .deform() take the rates there."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sitrack_amd as sit                      # noqa: E402
from sitrack_amd import ncio                   # noqa: E402

CAVEAT = (' *** NOTE: the file holds positions as f4 km: at |x| ~ 3000 km that is 0.24 m of rounding per coordinate, 2e-5 of a\n'
          '     10-km cell, the size of the strains of interest over a few hours; a running tracker takes the rates from its\n'
          '     fp64 positions on the device (IceTracker.deform_mark / deform).')


def _record(f, k, has_mask):
    """(yx (nb,2) fp64, valid (nb,) bool) of record k"""
    y = np.asarray(f.var('y_pos', k))
    x = np.asarray(f.var('x_pos', k))
    if has_mask:
        ok = np.asarray(f.var('mask', k)) != 0
    else:
        ok = np.isfinite(y) & np.isfinite(x)
        for a, nm in ((y, 'y_pos'), (x, 'x_pos')):
            fv = f.fill_of(nm)
            if fv is not None:
                ok &= a != np.asarray(fv).astype(a.dtype)
    return np.stack([y.astype(np.float64), x.astype(np.float64)], axis=1), ok


def _auto_cells(yx, ok):
    try:
        from scipy.spatial import Delaunay
    except ImportError:
        sys.exit('ERROR: `-c auto` needs scipy (scipy.spatial.Delaunay), which cannot be imported: give the cells with -c CELLS.npy')
    idx = np.flatnonzero(ok)
    if len(idx) < 3:
        sys.exit('ERROR: `-c auto`: fewer than 3 valid buoys at the first record')
    return idx[Delaunay(yx[idx]).simplices].astype(np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser(description='deformation rates of buoy cells from a trajectory file (MI355X build)')
    ap.add_argument('-i', '--fin', required=True, help='trajectory file written by the tracker')
    ap.add_argument('-c', '--cells', required=True, help='(nC,3|4) .npy array of id_buoy values, or `auto` (Delaunay, needs scipy)')
    ap.add_argument('-k', '--k0', type=int, default=0, help='first record (default 0)')
    ap.add_argument('-K', '--k1', type=int, default=-1, help='second record (default: the last)')
    ap.add_argument('-o', '--fout', default=None, help='output file (default: <input>_deform.npz)')
    ap.add_argument('--grid', type=float, default=None, metavar='D_KM',
                    help='also rasterise the valid cells at their first-record positions onto pixels of D_KM km (`owner`, `grid` in the output)')
    ap.add_argument('--coarse', default=None, metavar='NLEV[@FMIN]',
                    help='with --grid: also coarse-grain the valid cells on NLEV levels over that grid (`coarse_table`, `coarse`, `beta` in the output)')
    ap.add_argument('--features', default=None, metavar='WHAT@THR[@MINPIX[@CONN]]',
                    help='with --grid: also label the connected features of the map where the rate WHAT (div, conv, shr, vor, tot) passes '
                         'THR [1/s] (`features`, `features_counts`, `features_arg` in the output)')
    ap.add_argument('--pdf', default=None, metavar='WHAT@LO:HI:NB[@lin|log][,...]',
                    help='also the distribution of the rate WHAT (div, conv, shr, vor, tot, adiv, avor) over the valid cells: NB bins from LO '
                         'to HI [1/s] and six exact quantiles (`pdf_<WHAT>`, `q_<WHAT>`, `pdf_<WHAT>_edges`, `pdf_q` in the output)')
    ap.add_argument('--track', nargs='?', const='1', default=None, metavar='REACH',
                    help='with --features: also link the features to those of the next window of as many records, K1 -> K1 + (K1 - K0), '
                         'within REACH pixels (0..2, default 1) (`next_features`, `pairs`, `pairs_counts`, `parent`, `child`, '
                         '`track_arg` in the output)')
    ap.add_argument('--skeleton', nargs='?', const='4096', default=None, metavar='MAXSUB',
                    help='with --features: also thin the features to their skeletons, by at most MAXSUB sub-iterations (1..2^20, default '
                         '4096) (`skeleton`, `skeleton_nodes`, `skeleton_counts`, `skeleton_arg` in the output)')
    ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args(argv)
    max_sub = None
    if a.skeleton is not None:
        from sitrack_amd.features import skeleton_arg
        if a.features is None:
            sys.exit('ERROR: --skeleton: it thins the features of --features; give that flag too')
        try:
            max_sub = skeleton_arg(a.skeleton, '--skeleton')
        except ValueError as e:
            sys.exit('ERROR: %s' % e)
    reach = None
    if a.track is not None:
        from sitrack_amd.features import track_arg
        if a.features is None:
            sys.exit('ERROR: --track: it links the features of --features; give that flag too')
        try:
            reach = track_arg(a.track, '--track')
        except ValueError as e:
            sys.exit('ERROR: %s' % e)
    feat = None
    if a.features is not None:
        from sitrack_amd.features import features_arg
        if a.grid is None:
            sys.exit('ERROR: --features: it works on the grid of --grid; give that flag too')
        try:
            feat = features_arg(a.features, '--features')
        except ValueError as e:
            sys.exit('ERROR: %s' % e)
    pdf = None
    if a.pdf is not None:
        try:
            pdf = sit.pdf_arg(a.pdf, '--pdf')
        except ValueError as e:
            sys.exit('ERROR: %s' % e)
    coarse = None
    if a.coarse is not None:
        from sitrack_amd.coarse import coarse_arg
        if a.grid is None:
            sys.exit('ERROR: --coarse: it works on the grid of --grid; give that flag too')
        try:
            coarse = coarse_arg(a.coarse)
        except ValueError as e:
            sys.exit('ERROR: %s' % e)
    if a.grid is not None and not (np.isfinite(a.grid) and a.grid > 0.):
        sys.exit('ERROR: --grid: D_KM must be finite and > 0, got %r' % a.grid)
    ncio.chck4f(a.fin)
    with ncio._Reader(a.fin) as f:
        for cv in ('time', 'id_buoy', 'y_pos', 'x_pos'):
            if not f.has_var(cv):
                sys.exit('ERROR: no variable `%s` in %s' % (cv, a.fin))
        nrec = f.dim('time')
        ks = []
        for opt, k in (('-k', a.k0), ('-K', a.k1)):
            if not -nrec <= k < nrec:
                sys.exit('ERROR: %s %d outside the %d records of %s' % (opt, k, nrec, a.fin))
            ks.append(k % nrec)
        k0, k1 = ks
        vtime = np.asarray(f.var('time')).astype(np.int64)
        T = float(vtime[k1] - vtime[k0])
        if not T > 0.:
            sys.exit('ERROR: record %d (time %d) is not later than record %d (time %d)' % (k1, vtime[k1], k0, vtime[k0]))
        ids = np.asarray(f.var('id_buoy')).astype(np.int64)
        has_mask = f.has_var('mask')
        yx0, ok0 = _record(f, k0, has_mask)
        yx1, ok1 = _record(f, k1, has_mask)
        if reach is not None:
            k2 = k1 + (k1 - k0)
            if not k1 < k2 < nrec:
                sys.exit('ERROR: --track: the next window ends at record %d, outside the %d records of %s' % (k2, nrec, a.fin))
            yx2, ok2 = _record(f, k2, has_mask)
            T2 = float(vtime[k2] - vtime[k1])
            if not T2 > 0.:
                sys.exit('ERROR: --track: record %d (time %d) is not later than record %d (time %d)' % (k2, vtime[k2], k1, vtime[k1]))
    if a.cells == 'auto':
        cols = _auto_cells(yx0, ok0 & ok1)
        cell_ids = ids[cols]
    else:
        ncio.chck4f(a.cells)
        cell_ids = np.load(a.cells, allow_pickle=False)
        if cell_ids.ndim != 2 or cell_ids.shape[1] not in (3, 4) or cell_ids.dtype.kind not in 'iu':
            sys.exit('ERROR: %s must hold an (nC,3) or (nC,4) integer array, got %s %s' % (a.cells, cell_ids.dtype, cell_ids.shape))
        cell_ids = cell_ids.astype(np.int64)
        order = np.argsort(ids, kind='stable')
        pos = np.searchsorted(ids[order], cell_ids)
        hit = np.take(ids[order], np.minimum(pos, len(ids) - 1)) == cell_ids if len(ids) else np.zeros(cell_ids.shape, dtype=bool)
        if not hit.all():
            sys.exit('ERROR: id_buoy %d of %s is not in %s' % (cell_ids[~hit][0], a.cells, a.fin))
        cols = order[pos]
    print(CAVEAT)
    ctx = sit.Context(a.device)
    try:
        r = sit.DeformCells(yx0, yx1, cols, T, mask0=ok0, mask1=ok1, ctx=ctx)
        from sitrack_amd import distribution as dst
        for name, edges in pdf or ():
            d = dst.rate_distribution(r, name, edges=edges, q=dst.PDF_Q, use=r['valid'], ctx=ctx)
            r['pdf_' + name], r['q_' + name], r['pdf_%s_edges' % name] = d['counts'], d['values'], edges
            print(' *** --pdf %s: %d cells, %d below / %d at or above the edges, median %.6e /s, p95 %.6e /s'
                  % (name, d['m'], d['counts'][0], d['counts'][-1], d['values'][0], d['values'][4]))
        if pdf:
            r['pdf_q'] = np.array(dst.PDF_Q, dtype=np.float64)
        if a.grid is not None:
            if not ok0.any():
                sys.exit('ERROR: --grid: no valid buoy at record %d' % k0)
            grid = sit.raster_grid(yx0[ok0, 0].min(), yx0[ok0, 0].max(), yx0[ok0, 1].min(), yx0[ok0, 1].max(), a.grid)
            if grid[3] * grid[4] > 2 ** 28:
                sys.exit('ERROR: --grid: %g km over the points is %d x %d pixels, more than 2^28' % (a.grid, grid[3], grid[4]))
            r['owner'] = sit.RasterCells(yx0, cols, grid, draw=r['valid'], ctx=ctx)
            r['grid'] = np.array(grid, dtype=np.float64)
            if coarse is not None:
                if grid[3] * grid[4] > 2 ** 24:
                    sys.exit('ERROR: --coarse: %g km over the points is %d x %d pixels, more than 2^24' % (a.grid, grid[3], grid[4]))
                rc = sit.CoarseCells(yx0, yx1, cols, T, grid, coarse[0], fmin=coarse[1], mask0=ok0, mask1=ok1, ctx=ctx)
                r['coarse_table'], r['coarse'] = rc['table'], np.array(coarse, dtype=np.float64)
                r['beta'] = sit.scaling_exponents(rc['table'], a.grid)['beta']
            if feat is not None:
                if grid[3] > 32768 or grid[4] > 32768:
                    sys.exit('ERROR: --features: %g km over the points is %d x %d pixels, more than 32768 a side' % (a.grid, grid[3], grid[4]))
                what, sgn, thr, min_pix, conn = feat
                if isinstance(thr, dst.Percentile):                    # WHAT@pNN: resolved on the GPU over the valid cells
                    pct = thr.pct
                    d = dst.rate_distribution(r, 'conv' if (what, sgn) == ('div', -1) else what, q=[pct / 100.], use=r['valid'], ctx=ctx)
                    thr = (dst.percentile_threshold(what, d['t2'][0] if what == 'tot' else d['values'][0]) if d['m']
                           else float(np.finfo(np.float64).max))
                    r['features_thr'], r['features_pct'] = np.float64(thr), np.float64(pct)
                    print(' *** --features: percentile %g of %s over %d cells (rank %d) -> THR = %r /s' % (pct, what, d['m'], d['ranks'][0], thr))

                def labelled(rates, own):
                    at = np.maximum(own, 0)
                    with np.errstate(invalid='ignore'):
                        if what == 'tot':
                            hit = rates['div'][at] * rates['div'][at] + rates['shr'][at] * rates['shr'][at] >= thr * thr
                        else:
                            hit = sgn * rates[what][at] >= thr
                    return sit.LabelRaster((own >= 0) & hit, conn=conn, min_pix=min_pix, ctx=ctx)

                rf = labelled(r, r['owner'])
                r['features'] = rf['table']
                r['features_counts'] = np.array([rf['nfeat'], rf['ncomp'], rf['nactive']], dtype=np.int64)
                r['features_arg'] = np.array([sit.FEAT_WHAT[what], sgn, thr, min_pix, conn], dtype=np.float64)
                if max_sub is not None:
                    from sitrack_amd import features as ft
                    rs = ctx.skeleton_raster(ft.kept_labels(rf['labels'], min_pix), max_sub=max_sub, skel=False)
                    r['skeleton'], r['skeleton_nodes'] = rs['table'], rs['nodes']
                    r['skeleton_counts'] = np.array([rs['nfeat'], rs['nnode'], rs['nskel'], rs['nsub'], rs['converged']], dtype=np.int64)
                    r['skeleton_arg'] = np.array([max_sub], dtype=np.int64)
                if reach is not None:
                    # the features carried by their own cells to record K1, where the next window's map is drawn on the same grid
                    from sitrack_amd import features as ft
                    own1 = sit.RasterCells(yx1, cols, grid, draw=r['valid'], ctx=ctx)
                    carried, _ = ft.advect_labels(ft.kept_labels(rf['labels'], min_pix), r['owner'], own1, len(cols))
                    rn = sit.DeformCells(yx1, yx2, cols, T2, mask0=ok1, mask1=ok2, ctx=ctx)
                    rfn = labelled(rn, sit.RasterCells(yx1, cols, grid, draw=rn['valid'], ctx=ctx))
                    m = sit.MatchLabels(carried, ft.kept_labels(rfn['labels'], min_pix), reach=reach, ctx=ctx)
                    link = ft.link_features(m['pairs'], rf['table'], rfn['table'])
                    r['next_features'], r['pairs'] = rfn['table'], m['pairs']
                    r['pairs_counts'] = np.array([m['npair'], m['nhit']], dtype=np.int64)
                    r['parent'], r['child'], r['track_arg'] = link['parent'], link['child'], np.array([reach, k2], dtype=np.int64)
                    events = ft.track_events(link, *ft.feature_tracks([link], [len(rf['table']), len(rfn['table'])])[0])
    finally:
        ctx.close()
    fout = a.fout or os.path.splitext(a.fin)[0] + '_deform.npz'
    np.savez(fout, cells=cell_ids, time0=vtime[k0], time1=vtime[k1], **r)
    print(' *** records %d -> %d (T = %g s): %d of %d cells valid -> %s' % (k0, k1, T, int(r['valid'].sum()), len(cell_ids), fout))
    if a.grid is not None:
        print(' *** --grid %g km: %d x %d pixels, %d of them in a valid cell' % (a.grid, r['owner'].shape[0], r['owner'].shape[1],
                                                                               int((r['owner'] >= 0).sum())))
    if coarse is not None:
        print(' *** --coarse %d levels, fmin %g: filled boxes %s, beta(1..3) = %s'
              % (coarse[0], coarse[1], '/'.join('%d' % n for n in r['coarse_table'][:, 1]), ', '.join('%.4f' % b for b in r['beta'])))
    if feat is not None:
        n = r['features_counts']
        lengths = sit.feature_table(r['features'], tuple(r['grid'][:3]) + (r['owner'].shape[0], r['owner'].shape[1]))['length_km']
        print(' *** --features %s: %d features of >= %d pixels (%d components, %d active pixels), longest %s'
              % (a.features, n[0], feat[3], n[1], n[2], '%.3f km' % lengths.max() if len(lengths) else 'n/a'))
    if max_sub is not None:
        n = r['skeleton_counts']
        lengths = sit.skeleton_table(r['skeleton'], tuple(r['grid'][:3]) + (r['owner'].shape[0], r['owner'].shape[1]))['length_km']
        print(' *** --skeleton %d: %d features, %d skeleton pixels, %d nodes in %d sub-iterations, longest %s'
              % (max_sub, n[0], n[2], n[1], n[3], '%.3f km' % lengths.max() if len(lengths) else 'n/a'))
        if not n[4]:
            print(' *** WARNING --skeleton: the thinning had not ended after %d sub-iterations; the skeleton is not final' % max_sub)
    if reach is not None:
        print(' *** --track %d: records %d -> %d against %d -> %d: %d pairs, %d continued, %d born, %d ended, %d merged, %d split'
              % ((reach, k0, k1, k1, k2, r['pairs_counts'][0]) + events))
    return 0


if __name__ == '__main__':
    sys.exit(main())
