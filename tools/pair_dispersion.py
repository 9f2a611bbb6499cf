#!/usr/bin/env python3
"""Dispersion of buoy pairs between two records of a trajectory file the tracker wrote (the 2-record file or the `-F` series),
on the GPU (sitrk_pairs_points; contract in include/sitrk.h).

    python tools/pair_dispersion.py -i TRACKFILE [-k K0,K1] --edges R_LO:R_HI:NC|e0,e1,... [--min-pairs N] [-o OUT.npz]

For every pair of buoys valid at both records whose separation r0 at record K0 lies in a class [e_c, e_c+1) km -- NC geometric
classes from R_LO to R_HI, or the explicit edges -- the strain e = (r1 - r0)/r0 of the separation at record K1.  Records default
to the first and the last; the elapsed time T comes from `time`; validity from `mask` when the file has it, otherwise from the
`_FillValue` of `y_pos`.  OUT (default: TRACKFILE with `_pairs.npz` for its extension) holds `edges`, `table` (nc, 7) -- per class
the pairs and the sums of r0, e, |e|, e^2, |e|^3 and (r1 - r0)^2 --, `npts`, `T`, `time0`, `time1` and the curve
sit.dispersion_curve reads off the table: `L_km`, `rate` (nc, 3) = <|e|^q>/T^q, `mean` = <e>/T, `d2` = <(r1 - r0)^2>, and `beta`
(3,), the exponents of sit.dispersion_exponents over the classes with at least N pairs (default 10).  The work grows with the pairs
within the last edge: about nP * density * pi * e_nc^2 / 2.

Caveat: the files hold positions as f4 km.  At |x| ~ 3000 km that is 0.24 m of rounding per coordinate, 2e-5 of a 10-km
separation -- the size of the strains of interest over a few hours.  A running tracker holds the positions in fp64 on the device:
IceTracker.pairs_mark() / .pairs(), or `--pairs` of the command line, take the tables there."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sitrack_amd as sit                      # noqa: E402
from sitrack_amd import _lib, ncio             # noqa: E402
from deformation import CAVEAT, _record        # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description='dispersion of buoy pairs from a trajectory file (MI355X build)')
    ap.add_argument('-i', '--fin', required=True, help='trajectory file written by the tracker')
    ap.add_argument('-k', '--recs', default='0,-1', metavar='K0,K1', help='the two records (default 0,-1: the first and the last)')
    ap.add_argument('--edges', required=True, metavar='R_LO:R_HI:NC|e0,e1,...', help='the class edges in km')
    ap.add_argument('--min-pairs', type=int, default=10, help='pairs a class needs to enter the fit of the exponents (default 10)')
    ap.add_argument('-o', '--fout', default=None, help='output file (default: <input>_pairs.npz)')
    ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args(argv)
    try:
        edges = sit.pairs_arg(a.edges, '--edges')
    except ValueError as e:
        sys.exit('ERROR: %s' % e)
    try:
        k0, k1 = (int(x) for x in a.recs.split(','))
    except ValueError:
        sys.exit('ERROR: -k: expected K0,K1, got %r' % a.recs)
    ncio.chck4f(a.fin)
    with ncio._Reader(a.fin) as f:
        for cv in ('time', 'id_buoy', 'y_pos', 'x_pos'):
            if not f.has_var(cv):
                sys.exit('ERROR: no variable `%s` in %s' % (cv, a.fin))
        nrec = f.dim('time')
        for k in (k0, k1):
            if not -nrec <= k < nrec:
                sys.exit('ERROR: -k: record %d outside the %d records of %s' % (k, nrec, a.fin))
        k0, k1 = k0 % nrec, k1 % nrec
        vtime = np.asarray(f.var('time')).astype(np.int64)
        T = float(vtime[k1] - vtime[k0])
        if not T > 0.:
            sys.exit('ERROR: record %d (time %d) is not later than record %d (time %d)' % (k1, vtime[k1], k0, vtime[k0]))
        has_mask = f.has_var('mask')
        yx0, ok0 = _record(f, k0, has_mask)
        yx1, ok1 = _record(f, k1, has_mask)
    print(CAVEAT.replace('deform_mark / deform', 'pairs_mark / pairs').replace('10-km cell', '10-km separation'))
    ctx = _lib.Context(a.device)
    try:
        r = sit.PairDispersion(yx0, yx1, edges, mask0=ok0, mask1=ok1, ctx=ctx)
    finally:
        ctx.close()
    cur = sit.dispersion_curve(r["table"], T)
    fit = sit.dispersion_exponents(r["table"], T, min_pairs=a.min_pairs)
    print(' *** records %d -> %d, T = %g s, %d valid buoys, %d pairs' % (k0, k1, T, r["npts"], int(r["table"][:, 0].sum())))
    print('     class  edges [km]            pairs     L [km]   <|e|>/T [1/s]  <e>/T [1/s]   <d^2> [km^2]')
    for c in range(len(edges) - 1):
        print('     %5d  %8.3f .. %8.3f %9d %10.3f   %13.6e %13.6e %13.6e'
              % (c, edges[c], edges[c + 1], int(r["table"][c, 0]), cur["L_km"][c], cur["rate"][c, 0], cur["mean"][c], cur["d2"][c]))
    print('     beta(1..3) = %s over %d classes' % (' '.join('%.4f' % b for b in fit["beta"]), int(fit["used"].sum())))
    fout = a.fout or os.path.splitext(a.fin)[0] + '_pairs.npz'
    np.savez(fout, edges=edges, table=r["table"], npts=np.int64(r["npts"]), T=np.float64(T), time0=vtime[k0], time1=vtime[k1],
             L_km=cur["L_km"], rate=cur["rate"], mean=cur["mean"], d2=cur["d2"], beta=fit["beta"], used=fit["used"])
    print('      ===> ' + fout + ' saved!')
    return fout


if __name__ == "__main__":
    main()
