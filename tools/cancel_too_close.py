#!/usr/bin/env python3
"""Overlap cleaning of a trajectory file the tracker wrote (the 2-record file or the `-F` series): CancelTooClose at record
KREC and scale RDKM km (reference sitrack/util.py:520-565), on the GPU, then the same schema restricted to the kept buoys.

    python tools/cancel_too_close.py -i FILE -k KREC -r RDKM [-o OUT]

Validity comes from `mask` when the file has it, otherwise from the `_FillValue` of `latitude`.  The per-buoy counts of
valid records are summed record by record, so reading costs O(Nbuoy) memory whatever the number of records; the output
(the kept buoys' records, `time_pos` carried when present) is assembled in memory and written by ncio.ncSaveCloudBuoys.
Default OUT: FILE with `_ctc<RDKM>km` before its extension."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sitrack_amd as sit                      # noqa: E402
from sitrack_amd import ncio                   # noqa: E402


def _valid_row(f, k, has_mask, lat_fill):
    if has_mask:
        return np.asarray(f.var('mask', k)) != 0
    lat = np.asarray(f.var('latitude', k))
    ok = np.isfinite(lat)
    if lat_fill is not None:
        ok &= lat != np.asarray(lat_fill).astype(lat.dtype)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description='CancelTooClose on a trajectory file (MI355X build)')
    ap.add_argument('-i', '--fin', required=True, help='trajectory file written by the tracker')
    ap.add_argument('-k', '--krec', type=int, required=True, help='record at which the cloud is cleaned')
    ap.add_argument('-r', '--rdkm', type=float, required=True, help='distance criterion for the elimination [km]')
    ap.add_argument('-o', '--fout', default=None, help='output file (default: <input>_ctc<rdkm>km.nc)')
    ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args(argv)
    ncio.chck4f(a.fin)
    if not (np.isfinite(a.rdkm) and 0. < a.rdkm <= 9999.):
        sys.exit('ERROR: -r must be finite and in (0, 9999] km')
    with ncio._Reader(a.fin) as f:
        for cv in ('time', 'id_buoy', 'latitude', 'longitude', 'y_pos', 'x_pos'):
            if not f.has_var(cv):
                sys.exit('ERROR: no variable `%s` in %s' % (cv, a.fin))
        nrec, nb = f.dim('time'), f.dim('buoy')
        krec = a.krec
        if not -nrec <= krec < nrec:
            sys.exit('ERROR: -k %d outside the %d records of %s' % (krec, nrec, a.fin))
        krec %= nrec
        has_mask, has_tpos = f.has_var('mask'), f.has_var('time_pos')
        lat_fill = f.fill_of('latitude')
        nall = np.zeros(nb, dtype=np.int32)
        nbef = None
        for t in range(nrec):
            if t == krec:
                nbef = nall.copy()
                valid = _valid_row(f, t, has_mask, lat_fill)
                nall += valid
            else:
                nall += _valid_row(f, t, has_mask, lat_fill)
        _, _, zLatLon, _ = ncio.LoadNCdata(a.fin, krec=krec)
        lat, lon = zLatLon[:, 0], zLatLon[:, 1]
        ctx = sit.Context(a.device)
        keep, nclose = ctx.cancel_too_close(lat, lon, valid, nall, nbef, a.rdkm)
        idx = np.flatnonzero(keep)
        print(' *** CancelTooClose at record %d, scale %g km: %d valid buoys, %d closer than that to another'
              % (krec, a.rdkm, int(valid.sum()), nclose))
        print('      => we remove %d buoys at all records!' % (int(valid.sum()) - len(idx)))
        ptime = f.var('time')
        ids = np.asarray(f.var('id_buoy'))[idx]
        out = {v: np.empty((nrec, len(idx)), dtype=np.float32) for v in ('latitude', 'longitude', 'y_pos', 'x_pos')}
        if has_mask:
            out['mask'] = np.empty((nrec, len(idx)), dtype=np.int8)
        if has_tpos:
            out['time_pos'] = np.empty((nrec, len(idx)), dtype=np.int32)
        for t in range(nrec):
            for v in out:
                out[v][t] = np.asarray(f.var(v, t))[idx]
    fout = a.fout or '%s_ctc%gkm.nc' % (os.path.splitext(a.fin)[0], a.rdkm)
    ncio.ncSaveCloudBuoys(fout, ptime, ids, out['y_pos'], out['x_pos'], out['latitude'], out['longitude'],
                          mask=out.get('mask', []), xtime=out.get('time_pos', []),
                          cauthor='cancel_too_close.py')
    print(' *** kept %d of %d buoys -> %s' % (len(idx), nb, fout))
    return 0


if __name__ == '__main__':
    sys.exit(main())
