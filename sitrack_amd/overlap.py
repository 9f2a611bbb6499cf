"""Overlap cleaning of a tracked cloud: host side of the reference's `CancelTooClose` (sitrack/util.py:520-565).

The work runs on the GPU (`sitrk_cancel_too_close`, sitrack_amd/csrc/sitrk_overlap.hip): the nearest other buoy of every
buoy within `rdkm`, the compaction of the buoys that have one, and the reference's sequential scan over those.  There is
no host version.  The contract and its one extension (buoys invalid at `krec`) are in include/sitrk.h and DESIGN.md 3.6."""
import math

import numpy as np


def record_counts(pmsk, krec):
    """(nall, nbef): per buoy, the number of records with pmsk != 0 in all records and in the records before `krec`, summed
    record by record so that no (Nrec, Nbuoy) temporary is made."""
    nrec, nb = np.shape(pmsk)
    nall = np.zeros(nb, dtype=np.int32)
    nbef = None
    for t in range(nrec):
        if t == krec:
            nbef = nall.copy()
        nall += np.asarray(pmsk[t]) != 0
    return nall, (nall.copy() if nbef is None else nbef)


def CancelTooClose(krec, rdkm, plat, plon, pmsk, NbPass=2, iverbose=0, ctx=None):
    """Reference sitrack/util.py:520-565, same positional parameters and return pair (nBn, idx_keep): at record `krec` of
    the (Nrec, Nbuoy) series plat/plon/pmsk, of two buoys closer than `rdkm` km (the reference Haversine) one goes -- the
    one with the shorter series, the neighbour on equal counts -- scanning the buoys in index order.  `idx_keep` (int64)
    are the buoys left at `krec`, `nBn` their number.  Runs on the GPU.  Every pass of the reference starts afresh, so
    `NbPass` (>= 1) does not change the result and one pass is run.  Extension: a buoy with pmsk[krec] == 0 takes no part
    (the reference raises IndexError there); it is not in `idx_keep`.  Raises ValueError on bad arguments before any
    device work."""
    from .tracking import default_context
    cerr = 'ERROR [CancelTooClose()]: '
    if isinstance(NbPass, bool) or not isinstance(NbPass, (int, np.integer)) or NbPass < 1:
        raise ValueError(cerr + '`NbPass` must be an integer >= 1, got %r' % (NbPass,))
    try:
        rd = float(rdkm)
    except (TypeError, ValueError):
        raise ValueError(cerr + '`rdkm` must be a number, got %r' % (rdkm,)) from None
    if not math.isfinite(rd) or not 0. < rd <= 9999.:
        raise ValueError(cerr + '`rdkm` must be finite and in (0, 9999] km, got %r' % (rdkm,))
    if np.ndim(plat) != 2 or np.ndim(plon) != 2 or np.ndim(pmsk) != 2:
        raise ValueError(cerr + '`plat`, `plon` and `pmsk` must be 2-D (Nrec, Nbuoy) arrays')
    nrec, nb = np.shape(pmsk)
    if np.shape(plat) != (nrec, nb) or np.shape(plon) != (nrec, nb):
        raise ValueError(cerr + '`plat`, `plon` and `pmsk` must share one shape, got %s, %s, %s'
                         % (np.shape(plat), np.shape(plon), np.shape(pmsk)))
    if isinstance(krec, bool) or not isinstance(krec, (int, np.integer)) or not -nrec <= krec < nrec:
        raise ValueError(cerr + '`krec` must be an integer record index of the %d records, got %r' % (nrec, krec))
    krec = int(krec) % nrec
    valid = np.asarray(pmsk[krec]) != 0
    lat = np.asarray(plat[krec], dtype=np.float64)
    lon = np.asarray(plon[krec], dtype=np.float64)
    bad = np.flatnonzero(valid & ~(np.isfinite(lat) & np.isfinite(lon)))
    if len(bad):
        raise ValueError(cerr + 'non-finite coordinate of a valid buoy at index %d' % bad[0])
    nall, nbef = record_counts(pmsk, krec)
    if iverbose > 0:
        print('\n *** Applying initial overlap cleaning at the scale of ' + str(rdkm) + ' km')
    keep, _ = (ctx or default_context()).cancel_too_close(lat, lon, valid, nall, nbef, rd)
    idx_keep = np.flatnonzero(keep).astype(np.int64)
    nBn = len(idx_keep)
    if iverbose > 0:
        print('      => we remove ' + str(int(valid.sum()) - nBn) + ' buoys at all records!')
    return nBn, idx_keep
