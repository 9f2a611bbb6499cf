#!/usr/bin/env python3
"""Seeding file on the model grid -- the flags of the reference tools generate_idealized_seeding.py /
generate_sidfex_seeding.py (-d -m -i -v -k -S -f -C -N, --lsidfex).  Writes
./nc/sitrack_seeding_<nemoTsi3|nemoTmm|sidfex>_<YYYYMMDD_hh>[_HSS<S>|_<C>km].nc with the schema of reference
ncio.py:131-197.  `--lsidfex 1` seeds from a text file `id lon lat` (reference tools/sidfexloc.dat).

`-C <C>` coarsens the seed cloud to a spacing of about C km (reference :158-186, :323-360): the seeds' [y,x] km go through
`SubSampCloud` (greedy sparsification at radius rd_ss, on the GPU) and the kept rows keep their IDs, lat/lon and y/x;
C = 10 and 20 add the mesh's F-points to the T-seeds first.  rd_ss = 6.0 / 14.6 / 34.5 / 74.75 / 156. / 315.6 km for
C = 10 / 20 / 40 / 80 / 160 / 320.  C = 640 also needs the reference's dist-to-coast file and mojito's `MaskCoastal`, and is
refused; so is any other value.  A SIDFEx cloud is coarsened the same way, without F-points.

`--min-dist-land <KM>` (extra) is the coastal cleaning on its own, against the model's own coastline instead of a dist-to-coast
raster: after the seeding and before the coarsening (the reference's order), seeds closer than KM km to the nearest edge
between a sea and a land T-cell of the mesh file are removed (`Context.coast_build` on its `tmask` and F-points, then
`MaskCoastal`; distances in the polar-stereographic plane).  It combines with any `-C`; the file name gains `_dl<KM>km`."""
import argparse
import os
import sys
from datetime import datetime, timezone

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sitrack_amd as sit                      # noqa: E402
from sitrack_amd import driver, ncio           # noqa: E402
from sitrack_amd.seeding import nemoSeed, SidfexSeeding       # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description='SITRACK idealised seeding (MI355X build)')
    ap.add_argument('-d', '--dat0', required=True, help='initial date in the form <YYYY-MM-DD_hh:mm:ss>')
    ap.add_argument('-m', '--fmmm', default=None, help='model `mesh_mask` file of NEMO config used in SI3 run')
    ap.add_argument('--lsidfex', type=int, default=0, help='Switch to 1 for SIDFEX seeding.')
    ap.add_argument('--sidfex-file', default='./sidfexloc.dat', help='text file `id lon lat` (extra; the reference hard-codes ./sidfexloc.dat)')
    ap.add_argument('-i', '--fsi3', default=None, help='output file of SI3 containing sea-ice concentration')
    ap.add_argument('-v', '--nsic', default='siconc', help='name of sea-ice concentration in SI3 file')
    ap.add_argument('-k', '--krec', type=int, default=0, help='use sea-ice concentration at this record')
    ap.add_argument('-S', '--ihss', type=int, default=1, help='horizontal subsampling factor to apply')
    ap.add_argument('-f', '--fmsk', default=None, help='mask (on SI3 model domain) to control seeding region')
    ap.add_argument('-C', '--crsn', type=int, default=0, help='coarsening in km: 10, 20, 40, 80, 160 or 320')
    ap.add_argument('-N', '--ncnf', default='NANUK4', help='name of the horizontak NEMO config used')
    ap.add_argument('--min-dist-land', type=float, default=None, metavar='KM',
                    help='extra: remove the seeds closer than KM km to the coastline of the mesh (needs `-m`)')
    ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args(argv)
    rd_ss, add_f = coarsening(a.crsn)
    if a.min_dist_land is not None:
        if not (np.isfinite(a.min_dist_land) and a.min_dist_land > 0.):
            raise SystemExit('ERROR: `--min-dist-land` must be a finite distance > 0 km (got %r)' % a.min_dist_land)
        if not a.fmmm:
            raise SystemExit('ERROR: `--min-dist-land` needs the MeshMask file (`-m`): the coastline is the mesh\'s own')
    if a.ihss < 1 or a.ihss > 20:
        raise SystemExit('ERROR: chosen horizontal subsampling makes no sense iHSS=%d' % a.ihss)
    seeding_type = 'sidfex' if a.lsidfex == 1 else ('nemoTsi3' if a.fsi3 else 'nemoTmm')
    ctx = sit.Context(a.device)
    if seeding_type == 'sidfex':
        XseedGC, zIDs = SidfexSeeding(a.sidfex_file)
        if a.min_dist_land is not None:
            imaskt, _, _, _, _, xYf, xXf, _ = ncio.GetModelGrid(a.fmmm, ctx=ctx)
            ctx.coast_build(xYf, xXf, imaskt)
        return write_seeding(ctx, a, seeding_type, XseedGC, zIDs, rd_ss=rd_ss)
    if not a.fmmm:
        raise SystemExit('ERROR: you have to specify a MeshMask file with `-m`')
    if add_f:
        imaskt, xlatT, xlonT, xYt, xXt, xYf, xXf, xResKM, _, xlatF, xlonF = ncio.GetModelGrid(a.fmmm, alsoF=True, ctx=ctx)
    else:
        imaskt, xlatT, xlonT, xYt, xXt, xYf, xXf, xResKM = ncio.GetModelGrid(a.fmmm, ctx=ctx)
        xlatF, xlonF = [], []
    if a.fsi3:
        rec = ncio.ModelRecords(a.fsi3)
        (xIC,) = rec.fields(a.krec, (a.nsic,))
        rec.close()
        if np.shape(xIC) != np.shape(imaskt):
            raise SystemExit('ERROR: wrong shape for sea-ice concentration read')
    else:
        xIC = np.ones(np.shape(imaskt))
    FSmask = []
    if a.fmsk:
        with ncio._Reader(a.fmsk) as f:
            FSmask = np.array(f.var('tmask'), dtype='i1')
        if np.shape(FSmask) != np.shape(imaskt):
            raise SystemExit('ERROR: `shape(FSmask) != shape(imaskt)`')
    # which points carry a seed, their order and their projection: one call into the library (sitrk_nemo_seed)
    XseedGC, XseedYX = nemoSeed(imaskt, xlatT, xlonT, xIC, khss=a.ihss, fmsk_rstrct=FSmask, platF=xlatF, plonF=xlonF,
                                ctx=ctx, return_yx=True)
    zIDs = np.arange(1, XseedGC.shape[0] + 1, dtype=int)
    if a.min_dist_land is not None:
        ctx.coast_build(xYf, xXf, imaskt)
    return write_seeding(ctx, a, seeding_type, XseedGC, zIDs, XseedYX, rd_ss)


# -C <km> -> (rd_ss km, add F-points): reference :158-186
RD_SS = {10: (6.0, True), 20: (14.6, True), 40: (34.5, False), 80: (74.75, False), 160: (156., False), 320: (315.6, False)}


def coarsening(icrsn):
    """(rd_ss, add F-points) for `-C icrsn`, (None, False) without coarsening; SystemExit for what cannot be done."""
    if icrsn < 1:
        return None, False
    if icrsn == 640:
        raise SystemExit('ERROR: -C 640 also removes seeds near the coast: it needs the dist-to-coast file '
                         '$DATA_DIR/data/dist2coast/dist2coast_4deg_North.nc and mojito\'s `MaskCoastal`, which this build does not have')
    if icrsn not in RD_SS:
        raise SystemExit('ERROR: we do not know what `rd_ss` to pick for `icrsn` = %d (known: %s)' %
                         (icrsn, ', '.join(str(k) for k in sorted(RD_SS))))
    return RD_SS[icrsn]


def write_seeding(ctx, a, seeding_type, XseedGC, zIDs, XseedYX=None, rd_ss=None):
    t0 = driver.clock2epoch(a.dat0)
    if XseedYX is None:
        XseedYX = sit.Geo2CartNPSkm1D(XseedGC, ctx=ctx)
    cdate = datetime.fromtimestamp(t0, timezone.utc).strftime("%Y%m%d_%H")
    cextra = '_HSS' + str(a.ihss) if a.ihss > 1 else ''
    if a.min_dist_land is not None:
        # coastal cleaning (reference :276-306), on the coast index the caller built from the mesh
        nP0 = XseedGC.shape[0]
        mask = sit.MaskCoastal(XseedGC, rMinDistLand=a.min_dist_land, ctx=ctx)
        print(' * Need to remove ' + str(nP0 - np.sum(mask)) + ' points because too close to land! (' + str(a.min_dist_land) + 'km)')
        (idxKeep,) = np.where(mask == 1)
        XseedGC, XseedYX, zIDs = XseedGC[idxKeep, :], XseedYX[idxKeep, :], np.asarray(zIDs)[idxKeep]
    if rd_ss is not None:
        nP0 = XseedGC.shape[0]
        print(' *** Applying spatial sub-sampling with radius: %.2fkm' % rd_ss)
        _, XseedYX, idxKeep = sit.SubSampCloud(rd_ss, XseedYX, ctx=ctx)
        XseedGC = XseedGC[idxKeep, :]
        zIDs = np.asarray(zIDs)[idxKeep]
        print('    ==> nP, nPss = %d %d' % (nP0, len(idxKeep)))
        cextra = '_%dkm' % a.crsn
    if a.min_dist_land is not None:
        cextra += '_dl%gkm' % a.min_dist_land
    nP = XseedGC.shape[0]
    foutnc = './nc/sitrack_seeding_' + seeding_type + '_' + cdate + cextra + '.nc'
    ncio.ncSaveCloudBuoys(foutnc, np.array([t0], dtype='i4'), zIDs, XseedYX[None, :, 0], XseedYX[None, :, 1],
                          XseedGC[None, :, 0], XseedGC[None, :, 1], corigin='idealized_seeding', cauthor='generate_idealized_seeding.py')
    print(' *** %d buoys seeded => %s' % (nP, foutnc))
    return foutnc


if __name__ == '__main__':
    main()
