#!/usr/bin/env python3
"""Quadrangles of buoys from a triangulation of one record of a trajectory file the tracker wrote, on the GPU (sitrk_tri2quad;
contract in include/sitrk.h).

    python tools/generate_quad_mesh.py -i TRACKFILE [-k K0] -t TRIS.npy|auto|gpu [--rmax KM] [--angles LO,HI --ratio R --area MIN,MAX] -o CELLS.npy

TRIS.npy is an (nT, 3) integer array of `id_buoy` values, either orientation.  `-t auto` triangulates the valid positions of
record K0 (Delaunay; needs scipy).  `-t gpu --rmax KM` triangulates them on the device: every Delaunay triangle whose
circumradius is at most KM km (sitrk_delaunay), so no triangle spans open water or land wider than that.
Adjacent triangles are paired into strictly convex quadrangles whose interior angles lie in [LO, HI] degrees (default 60,120), whose shortest side is at least R times the longest (default 0.5) and whose area lies in
[MIN, MAX] km^2 (default: any), best pairs first.  CELLS.npy holds the (nQ, 4) `id_buoy` values of the quadrangles,
counter-clockwise: what `tools/deformation.py -c CELLS.npy` takes as it is.  Validity comes from `mask` when the file has it,
otherwise from the `_FillValue` of `y_pos`; a triangle with a buoy that is not valid at K0 pairs with nothing."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sitrack_amd as sit                      # noqa: E402
from sitrack_amd import ncio                   # noqa: E402
from sitrack_amd.quadmesh import _params       # noqa: E402
from sitrack_amd.delaunay import _rmax         # noqa: E402


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


def _auto_tris(yx, ok):
    try:
        from scipy.spatial import Delaunay
    except ImportError:
        sys.exit('ERROR: `-t auto` needs scipy (scipy.spatial.Delaunay), which cannot be imported: give the triangles with -t TRIS.npy')
    idx = np.flatnonzero(ok)
    if len(idx) < 3:
        sys.exit('ERROR: `-t auto`: fewer than 3 valid buoys at record K0')
    return idx[Delaunay(yx[idx]).simplices].astype(np.int64)


def _pair(text, opt):
    try:
        lo, hi = (float(v) for v in text.split(','))
    except ValueError:
        sys.exit('ERROR: %s takes two numbers `A,B`, got %r' % (opt, text))
    return lo, hi


def main(argv=None):
    ap = argparse.ArgumentParser(description='quadrangles of buoys from a triangulated record of a trajectory file (MI355X build)')
    ap.add_argument('-i', '--fin', required=True, help='trajectory file written by the tracker')
    ap.add_argument('-k', '--k0', type=int, default=0, help='record whose positions are meshed (default 0)')
    ap.add_argument('-t', '--tris', required=True,
                    help='(nT,3) .npy array of id_buoy values, `auto` (Delaunay on the host, needs scipy) or `gpu` (bounded Delaunay on the device, needs --rmax)')
    ap.add_argument('--rmax', type=float, default=None, help='with `-t gpu`: largest circumradius of a triangle [km], in (0, 500]')
    ap.add_argument('--angles', default='60,120', help='smallest,largest interior angle [degrees] (default 60,120)')
    ap.add_argument('--ratio', type=float, default=0.5, help='shortest / longest side, at least (default 0.5)')
    ap.add_argument('--area', default='0,inf', help='smallest,largest area [km^2] (default 0,inf)')
    ap.add_argument('-o', '--fout', required=True, help='output .npy file: (nQ,4) id_buoy values')
    ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args(argv)
    angles, area = _pair(a.angles, '--angles'), _pair(a.area, '--area')
    for opt, kw in (('--angles', dict(angles=angles)), ('--ratio', dict(ratio_min=a.ratio)), ('--area', dict(area=area))):
        try:
            _params('', np.zeros((0, 3), dtype=np.int32), **dict(dict(angles=(60., 120.), ratio_min=0.5, area=(0., float('inf'))), **kw))
        except ValueError as e:
            sys.exit('ERROR: %s: %s' % (opt, e))
    if a.tris == 'gpu':
        if a.rmax is None:
            sys.exit('ERROR: `-t gpu` needs --rmax KM, the largest circumradius of a triangle')
        try:
            _rmax('', a.rmax)
        except ValueError as e:
            sys.exit('ERROR: --rmax: %s' % e)
    elif a.rmax is not None:
        sys.exit('ERROR: --rmax goes with `-t gpu` only')
    ncio.chck4f(a.fin)
    with ncio._Reader(a.fin) as f:
        for cv in ('time', 'id_buoy', 'y_pos', 'x_pos'):
            if not f.has_var(cv):
                sys.exit('ERROR: no variable `%s` in %s' % (cv, a.fin))
        nrec = f.dim('time')
        if not -nrec <= a.k0 < nrec:
            sys.exit('ERROR: -k %d outside the %d records of %s' % (a.k0, nrec, a.fin))
        k0 = a.k0 % nrec
        ids = np.asarray(f.var('id_buoy')).astype(np.int64)
        yx, ok = _record(f, k0, f.has_var('mask'))
    ctx = None
    if a.tris == 'auto':
        cols = _auto_tris(yx, ok)
    elif a.tris == 'gpu':
        ctx = sit.Context(a.device)
        cols = sit.DelaunayTris(yx, a.rmax, mask=ok, ctx=ctx)
    else:
        ncio.chck4f(a.tris)
        tri_ids = np.load(a.tris, allow_pickle=False)
        if tri_ids.ndim != 2 or tri_ids.shape[1] != 3 or tri_ids.dtype.kind not in 'iu':
            sys.exit('ERROR: %s must hold an (nT,3) integer array, got %s %s' % (a.tris, tri_ids.dtype, tri_ids.shape))
        tri_ids = tri_ids.astype(np.int64)
        order = np.argsort(ids, kind='stable')
        pos = np.searchsorted(ids[order], tri_ids)
        hit = np.take(ids[order], np.minimum(pos, len(ids) - 1)) == tri_ids if len(ids) else np.zeros(tri_ids.shape, dtype=bool)
        if not hit.all():
            sys.exit('ERROR: id_buoy %d of %s is not in %s' % (tri_ids[~hit][0], a.tris, a.fin))
        cols = order[pos]
    ctx = ctx or sit.Context(a.device)
    try:
        quads, tri_quad = sit.Tri2Quad(yx, cols, mask=ok, angles=angles, ratio_min=a.ratio, area=area, ctx=ctx)
    finally:
        ctx.close()
    np.save(a.fout, ids[quads])
    print(' *** record %d: %d triangles (%d dead) -> %d quadrangles, %d triangles left single -> %s' %
          (k0, len(cols), int((tri_quad == -2).sum()), len(quads), int((tri_quad == -1).sum()), a.fout))
    return 0


if __name__ == '__main__':
    sys.exit(main())
