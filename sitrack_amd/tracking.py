"""Host-side mirror of the reference's `sit.*` functions on the hot path.

Same names, argument order and return shapes/dtypes as the reference
(`sitrack/tracking.py`, `sitrack/util.py`), so a driver written against the
reference cannot tell; the arithmetic runs in libsitrk.so on the GPU through
the C ABI of include/sitrk.h.  There is no CPU fallback.
"""
import numpy as np

from . import _lib

FillValue = _lib.FillValue     # sitrack/ncio.py:19
rmin_conc = 0.1                # sitrack/tracking.py:4
rFoundKM = 2.5                 # sitrack/tracking.py:5

_default_ctx = None


def default_context(device=0):
    """Process-wide context (one process = one GPU)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = _lib.Context(device)
    return _default_ctx


def vertices_of(jiT):
    """VRTCS from vJIt: [[jT-1,jT-1,jT,jT],[iT-1,iT,iT,iT-1]] (reference locate.py:320-321;
    tracking.py:257-300 shifts both identically, so VRTCS is a pure function of vJIt)."""
    jiT = np.asarray(jiT, dtype=np.int64)
    j, i = jiT[:, 0], jiT[:, 1]
    v = np.empty((jiT.shape[0], 2, 4), dtype=np.int64)
    v[:, 0, 0] = j - 1; v[:, 0, 1] = j - 1; v[:, 0, 2] = j; v[:, 0, 3] = j
    v[:, 1, 0] = i - 1; v[:, 1, 1] = i; v[:, 1, 2] = i; v[:, 1, 3] = i - 1
    return v


def GetTimeSpan(dt, vtime_mod, iSdA, iMdA, iMdB, iStop=None, iverbose=0):
    """First and last model record of a run (reference sitrack/tracking.py:8-37, same arguments and 5-tuple; raises where
    the reference prints and exits).  `vtime_mod` holds the record centres, the seeding date `iSdA` must fall inside the
    model span shifted back by half a step; the run starts at the first record centred strictly after the seeding date
    and ends at the record nearest to `iStop`, or at the last one."""
    centres = np.asarray(vtime_mod)
    half = dt / 2
    if not (iMdA - half <= iSdA <= iMdB - half):
        raise ValueError("PROBLEM: time in the seeding file (%d) is outside of what model spans!" % iSdA)
    first = int(np.abs(centres - iSdA).argmin())
    if centres[first] <= iSdA:
        first += 1
    last = int(np.abs(centres - iStop).argmin()) if iStop else len(centres) - 1
    if iverbose > 0:
        print('    * [GetTimeSpan]: records %d..%d => %d model records' % (first, last, last - first + 1))
    return last - first + 1, first, last, centres[first], centres[last]


def SeedInit(pIDs, pSG, pSC, platT, plonT, pYf, pXf, pResolKM, maskT, xIceConc=[], iverbose=0, ctx=None):
    """Reference sitrack/tracking.py:98-178, same 7-tuple:
    (nP, pSG[iKeep], pSC[iKeep], pIDs[iKeep], zjiT[iKeep] (nP,2) int, zJIvrt[iKeep] (nP,2,4) int, iKeep)."""
    pSG = np.asarray(pSG)
    pSC = np.asarray(pSC)
    (nP, n2) = np.shape(pSG)
    if np.shape(pSC) != (nP, n2):
        raise ValueError('ERROR [SeedInit]: shape disagreement for `pSG` and `pSC`!')
    if n2 != 2:
        raise ValueError('ERROR [SeedInit]: wrong shape for `pSG` and `pSC`!')
    if len(np.shape(xIceConc)) != 2:
        # the reference raises UnboundLocalError in Survive() here (tracking.py:86-89)
        raise ValueError('SeedInit: `xIceConc` must be the 2-D ice concentration at the seeding record')
    own = ctx is None
    if own:
        ctx = _lib.Context(default_context().device)
    try:
        if (ctx.Nj, ctx.Ni) != np.shape(pYf) or own:
            # only F-points and the mask are read by the locate kernels
            ctx.set_grid(pYf, pXf, pYf, pXf, pYf, pXf, maskT)
        jiT, keep, why = ctx.seed_init(pSG, pSC, platT, plonT, pResolKM, xIceConc)
    finally:
        if own:
            ctx.close()
    pIDs = np.asarray(pIDs)
    iKeep = np.arange(nP, dtype=int)
    nPn = int(np.sum(keep))
    if nPn < nP:
        (iKeep,) = np.where(keep == 1)
        if iverbose > 0:
            print(' * [SeedInit()]: ' + str(nP - nPn) + ' "to-be-seeded" buoys have to be canceled.')
        nP = nPn
    zjiT = jiT.astype(np.int64)
    zJIvrt = vertices_of(zjiT)
    return nP, pSG[iKeep, :], pSC[iKeep, :], pIDs[iKeep], zjiT[iKeep, :], zJIvrt[iKeep, :, :], iKeep


def FindContainingCell(pyx, kjiT, pYf=None, pXf=None, ctx=None):
    """Vectorised reference sitrack/locate.py:280-330: pyx (n,2), kjiT (n,2) ->
    (lPin (n) bool, jiT (n,2) int64, vertices (n,2,4) int64).  Needs a context whose grid is set."""
    ctx = ctx or default_context()
    found, ji = ctx.find_cells(pyx, kjiT)
    ji = ji.astype(np.int64)
    return found, ji, vertices_of(ji)


def CartNPSkm2Geo1D(pcoorC, lat0=70., lon0=-45., ctx=None):
    """Reference sitrack/util.py:413-429: (n,2) [y,x] km -> (n,2) [lat,lon] degrees."""
    (_, n2) = np.shape(pcoorC)
    if n2 != 2:
        raise ValueError(' ERROR [CartNPSkm2Geo1D()]: input array `pcoorC` has a wrong a shape!')
    return (ctx or default_context()).cart2geo(pcoorC, lat0, lon0)


def Geo2CartNPSkm1D(pcoorG, lat0=70., lon0=-45., ctx=None):
    """Reference sitrack/util.py:394-410: (n,2) [lat,lon] degrees -> (n,2) [y,x] km."""
    (_, n2) = np.shape(pcoorG)
    if n2 != 2:
        raise ValueError(' ERROR [Geo2CartNPSkm1D()]: input array `pcoorG` has a wrong a shape!')
    return (ctx or default_context()).geo2cart(pcoorG, lat0, lon0)


def ConvertGeo2CartesianNPSkm(plat, plon, lat0=70., lon0=-45., ctx=None):
    """reference util.py:434-451: geographic (lat, lon) [deg], any shape -> (Y, X) [km] of the WGS84 north polar
    stereographic plane (true-scale latitude lat0, central longitude lon0), same shape.  Projection on the device."""
    ctx = ctx or default_context()
    shp = np.shape(plat)
    ll = np.stack([np.asarray(plat, dtype=np.float64).ravel(), np.asarray(plon, dtype=np.float64).ravel()], axis=1)
    yx = ctx.geo2cart(ll, lat0, lon0)
    return np.ascontiguousarray(yx[:, 0].reshape(shp)), np.ascontiguousarray(yx[:, 1].reshape(shp))


def ConvertCartesianNPSkm2Geo(pY, pX, lat0=70., lon0=-45., ctx=None):
    """reference util.py:455-472: the inverse, (Y, X) [km] -> (lat, lon) [deg], same shape."""
    ctx = ctx or default_context()
    shp = np.shape(pX)
    yx = np.stack([np.asarray(pY, dtype=np.float64).ravel(), np.asarray(pX, dtype=np.float64).ravel()], axis=1)
    ll = ctx.cart2geo(yx, lat0, lon0)
    return np.ascontiguousarray(ll[:, 0].reshape(shp)), np.ascontiguousarray(ll[:, 1].reshape(shp))


def tinterp_phase(tinterp):
    """The `phase` of sitrk_run_tlerp from what IceTracker.run / --tinterp take: 'centre' = 0.5 (records are time means centred
    on their step interval, what NEMO writes), 'start' = 0 (snapshots at its start), or the number itself."""
    if isinstance(tinterp, str):
        try:
            return {'centre': 0.5, 'center': 0.5, 'start': 0.0}[tinterp]
        except KeyError:
            raise ValueError("tinterp: expected 'centre', 'start' or a number in [0,1], got %r" % tinterp)
    ph = float(tinterp)
    if not 0.0 <= ph <= 1.0:
        raise ValueError("tinterp: the phase must be in [0,1], got %r" % tinterp)
    return ph


class IceTracker:
    """The record loop body of the reference driver (si3_part_tracker.py:361-496) as an object.

    Holds the loop's state on the GPU.  Typical use, mirroring the driver:

        trk = IceTracker(xYf, xXf, xYu, xXu, xYv, xXv, imaskt, rdt=3600., iUVstrategy=1)
        trk.set_buoys(xPosC0, vJIt, z1stModelRec, zLstModelRec)
        for jt in range(Nt):
            jrec = jt + kstrt
            trk.load_record(0, xUu, xVv, xIC)          # :372-374
            trk.step(jrec, 0)                           # :378-490
            xPosC[jt+1], xmask[jt+1,:,0], xPosG[jt+1] = trk.record(jrec, latlon=True)   # :459-460,493
    """

    def __init__(self, xYf, xXf, xYu, xXu, xYv, xXv, imaskt, rdt=3600., iUVstrategy=1, rmin=rmin_conc,
                 nslots=1, field_dtype=np.float32, device=0, ctx=None, nsub=1):
        """`nsub` (extra): every record is advanced in nsub Euler sub-steps of rdt/nsub (sitrk_set_substeps)."""
        self.ctx = ctx or _lib.Context(device)
        self.ctx.set_grid(xYf, xXf, xYu, xXu, xYv, xXv, imaskt)
        self.ctx.set_params(rdt, iUVstrategy, rmin)
        self.ctx.set_substeps(nsub)
        self.ctx.alloc_records(nslots, field_dtype)
        self._rdt = float(rdt)
        self._pairs_jrec0 = None

    def set_buoys(self, xPosC0, vJIt, z1stModelRec=None, zLstModelRec=None, sort=True):
        self.ctx.set_buoys(xPosC0, vJIt, z1stModelRec, zLstModelRec, sort=sort)
        self._pairs_jrec0 = None                            # the library cancels the mark of pairs_mark()

    def _check_exact(self, xUu, xVv, xIC):
        dt = self.ctx.field_dtype
        for nm, a in (("u_ice", xUu), ("v_ice", xVv), ("siconc", xIC)):
            a = np.asarray(a)
            if a.dtype.newbyteorder('=') == dt:              # same type up to byte order (NetCDF-3 data are big-endian)
                continue
            if not np.array_equal(a.astype(dt).astype(a.dtype), a, equal_nan=True):
                raise ValueError("%s is not exactly representable as %s; allocate float64 records" % (nm, dt))

    def load_record(self, slot, xUu, xVv, xIC):
        """Fields must be exactly representable in the record dtype (NEMO output is f4)."""
        self._check_exact(xUu, xVv, xIC)
        self.ctx.push_record(slot, xUu, xVv, xIC)

    def band(self, age=0):
        """Rows [j0,j1) of the next record(s) that this tracker's buoys can touch (see sitrk_buoy_rows)."""
        return self.ctx.band(age)

    def load_record_rows(self, slot, j0, j1, xUu_rows, xVv_rows, xIC_rows):
        """Row-band ingest: only rows [j0,j1) of the record, as returned by band()."""
        self._check_exact(xUu_rows, xVv_rows, xIC_rows)
        self.ctx.push_record_rows(slot, j0, j1, xUu_rows, xVv_rows, xIC_rows)

    def step(self, jrec, slot=0):
        self.ctx.step(slot, jrec)

    def run(self, jrec0, slot0, nrec, tinterp=None, have_prev=False, have_next=False):
        """records jrec0 .. jrec0+nrec-1 from slots (slot0+k) % nslots: one fused launch where the library can
        (sitrk_run), same results as nrec calls of step().
        `tinterp` (extra): None = every sub-step of a record uses that record's velocities; a number in [0,1], 'centre' (0.5)
        or 'start' (0) = the velocities are interpolated linearly in time between consecutive records (sitrk_run_tlerp), the
        value being where in its step interval a record is valid; have_prev / have_next: records jrec0-1 / jrec0+nrec are
        resident in the slots in front of slot0 / behind the last one and are blended with."""
        if tinterp is not None:
            self.ctx.run_tlerp(slot0, jrec0, nrec, tinterp_phase(tinterp), have_prev, have_next)
        elif nrec == 1:
            self.ctx.step(slot0, jrec0)
        else:
            self.ctx.run(slot0, jrec0, nrec)

    def record(self, jrec, latlon=False):
        return self.ctx.fetch_record(jrec, latlon=latlon)

    def sample(self, jrec, fields=None, slot=None, mode='after'):
        """Model fields at every buoy's host cell (an extra the reference does not have; sitrk_sample_*): mode 'after' = right
        after the step of jrec, for the buoys record(jrec) masks 1; 'enter' = before it, for the buoys that start at jrec;
        -9999 elsewhere, no interpolation.  `fields`: a dict name -> (Nj,Ni) array or a list / tuple of them, all float32 or
        all float64; the string 'siconc' (as a value or list entry) is served from the resident record in `slot`.  Returns a
        dict under the same names, or a tuple in the order given.  fields=None: siconc of `slot` alone, as one array."""
        if fields is None:
            fields = 'siconc'
        single = isinstance(fields, str) or isinstance(fields, np.ndarray)
        if single:
            fields = [fields]
        names, vals = (list(fields.keys()), list(fields.values())) if isinstance(fields, dict) else (None, list(fields))
        out = [None] * len(vals)
        host = [k for k, x in enumerate(vals) if not isinstance(x, str)]
        for k, x in enumerate(vals):
            if isinstance(x, str):
                if slot is None:
                    raise ValueError("IceTracker.sample: '%s' is served from a resident record: give its slot" % x)
                out[k] = self.ctx.sample_slot(slot, jrec, mode, x)
        for b in range(0, len(host), _lib.SAMPLE_MAX_FIELDS):              # one pass over the buoys per 8 host fields
            part = host[b:b + _lib.SAMPLE_MAX_FIELDS]
            rows = self.ctx.sample_fields(jrec, mode, [vals[k] for k in part])
            for k, r in zip(part, rows):
                out[k] = r
        if names is not None:
            return dict(zip(names, out))
        return out[0] if single else tuple(out)

    def deform_mark(self, jrec0):
        """Snapshot every buoy's fp64 position on the device as the t0 of deform() (an extra the reference does not have;
        sitrk_deform_mark); `jrec0` = the model record that will be stepped next."""
        self.ctx.deform_mark(jrec0)

    def deform(self, jrec1, cells):
        """Right after the step of `jrec1`: deformation rates of the cells (nC, 3|4) of buoy indices between the mark and now,
        computed from the device-resident positions (sitrk_deform_since_mark).  Same dict as sit.DeformCells; a cell is valid
        where all its buoys are alive and were stepped at every record of the span."""
        from .deformation import _as_dict
        out, valid, _ = self.ctx.deform_since_mark(jrec1, cells)
        return _as_dict(out, valid)

    def pairs_mark(self, jrec0, mask=None):
        """Snapshot every buoy's fp64 position and validity on the device as the t0 of pairs() (an extra the reference does not
        have; sitrk_pairs_mark); `jrec0` = the model record that will be stepped next; mask (nP): 0 = the buoy takes no part.
        Independent of deform_mark() and of the meshes."""
        cerr = 'ERROR [IceTracker.pairs_mark()]: '
        try:
            bad = int(jrec0) != jrec0
        except (TypeError, ValueError):
            bad = True
        if bad:
            raise ValueError(cerr + '`jrec0` must be an integer, got %r' % (jrec0,))
        if mask is not None and np.shape(mask) != (self.ctx.nP,):
            raise ValueError(cerr + '`mask` must be (%d,), got %s' % (self.ctx.nP, np.shape(mask)))
        self.ctx.pairs_mark(int(jrec0), mask)
        self._pairs_jrec0 = int(jrec0)

    def pairs(self, jrec1, edges_km):
        """Right after the step of `jrec1`: the pair-dispersion table between the mark and now for the classes `edges_km`, from
        the device-resident positions (sitrk_pairs_since_mark).  Same dict as sit.PairDispersion plus "T" = (jrec1 - jrec0 + 1)*rdt
        seconds; a buoy takes part where it was valid at the mark, is alive and was stepped at every record of the span.  May be
        called again and again after one mark."""
        from .dispersion import check_edges
        cerr = 'ERROR [IceTracker.pairs()]: '
        e = check_edges(edges_km, cerr)
        if self._pairs_jrec0 is None:
            raise ValueError(cerr + 'no mark: call pairs_mark() first (set_buoys() and pairs_free() cancel it)')
        try:
            bad = int(jrec1) != jrec1
        except (TypeError, ValueError):
            bad = True
        if bad or int(jrec1) < self._pairs_jrec0:
            raise ValueError(cerr + '`jrec1` must be an integer >= the mark\'s record %d, got %r' % (self._pairs_jrec0, jrec1))
        r = self.ctx.pairs_since_mark(int(jrec1), e)
        r["T"] = float(int(jrec1) - self._pairs_jrec0 + 1) * self._rdt
        return r

    def pairs_free(self):
        """Drop the snapshot of pairs_mark() (sitrk_pairs_free)"""
        self.ctx.pairs_free()
        self._pairs_jrec0 = None

    def quads(self, tris, angles=(60., 120.), ratio_min=0.5, area=(0., float("inf"))):
        """Quadrangles (nQ,4) of buoy indices and tri_quad (nT,) from the triangles `tris` (nT,3) of buoy indices, at the buoys'
        current device-resident positions; a buoy that is not alive is no vertex (an extra the reference does not have;
        sitrk_tri2quad_buoys).  Arguments and result as sit.Tri2Quad; the rows go into deform() as they are."""
        from .quadmesh import _params
        quads, tri_quad, _ = self.ctx.tri2quad_buoys(tris, **_params('ERROR [IceTracker.quads()]: ', tris, angles, ratio_min, area))
        return quads, tri_quad

    def tris(self, rmax_km):
        """Triangles (nT,3) of buoy indices: every Delaunay triangle of circumradius <= rmax_km of the buoys alive now, at their
        current device-resident positions (an extra the reference does not have; sitrk_delaunay_buoys).  Rows as
        sit.DelaunayTris; they go into quads() and deform() as they are."""
        from .delaunay import _rmax
        tris, _, _ = self.ctx.delaunay_buoys(_rmax('ERROR [IceTracker.tris()]: ', rmax_km))
        return tris

    def mesh(self, rmax_km, jrec0, slot=0, mask=None, angles=(60., 120.), ratio_min=0.5, area=(0., float("inf"))):
        """Builds the device-resident quadrangle mesh `slot` (0..7) from the buoys alive now, at their current positions: tris()
        followed by quads() with nothing leaving the device, and the t0 positions of deform taken on the spot (an extra the
        reference does not have; sitrk_mesh_build).  `jrec0` = the model record that will be stepped next; mask (nP): 0 = the
        buoy is no point of this mesh; the other arguments as sit.Tri2Quad.  Returns {"nT", "nQ", "rounds"}."""
        from .delaunay import _rmax
        from .quadmesh import _params
        cerr = 'ERROR [IceTracker.mesh()]: '
        kw = _params(cerr, np.empty((0, 3), dtype=np.int32), angles, ratio_min, area)
        if mask is not None and np.shape(mask) != (self.ctx.nP,):
            raise ValueError(cerr + '`mask` must be (nP,), got %s' % (np.shape(mask),))
        nT, nQ, rounds = self.ctx.mesh_build(slot, jrec0, _rmax(cerr, rmax_km), mask=mask, **kw)
        return {"nT": nT, "nQ": nQ, "rounds": rounds}

    def mesh_cells(self, slot=0):
        """The quadrangles (nQ,4) int32 of buoy indices of mesh `slot`, rows as quads() gives them"""
        return self.ctx.mesh_cells(slot)

    def mesh_mark(self, jrec0, slot=0):
        """Takes the t0 positions of mesh `slot` again, for the same cells, at the current positions; `jrec0` = the model record
        that will be stepped next.  A cell with a vertex that is not alive now is invalid from then on."""
        self.ctx.mesh_mark(slot, jrec0)

    def mesh_deform(self, jrec1, slot=0, full=True):
        """Right after the step of `jrec1`: deformation rates of the cells of mesh `slot` between its t0 and now.  A dict with
        div, shr, vor, area0, area1 (nQ,) fp64 (FillValue where status is 0), status (nQ,) int8 -- 0 invalid, 1 valid and still an
        acceptable quadrangle now, 2 valid but distorted beyond the mesh's own acceptance tests -- and stats, a dict under the
        names _lib.MESH_STATS: the three counts and the area-weighted sums over the status-1 cells.  full=False: the stats only,
        80 bytes from the device."""
        r = self.ctx.mesh_deform(slot, jrec1, want=("out", "status", "stats") if full else ("stats",))
        stats = dict(zip(_lib.MESH_STATS, (float(x) for x in r["stats"])))
        if not full:
            return stats
        out = r["out"]
        return {"div": out[0], "shr": out[1], "vor": out[2], "area0": out[3], "area1": out[4], "status": r["status"], "stats": stats}

    def mesh_raster(self, jrec1, grid, slot=0, at="t0", fields=True):
        """Right after the step of `jrec1`: mesh `slot` rasterised onto the grid (y0_km, x0_km, d_km, ny, nx) of sit.raster_grid
        (an extra the reference does not have; sitrk_mesh_raster).  A dict with owner (ny,nx) int32 -- per pixel the lowest-indexed
        cell its centre lies in, -1 for none -- and, with fields=True, the maps div, shr, vor, area0, area1 (ny,nx) fp64: the
        values mesh_deform() gives for that cell, FillValue where there is none.  at="t0": the cells where they were when the mesh
        was built or marked, those of status 1 and 2; at="t1": where they are now, those of status 1.  The per-cell results stay
        on the device: only the raster comes down."""
        from .raster import check_grid
        cerr = 'ERROR [IceTracker.mesh_raster()]: '
        if at not in ("t0", "t1"):
            raise ValueError(cerr + '`at` must be "t0" or "t1", got %r' % (at,))
        g = check_grid(grid, cerr)
        r = self.ctx.mesh_raster(slot, jrec1, g, at_t1=(at == "t1"), want=("owner", "fields") if fields else ("owner",))
        res = {"owner": r["owner"]}
        if fields:
            res.update(zip(("div", "shr", "vor", "area0", "area1"), r["fields"]))
        return res

    def mesh_coarse(self, jrec1, grid, nlev, fmin=0.5, slot=0, boxes=False):
        """Right after the step of `jrec1`: the status-1 cells of mesh `slot` coarse-grained on a pyramid of `nlev` levels over the
        grid (y0_km, x0_km, d_km, ny, nx) of sit.raster_grid (an extra the reference does not have; sitrk_mesh_coarse): their
        area-weighted velocity gradients summed into the pixel of their t0 centroid and up the levels of side d*2^l.  A dict with
        table (nlev, 8) under the names _lib.COARSE_COLS -- per level the boxes with a cell, the filled boxes (area >= fmin of
        the box) and over those the sums of A, A*div, A*shr, A*tot^q for q = 1, 2, 3 --, nin and nout (the cells inside and outside
        the grid) and levels: None, or with boxes=True per level a dict of (ny_l, nx_l) arrays n, A, AUx, AUy, AVx, AVy.
        sit.scaling_exponents(table, d_km) reads the exponents off it.  The per-cell results stay on the device."""
        from .coarse import check_levels, name_levels
        from .raster import check_grid
        cerr = 'ERROR [IceTracker.mesh_coarse()]: '
        g = check_levels(check_grid(grid, cerr), nlev, fmin, cerr)
        return name_levels(self.ctx.mesh_coarse(slot, jrec1, g, int(nlev), fmin=float(fmin), boxes=boxes))

    def mesh_dist(self, jrec1, what="tot", sgn=+1, edges=None, q=None, slot=0):
        """Right after the step of `jrec1`: the distribution of a deformation rate over the status-1 cells of mesh `slot` (an
        extra the reference does not have; sitrk_mesh_dist) -- the cells the stats of mesh_deform() are summed over.  what =
        "div", "shr" or "vor", taken as f, -f or |f| for sgn = +1, -1, 0, or "tot" (sgn +1).  The dict of sit.ValueDistribution:
        counts (nb + 2,) int64 for the edges (nb + 1,), None without; values (nq,) and ranks (nq,) for the quantiles q, each the
        value at rank min(m - 1, floor(q*m)) of the ascending sample, bit for bit the rate of one cell; m, nnan.  For "tot" the
        device works on t2 = div*div + shr*shr, where no second square root enters: the edges given here are those of tot and
        are squared on the host (they must be >= 0 and stay strictly ascending), values = math.sqrt of the selected t2, and the
        selected t2 themselves come back as "t2" -- what sit.percentile_threshold("tot", t2) takes.  The per-cell results stay
        on the device: only the counts, the values and two integers come down."""
        import math
        from .distribution import check_edges, check_q, square_edges
        cerr = 'ERROR [IceTracker.mesh_dist()]: '
        if what not in _lib.DIST_WHAT:
            raise ValueError(cerr + '`what` must be one of %s, got %r' % (", ".join(sorted(_lib.DIST_WHAT)), what))
        if sgn not in (1, -1, 0):
            raise ValueError(cerr + '`sgn` must be +1, -1 or 0 (the absolute value), got %r' % (sgn,))
        if what == "tot" and sgn != 1:
            raise ValueError(cerr + 'what="tot" needs sgn = +1, got %r' % (sgn,))
        e = None if edges is None else check_edges(edges, cerr)
        e_dev = e if e is None or what != "tot" else square_edges(e, cerr)
        v = None if q is None else check_q(q, cerr)
        r = self.ctx.mesh_dist(slot, jrec1, what, sgn=int(sgn), edges=e_dev, q=v)
        r["edges"] = e
        if what == "tot":
            r["t2"] = r["values"]
            r["values"] = np.array([math.sqrt(t) if t == t else t for t in r["t2"]], dtype=np.float64)
        return r

    def mesh_features(self, jrec1, grid, what="tot", thr=0., sgn=1, conn=8, min_pix=1, maxfeat=65536, slot=0, at="t0", labels=False,
                      keep=None):
        """Right after the step of `jrec1`: the features of the map of mesh `slot` on the grid (y0_km, x0_km, d_km, ny, nx) of
        sit.raster_grid (an extra the reference does not have; sitrk_mesh_features): the connected sets, for conn = 4 or 8
        neighbours, of the pixels mesh_raster() gives an owner whose rate passes the test -- what = "div", "shr" or "vor":
        sgn*rate >= thr with sgn +1 or -1; what = "tot": div^2 + shr^2 >= thr^2 (sgn +1, thr >= 0); thr in the unit of mesh_deform().
        A dict with table (rows, 12) int64 under the names _lib.FEAT_COLS, one row per feature of at least min_pix pixels in
        ascending label, at most maxfeat rows; nfeat (all such features: above maxfeat the table is truncated), ncomp, nactive; and
        labels: None, or with labels=True (ny,nx) int32, -1 or the lowest linear index of the pixel's feature.
        sit.feature_table(table, grid) turns the rows into areas, lengths and orientations.  The map stays on the device.
        keep = 0..15: the labels of the features of at least min_pix pixels also stay on the device as kept map `keep`, for
        features_advect() and features_match() (sitrk_mesh_features_keep); everything returned is what it is without it."""
        from .features import check_keep, check_label_args, check_test
        from .raster import check_grid
        cerr = 'ERROR [IceTracker.mesh_features()]: '
        if at not in ("t0", "t1"):
            raise ValueError(cerr + '`at` must be "t0" or "t1", got %r' % (at,))
        g = check_grid(grid, cerr)
        conn, min_pix, maxfeat = check_label_args(g[3], g[4], conn, min_pix, maxfeat, cerr)
        what, sgn, thr = check_test(what, sgn, thr, cerr)
        if keep is not None:
            keep = check_keep(keep, "keep", cerr)
            return self.ctx.mesh_features_keep(keep, slot, jrec1, g, what, thr, sgn=sgn, conn=conn, min_pix=min_pix,
                                               maxfeat=maxfeat, at_t1=(at == "t1"), labels=labels)
        return self.ctx.mesh_features(slot, jrec1, g, what, thr, sgn=sgn, conn=conn, min_pix=min_pix, maxfeat=maxfeat,
                                      at_t1=(at == "t1"), labels=labels)

    def features_advect(self, jrec1, grid, keep_from, keep_to, slot=0):
        """Right after the step of `jrec1`: the kept map keep_from carried by the cells of mesh `slot` from where they were at the
        mesh's t0 to where they are now, into the kept map keep_to (an extra the reference does not have;
        sitrk_mesh_features_advect): a cell takes the lowest label among the pixels it owns on the t0 draw and gives it to the
        pixels it owns on the t1 draw.  A dict with ncells, the cells that carry a label, and ncarried, the pixels that received
        one.  Nothing else leaves the device."""
        from .features import check_keep
        from .raster import check_grid
        cerr = 'ERROR [IceTracker.features_advect()]: '
        g = check_grid(grid, cerr)
        keep_from, keep_to = check_keep(keep_from, "keep_from", cerr), check_keep(keep_to, "keep_to", cerr)
        ncells, ncarried = self.ctx.mesh_features_advect(keep_from, keep_to, slot, jrec1, g)
        return {"ncells": ncells, "ncarried": ncarried}

    def features_match(self, keepA, keepB, reach=0, dj=0, di=0, maxpair=1 << 20):
        """The features of the kept maps keepA and keepB that meet (an extra the reference does not have; sitrk_features_match):
        {"pairs": (rows, 3) int64 rows (a, b, count) in ascending (a, b), "npair", "nhit"} as sit.MatchLabels gives them."""
        from .features import check_keep, check_match_args
        cerr = 'ERROR [IceTracker.features_match()]: '
        reach, dj, di, maxpair = check_match_args(reach, dj, di, maxpair, cerr)
        keepA, keepB = check_keep(keepA, "keepA", cerr), check_keep(keepB, "keepB", cerr)
        return self.ctx.features_match(keepA, keepB, reach=reach, dj=dj, di=di, maxpair=maxpair)

    def features_skeleton(self, keep, max_sub=4096, maxfeat=65536, maxnode=1 << 20, skel=False):
        """The skeleton of the features of the kept map `keep` (an extra the reference does not have; sitrk_keep_skeleton): the
        dict of sit.SkeletonRaster without "labels" -- table, nodes, nfeat, nnode, nskel, nsub, converged and skel, None unless
        skel=True.  The kept map stays on the device and as it was; with a map kept by mesh_features(keep=...) the rows of the
        table follow those of its feature table.  sit.skeleton_table(table, grid) turns the rows into lengths."""
        from .features import check_keep, check_skeleton_args
        cerr = 'ERROR [IceTracker.features_skeleton()]: '
        keep = check_keep(keep, "keep", cerr)
        max_sub, maxfeat, maxnode = check_skeleton_args(max_sub, maxfeat, maxnode, cerr)
        return self.ctx.keep_skeleton(keep, max_sub=max_sub, maxfeat=maxfeat, maxnode=maxnode, skel=skel)

    def mesh_free(self, slot=0):
        self.ctx.mesh_free(slot)

    def dist2coast(self, rmax_km=None, return_seg=False):
        """Distance [km, polar-stereographic plane] of every buoy, alive or not, to the coastline of the tracker's own mesh, from
        the device-resident positions, in the caller's order (an extra the reference does not have; sitrk_coast_dist_buoys).
        The index is built from the tracker's grid on first use.  `rmax_km`: buoys further away report +inf."""
        if not getattr(self, "_coast_built", False):
            self.ctx.coast_build()
            self._coast_built = True
        dist, seg = self.ctx.coast_dist_buoys(rmax_km, want_seg=return_seg)
        return (dist, seg) if return_seg else dist

    def state(self):
        s = self.ctx.fetch()
        s["vJIt"] = s.pop("jiT").astype(np.int64)
        s["VRTCS"] = vertices_of(s["vJIt"])
        s["iAlive"] = s.pop("alive")
        return s

    def alive_count(self):
        return self.ctx.count_alive()

    def close(self):
        self.ctx.close()
