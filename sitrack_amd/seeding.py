"""Idealised seeding on the model grid -- the surface of the reference's seeding generators (`nemoSeed`, `SidfexSeeding`,
`ReadFromSidfexDatFile`; sitrack/tracking.py:331-442) and of the coarsening it applies (`SubSampCloud`, util.py:345-370) as
used by tools/generate_idealized_seeding.py.

`nemoSeed` runs on the GPU (`sitrk_nemo_seed`, sitrack_amd/csrc/sitrk_seed.h): the decision which points of the sub-sampled
mesh carry a seed, their compaction in the reference's output order and their projection to the polar-stereographic plane
happen in three kernels; only the mesh arrays go in and the seed list comes out.  There is no host version."""
import numpy as np


def _same_shape(a, ref):
    return np.shape(a) == np.shape(ref)


def nemoSeed(pmskT, platT, plonT, pIC, khss=1, fmsk_rstrct=[], platF=[], plonF=[], ctx=None, return_yx=False):
    """Seeds on every `khss`-th T-point (reference tracking.py:365-442, same arguments): where the land-sea mask --
    times the optional restriction mask `fmsk_rstrct` -- is 1, north of 55N, under an ice concentration of at least 0.9.
    When F-point coordinates of the mesh's shape are passed, F-points whose four sub-sampled T-neighbours all carry a
    seed are appended.  Returns the (n,2) [lat,lon] array in the reference's order; with `return_yx` also their (n,2)
    [y,x] km in the polar-stereographic plane (what the seeding tool computes next, util.py:394-410)."""
    from .tracking import default_context
    restricted = _same_shape(fmsk_rstrct, pmskT)
    with_f = _same_shape(platF, pmskT) and _same_shape(plonF, pmskT)
    if not (_same_shape(platT, pmskT) and _same_shape(plonT, pmskT) and _same_shape(pIC, pmskT)):
        raise ValueError('ERROR [nemoSeed()]: mask, coordinates and ice concentration must share one shape')
    latlon, yx, _, _ = (ctx or default_context()).nemo_seed(
        pmskT, platT, plonT, pIC, khss=khss, rmask=fmsk_rstrct if restricted else None,
        latF=platF if with_f else None, lonF=plonF if with_f else None)
    return (latlon, yx) if return_yx else latlon


def ReadFromSidfexDatFile(filepath='./sidfexloc.dat'):
    """Text file `id lon lat` per line (reference sitrack/tracking.py:344-361)."""
    import os
    if not os.path.exists(filepath):
        raise FileNotFoundError("'%s' file is missing." % filepath)
    return np.atleast_2d(np.genfromtxt(filepath))


def SidfexSeeding(filepath='./sidfexloc.dat'):
    """Reference sitrack/tracking.py:331-341 -> (n,2) [lat,lon] and the buoy IDs (int)."""
    dat = ReadFromSidfexDatFile(filepath)
    return dat[:, [2, 1]], dat[:, 0].astype(int)


def SubSampCloud(rd_km, pCoor, *, ctx=None):
    """Reference sitrack/util.py:345-370, same positional parameters and return tuple (Nb, zCoor, idxleft): the points of
    `pCoor` (n,2) -- the seeds' polar-stereographic [y,x] km -- kept by the greedy sparsification of
    gudhi.subsampling.sparsify_point_set(pCoor, min_squared_dist=rd_km**2), in input order.  Runs on the GPU
    (`sitrk_subsample_cloud`, sitrack_amd/csrc/sitrk_subsample.hip).  Raises ValueError where the reference prints and
    exits.  One deliberate deviation: the reference recovers `idxleft` with np.where(pCoor == zCoor[i]), which matches a
    row where EITHER coordinate is equal and can return an earlier, dropped point; here `idxleft` is the true index of
    each kept point, so zCoor == pCoor[idxleft] row by row."""
    from .tracking import default_context
    cerr = 'ERROR [SubSampCloud()]: '
    if not rd_km > 0. or rd_km > 2000:
        raise ValueError(cerr + 'silly value for `rd_km`: %r' % (rd_km,))
    pCoor = np.asarray(pCoor, dtype=np.float64)
    if pCoor.ndim != 2 or pCoor.shape[1] != 2:
        raise ValueError(cerr + 'second dimension of `pCoor` must be 2 !')
    keep, _ = (ctx or default_context()).subsample_cloud(pCoor, rd_km)
    idxleft = np.flatnonzero(keep)
    return len(idxleft), pCoor[idxleft, :].copy(), idxleft
