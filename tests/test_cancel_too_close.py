"""Overlap cleaning of a tracked cloud (CancelTooClose, sitrk_cancel_too_close), CPU side: the test-side restatement of the
contract, pinned against the reference's outputs (golden set G11), the closure property the GPU's scan relies on, and the
argument checks that come before any device work.  The GPU results are held against these in test_gpu_cancel_too_close.py.

Contract (include/sitrk.h): d(j,k) = the reference Haversine(la[j], lo[j], la[k], lo[k]); nn[j] = first index of the
minimum over the valid k != j; the reference's scan over j in index order drops, of j and nn[j], the one with the smaller
count (nall if alive, nbef once dropped; the neighbour on equal counts)."""
import importlib.util
import os

import numpy as np
import pytest

import sitrack_amd as sit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def haversine(plat, plon, xlat, xlon):
    """The reference Haversine (util.py:85-103) in its operation order."""
    to_rad = 3.141592653589793 / 180.
    R = 6360.
    a1 = np.sin(0.5 * ((xlat - plat) * to_rad))
    a2 = np.sin(0.5 * ((xlon - plon) * to_rad))
    a3 = np.cos(xlat * to_rad) * np.cos(plat * to_rad)
    return 2. * R * np.arcsin(np.sqrt(a1 * a1 + a3 * a2 * a2))


def nearest(la, lo, valid=None):
    """(nn, dmin) of every buoy over the valid others: the reference's masked vdist (self = 9999) and first minimum;
    invalid buoys get (-1, inf)."""
    la = np.asarray(la, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64)
    n = len(la)
    valid = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    nn = np.full(n, -1, dtype=np.int64)
    dmin = np.full(n, np.inf)
    for j in np.flatnonzero(valid):
        d = haversine(la[j], lo[j], la, lo)
        d[~valid] = np.inf
        d[j] = 9999.
        k = int(np.argmin(d))
        nn[j], dmin[j] = k, d[k]
    return nn, dmin


def scan(nn, dmin, valid, nall, nbef, rd):
    """The reference's sequential scan (util.py:536-556) on the nearest neighbours: the alive mask at krec."""
    alive = np.asarray(valid, dtype=bool).copy()
    for j in range(len(alive)):
        if alive[j] and dmin[j] < rd:
            k = nn[j]
            cj = nall[j]
            ck = nall[k] if alive[k] else nbef[k]
            alive[j if cj < ck else k] = False
    return alive


def restate(krec, rdkm, plat, plon, pmsk):
    """CancelTooClose restated: (nBn, idx_keep int64)."""
    pmsk = np.asarray(pmsk) != 0
    valid = pmsk[krec]
    nall = pmsk.sum(axis=0)
    nbef = pmsk[:krec].sum(axis=0)
    nn, dmin = nearest(plat[krec], plon[krec], valid)
    alive = scan(nn, dmin, valid, nall, nbef, rdkm)
    idx = np.flatnonzero(alive).astype(np.int64)
    return len(idx), idx


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_golden_g11", os.path.join(GOLDEN, "gen_golden_g11.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def g11_cases():
    """Every G11 case as (name, krec, rdkm, NbPass, plat, plon, pmsk, nBn, idx_keep) of the reference run."""
    gen = load_generator()
    with np.load(os.path.join(GOLDEN, "g11_cancel_too_close.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    out = []
    for c, name in enumerate(g["names"]):
        krec, nrec, nbpass = (int(v) for v in g["krec_nrec_nbpass"][c])
        la, lo = g["la_%d" % c], g["lo_%d" % c]
        n = len(la)
        pmsk = np.unpackbits(g["pmsk_%d" % c], count=nrec * n).reshape(nrec, n).astype(np.int8)
        plat, plon = gen.series(la, lo, pmsk, krec)
        out.append((str(name), krec, float(g["rdkm"][c]), nbpass, plat, plon, pmsk, int(g["nbn"][c]),
                    g["idx_keep_%d" % c].astype(np.int64)))
    return out


def test_restatement_equals_g11():
    cases = g11_cases()
    assert len(cases) >= 10
    for name, krec, rdkm, _, plat, plon, pmsk, nbn, idx in cases:
        rn, ridx = restate(krec, rdkm, plat, plon, pmsk)
        assert rn == nbn and np.array_equal(ridx, idx), name


def test_g11_covers_its_cases():
    cases = {c[0]: c for c in g11_cases()}
    for key in ("cluster", "duplicates", "pole", "lon0", "equal_counts", "count_drop"):
        assert any(key in k for k in cases), key
    assert len({c[3] for c in cases.values()}) >= 3                       # several NbPass values
    # the count drop after a cancel decides at least one case: nall for every buoy gives another result there
    hits = 0
    for name, krec, rdkm, _, plat, plon, pmsk, nbn, idx in cases.values():
        m = pmsk != 0
        nn, dmin = nearest(plat[krec], plon[krec], m[krec])
        alt = scan(nn, dmin, m[krec], m.sum(0), m.sum(0), rdkm)
        hits += not np.array_equal(np.flatnonzero(alt), idx)
    assert hits >= 1
    # exact duplicates are decided at distance 0
    name, krec, rdkm, _, plat, plon, pmsk, _, _ = next(c for k, c in cases.items() if "duplicates" in k)
    _, dmin = nearest(plat[krec], plon[krec])
    assert np.sum(dmin == 0.0) >= 10


def random_cloud(rng, n, rd, nclust=None):
    """Clustered cloud in the Arctic, a fraction of the buoys close to another."""
    nclust = nclust or max(1, n // 40)
    lat0 = rng.uniform(70., 89.5, nclust)
    lon0 = rng.uniform(0., 360., nclust)
    c = rng.integers(0, nclust, n)
    s = rd / 111.2 * rng.uniform(0.5, 4.0, nclust)[c]
    la = np.clip(lat0[c] + rng.normal(0, 1, n) * s, -89.9, 89.9)
    lo = np.mod(lon0[c] + rng.normal(0, 1, n) * s / np.cos(np.radians(la)), 360.)
    return la, lo


@pytest.mark.parametrize("seed", range(12))
def test_closure_property(seed):
    """dmin[nn[j]] <= dmin[j]: the close set {dmin < rd} is closed under nn, so a buoy outside it is never dropped and the
    scan need only visit the close set."""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(50, 700))
    rd = float(rng.uniform(0.5, 300.))
    la, lo = random_cloud(rng, n, rd)
    if seed % 3 == 0:
        la[: n // 10], lo[: n // 10] = la[n // 10: 2 * (n // 10)], lo[n // 10: 2 * (n // 10)]      # duplicates
    valid = rng.random(n) > 0.1
    nn, dmin = nearest(la, lo, valid)
    close = np.flatnonzero(valid & (dmin < rd))
    assert np.all(dmin[nn[close]] <= dmin[close])
    assert np.all(dmin[nn[close]] < rd)
    # the haversine as computed is symmetric
    j, k = close, nn[close]
    assert np.array_equal(haversine(la[j], lo[j], la[k], lo[k]), haversine(la[k], lo[k], la[j], lo[j]))
    # and a buoy outside the close set survives the scan
    nall = rng.integers(1, 6, n)
    alive = scan(nn, dmin, valid, nall, np.minimum(nall, rng.integers(0, 3, n)), rd)
    far = valid & ~(dmin < rd)
    assert np.all(alive[far])


class _NoDevice:
    """A context whose every use fails the test: the checks must come first."""

    def __getattr__(self, name):
        raise AssertionError("device touched before the argument checks: %s" % name)


def _ok():
    plat = np.full((3, 4), 75.)
    plon = np.arange(12, dtype=float).reshape(3, 4)
    return plat, plon, np.ones((3, 4), dtype=np.int8)


@pytest.mark.parametrize("kw,match", [
    (dict(rdkm=0.), "rdkm"), (dict(rdkm=-1.), "rdkm"), (dict(rdkm=np.inf), "rdkm"), (dict(rdkm=np.nan), "rdkm"),
    (dict(rdkm=10000.), "rdkm"), (dict(rdkm="x"), "rdkm"),
    (dict(NbPass=0), "NbPass"), (dict(NbPass=-2), "NbPass"), (dict(NbPass=1.5), "NbPass"),
    (dict(krec=3), "krec"), (dict(krec=-4), "krec"), (dict(krec=1.0), "krec"),
])
def test_argument_checks(kw, match):
    plat, plon, pmsk = _ok()
    args = dict(krec=1, rdkm=10., NbPass=2)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        sit.CancelTooClose(args["krec"], args["rdkm"], plat, plon, pmsk, NbPass=args["NbPass"], ctx=_NoDevice())


def test_argument_checks_arrays():
    plat, plon, pmsk = _ok()
    with pytest.raises(ValueError, match="share one shape"):
        sit.CancelTooClose(1, 10., plat[:, :3], plon, pmsk, ctx=_NoDevice())
    with pytest.raises(ValueError, match="2-D"):
        sit.CancelTooClose(1, 10., plat[1], plon[1], pmsk[1], ctx=_NoDevice())
    plat[1, 2] = np.nan
    with pytest.raises(ValueError, match="index 2"):
        sit.CancelTooClose(1, 10., plat, plon, pmsk, ctx=_NoDevice())
    pmsk[1, 2] = 0                                 # an invalid buoy may hold anything
    with pytest.raises(AssertionError, match="device touched"):
        sit.CancelTooClose(1, 10., plat, plon, pmsk, ctx=_NoDevice())


def test_record_counts():
    from sitrack_amd.overlap import record_counts
    rng = np.random.default_rng(3)
    m = (rng.random((7, 50)) > 0.3).astype(np.int8)
    for k in range(7):
        nall, nbef = record_counts(m, k)
        assert np.array_equal(nall, m.sum(0)) and np.array_equal(nbef, m[:k].sum(0))
