"""Golden set G11: the reference's util.CancelTooClose (sitrack/util.py:520-565) on clouds built here.

Run from the repository root where the reference is available: `python tests/golden/gen_golden_g11.py`.  The reference is
imported through refload.load_reference(); only its numeric outputs are written, with the inputs that produced them:
the positions at krec (float64), the (Nrec, n) mask (bit-packed) and the case parameters.  The other records of plat/plon
are not read by the reference and are rebuilt by series() below.  Every case is free of ulp-close decisions: no valid
buoy's dmin lies within 1e-9 relative of rdkm, and no buoy's nearest distance (when below rdkm and not 0) has a rival within
1e-9 relative other than exact copies of the same position -- the device's sin/cos/asin may differ from numpy's in the last
ulp, but the same inputs give the same value on either side."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g11_cancel_too_close.npz")
FILL = -9999.


def series(la, lo, pmsk, krec):
    """(plat, plon) of shape pmsk.shape: the positions at krec, drifting 0.01 degree a record elsewhere, fill where masked."""
    nrec, n = np.shape(pmsk)
    t = (np.arange(nrec) - krec)[:, None]
    plat = np.clip(la[None, :] + 0.01 * t, -90., 90.)
    plon = np.mod(lo[None, :] + 0.01 * t, 360.)
    off = (np.asarray(pmsk) == 0) & (t != 0)
    plat[off] = FILL
    plon[off] = FILL
    plat[krec], plon[krec] = la, lo
    return plat, plon


def haversine(plat, plon, xlat, xlon):
    to_rad = 3.141592653589793 / 180.
    a1 = np.sin(0.5 * ((xlat - plat) * to_rad))
    a2 = np.sin(0.5 * ((xlon - plon) * to_rad))
    a3 = np.cos(xlat * to_rad) * np.cos(plat * to_rad)
    return 2. * 6360. * np.arcsin(np.sqrt(a1 * a1 + a3 * a2 * a2))


def ulp_safe(la, lo, rd, tol=1e-9):
    for j in range(len(la)):
        d = haversine(la[j], lo[j], la, lo)
        d[j] = 9999.
        m = d.min()
        if abs(m - rd) <= tol * rd:
            return False
        if 0. < m < rd:
            k = np.flatnonzero(d <= m * (1 + tol))       # rivals: only copies of the one position (the same inputs, the same value)
            if np.any(d[k] != m) or np.any(la[k] != la[k[0]]) or np.any(lo[k] != lo[k[0]]):
                return False
    return True


def clustered(rng, n, rd, lat_lo=72., lat_hi=88., lon_lo=0., lon_hi=360., spread=(0.4, 3.0)):
    nclust = max(1, n // 30)
    lat0 = rng.uniform(lat_lo, lat_hi, nclust)
    lon0 = rng.uniform(lon_lo, lon_hi, nclust)
    c = rng.integers(0, nclust, n)
    s = rd / 111.2 * rng.uniform(*spread, nclust)[c]
    la = np.clip(lat0[c] + rng.normal(0, 1, n) * s, -89.99, 89.99)
    lo = np.mod(lon0[c] + rng.normal(0, 1, n) * s / np.cos(np.radians(la)), 360.)
    return la, lo


def masks(rng, nrec, n, krec, p_on=0.8):
    m = (rng.random((nrec, n)) < p_on).astype(np.int8)
    m[krec] = 1                                    # the reference needs every buoy valid at krec (else IndexError)
    return m


def build_cases():
    rng = np.random.default_rng(20261016)
    cases = []                                     # (name, krec, rdkm, NbPass, la, lo, pmsk)

    def attempt(name, make, tries=50):
        for _ in range(tries):
            out = make()
            if ulp_safe(out[3], out[4], out[1]):
                cases.append((name,) + out)
                return
        raise RuntimeError("no ulp-safe draw for " + name)

    # clustered clouds, several scales and passes
    for i, (n, rd, nrec, nbpass) in enumerate([(600, 10., 6, 1), (900, 25., 5, 2), (400, 3., 8, 3), (700, 120., 4, 2)]):
        def mk(n=n, rd=rd, nrec=nrec, nbpass=nbpass):
            la, lo = clustered(rng, n, rd)
            krec = int(rng.integers(0, nrec))
            return krec, rd, nbpass, la, lo, masks(rng, nrec, n, krec)
        attempt("cluster_%d" % i, mk)

    # exact duplicates: a fifth of the buoys repeat another one's position
    def mk_dup():
        n, rd, nrec = 500, 8., 5
        la, lo = clustered(rng, n, rd)
        src = rng.integers(0, n, n // 5)
        dst = rng.choice(n, n // 5, replace=False)
        la[dst], lo[dst] = la[src], lo[src]
        krec = 2
        return krec, rd, 2, la, lo, masks(rng, nrec, n, krec)
    attempt("duplicates", mk_dup)

    # near the pole
    def mk_pole():
        n, rd, nrec = 400, 15., 4
        la = 90. - np.abs(rng.normal(0, 0.3, n))
        lo = rng.uniform(0., 360., n)
        krec = 1
        return krec, rd, 2, la, lo, masks(rng, nrec, n, krec)
    attempt("pole", mk_pole)

    # across longitude 0/360
    def mk_lon0():
        n, rd, nrec = 500, 12., 5
        la = rng.uniform(70., 80., n)
        lo = np.mod(rng.normal(0., 1.5, n), 360.)
        krec = 3
        return krec, rd, 1, la, lo, masks(rng, nrec, n, krec)
    attempt("lon0_360", mk_lon0)

    # equal counts everywhere: the neighbour always goes
    def mk_eq():
        n, rd, nrec = 600, 10., 4
        la, lo = clustered(rng, n, rd)
        return 2, rd, 2, la, lo, np.ones((nrec, n), dtype=np.int8)
    attempt("equal_counts", mk_eq)

    # the count drop after a cancel: late krec, sparse early records, dense later ones
    for i in range(2):
        def mk_drop():
            n, rd, nrec = 600, 20., 8
            la, lo = clustered(rng, n, rd, spread=(0.3, 1.5))
            krec = 4
            m = np.zeros((nrec, n), dtype=np.int8)
            m[:krec] = rng.random((krec, n)) < 0.5
            m[krec:] = rng.random((nrec - krec, n)) < 0.9
            m[krec] = 1
            return krec, rd, 3, la, lo, m
        attempt("count_drop_%d" % i, mk_drop)

    # krec at the first and the last record, a large rd
    def mk_first():
        n, rd, nrec = 300, 300., 3
        la, lo = clustered(rng, n, 30.)
        return 0, rd, 2, la, lo, masks(rng, nrec, n, 0)
    attempt("cluster_krec0_rd300", mk_first)

    def mk_last():
        n, rd, nrec = 300, 0.8, 4
        la, lo = clustered(rng, n, rd)
        return nrec - 1, rd, 4, la, lo, masks(rng, nrec, n, nrec - 1)
    attempt("cluster_krec_last_rd0.8", mk_last)
    return cases


def main():
    sys.path.insert(0, HERE)
    from refload import load_reference
    util, _, _ = load_reference()
    cases = build_cases()
    z = {"names": np.array([c[0] for c in cases]), "rdkm": np.array([c[2] for c in cases]),
         "krec_nrec_nbpass": np.array([[c[1], c[6].shape[0], c[3]] for c in cases], dtype=np.int32), "nbn": []}
    for i, (name, krec, rd, nbpass, la, lo, pmsk) in enumerate(cases):
        assert ulp_safe(la, lo, rd), name
        plat, plon = series(la, lo, pmsk, krec)
        with contextlib.redirect_stdout(io.StringIO()):
            nbn, idx = util.CancelTooClose(krec, rd, plat, plon, pmsk, NbPass=nbpass)
        z["nbn"].append(int(nbn))
        z["la_%d" % i], z["lo_%d" % i] = la, lo
        z["pmsk_%d" % i] = np.packbits(pmsk.ravel())
        z["idx_keep_%d" % i] = np.asarray(idx, dtype=np.int32)
        print("%-24s n=%4d krec=%d/%d rd=%6.1f NbPass=%d -> kept %d" % (name, len(la), krec, pmsk.shape[0], rd, nbpass, nbn))
    z["nbn"] = np.array(z["nbn"], dtype=np.int64)
    np.savez_compressed(OUT, **z)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
