"""Restatements of the bounded-Delaunay contract of include/sitrk.h (sitrk_delaunay) on the host, checked against each other.
They are the references of tests/test_gpu_delaunay.py.

`delaunay_literal`  the contract word for word over ALL points, Python integers only: every pair (p,q), one pass for the apex,
                    one pass for conditions 4 and 5.  O(n^3): small clouds.
`delaunay_ref`      the same conditions, Python integers wherever a sign is in doubt, fp64 (np.float64) for tests 2 and 3, made
                    affordable by three prunings that cannot change the result (each argued where it is made): only points in
                    the reach box of p are looked at; a pair (p,q) is dropped when two of p's nearest neighbours on either side
                    of p->q show that no empty circle passes through p and q; the apex pass looks at the candidates whose
                    circle parameter is within 1e-9 of the smallest.  Signs of determinants are taken in fp64 where the value
                    exceeds 2^-40 of the sum of its terms' magnitudes (the rounding error is below 2^-49 of it), else exactly.
`delaunay_fast`     scipy's Delaunay on the integer coordinates, canonical rows, every interior edge asserted STRICTLY locally
                    Delaunay with exact integers (then the triangulation is the only one and no tie exists), tests 2 and 3.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNIT = 1048576.0


# ------------------------------------------------------------------------------------------------ the contract's pieces
def quantise(yx, mask=None):
    """(Y, X as lists of Python ints, vertex (nP,) int8): 1 vertex, 0 masked or not finite, 2 duplicate of a lower index"""
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    n = len(yx)
    ok = np.isfinite(yx).all(axis=1)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    if (np.abs(yx[ok]) > 2.0 ** 30).any():
        raise ValueError("coordinate beyond 2^30 km at index %d" % np.flatnonzero(ok & (np.abs(yx) > 2.0 ** 30).any(axis=1))[0])
    q = np.zeros((n, 2), dtype=np.int64)
    q[ok] = np.rint(yx[ok] * UNIT).astype(np.int64)
    vertex = np.zeros(n, dtype=np.int8)
    seen = {}
    for i in np.flatnonzero(ok):
        k = (int(q[i, 0]), int(q[i, 1]))
        if k in seen:
            vertex[i] = 2
        else:
            seen[k] = i
            vertex[i] = 1
    return q[:, 0].tolist(), q[:, 1].tolist(), vertex


def orient(Y, X, a, b, c):
    return (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])


def incircle(Y, X, a, b, c, d):
    r = []
    for k in (a, b, c):
        dx, dy = X[k] - X[d], Y[k] - Y[d]
        r.append((dx, dy, dx * dx + dy * dy))
    (a0, a1, a2), (b0, b1, b2), (c0, c1, c2) = r
    return a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0)


def r4_of(rmax_km):
    ru = np.float64(rmax_km) * np.float64(UNIT)
    return np.float64(4.0) * (ru * ru)


def size_and_reach(Y, X, p, q, r, R4):
    """conditions 2 and 3"""
    la = np.float64((X[q] - X[p]) ** 2 + (Y[q] - Y[p]) ** 2)
    lb = np.float64((X[r] - X[p]) ** 2 + (Y[r] - Y[p]) ** 2)
    lc = np.float64((X[r] - X[q]) ** 2 + (Y[r] - Y[q]) ** 2)
    A2 = np.float64(orient(Y, X, p, q, r))
    return bool(la <= R4 and lb <= R4 and lc <= R4 and (la * lb) * lc <= (R4 * A2) * A2)


def check_rmax(rmax_km):
    if not (np.isfinite(rmax_km) and 0. < rmax_km <= 500.):
        raise ValueError("rmax_km must be finite and in (0, 500]")


def as_rows(rows):
    return np.array(sorted(rows), dtype=np.int32).reshape(-1, 3)


def delaunay_literal(yx, rmax_km, mask=None):
    check_rmax(rmax_km)
    Y, X, vertex = quantise(yx, mask)
    R4 = r4_of(rmax_km)
    V = [int(i) for i in np.flatnonzero(vertex == 1)]
    rows = []
    for p in V:
        for q in V:
            if q <= p:
                continue
            r = None
            for s in V:
                if s <= p or orient(Y, X, p, q, s) <= 0:
                    continue
                if r is None:
                    r = s
                    continue
                ic = incircle(Y, X, p, q, r, s)
                if ic > 0 or (ic == 0 and orient(Y, X, q, r, s) < 0):
                    r = s
            if r is None or not size_and_reach(Y, X, p, q, r, R4):
                continue
            ok = True
            for s in V:
                if s in (p, q, r):
                    continue
                ic = incircle(Y, X, p, q, r, s)
                if ic > 0 or (ic == 0 and not (p < s and orient(Y, X, q, r, s) > 0)):
                    ok = False
                    break
            if ok:
                rows.append((p, q, r))
    return as_rows(rows), vertex


# ------------------------------------------------------------------------------------------------ signs of determinants, many at once
def incircle_signs(ux, uy, vx, vy, wx, wy):
    """sign of incircle(p,q,r,s) for int64 arrays (or scalars) of the differences u = q-p, v = r-p, w = s-p, all below 2^31:
    -(wx*Bx - wy*By + |w|^2*A), A = ux*vy - uy*vx, Bx = uy*|v|^2 - |u|^2*vy, By = ux*|v|^2 - |u|^2*vx.  fp64 where the value
    stands clear of its rounding error, Python integers elsewhere."""
    ux, uy, vx, vy, wx, wy = np.broadcast_arrays(*[np.asarray(a, dtype=np.int64) for a in (ux, uy, vx, vy, wx, wy)])
    f = [a.astype(np.float64) for a in (ux, uy, vx, vy, wx, wy)]                  # exact: below 2^53
    u2, v2, w2 = f[0] * f[0] + f[1] * f[1], f[2] * f[2] + f[3] * f[3], f[4] * f[4] + f[5] * f[5]
    t = [f[4] * (f[1] * v2), f[4] * (u2 * f[3]), f[5] * (f[0] * v2), f[5] * (u2 * f[2]), w2 * (f[0] * f[3]), w2 * (f[1] * f[2])]
    e = (t[0] - t[1]) - (t[2] - t[3]) + (t[4] - t[5])
    mag = sum(np.abs(x) for x in t)
    sign = -np.sign(e).astype(np.int8)
    for k in np.flatnonzero(np.abs(e) <= 2.0 ** -40 * mag):                       # every term carries < 8 roundings of 2^-53
        a, b, c, d, g, h = (int(x.flat[k]) for x in (ux, uy, vx, vy, wx, wy))
        U2, V2, W2 = a * a + b * b, c * c + d * d, g * g + h * h
        x = g * (b * V2 - U2 * d) - h * (a * V2 - U2 * c) + W2 * (a * d - b * c)
        sign.flat[k] = -1 if x > 0 else (1 if x < 0 else 0)
    return sign


def delaunay_ref(yx, rmax_km, mask=None, witnesses=16):
    from scipy.spatial import cKDTree
    check_rmax(rmax_km)
    Y, X, vertex = quantise(yx, mask)
    R4 = r4_of(rmax_km)
    D = int(np.floor(2.0 * float(rmax_km) * UNIT)) + 2          # la <= R4 in fp64 leaves |dy|, |dx| < D: the reach box
    V = np.flatnonzero(vertex == 1)
    if len(V) < 3:
        return np.zeros((0, 3), dtype=np.int32), vertex
    Yv, Xv = np.array([Y[i] for i in V], dtype=np.int64), np.array([X[i] for i in V], dtype=np.int64)
    assert max(abs(Yv).max(), abs(Xv).max()) < 2 ** 52
    tree = cKDTree(np.stack([Yv, Xv], axis=1).astype(np.float64))                # integers below 2^53: exact
    rows = []
    for kp, p in enumerate(V):
        # pruning 1: a triangle that passes test 2 has its circle, and so every point in or on it, within the reach box of p
        c = np.array(tree.query_ball_point([float(Yv[kp]), float(Xv[kp])], r=float(D), p=np.inf), dtype=np.int64)
        c = c[c != kp]
        if len(c) < 2:
            continue
        wy, wx, idx = Yv[c] - Yv[kp], Xv[c] - Xv[kp], V[c]
        w2 = wx * wx + wy * wy
        near = np.argsort(w2, kind="stable")[:witnesses]
        qs = np.flatnonzero((idx > p) & (w2.astype(np.float64) <= R4))
        if len(qs) == 0:
            continue
        # The circle through p, q and s has its centre at u/2 + t*(-uy,ux), t = num / (2 cross) with cross = orient(p,q,s) and
        # num = |w|^2 - w.u, both exact in int64; s left of p->q lies inside the circles of larger t, s on the right inside those
        # of smaller t.  pruning 2: an empty circle through p and q has t <= t(s) for every s on the left and t >= t(s) for
        # every s on the right, so a pair whose nearest neighbours already leave no such t has no triangle.  t carries three
        # roundings of 2^-53; the margin is 1e-9.
        with np.errstate(divide="ignore", invalid="ignore"):
            cn = wx[qs][:, None] * wy[near][None, :] - wy[qs][:, None] * wx[near][None, :]
            nn = w2[near][None, :] - (wx[near][None, :] * wx[qs][:, None] + wy[near][None, :] * wy[qs][:, None])
            tn = nn.astype(np.float64) / (2.0 * cn.astype(np.float64))
            lo = np.where(cn < 0, tn, -np.inf).max(axis=1)
            hi = np.where(cn > 0, tn, np.inf).min(axis=1)
            dead = lo - hi > 1e-9 * (np.abs(lo) + np.abs(hi))
        for kq in qs[~dead]:
            ux, uy = int(wx[kq]), int(wy[kq])
            cross = ux * wy - uy * wx
            num = w2 - (wx * ux + wy * uy)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = num.astype(np.float64) / (2.0 * cross.astype(np.float64))
            left = np.flatnonzero((cross > 0) & (idx > p))
            if len(left) == 0:
                continue
            # pruning 3: the apex has the smallest t; whatever the pass starts from, it ends at the apex if a valid one exists
            tl = t[left]
            first = left[tl <= tl.min() + 1e-9 * abs(tl.min())]
            r = None
            for s in first:
                if r is None:
                    r = s
                    continue
                ic = incircle(Y, X, p, idx[kq], idx[r], idx[s])
                if ic > 0 or (ic == 0 and orient(Y, X, idx[kq], idx[r], idx[s]) < 0):
                    r = s
            q_, r_ = int(idx[kq]), int(idx[r])
            if not size_and_reach(Y, X, int(p), q_, r_, R4):
                continue
            others = np.ones(len(c), dtype=bool)
            others[[kq, r]] = False
            sg = incircle_signs(ux, uy, int(wx[r]), int(wy[r]), wx[others], wy[others])
            if (sg > 0).any():
                continue
            ok = True
            for s in idx[others][sg == 0]:
                ok = ok and p < s and orient(Y, X, q_, r_, int(s)) > 0
            if ok:
                rows.append((int(p), q_, r_))
    return as_rows(rows), vertex


def delaunay_fast(yx, rmax_km, mask=None):
    from scipy.spatial import Delaunay
    check_rmax(rmax_km)
    Y, X, vertex = quantise(yx, mask)
    R4 = r4_of(rmax_km)
    V = np.flatnonzero(vertex == 1)
    Yv, Xv = np.array(Y, dtype=np.int64)[V], np.array(X, dtype=np.int64)[V]
    assert Yv.max() - Yv.min() < 2 ** 30 and Xv.max() - Xv.min() < 2 ** 30
    tri = Delaunay(np.stack([Xv - Xv.min(), Yv - Yv.min()], axis=1).astype(np.float64))
    T = tri.simplices.astype(np.int64)
    assert len(tri.coplanar) == 0 and len(np.unique(T)) == len(V), "scipy left points out"
    d = lambda a, b: (Xv[T[:, b]] - Xv[T[:, a]], Yv[T[:, b]] - Yv[T[:, a]])
    (ux, uy), (vx, vy) = d(0, 1), d(0, 2)
    A = ux * vy - uy * vx
    assert (A != 0).all()
    T[A < 0] = T[A < 0][:, [0, 2, 1]]
    # the guard: across every interior edge the opposite vertex lies strictly outside the circle
    nb = tri.neighbors
    t, e = np.nonzero(nb >= 0)
    opp = tri.simplices[nb[t, e]][np.arange(len(t)), np.argmax(tri.neighbors[nb[t, e]] == t[:, None], axis=1)]
    a, b, c = T[t, 0], T[t, 1], T[t, 2]
    sg = incircle_signs(Xv[b] - Xv[a], Yv[b] - Yv[a], Xv[c] - Xv[a], Yv[c] - Yv[a], Xv[opp] - Xv[a], Yv[opp] - Yv[a])
    assert (sg < 0).all(), "%d edge(s) are not strictly locally Delaunay: this input has ties, use delaunay_ref" % (sg >= 0).sum()
    G = V[T]
    k = np.argmin(G, axis=1)
    G = np.stack([G[np.arange(len(G)), (k + j) % 3] for j in range(3)], axis=1)
    Ya, Xa = np.array(Y, dtype=np.int64), np.array(X, dtype=np.int64)
    sq = lambda m, n: ((Xa[G[:, n]] - Xa[G[:, m]]) ** 2 + (Ya[G[:, n]] - Ya[G[:, m]]) ** 2).astype(np.float64)
    la, lb, lc = sq(0, 1), sq(0, 2), sq(1, 2)
    A2 = ((Xa[G[:, 1]] - Xa[G[:, 0]]) * (Ya[G[:, 2]] - Ya[G[:, 0]]) - (Ya[G[:, 1]] - Ya[G[:, 0]]) * (Xa[G[:, 2]] - Xa[G[:, 0]])).astype(np.float64)
    assert (A2 > 0).all()
    keep = (la <= R4) & (lb <= R4) & (lc <= R4) & ((la * lb) * lc <= (R4 * A2) * A2)
    G = G[keep]
    return G[np.lexsort((G[:, 1], G[:, 0]))].astype(np.int32), vertex


# ------------------------------------------------------------------------------------------------ inputs shared with the GPU tests
def lattice_case(a, b, spacing_km=4.0, seed=1, nmask=0):
    """an exact a x b lattice (spacing a multiple of 2^-20 km) with shuffled indices: (yx, mask)"""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(a, dtype=np.float64), np.arange(b, dtype=np.float64), indexing="ij")
    yx = spacing_km * np.stack([j.ravel(), i.ravel()], axis=1)[rng.permutation(a * b)]
    mask = np.ones(a * b, dtype=np.int8)
    mask[rng.choice(a * b, nmask, replace=False)] = 0
    return yx, mask


def cocircular_points(k=1, shift=(0, 0)):
    """the integer points with a^2 + b^2 = 32045 k^2 that come from 32045 = 5*13*17*29 (179^2 + 2^2 and its kin), scaled by k
    and shifted: as integer units (ints, (n,2) [Y,X])"""
    n = 32045
    pts = sorted({(sa * a, sb * b) for a in range(180) for b in [int(round((n - a * a) ** 0.5))] if a * a + b * b == n
                  for sa in (1, -1) for sb in (1, -1)})
    return np.array([(k * y + shift[0], k * x + shift[1]) for y, x in pts], dtype=np.int64)


def hull_orient_sum(Y, X, idx):
    """twice the area of the convex hull of the points idx (exact), by scipy's hull on exact floats"""
    from scipy.spatial import ConvexHull
    h = ConvexHull(np.array([[X[i], Y[i]] for i in idx], dtype=np.float64))
    v = [idx[k] for k in h.vertices]                                               # counter-clockwise
    return sum(orient(Y, X, v[0], v[k], v[k + 1]) for k in range(1, len(v) - 1))


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("seed,n,rmax", [(0, 60, 500.), (1, 70, 12.), (2, 50, 3.)])
def test_pruned_form_equals_the_literal_one(seed, n, rmax):
    rng = np.random.default_rng(seed)
    yx = rng.uniform(0., 40., (n, 2))
    yx[5] = yx[3]                                                                  # a duplicate
    yx[7, 0] = np.nan
    mask = np.ones(n, dtype=np.int8)
    mask[11] = 0
    want, v0 = delaunay_literal(yx, rmax, mask)
    got, v1 = delaunay_ref(yx, rmax, mask)
    assert np.array_equal(v0, v1) and v0[5] == 2 and v0[7] == 0 and v0[11] == 0
    assert np.array_equal(got, want) and len(want) > 10
    assert not np.isin(want, [5, 7, 11]).any()


def test_literal_and_pruned_on_ties():
    yx, mask = lattice_case(5, 4, nmask=2)
    for rmax in (0.75 * 4.0, 500.):
        want, _ = delaunay_literal(yx, rmax, mask)
        got, _ = delaunay_ref(yx, rmax, mask)
        assert np.array_equal(got, want) and len(want) >= 16
    P = cocircular_points()[::3] / UNIT
    want, _ = delaunay_literal(P, 500.)
    got, _ = delaunay_ref(P, 500.)
    assert np.array_equal(got, want) and len(want) == len(P) - 2


@pytest.mark.parametrize("seed", [3, 4])
def test_the_two_restatements_agree_on_random_clouds(seed):
    rng = np.random.default_rng(seed)
    yx = rng.uniform(0., 60., (300, 2))
    mask = (rng.uniform(size=300) > 0.05).astype(np.int8)
    for rmax in (3., 8., 500.):
        a, va = delaunay_ref(yx, rmax, mask)
        b, vb = delaunay_fast(yx, rmax, mask)
        assert np.array_equal(va, vb) and np.array_equal(a, b), rmax
        print("rmax %g km: %d triangles" % (rmax, len(a)))
    full, _ = delaunay_ref(yx, 500., mask)
    few, _ = delaunay_ref(yx, 3., mask)
    nV = int(mask.sum())                                                          # all but the hull's flattest slivers
    assert 2 * nV - 2 - len_hull(yx, mask) - 40 < len(full) <= 2 * nV - 2 - len_hull(yx, mask) and 0 < len(few) < len(full)


def len_hull(yx, mask):
    from scipy.spatial import ConvexHull
    return len(ConvexHull(yx[mask != 0]).vertices)


def test_fast_form_refuses_ties():
    yx, mask = lattice_case(6, 5)
    with pytest.raises(AssertionError, match="strictly locally Delaunay|left points out"):
        delaunay_fast(yx, 500., mask)


def test_exact_lattice_with_shuffled_indices():
    a, b = 6, 5
    yx, mask = lattice_case(a, b)
    tris, vertex = delaunay_ref(yx, 500.)
    assert (vertex == 1).all() and len(tris) == 2 * (a - 1) * (b - 1)
    Y, X, _ = quantise(yx)
    assert all(orient(Y, X, *t) > 0 for t in tris.tolist()) and (tris[:, 0] < tris[:, 1:].min(axis=1)).all()
    assert sum(orient(Y, X, *t) for t in tris.tolist()) == hull_orient_sum(Y, X, list(range(a * b)))
    edges = [(t[k], t[(k + 1) % 3]) for t in tris.tolist() for k in range(3)]
    assert len(set(edges)) == len(edges)                                           # no directed edge twice: nothing overlaps
    # the size test: the circumradius of a lattice triangle is 0.7071 spacings
    assert len(delaunay_ref(yx, 0.75 * 4.0)[0]) == len(tris) and len(delaunay_ref(yx, 0.6 * 4.0)[0]) == 0


def test_cocircular_points_give_the_fan_from_the_lowest_index():
    P = cocircular_points(k=3, shift=(10 ** 6, -2 * 10 ** 6))
    assert len(P) >= 12 and len({(y - 10 ** 6) ** 2 + (x + 2 * 10 ** 6) ** 2 for y, x in P.tolist()}) == 1
    rng = np.random.default_rng(5)
    P = P[rng.permutation(len(P))]
    tris, vertex = delaunay_ref(P / UNIT, 500.)
    n = len(P)
    assert (vertex == 1).all() and len(tris) == n - 2 and (tris[:, 0] == 0).all()
    # counter-clockwise from point 0: q -> r are consecutive points of the polygon
    ang = np.arctan2((P[:, 0] - 10 ** 6).astype(float), (P[:, 1] + 2 * 10 ** 6).astype(float))
    order = np.argsort((ang - ang[0]) % (2 * np.pi))
    assert order[0] == 0
    fan = sorted((0, int(order[k]), int(order[k + 1])) for k in range(1, n - 1))
    assert tris.tolist() == [list(t) for t in fan]


def test_bad_arguments():
    yx = np.zeros((4, 2))
    for bad in (np.nan, 0., -1., 501., np.inf):
        with pytest.raises(ValueError):
            delaunay_ref(yx, bad)
    with pytest.raises(ValueError, match="2\\^30 km at index 2"):
        delaunay_ref(np.array([[0., 0.], [1., 1.], [2.0 ** 31, 0.], [-2.0 ** 31, 0.]]), 5.)


# ------------------------------------------------------------------------------------------------ the interfaces
NAMES = ("sitrk_delaunay", "sitrk_delaunay_buoys", "sitrk_delaunay_kernel_ms")


def test_the_feature_is_declared_and_offered(monkeypatch):
    """fails without the feature: the public function, the header's three entry points, the tool's `-t gpu`"""
    import sitrack_amd as sit
    from sitrack_amd import _lib
    assert callable(sit.DelaunayTris) and callable(sit.IceTracker.tris)
    txt = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    for name in NAMES:
        assert "int %s(sitrk_t *h" % name in txt and name in _lib._SIGNATURES
    for name in ("delaunay", "delaunay_buoys", "delaunay_kernel_ms"):
        assert callable(getattr(_lib.Context, name))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import generate_quad_mesh as tool
    src = open(tool.__file__).read()
    assert "'--rmax'" in src and "`gpu`" in src
    with pytest.raises(SystemExit, match="--rmax"):                                # -t gpu without --rmax, before any file is opened
        tool.main(["-i", "nowhere.nc", "-t", "gpu", "-o", "out.npy"])

    def no_device(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(_lib, "Context", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    import sitrack_amd.tracking as trk
    monkeypatch.setattr(trk, "default_context", no_device)
    for bad in (np.nan, 0., -2., 501., "far"):
        with pytest.raises(ValueError, match="`rmax_km`"):
            sit.DelaunayTris(yx_ok(), bad)
    with pytest.raises(ValueError, match="`yx`"):
        sit.DelaunayTris(np.zeros((6, 3)), 5.)
    with pytest.raises(ValueError, match="`mask`"):
        sit.DelaunayTris(yx_ok(), 5., mask=np.ones(5))


def yx_ok():
    return np.zeros((6, 2))
