"""Device-resident quadrangle meshes, host side: the numpy restatement `mesh_deform_ref` of sitrk_mesh_deform's contract
(include/sitrk.h) -- the rates of tests/test_deform.py's `deform_ref`, the acceptance arithmetic of
tests/test_tri2quad.py's `candidates` applied to the stored order at t1, the ten sums by math.fsum -- with its self-checks; the
binding; `plan_batches(..., cuts=)` and the `--deform` parser of the command line.  The reference of tests/test_gpu_mesh.py."""
import math
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import driver as drv
from sitrack_amd._lib import MESH_NSTATS, MESH_STATS
from test_deform import DAY3, FILL, LIN_DIV, deform_ref, linear_move
from test_tri2quad import _shoelace, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = ("sitrk_mesh_build", "sitrk_mesh_cells", "sitrk_mesh_mark", "sitrk_mesh_deform", "sitrk_mesh_free", "sitrk_mesh_kernel_ms")


def acceptable(P, cos_lo=0.5, cos_hi=-0.5, ratio_min=0.5, area_min=0., area_max=INF):
    """The acceptance of DESIGN.md 3.12 on quadrangles P (n, 4, 2) [y,x] in the order given, never made canonical again: the
    shoelace sum relative to vertex 0 is > 0 and finite, tests 1-4 hold, the score is finite.  The statements of `candidates`."""
    c_lo2, c_hi2 = np.float64(cos_lo) * abs(np.float64(cos_lo)), np.float64(cos_hi) * abs(np.float64(cos_hi))
    ratio2 = np.float64(ratio_min) * np.float64(ratio_min)
    with np.errstate(all="ignore"):
        A2 = _shoelace(P)
        ok = (A2 > 0.0) & np.isfinite(A2)
        nx = np.roll(np.arange(4), -1)
        ex, ey = P[:, nx, 1] - P[:, :, 1], P[:, nx, 0] - P[:, :, 0]
        L = ex * ex + ey * ey
        score = np.zeros(len(P))
        for c in range(4):
            m = (c + 3) % 4
            cr = ex[:, m] * ey[:, c] - ey[:, m] * ex[:, c]
            ok &= cr > 0.0
            d = (-ex[:, m]) * ex[:, c] + (-ey[:, m]) * ey[:, c]
            n = L[:, m] * L[:, c]
            sq = d * np.abs(d)
            ok &= (sq <= c_lo2 * n) & (sq >= c_hi2 * n)
            qc = (d * d) / n
            score = qc if c == 0 else np.where(qc > score, qc, score)
        ok &= L.min(axis=1) >= ratio2 * L.max(axis=1)
        area = 0.5 * A2
        ok &= (np.float64(area_min) <= area) & (area <= np.float64(area_max))
        ok &= score < INF
    return ok


def stat_terms(out, status):
    """(7, n1) terms of the seven sums over the status-1 cells, one rounded operation per symbol: area0, area1, area0*div,
    area0*shr, a*tot, (a*tot)*tot, ((a*tot)*tot)*tot with tot = sqrt(div*div + shr*shr)"""
    s1 = np.asarray(status) == 1
    div, shr, a0, a1 = out[0][s1], out[1][s1], out[3][s1], out[4][s1]
    tot = np.sqrt(div * div + shr * shr)
    m1 = a0 * tot
    m2 = m1 * tot
    return np.stack([a0, a1, a0 * div, a0 * shr, m1, m2, m2 * tot])


def mesh_deform_ref(yx0, yx1, quads, T, mask0=None, mask1=None, params=None):
    """sitrk_mesh_deform restated: (out (5, nQ), status (nQ,) int8, stats (10,)) of the quadrangles `quads` (nQ, 4) between the
    positions yx0 and yx1, T seconds apart; params = the library's five pairing parameters as keywords (default: its defaults)"""
    quads = np.asarray(quads).reshape(-1, 4)
    out, valid = deform_ref(yx0, yx1, quads, T, mask0, mask1)
    acc = acceptable(np.asarray(yx1, dtype=np.float64)[quads], **(params or {}))
    status = np.where(valid, np.where(acc, 1, 2), 0).astype(np.int8)
    terms = stat_terms(out, status)
    stats = np.array([(status == k).sum() for k in range(3)] + [math.fsum(t) for t in terms], dtype=np.float64)
    assert stats.shape == (MESH_NSTATS,) and MESH_STATS[:3] == ("n0", "n1", "n2")
    return out, status, stats


# ------------------------------------------------------------------------------------------------ the restatement's self-checks
def exact_lattice(ny=12, nx=14, dkm=8.0):
    j, i = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return np.stack([-1500. + dkm * j.ravel(), 2000. + dkm * i.ravel()], axis=1)


def ccw_quads(ny, nx):
    """the lattice's quadrangles, counter-clockwise with x to the right and y up, started at their smallest index"""
    j, i = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    a = (j * nx + i).ravel()
    return np.stack([a, a + 1, a + nx + 1, a + nx], axis=1).astype(np.int32)


def test_restatement_on_an_exact_lattice_under_a_linear_field():
    yx0 = exact_lattice()
    yx1 = linear_move(yx0, DAY3)
    quads = ccw_quads(12, 14)
    assert (_shoelace(yx0[quads]) > 0).all()
    out, status, stats = mesh_deform_ref(yx0, yx1, quads, DAY3)
    assert (status == 1).all() and stats[:3].tolist() == [0., len(quads), 0.]
    mean_div = stats[5] / stats[3]
    print("area-weighted divergence %.17g, imposed %.17g" % (mean_div, LIN_DIV))
    assert abs(mean_div - LIN_DIV) <= 1e-12 * abs(LIN_DIV)
    assert abs(stats[3] - 64. * len(quads)) <= 1e-9 * stats[3]
    tot = np.sqrt(out[0] * out[0] + out[1] * out[1])
    assert np.isclose(stats[7], (out[3] * tot).sum(), rtol=1e-13) and np.isclose(stats[9], (out[3] * tot ** 3).sum(), rtol=1e-13)


def test_restatement_flags_a_cell_turned_inside_out_and_a_masked_vertex():
    yx0 = exact_lattice()
    yx1 = linear_move(yx0, DAY3)
    quads = ccw_quads(12, 14)
    c = 40
    v1, v3 = quads[c, 1], quads[c, 3]
    yx1x = yx1.copy()
    yx1x[[v1, v3]] = yx1[[v3, v1]]                                   # two vertices exchanged at t1: the cell is clockwise now
    out, status, stats = mesh_deform_ref(yx0, yx1x, quads, DAY3)
    assert status[c] == 2 and (out[:, c] != FILL).all()
    touched = np.isin(quads, [v1, v3]).any(axis=1)
    assert (status[touched] == 2).all() and (status[~touched] == 1).all() and stats[2] == touched.sum()
    # a masked vertex, at t0 or at t1: status 0 and FILL, and its cells leave every sum
    for kw in ({"mask0": None}, {"mask1": None}):
        m = np.ones(len(yx0), dtype=np.int8)
        m[v1] = 0
        kw = {k: m for k in kw}
        out, status, stats = mesh_deform_ref(yx0, yx1, quads, DAY3, **kw)
        hit = (quads == v1).any(axis=1)
        assert hit.sum() == 4 and (status[hit] == 0).all() and (out[:, hit] == FILL).all() and (status[~hit] == 1).all()
        assert stats[:3].tolist() == [4., len(quads) - 4., 0.] and np.isclose(stats[3], 64. * (len(quads) - 4))
    # the mesh's own parameters decide: a band of areas that excludes the 64 km^2 cells
    _, status, _ = mesh_deform_ref(yx0, yx1, quads, DAY3, params=params(area=(0., 50.)))
    assert (status == 2).all()
    # no cells
    out, status, stats = mesh_deform_ref(yx0, yx1, np.zeros((0, 4), dtype=np.int32), DAY3)
    assert out.shape == (5, 0) and status.shape == (0,) and (stats == 0.).all()


# ------------------------------------------------------------------------------------------------ the binding
def test_symbols_are_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert "int %s(sitrk_t *h" % name in txt and name in _lib._SIGNATURES and hasattr(L, name)
    assert "#define SITRK_MESH_MAX 8" in txt and "#define SITRK_MESH_NSTATS 10" in txt
    assert _lib.MESH_MAX == 8 and _lib.MESH_NSTATS == 10 and len(_lib.MESH_STATS) == 10 and len(set(_lib.MESH_STATS)) == 10
    for name in ("mesh_build", "mesh_cells", "mesh_mark", "mesh_deform", "mesh_free", "mesh_kernel_ms"):
        assert callable(getattr(_lib.Context, name))
    for name in ("mesh", "mesh_cells", "mesh_mark", "mesh_deform"):
        assert callable(getattr(sit.IceTracker, name))


# ------------------------------------------------------------------------------------------------ the command line's planning
def old_plan(Nt, kstrt, K, lFull, stride=1, ends=(), firsts=None):
    """plan_batches as it was before `cuts`"""
    firsts = set(firsts) if firsts is not None else set()
    batches, jt = [], 0
    while jt < Nt:
        m = 1
        while m < K // 2 and jt + m < Nt and not drv.output_due(jt + m - 1 + kstrt, kstrt, Nt, lFull, stride, ends) \
                and (jt + m + kstrt) not in firsts:
            m += 1
        batches.append((jt, m))
        jt += m
    return batches


# the argument sets of the planning tests (tests/test_sample.py, tests/test_tlerp.py) and the command line's defaults
PLANS = [(30, 3, 32, False, 1, {20, 32}), (30, 3, 32, False, 1, {20, 32}, {3, 7, 12}), (30, 3, 32, True, 4), (30, 3, 32, True, 4, (), None),
         (5, 0, 8, True, 1), (5, 2, 2, True), (23, 0, 10, False, 1, {6, 22}), (14, 0, 32, False, 1, {13}), (100, 7, 64, False, 1, {106})]


def test_plan_batches_without_cuts_is_the_old_plan():
    for args in PLANS:
        want = old_plan(*args)
        assert drv.plan_batches(*args) == want and drv.plan_batches(*args, cuts=None) == want and drv.plan_batches(*args, cuts=()) == want


def test_plan_batches_ends_a_batch_after_every_cut():
    for args in PLANS:
        Nt, kstrt = args[0], args[1]
        for nwin in (0, 1, 5, 7, Nt, Nt + 3):
            win = drv.deform_windows(Nt, kstrt, nwin)
            assert win[0][0] == kstrt and win[-1][1] == kstrt + Nt - 1 and all(b[0] == a[1] + 1 for a, b in zip(win, win[1:]))
            assert all(w[1] - w[0] + 1 == (nwin or Nt) for w in win[:-1]) and 1 <= win[-1][1] - win[-1][0] + 1 <= (nwin or Nt)
            cuts = {w[1] for w in win}
            b = drv.plan_batches(*args, cuts=cuts)
            assert [jt for jt, _ in b] == list(np.cumsum([0] + [m for _, m in b])[:-1]) and sum(m for _, m in b) == Nt
            lasts = {jt + m - 1 + kstrt for jt, m in b}
            assert cuts <= lasts                                        # every listed record ends a batch
            for jt, m in b:                                             # ... and no batch crosses one
                assert not any(jt + kstrt <= c < jt + m - 1 + kstrt for c in cuts)
            lFull, stride, ends = args[3], (args[4] if len(args) > 4 else 1), (args[5] if len(args) > 5 else ())
            due = {j for j in range(kstrt, kstrt + Nt) if drv.output_due(j, kstrt, Nt, lFull, stride, ends)}
            assert due <= lasts and max(m for _, m in b) <= max(1, args[2] // 2)    # what cut the old plan still does
    assert drv.plan_batches(12, 3, 32, False, cuts={7, 12}) == [(0, 5), (5, 5), (10, 2)]
    assert drv.deform_windows(12, 3, 5) == [(3, 7), (8, 12), (13, 14)] and drv.deform_windows(12, 3, 0) == [(3, 14)]


def test_deform_flag_parser():
    base = ["-i", "a", "-m", "b", "-s", "c"]
    a = drv.parse_args(base)
    assert a.deform == [] and a.deform_window == 0
    a = drv.parse_args(base + ["--deform", "10"])
    assert a.deform == [(10., 0.)]
    a = drv.parse_args(base + ["--deform", "3.5,7@2.5, 500@1e-3", "--deform-window", "24"])
    assert a.deform == [(3.5, 0.), (7., 2.5), (500., 1e-3)] and a.deform_window == 24
    assert len(drv.parse_args(base + ["--deform", ",".join(["5"] * 8)]).deform) == 8
    for bad in (",".join(["5"] * 9), "", "5,", "abc", "5@", "@5", "5@2@1", "5@0", "5@-1", "5@nan", "5@inf", "0", "-3", "500.5", "nan",
                "inf", "5;6"):
        with pytest.raises(SystemExit):
            drv.parse_args(base + ["--deform", bad])
    for bad in ("-1", "2.5", "x"):
        with pytest.raises(SystemExit):
            drv.parse_args(base + ["--deform", "5", "--deform-window", bad])


def test_more_than_one_rank_is_refused_before_anything_is_computed(monkeypatch):
    class TwoRanks:
        multi, world, root, rank = True, 2, True, 0

        def close(self):
            pass

    def untouched(*a, **k):
        raise AssertionError("the run went on")
    monkeypatch.setattr(drv, "Comm", TwoRanks)
    monkeypatch.setattr(drv.ncio, "SeedFileTimeInfo", untouched)
    monkeypatch.setattr(_lib, "Context", untouched)
    with pytest.raises(ValueError, match="--deform.*one rank"):
        drv.main(["-i", "a", "-m", "b", "-s", "sitrack_seeding_nemoTsi3_19961215_00_HSS5.nc", "--deform", "5"])
