"""Sub-stepped advection (--rdt / --nsub, sitrk_set_substeps): the contract on the CPU side.

The contract (include/sitrk.h): with nsub = n, a model record advances every buoy its gate admits by n reference steps of
dt = rdt / n with that record's fields -- the reference loop body run n times per record.  Golden set G12
(tests/golden/gen_golden_g12.py) holds that loop restated with the reference's own functions; the CPU oracle replays it
as oracle.Tracker(rdt=rdt/n) stepped n times per record.  The GPU side is tests/test_gpu_substep.py."""
import ctypes
import os

import numpy as np
import pytest

from sitrack_amd import _lib
from sitrack_amd import driver as drv

FILL = -9999.0


def oracle_replay(grid, yx0, jiT0, u, v, sic, rec_first, rec_last, kstrt, Nt, rdt, nsub, strat):
    """The contract through the oracle: n calls of step(jrec) at rdt/n per record.  Returns per-record outputs (the last
    sub-step of the record whose mask is 1), host cells and alive flags after every record, kill records, final positions."""
    from oracle import oracle as orc
    nP = yx0.shape[0]
    K = u.shape[0]
    trk = orc.Tracker(grid, yx0, jiT0, rec_first=rec_first, rec_last=rec_last, rdt=rdt / nsub, uv_strategy=strat)
    pos = np.zeros((Nt + 1, nP, 2)) + FILL
    msk = np.zeros((Nt + 1, nP), dtype="i1")
    jit = np.zeros((Nt + 1, nP, 2), dtype=np.int32)
    alv = np.zeros((Nt + 1, nP), dtype="i1")
    kill = np.full(nP, -1, dtype=np.int32)
    k0 = np.asarray(rec_first) - kstrt
    pos[k0, np.arange(nP)] = yx0
    msk[k0, np.arange(nP)] = 1
    jit[0], alv[0] = trk.jiT, trk.alive
    for jt in range(Nt):
        jrec = jt + kstrt
        uu, vv, ss = (np.asarray(a[jrec % K], dtype=np.float64) for a in (u, v, sic))
        for _ in range(nsub):
            was = trk.alive.copy()
            pn, mn = trk.step(jrec, uu, vv, ss)
            pos[jt + 1, mn == 1] = pn[mn == 1]
            msk[jt + 1, mn == 1] = 1
            kill[(was == 1) & (trk.alive == 0)] = jrec
        jit[jt + 1], alv[jt + 1] = trk.jiT, trk.alive
    return dict(pos=pos, msk=msk, jiT=jit, alive=alv, kill_rec=kill, final=trk.pos.copy(), ncross=trk.ncross)


def g12_cases(g):
    """(tag, rdt, nsub, Nt, strat, rec_first, rec_last) of every case stored in G12"""
    for rdt, nsub, Nt in g["cases"]:
        for win in ("all", "win"):
            tag = "n%d_%s" % (int(nsub), win)
            for strat in (1, 0):
                yield ("%s_s%d" % (tag, strat), float(rdt), int(nsub), int(Nt), strat,
                       g["rec_first_" + tag].astype(np.int64), g["rec_last_" + tag].astype(np.int64))


def g12_inputs(golden):
    from conftest import g6b_case
    g = golden("g12_substep.npz")
    g6b = golden("g6b_traj_fast.npz")
    grid, u, v, sic = g6b_case(g6b)
    sel = g["sel"]
    return g, grid, u, v, sic, g6b["yx0"][sel].copy(), g6b["jiT0"][sel].astype(np.int64)


def test_g12_is_small_and_complete(golden):
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "g12_substep.npz")) < 512 * 1024
    g = golden("g12_substep.npz")
    tags = [c[0] for c in g12_cases(g)]
    assert len(tags) == 8 and {int(n) for _, n, _ in g["cases"]} == {6, 24}
    for t in tags:                                      # every case kills buoys and keeps some alive: both paths are exercised
        a = g["alive_" + t][-1]
        assert 0 < a.sum() < a.size


@pytest.mark.parametrize("case", range(8))
def test_oracle_replay_reproduces_g12(golden, case):
    g, grid, u, v, sic, yx0, jiT0 = g12_inputs(golden)
    tag, rdt, nsub, Nt, strat, rf, rl = list(g12_cases(g))[case]
    kstrt = int(g["kstrt"])
    r = oracle_replay(grid, yx0, jiT0, u, v, sic, rf, rl, kstrt, Nt, rdt, nsub, strat)
    assert np.array_equal(r["msk"], g["msk_" + tag])
    assert np.array_equal(r["pos"].view(np.uint64), g["pos_" + tag].view(np.uint64))          # bit for bit
    assert np.array_equal(r["jiT"], g["jiT_" + tag]) and np.array_equal(r["alive"], g["alive_" + tag])
    assert np.array_equal(r["kill_rec"], g["kill_rec_" + tag])


def test_nsub_1_replay_is_the_plain_oracle(golden):
    """the replay with n = 1 is the oracle's own record loop (the sub-step contract reduces to today's)"""
    from oracle import oracle as orc
    g, grid, u, v, sic, yx0, jiT0 = g12_inputs(golden)
    r = oracle_replay(grid, yx0, jiT0, u, v, sic, np.full(len(yx0), 2), np.full(len(yx0), 9), 2, 8, 3600., 1, 1)
    t = orc.Tracker(grid, yx0, jiT0, rdt=3600.)
    for jt in range(8):
        t.step(jt + 2, u[(jt + 2) % 6].astype(np.float64), v[(jt + 2) % 6].astype(np.float64), sic[(jt + 2) % 6].astype(np.float64))
    assert np.array_equal(r["final"], t.pos) and np.array_equal(r["jiT"][-1], t.jiT)


def test_parse_args_rdt_and_nsub():
    base = ["-i", "a.nc", "-m", "m.nc", "-s", "s.nc"]
    a = drv.parse_args(base)
    assert a.rdt == 3600. and a.nsub == 1                    # the reference's constant, one step per record
    assert drv.parse_args(base + ["--rdt", "21600"]).rdt == 21600.
    assert drv.parse_args(base + ["--rdt", "auto"]).rdt == "auto"
    assert drv.parse_args(base + ["--nsub", "6"]).nsub == 6
    a = drv.parse_args(base + ["--rdt", "auto", "--nsub", "24"])
    assert a.rdt == "auto" and a.nsub == 24
    for bad in (["--nsub", "0"], ["--nsub", "1025"], ["--rdt", "-5"], ["--rdt", "daily"]):
        with pytest.raises(SystemExit):
            drv.parse_args(base + bad)


@pytest.mark.parametrize("step", [3600, 21600, 86400])
def test_axis_spacing_of_uniform_axes(step):
    tc = (850608000 + step // 2 + step * np.arange(10)).astype('i4')
    assert drv.axis_spacing(tc) == float(step)
    assert drv.run_rdt("auto", tc) == float(step)
    said = []
    assert drv.run_rdt(float(step), tc, said.append) == float(step) and said == []
    assert drv.run_rdt(3600. if step != 3600 else 7200., tc, said.append) in (3600., 7200.) and len(said) == 1   # one warning


def test_axis_spacing_refuses_non_uniform_or_single_record_axes():
    tc = (850608000 + 1800 + 3600 * np.arange(10)).astype('i4')
    tc[5] += 60
    with pytest.raises(ValueError, match="not uniform"):
        drv.axis_spacing(tc)
    with pytest.raises(ValueError, match="at least 2"):
        drv.axis_spacing(tc[:1])
    with pytest.raises(ValueError):
        drv.run_rdt("auto", tc)
    assert drv.run_rdt(3600., tc, lambda *a: None) == 3600.       # an explicit period on such an axis: kept, no check


def test_record_windows_on_a_6_hourly_axis():
    """record_windows(..., rdt=21600) == the reference's own loop form (:289-312) with rdt/2 = 10800"""
    base, step = 850608000, 21600
    vt = (base + step // 2 + step * np.arange(20)).astype('i4')
    kstrt, kstop = 0, 19
    iTmA, iTmB = vt[kstrt], vt[kstop]
    rng = np.random.default_rng(12)
    n = 3000
    zT = np.stack([rng.integers(vt[0] - step, vt[-1] + step // 2, n), rng.integers(vt[0] + step // 2, vt[-1] + 2 * step, n)])
    zT[0, ::9] = vt[rng.integers(0, 20, len(zT[0, ::9]))] + rng.choice([-10800, 10800, 0, 10799, 10801], len(zT[0, ::9]))
    zT[1, ::7] = vt[rng.integers(0, 20, len(zT[1, ::7]))] + rng.choice([-10800, 10800, 0, -10799, -10801], len(zT[1, ::7]))
    zT[0][zT[0] == iTmA + 10800] += 1
    fast = drv.record_windows(zT, vt, kstrt, kstop, iTmA, iTmB, n, rdt=21600.)
    late = np.where(zT[0] >= iTmA + 10800)[0]; early = np.where(zT[1] < iTmB - 10800)[0]
    slow = drv._record_windows_loop(zT, vt, np.zeros(n, dtype=int) + kstrt, np.zeros(n, dtype=int) + kstop, late, early, 10800)
    assert np.array_equal(fast[0], slow[0]) and np.array_equal(fast[1], slow[1])
    assert len(np.unique(fast[0])) > 5 and len(np.unique(fast[1])) > 5
    # the positional form (no rdt) is unchanged: hourly half-width
    hourly = drv.record_windows(zT, vt, kstrt, kstop, iTmA, iTmB, n)
    late1 = np.where(zT[0] >= iTmA + 1800)[0]; early1 = np.where(zT[1] < iTmB - 1800)[0]
    slow1 = drv._record_windows_loop(zT, vt, np.zeros(n, dtype=int) + kstrt, np.zeros(n, dtype=int) + kstop, late1, early1, 1800)
    assert np.array_equal(hourly[0], slow1[0]) and np.array_equal(hourly[1], slow1[1])


def test_set_substeps_is_exported_and_bound():
    _lib.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(so, "sitrk_set_substeps")
    assert _lib._SIGNATURES["sitrk_set_substeps"][1][1] is ctypes.c_int
    assert hasattr(_lib.Context, "set_substeps")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "sitrk.h")).read()
    assert "int sitrk_set_substeps(sitrk_t *h, int nsub);" in hdr


def test_band_and_box_arithmetic_with_substeps():
    """D(age) = (age+1)*nsub - 1 cells: what a record `age` records after the evaluation can reach (D = age for nsub = 1)"""
    assert [_lib.reach(a, 1) for a in range(4)] == [0, 1, 2, 3]
    assert [_lib.reach(a, 6) for a in range(3)] == [5, 11, 17]

    class Mesh:
        Nj, Ni, nsub = 100, 64, 3
    box_of = _lib.Context.box_of
    assert box_of(Mesh, 40, 50, 20, 30, 0, align=1) == (36, 55, 16, 35)           # D = 2
    assert box_of(Mesh, 40, 50, 20, 30, 1, align=1) == (33, 58, 13, 38)           # D = 5
    Mesh.nsub = 1
    assert box_of(Mesh, 40, 50, 20, 30, 1, align=1) == (37, 54, 17, 34)           # today's rule
