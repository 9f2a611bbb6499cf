"""Sub-stepped advection with the fields interpolated in time (--tinterp, sitrk_run_tlerp): the contract on the CPU side.

The contract (include/sitrk.h): sub-step s of a record is one reference step of dt = rdt / n with the velocity fields
    F = f_cur + w * (f_partner - f_cur),   tau = (2s+1)/(2n),  theta = tau - phase,  w = |theta|,
the partner being the record before (theta < 0) or behind (theta > 0) -- three rounded fp64 operations on the records' values --
and with the record's own siconc.  tlerp_weights / tlerp_fields restate that in numpy, oracle_replay_tlerp feeds the CPU oracle
with the blended fields.  The GPU side is tests/test_gpu_tlerp.py."""
import ctypes
import os

import numpy as np
import pytest

from sitrack_amd import _lib
from sitrack_amd import driver as drv
from sitrack_amd.tracking import tinterp_phase
from test_substep import g12_inputs, oracle_replay

FILL = -9999.0


def tlerp_weights(nsub, phase):
    """[(side, w)] of the nsub sub-steps of a record: side -1 / +1 = the partner is the record before / behind, 0 = none"""
    out = []
    for s in range(nsub):
        tau = np.float64(2 * s + 1) / np.float64(2 * nsub)
        theta = tau - np.float64(phase)
        out.append((-1, -theta) if theta < 0 else ((1, theta) if theta > 0 else (0, np.float64(0.))))
    return out


def tlerp_fields(f_cur, f_partner, w):
    """F = f_cur + w * (f_partner - f_cur) in fp64, one rounded operation per symbol; f_partner None: f_cur itself"""
    fc = np.asarray(f_cur, dtype=np.float64)
    if f_partner is None:
        return fc
    d = np.asarray(f_partner, dtype=np.float64) - fc
    return fc + np.float64(w) * d


def oracle_replay_tlerp(grid, yx0, jiT0, u, v, sic, rec_first, rec_last, kstrt, Nt, rdt, nsub, strat, phase, span=None):
    """oracle_replay (tests/test_substep.py) with the blended fields: n calls of step(jrec, u_s, v_s, sic[jrec]) at rdt/n per
    record.  u, v, sic hold the records' values (record jrec = index jrec % K); span = (first, last) model record that may
    serve as a partner (default: the records stepped, kstrt .. kstrt + Nt - 1); None in place of span[k]: no partner at all."""
    from oracle import oracle as orc
    nP = yx0.shape[0]
    K = u.shape[0]
    lo, hi = (kstrt, kstrt + Nt - 1) if span is None else span
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
    wts = tlerp_weights(nsub, phase)
    for jt in range(Nt):
        jrec = jt + kstrt
        ss = np.asarray(sic[jrec % K], dtype=np.float64)
        for side, w in wts:
            jp = jrec + side
            there = side != 0 and lo is not None and lo <= jp <= hi
            uu = np.ascontiguousarray(tlerp_fields(u[jrec % K], u[jp % K] if there else None, w))
            vv = np.ascontiguousarray(tlerp_fields(v[jrec % K], v[jp % K] if there else None, w))
            was = trk.alive.copy()
            pn, mn = trk.step(jrec, uu, vv, ss)
            pos[jt + 1, mn == 1] = pn[mn == 1]
            msk[jt + 1, mn == 1] = 1
            kill[(was == 1) & (trk.alive == 0)] = jrec
        jit[jt + 1], alv[jt + 1] = trk.jiT, trk.alive
    return dict(pos=pos, msk=msk, jiT=jit, alive=alv, kill_rec=kill, final=trk.pos.copy(), ncross=trk.ncross)


def same_replay(a, b):
    return (np.array_equal(a["pos"].view(np.uint64), b["pos"].view(np.uint64)) and np.array_equal(a["msk"], b["msk"])
            and np.array_equal(a["jiT"], b["jiT"]) and np.array_equal(a["alive"], b["alive"])
            and np.array_equal(a["kill_rec"], b["kill_rec"]) and np.array_equal(a["final"].view(np.uint64), b["final"].view(np.uint64)))


def test_weights_follow_the_contract():
    # n = 1: one sub-step at tau = 1/2
    assert tlerp_weights(1, 0.5) == [(0, 0.)]
    assert tlerp_weights(1, 0.) == [(1, 0.5)] and tlerp_weights(1, 1.) == [(-1, 0.5)]
    # odd n, centred records: the middle sub-step has no partner, the halves look back and ahead with mirrored weights
    w5 = tlerp_weights(5, 0.5)
    assert [s for s, _ in w5] == [-1, -1, 0, 1, 1]
    assert [w for _, w in w5] == [0.5 - 0.1, 0.5 - 0.3, 0., 0.7 - 0.5, 0.9 - 0.5]
    # even n: no sub-step sits on the validity time; snapshots at the start never look back
    assert [s for s, _ in tlerp_weights(6, 0.5)] == [-1, -1, -1, 1, 1, 1]
    assert [s for s, _ in tlerp_weights(6, 0.)] == [1] * 6 and [s for s, _ in tlerp_weights(24, 0.3)].count(-1) == 7
    for n in (1, 2, 5, 6, 24):
        for ph in (0., 0.3, 0.5, 1.):
            w = tlerp_weights(n, ph)
            assert all(0. <= x <= 1. for _, x in w)
            assert [s for s, _ in w] == sorted(s for s, _ in w)              # at most two phases, looking back first


def test_blend_is_three_rounded_fp64_operations_on_the_records_values():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    w = np.float64(1.) / np.float64(3.)
    F = tlerp_fields(a, b, w)
    assert F.dtype == np.float64
    for k in range(0, 1000, 97):                         # element by element with python floats (fp64, no FMA)
        fc, fp = float(a[k]), float(b[k])
        assert F[k] == fc + float(w) * (fp - fc)
    assert tlerp_fields(a, None, w).dtype == np.float64 and np.array_equal(tlerp_fields(a, None, w), a.astype(np.float64))
    bad = b.copy()
    bad[::3] = np.nan
    assert np.array_equal(tlerp_fields(a, None, 0.25), a.astype(np.float64))   # an absent partner cannot leak in


def _g12_replays(golden, nsub, phase, span, strat=1):
    g, grid, u, v, sic, yx0, jiT0 = g12_inputs(golden)
    nP = len(yx0)
    rf, rl = np.full(nP, 2), np.full(nP, 7)
    rl[::5] = 5
    rf[::7] = 3
    args = (grid, yx0, jiT0, u, v, sic, rf, rl, 2, 6, 3600. * nsub, nsub, strat)
    return oracle_replay(*args), oracle_replay_tlerp(*args, phase, span=span)


@pytest.mark.parametrize("strat", [0, 1])
def test_centred_records_and_one_step_per_record_is_the_plain_replay(golden, strat):
    """phase 0.5, n = 1: the one sub-step sits on the record's validity time -> no partner, today's loop, bit for bit"""
    plain, tl = _g12_replays(golden, 1, 0.5, None, strat)
    assert same_replay(plain, tl)


@pytest.mark.parametrize("nsub,phase", [(6, 0.5), (5, 0.3), (2, 0.)])
def test_no_partner_anywhere_is_the_substep_replay(golden, nsub, phase):
    plain, tl = _g12_replays(golden, nsub, phase, (None, None))
    assert same_replay(plain, tl)
    assert 0 < plain["alive"][-1].sum() < plain["alive"].shape[1]


def test_blending_changes_the_trajectories(golden):
    """... and with partners the replay is another run (the identities above are not vacuous)"""
    plain, tl = _g12_replays(golden, 6, 0.5, None)
    assert not np.array_equal(plain["final"], tl["final"])
    # partners outside the span are not used: a span that holds no neighbour of any stepped record is the plain replay again
    assert same_replay(_g12_replays(golden, 6, 0.5, (20, 30))[1], plain)


# ---- the driver's planning ----------------------------------------------------------------------------------------------------
def test_plan_tinterp_fixed_time_mode():
    """-F: batches of one record; every launch needs the record before (resident), the record behind (uploaded in front of it)"""
    Nt, kstrt = 5, 2
    K, K_plan = drv.tinterp_slots(2)
    assert (K, K_plan) == (3, 2)
    batches = drv.plan_batches(Nt, kstrt, K_plan, True)
    assert batches == [(k, 1) for k in range(Nt)]
    plan = drv.plan_tinterp(batches, Nt, K)
    assert [p["slot0"] for p in plan] == [0, 1, 2, 0, 1]
    assert [p["have_prev"] for p in plan] == [False, True, True, True, True]
    assert [p["have_next"] for p in plan] == [True, True, True, True, False]
    assert [p["prev_slot"] for p in plan] == [None, 0, 1, 2, 0] and [p["next_slot"] for p in plan] == [1, 2, 0, 1, None]
    assert [p["ahead"] for p in plan] == [1, 2, 3, 4, None] and all(p["behind"] == [] for p in plan)
    for p in plan:                                       # a launch's record and partners sit in distinct slots
        used = [p["slot0"]] + [s for s in (p["prev_slot"], p["next_slot"]) if s is not None]
        assert len(set(used)) == len(used)


def test_plan_tinterp_fused_batches():
    Nt, kstrt = 23, 0
    K, K_plan = drv.tinterp_slots(12)
    assert (K, K_plan) == (12, 10)
    ends = {6, 22}                                       # 2-D time: some buoys end at record 6
    batches = drv.plan_batches(Nt, kstrt, K_plan, False, 1, ends)
    assert batches == [(0, 5), (5, 2), (7, 5), (12, 5), (17, 5), (22, 1)]
    plan = drv.plan_tinterp(batches, Nt, K)
    assert [p["ahead"] for p in plan] == [5, 7, 12, 17, 22, None]
    assert [p["behind"] for p in plan] == [[6], [8, 9, 10, 11], [13, 14, 15, 16], [18, 19, 20, 21], [], []]
    assert [(p["have_prev"], p["have_next"]) for p in plan] == [(False, True)] + [(True, True)] * 4 + [(True, False)]
    for ib, p in enumerate(plan):
        jt0, m = batches[ib]
        # what is resident or travelling while batch ib runs: its partners, itself, the next batch and -- uploaded in front of the
        # next launch, possibly while this one still runs -- the look-ahead of the next batch: all in distinct slots
        recs = list(range(jt0 - 1 if p["have_prev"] else jt0, jt0 + m)) + ([p["ahead"]] if p["ahead"] is not None else []) + p["behind"]
        if ib + 1 < len(plan) and plan[ib + 1]["ahead"] is not None:
            recs.append(plan[ib + 1]["ahead"])
        assert recs == list(range(recs[0], recs[-1] + 1)) and len(recs) <= K
        assert p["prev_slot"] == ((jt0 - 1) % K if jt0 else None) and p["slot0"] == jt0 % K
    with pytest.raises(ValueError, match="do not fit"):
        drv.plan_tinterp([(0, 5)], 9, 6)


def test_boxes_are_one_record_wider_with_tinterp():
    assert drv.batch_box_age(0, 4) == 3 and drv.batch_box_age(7, 1) == 7            # today's rule
    assert drv.batch_box_age(0, 4, True) == 4 and drv.batch_box_age(7, 1, True) == 8

    class Mesh:
        Nj, Ni, nsub = 200, 200, 6
    box_of = _lib.Context.box_of
    b0 = (100, 110, 80, 90)
    # a batch of 2 records planned right after the evaluation, then one of 3: the first batch's box must hold what the FIRST
    # record of the second batch can touch (D = reach(2) = 17), because its last record is that record's partner
    first = box_of(Mesh, *b0, drv.batch_box_age(0, 2, True), align=1)
    need = box_of(Mesh, *b0, 2, align=1)
    assert first == need == (100 - 2 - 17, 110 + 3 + 17, 80 - 2 - 17, 90 + 3 + 17)
    today = box_of(Mesh, *b0, drv.batch_box_age(0, 2, False), align=1)
    assert today[0] == first[0] + Mesh.nsub and today[1] == first[1] - Mesh.nsub    # too small by nsub cells on every side


def test_parse_args_tinterp():
    base = ["-i", "a.nc", "-m", "m.nc", "-s", "s.nc"]
    assert drv.parse_args(base).tinterp == "off"
    for v in ("off", "centre", "start"):
        assert drv.parse_args(base + ["--tinterp", v]).tinterp == v
    a = drv.parse_args(base + ["--rdt", "auto", "--nsub", "24", "--tinterp", "centre"])
    assert a.nsub == 24 and a.tinterp == "centre"
    for bad in (["--tinterp", "linear"], ["--tinterp", "0.5"], ["--tinterp"]):
        with pytest.raises(SystemExit):
            drv.parse_args(base + bad)
    assert tinterp_phase("centre") == 0.5 and tinterp_phase("start") == 0. and tinterp_phase(0.3) == 0.3
    for bad in ("middle", -0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            tinterp_phase(bad)


def test_run_tlerp_is_exported_and_bound():
    _lib.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(so, "sitrk_run_tlerp")
    res, args = _lib._SIGNATURES["sitrk_run_tlerp"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                            ctypes.c_int, ctypes.c_int]
    assert hasattr(_lib.Context, "run_tlerp")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "sitrk.h")).read()
    assert "int sitrk_run_tlerp(sitrk_t *h, int slot0, int jrec0, int nsteps, double phase, int have_prev, int have_next);" in hdr
