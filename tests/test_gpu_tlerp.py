"""Sub-stepped advection with the fields interpolated in time on the MI355X (sitrk_run_tlerp, advect_tlerp_kernel): bit parity
with the oracle fed with blended fields (tests/test_tlerp.py::oracle_replay_tlerp), the identities with sitrk_run / sitrk_step,
a closed-form trajectory, ingest with partner slots, errors, the command line with --tinterp."""
import numpy as np
import pytest

from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv
from sitrack_amd import synthetic as syn
from test_gpu_substep import expected_record, load_all, make_case_6h, random_case, same_bits, tracker
from test_tlerp import oracle_replay_tlerp

pytestmark = pytest.mark.gpu


def load_ring(trk, u, v, sic, dtype, nrec):
    """record k = fields k % K in slot k, k < nrec (the ring random_case's six fields are replayed on)"""
    K = u.shape[0]
    for k in range(nrec):
        trk.load_record(k, u[k % K].astype(dtype), v[k % K].astype(dtype), sic[k % K].astype(dtype))


def same_state(a, b):
    return (same_bits(a["yx"], b["yx"]) and np.array_equal(a["vJIt"], b["vJIt"]) and np.array_equal(a["iAlive"], b["iAlive"])
            and np.array_equal(a["kill_rec"], b["kill_rec"]))


# strategies 0 / 1 / 2, both record types, sorted and unsorted buoys, per-buoy record windows everywhere; nsub odd (a sub-step on
# the validity time: no partner) and even; phase 0 (never looks back), 0.5, 0.3; `outer`: records 0 and 8 are partners of the first
# and the last record stepped.  Every input has more crossings than buoys and 0 < alive < nP at the end (checked on the oracle).
@pytest.mark.parametrize("strat,warp,sort,dtype,nsub,phase,outer", [
    (1, 1.0, True, np.float32, 6, 0.5, True), (0, 1.0, False, np.float64, 5, 0.5, True), (2, 0.0, True, np.float32, 24, 0.3, True),
    (1, 0.0, False, np.float64, 2, 0.0, False), (2, 1.0, False, np.float64, 1, 0.3, True), (0, 0.0, True, np.float32, 24, 0.5, True),
    (1, 1.0, True, np.float32, 1, 0.0, True)])
def test_random_clouds_vs_oracle_replay_tlerp(strat, warp, sort, dtype, nsub, phase, outer):
    grid, u, v, sic, yx, ji = random_case(warp, 31 + nsub + strat)
    nP, Nt, kstrt, rdt = len(yx), 7, 1, 3600. * nsub
    rng = np.random.default_rng(nsub)
    rf = np.full(nP, kstrt) + rng.integers(0, 3, nP) * (rng.random(nP) < 0.2)
    rl = np.full(nP, kstrt + Nt - 1) - rng.integers(0, 3, nP) * (rng.random(nP) < 0.2)
    ref = oracle_replay_tlerp(grid, yx, ji, u.astype(dtype).astype(np.float64), v.astype(dtype).astype(np.float64),
                              sic.astype(dtype).astype(np.float64), rf, rl, kstrt, Nt, rdt, nsub, strat, phase,
                              span=(0, 8) if outer else None)
    assert ref["ncross"] > nP and 0 < ref["alive"][-1].sum() < nP
    trk = tracker(grid, rdt, nsub, strat, nslots=9, dtype=dtype)
    load_ring(trk, u, v, sic, dtype, 9)
    # record by record: one launch of one record with its partners; every record's output
    trk.set_buoys(yx, ji, rf, rl, sort=sort)
    trk.ctx.launch_stats(reset=True)
    for jt in range(Nt):
        trk.run(jt + kstrt, jt + kstrt, 1, tinterp=phase, have_prev=outer or jt > 0, have_next=outer or jt < Nt - 1)
        pos, msk = trk.record(jt + kstrt)
        want_p, want_m = expected_record(ref["pos"], ref["msk"], rf, kstrt, jt + 1)
        assert np.array_equal(msk, want_m) and same_bits(pos, want_p), jt
    st = trk.state()
    assert same_bits(st["yx"], ref["final"]) and np.array_equal(st["vJIt"], ref["jiT"][-1])
    assert np.array_equal(st["iAlive"], ref["alive"][-1]) and np.array_equal(st["kill_rec"], ref["kill_rec"])
    assert trk.ctx.launch_stats(reset=True) == {"fused_launches": Nt, "fused_records": Nt, "step_launches": 0}
    assert trk.ctx.lane_stats() == {"lane_segments": 0, "lane_launches": 0}
    # the same records in one call
    trk.set_buoys(yx, ji, rf, rl, sort=sort)
    trk.run(kstrt, kstrt, Nt, tinterp=phase, have_prev=outer, have_next=outer)
    st2 = trk.state()
    assert same_state(st2, st)
    pos, msk = trk.record(kstrt + Nt - 1)
    want_p, want_m = expected_record(ref["pos"], ref["msk"], rf, kstrt, Nt)
    assert np.array_equal(msk, want_m) and same_bits(pos, want_p)
    ls = trk.ctx.launch_stats()
    assert ls["fused_records"] == Nt and ls["step_launches"] == 0 and 1 <= ls["fused_launches"] <= Nt
    trk.close()


# ---- identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsub,phase,dtype,strat", [(6, 0.5, np.float32, 1), (1, 0.3, np.float32, 1), (5, 0.0, np.float64, 0)])
def test_no_partner_one_record_equals_step(nsub, phase, dtype, strat):
    grid, u, v, sic, yx, ji = random_case(1.0, 77, nP=4000)
    out = []
    for mode in ("step", "tlerp"):
        trk = tracker(grid, 3600. * nsub, nsub, strat, nslots=6, dtype=dtype)
        load_all(trk, u, v, sic, dtype)
        trk.set_buoys(yx, ji)
        recs = []
        for k in range(6):
            if mode == "step":
                trk.step(k, k)
            else:
                trk.run(k, k, 1, tinterp=phase)
            recs.append(trk.record(k))
        out.append((trk.state(), recs))
        trk.close()
    (a, ra), (b, rb) = out
    assert same_state(a, b) and 0 < a["iAlive"].sum() < len(yx)
    for (pa, ma), (pb, mb) in zip(ra, rb):
        assert same_bits(pa, pb) and np.array_equal(ma, mb)


@pytest.mark.parametrize("dtype,strat", [(np.float32, 1), (np.float64, 2), (np.float32, 0)])
def test_centred_records_one_step_per_record_equals_run(dtype, strat):
    """phase 0.5, nsub 1: the one sub-step sits on the record's validity time -- partners resident, none read"""
    grid, u, v, sic, yx, ji = random_case(1.0, 5, nP=4000)
    out = []
    for mode in ("run", "tlerp"):
        trk = tracker(grid, 3600., 1, strat, nslots=6, dtype=dtype)
        load_all(trk, u, v, sic, dtype)
        trk.set_buoys(yx, ji)
        if mode == "run":
            trk.ctx.run(1, 1, 4)
        else:
            trk.run(1, 1, 4, tinterp='centre', have_prev=True, have_next=True)
        out.append(trk.state())
        trk.close()
    assert same_state(out[0], out[1]) and (out[0]["vJIt"] != ji).any()


def test_one_call_equals_record_by_record_and_resort_changes_nothing():
    grid, u, v, sic, yx, ji = random_case(1.0, 77, nP=5000)
    nsub, Nt = 6, 7
    out = []
    for mode in ("one", "each", "resort", "fuse3"):
        trk = tracker(grid, 3600. * nsub, nsub, nslots=9)
        load_ring(trk, u, v, sic, np.float32, 9)
        if mode == "resort":
            trk.ctx.set_resort(2)
        if mode == "fuse3":
            trk.ctx.set_tuning(fuse=3)
        trk.set_buoys(yx, ji, sort=(mode != "resort"))
        trk.ctx.launch_stats(reset=True)
        if mode == "each":
            for k in range(Nt):
                trk.run(1 + k, 1 + k, 1, tinterp=0.5, have_prev=True, have_next=True)
        else:
            trk.run(1, 1, Nt, tinterp=0.5, have_prev=True, have_next=True)
        out.append((trk.state(), trk.record(Nt), trk.ctx.launch_stats()))
        trk.close()
    for s, r, ls in out[1:]:
        assert same_state(out[0][0], s)
        assert same_bits(out[0][1][0], r[0]) and np.array_equal(out[0][1][1], r[1])
        assert ls["fused_records"] == Nt and ls["step_launches"] == 0
    assert out[1][2]["fused_launches"] == Nt and out[3][2]["fused_launches"] == 3 and out[2][2]["fused_launches"] >= 4
    assert 0 < out[0][0]["iAlive"].sum() < len(yx)


# ---- physics ----------------------------------------------------------------------------------------------------------------------
def test_linear_in_time_field_is_integrated_exactly():
    """uniform u_k = a k rdt as snapshots at the start of their interval (phase 0): midpoint sampling of the linear blend
    integrates it exactly, x = x0 + sum_k (u_k + u_k+1)/2 rdt/1000.  Tolerance 1e-9 km: 48 additions at magnitudes below 2^11 km
    round to about 1e-11 km in total, times a margin of 100.  sitrk_run on the same records is a*rdt^2*N/2 = 4.32 km short."""
    Nj, Ni, rdt, nsub, N = 60, 80, 21600., 6, 4
    a = 0.4 / 86400.
    grid = syn.make_grid(Nj, Ni, dkm=4.0, warp=0.0)
    _, yx = syn.make_buoys(grid, 1500, seed=7, frac=0.7)
    ji = syn.regular_host_cell(grid, yx).astype(np.int64)
    sel = (ji[:, 0] > 5) & (ji[:, 0] < Nj - 6) & (ji[:, 1] > 5) & (ji[:, 1] < Ni - 14)     # 17.3 km = 4.3 cells to travel, no rim
    yx, ji = yx[sel], ji[sel]
    assert len(yx) > 500
    uk = (a * np.arange(N + 1) * rdt).astype(np.float32)                                    # the stored values
    want = yx[:, 1] + sum((np.float64(uk[k]) + np.float64(uk[k + 1])) / 2. * rdt / 1000. for k in range(N))
    res = []
    for mode in ("tlerp", "run"):
        trk = tracker(grid, rdt, nsub, nslots=N + 1)
        for k in range(N + 1):
            trk.load_record(k, np.full((Nj, Ni), uk[k], dtype=np.float32), np.zeros((Nj, Ni), dtype=np.float32),
                            np.ones((Nj, Ni), dtype=np.float32))
        trk.set_buoys(yx, ji)
        if mode == "tlerp":
            trk.run(0, 0, N, tinterp='start', have_next=True)
        else:
            trk.ctx.run(0, 0, N)
        res.append(trk.state())
        trk.close()
    tl, plain = res
    assert tl["iAlive"].all() and plain["iAlive"].all()
    err = np.abs(tl["yx"][:, 1] - want).max()
    print("max |x - closed form| = %.3e km; sitrk_run differs by %.6f km" % (err, np.abs(plain["yx"][:, 1] - want).min()))
    assert err <= 1e-9
    assert same_bits(tl["yx"][:, 0], yx[:, 0])                                              # v = 0: y untouched
    assert np.abs(plain["yx"][:, 1] - want).min() > 4.0
    assert (tl["vJIt"][:, 1] - ji[:, 1]).min() >= 4                                         # the buoys did change cells


# ---- ingest -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsub", [3, 6])
def test_box_and_band_ingest_with_partner_boxes_equal_full_ingest(nsub):
    grid, u, v, sic, yx, ji = random_case(1.0, 123, nP=2500, Nj=140, Ni=150, umax=1.0)
    sel = (ji[:, 0] > 50) & (ji[:, 0] < 90) & (ji[:, 1] > 55) & (ji[:, 1] < 95)      # a compact cloud: the box is a small part
    yx, ji = yx[sel], ji[sel]
    rdt, m, S = 3600. * nsub, 3, 8
    res = []
    for mode in ("full", "box", "rows"):
        trk = tracker(grid, rdt, nsub, nslots=S)
        trk.set_buoys(yx, ji)
        ctx = trk.ctx
        for b in range(2):
            # the batch's records and the record behind it (its last partner) over ONE box: what the batch's last record can touch,
            # one record wider -- the last record will be the partner of the next batch's first one.  The record in front of
            # the batch stays as the batch before left it.
            box = ctx.buoy_box() if mode != "full" else None
            for r in range(m + 1):
                k, slot = (b * m + r) % 6, (b * m + r) % S
                if mode == "box":
                    j0, j1, i0, i1 = ctx.box_of(*box, m)
                    assert (j1 - j0) * (i1 - i0) < grid["Nj"] * grid["Ni"]
                    ctx.push_record_box(slot, j0, j1, i0, i1, u[k][j0:j1, i0:i1], v[k][j0:j1, i0:i1], sic[k][j0:j1, i0:i1])
                elif mode == "rows":
                    j0, j1 = ctx.band(m)
                    ctx.push_record_rows(slot, j0, j1, u[k][j0:j1], v[k][j0:j1], sic[k][j0:j1])
                else:
                    trk.load_record(slot, u[k], v[k], sic[k])
            trk.run(b * m, (b * m) % S, m, tinterp='centre', have_prev=b > 0, have_next=True)
        res.append(trk.state())
        trk.close()
    for s in res[1:]:
        assert same_state(res[0], s)
    alive = res[0]["iAlive"] == 1
    assert np.abs(res[0]["vJIt"][alive] - ji[alive]).max() > m


def test_unwidened_partner_box_is_refused_and_the_handle_goes_on():
    """record 0's own box (D = reach(0)) is too small for it as the partner of record 1 (D = reach(1)): refused with check_band's
    message; uploaded again over the wider box, the same handle steps on and ends where full ingest ends"""
    grid, u, v, sic, yx, ji = random_case(1.0, 124, nP=1500, Nj=140, Ni=150)
    sel = (ji[:, 0] > 50) & (ji[:, 0] < 90) & (ji[:, 1] > 55) & (ji[:, 1] < 95)
    yx, ji = yx[sel], ji[sel]
    nsub = 6
    full = tracker(grid, 21600., nsub, nslots=4)
    load_all(full, u[:3], v[:3], sic[:3], np.float32)
    full.set_buoys(yx, ji)
    full.run(0, 0, 2, tinterp='centre', have_next=True)
    want = full.state()
    full.close()

    trk = tracker(grid, 21600., nsub, nslots=4)
    trk.set_buoys(yx, ji)
    ctx = trk.ctx
    box = ctx.buoy_box()

    def push(slot, k, age):
        j0, j1, i0, i1 = ctx.box_of(*box, age)
        ctx.push_record_box(slot, j0, j1, i0, i1, u[k][j0:j1, i0:i1], v[k][j0:j1, i0:i1], sic[k][j0:j1, i0:i1])
    push(0, 0, 0)
    push(1, 1, 1)
    push(2, 2, 1)
    trk.run(0, 0, 1, tinterp='centre', have_next=True)                  # record 0: its own box is enough, partner 1 holds more
    with pytest.raises(_lib.SitrkError, match="can touch (rows|columns)"):
        trk.run(1, 1, 1, tinterp='centre', have_prev=True, have_next=True)
    push(0, 0, 1)
    trk.run(1, 1, 1, tinterp='centre', have_prev=True, have_next=True)
    assert same_state(trk.state(), want)
    trk.close()


def test_upload_into_a_partner_slot_waits_for_the_launch():
    """a record pushed into a partner slot right behind the asynchronous launch that reads it must wait for that launch"""
    grid, u, v, sic, yx, ji = random_case(1.0, 77, nP=20000)
    out = []
    for sync in (True, False):
        trk = tracker(grid, 3600. * 24, 24, nslots=5)
        load_all(trk, u[:5], v[:5], sic[:5], np.float32)
        trk.set_buoys(yx, ji)
        trk.run(1, 1, 3, tinterp='centre', have_prev=True, have_next=True)      # reads slots 0 and 4 as partners only
        if sync:
            trk.ctx.sync()
        trk.load_record(4, u[5], 2 * v[5], sic[5])
        trk.load_record(0, 2 * u[5], v[0], sic[0])
        trk.run(4, 4, 1, tinterp='centre', have_next=True)                      # ... and steps with what was pushed
        out.append(trk.state())
        trk.close()
    assert same_state(out[0], out[1])


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    grid, u, v, sic, yx, ji = random_case(0.0, 9, nP=2000)
    trk = tracker(grid, 21600., 6, nslots=3)
    load_all(trk, u[:3], v[:3], sic[:3], np.float32)
    trk.set_buoys(yx, ji)
    with pytest.raises(_lib.SitrkError, match="do not fit 3 slots"):
        trk.ctx.run_tlerp(0, 0, 2, 0.5, True, True)
    with pytest.raises(_lib.SitrkError, match="do not fit 3 slots"):
        trk.ctx.run_tlerp(0, 0, 3, 0.5, False, True)
    trk.ctx.run_tlerp(0, 0, 2, 0.5, False, True)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(_lib.SitrkError, match=r"phase must be in \[0,1\]"):
            trk.ctx.run_tlerp(2, 2, 1, bad, True, False)
        trk.ctx.run_tlerp(2, 2, 1, 0.5, True, False)
    with pytest.raises(_lib.SitrkError, match="nsteps"):
        trk.ctx.run_tlerp(0, 0, -1, 0.5, False, False)
    with pytest.raises(_lib.SitrkError, match="slot0 out of range"):
        trk.ctx.run_tlerp(3, 0, 1, 0.5, False, False)
    st = trk.state()
    assert 0 < st["iAlive"].sum() <= len(yx)
    # a buoy in row 1: the fused kernels do not apply and the one-record kernel cannot blend
    yr = grid["Yf"][1, 40] - 1.0
    yx2 = np.concatenate([yx, [[yr, 0.5 * (grid["Xf"][1, 39] + grid["Xf"][1, 40])]]])
    ji2 = np.concatenate([ji, np.array([[1, 40]])])
    trk.set_buoys(yx2, ji2)
    with pytest.raises(_lib.SitrkError, match="cannot blend"):
        trk.run(0, 0, 1, tinterp=0.5, have_next=True)
    trk.run(0, 0, 1)                                                   # the same set without blending: sitrk_step's fallback
    trk.set_buoys(yx, ji)
    trk.run(0, 0, 1, tinterp=0.5, have_next=True)
    trk.close()
    empty = tracker(grid, 21600., 6, nslots=3)
    with pytest.raises(_lib.SitrkError, match="sitrk_set_buoys"):
        empty.ctx.run_tlerp(0, 0, 1, 0.5, False, False)
    empty.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------
def oracle_driver_6h_tlerp(c, two_d_time, rdt, nsub, phase):
    """tests/test_gpu_substep.py::oracle_driver_6h with the blended replay; partners inside the records the run reads"""
    from oracle import oracle as orc
    g = c["g"]
    Nj, Ni = g["Nj"], g["Ni"]
    grid = {}
    for p in "fuvt":
        lat = c["ll"][p][:, 0]; lon = np.mod(c["ll"][p][:, 1], 360.)
        yx = orc.Geo2CartNPSkm1D(np.stack([lat, lon], axis=1))
        grid["Y" + p] = np.ascontiguousarray(yx[:, 0].reshape(Nj, Ni)); grid["X" + p] = np.ascontiguousarray(yx[:, 1].reshape(Nj, Ni))
    grid["tmask"] = c["tmask"]
    latT = c["ll"]["t"][:, 0].reshape(Nj, Ni); lonT = np.mod(c["ll"]["t"][:, 1], 360.).reshape(Nj, Ni)
    pSG = np.stack([c["sll"][:, 0].astype('f4').astype('f8'), np.mod(c["sll"][:, 1].astype('f4'), np.float32(360.)).astype('f8')], axis=1)
    pSC = c["yx"].astype('f4').astype('f8')
    res = np.full((Nj, Ni), np.sqrt(2.) * c.get("dkm", 10.0))
    tc = c["tc"]
    kstrt, Nt = 0, len(tc)
    nP, oSG, oSC, oIDs, ojiT, overt, keep = orc.SeedInit(c["ids"], pSG, pSC, np.ascontiguousarray(latT), np.ascontiguousarray(lonT),
                                                          grid["Yf"], grid["Xf"], res, c["tmask"], c["sic"][kstrt].astype('f8'))
    z1 = np.zeros(nP, dtype=int) + kstrt; zL = np.zeros(nP, dtype=int) + (kstrt + Nt - 1)
    if two_d_time:
        z1, zL = drv.record_windows(c["tp"], tc, kstrt, kstrt + Nt - 1, tc[0], tc[-1], len(c["ids"]), rdt=rdt)
        z1, zL = z1[keep], zL[keep]
    r = oracle_replay_tlerp(grid, oSC, ojiT, c["u"].astype('f8'), c["v"].astype('f8'), c["sic"].astype('f8'), z1, zL, kstrt, Nt,
                            rdt, nsub, 1, phase, span=(kstrt, kstrt + Nt - 1))
    return dict(r, nP=nP, ids=oIDs, z1=z1, zL=zL)


@pytest.mark.parametrize("two_d_time,mode,extra", [(False, "centre", []), (True, "centre", []), (True, "start", []),
                                                   (False, "centre", ["--slots", "3"]), (True, "centre", ["--full-records"])])
def test_cli_6_hourly_tinterp_vs_oracle(tmp_path, monkeypatch, two_d_time, mode, extra):
    monkeypatch.chdir(tmp_path)
    c = make_case_6h(str(tmp_path), two_d_time)
    argv = (["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "--rdt", "auto", "--nsub", "6", "--tinterp", mode]
            + ([] if two_d_time else ["-F"]) + extra)
    out = drv.main(argv)
    Nt, step = len(c["tc"]), 21600
    assert out["Nt"] == Nt and out["kstrt"] == 0
    ref = oracle_driver_6h_tlerp(c, two_d_time, 21600., 6, 0.5 if mode == "centre" else 0.)
    nP = ref["nP"]
    assert out["nP"] == nP and np.array_equal(out["IDs"], ref["ids"])
    assert np.array_equal(out["vJIt"], ref["jiT"][-1]) and np.array_equal(out["iAlive"], ref["alive"][-1])
    assert out["launches"]["fused_launches"] > 0 and out["launches"]["step_launches"] == 0
    assert out["launches"]["fused_records"] == Nt
    if not two_d_time:
        f_full, f_12 = out["files"]
        t, ids, llo, yxo, mko = ncio.LoadNCdata(f_full, krec=-1, lmask=True)
        assert t.shape == (Nt + 1,) and t[0] == c["base"] and t[-1] == c["base"] + Nt * step
        assert np.array_equal(mko, ref["msk"])
        assert np.array_equal(yxo.astype('f4'), ref["pos"].astype('f4'))
        t2, _, _, yx2, mk2 = ncio.LoadNCdata(f_12, krec=-1, lmask=True)
        assert np.array_equal(yx2[1].astype('f4'), ref["pos"][Nt].astype('f4')) and np.array_equal(mk2[1], ref["msk"][Nt])
    else:
        (f_12,) = out["files"]
        t2, _, _, yx2, mk2, tp2 = ncio.LoadNCdata(f_12, krec=-1, lmask=True, lGetTimePos=True)
        kN, k0 = ref["zL"] + 1, ref["z1"]
        assert np.array_equal(yx2[0].astype('f4'), ref["pos"][k0, np.arange(nP)].astype('f4'))
        assert np.array_equal(yx2[1].astype('f4'), ref["pos"][kN, np.arange(nP)].astype('f4'))
        assert np.array_equal(mk2[1], ref["msk"][kN, np.arange(nP)])
        want_t1 = np.where(ref["msk"][kN, np.arange(nP)] == 1, c["tc"][ref["zL"]] - step // 2 + step, -9999)
        assert np.array_equal(tp2[1], want_t1) and np.array_equal(tp2[0], c["tc"][k0] - step // 2)
