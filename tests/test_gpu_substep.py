"""Sub-stepped advection on the MI355X (sitrk_set_substeps, advect_substep_kernel): bit parity with G12 and with the oracle
replay (tests/test_substep.py::oracle_replay), fused = stepped = host replay of today's kernels, ingest bands, the
command line on a 6-hourly file."""
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv
from sitrack_amd import synthetic as syn
from test_substep import g12_cases, g12_inputs, oracle_replay

pytestmark = pytest.mark.gpu
FILL = -9999.0


def tracker(grid, rdt, nsub, strat=1, nslots=6, dtype=np.float32):
    return sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=rdt,
                          iUVstrategy=strat, nslots=nslots, field_dtype=dtype, nsub=nsub)


def load_all(trk, u, v, sic, dtype):
    for k in range(u.shape[0]):
        trk.load_record(k, u[k].astype(dtype), v[k].astype(dtype), sic[k].astype(dtype))


def expected_record(pos, msk, rec_first, kstrt, k):
    """what sitrk_fetch_record answers for the record that produced series row k: the buoys that stepped there.  The
    reference's series also holds the seed position of a buoy whose window opens at row k (pre-written, :331-333), which
    no step produced: FillValue and mask 0 in the per-record output"""
    pre = (np.asarray(rec_first) - kstrt) == k
    m = np.where(pre, 0, msk[k]).astype(np.int8)
    p = np.where(m[:, None] == 1, pos[k], FILL)
    return p, m


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", range(8))
def test_g12_parity_stepped_and_fused(golden, case, dtype):
    g, grid, u, v, sic, yx0, jiT0 = g12_inputs(golden)
    tag, rdt, nsub, Nt, strat, rf, rl = list(g12_cases(g))[case]
    kstrt, K = int(g["kstrt"]), u.shape[0]
    trk = tracker(grid, rdt, nsub, strat, nslots=K, dtype=dtype)
    load_all(trk, u, v, sic, dtype)
    # record by record: sitrk_step launches the sub-stepping kernel with one record; every record's output
    trk.set_buoys(yx0, jiT0, rf, rl)
    for jt in range(Nt):
        jrec = jt + kstrt
        trk.step(jrec, jrec % K)
        pos, msk = trk.record(jrec)
        want_p, want_m = expected_record(g["pos_" + tag], g["msk_" + tag], rf, kstrt, jt + 1)
        assert np.array_equal(msk, want_m), (tag, jrec)
        assert same_bits(pos, want_p), (tag, jrec)
    st = trk.state()
    assert np.array_equal(st["vJIt"], g["jiT_" + tag][-1]) and np.array_equal(st["iAlive"], g["alive_" + tag][-1])
    assert np.array_equal(st["kill_rec"], g["kill_rec_" + tag])
    stepped = trk.ctx.launch_stats(reset=True)
    assert stepped["fused_launches"] == Nt and stepped["step_launches"] == 0
    # the same records in one fused launch
    trk.set_buoys(yx0, jiT0, rf, rl)
    trk.run(kstrt, kstrt % K, Nt) if Nt <= K else [trk.run(kstrt + b, (kstrt + b) % K, min(K, Nt - b)) for b in range(0, Nt, K)]
    st2 = trk.state()
    assert same_bits(st2["yx"], st["yx"])
    assert np.array_equal(st2["vJIt"], st["vJIt"]) and np.array_equal(st2["iAlive"], st["iAlive"])
    assert np.array_equal(st2["kill_rec"], st["kill_rec"])
    pos, msk = trk.record(kstrt + Nt - 1)
    want_p, want_m = expected_record(g["pos_" + tag], g["msk_" + tag], rf, kstrt, Nt)
    assert np.array_equal(msk, want_m) and same_bits(pos, want_p)
    trk.close()


def random_case(warp, seed, nP=3000, Nj=90, Ni=100, umax=1.2):
    grid = syn.make_grid(Nj, Ni, dkm=4.0, warp=warp)
    u, v, sic = syn.make_fields(grid, K=6, seed=seed, umax=umax, drift=0.4, ripple=0.15)
    sic = sic.copy()
    sic[:, 20:26, 30:50] = 0.02
    tm = grid["tmask"].copy()
    tm[50:54, 60:66] = 0
    grid["tmask"] = tm
    _, yx = syn.make_buoys(grid, nP, seed=seed + 1, frac=0.7)
    ctx = _lib.Context(0)
    ctx.set_grid(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"])
    found, ji, _ = sit.FindContainingCell(yx, syn.nearest_t_plane(grid, yx), ctx=ctx)
    ctx.close()
    return grid, u, v, sic, yx[found], ji[found].astype(np.int64)


@pytest.mark.parametrize("strat,warp,sort,dtype,nsub", [
    (1, 1.0, True, np.float32, 6), (0, 1.0, False, np.float64, 6), (2, 0.0, True, np.float32, 24),
    (1, 0.0, False, np.float64, 24), (2, 1.0, False, np.float64, 6), (0, 0.0, True, np.float32, 24)])
def test_random_clouds_vs_oracle_replay(strat, warp, sort, dtype, nsub):
    grid, u, v, sic, yx, ji = random_case(warp, 31 + nsub + strat)
    nP, Nt, kstrt, rdt = len(yx), 7, 1, 3600. * nsub
    rng = np.random.default_rng(nsub)
    rf = np.full(nP, kstrt) + rng.integers(0, 3, nP) * (rng.random(nP) < 0.2)
    rl = np.full(nP, kstrt + Nt - 1) - rng.integers(0, 3, nP) * (rng.random(nP) < 0.2)
    ref = oracle_replay(grid, yx, ji, u.astype(dtype).astype(np.float64), v.astype(dtype).astype(np.float64),
                        sic.astype(dtype).astype(np.float64), rf, rl, kstrt, Nt, rdt, nsub, strat)
    assert ref["ncross"] > nP and 0 < ref["alive"][-1].sum() < nP
    trk = tracker(grid, rdt, nsub, strat, nslots=6, dtype=dtype)
    load_all(trk, u, v, sic, dtype)
    trk.set_buoys(yx, ji, rf, rl, sort=sort)
    for jt in range(Nt):
        trk.step(jt + kstrt, (jt + kstrt) % 6)
        pos, msk = trk.record(jt + kstrt)
        want_p, want_m = expected_record(ref["pos"], ref["msk"], rf, kstrt, jt + 1)
        assert np.array_equal(msk, want_m) and same_bits(pos, want_p), jt
    st = trk.state()
    assert same_bits(st["yx"], ref["final"]) and np.array_equal(st["vJIt"], ref["jiT"][-1])
    assert np.array_equal(st["iAlive"], ref["alive"][-1]) and np.array_equal(st["kill_rec"], ref["kill_rec"])
    trk.close()


@pytest.mark.parametrize("nsub", [2, 6])
def test_fused_equals_stepped_equals_host_replay(nsub):
    grid, u, v, sic, yx, ji = random_case(1.0, 77, nP=5000)
    m, rdt = 6, 3600. * nsub
    states = []
    for mode in ("run", "step", "replay"):
        trk = tracker(grid, rdt if mode != "replay" else rdt / nsub, nsub if mode != "replay" else 1, nslots=6)
        load_all(trk, u, v, sic, np.float32)
        trk.set_buoys(yx, ji)
        trk.ctx.launch_stats(reset=True)
        if mode == "run":
            trk.run(0, 0, m)
        elif mode == "step":
            for k in range(m):
                trk.step(k, k)
        else:
            for k in range(m):
                for _ in range(nsub):
                    trk.step(k, k)             # today's one-record kernel, nsub times with the same jrec
        states.append((trk.state(), trk.record(m - 1), trk.ctx.launch_stats()))
        trk.close()
    (a, ra, la), (b, rb, lb), (c, rc, lc) = states
    for s in (b, c):
        assert same_bits(a["yx"], s["yx"]) and np.array_equal(a["vJIt"], s["vJIt"])
        assert np.array_equal(a["iAlive"], s["iAlive"]) and np.array_equal(a["kill_rec"], s["kill_rec"])
    assert same_bits(ra[0], rb[0]) and same_bits(ra[0], rc[0]) and np.array_equal(ra[1], rc[1])
    assert la == {"fused_launches": 1, "fused_records": m, "step_launches": 0}
    assert lb == {"fused_launches": m, "fused_records": m, "step_launches": 0}
    assert lc == {"fused_launches": 0, "fused_records": 0, "step_launches": m * nsub}
    assert 0 < a["iAlive"].sum() < len(yx)


def test_explicit_nsub_1_is_today():
    grid, u, v, sic, yx, ji = random_case(1.0, 5, nP=4000)
    out = []
    for explicit in (False, True):
        trk = tracker(grid, 3600., 1, nslots=6)
        if explicit:
            trk.ctx.set_substeps(1)
        load_all(trk, u, v, sic, np.float32)
        trk.set_buoys(yx, ji)
        trk.ctx.launch_stats(reset=True)
        trk.run(0, 0, 6)
        trk.step(6, 0)
        out.append((trk.state(), trk.ctx.launch_stats()))
        trk.close()
    (a, la), (b, lb) = out
    assert same_bits(a["yx"], b["yx"]) and np.array_equal(a["vJIt"], b["vJIt"]) and np.array_equal(a["kill_rec"], b["kill_rec"])
    assert la == lb == {"fused_launches": 1, "fused_records": 6, "step_launches": 1}
    with pytest.raises(_lib.SitrkError):
        _lib.Context(0).set_substeps(0)
    with pytest.raises(_lib.SitrkError):
        _lib.Context(0).set_substeps(1025)


def test_rim_buoys_take_the_one_record_kernel_nsub_times():
    """buoys set in the two outermost rows/columns: the fused kernels do not apply; the one-record kernel runs nsub times"""
    grid, u, v, sic, yx, ji = random_case(0.0, 9, nP=2000)
    yr, jr = grid["Yf"][1, 40] - 1.0, np.array([[1, 40]])          # a buoy in row 1 (numpy's wrap possible there)
    yx2 = np.concatenate([yx, [[yr, 0.5 * (grid["Xf"][1, 39] + grid["Xf"][1, 40])]]])
    ji2 = np.concatenate([ji, jr])
    ref = oracle_replay(grid, yx2, ji2, u.astype(np.float64), v.astype(np.float64), sic.astype(np.float64),
                        np.zeros(len(yx2), dtype=np.int64), np.full(len(yx2), 3), 0, 4, 21600., 6, 1)
    trk = tracker(grid, 21600., 6, nslots=6)
    load_all(trk, u, v, sic, np.float32)
    trk.set_buoys(yx2, ji2)
    trk.ctx.launch_stats(reset=True)
    trk.run(0, 0, 4)
    st = trk.state()
    assert same_bits(st["yx"], ref["final"]) and np.array_equal(st["vJIt"], ref["jiT"][-1])
    assert trk.ctx.launch_stats() == {"fused_launches": 0, "fused_records": 0, "step_launches": 24}
    trk.close()


@pytest.mark.parametrize("nsub", [3, 6])
def test_box_and_band_ingest_equal_full_ingest(nsub):
    grid, u, v, sic, yx, ji = random_case(1.0, 123, nP=2500, Nj=140, Ni=150, umax=1.0)
    sel = (ji[:, 0] > 50) & (ji[:, 0] < 90) & (ji[:, 1] > 55) & (ji[:, 1] < 95)      # a compact cloud: the box is a small part
    yx, ji = yx[sel], ji[sel]
    rdt, m = 3600. * nsub, 4
    res = []
    for mode in ("full", "box", "rows"):
        trk = tracker(grid, rdt, nsub, nslots=8)
        trk.set_buoys(yx, ji)
        ctx = trk.ctx
        if mode == "full":
            load_all(trk, u, v, sic, np.float32)
        for b in range(2):
            if mode != "full":
                box = ctx.buoy_box()
                for r in range(m):
                    k = (b * m + r) % 6
                    if mode == "box":
                        j0, j1, i0, i1 = ctx.box_of(*box, r)
                        assert (j1 - j0) * (i1 - i0) < grid["Nj"] * grid["Ni"]
                        ctx.push_record_box((b * m + r) % 8, j0, j1, i0, i1, u[k][j0:j1, i0:i1], v[k][j0:j1, i0:i1], sic[k][j0:j1, i0:i1])
                    else:
                        j0, j1 = ctx.band(r)
                        ctx.push_record_rows((b * m + r) % 8, j0, j1, u[k][j0:j1], v[k][j0:j1], sic[k][j0:j1])
            else:
                for r in range(m):
                    k = (b * m + r) % 6
                    trk.load_record((b * m + r) % 8, u[k], v[k], sic[k])
            trk.run(b * m, (b * m) % 8, m)
        res.append(trk.state())
        trk.close()
    for s in res[1:]:
        assert same_bits(res[0]["yx"], s["yx"]) and np.array_equal(res[0]["vJIt"], s["vJIt"])
        assert np.array_equal(res[0]["kill_rec"], s["kill_rec"])
    alive = res[0]["iAlive"] == 1
    moved = np.abs(res[0]["vJIt"][alive] - ji[alive]).max()
    assert moved > m                                   # several cells per launch of m records


def test_todays_band_is_refused_with_substeps():
    """a slot uploaded over today's rows [jmin-2-a, jmax+3+a) only is refused once each record has 6 sub-steps (D = 5 at a = 0);
    the widened band of the same record is accepted"""
    grid, u, v, sic, yx, ji = random_case(1.0, 124, nP=1500, Nj=140, Ni=150)
    sel = (ji[:, 0] > 50) & (ji[:, 0] < 90)
    Nj = grid["Nj"]
    for D, ok in ((0, False), (5, True)):
        trk = tracker(grid, 21600., 6, nslots=4)
        trk.set_buoys(yx[sel], ji[sel])
        jmin, jmax = trk.ctx.buoy_rows()
        lo, hi = max(0, jmin - 2 - D), min(Nj, jmax + 3 + D)
        trk.ctx.push_record_rows(0, lo, hi, u[0][lo:hi], v[0][lo:hi], sic[0][lo:hi])
        if ok:
            assert trk.ctx.band(0) == (lo, hi)
            trk.step(0, 0)
        else:
            with pytest.raises(_lib.SitrkError, match="can touch rows"):
                trk.step(0, 0)
        trk.close()


# ---- the command line on a 6-hourly file ------------------------------------------------------------------------------------
def make_case_6h(tmp, two_d_time, nrec=8):
    from test_driver import _write_nc3, make_case
    c = make_case(tmp, nrec=nrec, two_d_time=two_d_time)
    base, step = c["base"], 21600
    tc = (base + step // 2 + step * np.arange(nrec)).astype('i4')
    _write_nc3(c["si3"], {"time_counter": None, "y": c["g"]["Nj"], "x": c["g"]["Ni"]},
               {"time_counter": ('i4', ('time_counter',), tc, {"units": ncio.tunits_default}),
                "siconc": ('f4', ('time_counter', 'y', 'x'), c["sic"], None),
                "u_ice": ('f4', ('time_counter', 'y', 'x'), c["u"], None),
                "v_ice": ('f4', ('time_counter', 'y', 'x'), c["v"], None)})
    nP = len(c["ids"])
    tp = None
    if two_d_time:
        tp = np.stack([np.full(nP, base), np.full(nP, tc[-1] + step // 2)]).astype('i4')
        tp[0, ::7] = base + 2 * step
        tp[1, ::5] = base + 5 * step
        sv = {"time": ('i4', ('time',), np.array([base, tc[-1] + step // 2], dtype='i4'), {"units": ncio.tunits_default}),
              "buoy": ('i4', ('buoy',), np.arange(nP, dtype='i4'), None),
              "id_buoy": ('f8', ('buoy',), c["ids"].astype(np.float64), {"units": "ID of buoy"}),
              "time_pos": ('i4', ('time', 'buoy'), tp, {"units": ncio.tunits_default})}
        for k, a in (("latitude", c["sll"][:, 0]), ("longitude", c["sll"][:, 1]), ("y_pos", c["yx"][:, 0]), ("x_pos", c["yx"][:, 1])):
            sv[k] = ('f4', ('time', 'buoy'), np.repeat(a[None, :].astype('f4'), 2, axis=0), None)
        _write_nc3(c["seed"], {"time": None, "buoy": nP}, sv)
    c["tc"], c["tp"] = tc, tp
    return c


def oracle_driver_6h(c, two_d_time, rdt, nsub):
    """the driver restated with the oracle (seeding as tests/test_driver.py::oracle_run does it) and the sub-step replay"""
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
    r = oracle_replay(grid, oSC, ojiT, c["u"].astype('f8'), c["v"].astype('f8'), c["sic"].astype('f8'), z1, zL, kstrt, Nt,
                      rdt, nsub, 1)
    return dict(r, nP=nP, ids=oIDs, z1=z1, zL=zL)


@pytest.mark.parametrize("two_d_time,extra", [(False, []), (True, []), (False, ["--full-records"]), (True, ["--full-records"])])
def test_cli_6_hourly_rdt_auto_nsub_6_vs_oracle(tmp_path, monkeypatch, two_d_time, extra):
    monkeypatch.chdir(tmp_path)
    c = make_case_6h(str(tmp_path), two_d_time)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "--rdt", "auto", "--nsub", "6"] + ([] if two_d_time else ["-F"]) + extra
    out = drv.main(argv)
    Nt, step = len(c["tc"]), 21600
    assert out["Nt"] == Nt and out["kstrt"] == 0
    ref = oracle_driver_6h(c, two_d_time, 21600., 6)
    nP = ref["nP"]
    assert out["nP"] == nP and np.array_equal(out["IDs"], ref["ids"])
    assert np.array_equal(out["vJIt"], ref["jiT"][-1]) and np.array_equal(out["iAlive"], ref["alive"][-1])
    assert out["launches"]["fused_launches"] > 0 and out["launches"]["step_launches"] == 0
    if not two_d_time:
        f_full, f_12 = out["files"]
        assert f_full == './nc/NEMO-SI3_TEST4_EXP01_tracking_nemoTsi3_idlSeed_19961215h00_19961217h00.nc'
        assert f_12 == './nc/NEMO-SI3_TEST4_EXP01_tracking12_nemoTsi3_idlSeed_19961215h00_19961217h00.nc'
        t, ids, llo, yxo, mko = ncio.LoadNCdata(f_full, krec=-1, lmask=True)
        assert t.shape == (Nt + 1,) and t[0] == c["base"] and t[-1] == c["base"] + Nt * step
        assert np.array_equal(mko, ref["msk"])
        assert np.array_equal(yxo.astype('f4'), ref["pos"].astype('f4'))
        t2, _, _, yx2, mk2 = ncio.LoadNCdata(f_12, krec=-1, lmask=True)
        assert np.array_equal(yx2[1].astype('f4'), ref["pos"][Nt].astype('f4')) and np.array_equal(mk2[1], ref["msk"][Nt])
    else:
        (f_12,) = out["files"]
        assert '_tracking12_nemoTsi3_idlSeed_' in f_12
        t2, _, _, yx2, mk2, tp2 = ncio.LoadNCdata(f_12, krec=-1, lmask=True, lGetTimePos=True)
        kN, k0 = ref["zL"] + 1, ref["z1"]
        assert np.array_equal(yx2[0].astype('f4'), ref["pos"][k0, np.arange(nP)].astype('f4'))
        assert np.array_equal(yx2[1].astype('f4'), ref["pos"][kN, np.arange(nP)].astype('f4'))
        assert np.array_equal(mk2[1], ref["msk"][kN, np.arange(nP)])
        want_t1 = np.where(ref["msk"][kN, np.arange(nP)] == 1, c["tc"][ref["zL"]] - step // 2 + step, -9999)
        assert np.array_equal(tp2[1], want_t1) and np.array_equal(tp2[0], c["tc"][k0] - step // 2)
