"""Model fields along the trajectories on the MI355X (sitrk_sample_slot, sitrk_sample_fields, --sample).  Every buoy is
compared, values as bit patterns (NaN land values count), no tolerance.

Note on the reference-anchored test: row k+1 of the goldens' masks also carries the driver's pre-written seed row of the
buoys whose window opens at the NEXT record (mask 1 at their record k0, reference si3_part_tracker.py:331-333).  Those buoys
have not stepped at record k -- sitrk_fetch_record gives them mask 0, as tests/test_gpu_parity.py states -- so mode AFTER gives
them -9999 there, and their seed cell is checked by mode ENTER at the record they start in."""
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv
from sitrack_amd import synthetic as syn
from test_substep import oracle_replay

pytestmark = pytest.mark.gpu
FILL = -9999.


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def synth_fields(Nj, Ni, tmask, seed=0):
    """one f4 field with NaN on land and one f8 field, every cell a different value"""
    rng = np.random.default_rng(seed)
    a = (np.arange(Nj * Ni, dtype=np.float32).reshape(Nj, Ni) * np.float32(0.25) + rng.uniform(0, 0.1, (Nj, Ni)).astype(np.float32))
    a[np.asarray(tmask) == 0] = np.nan
    b = 1e3 + np.arange(Nj * Ni, dtype=np.float64).reshape(Nj, Ni) / 7. + rng.uniform(0, 1e-3, (Nj, Ni))
    return a, b


def expect(field, cells, take):
    out = np.full(len(take), FILL, dtype=field.dtype)
    t = np.asarray(take, dtype=bool)
    out[t] = field[cells[t, 0], cells[t, 1]]
    return out


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, "%s: %d of %d buoys differ, first %d: got %r want %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ----------------------------------------------------------------------------------------------- reference-anchored (G6)
@pytest.mark.parametrize("tag", ["curvi", "regular"])
@pytest.mark.parametrize("strat", [1, 0])
def test_g6_reference_cells_and_masks(golden, tag, strat):
    g = golden("g6_traj_%s.npz" % tag)
    Nj, Ni = int(g["Nj"]), int(g["Ni"])
    grid = syn.make_grid(Nj, Ni, dkm=float(g["dkm"]), warp=float(g["warp"]))
    K, kstrt, Nt = g["u"].shape[0], int(g["kstrt"]), int(g["Nt"])
    f4, f8 = synth_fields(Nj, Ni, g["tmask"], seed=1)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], g["tmask"], rdt=float(g["rdt"]),
                         iUVstrategy=strat, nslots=K)
    try:
        first, jiT0 = g["rec_first"], g["jiT0"]
        assert (first > kstrt).sum() == 12 and (g["rec_last"] < kstrt + Nt - 1).sum() == 12
        trk.set_buoys(g["yx0"], jiT0, first, g["rec_last"])
        trk.ctx.set_resort(5)
        for k in range(K):
            trk.load_record(k, g["u"][k], g["v"][k], g["sic"][k])
        msk, jit = g["msk_s%d" % strat], g["jiT_s%d" % strat]
        seen = np.zeros(len(first), dtype=bool)
        for jt in range(Nt):
            jrec = jt + kstrt
            starts = first == jrec
            seen |= starts
            (e4,) = trk.ctx.sample_fields(jrec, 'enter', [f4])
            (e8,) = trk.ctx.sample_fields(jrec, 'enter', [f8])
            same_bits(e4, expect(f4, jiT0, starts), "enter f4, record %d" % jrec)
            same_bits(e8, expect(f8, jiT0, starts), "enter f8, record %d" % jrec)
            trk.step(jrec, jrec % K)
            opening = (first - kstrt) == (jt + 1)            # the driver's pre-written seed row (module docstring)
            assert np.array_equal(jit[jt + 1][opening], jiT0[opening]) and (msk[jt + 1][opening] == 1).all()
            take = (msk[jt + 1] == 1) & ~opening
            (a4,) = trk.ctx.sample_fields(jrec, 'after', [f4])
            (a8,) = trk.ctx.sample_fields(jrec, 'after', [f8])
            same_bits(a4, expect(f4, jit[jt + 1], take), "after f4, record %d" % jrec)
            same_bits(a8, expect(f8, jit[jt + 1], take), "after f8, record %d" % jrec)
        assert seen.all()
    finally:
        trk.close()


# ----------------------------------------------------------------------------------------------- oracle replay
_CLOUD = {}


def cloud(warp, nP=4000, K=6):
    if warp not in _CLOUD:
        grid = syn.make_grid(90, 100, dkm=4.0, warp=warp)
        u, v, sic = syn.make_fields(grid, K=K, seed=41, umax=1.2, drift=0.4, ripple=0.15)
        sic = sic.copy()
        sic[:, 20:26, 30:50] = 0.02
        sic[:, 64:70, 25:70] = 0.02
        tm = grid["tmask"].copy()
        tm[50:54, 60:66] = 0
        grid["tmask"] = tm
        _, yx = syn.make_buoys(grid, 2 * nP, seed=42, frac=0.7)
        ctx = _lib.Context(0)
        ctx.set_grid(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"])
        found, ji, _ = sit.FindContainingCell(yx, syn.nearest_t_plane(grid, yx), ctx=ctx)
        ctx.close()
        assert found.sum() >= nP
        _CLOUD[warp] = (grid, u, v, sic, np.ascontiguousarray(yx[found][:nP]), ji[found][:nP].astype(np.int64))
    return _CLOUD[warp]


def windows_for(nP, Nt, seed=9):
    rng = np.random.default_rng(seed)
    first = np.zeros(nP, dtype=np.int64)
    last = np.full(nP, Nt - 1, dtype=np.int64)
    late = rng.uniform(size=nP) < 0.2
    first[late] = rng.integers(1, Nt - 2, late.sum())
    early = rng.uniform(size=nP) < 0.2
    last[early] = np.maximum(first[early], rng.integers(1, Nt - 1, early.sum()))
    return first, last


@pytest.mark.parametrize("warp", [1.0, 0.0])
@pytest.mark.parametrize("dtype,windowed,sort,nsub", [(np.float32, False, True, 1), (np.float64, True, True, 1),
                                                      (np.float32, True, False, 3), (np.float64, False, False, 3)])
def test_oracle_replay_record_by_record(warp, dtype, windowed, sort, nsub):
    grid, u, v, sic, yx, ji = cloud(warp)
    nP, K, Nt = len(yx), u.shape[0], 9
    Nj, Ni = grid["tmask"].shape
    f4, f8 = synth_fields(Nj, Ni, grid["tmask"], seed=2)
    first, last = windows_for(nP, Nt) if windowed else (np.zeros(nP, dtype=np.int64), np.full(nP, Nt - 1, dtype=np.int64))
    uu, vv, ss = (a.astype(dtype) for a in (u, v, sic))
    ref = oracle_replay(grid, yx, ji, *(a.astype(np.float64) for a in (uu, vv, ss)), first, last, 0, Nt, 3600. * nsub, nsub, 1)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=3600. * nsub,
                         nslots=K, field_dtype=dtype, nsub=nsub)
    try:
        for k in range(K):
            trk.load_record(k, uu[k], vv[k], ss[k])
        trk.set_buoys(yx, ji, first if windowed else None, last if windowed else None, sort=sort)
        trk.ctx.set_resort(4 if sort else 0)
        killed = 0
        for jrec in range(Nt):
            starts = ((first == jrec) if windowed else True) & (ref["alive"][jrec] == 1)      # no windows: every alive buoy
            cells0 = ref["jiT"][jrec].astype(np.int64)
            same_bits(trk.ctx.sample_slot(jrec % K, jrec, 'enter', 'siconc'), expect(ss[jrec % K], cells0, starts), "enter siconc %d" % jrec)
            trk.step(jrec, jrec % K)
            pos, mk = trk.record(jrec)
            take = (ref["msk"][jrec + 1] == 1) & ~(first == jrec + 1)          # (the oracle replay pre-writes the seed rows)
            assert np.array_equal(mk == 1, take)
            cells = ref["jiT"][jrec + 1].astype(np.int64)
            killed += int((take & (ref["alive"][jrec + 1] == 0)).sum())
            same_bits(trk.ctx.sample_slot(jrec % K, jrec, 'after', 'siconc'), expect(ss[jrec % K], cells, take), "after siconc %d" % jrec)
            same_bits(trk.ctx.sample_slot(jrec % K, jrec, 'after', 'u'), expect(uu[jrec % K], cells, take), "after u %d" % jrec)
            a4, b4 = trk.ctx.sample_fields(jrec, 'after', [f4, f4[::-1].copy()])
            same_bits(a4, expect(f4, cells, take), "after f4 %d" % jrec)
            same_bits(b4, expect(f4[::-1], cells, take), "after f4 flipped %d" % jrec)
            (a8,) = trk.ctx.sample_fields(jrec, 'after', [f8])
            same_bits(a8, expect(f8, cells, take), "after f8 %d" % jrec)
            got = trk.sample(jrec, {"thk": f4, "sic": 'siconc'}, slot=jrec % K)
            same_bits(got["thk"], a4, "IceTracker.sample dict")
            same_bits(got["sic"], expect(ss[jrec % K], cells, take), "IceTracker.sample siconc")
        assert killed > 0                                                    # buoys sampled in the cell that killed them
    finally:
        trk.close()


@pytest.mark.parametrize("windowed", [False, True])
def test_after_a_fused_run_on_two_lanes_and_a_resort(windowed):
    grid, u, v, sic, yx, ji = cloud(1.0)
    nP, K, Nt = len(yx), u.shape[0], 20
    Nj, Ni = grid["tmask"].shape
    f4, f8 = synth_fields(Nj, Ni, grid["tmask"], seed=3)
    first, last = windows_for(nP, Nt) if windowed else (np.zeros(nP, dtype=np.int64), np.full(nP, Nt - 1, dtype=np.int64))
    uu, vv, ss = (a.astype(np.float32) for a in (u, v, sic))
    ref = oracle_replay(grid, yx, ji, *(a.astype(np.float64) for a in (uu, vv, ss)), first, last, 0, Nt, 3600., 1, 1)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], nslots=K)
    try:
        ctx = trk.ctx
        ctx.set_tuning(lanes=2, lane_min_wg=1, xcd_group=1, fuse=2)
        for k in range(K):
            trk.load_record(k, uu[k], vv[k], ss[k])
        trk.set_buoys(yx, ji, first if windowed else None, last if windowed else None)
        ctx.set_resort(0)
        ctx.run(0, 0, Nt - 4)                                # two lanes
        assert windowed or ctx.lane_stats()["lane_segments"] >= 1
        ctx.sort_buoys()                                     # a re-sort between the run and the sample
        ctx.run((Nt - 4) % K, Nt - 4, 4)
        jrec = Nt - 1
        _, mk = trk.record(jrec)
        take, cells = mk == 1, ref["jiT"][Nt].astype(np.int64)
        assert take.any() and not take.all()
        same_bits(ctx.sample_slot(jrec % K, jrec, 'after', 'siconc'), expect(ss[jrec % K], cells, take), "after siconc")
        a4, = ctx.sample_fields(jrec, 'after', [f4])
        same_bits(a4, expect(f4, cells, take), "after f4")
        st = ctx.fetch()
        assert np.array_equal(st["jiT"], ref["jiT"][Nt]) and np.array_equal(st["alive"], ref["alive"][Nt])
    finally:
        trk.close()


# ----------------------------------------------------------------------------------------------- boxes, uploads in flight, limits
def test_box_ingest_in_flight_upload_and_refusals():
    grid, u, v, sic, yx, ji = cloud(1.0)
    nP, K = len(yx), u.shape[0]
    Nj, Ni = grid["tmask"].shape
    f4, f8 = synth_fields(Nj, Ni, grid["tmask"], seed=4)
    uu, vv, ss = (a.astype(np.float32) for a in (u, v, sic))
    ref = oracle_replay(grid, yx, ji, *(a.astype(np.float64) for a in (uu, vv, ss)), np.zeros(nP, dtype=np.int64), np.full(nP, 3, dtype=np.int64),
                        0, 3, 3600., 1, 1)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], nslots=K)
    try:
        ctx = trk.ctx
        trk.set_buoys(yx, ji)
        alive0 = np.ones(nP, dtype=bool)
        # a slot that never held a record
        with pytest.raises(_lib.SitrkError, match="holds no record"):
            ctx.sample_slot(1, 0, 'enter', 'siconc')
        trk.load_record(0, uu[0], vv[0], ss[0])
        full = ctx.sample_slot(0, 0, 'enter', 'siconc')
        same_bits(full, expect(ss[0], ji, alive0), "enter siconc, whole record")
        # the same record as a box in another slot: equal to the whole record
        j0, j1, i0, i1 = ctx.box(0)
        assert (j1 - j0) * (i1 - i0) < Nj * Ni
        ctx.push_record_box(1, j0, j1, i0, i1, uu[0][j0:j1, i0:i1], vv[0][j0:j1, i0:i1], ss[0][j0:j1, i0:i1])
        same_bits(ctx.sample_slot(1, 0, 'enter', 'siconc'), full, "enter siconc, box slot")
        box4, = ctx.sample_fields(0, 'enter', [f4[j0:j1, i0:i1]], box=(j0, j1, i0, i1))              # a view into the whole field: ld = Ni
        same_bits(box4, expect(f4, ji, alive0), "enter f4, box view")
        box8, = ctx.sample_fields(0, 'enter', [f8[j0:j1, i0:i1].copy()], box=(j0, j1, i0, i1))       # a packed box: ld = i1 - i0
        same_bits(box8, expect(f8, ji, alive0), "enter f8, packed box")
        # a box that misses a live buoy's cell
        jmid = int(np.median(ji[:, 0]))
        with pytest.raises(_lib.SitrkError, match=r"\d+ buoy\(s\) to sample"):
            ctx.sample_fields(0, 'enter', [f4[j0:jmid, i0:i1]], box=(j0, jmid, i0, i1))
        # a slot whose remembered box is stale: it holds rows the buoys are not in, its memory is full of numbers all the same
        ctx.push_record_box(2, 0, Nj, 0, Ni, uu[0], vv[0], ss[0])
        ctx.push_record_box(2, j0, jmid, i0, i1, uu[1][j0:jmid, i0:i1], vv[1][j0:jmid, i0:i1], ss[1][j0:jmid, i0:i1])
        with pytest.raises(_lib.SitrkError, match=r"\d+ buoy\(s\) to sample"):
            ctx.sample_slot(2, 0, 'enter', 'siconc')
        # nf = 8 works; nf = 9, a bad mode and a bad field are refused with a message
        many = ctx.sample_fields(0, 'enter', [f4 + np.float32(k) for k in range(8)])
        for k in range(8):
            same_bits(many[k], expect(f4 + np.float32(k), ji, alive0), "nf = 8, field %d" % k)
        with pytest.raises(_lib.SitrkError, match="nf must be in 1..8"):
            ctx.sample_fields(0, 'enter', [f4] * 9)
        with pytest.raises(_lib.SitrkError, match="mode must be"):
            ctx.sample_fields(0, 7, [f4])
        with pytest.raises(_lib.SitrkError, match="field must be"):
            ctx.sample_slot(0, 0, 'enter', 3)
        with pytest.raises(_lib.SitrkError, match="empty or outside"):
            ctx.sample_fields(0, 'enter', [f4[0:0]], box=(5, 5, 0, Ni))
        # a sample while the staged upload of the next record is in flight: same values, and the upload lands intact
        trk.step(0, 0)
        want = ctx.sample_slot(0, 0, 'after', 'siconc')

        def fill(bu, bv, bs):
            bu[...], bv[...], bs[...] = uu[1], vv[1], ss[1]
        ctx.stage_fill(3, 0, Nj, fill)
        got = ctx.sample_slot(0, 0, 'after', 'siconc')                 # no sync in between
        g4, = ctx.sample_fields(0, 'after', [f4])
        same_bits(got, want, "sample next to an upload in flight")
        take, cells = ref["msk"][1] == 1, ref["jiT"][1].astype(np.int64)
        same_bits(got, expect(ss[0], cells, take), "after siconc vs oracle")
        same_bits(g4, expect(f4, cells, take), "after f4 vs oracle")
        trk.step(1, 3)
        st = ctx.fetch()
        assert np.array_equal(st["jiT"], ref["jiT"][2]) and np.array_equal(st["alive"], ref["alive"][2])
        take2 = ref["msk"][2] == 1
        same_bits(ctx.sample_slot(3, 1, 'after', 'siconc'), expect(ss[1], ref["jiT"][2].astype(np.int64), take2), "the uploaded record")
        # no buoys
        trk.set_buoys(yx[:0], ji[:0])
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.sample_slot(0, 0, 'after', 'siconc')
    finally:
        trk.close()


# ----------------------------------------------------------------------------------------------- command line
def cli_case(tmp, two_d_time):
    """the case of tests/test_driver.py, its model file rewritten with a fourth (t,j,i) variable `sithic`"""
    from test_driver import _write_nc3, make_case
    c = make_case(str(tmp), two_d_time=two_d_time)
    nrec, (Nj, Ni) = len(c["tc"]), c["tmask"].shape
    rng = np.random.default_rng(12)
    thk = (rng.uniform(0.1, 4., (nrec, Nj, Ni)) + np.arange(nrec)[:, None, None]).astype('f4')
    thk[:, c["tmask"] == 0] = np.nan
    _write_nc3(c["si3"], {"time_counter": None, "y": Nj, "x": Ni},
               {"time_counter": ('i4', ('time_counter',), c["tc"], {"units": ncio.tunits_default}),
                "siconc": ('f4', ('time_counter', 'y', 'x'), c["sic"], None),
                "u_ice": ('f4', ('time_counter', 'y', 'x'), c["u"], None),
                "v_ice": ('f4', ('time_counter', 'y', 'x'), c["v"], None),
                "sithic": ('f4', ('time_counter', 'y', 'x'), thk, {"units": "m", "long_name": "ice thickness"})})
    c["sithic"] = thk
    return c


def cli_oracle(c, two_d_time):
    """oracle-driven restatement with the host cells after every record: what the numpy gather needs"""
    from oracle import oracle as orc
    from test_driver import oracle_run
    base = oracle_run(c, two_d_time)
    g = c["g"]
    Nj, Ni = g["Nj"], g["Ni"]
    grid = {}
    for p in "fuvt":
        lat = c["ll"][p][:, 0]; lon = np.mod(c["ll"][p][:, 1], 360.)
        yx = orc.Geo2CartNPSkm1D(np.stack([lat, lon], axis=1))
        grid["Y" + p] = np.ascontiguousarray(yx[:, 0].reshape(Nj, Ni)); grid["X" + p] = np.ascontiguousarray(yx[:, 1].reshape(Nj, Ni))
    grid["tmask"] = c["tmask"]
    Nt, nP = len(c["tc"]), base["nP"]
    # seeds as oracle_run located them: positions of row k0, cells by the oracle's own FindContainingCell through SeedInit
    latT = c["ll"]["t"][:, 0].reshape(Nj, Ni); lonT = np.mod(c["ll"]["t"][:, 1], 360.).reshape(Nj, Ni)
    pSG = np.stack([c["sll"][:, 0].astype('f4').astype('f8'), np.mod(c["sll"][:, 1].astype('f4'), np.float32(360.)).astype('f8')], axis=1)
    pSC = c["yx"].astype('f4').astype('f8')
    res = np.full((Nj, Ni), np.sqrt(2.) * c.get("dkm", 10.0))
    _, _, oSC, _, ojiT, _, _ = orc.SeedInit(c["ids"], pSG, pSC, np.ascontiguousarray(latT), np.ascontiguousarray(lonT), grid["Yf"], grid["Xf"],
                                            res, c["tmask"], c["sic"][0].astype('f8'))
    trk = orc.Tracker(grid, oSC, ojiT, rec_first=base["z1"], rec_last=base["zL"])
    cells = np.zeros((Nt + 1, nP, 2), dtype=np.int64)
    stepped = np.zeros((Nt + 1, nP), dtype=bool)
    cells[0] = ojiT
    for jt in range(Nt):
        _, mn = trk.step(jt, c["u"][jt].astype('f8'), c["v"][jt].astype('f8'), c["sic"][jt].astype('f8'))
        cells[jt + 1], stepped[jt + 1] = trk.jiT, mn == 1
    assert np.array_equal(trk.jiT, base["jiT"])
    base.update(cells=cells, stepped=stepped, jiT0=np.asarray(ojiT, dtype=np.int64))
    return base


def read_var(fname, name):
    with ncio._Reader(fname) as f:
        a = np.ascontiguousarray(np.asarray(f.var(name)), dtype=np.float32)
        att = {k: f.attr(name, k) for k in ("units", "long_name") if f.has_attr(name, k)}
    return a, att


def check_cli_files(c, ref, out, plain, two_d_time, stride=1):
    Nt, nP = len(c["tc"]), ref["nP"]
    fields = {"siconc": c["sic"].astype('f4'), "sithic": c["sithic"]}
    every = np.ones(nP, dtype=bool)
    assert out["files"] == plain["files"]
    for f in out["files"]:                                   # the position variables: those of a run without --sample, bit for bit
        for name in ("latitude", "longitude", "y_pos", "x_pos", "mask") + (("time_pos",) if two_d_time else ()):
            with ncio._Reader(f) as fa, ncio._Reader(os.path.join("..", "plain", f)) as fb:
                assert np.asarray(fa.var(name)).tobytes() == np.asarray(fb.var(name)).tobytes(), (f, name)
    for name, X in fields.items():
        if not two_d_time:
            f_full, f_12 = out["files"]
            got, att = read_var(f_full, name)
            assert got.shape == (len(range(0, Nt + 1, stride)), nP)
            same_bits(got[0], expect(X[0], ref["jiT0"], every), "%s series row 0" % name)
            for r, k in enumerate(range(0, Nt + 1, stride)):
                if k >= 1:
                    same_bits(got[r], expect(X[k - 1], ref["cells"][k], ref["stepped"][k]), "%s series record %d" % (name, k))
            want0, want1 = expect(X[0], ref["jiT0"], every), expect(X[Nt - 1], ref["cells"][Nt], ref["stepped"][Nt])
        else:
            (f_12,) = out["files"]
            z1, zL = ref["z1"], ref["zL"]
            want0 = X[z1, ref["jiT0"][:, 0], ref["jiT0"][:, 1]]
            want1 = np.full(nP, FILL, dtype=np.float32)
            for b in range(nP):
                if ref["stepped"][zL[b] + 1, b]:
                    want1[b] = X[zL[b], ref["cells"][zL[b] + 1, b, 0], ref["cells"][zL[b] + 1, b, 1]]
        got12, att12 = read_var(f_12, name)
        same_bits(got12[0], want0, "%s tracking12 row 0" % name)
        same_bits(got12[1], want1, "%s tracking12 row 1" % name)
        if name == "sithic":
            assert att12 == {"units": "m", "long_name": "ice thickness"}
        else:
            assert att12 == {}


@pytest.mark.parametrize("two_d_time,extra", [(False, []), (False, ["--out-stride", "4"]), (True, []), (False, ["--full-records"]),
                                              (True, ["--full-records"])])
def test_cli_sample_equals_the_numpy_gather(tmp_path, monkeypatch, two_d_time, extra):
    c = cli_case(tmp_path, two_d_time)
    ref = cli_oracle(c, two_d_time)
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4"] + ([] if two_d_time else ["-F"]) + extra
    (tmp_path / "plain").mkdir(); (tmp_path / "smp").mkdir()
    monkeypatch.chdir(tmp_path / "plain")
    plain = drv.main(argv)
    monkeypatch.chdir(tmp_path / "smp")
    out = drv.main(argv + ["--sample", "siconc,sithic"])
    assert "sample_s" in out["timing"] and "sample_s" not in plain["timing"]
    assert np.array_equal(out["vJIt"], ref["jiT"]) and np.array_equal(out["iAlive"], ref["alive"])
    stride = int(extra[1]) if "--out-stride" in extra else 1
    check_cli_files(c, ref, out, plain, two_d_time, stride)
    for bad, msg in (("nope", "no variable"), ("time_counter", "not a")):
        with pytest.raises(ValueError, match=msg):
            drv.main(argv + ["--sample", bad])


@pytest.mark.parametrize("two_d_time", [False, True])
def test_cli_sample_two_ranks_equals_one(tmp_path, monkeypatch, two_d_time):
    import socket
    import torch.multiprocessing as mp
    from test_driver import _dist_worker
    c = cli_case(tmp_path, two_d_time)
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir(); d2.mkdir()
    argv = ["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4", "--sample", "siconc,sithic"] + ([] if two_d_time else ["-F"])
    monkeypatch.chdir(d1)
    one = drv.main(argv)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_dist_worker, args=(r, 2, port, str(d2), argv + ["--rebalance", "4"], q)) for r in range(2)]
    for p in procs:
        p.start()
    two = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert two["files"] == one["files"] and np.array_equal(two["vJIt"], one["vJIt"])
    for f in one["files"]:
        for name in ("siconc", "sithic", "y_pos", "x_pos", "mask"):
            with ncio._Reader(str(d1 / f)) as fa, ncio._Reader(str(d2 / f)) as fb:
                assert np.asarray(fa.var(name)).tobytes() == np.asarray(fb.var(name)).tobytes(), (f, name)
