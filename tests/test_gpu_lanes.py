"""Two staggered buoy lanes in sitrk_run (knobs "lanes", "lane_min_wg") on the MI355X: lanes = 2, forced on small sets, equals
lanes = 1 and the oracle bit for bit in yx, jiT, alive and kill_rec, and counts the same launches (sitrk_launch_stats stays
logical; sitrk_lane_stats shows that the lanes were really used)."""
import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import synthetic as syn
from test_substep import oracle_replay

pytestmark = pytest.mark.gpu
K = 6                                   # records and slots
UNIT = 256 * 8                          # lane cut unit with xcd_group = 1
_CASE = {}


def case(nP=5003):
    """90 x 100 warped mesh, low-concentration patches in its lower and its upper rows (kills at both ends of the sorted order)
    and a land patch; nP buoys, not a multiple of 256: cut = 4096, lane 1 keeps 907 buoys (3.5 workgroups)"""
    if nP not in _CASE:
        grid = syn.make_grid(90, 100, dkm=4.0, warp=1.0)
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
        assert found.sum() >= nP and nP % 256 != 0
        _CASE[nP] = (grid, u, v, sic, np.ascontiguousarray(yx[found][:nP]), ji[found][:nP].astype(np.int64))
    return _CASE[nP]


def cut_of(nP):
    return ((nP + UNIT - 1) // UNIT + 1) // 2 * UNIT


def gpu_run(lanes, nrec, fuse=2, dtype=np.float32, nsub=1, sort=True, resort=0, windows=(None, None), tune=None, stream=None, nP=5003,
            chunks=None):
    grid, u, v, sic, yx, ji = case(nP)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=3600. * nsub,
                         nslots=K, field_dtype=dtype, nsub=nsub)
    ctx = trk.ctx
    ctx.set_tuning(lanes=lanes, lane_min_wg=1, xcd_group=1, fuse=fuse, **(tune or {}))
    if stream is not None:
        ctx.set_stream(stream.cuda_stream)
    for k in range(K):
        trk.load_record(k, u[k].astype(dtype), v[k].astype(dtype), sic[k].astype(dtype))
    trk.set_buoys(yx, ji, windows[0], windows[1], sort=sort)
    ctx.set_resort(resort)
    ctx.launch_stats(reset=True)
    done = 0
    for n in (chunks or [nrec]):
        ctx.run(done % K, done, n)
        done += n
    assert done == nrec
    out = ctx.fetch()                   # right behind run: no explicit sync
    st, ln = ctx.launch_stats(), ctx.lane_stats()
    trk.close()
    return out, st, ln


def oracle(nrec, dtype=np.float32, nsub=1, windows=(None, None), nP=5003, fields=None):
    grid, u, v, sic, yx, ji = case(nP)
    u, v, sic = fields or (u, v, sic)
    rf = np.zeros(nP, dtype=np.int64) if windows[0] is None else windows[0]
    rl = np.full(nP, nrec - 1, dtype=np.int64) if windows[1] is None else windows[1]
    r = oracle_replay(grid, yx, ji, *(a.astype(dtype).astype(np.float64) for a in (u, v, sic)), rf, rl, 0, nrec, 3600. * nsub, nsub, 1)
    return {"yx": r["final"], "jiT": r["jiT"][-1], "alive": r["alive"][-1], "kill_rec": r["kill_rec"]}


def same(a, b):
    return (np.array_equal(np.ascontiguousarray(a["yx"]).view(np.uint64), np.ascontiguousarray(b["yx"], dtype=np.float64).view(np.uint64))
            and np.array_equal(a["jiT"], b["jiT"]) and np.array_equal(a["alive"], b["alive"]) and np.array_equal(a["kill_rec"], b["kill_rec"]))


def check(nrec, segments, **kw):
    """lanes = 2 == lanes = 1 == oracle, same launch_stats; lanes = 2 really ran `segments` segments on two lanes"""
    okw = {k: kw[k] for k in ("dtype", "nsub", "windows", "nP") if k in kw}
    one, st1, ln1 = gpu_run(1, nrec, **kw)
    two, st2, ln2 = gpu_run(2, nrec, **kw)
    ref = oracle(nrec, **okw)
    assert same(one, ref), "lanes=1 differs from the oracle"
    assert same(two, ref), "lanes=2 differs from the oracle"
    assert same(two, one)
    assert st1 == st2, (st1, st2)
    assert ln1 == {"lane_segments": 0, "lane_launches": 0}
    assert ln2["lane_segments"] == segments, ln2
    assert 0 < ref["alive"].sum() < len(ref["alive"])
    return two, st2, ln2


def test_sorted_set_short_lane_1():
    """nP = 5003: not a multiple of 256, the cut at 4096 leaves lane 1 with 907 buoys.  20 records at 2 per launch: lane 0 queues
    10 launches, lane 1 one of 1 record, 9 of 2 and a last one of 1"""
    two, st, ln = check(20, 1)
    assert st == {"fused_launches": 10, "fused_records": 20, "step_launches": 0}
    assert ln["lane_launches"] == 10 + 11


def test_fuse_4_and_a_lone_last_record():
    """21 records at 4 per launch: the one-lane path steps the last record with the one-record kernel and counts it so; on lanes
    it is a one-record fused launch, counted the same"""
    two, st, ln = check(21, 1, fuse=4)
    assert st == {"fused_launches": 5, "fused_records": 20, "step_launches": 1}
    assert ln["lane_launches"] == 6 + 6              # lane 0: 4 4 4 4 4 1, lane 1: 2 4 4 4 4 3


def test_unsorted_set_kills_in_both_lanes():
    nP = 5003
    two, st, ln = check(20, 1, sort=False)
    c = cut_of(nP)
    assert c == 4096
    assert (two["kill_rec"][:c] >= 0).any() and (two["kill_rec"][c:] >= 0).any()


def test_row_major_sort_kills_in_both_lanes():
    """row-major cell order: lane 1 holds the buoys of the uppermost rows"""
    nP = 5003
    grid, u, v, sic, yx, ji = case(nP)
    two, st, ln = check(20, 1, tune={"sort_tile": 0})
    key = np.sort(ji[:, 0] * grid["Ni"] + ji[:, 1])
    c = cut_of(nP)
    mykey = ji[:, 0] * grid["Ni"] + ji[:, 1]
    lane0, lane1 = mykey < key[c - 1], mykey > key[c]          # (buoys of the cell at the cut may be in either)
    assert lane0.sum() > 3000 and lane1.sum() > 500
    assert (two["kill_rec"][lane0] >= 0).any() and (two["kill_rec"][lane1] >= 0).any()


def test_per_buoy_windows_both_kernel_forms():
    """windows [0 or 3, 19 or 15]: launches inside records 3..15 take the form without the window test, the others the one with it;
    the two lanes' launches cover different records, so they choose differently for the same record"""
    nP = 5003
    rng = np.random.default_rng(7)
    rf = np.where(rng.random(nP) < 0.2, 3, 0).astype(np.int64)
    rl = np.where(rng.random(nP) < 0.2, 15, 19).astype(np.int64)
    check(20, 1, windows=(rf, rl))


def test_resort_boundary_inside_a_run():
    """re-sort every 7 records, 30 records: segments of 7 7 7 7 (two lanes each, a join, the re-sort, a fork) and 2 (one lane)"""
    two, st, ln = check(30, 4, resort=7)
    assert st["fused_records"] + st["step_launches"] == 30


def test_two_runs_and_a_short_one():
    """runs of 12 (two lanes), 3 (below 2.5 launches: one lane) and 9 records"""
    two, st, ln = check(24, 2, chunks=[12, 3, 9])


def test_substeps():
    check(12, 1, nsub=3)


def test_fp64_records():
    check(20, 1, dtype=np.float64)


def test_external_stream():
    import torch
    s = torch.cuda.Stream()
    check(20, 1, stream=s)
    s.synchronize()


def test_threshold_keeps_one_lane():
    """the default lane_min_wg keeps small sets on one lane, and so does a run of fewer than 2.5 launches"""
    grid, u, v, sic, yx, ji = case()
    for tune, nrec in (({"lanes": 2, "xcd_group": 1}, 20), ({"lanes": 2, "xcd_group": 1, "lane_min_wg": 1, "fuse": 6}, 14)):
        trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], nslots=K)
        trk.ctx.set_tuning(**tune)
        for k in range(K):
            trk.load_record(k, u[k], v[k], sic[k])
        trk.set_buoys(yx, ji)
        trk.ctx.run(0, 0, nrec)
        assert trk.ctx.lane_stats() == {"lane_segments": 0, "lane_launches": 0}
        trk.close()
    with pytest.raises(_lib.SitrkError):
        _lib.Context(0).set_tuning(lanes=3)
    with pytest.raises(_lib.SitrkError):
        _lib.Context(0).set_tuning(lane_min_wg=0)


@pytest.mark.parametrize("lanes", [1, 2])
def test_fetch_box_and_commit_right_behind_run(lanes):
    """no explicit sync anywhere: fetch, buoy_box_begin, an upload into every slot the lanes have just read, and
    commit_records_box of a box of them follow a run at once; then 12 more records with the new fields"""
    nP = 5003
    grid, u, v, sic, yx, ji = case(nP)
    uB, vB, sicB = u[::-1].copy(), v[::-1].copy(), sic[::-1].copy()
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], nslots=K)
    ctx = trk.ctx
    ctx.set_tuning(lanes=lanes, lane_min_wg=1, xcd_group=1, fuse=2)
    for k in range(K):
        trk.load_record(k, u[k], v[k], sic[k])
    trk.set_buoys(yx, ji)
    ctx.set_resort(0)
    ctx.run(0, 0, 12)
    a = ctx.fetch()
    assert same(a, oracle(12))
    ctx.run(0, 12, 12)
    ctx.buoy_box_begin()
    for k in range(K):
        trk.load_record(k, uB[k], vB[k], sicB[k])
    jmin, jmax, imin, imax, age = ctx.buoy_box_end()
    assert age == 0
    ref24 = oracle(24)
    live = ref24["alive"] == 1
    assert (jmin, jmax, imin, imax) == (ref24["jiT"][live, 0].min(), ref24["jiT"][live, 0].max(),
                                        ref24["jiT"][live, 1].min(), ref24["jiT"][live, 1].max())
    j0, j1, i0, i1 = ctx.box_of(jmin, jmax, imin, imax, age=11)
    ctx.commit_records_box(0, K, j0, j1, i0, i1)
    ctx.run(0, 24, 12)
    b = ctx.fetch()
    seq = tuple(np.concatenate([x, x, x, x, y, y]) for x, y in ((u, uB), (v, vB), (sic, sicB)))               # K = 36 records in order
    assert same(b, oracle(36, fields=seq))
    assert ctx.lane_stats()["lane_segments"] == (3 if lanes == 2 else 0)
    trk.close()
