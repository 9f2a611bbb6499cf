"""The stages of the command-line driver (sitrack_amd/driver.py) on the CPU, with numpy and fakes: where re-balancing puts
the buoys (rebalance_places), when BoxIngest evaluates the buoys' box and which age it widens it by, and the rows Outputs keeps
for the two-record file and hands to the series writer.  The end-to-end runs against the oracle are tests/test_driver.py."""
from types import SimpleNamespace

import numpy as np
import pytest

from sitrack_amd import _lib
from sitrack_amd import driver as drv
from sitrack_amd.distributed import all_ranges

FILL = drv.FILL


# ---- re-balance placement

def _world_rows(case, world, nP=1000, Nj=17):
    """per rank, the host rows of its buoys in local order"""
    rng = np.random.default_rng(11 * world + len(case))
    owner = rng.integers(0, world, nP)
    rows = rng.integers(0, Nj, nP)
    if case == "empty_rank":
        owner[owner == world - 1] = 0
    elif case == "empty_rows":
        rows[(rows == 0) | (rows == 5) | (rows == Nj - 1)] = 3
    elif case == "one_row":
        rows[:] = 9
    return [rows[owner == r].astype(np.int64) for r in range(world)]


@pytest.mark.parametrize("world,case", [(w, c) for w in (1, 2, 3) for c in ("random", "empty_rows", "one_row")]
                         + [(2, "empty_rank"), (3, "empty_rank")])
def test_rebalance_places_is_the_order_by_row_rank_and_local_order(world, case):
    Nj, per_rank = 17, _world_rows(case, world)
    nP = sum(len(r) for r in per_rank)
    assert nP == 1000 and (case != "empty_rank" or len(per_rank[-1]) == 0)
    allh = np.stack([np.bincount(r, minlength=Nj).astype(np.int64) for r in per_rank])          # what the all-gather hands every rank
    ranges = all_ranges(nP, world)
    placed = [drv.rebalance_places(per_rank[r], allh, r, ranges) for r in range(world)]
    newpos = np.concatenate([p[0] for p in placed])
    dest = np.concatenate([p[1] for p in placed])
    assert np.array_equal(np.sort(newpos), np.arange(nP))                      # every place taken exactly once
    row = np.concatenate(per_rank)
    rank = np.concatenate([np.full(len(r), k) for k, r in enumerate(per_rank)])
    local = np.concatenate([np.arange(len(r)) for r in per_rank])
    assert np.array_equal(np.argsort(newpos), np.lexsort((local, rank, row)))
    want = np.array([next(r for r, (lo, hi) in enumerate(ranges) if lo <= p < hi) for p in newpos])
    assert np.array_equal(dest, want)


# ---- box ageing

class FakeCtx:
    """records what BoxIngest asks of a context; the box rule itself is the real Context.box_of"""
    Nj, Ni, nsub = 600, 700, 2

    def __init__(self, live=(300, 310, 330, 340)):
        self.live, self.evaluations, self.ages, self.staged, self.committed = live, 0, [], [], []

    def buoy_box(self):
        self.evaluations += 1
        return self.live

    def box_of(self, jmin, jmax, imin, imax, age=0, align=4):
        self.ages.append(age)
        return _lib.Context.box_of(self, jmin, jmax, imin, imax, age, align)

    def stage_fill(self, slot, j0, nrows, fill, i0=0, ncols=None):
        self.staged.append((slot, j0, nrows, i0, ncols))
        fill(None, None, None)

    def commit_record_rows(self, slot, j0, j1):
        self.committed.append((slot, j0, j1))


class FakeRecords:
    def __init__(self):
        self.boxes, self.rows = [], []

    def fields_box_into(self, jrec, j0, j1, i0, i1, outs):
        self.boxes.append((jrec, j0, j1, i0, i1))

    def fields_rows_into(self, jrec, j0, j1, outs):
        self.rows.append((jrec, j0, j1))


ONE_RANK = SimpleNamespace(multi=False, root=True, rank=0, world=1)


def _ingest(ctx, records=None, kstrt=3, K=8, **kw):
    return drv.BoxIngest(ctx, records or FakeRecords(), ONE_RANK, drv._Clock(), kstrt, K, ctx.Nj, 4, **kw)


@pytest.mark.parametrize("tinterp", [False, True])
def test_the_box_is_evaluated_when_a_batch_would_pass_its_age_limit(tinterp):
    assert drv.BoxIngest.REEVALUATE_AFTER == 96
    ctx, records = FakeCtx(), FakeRecords()
    ing = _ingest(ctx, records, tinterp=tinterp)
    seen = []
    for jt0, m in ((0, 40), (40, 40), (80, 40)):
        ing.upload(jt0, m)
        seen.append(ctx.evaluations)
    assert seen == [1, 1, 2]                                    # 40 + 40 <= 96, 80 + 40 > 96
    assert ctx.ages == [drv.batch_box_age(0, 40, tinterp), drv.batch_box_age(40, 40, tinterp), drv.batch_box_age(0, 40, tinterp)]
    assert ctx.ages == ([40, 80, 40] if tinterp else [39, 79, 39])
    # every record went into slot jt % K as the box of its batch, read from model record jt + kstrt, and was counted
    assert ing.boxes[0] == ing.boxes[80] == _lib.Context.box_of(ctx, *ctx.live, ctx.ages[0])
    assert ing.boxes[40] == _lib.Context.box_of(ctx, *ctx.live, ctx.ages[1]) and ing.boxes[40] != ing.boxes[0]
    assert len(ctx.staged) == 120 and not ctx.committed
    for jt, st, rd in zip(range(120), ctx.staged, records.boxes):
        j0, j1, i0, i1 = ing.boxes[jt - jt % 40]
        assert st == (jt % 8, j0, j1 - j0, i0, i1 - i0) and rd == (jt + 3, j0, j1, i0, i1)
    assert ing.bytes == sum(3 * (b[1] - b[0]) * (b[3] - b[2]) * 4 for b in ing.boxes.values()) * 40 > 0


def test_a_plan_in_front_of_the_launch_restarts_the_age_at_the_records_not_queued():
    ctx = FakeCtx()
    ing = _ingest(ctx, tinterp=True)
    ing.plan(4, 3, not_queued=4)                # the batch of 4 records in front of it has not been given to the GPU
    ing.plan(7, 2)
    assert ctx.evaluations == 1 and ctx.ages == [drv.batch_box_age(4, 3, True), drv.batch_box_age(7, 2, True)] == [7, 9]
    assert not ctx.staged                       # plan() reads nothing


def test_reset_forces_an_evaluation_at_the_next_batch():
    ctx = FakeCtx()
    ing = _ingest(ctx)
    ing.upload(0, 2)
    ing.upload(2, 2)
    assert ctx.evaluations == 1
    ing.reset()
    ing.upload(4, 2)
    assert ctx.evaluations == 2 and ctx.ages == [1, 3, 1]


def test_no_live_buoy_commits_empty_slots_and_reads_nothing():
    ctx, records = FakeCtx(live=(5, 4, 9, 8)), FakeRecords()               # jmin > jmax
    ing = _ingest(ctx, records)
    ing.upload(6, 3)
    assert ing.boxes[6] == (0, 0, 0, 0)
    assert ctx.committed == [(6, 0, 0), (7, 0, 0), (0, 0, 0)] and not ctx.staged and not records.boxes
    assert ing.bytes == 0


def test_full_records_never_ask_for_the_box():
    ctx, records = FakeCtx(), FakeRecords()
    ing = _ingest(ctx, records, full_records=True)
    ing.upload(0, 40)
    ing.upload(40, 60)
    assert ctx.evaluations == 0 and not ctx.ages and ing.boxes == {} and ing.boxes.get(40) is None
    assert ctx.staged == [(jt % 8, 0, ctx.Nj, 0, None) for jt in range(100)]
    assert records.rows == [(jt + 3, 0, ctx.Nj) for jt in range(100)] and ing.bytes == 0


# ---- output rows

class GeoCtx:
    """cart2geo stand-in: any map that tells converted rows from unconverted ones"""

    @staticmethod
    def cart2geo(yx):
        return 0.5 * np.asarray(yx) + 7.


class Stream:
    """recording stand-in for ncio.CloudBuoysStream; put() of series index `fail_at` raises"""
    made = []

    def __init__(self, fname, vtime, ids, with_mask=False, corigin=None, extra_names=None):
        self.fname, self.vtime, self.puts, self.aborts, self.closed, self.fail_at = fname, np.array(vtime), [], 0, 0, None
        Stream.made.append(self)

    def put(self, k, y, x, lat, lon, msk, extra=None):
        if k == self.fail_at:
            raise OSError("disk full")
        self.puts.append((k, np.stack([y, x], axis=1), np.stack([lat, lon], axis=1), np.array(msk)))

    def abort(self):
        self.aborts += 1

    def close(self):
        self.closed += 1


def _case(two_d_time, Nt, kstrt=2, nP=10):
    rng = np.random.default_rng(3)
    tm = 850608000 + 1800 + 3600 * np.arange(kstrt + Nt + 1)
    run = SimpleNamespace(lUse2DTime=two_d_time, Nt=Nt, kstrt=kstrt, kstop=kstrt + Nt - 1, rdt=3600., ztime_model=tm, corgn="NEMO-SI3_C_E",
                          SeedBatch="B", cdtbin="_dt72", csfkm="_10km")
    seeds = SimpleNamespace(nP=nP, IDs=100 + np.arange(nP), xPosC0=rng.uniform(-500., 500., (nP, 2)), xPosG0=rng.uniform(60., 80., (nP, 2)))
    records = SimpleNamespace(time=lambda jrec: int(tm[jrec]))
    return run, seeds, records


@pytest.fixture
def saved(monkeypatch):
    """what ncio.ncSaveCloudBuoys is called with; the stream writer is the recording stand-in"""
    calls = []
    monkeypatch.setattr(drv.ncio, "ncSaveCloudBuoys", lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(drv.ncio, "CloudBuoysStream", Stream)
    Stream.made = []
    return calls


def test_two_d_time_keeps_every_buoys_first_and_last_row(saved):
    Nt, kstrt, nP = 6, 2, 10
    run, seeds, records = _case(True, Nt)
    z1st = np.full(nP, kstrt)
    zLst = np.array([7, 7, 4, 6, 7, 4, 6, 7, 7, 6])
    z1st[3] = 4                                                 # a window that opens late
    dead = 5
    out = drv.Outputs(run, seeds, z1st, zLst, records, GeoCtx, stride=4)
    assert out.ends == {4, 6, 7} and out.stride == 1 and not Stream.made
    assert [j for j in range(kstrt, kstrt + Nt) if out.need(j)] == [4, 6, 7]
    rng = np.random.default_rng(4)
    fed = {}
    for jrec in (4, 6, 7):
        pos, msk = rng.uniform(-500., 500., (nP, 2)), np.ones(nP, dtype='i1')
        pos[dead], msk[dead] = FILL, 0
        fed[jrec] = (pos, msk)
        out.store(jrec, pos, msk)
    outs, zvt = out.write()

    # the driver's bookkeeping, restated
    vTime = np.array([run.ztime_model[kstrt + j] - 1800 for j in range(Nt)])
    e2XY, e2GC = np.zeros((2, nP, 2)) + FILL, np.zeros((2, nP, 2)) + FILL
    eMSK, eTim = np.zeros((2, nP), dtype='i1'), np.zeros((2, nP), dtype=int) + int(FILL)
    e2XY[0], e2GC[0], eMSK[0] = seeds.xPosC0, seeds.xPosG0, 1
    eTim[0] = run.ztime_model[z1st] - 1800
    late = z1st - kstrt > 0
    e2GC[0, late] = GeoCtx.cart2geo(seeds.xPosC0[late])
    for jrec, (pos, msk) in fed.items():
        sel = np.where(zLst == jrec)[0]
        e2XY[1, sel], e2GC[1, sel], eMSK[1, sel] = pos[sel], GeoCtx.cart2geo(pos[sel]), msk[sel]
        eTim[1, sel[msk[sel] == 1]] = int(vTime[jrec - kstrt] + 3600.)
    assert np.array_equal(out.z2XY, e2XY) and np.array_equal(out.z2GC, e2GC)
    assert np.array_equal(out.zMSK, eMSK) and np.array_equal(out.zTim, eTim)
    # ... and by hand: the late seed is converted, the others are as the seeding file gave them; the dead buoy did not step
    assert np.array_equal(out.z2GC[0, 3], 0.5 * seeds.xPosC0[3] + 7.) and np.array_equal(out.z2GC[0, 0], seeds.xPosG0[0])
    assert out.zTim[0, 3] == run.ztime_model[4] - 1800 and out.zTim[0, 0] == run.ztime_model[2] - 1800
    assert out.zTim[1, dead] == int(FILL) and out.zMSK[1, dead] == 0 and out.zTim[1, 2] == run.ztime_model[4] + 1800
    assert out.zTim[1, 0] == run.ztime_model[7] + 1800
    # what is written: one file, named after the mean first and last times, the four rows and the times
    (args, kw), = saved
    assert np.array_equal(zvt, [eTim[0].mean(), eTim[1].mean()]) and np.array_equal(args[1], zvt)
    assert outs == [args[0]] == ['./nc/NEMO-SI3_C_E_tracking12_B_dt72_%s_%s_10km.nc' % (drv.date_tag(zvt[0]), drv.date_tag(zvt[1]))]
    assert np.array_equal(args[2], seeds.IDs)
    for got, want in zip(args[3:7], (e2XY[:, :, 0], e2XY[:, :, 1], e2GC[:, :, 0], e2GC[:, :, 1])):
        assert np.array_equal(got, want)
    assert np.array_equal(kw["mask"], eMSK) and np.array_equal(kw["xtime"], eTim) and kw["extra"] is None


def _feed_series(out, run, nP):
    fed = {}
    rng = np.random.default_rng(6)
    for jrec in range(run.kstrt, run.kstrt + run.Nt):
        if out.need(jrec):
            fed[jrec] = (rng.uniform(-500., 500., (nP, 2)), np.ones(nP, dtype='i1'), rng.uniform(60., 80., (nP, 2)))
            out.store(jrec, *fed[jrec])
    return fed


def test_fixed_time_streams_every_stride_th_record_and_keeps_the_last(saved):
    Nt, kstrt, nP = 7, 2, 10
    run, seeds, records = _case(False, Nt)
    z = np.full(nP, kstrt)
    out = drv.Outputs(run, seeds, z, z + Nt - 1, records, GeoCtx, stride=3)
    (series,) = Stream.made
    vTime = np.array([run.ztime_model[kstrt + j] - 1800 for j in range(Nt)] + [run.ztime_model[kstrt + Nt - 1] + 1800])
    assert np.array_equal(out.vTime, vTime) and np.array_equal(series.vtime, vTime[[0, 3, 6]]) and out.ends == ()
    assert series.fname == './nc/NEMO-SI3_C_E_tracking_B_dt72_%s_%s_10km_stride3.nc' % (drv.date_tag(vTime[0]), drv.date_tag(vTime[7]))
    fed = _feed_series(out, run, nP)
    assert sorted(fed) == [kstrt + 2, kstrt + 5, kstrt + 6]                 # k = 3, 6 and Nt = 7
    assert [p[0] for p in series.puts] == [0, 1, 2]
    assert np.array_equal(series.puts[0][1], seeds.xPosC0) and np.array_equal(series.puts[0][2], seeds.xPosG0)
    for (k, pos, ll, msk), jrec in zip(series.puts[1:], (kstrt + 2, kstrt + 5)):
        assert np.array_equal(pos, fed[jrec][0]) and np.array_equal(ll, fed[jrec][2]) and np.array_equal(msk, fed[jrec][1])
    outs, zvt = out.write()
    (args, kw), = saved
    assert series.closed == 1 and series.aborts == 0 and outs == [series.fname, args[0]]
    assert np.array_equal(zvt, [vTime[0], vTime[7]]) and len(kw["xtime"]) == 0
    last = fed[kstrt + 6]
    assert np.array_equal(args[3][0], seeds.xPosC0[:, 0]) and np.array_equal(args[5][0], seeds.xPosG0[:, 0])
    assert np.array_equal(args[3][1], last[0][:, 0]) and np.array_equal(args[4][1], last[0][:, 1])
    assert np.array_equal(args[5][1], last[2][:, 0]) and np.array_equal(args[6][1], last[2][:, 1])
    assert np.array_equal(kw["mask"], np.ones((2, nP), dtype='i1'))


def test_a_failing_put_aborts_the_series_once_and_propagates(saved):
    Nt, kstrt, nP = 7, 2, 10
    run, seeds, records = _case(False, Nt)
    z = np.full(nP, kstrt)
    out = drv.Outputs(run, seeds, z, z + Nt - 1, records, GeoCtx, stride=3)
    (series,) = Stream.made
    series.fail_at = 1
    with pytest.raises(OSError, match="disk full"):
        _feed_series(out, run, nP)
    assert series.aborts == 1 and [p[0] for p in series.puts] == [0] and series.closed == 0 and not saved
