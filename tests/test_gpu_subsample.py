"""Seed-cloud coarsening on the GPU (sitrk_subsample_cloud, SubSampCloud, generate_idealized_seeding.py -C) against the
test-side statements of the contract in test_subsample.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

import sitrack_amd as sit
from sitrack_amd import driver as drv
from sitrack_amd import ncio
from sitrack_amd import synthetic as syn

from test_subsample import greedy_reference, characterisation_violations, hand_cases, fma_case, d2
from test_cloud_trips import NP_TRIP, TRIP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = sit.Context(0)
    yield c
    c.close()


def mesh_seeds(ctx, N, dkm):
    """T+F seeds of an N x N polar mesh in the library's order (sitrk_nemo_seed: T in C order, then F): (n,2) [y,x] km"""
    g = syn.make_grid(N, N, dkm=dkm, warp=0.5)
    llT = ctx.cart2geo(np.stack([g["Yt"].ravel(), g["Xt"].ravel()], axis=1))
    llF = ctx.cart2geo(np.stack([g["Yf"].ravel(), g["Xf"].ravel()], axis=1))
    latT, lonT = llT[:, 0].reshape(N, N).copy(), np.mod(llT[:, 1], 360.).reshape(N, N).copy()
    latF, lonF = llF[:, 0].reshape(N, N).copy(), np.mod(llF[:, 1], 360.).reshape(N, N).copy()
    _, yx, nT, nF = ctx.nemo_seed(np.ones((N, N), np.int8), latT, lonT, np.ones((N, N)), latF=latF, lonF=lonF)
    assert nF > 0
    return yx


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_cases(ctx, case):
    _, yx, rd, want = case
    yx = np.asarray(yx, dtype=np.float64).reshape(-1, 2)
    keep, nl = ctx.subsample_cloud(yx, rd)
    assert np.array_equal(keep, np.asarray(want, dtype=bool))
    assert nl >= (1 if len(yx) else 0)


def test_fma_sensitive_pair(ctx):
    yx, want = fma_case()
    keep, _ = ctx.subsample_cloud(yx, 6.0)
    assert np.array_equal(keep, want)


@pytest.mark.parametrize("seed,rd", [(1, 0.9), (2, 2.5), (3, 6.0)])
def test_random_clouds_random_order_equal_the_sequential_greedy(ctx, seed, rd):
    rng = np.random.default_rng(seed)
    n = 20000
    yx = rng.uniform(-80., 80., (n, 2))
    yx[::13] = yx[::13].round(1)                  # shared coordinates and duplicates
    yx = yx[rng.permutation(n)]
    keep, _ = ctx.subsample_cloud(yx, rd)
    assert np.array_equal(keep, greedy_reference(yx, rd))


@pytest.fixture(scope="module")
def mesh1m(ctx):
    return mesh_seeds(ctx, 708, 4.0)             # ~1.0e6 T+F seeds, C-ordered


@pytest.mark.parametrize("rd", [6.0, 34.5])
def test_mesh_seeds_characterisation_and_launch_shape(ctx, mesh1m, rd):
    yx = mesh1m
    assert len(yx) > 900_000
    keep, nl = ctx.subsample_cloud(yx, rd)
    assert 0 < keep.sum() < len(yx)
    assert characterisation_violations(yx, rd, keep) == 0
    again, _ = ctx.subsample_cloud(yx, rd)
    assert np.array_equal(again, keep)
    try:
        for blk in (256, 4096):
            ctx.set_tuning(subsample_block=blk)
            other, _ = ctx.subsample_cloud(yx, rd)
            assert np.array_equal(other, keep), "subsample_block=%d" % blk
    finally:
        ctx.set_tuning(subsample_block=1024)


def test_bad_arguments_return_einval(ctx):
    L, h = ctx._L, ctx._h
    yx = np.zeros((5, 2))
    yx[3, 1] = np.nan
    keep = np.zeros(5, np.int8)
    nk = C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    assert L.sitrk_subsample_cloud(h, 5, p(yx), 1.0, p(keep), C.byref(nk), None) == -1
    assert b"index 3" in L.sitrk_last_error(h)
    yx[3, 1] = np.inf
    assert L.sitrk_subsample_cloud(h, 5, p(yx), 1.0, p(keep), C.byref(nk), None) == -1
    yx[3, 1] = 0.
    for rd in (0.0, -2.0, float("nan"), float("inf")):
        assert L.sitrk_subsample_cloud(h, 5, p(yx), rd, p(keep), C.byref(nk), None) == -1
    assert L.sitrk_subsample_cloud(h, 5, None, 1.0, p(keep), C.byref(nk), None) == -1
    assert L.sitrk_subsample_cloud(h, 5, p(yx), 1.0, None, C.byref(nk), None) == -1
    assert L.sitrk_subsample_cloud(h, 5, p(yx), 1.0, p(keep), None, None) == -1
    assert L.sitrk_subsample_cloud(h, 0, None, 1.0, None, C.byref(nk), None) == 0 and nk.value == 0
    assert L.sitrk_subsample_cloud(h, 5, p(yx), 1.0, p(keep), C.byref(nk), None) == 0 and nk.value == 1       # five duplicates
    with pytest.raises(sit.SitrkError):
        ctx.set_tuning(subsample_block=300)


def test_einval_names_the_first_index_of_the_second_trip(ctx):
    """the first bad index lies past one trip of bbox_kernel's capped grid"""
    yx = np.random.default_rng(5).uniform(-300., 300., (NP_TRIP, 2))
    _, small, rd, want = hand_cases()[-1]
    yx[TRIP + 3, 0] = np.nan
    yx[TRIP + 700, 1] = np.nan
    with pytest.raises(sit.SitrkError, match="non-finite coordinate at index %d$" % (TRIP + 3)):
        ctx.subsample_cloud(yx, 3.0)
    assert np.array_equal(ctx.subsample_cloud(np.array(small), rd)[0], np.array(want, dtype=bool))
    yx[TRIP + 3, 0] = 0.                          # there is no validity mask: mended, the next one is named
    with pytest.raises(sit.SitrkError, match="non-finite coordinate at index %d$" % (TRIP + 700)):
        ctx.subsample_cloud(yx, 3.0)
    yx[TRIP + 3, 0] = np.nan
    yx[9, 1] = np.inf                             # an earlier one, in the first trip
    with pytest.raises(sit.SitrkError, match="non-finite coordinate at index 9$"):
        ctx.subsample_cloud(yx, 3.0)
    assert np.array_equal(ctx.subsample_cloud(np.array(small), rd)[0], np.array(want, dtype=bool))


def test_tracker_state_is_untouched_by_a_coarsening_on_the_same_handle():
    g = syn.make_grid(64, 64, dkm=4.0, warp=1.0)
    u, v, sic = syn.make_fields(g, K=4, seed=2024, umax=0.75, drift=0.25, ripple=0.12)
    _, yx = syn.make_buoys(g, 2000, seed=1234, frac=0.7)
    cloud = np.random.default_rng(9).uniform(-500., 500., (300_000, 2))     # larger than anything the tracker staged
    runs = []
    for with_cloud in (False, True):
        trk = sit.IceTracker(g["Yf"], g["Xf"], g["Yu"], g["Xu"], g["Yv"], g["Xv"], g["tmask"], nslots=4)
        found, ji, _ = sit.FindContainingCell(yx, syn.nearest_t_plane(g, yx), ctx=trk.ctx)
        trk.set_buoys(yx[found], ji[found])
        for k in range(4):
            trk.load_record(k, u[k], v[k], sic[k])
        trk.run(0, 0, 4)
        if with_cloud:
            trk.ctx.subsample_cloud(cloud, 3.0)
        trk.run(4, 0, 4)
        st = trk.state()
        rec = trk.record(7)
        runs.append((st, rec))
        trk.ctx.close()
    (a, ra), (b, rb) = runs
    for k in ("yx", "vJIt", "iAlive"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])


def test_subsampcloud_returns_true_indices(ctx):
    # p1 is dropped (within 2 km of p0); p2 is kept and shares its y with p1: the reference's np.where(pCoor == zCoor[i])
    # lookup (util.py:365-368) would name p1
    p = np.array([[0., 0.], [1., 0.], [1., 5.], [9., 9.]])
    Nb, zCoor, idx = sit.SubSampCloud(2.0, p, ctx=ctx)
    assert Nb == 3 and list(idx) == [0, 2, 3]
    assert np.array_equal(zCoor, p[idx])
    ref_idx = [np.where(p[:, :] == zCoor[i, :])[0][0] for i in range(Nb)]
    assert ref_idx == [0, 1, 3] and ref_idx != list(idx)


def _gis():
    spec = importlib.util.spec_from_file_location("gis_gpu", os.path.join(ROOT, "tools", "generate_idealized_seeding.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _mesh_mask_with_fmask(c, path):
    """make_case's mesh_mask plus `fmask` (GetModelGrid(alsoF=True) reads it)"""
    from test_driver import _write_nc3
    Nj, Ni = c["tmask"].shape
    dkm = c["dkm"]
    var = {"tmask": ('i1', ('t', 'z', 'y', 'x'), c["tmask"][None, None], None),
           "fmask": ('i1', ('t', 'z', 'y', 'x'), np.ones((1, 1, Nj, Ni), np.int8), None),
           "e1t": ('f8', ('t', 'y', 'x'), np.full((1, Nj, Ni), dkm * 1000.), None),
           "e2t": ('f8', ('t', 'y', 'x'), np.full((1, Nj, Ni), dkm * 1000.), None)}
    for q in "tufv":
        var["glam" + q] = ('f8', ('t', 'y', 'x'), c["ll"][q][:, 1].reshape(1, Nj, Ni), None)
        var["gphi" + q] = ('f8', ('t', 'y', 'x'), c["ll"][q][:, 0].reshape(1, Nj, Ni), None)
    _write_nc3(path, {"t": 1, "z": 1, "y": Nj, "x": Ni}, var)
    return path


def test_seeding_tool_C10_end_to_end(tmp_path, monkeypatch):
    from test_driver import make_case
    monkeypatch.chdir(tmp_path)
    c = make_case(str(tmp_path), dkm=4.0)
    mm = _mesh_mask_with_fmask(c, str(tmp_path / "mesh_mask_TEST4F.nc"))
    gis = _gis()
    base = ["-d", "1996-12-15_00:00:00", "-m", mm, "-i", c["si3"], "-k", "0", "-N", "TEST4"]
    f = gis.main(base + ["-C", "10"])
    assert f == './nc/sitrack_seeding_nemoTsi3_19961215_00_10km.nc'
    # the un-coarsened T+F cloud of the same inputs, written by the same writer
    ctx = sit.default_context()
    imaskt, latT, lonT, _, _, _, _, _, _, latF, lonF = ncio.GetModelGrid(mm, alsoF=True)
    rec = ncio.ModelRecords(c["si3"])
    (ic,) = rec.fields(0, ("siconc",))
    rec.close()
    gc_all, yx_all = sit.seeding.nemoSeed(imaskt, latT, lonT, ic, platF=latF, plonF=lonF, ctx=ctx, return_yx=True)
    ids_all = np.arange(1, len(gc_all) + 1)
    fall = './nc/all.nc'
    ncio.ncSaveCloudBuoys(fall, np.array([c["base"]], dtype='i4'), ids_all, yx_all[None, :, 0], yx_all[None, :, 1],
                          gc_all[None, :, 0], gc_all[None, :, 1], corigin='idealized_seeding', cauthor='test')
    _, ids, ll, yx = ncio.LoadNCdata(f, krec=0)
    _, ids0, ll0, yx0 = ncio.LoadNCdata(fall, krec=0)
    ids = np.asarray(ids).astype(np.int64)
    assert 10 < len(ids) < len(ids0)
    assert np.all(np.diff(ids) > 0) and np.isin(ids, ids0).all()
    assert np.array_equal(ll, ll0[ids - 1]) and np.array_equal(yx, yx0[ids - 1])
    # no two seeds closer than rd_ss = 6 km (fp64 positions of the kept rows)
    kept = yx_all[ids - 1]
    pairs = cKDTree(kept).query_pairs(6.0 * (1 + 1e-9), output_type='ndarray')
    assert len(pairs) == 0 or np.all(d2(kept[pairs[:, 0]], kept[pairs[:, 1]]) >= 36.0)
    # the tracker reads it and tags its outputs with the spacing
    out = drv.main(["-i", c["si3"], "-m", c["mm"], "-s", f, "-N", "TEST4", "-F", "-e", "1996-12-15_06:00:00"])
    assert out["nP"] > 0 and out["files"][0].endswith('_10km.nc')
