"""The stage before the first step at the sizes where its loops take a second trip: `sitrk_nemo_seed` across blocks and scan
chunks (one chunk = 1024 blocks of 1024 points), the seed search beyond 64 superblocks (a wavefront looks at 64 superblock
spheres per round), and the compaction of `sitrk_tri2quad` across a scan chunk.  References: numpy for the seeding, the CPU
oracle for the search, the round form of tests/test_tri2quad.py for the quadrangles.  The assertions on the inputs and the G10
self-check of the numpy helper need no GPU."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import synthetic as syn
from oracle import oracle as orc
from test_deform import jittered_lattice
from test_tri2quad import tri2quad_rounds

SEED_BLOCK = 1024                 # points per block of the seeding kernels
SCAN_CHUNK = 1024                 # blocks per trip of the one-workgroup scan
SB_POINTS = 256                   # mesh points per superblock edge of the seed search (16 blocks of 16)
SB_ROUND = 64                     # superblocks per round of a wavefront


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    """equal bit for bit, a NaN equal to a NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------- 1. sitrk_nemo_seed
def nemo_seed_ref(tmask, lat, lon, sic, khss=1, rmask=None, latF=None, lonF=None):
    """numpy restatement of nemoSeed (the lines of tests/test_abi.py::test_nemoseed_matches_reference_golden):
    (T-seeds (nT,2), F-seeds (nF,2), T flags, F flags of the sub-sampled mesh)."""
    s = (slice(None, None, khss), slice(None, None, khss))
    m = tmask[s].astype('i1')
    if rmask is not None:
        m = (m * rmask[s]).astype('i1')
    with np.errstate(invalid='ignore'):
        m[lat[s] < 55.] = 0
        m[sic[s] < 0.9] = 0
    wantT = np.stack([lat[s][m == 1], lon[s][m == 1]], axis=1)
    mf = np.zeros_like(m)
    if latF is not None:
        mf[1:-1, 1:-1] = (m[2:, 1:-1] + m[1:-1, 2:] + m[:-2, 1:-1] + m[1:-1, :-2]) / 4
        wantF = np.stack([latF[s][mf == 1], lonF[s][mf == 1]], axis=1)
    else:
        wantF = np.zeros((0, 2))
    return wantT, wantF, m == 1, mf == 1


def test_numpy_helper_reproduces_the_g10_golden(golden):
    g = golden("g10_nemoseed.npz")
    cases = {"a": dict(khss=1), "b": dict(khss=3), "c": dict(khss=2, rmask=g["rmask"]),
             "d": dict(khss=1, latF=g["latF"], lonF=g["lonF"]),
             "e": dict(khss=4, rmask=g["rmask"], latF=g["latF"], lonF=g["lonF"])}
    for tag, kw in cases.items():
        wantT, wantF, _, _ = nemo_seed_ref(g["tmask"], g["lat"], g["lon"], g["sic"], **kw)
        assert same_bits(np.concatenate([wantT, wantF]), g["seed_" + tag]), tag
        assert len(wantT) > 0 and (len(wantF) > 0 or "latF" not in kw or tag == "e")      # (10 x 11 points: no F-seed in the golden)


# rows of the model mesh that are emptied (tmask 0) / filled (every point seeds): around the rows where the chunk boundaries of
# the block sequence fall, plus some elsewhere
SEED_CASES = {
    # 1024 x 1024: T-block b is row b, block 1024 (chunk 1) is F-row 0.  The last T-rows are empty and so are the first F-rows.
    "one_chunk_of_T": dict(shape=(1024, 1024), khss=1, with_f=True, with_r=False,
                           empty=[(0, 5), (100, 104), (1010, 1024)], full=[(300, 306), (640, 660)],
                           nblk_t=1024, empty_at=[1024], full_at=[]),
    # 1030 x 1031: a block is 1024/1031 of a row.  Block 1024 begins in row 1017 (T part); block 2048 is F-block 1010, which
    # begins in F-row 1003.
    "three_chunks": dict(shape=(1030, 1031), khss=1, with_f=True, with_r=True,
                         empty=[(200, 204), (995, 1010)], full=[(500, 504), (1012, 1026)],
                         nblk_t=1038, empty_at=[2048], full_at=[1024]),
    "khss3": dict(shape=(1030, 1031), khss=3, with_f=True, with_r=False,
                  empty=[(198, 246), (995, 1010)], full=[(500, 530), (1012, 1026)],
                  nblk_t=116, empty_at=[], full_at=[]),
    "no_F": dict(shape=(1030, 1031), khss=1, with_f=False, with_r=False,
                 empty=[(200, 204), (995, 1010)], full=[(500, 504), (1012, 1026)],
                 nblk_t=1038, empty_at=[], full_at=[1024]),
}


@functools.lru_cache(maxsize=None)
def seed_case(name):
    """inputs of one case, the numpy answer and the seeds of every block (T-blocks, then F-blocks); treated as read-only"""
    c = SEED_CASES[name]
    Nj, Ni = c["shape"]
    n = Nj * Ni
    rng = np.random.default_rng(1000 + len(name))
    flat = np.arange(n, dtype=np.float64).reshape(Nj, Ni)
    # distinct coordinates: smooth in the flat index, so a seed at the wrong rank or offset cannot compare equal
    lat = 60. + 29. * flat / n
    lon = 359.5 * (1. - flat / n)
    latF, lonF = lat + 0.013, lon + 0.021
    lat[rng.random((Nj, Ni)) < 0.03] -= 20.                     # 40 .. 69: most of them below 55
    lat[rng.random((Nj, Ni)) < 0.02] = np.nan
    # the seeding density varies along the rows between nothing and nearly everything, so that the block counts do
    dens = (0.5 + 0.5 * np.sin(np.arange(Nj) / 17.))[:, None]
    tmask = np.where(rng.random((Nj, Ni)) < dens, 1, rng.choice([0, 0, 2], size=(Nj, Ni))).astype('i1')
    sic = np.where(rng.random((Nj, Ni)) < 0.9, rng.choice([0.9, 0.95, 0.95, np.nan], size=(Nj, Ni)), rng.choice([0.5, 0.89], size=(Nj, Ni)))
    rmask = np.where(rng.random((Nj, Ni)) < 0.9, 1, rng.choice([0, -1], size=(Nj, Ni))).astype('i1')
    for j0, j1 in c["empty"]:
        tmask[j0:j1] = 0
    for j0, j1 in c["full"]:
        tmask[j0:j1] = 1
        rmask[j0:j1] = 1
        sic[j0:j1] = np.where(np.isnan(sic[j0:j1]), np.nan, 0.95)
        lat[j0:j1] = np.where(np.isnan(lat[j0:j1]), np.nan, np.maximum(lat[j0:j1], 60. + 29. * flat[j0:j1] / n))
    kw = dict(khss=c["khss"])
    if c["with_r"]:
        kw["rmask"] = rmask
    if c["with_f"]:
        kw.update(latF=latF, lonF=lonF)
    wantT, wantF, fT, fF = nemo_seed_ref(tmask, lat, lon, sic, **kw)
    ns = fT.size
    nblk_t = -(-ns // SEED_BLOCK)
    counts = np.zeros(2 * nblk_t * SEED_BLOCK, dtype=np.int64)
    counts[:ns] = fT.ravel()
    counts[nblk_t * SEED_BLOCK:nblk_t * SEED_BLOCK + ns] = fF.ravel()
    counts = counts.reshape(2 * nblk_t, SEED_BLOCK).sum(axis=1)
    return dict(tmask=tmask, lat=lat, lon=lon, sic=sic, kw=kw, wantT=wantT, wantF=wantF, ns=ns, nblk_t=nblk_t, counts=counts)


def longest_run(flags):
    best = run = 0
    for f in flags:
        run = run + 1 if f else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("name", list(SEED_CASES))
def test_seed_inputs_reach_what_they_are_meant_to(name):
    """from the numpy side: the block and chunk layout of every case, varying block counts, runs of empty and of full blocks,
    and such runs across the chunk boundaries"""
    c, d = SEED_CASES[name], seed_case(name)
    counts, nblk_t = d["counts"], d["nblk_t"]
    assert nblk_t == c["nblk_t"] and len(counts) == 2 * nblk_t
    nT, nF = len(d["wantT"]), len(d["wantF"])
    assert counts[:nblk_t].sum() == nT and counts[nblk_t:].sum() == nF
    assert nT > 0.1 * d["ns"] and (nF > 0.02 * d["ns"]) == c["with_f"] and (nF == 0) == (not c["with_f"])
    if name == "one_chunk_of_T":
        assert d["ns"] == SEED_BLOCK * SCAN_CHUNK and nblk_t == SCAN_CHUNK               # no padded tail, F-blocks all in chunk 1
    elif name in ("three_chunks", "no_F"):
        assert d["ns"] == 1061930 and 2 * nblk_t == 2076 and -(-2 * nblk_t // SCAN_CHUNK) == 3
        assert (nblk_t - 1) % SCAN_CHUNK == 13 and (nblk_t - 1) // SCAN_CHUNK == 1      # total[0] from position 13 -> split at 14 of chunk 1
        assert d["ns"] % SEED_BLOCK != 0 and nblk_t < 2 * SCAN_CHUNK < 2 * nblk_t       # a partly filled T-block, F-blocks in chunks 1 and 2
    else:
        assert d["ns"] == 344 * 344 and 100 < 2 * nblk_t <= SCAN_CHUNK and 1030 % 3 and 1031 % 3
    # distinct coordinates, NaN and low latitudes, every concentration value
    lat, lon = d["lat"], d["lon"]
    ok = ~np.isnan(lat)
    assert len(np.unique(lon)) == lon.size and len(np.unique(lat[ok])) == ok.sum() and 0 < (~ok).sum()
    assert (lat[ok] < 55.).sum() > 1000 and np.isnan(d["sic"]).sum() > 1000
    assert set(np.unique(d["sic"][~np.isnan(d["sic"])])) == {0.5, 0.89, 0.9, 0.95}
    assert np.isnan(d["wantT"][:, 0]).any()                                           # a NaN latitude keeps its point
    # block counts vary; several consecutive blocks empty, some blocks full
    tb = counts[:nblk_t]
    assert len(np.unique(tb)) > (30 if c["khss"] == 1 else 15)
    assert longest_run(tb == 0) >= 3 and (c["khss"] != 1 or longest_run(tb == SEED_BLOCK) >= 3)
    for b in c["empty_at"]:
        assert b < len(counts) and (counts[b - 3:b + 3] == 0).all() and counts[b - 40:b + 40].any(), b
    for b in c["full_at"]:
        assert (counts[b - 3:b + 3] == SEED_BLOCK).all(), b
    # the offsets the scan hands out in the later chunks are larger than one block's worth
    assert c["khss"] != 1 or counts[:SCAN_CHUNK].sum() > 100 * SEED_BLOCK


def test_one_empty_and_one_full_run_straddle_block_1024():
    assert any(1024 in c["empty_at"] for c in SEED_CASES.values()) and any(1024 in c["full_at"] for c in SEED_CASES.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEED_CASES))
def test_nemo_seed_across_blocks_and_scan_chunks(ctx, name):
    """which seeds, in which order, bit for bit against numpy; the fused projection against the projection entry point; the
    counting call and a capacity one short through the raw binding"""
    d = seed_case(name)
    want = np.concatenate([d["wantT"], d["wantF"]])
    nT, nF = len(d["wantT"]), len(d["wantF"])
    # raw binding first: the counting call, then one seed too little room -> SITRK_EINVAL; the handle must go on working
    C, p = _lib.C, _lib._ptr
    tm = d["tmask"]
    Nj, Ni = tm.shape
    kw = d["kw"]
    arrs = [np.ascontiguousarray(d[k]) for k in ("lat", "lon", "sic")]
    opt = [None if kw.get(k) is None else np.ascontiguousarray(kw[k]) for k in ("rmask", "latF", "lonF")]
    cT, cF = C.c_int64(-1), C.c_int64(-1)
    args = (ctx._h, Nj, Ni, kw["khss"], p(tm), p(opt[0]), p(arrs[0]), p(arrs[1]), p(arrs[2]), p(opt[1]), p(opt[2]), 70., -45.)
    assert ctx._L.sitrk_nemo_seed(*args, 0, None, None, C.byref(cT), C.byref(cF)) == 0
    print("%s: nT = %d (numpy %d), nF = %d (numpy %d)" % (name, cT.value, nT, cF.value, nF))
    assert (cT.value, cF.value) == (nT, nF)
    short = np.full((nT + nF - 1, 2), -7.)
    assert ctx._L.sitrk_nemo_seed(*args, nT + nF - 1, p(short), None, C.byref(cT), C.byref(cF)) == -1      # SITRK_EINVAL
    assert b"do not fit the capacity" in ctx._L.sitrk_last_error(ctx._h)
    assert (short == -7.).all()
    ll, yx, gT, gF = ctx.nemo_seed(tm, d["lat"], d["lon"], d["sic"], **kw)
    assert (gT, gF) == (nT, nF)
    bad = np.flatnonzero(~((ll.view(np.uint64) == want.view(np.uint64)) | (np.isnan(ll) & np.isnan(want))).all(axis=1))
    print("%s: %d of %d seeds differ, first at %s" % (name, len(bad), len(want), bad[:4]))
    assert same_bits(ll, want) and np.array_equal(ll, want, equal_nan=True)
    assert same_bits(yx, ctx.geo2cart(ll))


# ------------------------------------------------------------------------------------- 2. seed search beyond 64 superblocks
SEARCH_MESHES = {
    # name: Nj, Ni, dkm, superblocks (rows, columns), seeds of the oracle subsample per group
    "tall": dict(shape=(16400, 40), dkm=0.3, nsb=(65, 1), sub=dict(U=150, T=50, F=50, U2=55, T2=28, F2=28, P=8)),
    "wide": dict(shape=(40, 16660), dkm=0.3, nsb=(1, 66), sub=dict(U=80, T=30, F=30, U2=55, T2=28, F2=28, P=8)),
    "both": dict(shape=(8200, 260), dkm=0.6, nsb=(33, 2), sub=dict(U=8, T=3, F=3, U2=52, T2=2, F2=2, P=2)),
}
YC, XC = -300., 200.


def sb_of(ji, Ni):
    nsi = -(-Ni // SB_POINTS)
    return (ji[..., 0] // SB_POINTS) * nsi + ji[..., 1] // SB_POINTS


@functools.lru_cache(maxsize=None)
def search_mesh(name):
    """mesh, seeds by group and the subsample the oracle answers for; treated as read-only"""
    c = SEARCH_MESHES[name]
    (Nj, Ni), dkm = c["shape"], c["dkm"]
    grid = syn.shift_grid(syn.make_grid(Nj, Ni, dkm=dkm, warp=1.0), YC, XC)
    llT = orc.CartNPSkm2Geo1D(np.stack([grid["Yt"].ravel(), grid["Xt"].ravel()], axis=1))
    latT = np.ascontiguousarray(llT[:, 0].reshape(Nj, Ni))
    lonT = np.ascontiguousarray(np.mod(llT[:, 1], 360.).reshape(Nj, Ni))
    nsj, nsi = -(-Nj // SB_POINTS), -(-Ni // SB_POINTS)
    assert (nsj, nsi) == c["nsb"] and SB_ROUND < nsj * nsi <= 2 * SB_ROUND
    round2 = list(range(SB_ROUND, nsj * nsi))
    rng = np.random.default_rng({"tall": 41, "wide": 42, "both": 43}[name])

    def plane(jj, ii):                                       # fractional index -> (y, x) of this mesh
        y, x = syn._index_to_plane(np.asarray(jj, dtype=np.float64), np.asarray(ii, dtype=np.float64), Nj, Ni, dkm, 1.0)
        return np.stack([y + YC, x + XC], axis=1)

    def on_points(jj, ii):
        return (np.stack([grid["Yt"][jj, ii], grid["Xt"][jj, ii]], axis=1), np.stack([grid["Yf"][jj, ii], grid["Xf"][jj, ii]], axis=1))

    # a hole in the mask and a patch of open water, away from the second round's superblocks
    hj, hi = int(0.31 * Nj), int(0.31 * Ni)
    sj, si = int(0.55 * Nj), int(0.55 * Ni)
    hole = (hj, hj + min(24, Nj // 4), hi, hi + min(24, Ni // 4))
    water = (sj, sj + min(30, Nj // 4), si, si + min(30, Ni // 4))
    tmask = grid["tmask"].copy(); tmask[hole[0]:hole[1], hole[2]:hole[3]] = 0
    sic = np.ones((Nj, Ni)); sic[water[0]:water[1], water[2]:water[3]] = 0.05

    groups, parts, onpt = {}, [], {}

    def add(key, yx, ji=None):
        n0 = sum(len(p_) for p_ in parts)
        groups[key] = np.arange(n0, n0 + len(yx))
        parts.append(yx)
        if ji is not None:
            onpt[key] = ji

    n_u, n_p = 2000, 1500
    add("U", np.stack([rng.uniform(grid["Yt"].min() - 2., grid["Yt"].max() + 2., n_u),
                       rng.uniform(grid["Xt"].min() - 2., grid["Xt"].max() + 2., n_u)], axis=1))
    jj, ii = rng.integers(0, Nj, n_p), rng.integers(0, Ni, n_p)
    onT, onF = on_points(jj, ii)
    add("T", onT, np.stack([jj, ii], axis=1)); add("F", onF, np.stack([jj, ii], axis=1))
    for sb in round2:
        j0, i0 = (sb // nsi) * SB_POINTS, (sb % nsi) * SB_POINTS
        j1, i1 = min(Nj, j0 + SB_POINTS), min(Ni, i0 + SB_POINTS)
        # uniform over the superblock's own points, a little inside its edge towards the neighbouring superblock
        add("U2_%d" % sb, plane(rng.uniform(j0 - 0.3 if j0 == 0 else j0 - 0.1, j1 - 0.6, 60), rng.uniform(i0 - 0.3 if i0 == 0 else i0 - 0.1, i1 - 0.6, 60)))
        jj, ii = rng.integers(j0, j1, 60), rng.integers(i0, i1, 60)
        onT, onF = on_points(jj, ii)
        add("T2_%d" % sb, onT, np.stack([jj, ii], axis=1)); add("F2_%d" % sb, onF, np.stack([jj, ii], axis=1))
    add("Phole", plane(rng.uniform(hole[0] + 2, hole[1] - 3, 20), rng.uniform(hole[2] + 2, hole[3] - 3, 20)))
    add("Pwater", plane(rng.uniform(water[0] + 2, water[1] - 3, 20), rng.uniform(water[2] + 2, water[3] - 3, 20)))
    add("far", np.array([[grid["Yt"].min() - 900., XC], [YC, grid["Xt"].max() + 1500.], [YC + 4000., XC - 4000.]]))
    yx = np.ascontiguousarray(np.concatenate(parts))
    ll = orc.CartNPSkm2Geo1D(yx)
    ll[:, 1] = np.mod(ll[:, 1], 360.)
    for key, ji in onpt.items():                            # seeds on T-points take the grid's own lat/lon bits: distance exactly 0
        if key.startswith("T"):
            ll[groups[key], 0] = latT[ji[:, 0], ji[:, 1]]
            ll[groups[key], 1] = lonT[ji[:, 0], ji[:, 1]]
    sub = c["sub"]
    sel = [groups["U"][:sub["U"]], groups["T"][:sub["T"]], groups["F"][:sub["F"]], groups["Phole"][:sub["P"]], groups["Pwater"][:sub["P"]],
           groups["far"]]
    for sb in round2:
        sel += [groups["U2_%d" % sb][:sub["U2"]], groups["T2_%d" % sb][:sub["T2"]], groups["F2_%d" % sb][:sub["F2"]]]
    return dict(grid=grid, latT=latT, lonT=lonT, tmask=tmask, sic=sic, yx=yx, ll=ll, groups=groups, onpt=onpt, round2=round2,
                sel=np.concatenate(sel), Nj=Nj, Ni=Ni)


def oracle_nearest(m, idx, **kw):
    """oracle.NearestPoint of the seeds `idx`, one call per seed on 8 threads: ((n,2) indices, (n,) distances of the argmin)"""
    def one(k):
        return orc.NearestPoint(m["ll"][k], m["latT"], m["lonT"], return_dist=True, **kw)
    with ThreadPoolExecutor(8) as ex:
        r = list(ex.map(one, idx))
    return np.array([(a, b) for a, b, _ in r], dtype=np.int64), np.array([d for _, _, d in r])


@functools.lru_cache(maxsize=None)
def search_oracle(name):
    """the oracle's SeedInit and NearestPoint on the subsample"""
    m = search_mesh(name)
    sel, g = m["sel"], m["grid"]
    o = orc.SeedInit(np.arange(len(sel)), m["ll"][sel], m["yx"][sel], m["latT"], m["lonT"], g["Yf"], g["Xf"], g["resol"], m["tmask"], m["sic"],
                     return_why=True, nthreads=8)
    keep = np.zeros(len(sel), dtype=np.int8); keep[o[6]] = 1
    near, dmin = oracle_nearest(m, sel, resolkm=g["resol"], rd_found_km=2.5, max_itr=10)
    return dict(keep=keep, why=o[7], jiT=o[4], near=near, dmin=dmin)


@functools.lru_cache(maxsize=None)
def search_near_ties(name):
    """Positions in the subsample of the one kind of seed that may be left out of the comparison with the oracle: its two smallest
    Haversine distances over the field differ by a non-zero amount below 1e-12 relative (the device's libm and the host's may
    order them differently).  From the oracle alone."""
    m = search_mesh(name)

    def one(k):
        d = np.partition(orc.Haversine(m["ll"][k, 0], m["ll"][k, 1], m["latT"], m["lonT"]).ravel(), 1)[:2]
        return bool(0. < d[1] - d[0] < 1e-12 * d[1])
    with ThreadPoolExecutor(8) as ex:
        return np.flatnonzero(list(ex.map(one, m["sel"])))


@pytest.mark.parametrize("name", list(SEARCH_MESHES))
def test_search_seeds_reach_the_second_round(name):
    """from the oracle's answer: every superblock of the second round holds >= 50 seeds on its T- and F-points and the nearest
    T-point of >= 50 uniform seeds; the subsample takes every reason for leaving a seed out"""
    m, o = search_mesh(name), search_oracle(name)
    sel, Ni = m["sel"], m["Ni"]
    pos = {int(k): q for q, k in enumerate(sel)}
    assert len(pos) == len(sel) and (len(sel) < 160 if name == "both" else 350 < len(sel) < 450)
    assert len(m["round2"]) == {"tall": 1, "wide": 2, "both": 2}[name]
    for sb in m["round2"]:
        for key in ("T2_%d" % sb, "F2_%d" % sb):
            assert (sb_of(m["onpt"][key], Ni) == sb).sum() >= 50
        # a seed on a T-point: the oracle finds that very point (or an earlier one at distance 0: there is none on these meshes)
        q = [pos[int(k)] for k in m["groups"]["T2_%d" % sb] if int(k) in pos]
        ji = m["onpt"]["T2_%d" % sb][:len(q)]
        assert len(q) >= 2 and np.array_equal(o["near"][q], ji) and (o["dmin"][q] == 0.).all()
        q = [pos[int(k)] for k in m["groups"]["U2_%d" % sb] if int(k) in pos]
        there = (o["near"][q, 0] >= 0) & (sb_of(o["near"][q], Ni) == sb)
        assert there.sum() >= 50, (sb, int(there.sum()))
    assert set(np.unique(o["why"])) == {0, 1, 2, 3}
    q = [pos[int(k)] for k in m["groups"]["U"] if int(k) in pos]
    assert (o["why"][q] == 1).any() or name == "both"                   # uniform seeds in the margin: farther than the acceptance radius
    assert (o["near"][[pos[int(k)] for k in m["groups"]["far"]]] == -1).all()
    # what the comparison on the device may leave out at most, known before any device runs (0 on all three meshes)
    assert len(search_near_ties(name)) <= 0.01 * len(sel)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEARCH_MESHES))
def test_seed_search_beyond_64_superblocks(ctx, name):
    """bounding-sphere search == whole-grid scan on all seeds; both == the oracle's SeedInit and NearestPoint on the subsample"""
    m, o = search_mesh(name), search_oracle(name)
    g, sel = m["grid"], m["sel"]
    ctx.set_grid(g["Yf"], g["Xf"], g["Yf"], g["Xf"], g["Yf"], g["Xf"], m["tmask"])
    res = {}
    try:
        for mode in (0, 1):
            ctx.set_tuning(locate_bruteforce=mode)
            res[mode] = ctx.seed_init(m["ll"], m["yx"], m["latT"], m["lonT"], g["resol"], m["sic"])
    finally:
        ctx.set_tuning(locate_bruteforce=0)
    for what, a, b in zip(("jiT", "keep", "why"), res[0], res[1]):
        bad = np.flatnonzero(a != b) if a.ndim == 1 else np.flatnonzero((a != b).any(axis=1))
        print("%s: search vs whole-grid scan, %s differs at %d of %d seeds %s" % (name, what, len(bad), len(a), bad[:6]))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)                                     # no exclusions between the two device modes
    jiT, keep, why = res[0]
    assert set(np.unique(why)) == {0, 1, 2, 3} and 0 < keep.sum() < len(keep)
    near, dmin = ctx.nearest_point(m["ll"][sel], m["latT"], m["lonT"], resolkm=g["resol"], rd_found_km=2.5, max_itr=10)
    # against the oracle; a disagreement is excused only on a near-tie of the oracle's own distances, at most 1 % of them
    kept_o = o["keep"] == 1
    full_ji = np.zeros((len(sel), 2), dtype=np.int64); full_ji[kept_o] = o["jiT"]
    differs = (keep[sel] != o["keep"]) | (why[sel] != o["why"]) | (kept_o & (jiT[sel] != full_ji).any(axis=1)) | (near != o["near"]).any(axis=1)
    left_out = np.intersect1d(np.flatnonzero(differs), search_near_ties(name))
    print("%s: %d of %d subsample seeds differ from the oracle, %d of them near-ties" % (name, differs.sum(), len(sel), len(left_out)))
    assert len(left_out) <= 0.01 * len(sel)
    assert np.array_equal(left_out, np.flatnonzero(differs)), np.flatnonzero(differs)[:8]
    # distances: the project's tolerance where the device searched; where it skipped the search (farther from every superblock
    # than the largest radius the acceptance loop reaches) it answers +inf, and the oracle's point is rejected too
    searched = np.isfinite(dmin)
    assert np.allclose(dmin[searched], o["dmin"][searched], rtol=1e-12, atol=1e-9)
    rmax = 0.5 * g["resol"].max() * 1.2 ** 8
    assert (dmin[~searched] == np.inf).all() and (o["near"][~searched] == -1).all() and (o["dmin"][~searched] > rmax).all()
    far = np.flatnonzero(np.isin(sel, m["groups"]["far"]))
    assert len(far) == 3 and (near[far] == -1).all() and (dmin[far] == np.inf).all()
    if name == "tall":
        # the other source of the skip distance: no resolution field, rd_found_km and 3 enlargements
        sub = np.r_[0:60, len(sel) - 60:len(sel), far]
        near2, dmin2 = ctx.nearest_point(m["ll"][sel[sub]], m["latT"], m["lonT"], resolkm=None, rd_found_km=1.0, max_itr=5)
        o_near2, o_dmin2 = oracle_nearest(m, sel[sub], resolkm=None, rd_found_km=1.0, max_itr=5)
        excused = np.isin(sub, left_out)
        assert np.array_equal(near2[~excused], o_near2[~excused]) and (near2 == -1).any() and (near2 >= 0).any()
        searched = np.isfinite(dmin2)
        assert np.allclose(dmin2[searched], o_dmin2[searched], rtol=1e-12, atol=1e-9)
        assert (dmin2[~searched] == np.inf).all() and (o_near2[~searched] == -1).all() and (o_dmin2[~searched] > 1.0 * 1.2 ** 3).all()
        assert (near2[-3:] == -1).all() and (dmin2[-3:] == np.inf).all()


# ------------------------------------------------------------------------------------- 3. sitrk_tri2quad across a scan chunk
QM_BLOCK = 1024                    # triangles per block of the compaction
QM_EDGE = QM_BLOCK * SCAN_CHUNK    # first triangle of the scan's second chunk


@functools.lru_cache(maxsize=None)
def big_lattice():
    """726 x 726 jittered lattice, 1 051 250 triangles = 1027 blocks = 2 chunks, with masked points and dead triangles that
    leave unmatched runs on both sides of triangle 1 048 576; and the round form's answer"""
    ny = nx = 726
    yx = jittered_lattice(ny, nx, -2000., 1500., seed=31)
    tris = sit.lattice_cells(ny, nx, "tri").copy()
    assert len(tris) == 1051250 and -(-len(tris) // QM_BLOCK) == 1027
    rng = np.random.default_rng(8)
    tris[::3] = tris[::3, ::-1]
    mask = np.ones(ny * nx, dtype=np.int8)
    mask[rng.choice(ny * nx, 4000, replace=False)] = 0
    # triangle t belongs to lattice cell t // 2: cell row 723 holds triangle 1 048 576.  Masked points there ...
    row, col = (QM_EDGE // 2) // (nx - 1), (QM_EDGE // 2) % (nx - 1)
    assert row == 723 and 60 < col < nx - 120
    mask[row * nx + col - 40:row * nx + col - 25] = 0
    mask[row * nx + col + 30:row * nx + col + 50] = 0
    # ... and triangles with a repeated vertex: scattered, and in runs on both sides of the chunk boundary
    dead = np.concatenate([rng.choice(len(tris), 3000, replace=False), np.arange(QM_EDGE - 300, QM_EDGE - 120),
                           np.arange(QM_EDGE - 9, QM_EDGE + 5), np.arange(QM_EDGE + 200, QM_EDGE + 520)])
    tris[dead, 1] = tris[dead, 0]
    tris = np.ascontiguousarray(tris)
    quads, tri_quad, rounds = tri2quad_rounds(yx, tris, mask)
    return yx, mask, tris, quads, tri_quad, rounds


def test_big_lattice_has_unequal_blocks_around_the_chunk_boundary():
    yx, mask, tris, quads, tri_quad, rounds = big_lattice()
    assert 400000 < len(quads) < len(tris) // 2 and rounds >= 2
    un = tri_quad < 0
    assert longest_run(un[QM_EDGE - QM_BLOCK:QM_EDGE]) >= 100 and longest_run(un[QM_EDGE:QM_EDGE + QM_BLOCK]) >= 100
    assert un[QM_EDGE - 9:QM_EDGE + 5].all()                                 # one run across the boundary itself
    assert (tri_quad == -2).sum() > 1000 and (tri_quad == -1).sum() > 1000
    # what the device's blocks count: the pairs whose smaller triangle lies in the block, i.e. the first triangle of each quadrangle
    first = np.full(len(quads), len(tris))
    np.minimum.at(first, tri_quad[~un], np.flatnonzero(~un))
    per_block = np.bincount(first // QM_BLOCK, minlength=1027)
    assert per_block.sum() == len(quads) and len(set(per_block[1021:1027])) >= 4
    assert per_block[:SCAN_CHUNK].sum() > 100 * QM_BLOCK                      # the carry into chunk 1 is far more than a block's worth


@pytest.mark.gpu
def test_tri2quad_compaction_across_a_scan_chunk(ctx):
    yx, mask, tris, rq, rtq, rrounds = big_lattice()
    quads, tri_quad, rounds = ctx.tri2quad(yx, tris, mask=mask)
    print("726 x 726: %d quadrangles in %d rounds (round form: %d in %d)" % (len(quads), rounds, len(rq), rrounds))
    assert quads.dtype == np.int32 and tri_quad.dtype == np.int32
    assert len(quads) == len(rq)
    assert np.array_equal(tri_quad, rtq), np.flatnonzero(tri_quad != rtq)[:8]
    assert np.array_equal(quads, rq), np.flatnonzero((quads != rq).any(axis=1))[:8]
    assert rounds == rrounds
