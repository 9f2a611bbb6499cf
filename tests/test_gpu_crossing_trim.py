"""The crossing path's skips on the MI355X (crossed_edge_row: the terms of the right and of the upper / left edge sit behind a
test of the lanes still undecided; the selects of a diagonal destination behind the test that can make one): the fused run,
the sub-stepped run and the time-blend run bit-exact (yx, jiT, alive, kill_rec) against the oracle and against sitrk_step, on
small sets built so that WHOLE WAVES fall into each skip class.

512 buoys (two workgroups, eight waves) are seeded inside a 6 x 6-cell block of a 48 x 48 mesh and moved ~0.25 cell per
record for 24 records, 8 records per launch, so every wave has several crossers in every record:
  * a flow uniform over the mesh in each of the eight compass directions -- S: every crosser leaves by the bottom edge (both
    groups skipped), SE / E: by the bottom or the right edge (the second group skipped), the others need all three tests;
  * a solid-body rotation about the block (every exit inside one wave);
  * an outflow from the block's centre through a frame of land / of thin ice: buoys are killed while they leave through
    each of the four edges and through a corner (checked on the oracle's host cells);
each with the LDS patch and without (patch_kb = 0: the global-table path); fp32 and fp64 records, both velocity rules, and
per-buoy record windows on the rotation."""
import functools

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import synthetic as syn
from oracle import oracle as orc
from test_substep import oracle_replay
from test_tlerp import oracle_replay_tlerp

pytestmark = pytest.mark.gpu

NJ = NI = 48
DKM = 4.0
B0, B1 = 21, 27                         # the seeded block: cells [B0, B1) x [B0, B1)
NP, NT, K, FUSE = 512, 24, 8, 8
A, D = 0.28125, 0.203125                # m/s: 1.0125 km = 0.253 cell per hourly record along an axis, 0.73 km on each axis of a diagonal
SCALE = (1.0, 0.875, 1.125, 0.9375)     # per record (cycled): the time-blend run has something to blend; all exact in binary32
FLOWS = {"S": (0., -A), "SE": (D, -D), "E": (A, 0.), "NE": (D, D), "N": (0., A), "NW": (-D, D), "W": (-A, 0.), "SW": (-D, -D)}
# the cell moves (dj, di) a uniform flow can produce on the regular mesh: straight through the edges it points at, or their corner
MOVES = {"S": {(-1, 0)}, "E": {(0, 1)}, "N": {(1, 0)}, "W": {(0, -1)},
         "SE": {(-1, 0), (0, 1), (-1, 1)}, "NE": {(1, 0), (0, 1), (1, 1)}, "NW": {(1, 0), (0, -1), (1, -1)}, "SW": {(-1, 0), (0, -1), (-1, -1)}}


@functools.lru_cache(maxsize=None)
def case(warp, flow, kill=None):
    """grid, fields (K records, fp64 masters), seeds and their host cells"""
    grid = syn.make_grid(NJ, NI, dkm=DKM, warp=warp)
    yc, xc = syn._index_to_plane(0.5 * (B0 + B1 - 1), 0.5 * (B0 + B1 - 1), NJ, NI, DKM, warp)
    if flow in FLOWS:
        u1, v1 = np.full((NJ, NI), FLOWS[flow][0]), np.full((NJ, NI), FLOWS[flow][1])
    elif flow == "rot":                 # 0.35 m/s at 12 km from the centre, < 0.5 cell per record on the block; 2.5 rad in 24 records
        u1, v1 = -(0.35 / 12.) * (grid["Yu"] - yc), (0.35 / 12.) * (grid["Xv"] - xc)
    else:                               # "out": away from the centre on both axes, full speed beyond 8 km
        u1, v1 = A * np.clip((grid["Xu"] - xc) / 8., -1., 1.), A * np.clip((grid["Yv"] - yc) / 8., -1., 1.)
    u = np.stack([u1 * SCALE[k % 4] for k in range(K)])
    v = np.stack([v1 * SCALE[k % 4] for k in range(K)])
    sic = np.ones((K, NJ, NI))
    grid = dict(grid)
    if kill == "land":                  # a frame of land three cells off the block (Survive's land stencil reaches one cell further in)
        tm = grid["tmask"].copy()
        tm[B0 - 4:B1 + 4, B0 - 4:B1 + 4] = 0
        tm[B0 - 3:B1 + 3, B0 - 3:B1 + 3] = 1
        grid["tmask"] = tm
    elif kill == "ice":                 # thin ice everywhere but on the block and two cells around it (Survive: the mean of 5 cells)
        thin = np.ones((NJ, NI), dtype=bool)
        thin[B0 - 2:B1 + 2, B0 - 2:B1 + 2] = False
        sic[:, thin] = 0.02
    rng = np.random.default_rng(7)
    jj, ii = rng.uniform(B0 - 0.5, B1 - 0.5, NP), rng.uniform(B0 - 0.5, B1 - 0.5, NP)
    y, x = syn._index_to_plane(jj, ii, NJ, NI, DKM, warp)
    yx = np.ascontiguousarray(np.stack([y, x], axis=1))
    guess = np.stack([np.rint(jj), np.rint(ii)], axis=1).astype(np.int64)
    ji = np.zeros((NP, 2), dtype=np.int64)
    for b in range(NP):
        ok, ji[b], _ = orc.FindContainingCell(yx[b], guess[b], grid["Yf"], grid["Xf"])
        assert ok
    assert ji.min() >= B0 - 1 and ji.max() <= B1
    return grid, u, v, sic, yx, ji


def windows(windowed):
    if not windowed:
        return np.zeros(NP, dtype=np.int64), np.full(NP, NT - 1, dtype=np.int64)
    rng = np.random.default_rng(11)
    return (rng.integers(0, 4, NP) * (rng.random(NP) < 0.3)).astype(np.int64), \
        (NT - 1 - rng.integers(0, 4, NP) * (rng.random(NP) < 0.3)).astype(np.int64)


def as_records(a, dtype):
    return a.astype(dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(warp, flow, kill=None, dtype=np.float32, strat=1, windowed=False, nsub=1, phase=None):
    """the oracle's run of a case (computed once, read only): oracle_replay / oracle_replay_tlerp of the CPU tests"""
    grid, u, v, sic, yx, ji = case(warp, flow, kill)
    rf, rl = windows(windowed)
    args = (grid, yx, ji, as_records(u, dtype), as_records(v, dtype), as_records(sic, dtype), rf, rl, 0, NT, 3600., nsub, strat)
    ref = oracle_replay(*args) if phase is None else oracle_replay_tlerp(*args, phase)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def moves_of(ref, only_killed=False):
    """the set of cell moves (dj, di) the oracle made (of the buoys in the record that killed them, if only_killed)"""
    jit, out = ref["jiT"], set()
    for k in range(NT):
        d = jit[k + 1] - jit[k]
        sel = d.any(axis=1)
        if only_killed:
            sel &= ref["kill_rec"] == k
        out |= {tuple(int(t) for t in m) for m in d[sel]}
    return out


def gpu_state(warp, flow, kill, dtype, strat, windowed, mode, patch_kb=None, nsub=1, phase=None):
    grid, u, v, sic, yx, ji = case(warp, flow, kill)
    rf, rl = windows(windowed)
    nslots = NT if phase is not None else K
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=3600.,
                         iUVstrategy=strat, nslots=nslots, field_dtype=dtype, nsub=nsub)
    try:
        for s in range(nslots):
            trk.load_record(s, u[s % K].astype(dtype), v[s % K].astype(dtype), sic[s % K].astype(dtype))
        knobs = {"fuse": FUSE}
        if patch_kb is not None:
            knobs["patch_kb"] = patch_kb
        trk.ctx.set_tuning(**knobs)
        trk.set_buoys(yx, ji, rf if windowed else None, rl if windowed else None)
        if mode == "step":
            for k in range(NT):
                trk.step(k, k % K)
        elif phase is not None:
            trk.run(0, 0, NT, tinterp=phase)
        else:
            trk.ctx.run(0, 0, NT)
        if mode != "step":              # the fused kernels did the work, 8 records per launch where the records are not blended
            ls = trk.ctx.launch_stats()
            assert ls["step_launches"] == 0 and ls["fused_records"] == NT and (phase is not None or ls["fused_launches"] == NT // FUSE), ls
        return trk.state()
    finally:
        trk.close()


def assert_state(st, ref, what):
    assert np.array_equal(st["yx"].view(np.uint64), ref["final"].view(np.uint64)), what
    assert np.array_equal(st["vJIt"], ref["jiT"][-1]), what
    assert np.array_equal(st["iAlive"], ref["alive"][-1]), what
    assert np.array_equal(st["kill_rec"], ref["kill_rec"]), what


def check(warp, flow, kill=None, dtype=np.float32, strat=1, windowed=False, nsub=1, phase=None, step=True):
    ref = reference(warp, flow, kill, dtype, strat, windowed, nsub, phase)
    for patch_kb in (None, 0):
        assert_state(gpu_state(warp, flow, kill, dtype, strat, windowed, "run", patch_kb, nsub, phase), ref, ("run", patch_kb))
    if step:
        assert_state(gpu_state(warp, flow, kill, dtype, strat, windowed, "step", None, nsub), ref, "step")
    return ref


@pytest.mark.parametrize("warp", [0.0, 1.0])
@pytest.mark.parametrize("flow", list(FLOWS) + ["rot"])
def test_fused_run_in_every_skip_class(flow, warp):
    ref = check(warp, flow)
    assert ref["ncross"] >= 0.2 * NP * NT and ref["alive"][-1].all()     # >= 12 crossers per wave and record on average
    got = moves_of(ref)
    if flow == "rot":
        assert {(-1, 0), (0, 1), (1, 0), (0, -1)} <= got
    elif warp == 0.0:
        assert got <= MOVES[flow] and {m for m in MOVES[flow] if 0 in m} <= got


@pytest.mark.parametrize("kill", ["land", "ice"])
@pytest.mark.parametrize("warp", [0.0, 1.0])
def test_kills_through_every_edge_and_a_corner(warp, kill):
    ref = check(warp, "out", kill)
    died = moves_of(ref, only_killed=True)
    assert {(-1, 0), (0, 1), (1, 0), (0, -1)} <= died and any(0 not in m for m in died), died
    assert 0 < ref["alive"][-1].sum() < NP


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("strat", [0, 1])
def test_record_types_and_velocity_rules(strat, dtype):
    for flow, kill in (("rot", None), ("SE", None), ("out", "ice")):
        check(1.0, flow, kill, dtype, strat)


def test_record_windows():
    ref = check(1.0, "rot", windowed=True)
    assert ref["ncross"] > NP
    check(0.0, "out", "land", windowed=True)


@pytest.mark.parametrize("kernel", ["substep", "tlerp"])
@pytest.mark.parametrize("flow", list(FLOWS) + ["rot"])
def test_the_other_kernels_share_the_crossing_functions(flow, kernel):
    """three sub-steps per record, ~0.25 cell per record as above: advect_substep_kernel (the record's fields) and advect_tlerp_kernel (blended with
    the neighbouring records, phase 0.5), against the oracle replay of the CPU tests; the sub-stepped one also record by record"""
    phase = 0.5 if kernel == "tlerp" else None
    ref = check(1.0, flow, nsub=3, phase=phase, step=phase is None)
    assert ref["ncross"] >= 0.2 * NP * NT
