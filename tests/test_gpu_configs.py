"""Every BASELINE.json configuration SHAPE on the GPU (`pytest -m gpu`), as far as one GPU and this image allow:

* C2  (512x512, 1e5 buoys)  at its full 1000 steps, resident regime, `bench.py --check` = the oracle replays the run;
* C3  (4096x4096, 1e7 buoys) at its full 1000 steps, same check (24-step property tests: test_gpu_fullsize.py);
* C4  (4096x4096, 1e8 buoys over 8 GPUs): the per-rank shard (1.25e7 buoys) of ranks 0 and 7 through the fused path with
  the oracle on a subsample, and two adjacent shards in one context == the two shards separately (the partition
  invariance the 8-GPU run relies on).  The 8-GPU run itself is the driver's to launch;
* C5  (NANUK4 mesh, 1e7 buoys under the ice mask): the command line on a NANUK4-SHAPED synthetic mesh (566 x 492 at
  12.5 km -- the real mesh_mask and the demo tarball are not in the container), >= 1e6 seeds placed under a synthetic
  ice mask by `nemoSeed`'s rule, the reference's default 2-D-time mode, diffed against the oracle on a subsample;
* C1  (NANUK4 demo, 986 buoys, CPU reference path) cannot run here: tarball, netCDF4 and mojito are absent.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=1500):
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]), r.stderr


def test_c2_full_1000_steps_checked_by_the_oracle():
    d, err = _bench(["--config", "c2", "--steps", "1000", "--warmup", "50", "--check", "--no-cpu-baseline"])
    assert "check OK" in err, err[-2000:]
    assert d["steps"] == 1000 and d["config"]["grid"] == [512, 512] and d["config"]["buoys_per_gpu"] == 100000
    r = d["roofline"]
    # what the line says about its launches is what the library launched
    assert r["launches"] + r["one_record_launches"] >= 1000 // 32 and r["records_advanced"] + r["one_record_launches"] == 1000


def test_c3_full_1000_steps_checked_by_the_oracle():
    """the headline workload at the length BASELINE quotes it: 1e7 buoys x 1000 records (+ the fresh-records leg and the two
    reference legs of the same run), first 20 000 buoys bit-exact against the oracle at the end"""
    d, err = _bench(["--steps", "1000", "--warmup", "50", "--full", "--check", "--no-cpu-baseline", "--no-c2"])
    assert "check OK" in err and "after 4050 steps" in err, err[-2000:]          # warm-up + headline + fresh + per-record + 8-per-launch legs
    assert d["config"]["grid"] == [4096, 4096] and d["config"]["buoys_per_gpu"] == 10_000_000 and d["value"] > 1e9
    r = d["roofline"]
    # round 4: the bound is named after what DESIGN 3.2 item 35 found, the share of working lanes is stated next to it, and the
    # constants behind `frac` are tied to the binary that ran
    assert r["bound"] == "valu_issue+wave_chain" and r["records_advanced"] + r["one_record_launches"] == 1000
    assert 0.3 < r["lane_utilisation"] < 0.7 and "crossing-path" in r["lane_utilisation_note"]
    assert isinstance(r["stale"], bool) and len(r["isa_shipped"]["sha256"]) == 16 and r["isa_shipped"]["static"]["valu"] > 300
    if r["stale"]:
        assert r["frac"] is None and r["frac_uniform_4_cycles"] is None and "stale_note" in r
    else:
        assert r["isa_profiled"]["sha256"] == r["isa_shipped"]["sha256"]
        # frac follows from the line's own numbers
        want = r["valu_inst_per_wave_record"] * r["waves_per_launch"] * (r["records_advanced"] + r["one_record_launches"]) / \
            (r["avg_launch_ms"] * 1e-3 * (r["launches"] + r["one_record_launches"])) / 1e9 / r["peak"]
        assert abs(r["frac"] - want) < 1e-6 * want
        assert r["frac_uniform_4_cycles"] > r["frac"] and r["frac_at_held_clock"] > r["frac"] and 1.5 < r["clock_held_ghz"] <= 2.4
    # the ceiling weights the instruction classes (4 cycles for the 64-bit ones, 2 for the rest; a model, labelled as one), the
    # instruction count is the one of THIS run's launch length (fixed per launch + per record), and SURVEY's closed-form bytes
    # charged to every record of a launch come out above the HBM peak (the launch reads state and geometry once)
    assert 2.0 < r["cycles_per_valu_inst"] < 4.0 and abs(r["peak"] - 1024 * 2.4 / r["cycles_per_valu_inst"]) < 1e-6 * r["peak"]
    assert "MODEL" in r["peak_note"] and "fixed per launch" in r["valu_inst_source"] and 190 < r["valu_inst_per_wave_record"] < 230
    assert r["hbm"]["survey_formula_frac"] > 1.0 and r["hbm"]["frac"] < 0.5
    # the HBM-bound form (one record per launch): algorithmic bytes over THIS run's launch time, at least half of the 8 TB/s; the counter
    # traffic next to it is tied to the step kernel's own fingerprint
    pr = d["per_record_launch"]["roofline"]
    assert pr["bound"] == "hbm" and pr["kernel"] == "advect_step_kernel" and 0.5 < pr["frac"] < 1.0 and isinstance(pr["traffic_stale"], bool)
    if not pr["traffic_stale"]:
        assert 0.9 < pr["traffic"] / pr["algorithmic_bytes_per_launch"] < 1.3
    # the Survive derivation inside the clock: every record committed afresh over the box the buoys can touch
    f = d["fresh_records"]
    assert "amortised" not in d["note"] and "OUTSIDE the timed region" in d["note"]
    assert f["records_advanced"] == 1000 and f["launches"] >= 1000 // 32 and 0.3 < f["survive_box_share_of_grid"] < 0.6
    assert d["value_fresh_records"] == f["value"] and 0.6 * d["value"] < f["value"] < d["value"]
    assert 3.0 < d["survive_us_per_record"] < 40.0 and abs(f["ms_per_step"] - d["ms_per_step"]) * 1e3 < 4 * d["survive_us_per_record"]
    # the N = 1 extras: C4's per-rank shard on this GPU and the end-to-end upload segment (whole records and boxes)
    assert d["c4_shard"]["buoys"] == 12_500_000 and d["c4_shard"]["value"] > 1e10
    e = d["e2e_upload"]
    assert e["box"]["upload_bytes_per_step"] < 0.7 * e["whole_record"]["upload_bytes_per_step"] == 0.7 * e["slab_bytes"]
    assert e["box"]["particle_steps_per_s"] > e["whole_record"]["particle_steps_per_s"] > 1e9


def test_c3_cell_mean_rule_claims_no_issue_fraction():
    """`iUVstrategy = 0` runs another instantiation of the fused kernel than the one the committed counter passes describe: the
    line carries the throughput (oracle-checked) and withholds `roofline.frac` instead of pricing it with the wrong instruction count"""
    d, err = _bench(["--uv-strategy", "0", "--records", "8", "--fuse", "8", "--steps", "64", "--warmup", "8", "--only-fused", "--check",
                     "--no-cpu-baseline", "--no-c2"])
    assert "check OK" in err, err[-2000:]
    r = d["roofline"]
    assert d["value"] > 1e10 and r["frac"] is None and r["achieved"] is None and "iUVstrategy = 0" in r["frac_note"]


@pytest.fixture(scope="module")
def c4():
    from bench import CONFIGS
    Nj, Ni, nP, _ = CONFIGS["c4"]
    assert (Nj, Ni, nP) == (4096, 4096, 12_500_000)
    K = 6
    grid = syn.make_grid(Nj, Ni, dkm=4.0, warp=0.0)
    u, v, sic = syn.make_fields(grid, K=K, seed=2024, umax=0.3, drift=0.05)
    sic[:, 2000:2080, 1400:1700] = 0.02                 # open water: some buoys of every shard die
    return dict(grid=grid, u=u, v=v, sic=sic, K=K, nP=nP)


def _shard(c4, rank):
    """rank r's buoys exactly as bench.py --gpus 8 seeds them"""
    _, yx = syn.make_buoys(c4["grid"], c4["nP"], seed=1234 + rank, frac=0.6)
    return yx, syn.regular_host_cell(c4["grid"], yx).astype(np.int32)


def _run(c4, yx, ji, nsteps):
    g = c4["grid"]
    ctx = sit.Context(0)
    try:
        ctx.set_grid(g["Yf"], g["Xf"], g["Yu"], g["Xu"], g["Yv"], g["Xv"], g["tmask"])
        ctx.alloc_records(c4["K"], np.float32)
        for k in range(c4["K"]):
            ctx.push_record(k, c4["u"][k], c4["v"][k], c4["sic"][k])
        ctx.set_buoys(yx, ji)
        ctx.run(0, 0, nsteps)
        return ctx.fetch()
    finally:
        ctx.close()


def test_c4_rank_shards_and_partition_invariance(c4):
    from oracle import oracle as orc
    nsteps = 30
    f64 = [(c4["u"][k].astype(np.float64), c4["v"][k].astype(np.float64), c4["sic"][k].astype(np.float64)) for k in range(c4["K"])]
    shards, outs = {}, {}
    for rank in (0, 1, 7):
        shards[rank] = _shard(c4, rank)
        outs[rank] = _run(c4, *shards[rank], nsteps)
    for rank in (0, 7):                                  # the oracle on every 1201st buoy of the first and last rank
        yx, ji = shards[rank]
        sel = np.arange(0, len(yx), 1201)
        ref = orc.Tracker(c4["grid"], yx[sel], ji[sel], nthreads=8)
        for s in range(nsteps):
            ref.step(s, *f64[s % c4["K"]], want_out=False)
        o = outs[rank]
        assert np.array_equal(o["yx"][sel], ref.pos) and np.array_equal(o["jiT"][sel], ref.jiT)
        assert np.array_equal(o["alive"][sel], ref.alive) and 0 < o["alive"].sum() < len(yx)
    # two adjacent shards in ONE context == each on its own (2.5e7 buoys on one GPU)
    both = _run(c4, np.concatenate([shards[0][0], shards[1][0]]), np.concatenate([shards[0][1], shards[1][1]]), nsteps)
    for k in ("yx", "jiT", "alive", "kill_rec"):
        assert np.array_equal(both[k], np.concatenate([outs[0][k], outs[1][k]])), k


def _c5_cli_case(tmp_path, monkeypatch, ncand, nrec, min_seeds, stride):
    """The command line, files in -> files out, on the NANUK4-shaped synthetic mesh with `ncand` candidate seeds filtered by
    `nemoSeed`'s rule; every `stride`-th kept buoy is replayed on the oracle from the seed cache the run wrote."""
    import time
    import test_driver as td
    from oracle import oracle as orc
    from sitrack_amd import driver as drv, ncio
    monkeypatch.chdir(tmp_path)
    c = td.make_case(str(tmp_path), nrec=nrec, nP=ncand, Nj=566, Ni=492, dkm=12.5, two_d_time=True, ice_mask_seeding=True)
    assert len(c["ids"]) >= min_seeds
    t0 = time.perf_counter()
    out = drv.main(["-i", c["si3"], "-m", c["mm"], "-s", c["seed"], "-N", "TEST4"])
    wall = time.perf_counter() - t0
    with np.load(glob.glob("./seed/Initialized_buoys_*.npz")[0]) as z:
        nP, xPosC0, vJIt0, keep = int(z["nP"]), z["xPosC0"], z["vJIt"], z["idxKeep"]
    assert nP == out["nP"] and nP > 0.9 * min_seeds
    imaskt, _, _, _, _, xYf, xXf, _ = ncio.GetModelGrid(c["mm"])
    xYv, xXv, xYu, xXu = ncio.GetModelUVGrid(c["mm"])
    grid = dict(Yf=xYf, Xf=xXf, Yu=xYu, Xu=xXu, Yv=xYv, Xv=xXv, tmask=imaskt)
    tc, base, n0 = c["tc"], c["base"], len(c["ids"])
    tp0 = np.full(n0, base); tp0[::7] = base + 4 * 3600
    tp1 = np.full(n0, tc[-1] + 1800); tp1[::5] = base + 9 * 3600
    z1, zL = drv.record_windows(np.stack([tp0, tp1]), tc, 0, len(tc) - 1, tc[0], tc[-1], n0)
    z1, zL = z1[keep], zL[keep]
    sub = np.arange(0, nP, stride)
    ref = orc.Tracker(grid, xPosC0[sub], vJIt0[sub], rec_first=z1[sub], rec_last=zL[sub], nthreads=8)
    last = xPosC0[sub].copy()
    for jt in range(len(tc)):
        pn, mn = ref.step(jt, c["u"][jt].astype('f8'), c["v"][jt].astype('f8'), c["sic"][jt].astype('f8'))
        last[mn == 1] = pn[mn == 1]
    assert np.array_equal(out["vJIt"][sub], ref.jiT) and np.array_equal(out["iAlive"][sub], ref.alive)
    assert 0 < (ref.alive == 0).sum() < len(sub)                         # some die, most live
    _, ids2, _, yx2, mk2 = ncio.LoadNCdata(out["files"][0], krec=-1, lmask=True)
    assert np.array_equal(ids2, out["IDs"])
    ok = mk2[1][sub] == 1
    assert ok.sum() > 0.5 * len(sub)
    assert np.array_equal(yx2[1][sub][ok].astype('f4'), last[ok].astype('f4'))
    return out, wall, nP


def test_c5_shape_cli_on_a_nanuk4_shaped_mesh(tmp_path, monkeypatch):
    """NANUK4-SHAPED, not NANUK4: synthetic 566 x 492 mesh at 12.5 km, hourly records, >= 1e6 seeds under a synthetic ice
    mask (a seed is kept where `nemoSeed` would seed its nearest T-point: tmask = 1, lat >= 55, siconc >= 0.9), the
    reference's default 2-D-time mode with late starters / early stoppers.  The command line runs files in -> files
    out; every 997th kept buoy is replayed on the oracle from the seed cache the run wrote."""
    _c5_cli_case(tmp_path, monkeypatch, 1_300_000, 40, 1_000_000, 997)


def test_c5_size_cli_1e7_seeds_under_the_ice_mask(tmp_path, monkeypatch):
    """BASELINE config 5 at its SIZE (the mesh is still the NANUK4-shaped synthetic one): >= 1e7 seeds under the ice mask,
    48 hourly records, 2-D-time mode, files in -> files out through the command line (4 fused launches of the windowed
    kernel form, NetCDF-4 output at deflate 9), every 3989th kept buoy replayed on the oracle.  (tests/sweeps/demo_cli.py
    --big, 7.2 s in profiles/r02aq_cli_demo_1e7.json, promoted into the GPU suite.)"""
    out, wall, nP = _c5_cli_case(tmp_path, monkeypatch, 11_300_000, 48, 10_000_000, 3989)
    assert out["launches"]["fused_launches"] >= 2 and out["launches"]["step_launches"] <= 2
    print("C5 size: %d buoys kept of %d seeds, command line %.1f s, launches %s" % (nP, len(out["IDs"]), wall, out["launches"]))
