"""bench.py's command line: a plain run times the headline leg only (everything else behind --full), and --dump-outputs writes
what the timed steps leave a caller with, as a fixed sample that two runs (or two builds) can be compared on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("per_record_launch", "eight_records_per_launch", "fresh_records", "value_fresh_records", "cpu_baseline", "c2",
             "c4_shard", "e2e_upload", "solo_same_shard", "e2e_broadcast")


class _FakeCtx:
    """the part of sitrack_amd.Context that dump_outputs reads: nP and fetch()"""

    def __init__(self, nP):
        self.nP = nP
        k = np.arange(nP)
        self.st = {"yx": np.stack([k * 0.5, -k * 0.25], axis=1), "jiT": np.stack([k % 4093, k % 4091], axis=1).astype(np.int32),
                   "alive": (k % 7 != 0).astype(np.int8), "kill_rec": np.where(k % 7 != 0, -1, k % 1000).astype(np.int32)}

    def fetch(self):
        return {key: val.copy() for key, val in self.st.items()}


def test_plain_run_is_the_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs == "" and a.steps == 20 and a.warmup == 5
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_small_shard_is_written_whole_and_exact(tmp_path):
    import bench
    ctx = _FakeCtx(1000)
    bench.dump_outputs(ctx, str(tmp_path / "d"))
    got = {n: np.load(str(tmp_path / "d" / (n + ".npy"))) for n in ("yx", "jiT", "alive", "kill_rec")}
    assert sorted(os.listdir(str(tmp_path / "d"))) == ["alive.npy", "jiT.npy", "kill_rec.npy", "yx.npy"]
    for n, arr in got.items():
        assert arr.dtype in (np.float32, np.float64), n
        assert np.array_equal(arr, ctx.st[n]), n                          # every buoy, in the caller's order, every value exact


def test_dump_outputs_large_shard_is_a_fixed_sample_under_64_mb(tmp_path):
    import bench
    nP = 3 * bench.DUMP_SAMPLE
    ctx = _FakeCtx(nP)
    bench.dump_outputs(ctx, str(tmp_path / "a"))
    bench.dump_outputs(ctx, str(tmp_path / "b"))
    total = 0
    for n in ("yx", "jiT", "alive", "kill_rec"):
        a = np.load(str(tmp_path / "a" / (n + ".npy")))
        b = np.load(str(tmp_path / "b" / (n + ".npy")))
        assert len(a) == bench.DUMP_SAMPLE and np.array_equal(a, b), n  # the same buoys every time
        total += os.path.getsize(str(tmp_path / "a" / (n + ".npy")))
    assert total <= 64 << 20
    # the sample is a set of distinct buoys spread over the whole shard, and its values are the fetched ones
    idx = np.load(str(tmp_path / "a" / "yx.npy"))[:, 0] / 0.5
    assert np.array_equal(idx, np.unique(idx)) and idx[0] < nP / 100 and idx[-1] > nP * 0.99
    k = idx.astype(np.int64)
    assert np.array_equal(np.load(str(tmp_path / "a" / "kill_rec.npy")), ctx.st["kill_rec"][k].astype(np.float64))


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """C2, a plain run twice with --dump-outputs: no --full leg in the line, the run's own --check replays exactly the warm-up and
    the timed steps, the dump is the state the line describes, and identical arguments give identical outputs"""
    dumps = []
    for r in range(2):
        out = str(tmp_path / ("run%d" % r))
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--config", "c2", "--steps", "64", "--warmup", "8", "--dump-outputs", out]
        if r == 0:
            cmd.append("--check")
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert not [k for k in FULL_ONLY if k in d], d.keys()
        assert d["steps"] == 64 and d["warmup"] == 8 and d["ms_per_step"] > 0 and d["dtype"] == "f64"
        assert abs(d["value"] - 100000 * 64 / (d["ms_per_step"] * 64e-3)) < 1e-6 * d["value"]
        assert d["roofline"]["records_advanced"] + d["roofline"]["one_record_launches"] == 64
        if r == 0:
            assert "check OK" in p.stderr and "after 72 steps" in p.stderr, p.stderr[-2000:]
        got = {n: np.load(os.path.join(out, n + ".npy")) for n in ("yx", "jiT", "alive", "kill_rec")}
        assert got["yx"].shape == (100000, 2) and got["yx"].dtype == np.float64
        assert int((got["alive"] != 0).sum()) == d["config"]["alive_after"]
        assert ((got["kill_rec"] == -1) == (got["alive"] != 0)).all()
        dumps.append(got)
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n
