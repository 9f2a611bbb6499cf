"""The lanes of sitrk_run are host code only: the fused kernels of the built library are the ones profiles/traffic.json was
measured on (so bench.py's roofline.stale stays false), and the new entry point is exported."""
import json
import os

from sitrack_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_kernel_fingerprint_is_the_profiled_one():
    with open(os.path.join(ROOT, "sitrack_amd", "libsitrk.isa.json")) as f:
        built = json.load(f)["kernels"]
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        traffic = json.load(f)
    assert built["advect_run_kernel<float,1,false>"]["sha256"] == traffic["c3_fused"]["isa"]["sha256"]
    assert built["advect_step_kernel<float,1,false,512>"]["sha256"] == traffic["c3"]["isa"]["sha256"]


def test_lane_stats_is_exported():
    L = _lib.lib()
    assert hasattr(L, "sitrk_lane_stats") and "sitrk_lane_stats" in _lib._SIGNATURES
