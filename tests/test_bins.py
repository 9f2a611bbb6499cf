"""What the point-cloud modules share (sitrack_amd/csrc/sitrk_bins.h), as far as it can be said without a GPU: the header's plain
C++ part in a host program of its own, and that the five modules use it and no copy of their own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sitrack_amd", "csrc")
MODULES = ("sitrk_subsample.hip", "sitrk_overlap.hip", "sitrk_coast.hip", "sitrk_delaunay.hip", "sitrk_pairs.hip")


def test_host_primitives_against_the_loops_they_replace(tmp_path):
    """tests/c/bins_check.cpp includes sitrk_bins.h alone (no HIP) and restates the two end-bit loops, pairs' trip count and a
    fixed-trip search: key_bits under both call conventions, the order key's round trip and order at the edges of the doubles,
    lower_bound_steps over runs of every length at and around powers of two up to 2^31 + 1"""
    exe = str(tmp_path / "bins_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "bins_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    m = re.search(r"^bins_check: (\d+) checks, 0 failed$", r.stdout, re.M)
    # 20 key_bits inputs x 5; 10 round trips + 200 ordered pairs + 2; 19 lengths x (1 + 42 + 2), none of the last 2 at length 0, and
    # the 10 lengths up to 2^16 + 1 once more as arrays (1 + 42): no check was skipped
    assert m and int(m.group(1)) == 20 * 5 + (10 + 200 + 2) + (19 * 45 - 2) + 10 * 43


@pytest.mark.parametrize("name", MODULES)
def test_the_modules_keep_no_copy_of_what_they_share(name):
    src = open(os.path.join(CSRC, name)).read()
    assert '#include "sitrk_bins.h"' in src
    for gone in ("dkey", "subsample_key_to_double", "0x8000000000000000", "end_bit++", "_start_kernel("):
        assert gone not in src, (name, gone)
    assert len(re.findall(r"\bint cell_coord\(", src)) == 0
    assert "subsample_key_to_double" not in open(os.path.join(CSRC, "sitrk_internal.h")).read()
