"""Model fields along the trajectories (--sample, sitrk_sample_*): everything that needs no GPU -- the ABI's names, the extra
variables of the trajectory files in the backend available here, the command line's argument and its batch plan."""
import os
import re

import numpy as np
import pytest

from sitrack_amd import _lib, ncio
from sitrack_amd import driver as drv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sitrk_sample_slot", "sitrk_sample_fields")


def test_header_and_signatures_carry_the_new_names():
    txt = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["sitrk_sample_slot"][1]) == 6 and len(_lib._SIGNATURES["sitrk_sample_fields"][1]) == 12
    for macro, val in (("SITRK_SAMPLE_AFTER", 0), ("SITRK_SAMPLE_ENTER", 1), ("SITRK_SAMPLE_MAX_FIELDS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), txt), macro
    assert (_lib.SAMPLE_AFTER, _lib.SAMPLE_ENTER, _lib.SAMPLE_MAX_FIELDS) == (0, 1, 8)
    for meth in ("sample_slot", "sample_fields"):
        assert callable(getattr(_lib.Context, meth))


def test_library_exports_the_new_names():
    import subprocess
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)
    exported = set(re.findall(r" T (sitrk_[a-z0-9_]+)", out))
    assert set(NEW) <= exported


def _cloud(Nt=3, Nb=37, seed=3):
    rng = np.random.default_rng(seed)
    t = (850608000 + 3600 * np.arange(Nt)).astype(int)
    ids = (300534062025510 + 7 * np.arange(Nb)).astype(np.int64)
    arr = [rng.uniform(-500, 500, (Nt, Nb)) for _ in range(4)]
    msk = (rng.uniform(size=(Nt, Nb)) > 0.2).astype('i1')
    sic = rng.uniform(0, 1, (Nt, Nb)).astype(np.float32)
    thk = rng.uniform(0, 4, (Nt, Nb)).astype(np.float32)
    sic[msk == 0] = -9999.
    thk[msk == 0] = -9999.
    thk[0, 1] = np.nan                                      # a land value survives as it is
    return t, ids, arr, msk, sic, thk


EXTRA_ATTRS = {"siconc": {"units": "1", "long_name": "ice concentration"}, "sithic": {"units": "m"}}


def _check_extras(fname, sic, thk):
    with ncio._Reader(fname) as f:
        for name, want in (("siconc", sic), ("sithic", thk)):
            assert f.has_var(name)
            got = np.asarray(f.var(name))
            assert got.dtype.newbyteorder('=') == np.float32 and got.shape == want.shape
            assert np.array_equal(np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), want.view(np.uint32)), name
            assert float(np.asarray(f.fill_of(name)).reshape(-1)[0]) == -9999.
            for k, v in EXTRA_ATTRS[name].items():
                assert f.attr(name, k) == v
        assert not f.has_attr("sithic", "long_name")
        for name in ("latitude", "longitude", "y_pos", "x_pos", "mask"):
            assert f.has_var(name)


def test_whole_array_writer_round_trips_two_extra_variables(tmp_path):
    t, ids, (Y, X, La, Lo), msk, sic, thk = _cloud()
    fn = str(tmp_path / "a.nc")
    ncio.ncSaveCloudBuoys(fn, t, ids, Y, X, La, Lo, mask=msk, corigin="T",
                          extra={"siconc": (sic, EXTRA_ATTRS["siconc"]), "sithic": (thk, EXTRA_ATTRS["sithic"])})
    _check_extras(fn, sic, thk)
    for bad in ("y_pos", "mask", "time", "id_buoy"):
        with pytest.raises(ValueError, match="collides"):
            ncio.ncSaveCloudBuoys(str(tmp_path / "bad.nc"), t, ids, Y, X, La, Lo, mask=msk, extra={bad: (sic, None)})
    with pytest.raises(ValueError, match="shape"):
        ncio.ncSaveCloudBuoys(str(tmp_path / "bad.nc"), t, ids, Y, X, La, Lo, mask=msk, extra={"sithic": (thk[:1], None)})


def test_stream_writer_round_trips_two_extra_variables_and_counts_them(tmp_path):
    t, ids, (Y, X, La, Lo), msk, sic, thk = _cloud()
    fn = str(tmp_path / "s.nc")
    w = ncio.CloudBuoysStream(fn, t, ids, with_mask=True, corigin="T", extra_names=EXTRA_ATTRS)
    for k in range(len(t)):
        w.put(k, Y[k], X[k], La[k], Lo[k], msk[k], extra={"siconc": sic[k], "sithic": thk[k]})
    w.close()
    _check_extras(fn, sic, thk)
    # a record without its extra variables is refused, and so is a file closed one record short
    w = ncio.CloudBuoysStream(str(tmp_path / "s2.nc"), t, ids, with_mask=True, extra_names=["sithic"])
    with pytest.raises(ValueError, match="extra"):
        w.put(0, Y[0], X[0], La[0], Lo[0], msk[0])
    w.put(0, Y[0], X[0], La[0], Lo[0], msk[0], extra={"sithic": thk[0]})
    with pytest.raises(ValueError, match="1 of 3"):
        w.close()
    with pytest.raises(ValueError, match="collides"):
        ncio.CloudBuoysStream(str(tmp_path / "s3.nc"), t, ids, extra_names=["x_pos"])


def test_files_without_extra_are_what_they_were(tmp_path):
    """extra absent == extra=None == the call as it was before the argument existed: same bytes, same variables"""
    t, ids, (Y, X, La, Lo), msk, sic, thk = _cloud()
    a, b = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
    ncio.ncSaveCloudBuoys(a, t, ids, Y, X, La, Lo, mask=msk, corigin="T")
    ncio.ncSaveCloudBuoys(b, t, ids, Y, X, La, Lo, mask=msk, corigin="T", extra=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    c, d = str(tmp_path / "c.nc"), str(tmp_path / "d.nc")
    for fn, kw in ((c, {}), (d, {"extra_names": None})):
        w = ncio.CloudBuoysStream(fn, t, ids, with_mask=True, corigin="T", **kw)
        for k in range(len(t)):
            w.put(k, Y[k], X[k], La[k], Lo[k], msk[k])
        w.close()
    assert open(c, "rb").read() == open(d, "rb").read()
    with ncio._Reader(a) as f:
        assert not f.has_var("siconc") and not f.has_var("sithic")


def test_sample_argument_parses():
    base = ["-i", "a.nc", "-m", "m.nc", "-s", "s.nc"]
    assert drv.parse_args(base).sample == []
    assert drv.parse_args(base + ["--sample", "siconc,sithic"]).sample == ["siconc", "sithic"]
    assert drv.parse_args(base + ["--sample", "sithic"]).sample == ["sithic"]
    with pytest.raises(SystemExit):
        drv.parse_args(base + ["--sample", "siconc,siconc"])


def test_batch_plan_cuts_at_first_records_only_with_sample():
    """2-D-time case: windows open at records 3, 7 and 12 and close at 20 and 29; 30 records, 32 slots"""
    Nt, kstrt, K = 30, 3, 32
    ends = {20 + kstrt - 3, 29 + kstrt - 3 + 3}             # model records 20 and 32 (the last one)
    firsts = {3, 7, 12}
    plain = drv.plan_batches(Nt, kstrt, K, False, 1, ends)
    smp = drv.plan_batches(Nt, kstrt, K, False, 1, ends, firsts)
    for b in (plain, smp):                                  # both cover every record once, in order, K // 2 at most per batch
        assert [jt for jt, _ in b] == list(np.cumsum([0] + [m for _, m in b])[:-1]) and sum(m for _, m in b) == Nt
        assert max(m for _, m in b) <= K // 2
    starts = lambda b: {jt + kstrt for jt, _ in b}          # noqa: E731
    after_end = {e + 1 for e in ends if e + 1 < kstrt + Nt}
    assert starts(plain) & (firsts - {kstrt} - after_end) == set()      # today's plan does not know the first records
    assert firsts <= starts(smp)                                        # with --sample every one of them opens a batch
    for b in (plain, smp):                                              # the cuts behind the records that are written stay
        assert after_end <= starts(b)
    assert len(smp) >= len(plain)
    # -F: the plan does not depend on --sample (record kstrt opens the first batch anyway)
    assert drv.plan_batches(Nt, kstrt, K, True, 4) == drv.plan_batches(Nt, kstrt, K, True, 4, (), None)
    assert drv.plan_batches(5, 0, 8, True, 1) == [(k, 1) for k in range(5)]
