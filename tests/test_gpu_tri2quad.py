"""Quadrangles from triangles on the MI355X (sitrk_tri2quad, sitrk_tri2quad_buoys, sit.Tri2Quad, IceTracker.quads) against the
numpy restatement of the contract in tests/test_tri2quad.py: quads, tri_quad and nQ equal as integers in every case, the number
of rounds equal to the round form's."""
import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from test_deform import DAY3, check_linear_field, jittered_lattice, linear_move
from test_gpu_deform import tracked_case
from test_tri2quad import (INF, _shoelace, as_set, big_case, big_ref, candidates, chain_case, chain_constants, check_shape,
                           check_shape_fast, defect_case, params, scan_shape, tri2quad_ref, tri2quad_rounds, up)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_as_ref(ctx, yx, tris, mask=None, **kw):
    """the device against both restatements: quads, tri_quad, nQ as integers, and the rounds; returns (quads, tri_quad, rounds)"""
    quads, tri_quad, rounds = ctx.tri2quad(yx, tris, mask=mask, **kw)
    rq, rtq = tri2quad_ref(yx, tris, mask, **kw)
    assert quads.dtype == np.int32 and tri_quad.dtype == np.int32
    assert len(quads) == len(rq), (len(quads), len(rq))
    assert np.array_equal(tri_quad, rtq), np.flatnonzero(tri_quad != rtq)[:8]
    assert np.array_equal(quads, rq), np.flatnonzero((quads != rq).any(axis=1))[:8]
    _, _, rrounds = tri2quad_rounds(yx, tris, mask, **kw)
    assert rounds == rrounds, (rounds, rrounds)
    return quads, tri_quad, rounds


def test_smallest_inputs(ctx):
    yx = np.array([[0., 0.], [0., 10.], [10., 10.], [10., 0.], [2., 6.]])
    q, tq, rounds = same_as_ref(ctx, yx, np.zeros((0, 3), dtype=np.int32))
    assert q.shape == (0, 4) and tq.shape == (0,) and rounds == 0
    q, tq, rounds = same_as_ref(ctx, yx, np.array([[0, 1, 2]]))
    assert q.shape == (0, 4) and tq.tolist() == [-1]
    q, tq, rounds = same_as_ref(ctx, yx, np.array([[2, 0, 1], [3, 2, 0]]))
    assert q.tolist() == [[0, 1, 2, 3]] and tq.tolist() == [0, 0]
    q, tq, rounds = same_as_ref(ctx, yx, np.array([[0, 1, 4], [0, 4, 3]]), **params(angles=(1., 179.), ratio_min=0.))
    assert q.shape == (0, 4) and tq.tolist() == [-1, -1]                     # concave
    # a masked vertex and a point list of one triangle only
    q, tq, _ = same_as_ref(ctx, yx, np.array([[2, 0, 1], [3, 2, 0]]), mask=np.array([1, 1, 1, 0, 1]))
    assert q.shape == (0, 4) and tq.tolist() == [-1, -2]


def test_jittered_lattice_with_defects(ctx):
    yx, mask, tris = defect_case()
    quads, tri_quad, _ = same_as_ref(ctx, yx, tris, mask)
    assert 800 < len(quads) < 1024 and (tri_quad == -2).sum() > 8 and (tri_quad == -1).sum() > 8
    check_shape(yx, tris, quads, tri_quad)
    perm = np.random.default_rng(5).permutation(len(tris))
    q2, _, _ = same_as_ref(ctx, yx, tris[perm], mask)
    assert as_set(q2) == as_set(quads)
    # the same through the public function
    q3, tq3 = sit.Tri2Quad(yx, tris, mask=mask, ctx=ctx)
    assert np.array_equal(q3, quads) and np.array_equal(tq3, tri_quad)


def test_chain_takes_one_pair_per_round(ctx):
    yx, tris, kw = chain_case()
    _, _, want_rounds = tri2quad_rounds(yx, tris, **kw)
    assert want_rounds >= 32 and want_rounds == 65
    quads, tri_quad, rounds = same_as_ref(ctx, yx, tris, **kw)
    assert rounds == want_rounds and len(quads) == 64


def test_many_workgroups_and_a_contended_table(ctx):
    yx = jittered_lattice(257, 257, -2000., 1500., seed=31)
    tris = sit.lattice_cells(257, 257, "tri")
    assert len(tris) == 131072
    quads, tri_quad, rounds = same_as_ref(ctx, yx, tris)
    assert len(quads) > 50000
    ms = ctx.tri2quad_kernel_ms()
    print("257 x 257: %d quadrangles in %d rounds; adjacency %.3f, scores %.3f, rounds %.3f, compaction %.3f ms" % ((len(quads), rounds) + ms))
    assert all(m >= 0. for m in ms)


def test_more_than_one_chunk_of_block_counts(ctx):
    """quad_scan_kernel scans the counts of the compaction's blocks (kQmBlock triangles each) in chunks of kQmBlock blocks, with a
    carry in LDS from chunk to chunk: a second chunk needs more than kQmBlock^2 = 1 048 576 triangles.  The 726 x 726 jittered
    lattice has 1 051 250: 1 027 blocks, two chunks, the second of three blocks, all three with leaders.

    The comparison is the full one, against tri2quad_ref: 2.7 s on the CPU at this size, computed once (tests/test_tri2quad.py,
    which also proves the sizes without a device).  The round form, 3.0 s more, is left to the cases below 2^20 triangles: the
    rounds are over before the scan starts.  What a wrong second trip breaks: a carry that is dropped, or not added, makes the rows
    of the blocks from kQmBlock on start again at 0 -- tri_quad differs from the restatement's in every matched triangle from
    number kQmBlock^2 on (more than 100 leaders, asserted), the rows of `quads` from late_offset on are overwritten or never
    written, and the total, hence the length of `quads`, is short by late_offset; a chunk read at a wrong stride moves every
    offset behind it.  check_shape_fast pins the same from the device's output alone: the leaders in ascending triangle id hold
    0, 1, 2, ..., nQ - 1, and every row is the canonical quadrangle of its two triangles."""
    c = chain_constants()
    B = c["kQmBlock"]
    yx, tris = big_case()
    nT = len(tris)
    assert nT == 1051250 and (up(nT, B), up(up(nT, B), B)) == (1027, 2)                 # before the device is asked anything
    rq, rtq = big_ref()
    quads, tri_quad, rounds = ctx.tri2quad(yx, tris)
    assert quads.dtype == np.int32 and tri_quad.dtype == np.int32
    assert len(quads) == len(rq), (len(quads), len(rq))
    assert np.array_equal(tri_quad, rtq), np.flatnonzero(tri_quad != rtq)[:8]
    assert np.array_equal(quads, rq), np.flatnonzero((quads != rq).any(axis=1))[:8]
    lead, second = check_shape_fast(yx, tris, quads, tri_quad)
    s = scan_shape(nT, lead, c)
    print("726 x 726: %d quadrangles in %d rounds, %r" % (len(quads), rounds, s))
    assert s["chunks"] == 2 and s["late_blocks_with_leaders"] == 3 and s["late_leaders"] >= 100 and s["late_offset"] > 0
    assert tri_quad[lead[lead >= B * B][0]] == s["late_offset"] and s["late_offset"] + s["late_leaders"] == len(quads)
    assert rounds == 3                                                      # what tri2quad_rounds gives on this case, recorded
    ms = ctx.tri2quad_kernel_ms()
    assert all(m >= 0. for m in ms)


@pytest.mark.parametrize("what", ["angles", "ratio", "area", "wide"])
def test_parameter_edges(ctx, what):
    yx, mask, tris = defect_case()
    if what == "angles":
        q, _, _ = same_as_ref(ctx, yx, tris, mask, **params(angles=(90., 90.)))
        assert len(q) == 0
    elif what == "ratio":
        q, _, _ = same_as_ref(ctx, yx, tris, mask, **params(ratio_min=1.))
        assert len(q) == 0
    elif what == "area":
        live, ta, tb, v, score, key = candidates(yx, tris, mask)
        areas = 0.5 * _shoelace(np.nan_to_num(yx)[v])
        lo = float(np.median(areas))
        q, _, _ = same_as_ref(ctx, yx, tris, mask, **params(area=(lo, INF)))
        assert (areas >= lo).sum() == len(areas) - len(areas) // 2 and 0 < len(q) <= (areas >= lo).sum()
    else:
        # the angles open: the diagonal pairings compete with the lattice's
        q, _, rounds = same_as_ref(ctx, yx, tris, mask, **params(angles=(35., 145.), ratio_min=0.3))
        assert rounds >= 3 and len(q) > 900


def test_buoys_equal_tri2quad_on_fetched_positions():
    grid, u, v, sic, yx, ji = tracked_case()
    K = 8
    tris = sit.lattice_cells(25, 24, "tri").copy()
    tris[::3] = tris[::3, ::-1]
    kw = params(angles=(50., 130.), ratio_min=0.4)
    trk = sit.IceTracker(grid["Yf"], grid["Xf"], grid["Yu"], grid["Xu"], grid["Yv"], grid["Xv"], grid["tmask"], rdt=3600., nslots=K)
    try:
        c = trk.ctx
        for k in range(K):
            trk.load_record(k, u[k], v[k], sic[k])
        trk.set_buoys(yx, ji)
        c.set_resort(0)
        c.run(0, 0, 8)
        s = c.fetch()
        alive = s["alive"] == 1
        assert 5 <= (~alive).sum() < len(yx) // 2
        got = c.tri2quad_buoys(tris, **kw)
        want = c.tri2quad(s["yx"], tris, mask=alive, **kw)
        rq, rtq = tri2quad_ref(s["yx"], tris, alive, **kw)
        assert np.array_equal(want[0], rq) and np.array_equal(want[1], rtq)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert len(rq) > 100 and (rtq == -2).sum() >= 5
        q, tq = trk.quads(tris, angles=(50., 130.), ratio_min=0.4)
        assert np.array_equal(q, rq) and np.array_equal(tq, rtq)
        pq, ptq = sit.Tri2Quad(s["yx"], tris, mask=alive, angles=(50., 130.), ratio_min=0.4, ctx=c)
        assert np.array_equal(pq, rq) and np.array_equal(ptq, rtq)
        c.sort_buoys()                                                       # a re-sort in between changes nothing
        again = c.tri2quad_buoys(tris, **kw)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
        s2 = c.fetch()
        assert np.array_equal(s2["yx"], s["yx"], equal_nan=True)             # ... and nothing of the tracker moved
    finally:
        trk.close()


def test_errors_leave_the_handle_usable():
    yx, mask, tris = defect_case()
    nP = len(yx)
    ctx = _lib.Context(0)
    try:
        want = ctx.tri2quad(yx, tris, mask=mask)
        for bad_index, n_bad in ((nP, 1), (-1, 3)):
            t = tris.copy()
            t[np.arange(n_bad) * 17 + 5, 1] = bad_index
            with pytest.raises(IndexError, match=r"sitrk_tri2quad: %d triangle\(s\) have a vertex index outside \[0, %d\)" % (n_bad, nP)):
                ctx.tri2quad(yx, t, mask=mask)
            with pytest.raises(IndexError, match=r"%d triangle\(s\)" % n_bad):
                sit.Tri2Quad(yx, t, mask=mask, ctx=ctx)
            again = ctx.tri2quad(yx, tris, mask=mask)
            assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
        big = tris.astype(np.int64)
        big[7, 2] = 2 ** 40                                                  # does not fit int32: out of range all the same
        with pytest.raises(IndexError, match=r"1 triangle\(s\)"):
            ctx.tri2quad(yx, big, mask=mask)
        # too little room for the quadrangles: refused before any device work
        with pytest.raises(_lib.SitrkError, match="room for 1024 rows, 2050 triangles need 1025"):
            ctx.tri2quad(yx, tris, mask=mask, cap=len(tris) // 2 - 1)
        # the raw ABI: parameters and pointers
        lib, h, p = ctx._L, ctx._h, _lib._ptr
        t32 = np.ascontiguousarray(tris, dtype=np.int32)
        quads, tq = np.empty((len(tris) // 2, 4), dtype=np.int32), np.empty(len(tris), dtype=np.int32)

        def raw(cos_lo=0.5, cos_hi=-0.5, ratio=0.5, amin=0., amax=INF, tris_p=p(t32), tq_p=p(tq)):
            return lib.sitrk_tri2quad(h, nP, p(yx), None, len(t32), tris_p, cos_lo, cos_hi, ratio, amin, amax, len(quads), p(quads), tq_p,
                                      None, None)
        assert raw() == 0
        for kw in (dict(cos_lo=-0.5, cos_hi=0.5), dict(cos_lo=1.5), dict(cos_hi=float("nan")), dict(ratio=1.5), dict(ratio=-0.1),
                   dict(amin=2., amax=1.), dict(amin=float("nan")), dict(tris_p=None), dict(tq_p=None)):
            assert raw(**kw) == -1, kw
        with pytest.raises(_lib.SitrkError, match="no buoys"):
            ctx.tri2quad_buoys(tris)
        again = ctx.tri2quad(yx, tris, mask=mask)
        assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    finally:
        ctx.close()


def test_round_trip_through_deform_cells(ctx):
    yx, mask, tris = defect_case()
    quads, tri_quad, _ = same_as_ref(ctx, yx, tris, mask)
    yx0 = np.nan_to_num(yx)                                                  # the NaN point is in no quadrangle
    r = sit.DeformCells(yx0, linear_move(yx0, DAY3), quads, DAY3, mask0=mask, mask1=mask, ctx=ctx)
    assert r["valid"].all() and len(r["div"]) == len(quads)
    check_linear_field(np.stack([r["div"], r["shr"], r["vor"]]), r["valid"])
    assert (r["area0"] > 0).all()
