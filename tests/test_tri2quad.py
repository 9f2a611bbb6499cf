"""Quadrangles from triangles, host side: two numpy restatements of the contract of include/sitrk.h -- the
greedy form `tri2quad_ref`, the reference of tests/test_gpu_tri2quad.py, and the round form `tri2quad_rounds`, which also gives
the number of rounds the device must report -- held against each other on every case, the exact lattice, the invariances, dead
and repeated triangles, three-fold edges, the binding and sit.Tri2Quad's argument errors."""
import math
import os
import re
import sys

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from test_deform import jittered_lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def params(angles=(60., 120.), ratio_min=0.5, area=(0., INF)):
    """the library's parameters from sit.Tri2Quad's"""
    from sitrack_amd.quadmesh import _params
    return _params("", np.zeros((0, 3), dtype=np.int32), angles, ratio_min, area)


def _shoelace(P):
    """signed shoelace sum of (n, nv, 2) [y,x] points relative to vertex 0, the expression of sitrk_deform_cells"""
    nv = P.shape[1]
    dx, dy = P[:, :, 1] - P[:, :1, 1], P[:, :, 0] - P[:, :1, 0]
    A2 = np.zeros(len(P))
    for k in range(nv):
        q = (k + 1) % nv
        A2 = A2 + (dx[:, k] * dy[:, q] - dx[:, q] * dy[:, k])
    return A2


def candidates(yx, tris, mask=None, cos_lo=0.5, cos_hi=-0.5, ratio_min=0.5, area_min=0., area_max=INF):
    """The contract up to the matching, one rounded fp64 operation per symbol: (live (nT,) bool, and of every ACCEPTABLE candidate
    in ascending order of (score, key): ta < tb its triangles, quad its canonical row, score, key)."""
    yx = np.array(yx, dtype=np.float64)
    tris = np.asarray(tris).astype(np.int64).reshape(-1, 3)
    nP, nT = len(yx), len(tris)
    bad = ((tris < 0) | (tris >= nP)).any(axis=1)
    if bad.any():
        raise IndexError("%d triangle(s) have a vertex index outside [0, %d)" % (bad.sum(), nP))
    pts = yx.copy()
    if mask is not None:
        pts[np.asarray(mask) == 0, 0] = np.nan
    c_lo2, c_hi2 = np.float64(cos_lo) * abs(np.float64(cos_lo)), np.float64(cos_hi) * abs(np.float64(cos_hi))
    ratio2 = np.float64(ratio_min) * np.float64(ratio_min)
    with np.errstate(all="ignore"):
        P3 = pts[tris] if nT else np.zeros((0, 3, 2))
        live = np.isfinite(P3).all(axis=(1, 2))
        live &= (tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 2] != tris[:, 0])
        A2t = _shoelace(P3)
        live &= (A2t != 0.0) & np.isfinite(A2t)
        # half-edges of the live triangles
        t = np.repeat(np.flatnonzero(live), 3)
        k = np.tile(np.arange(3), int(live.sum()))
        a, b, apex = tris[t, k], tris[t, (k + 1) % 3], tris[t, (k + 2) % 3]
        p, q = np.minimum(a, b), np.maximum(a, b)
        key = (p << 32) | q
        order = np.argsort(key, kind="stable")
        t, apex, p, q, key = t[order], apex[order], p[order], q[order], key[order]
        _, first, count = np.unique(key, return_index=True, return_counts=True)
        first = first[count == 2]                                       # exactly two live triangles
        t1, t2, r, s, p, q, key = t[first], t[first + 1], apex[first], apex[first + 1], p[first], q[first], key[first]
        keep = r != s                                                   # the same triangle listed twice
        t1, t2, r, s, p, q, key = (x[keep] for x in (t1, t2, r, s, p, q, key))
        # canonical form
        lo, hi = np.minimum(r, s), np.maximum(r, s)
        pf = p < lo
        v = np.where(pf[:, None], np.stack([p, lo, q, hi], axis=1), np.stack([lo, p, hi, q], axis=1))
        A2 = _shoelace(pts[v])
        turn = A2 < 0.0
        v[turn] = v[turn][:, [0, 3, 2, 1]]
        P = pts[v]
        A2 = _shoelace(P)
        ok = (A2 > 0.0) & np.isfinite(A2)
        # acceptance and score
        nx = np.roll(np.arange(4), -1)
        ex, ey = P[:, nx, 1] - P[:, :, 1], P[:, nx, 0] - P[:, :, 0]
        L = ex * ex + ey * ey
        score = np.zeros(len(v))
        for c in range(4):
            m = (c + 3) % 4
            cr = ex[:, m] * ey[:, c] - ey[:, m] * ex[:, c]
            ok &= cr > 0.0
            d = (-ex[:, m]) * ex[:, c] + (-ey[:, m]) * ey[:, c]
            n = L[:, m] * L[:, c]
            sq = d * np.abs(d)
            ok &= (sq <= c_lo2 * n) & (sq >= c_hi2 * n)
            qc = (d * d) / n
            score = qc if c == 0 else np.where(qc > score, qc, score)
        ok &= L.min(axis=1) >= ratio2 * L.max(axis=1)
        area = 0.5 * A2
        ok &= (np.float64(area_min) <= area) & (area <= np.float64(area_max))
        ok &= score < INF
    ta, tb = np.minimum(t1, t2)[ok], np.maximum(t1, t2)[ok]
    v, score, key = v[ok], score[ok], key[ok]
    order = np.lexsort((key, score))
    return live, ta[order], tb[order], v[order].astype(np.int32), score[order], key[order]


def _result(nT, live, pairs, quad_of):
    """(quads, tri_quad) from the taken candidates, ordered by the smaller triangle id"""
    pairs = sorted(pairs)
    quads = np.array([quad_of[c] for _, _, c in pairs], dtype=np.int32).reshape(-1, 4)
    tri_quad = np.where(live, -1, -2).astype(np.int32)
    for row, (a, b, _) in enumerate(pairs):
        tri_quad[a] = tri_quad[b] = row
    return quads, tri_quad


def tri2quad_ref(yx, tris, mask=None, **kw):
    """The contract in its greedy form: (quads (nQ,4) int32, tri_quad (nT,) int32)."""
    live, ta, tb, v, score, key = candidates(yx, tris, mask, **kw)
    taken = np.zeros(len(live), dtype=bool)
    pairs = []
    for c, (a, b) in enumerate(zip(ta.tolist(), tb.tolist())):
        if not taken[a] and not taken[b]:
            taken[a] = taken[b] = True
            pairs.append((a, b, c))
    return _result(len(live), live, pairs, v)


def tri2quad_rounds(yx, tris, mask=None, **kw):
    """The contract in its round form, as the device runs it: (quads, tri_quad, rounds run, the last, empty one included)."""
    live, ta, tb, v, score, key = candidates(yx, tris, mask, **kw)
    nT, nC = len(live), len(ta)
    if nT == 0:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.int32), 0
    rank = np.arange(nC)                                                # candidates are in ascending (score, key)
    taken = np.zeros(nT, dtype=bool)
    pairs, rounds = [], 0
    while True:
        rounds += 1
        assert rounds <= nT // 2 + 1
        open_ = ~taken[ta] & ~taken[tb]
        best = np.full(nT, nC)                                          # every untaken triangle's pick
        np.minimum.at(best, ta[open_], rank[open_])
        np.minimum.at(best, tb[open_], rank[open_])
        mutual = np.flatnonzero(open_ & (best[ta] == rank) & (best[tb] == rank))
        if mutual.size == 0:
            break
        taken[ta[mutual]] = True
        taken[tb[mutual]] = True
        pairs += [(int(ta[c]), int(tb[c]), int(c)) for c in mutual]
    return _result(nT, live, pairs, v) + (rounds,)


def both_forms(yx, tris, mask=None, **kw):
    """the two restatements agree; returns (quads, tri_quad, rounds)"""
    q1, tq1 = tri2quad_ref(yx, tris, mask, **kw)
    q2, tq2, rounds = tri2quad_rounds(yx, tris, mask, **kw)
    assert np.array_equal(q1, q2) and np.array_equal(tq1, tq2)
    check_shape(yx, tris, q1, tq1)
    return q1, tq1, rounds


def check_shape(yx, tris, quads, tri_quad):
    """what holds for every result: each row twice in tri_quad, made of its two triangles' vertices, counter-clockwise from
    its smallest index, rows ordered by their smaller triangle"""
    tris = np.asarray(tris).reshape(-1, 3)
    assert quads.dtype == np.int32 and tri_quad.dtype == np.int32 and tri_quad.shape == (len(tris),)
    rows, cnt = np.unique(tri_quad[tri_quad >= 0], return_counts=True)
    assert np.array_equal(rows, np.arange(len(quads))) and (cnt == 2).all()
    firsts = [int(np.flatnonzero(tri_quad == r)[0]) for r in range(len(quads))]
    assert firsts == sorted(firsts)
    for r, row in enumerate(quads.tolist()):
        a, b = np.flatnonzero(tri_quad == r)
        assert set(row) == set(tris[a].tolist()) | set(tris[b].tolist()) and len(set(row)) == 4
        assert row[0] == min(row)
    if len(quads):
        assert (_shoelace(np.asarray(yx, dtype=np.float64)[quads]) > 0).all()


def check_shape_fast(yx, tris, quads, tri_quad):
    """check_shape() without a Python loop over the rows, for results of a million triangles.  The leaders -- the first
    triangle of every row, in ascending triangle id -- hold exactly 0, 1, 2, ..., nQ - 1, every row occurs exactly twice, and
    every row is made of its two triangles' vertices, counter-clockwise from its smallest index.  Returns (leaders, seconds),
    the triangle ids of the two halves of every row."""
    tris = np.asarray(tris).reshape(-1, 3)
    assert quads.dtype == np.int32 and tri_quad.dtype == np.int32 and tri_quad.shape == (len(tris),)
    tid = np.flatnonzero(tri_quad >= 0)
    val = tri_quad[tid]
    assert len(tid) == 2 * len(quads)
    order = np.argsort(val, kind="stable")                          # equal values stay in ascending triangle id
    val, tid = val[order], tid[order]
    assert np.array_equal(val, np.repeat(np.arange(len(quads)), 2))
    lead, second = tid[0::2], tid[1::2]
    assert (lead < second).all() and (np.diff(lead) > 0).all()
    six = np.concatenate([tris[lead], tris[second]], axis=1)
    assert (quads[:, :, None] == six[:, None, :]).any(axis=2).all() and (six[:, :, None] == quads[:, None, :]).any(axis=2).all()
    assert (np.diff(np.sort(quads, axis=1), axis=1) > 0).all() and (quads[:, 0] == quads.min(axis=1)).all()
    if len(quads):
        assert (_shoelace(np.asarray(yx, dtype=np.float64)[quads]) > 0).all()
    return lead, second


def chain_constants():
    """the launch constants of the deformation chain (tri2quad, mesh, coarse), read from the text of its sources: name -> int"""
    out = {}
    for fn, names in (("sitrk_quadmesh.hip", ("kQmThreads", "kQmBlock")), ("sitrk_mesh.hip", ("kMeshThreads",)),
                      ("sitrk_coarse.hip", ("kCoThreads",))):
        src = open(os.path.join(ROOT, "sitrack_amd", "csrc", fn)).read()
        for name in names:
            found = re.findall(r"constexpr\s+[\w\s]+?\b%s\s*=\s*(\d+(?:\s*\*\s*\d+)*)\s*;" % name, src)
            assert len(found) == 1, (fn, name, found)
            out[name] = math.prod(int(f) for f in found[0].split("*"))
    return out


def up(a, b):
    """ceil(a / b) of two integers"""
    return -(-a // b)


def as_set(quads):
    return set(map(tuple, np.asarray(quads).tolist()))


# the case of tests/test_gpu_tri2quad.py that takes quad_scan_kernel into a second chunk: a jittered lattice of BIG_N x BIG_N points
BIG_N = 726


def big_case():
    """(yx, tris) of the BIG_N x BIG_N jittered lattice, 2 (BIG_N - 1)^2 triangles"""
    return jittered_lattice(BIG_N, BIG_N, -2000., 1500., seed=31), sit.lattice_cells(BIG_N, BIG_N, "tri")


_BIG = {}


def big_ref():
    """tri2quad_ref of big_case(), computed once and left unchanged: (quads, tri_quad)"""
    if not _BIG:
        _BIG["ref"] = tri2quad_ref(*big_case())
    return _BIG["ref"]


def scan_shape(nT, lead, c):
    """what quad_count_kernel / quad_scan_kernel / quad_emit_kernel see of nT triangles whose leaders are `lead`: a dict with the
    blocks, the chunks of the scan, the leaders in blocks of the second and later chunks and the offset of the first such block"""
    B = c["kQmBlock"]
    blocks = up(nT, B)
    return {"blocks": blocks, "chunks": up(blocks, B), "late_leaders": int((lead // B >= B).sum()), "late_offset": int((lead < B * B).sum()),
            "late_blocks_with_leaders": len(np.unique(lead[lead // B >= B] // B))}


def defect_case():
    """The 33 x 33 jittered lattice of the deformation tests with 2048 triangles and every defect the contract names: every third
    triangle reversed, 20 points masked, one coordinate NaN, 8 triangles with a repeated vertex, one triangle listed twice, one
    extra triangle that makes an edge three-fold.  (yx, mask, tris (2050, 3))."""
    yx = jittered_lattice(33, 33, -2900., 3000., seed=11)
    rng = np.random.default_rng(21)
    pick = rng.permutation(33 * 33)
    mask = np.ones(33 * 33, dtype=np.int8)
    mask[pick[:20]] = 0
    yx[pick[20], 1] = np.nan
    tris = sit.lattice_cells(33, 33, "tri").copy()
    assert tris.shape == (2048, 3)
    tris[::3] = tris[::3, ::-1]
    flat = rng.choice(2048, 8, replace=False)
    tris[flat, 1] = tris[flat, 0]
    twice = tris[[777]]
    # cell (10, 10): its diagonal (a, c) gets a third triangle (a, c, far) -> neither of the cell's halves may use it
    a = 10 * 33 + 10
    extra = np.array([[a, a + 34, a + 36]], dtype=np.int32)
    return yx, mask, np.ascontiguousarray(np.concatenate([tris, twice, extra]))


def chain_case():
    """A strip of 129 triangles on a zigzag of 131 points, triangle i = points i, i+1, i+2, whose width grows by 1 % from point to
    point: the scores of its 128 interior edges fall strictly along the strip, so every triangle prefers its right-hand
    neighbour and each round can take only the last open pair.  (yx, tris, keywords)."""
    i = np.arange(131)
    yx = 10. * np.stack([np.where(i % 2 == 1, 1., -1.) * 0.25 * 1.01 ** i, 0.5 * i], axis=1)
    tris = np.stack([i[:-2], i[1:-1], i[2:]], axis=1).astype(np.int32)
    assert tris.shape == (129, 3)
    return yx, tris, params(angles=(30., 150.), ratio_min=0.2)


# ------------------------------------------------------------------------------------------------ the cases
def test_exact_lattice_gives_the_lattice_quadrangles():
    j, i = np.meshgrid(np.arange(9.), np.arange(9.), indexing="ij")
    yx = 10. * np.stack([j.ravel(), i.ravel()], axis=1)
    quads, tri_quad, rounds = both_forms(yx, sit.lattice_cells(9, 9, "tri"))
    want = sit.lattice_cells(9, 9, "quad")
    assert as_set(quads) == as_set(want) and len(quads) == 64
    assert np.array_equal(quads, want)                  # ... and in the lattice's order: the pairs are (2c, 2c+1)
    assert np.array_equal(tri_quad, np.repeat(np.arange(64), 2)) and rounds == 2
    # the other pairings have 45 / 135 degree corners: with the angles open they compete, with the default they do not exist
    live, ta, tb, v, score, key = candidates(yx, sit.lattice_cells(9, 9, "tri"))
    assert len(ta) == 64 and (score == 0.).all()
    live, ta, tb, v, score, key = candidates(yx, sit.lattice_cells(9, 9, "tri"), **params(angles=(40., 140.)))
    assert len(ta) > 64 and np.isclose(score.max(), 0.5)


def test_orientation_and_order_do_not_change_the_quadrangles():
    yx = jittered_lattice(12, 11, 500., -700., seed=3)
    tris = sit.lattice_cells(12, 11, "tri")
    base, _, _ = both_forms(yx, tris)
    assert len(base) > 60
    rng = np.random.default_rng(4)
    turned = tris.copy()
    turned[::2] = turned[::2, ::-1]
    turned[1::3] = np.roll(turned[1::3], 1, axis=1)
    assert as_set(both_forms(yx, turned)[0]) == as_set(base)
    perm = rng.permutation(len(tris))
    quads, tri_quad, _ = both_forms(yx, turned[perm])
    assert as_set(quads) == as_set(base)
    assert not np.array_equal(quads, base)              # the rows follow the triangles' order


def test_dead_double_and_threefold():
    yx, mask, tris = defect_case()
    quads, tri_quad, rounds = both_forms(yx, tris, mask)
    clean, clean_tq, _ = both_forms(jittered_lattice(33, 33, -2900., 3000., seed=11), sit.lattice_cells(33, 33, "tri"))
    assert 0 < len(quads) < len(clean) and rounds >= 2
    dead = tri_quad == -2
    # dead: a masked or NaN vertex, or a repeated one -- and nothing else
    bad_pt = (mask == 0) | ~np.isfinite(yx).all(axis=1)
    rep = (tris[:, 0] == tris[:, 1]) | (tris[:, 1] == tris[:, 2]) | (tris[:, 2] == tris[:, 0])
    assert np.array_equal(dead, bad_pt[tris].any(axis=1) | rep) and rep.sum() == 8 and bad_pt.sum() == 21
    assert not np.isin(quads, np.flatnonzero(bad_pt)).any()
    # the triangle listed twice: both copies alive, single, and so is every neighbour across their three-fold edges
    assert tri_quad[777] == -1 and tri_quad[2048] == -1
    # the three-fold diagonal of cell (10, 10): triangles 2*(10*32+10) and +1 share it with the extra one
    t0 = 2 * (10 * 32 + 10)
    a = 10 * 33 + 10
    for r in {int(tri_quad[t0]), int(tri_quad[t0 + 1]), int(tri_quad[2049])} - {-1, -2}:
        row = quads[r].tolist()
        assert not (a in row and a + 34 in row and abs(row.index(a) - row.index(a + 34)) == 2)
    assert tri_quad[t0] != tri_quad[t0 + 1] or tri_quad[t0] < 0
    # permuted: the same set
    perm = np.random.default_rng(5).permutation(len(tris))
    assert as_set(both_forms(yx, tris[perm], mask)[0]) == as_set(quads)
    # an index outside the points is an error, not a dead triangle
    t = tris.copy(); t[5, 2] = len(yx); t[9, 0] = -1
    with pytest.raises(IndexError, match=r"2 triangle\(s\)"):
        tri2quad_ref(yx, t, mask)


def test_smallest_inputs():
    yx = np.array([[0., 0.], [0., 10.], [10., 10.], [10., 0.], [2., 6.]])
    q, tq, rounds = both_forms(yx, np.zeros((0, 3), dtype=np.int32))
    assert q.shape == (0, 4) and tq.shape == (0,) and rounds == 0
    q, tq, rounds = both_forms(yx, np.array([[0, 1, 2]]))
    assert q.shape == (0, 4) and tq.tolist() == [-1] and rounds == 1
    # points are [y, x]: 0 (0,0), 1 (y 0, x 10), 2 (10, 10), 3 (y 10, x 0): counter-clockwise with x right and y up is 0, 1, 2, 3
    q, tq, rounds = both_forms(yx, np.array([[2, 0, 1], [3, 2, 0]]))
    assert q.tolist() == [[0, 1, 2, 3]] and tq.tolist() == [0, 0] and rounds == 2
    # concave: 0, 1, 4, 3 with 4 = (y 2, x 6) inside the triangle 0, 1, 3: the corner at 4 is reflex
    q, tq, rounds = both_forms(yx, np.array([[0, 1, 4], [0, 4, 3]]), **params(angles=(1., 179.), ratio_min=0.))
    assert q.shape == (0, 4) and tq.tolist() == [-1, -1] and rounds == 1


def test_chain_needs_one_round_per_pair():
    yx, tris, kw = chain_case()
    live, ta, tb, v, score, key = candidates(yx, tris, **kw)
    assert len(ta) == 128                               # every interior edge is acceptable
    along = np.argsort(ta + tb)                         # the edge between triangles i and i + 1
    assert (np.diff(score[along]) < 0).all()
    quads, tri_quad, rounds = both_forms(yx, tris, **kw)
    assert len(quads) == 64 and rounds == 65 and tri_quad[0] == -1


def test_parameter_edges():
    yx, mask, tris = defect_case()
    base, _, _ = both_forms(yx, tris, mask)
    none, tq, rounds = both_forms(yx, tris, mask, **params(angles=(90., 90.)))
    assert len(none) == 0 and rounds == 1
    one, _, _ = both_forms(yx, tris, mask, **params(ratio_min=1.))
    assert len(one) == 0
    live, ta, tb, v, score, key = candidates(yx, tris, mask)
    areas = 0.5 * _shoelace(np.nan_to_num(yx)[v])
    half, _, _ = both_forms(yx, tris, mask, **params(area=(float(np.median(areas)), INF)))
    assert 0 < len(half) < len(base)
    # with the angles open the diagonal pairings compete with the lattice's: several rounds, other quadrangles
    wide, _, rounds = both_forms(yx, tris, mask, **params(angles=(35., 145.), ratio_min=0.3))
    print("angles 35..145: %d quadrangles in %d rounds" % (len(wide), rounds))
    assert rounds >= 3 and len(wide) >= len(base) and as_set(wide) != as_set(base)
    # exact rectangles do pass (90, 90) and ratio_min = 1
    j, i = np.meshgrid(np.arange(4.), np.arange(4.), indexing="ij")
    sq = 10. * np.stack([j.ravel(), i.ravel()], axis=1)
    q, _, _ = both_forms(sq, sit.lattice_cells(4, 4, "tri"), **params(angles=(90., 90.), ratio_min=1.))
    assert len(q) == 9


def test_check_shape_fast_holds_what_check_shape_holds():
    yx, mask, tris = defect_case()
    quads, tri_quad = tri2quad_ref(yx, tris, mask)
    check_shape(yx, tris, quads, tri_quad)
    lead, second = check_shape_fast(yx, tris, quads, tri_quad)
    assert np.array_equal(tri_quad[lead], np.arange(len(quads))) and np.array_equal(tri_quad[second], np.arange(len(quads)))
    r = len(quads) // 2
    spoiled = []
    tq = tri_quad.copy(); tq[tq >= r] -= r; spoiled.append((quads, tq))                   # the rows start again at 0, a lost carry
    tq = tri_quad.copy(); tq[tq >= r] += 1; spoiled.append((quads, tq))                    # a row number left out
    tq = tri_quad.copy(); tq[lead[5]] = -1; spoiled.append((quads, tq))                    # a row that occurs once
    tq = tri_quad.copy(); tq[lead[[5, 6]]] = tq[lead[[6, 5]]]; tq[second[[5, 6]]] = tq[second[[6, 5]]]; spoiled.append((quads, tq))
    q = quads.copy(); q[7] = q[7, [1, 2, 3, 0]]; spoiled.append((q, tri_quad))              # not started at its smallest index
    q = quads.copy(); q[7] = q[7, [0, 3, 2, 1]]; spoiled.append((q, tri_quad))              # clockwise
    q = quads.copy(); q[7] = q[8]; spoiled.append((q, tri_quad))                            # another pair's row
    for q, tq in spoiled:
        with pytest.raises(AssertionError):
            check_shape_fast(yx, tris, q, tq)
        with pytest.raises(AssertionError):
            check_shape(yx, tris, q, tq)


def test_big_case_takes_the_block_scan_into_a_second_chunk():
    """The size conditions of tests/test_gpu_tri2quad.py's case of more than one chunk, from the restatement and the constants
    read from sitrk_quadmesh.hip, without a device.  tri2quad_ref takes 2.7 s on this case (1 051 250 triangles, 477 010
    quadrangles; 2.0 s of it are `candidates`), tri2quad_rounds 3.0 s more, measured on the CPU of the development machine."""
    c = chain_constants()
    B = c["kQmBlock"]
    yx, tris = big_case()
    nT = len(tris)
    assert nT == 2 * (BIG_N - 1) ** 2 == 1051250 and nT > B * B
    quads, tri_quad = big_ref()
    lead, second = check_shape_fast(yx, tris, quads, tri_quad)
    s = scan_shape(nT, lead, c)
    print("%d triangles, %d quadrangles: %r" % (nT, len(quads), s))
    assert (s["blocks"], s["chunks"]) == (1027, 2) and s["blocks"] > B
    # blocks of the second chunk hold leaders, and their offsets are the carry: not zero, and not what a chunk scanned alone gives
    assert s["late_blocks_with_leaders"] == s["blocks"] - B and s["late_leaders"] >= 100 and s["late_offset"] > 0
    assert s["late_offset"] + s["late_leaders"] == len(quads)
    assert tri_quad[lead[lead >= B * B][0]] == s["late_offset"]


# ------------------------------------------------------------------------------------------------ the interfaces
NAMES = ("sitrk_tri2quad", "sitrk_tri2quad_buoys", "sitrk_tri2quad_kernel_ms")


def test_symbols_are_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert "int %s(sitrk_t *h" % name in txt and name in _lib._SIGNATURES and hasattr(L, name)
    for name in ("tri2quad", "tri2quad_buoys", "tri2quad_kernel_ms"):
        assert callable(getattr(_lib.Context, name))
    assert callable(sit.Tri2Quad) and callable(sit.IceTracker.quads)


def test_tri2quad_refuses_bad_arguments_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(_lib, "Context", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    import sitrack_amd.tracking as trk
    monkeypatch.setattr(trk, "default_context", no_device)
    yx = np.zeros((6, 2))
    good = np.zeros((2, 3), dtype=np.int64)
    for tris in (np.zeros((2, 4), dtype=np.int64), np.zeros((2, 3)), np.zeros(6, dtype=np.int32)):
        with pytest.raises(ValueError, match="`tris`"):
            sit.Tri2Quad(yx, tris)
    for angles in ((120., 60.), (-1., 90.), (60., 181.), (np.nan, 90.), 60., ("a", "b"), (60., 90., 120.)):
        with pytest.raises(ValueError, match="`angles`"):
            sit.Tri2Quad(yx, good, angles=angles)
    for r in (-0.1, 1.5, np.nan, "wide"):
        with pytest.raises(ValueError, match="`ratio_min`"):
            sit.Tri2Quad(yx, good, ratio_min=r)
    for area in ((5., 1.), (np.nan, 1.), 3., (1., 2., 3.)):
        with pytest.raises(ValueError, match="`area`"):
            sit.Tri2Quad(yx, good, area=area)
    with pytest.raises(ValueError, match="`yx`"):
        sit.Tri2Quad(np.zeros((6, 3)), good)
    with pytest.raises(ValueError, match="`mask`"):
        sit.Tri2Quad(yx, good, mask=np.ones(5))
    # what goes to the library: cosines of the angles, 90 degrees exactly 0
    kw = params(angles=(60., 120.))
    assert kw["cos_lo"] == math.cos(math.radians(60.)) and kw["cos_hi"] == math.cos(math.radians(120.))
    assert params(angles=(90., 90.))["cos_lo"] == 0. and params(angles=(90., 90.))["cos_hi"] == 0.


def test_tool_argument_errors(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import generate_quad_mesh as tool
    from test_deform import linear_move, track_file, DAY3
    monkeypatch.setattr(sit, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device context was asked for")))
    yx0 = jittered_lattice(4, 5, -1500., 2000.)
    ids = 100 + 3 * np.arange(20, dtype=np.int64)[::-1]
    fin = track_file(tmp_path / "trk.nc", yx0, linear_move(yx0, DAY3), ids)
    good = str(tmp_path / "tris.npy")
    np.save(good, ids[sit.lattice_cells(4, 5, "tri")])
    out = str(tmp_path / "cells.npy")
    bad = ids[sit.lattice_cells(4, 5, "tri")].copy()
    bad[5, 1] = 101
    np.save(str(tmp_path / "bad.npy"), bad)
    with pytest.raises(SystemExit, match="id_buoy 101 "):
        tool.main(["-i", fin, "-t", str(tmp_path / "bad.npy"), "-o", out])
    with pytest.raises(SystemExit, match="-k 2 outside the 2 records"):
        tool.main(["-i", fin, "-t", good, "-k", "2", "-o", out])
    np.save(str(tmp_path / "four.npy"), np.zeros((3, 4), dtype=np.int64))
    with pytest.raises(SystemExit, match=r"\(nT,3\)"):
        tool.main(["-i", fin, "-t", str(tmp_path / "four.npy"), "-o", out])
    for opt, val in (("--angles", "120,60"), ("--angles", "60"), ("--ratio", "2"), ("--area", "5,1")):
        with pytest.raises(SystemExit, match=opt):
            tool.main(["-i", fin, "-t", good, "-o", out, opt, val])
    monkeypatch.setitem(sys.modules, "scipy.spatial", None)               # the import of scipy.spatial fails
    with pytest.raises(SystemExit, match="-t TRIS.npy"):
        tool.main(["-i", fin, "-t", "auto", "-o", out])
