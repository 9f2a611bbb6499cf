"""Skeletons of a label map (sitrk_skeleton_raster / sitrk_keep_skeleton) without a GPU: the numpy restatement of
the contract of include/sitrk.h that the GPU tests compare against -- thin_ref, skeleton_table_ref, nodes_ref -- with its own
checks: known answers, topology against scipy's labelling, the fixpoint, nsub and converged; and the host side of the feature:
skeleton_table, node_yx, the command lines' refusals."""
import math
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import sitrack_amd as sit
from sitrack_amd import _lib, driver as drv, features as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGHT = np.ones((3, 3), dtype=int)


# ------------------------------------------------------------------------------------------------ the restatement
def _ring(S):
    """p2 .. p9 of every pixel of the 0/1 state S (ny, nx), pixels outside counting as 0: eight shifted views of a padded copy"""
    ny, nx = S.shape
    P = np.zeros((ny + 2, nx + 2), dtype=np.uint8)
    P[1:-1, 1:-1] = S
    v = lambda dj, di: P[1 + dj:1 + dj + ny, 1 + di:1 + di + nx]
    return v(-1, 0), v(-1, 1), v(0, 1), v(1, 1), v(1, 0), v(1, -1), v(0, -1), v(-1, -1)


def sub_iteration(S, k):
    """(the state after sub-iteration k of the contract, the pixels it removed)"""
    p2, p3, p4, p5, p6, p7, p8, p9 = _ring(S)
    C = ((1 - p2) & (p3 | p4)).astype(int) + ((1 - p4) & (p5 | p6)) + ((1 - p6) & (p7 | p8)) + ((1 - p8) & (p9 | p2))
    N = np.minimum((p9 | p2).astype(int) + (p3 | p4) + (p5 | p6) + (p7 | p8), (p2 | p3).astype(int) + (p4 | p5) + (p6 | p7) + (p8 | p9))
    m = ((p6 | p7 | (1 - p9)) & p8) if k % 2 == 0 else ((p2 | p3 | (1 - p5)) & p4)
    gone = (S == 1) & (C == 1) & (N >= 2) & (N <= 3) & (m == 0)
    return np.where(gone, 0, S).astype(np.uint8), int(gone.sum())


def thin_ref(lab, max_sub):
    """(K (ny, nx) int8, nsub, converged) of the label map `lab` after the sub-iterations 0 .. max_sub-1"""
    S = (np.asarray(lab) >= 0).astype(np.uint8)
    nsub = quiet = 0
    for k in range(max_sub):
        S, n = sub_iteration(S, k)
        if n:
            nsub, quiet = k + 1, 0
        else:
            quiet += 1
            if quiet == 2:                                             # one of each kind removed nothing: the fixpoint
                break
    return S.astype(np.int8), nsub, int(max_sub >= nsub + 2)


def crossings(K):
    """X of every pixel of K"""
    r = _ring(np.asarray(K).astype(np.uint8))
    return sum(((1 - r[k]) & r[(k + 1) % 8]).astype(int) for k in range(8))


def skeleton_table_ref(lab, K):
    """the rows (value, npix, nskel, nend, njunc, north, ndiag) of every distinct value >= 0 of lab, ascending; all of them"""
    lab, K = np.asarray(lab).astype(np.int64), np.asarray(K) != 0
    ny, nx = lab.shape
    vals, npix = np.unique(lab[lab >= 0], return_counts=True)
    X = crossings(K)
    Kp = np.zeros((ny + 1, nx + 2), dtype=bool)                        # a column left and right, a row below
    Kp[:ny, 1:-1] = K
    Lp = np.full((ny + 1, nx + 2), -1, dtype=np.int64)
    Lp[:ny, 1:-1] = lab
    k = lambda dj, di: Kp[dj:dj + ny, 1 + di:1 + di + nx]
    same = lambda dj, di: k(dj, di) & (Lp[dj:dj + ny, 1 + di:1 + di + nx] == lab)
    right, down = K & same(0, 1), K & same(1, 0)
    dr = K & same(1, 1) & ~k(0, 1) & ~k(1, 0)
    dl = K & same(1, -1) & ~k(0, -1) & ~k(1, 0)
    row = np.searchsorted(vals, np.where(lab >= 0, lab, vals[0] if len(vals) else 0))
    cnt = lambda m: np.bincount(row[m], minlength=len(vals)).astype(np.int64)
    t = np.zeros((len(vals), 7), dtype=np.int64)
    t[:, 0], t[:, 1], t[:, 2] = vals, npix, cnt(K)
    t[:, 3], t[:, 4] = cnt(K & (X == 1)), cnt(K & (X >= 3))
    t[:, 5], t[:, 6] = cnt(right) + cnt(down), cnt(dr) + cnt(dl)
    return t


def nodes_ref(lab, K):
    """the rows (p, lab[p], X(p)) of the pixels of K with X != 2, in ascending p; all of them"""
    lab, K = np.asarray(lab), np.asarray(K) != 0
    X = crossings(K)
    p = np.flatnonzero(K.ravel() & (X.ravel() != 2))
    return np.stack([p, lab.ravel()[p], X.ravel()[p]], axis=1).astype(np.int64).reshape(-1, 3)


_REF = {}


def skeleton_ref(key, make, max_sub=4096):
    """the whole answer for a map, cached under `key`: make() is called once; the result is shared and must not be written to"""
    if (key, max_sub) not in _REF:
        if key not in _REF:
            _REF[key] = np.ascontiguousarray(make(), dtype=np.int32)
            _REF[key].setflags(write=False)
        lab = _REF[key]
        K, nsub, conv = thin_ref(lab, max_sub)
        r = {"labels": lab, "skel": K, "table": skeleton_table_ref(lab, K), "nodes": nodes_ref(lab, K), "nsub": nsub, "converged": conv,
             "nskel": int(K.sum())}
        r["nfeat"], r["nnode"] = len(r["table"]), len(r["nodes"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[(key, max_sub)] = r
    return _REF[(key, max_sub)]


def labels_of(mask, conn=8):
    """the canonical labels of a mask (lowest linear index of the component), from scipy"""
    mask = np.asarray(mask) != 0
    lab, n = ndimage.label(mask, structure=EIGHT if conn == 8 else None)
    out = np.full(mask.shape, -1, dtype=np.int32)
    if n:
        idx = np.arange(mask.size).reshape(mask.shape)
        low = ndimage.minimum(idx, lab, index=np.arange(1, n + 1)).astype(np.int32)
        out[mask] = low[lab[mask] - 1]
    return out


def one(mask):
    """the label map of a mask with every set pixel labelled 0"""
    return np.where(np.asarray(mask) != 0, 0, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ shapes
def plus(w, arm=40):
    n = 2 * arm + w
    m = np.zeros((n, n), dtype=np.int8)
    m[arm:arm + w, :] = 1
    m[:, arm:arm + w] = 1
    return m


def band(h, n=120):
    j, i = np.mgrid[0:n, 0:n]
    return (np.abs(j - i) <= h).astype(np.int8)


def smooth_noise(n, seed, thr=0.0):
    rng = np.random.default_rng(seed)
    return (ndimage.gaussian_filter(rng.standard_normal((n, n)), 3.0) > thr).astype(np.int8)


def full_table(mask):
    K, nsub, conv = thin_ref(one(mask), 4096)
    assert conv == 1
    t = skeleton_table_ref(one(mask), K)
    assert len(t) == 1
    return K, dict(zip(_lib.SKEL_COLS, (int(v) for v in t[0])))


# ------------------------------------------------------------------------------------------------ known answers
def test_a_row_of_nine_pixels():
    m = np.ones((1, 9), dtype=np.int8)
    K, t = full_table(m)
    assert np.array_equal(K, m)
    assert (t["nskel"], t["nend"], t["njunc"], t["north"], t["ndiag"]) == (9, 2, 0, 8, 0)
    n = nodes_ref(one(m), K)
    assert np.array_equal(n, [[0, 0, 1], [8, 0, 1]])


def test_a_diagonal_of_fifty_pixels():
    m = np.eye(50, dtype=np.int8)
    K, t = full_table(m)
    assert np.array_equal(K, m) and (t["nskel"], t["nend"], t["njunc"], t["north"], t["ndiag"]) == (50, 2, 0, 0, 49)
    K, t = full_table(m[:, ::-1])
    assert (t["nskel"], t["nend"], t["north"], t["ndiag"]) == (50, 2, 0, 49)


@pytest.mark.parametrize("w", [2, 9, 33])
def test_a_plus_has_four_ends_and_one_junction(w):
    K, t = full_table(plus(w))
    assert (t["nend"], t["njunc"]) == (4, 1)
    assert t["north"] + t["ndiag"] == t["nskel"] - 1                   # a tree: one link fewer than pixels


def test_a_square_ring_has_no_end():
    m = np.zeros((40, 40), dtype=np.int8)
    m[5:35, 5:35] = 1
    m[12:28, 12:28] = 0
    K, t = full_table(m)
    assert t["nend"] == 0 and t["north"] + t["ndiag"] == t["nskel"] and t["nskel"] > 40


def test_a_one_pixel_y_is_left_alone():
    m = np.zeros((9, 9), dtype=np.int8)
    m[4, 0:5] = 1                                                      # a stem from the left, two diagonal arms to the right
    for k in range(1, 5):
        m[4 - k, 4 + k] = 1
        m[4 + k, 4 + k] = 1
    K, t = full_table(m)
    assert np.array_equal(K, m) and (t["nend"], t["njunc"]) == (3, 1)
    assert thin_ref(one(m), 4096)[1] == 0


@pytest.mark.parametrize("n", [2, 3, 64])
def test_a_full_block_thins_to_one_pixel(n):
    K, t = full_table(np.ones((n, n), dtype=np.int8))
    assert t["nskel"] == 1 and t["npix"] == n * n and (t["nend"], t["njunc"], t["north"], t["ndiag"]) == (0, 0, 0, 0)
    assert nodes_ref(one(np.ones((n, n))), K)[:, 2].tolist() == [0]    # an isolated pixel is a node


# ------------------------------------------------------------------------------------------------ topology, fixpoint
def topology_cases():
    rng = np.random.default_rng(11)
    for dens in (0.30, 0.45, 0.55, 0.70, 0.90):
        yield "random %.2f" % dens, (rng.random((130, 200)) < dens).astype(np.int8)
    yield "smooth noise", smooth_noise(300, 5)
    for h in range(1, 21):
        yield "band %d" % h, band(h)
    for w in (2, 9, 33):
        yield "plus %d" % w, plus(w)
    yield "block 64", np.ones((64, 64), dtype=np.int8)
    yield "block 65x130", np.ones((65, 130), dtype=np.int8)


@pytest.mark.parametrize("name,mask", list(topology_cases()), ids=[n for n, _ in topology_cases()])
def test_every_component_of_the_mask_holds_exactly_one_component_of_the_skeleton(name, mask):
    K, nsub, conv = thin_ref(one(mask), 4096)
    assert conv == 1
    assert not np.any((K == 1) & (mask == 0))                          # the skeleton lies in the mask
    lab, n = ndimage.label(mask, structure=EIGHT)
    klab, kn = ndimage.label(K, structure=EIGHT)
    assert kn == n
    owner = lab[K == 1]                                                # the mask component of every skeleton pixel
    pairs = np.unique(np.stack([owner, klab[K == 1]], axis=1), axis=0)
    assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
    # the fixpoint: thinning K again removes nothing, in either kind of sub-iteration
    K2, nsub2, conv2 = thin_ref(one(K), 4096)
    assert np.array_equal(K2, K) and nsub2 == 0 and conv2 == 1


def test_a_large_random_mask_thins_quickly():
    import time
    m = (np.random.default_rng(3).random((727, 733)) < 0.6).astype(np.int8)
    t0 = time.perf_counter()
    K, nsub, conv = thin_ref(one(m), 4096)
    assert conv == 1 and 0 < K.sum() < m.sum() and time.perf_counter() - t0 < 5.0


# ------------------------------------------------------------------------------------------------ nsub, converged
def test_nsub_and_converged():
    empty = np.full((5, 7), -1, dtype=np.int32)
    assert thin_ref(empty, 1)[1:] == (0, 0) and thin_ref(empty, 2)[1:] == (0, 1) and thin_ref(empty, 4096)[1:] == (0, 1)
    blk = one(np.ones((64, 64)))
    K, nsub, conv = thin_ref(blk, 4096)
    assert conv == 1 and nsub > 8
    for cut in (1, 2, 3, 7, 8, 9, 17, nsub - 1, nsub, nsub + 1, nsub + 2):
        Kc, nc, cc = thin_ref(blk, cut)
        S = (blk >= 0).astype(np.uint8)
        last = 0
        for k in range(cut):                                           # the plain loop, no early stop
            S, n = sub_iteration(S, k)
            last = k + 1 if n else last
        assert np.array_equal(Kc, S) and nc == last
        assert cc == (1 if cut >= nc + 2 else 0)
    assert thin_ref(blk, nsub + 1)[2] == 0 and thin_ref(blk, nsub + 2)[2] == 1


def test_the_table_follows_the_labels_not_the_components():
    """two features that touch are thinned as one; the rows are per value, in ascending value, whatever the values are"""
    m = np.ones((1, 9), dtype=np.int8)
    lab = np.array([[7, 7, 7, 7, 2, 2, 2, 2, 2]], dtype=np.int32)
    K, _, _ = thin_ref(lab, 64)
    assert np.array_equal(K, m)
    t = skeleton_table_ref(lab, K)
    assert t.tolist() == [[2, 5, 5, 1, 0, 4, 0], [7, 4, 4, 1, 0, 3, 0]]   # the link between 7 and 2 belongs to neither
    assert nodes_ref(lab, K).tolist() == [[0, 7, 1], [8, 2, 1]]
    # a diagonal link is blocked by a pixel of any label
    lab = np.array([[0, 5], [-1, 0]], dtype=np.int32)
    t = skeleton_table_ref(lab, (lab >= 0))
    assert t.tolist() == [[0, 2, 2, 2, 0, 0, 0], [5, 1, 1, 0, 0, 0, 0]]   # two ends of label 0, no link; (0,1) has X = 2


# ------------------------------------------------------------------------------------------------ host logic
def test_skeleton_table_and_node_yx():
    grid = (100., -50., 2.5, 10, 20)
    t = np.array([[3, 40, 9, 2, 0, 8, 0], [17, 90, 50, 2, 0, 0, 49], [30, 4, 1, 0, 0, 0, 0]], dtype=np.int64)
    s = sit.skeleton_table(t, grid)
    assert np.array_equal(s["label"], [3, 17, 30]) and np.array_equal(s["n_end"], [2, 2, 0]) and np.array_equal(s["n_junc"], [0, 0, 0])
    assert np.array_equal(s["nskel"], [9, 50, 1]) and np.array_equal(s["npix"], [40, 90, 4])
    assert np.array_equal(s["length_km"], [2.5 * 8, 2.5 * (math.sqrt(2.) * 49), 0.])     # links, not pixels
    yx = sit.node_yx(np.array([[0, 3, 1], [25, 3, 1], [199, 17, 3]], dtype=np.int64), grid)
    assert np.array_equal(yx, [[101.25, -48.75], [103.75, -36.25], [123.75, -1.25]])
    assert sit.node_yx(np.zeros((0, 3), dtype=np.int64), grid).shape == (0, 2)
    with pytest.raises(ValueError, match="skeleton_table"):
        sit.skeleton_table(np.zeros((2, 12), dtype=np.int64), grid)
    with pytest.raises(ValueError, match="outside"):
        sit.node_yx(np.array([[200, 0, 1]]), grid)
    for bad in (dict(max_sub=0), dict(max_sub=(1 << 20) + 1), dict(maxfeat=-1), dict(maxnode=-1), dict(max_sub=1.5)):
        with pytest.raises(ValueError):
            ft.check_skeleton_args(**{**dict(max_sub=8, maxfeat=1, maxnode=1), **bad})
    with pytest.raises(ValueError, match="SkeletonRaster"):           # before any device work: no GPU is needed to refuse
        sit.SkeletonRaster(np.zeros((3, 3), dtype=np.float64))
    with pytest.raises(ValueError, match="max_sub"):
        sit.SkeletonRaster(np.zeros((3, 3), dtype=np.int32), max_sub=0)


def test_the_binding_and_the_header_agree():
    hdr = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    assert "#define SITRK_SKEL_NCOLS 7" in hdr and _lib.SKEL_NCOLS == 7 == len(_lib.SKEL_COLS)
    for name in ("sitrk_skeleton_raster", "sitrk_keep_skeleton", "sitrk_skeleton_kernel_ms"):
        assert name in _lib._SIGNATURES
    src = open(os.path.join(ROOT, "sitrack_amd", "csrc", "Makefile")).read()
    assert "sitrk_skeleton.o" in src
    c = kernel_constants()
    assert 1 <= c["kSkBatch"] <= c["kSkHalo"] and c["kSkTile"] == 64 and c["kSkThreads"] % 64 == 0


def kernel_constants():
    """the launch constants of sitrk_skeleton.hip, read from its text: name -> int"""
    src = open(os.path.join(ROOT, "sitrack_amd", "csrc", "sitrk_skeleton.hip")).read()
    out = {}
    for name in ("kSkThreads", "kSkTile", "kSkHalo", "kSkBatch", "kSkBlocks", "kSkSpanWaves", "kSkMinTrips"):
        found = re.findall(r"constexpr\s+[\w\s]+?\b%s\s*=\s*(\d+(?:\s*\*\s*\d+)*)\s*;" % name, src)
        assert len(found) == 1, (name, found)
        out[name] = math.prod(int(f) for f in found[0].split("*"))
    return out


def test_deform_skeleton_flag_parser_and_its_refusal(capsys):
    base = ["-i", "a", "-m", "b", "-s", "c"]
    feat = base + ["--deform", "10", "--deform-grid", "12.5", "--deform-features", "tot@1e-6"]
    assert drv.parse_args(base).deform_skeleton is None and drv.parse_args(feat).deform_skeleton is None
    assert drv.parse_args(feat + ["--deform-skeleton"]).deform_skeleton == 4096
    assert drv.parse_args(["--deform-skeleton"] + feat).deform_skeleton == 4096
    assert drv.parse_args(feat + ["--deform-skeleton", "17", "--deform-track"]).deform_skeleton == 17
    for bad in ("0", "-1", "1.5", "x", "", str((1 << 20) + 1)):
        with pytest.raises(SystemExit):
            drv.parse_args(feat + ["--deform-skeleton", bad])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        drv.parse_args(base + ["--deform", "10", "--deform-grid", "12.5", "--deform-skeleton"])
    err = capsys.readouterr().err
    assert "--deform-skeleton" in err and "--deform-features" in err
    f = ("tot", 1, 1e-6, 1, 8)
    assert drv.deform_skeleton_refusal(None, None) is None and drv.deform_skeleton_refusal(4096, f) is None
    assert "--deform-features" in drv.deform_skeleton_refusal(8, None)
    assert ft.skeleton_arg("1048576") == 1 << 20
    with pytest.raises(ValueError, match="--skeleton"):
        ft.skeleton_arg("0", "--skeleton")


def test_tool_refuses_skeleton_without_features(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    with pytest.raises(SystemExit, match="--skeleton.*--features"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--grid", "5", "--skeleton"])
    with pytest.raises(SystemExit, match="MAXSUB"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--grid", "5", "--features", "tot@1e-6", "--skeleton", "0"])
