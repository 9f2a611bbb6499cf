"""Features from window to window (sitrk_mesh_features_keep / sitrk_keep_* / sitrk_mesh_features_advect / sitrk_features_match,
DESIGN.md 3.18) without a GPU: the restatements of the contract that the GPU tests compare against -- match_ref, advect_ref,
kept_ref --, their self-checks against independent witnesses, sit.link_features and sit.feature_tracks on hand-made cases,
the parser of --deform-track, and the refusals of the wrappers."""
import os

import numpy as np
import pytest

import sitrack_amd as sit
from sitrack_amd import _lib
from sitrack_amd import driver as drv
from sitrack_amd import features as ft
from test_features import checkerboard, comb, label_ref, random_mask, serpentine, table_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatements
def match_ref(A, B, reach=0, dj=0, di=0):
    """(pairs (rows,3) int64 in ascending (a, b), nhit) of the contract: for every pixel p with a = A[p] >= 0 the distinct b >= 0
    among B[p + (dj, di) + (s, t)], |s|, |t| <= reach, count once for (a, b)"""
    A, B = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    ny, nx = A.shape
    jj, ii = np.nonzero(A >= 0)
    ps, bs = [], []
    for s in range(-reach, reach + 1):
        for t in range(-reach, reach + 1):
            j, i = jj + dj + s, ii + di + t
            ok = (j >= 0) & (j < ny) & (i >= 0) & (i < nx)
            b = B[j[ok], i[ok]]
            ps.append((jj[ok] * nx + ii[ok])[b >= 0])
            bs.append(b[b >= 0])
    p, b = np.concatenate(ps), np.concatenate(bs)
    if not len(p):
        return np.zeros((0, 3), dtype=np.int64), 0
    npix = ny * nx                                                     # every value is below it: (p, b) and (a, b) as one integer
    pb = np.unique(p * npix + b)                                       # S(p), one entry per member
    p, b = pb // npix, pb % npix
    nhit = len(np.unique(p))
    ab, cnt = np.unique(A.ravel()[p] * npix + b, return_counts=True)
    return np.stack([ab // npix, ab % npix, cnt], axis=1).astype(np.int64), nhit


def advect_ref(L, o0, o1, nQ):
    """(M, ncells, ncarried) of the contract, pixel by pixel"""
    L, o0, o1 = np.asarray(L), np.asarray(o0), np.asarray(o1)
    cellfeat = {}
    for q, l in zip(o0.ravel().tolist(), L.ravel().tolist()):
        if q >= 0 and l >= 0 and l < cellfeat.get(q, 1 << 40):
            cellfeat[q] = l
    assert all(0 <= q < nQ for q in cellfeat)
    M = np.array([cellfeat.get(q, -1) if q >= 0 else -1 for q in o1.ravel().tolist()], dtype=np.int32).reshape(o1.shape)
    return M, len(cellfeat), int((M >= 0).sum())


def kept_ref(labels, min_pix):
    """the map sitrk_mesh_features_keep keeps, from the labels and the restated table"""
    tab, _, _ = table_ref(labels, min_pix)
    return np.where(np.isin(labels, tab[:, 0]), labels, -1).astype(np.int32)


def permuted(labels, seed):
    """the same partition under other names: every label replaced by another value of [0, npix), not canonical any more"""
    perm = np.random.default_rng(seed).permutation(labels.size).astype(np.int32)
    return np.where(labels >= 0, perm[np.maximum(labels, 0)], -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ self-checks of the restatements
@pytest.mark.parametrize("shift", [(0, 0), (1, -2), (-3, 4)])
def test_match_ref_at_reach_0_is_the_pixel_overlap(shift):
    ny, nx = 37, 53
    A, B = label_ref(random_mask(ny, nx, 0.55, 1), 4), label_ref(random_mask(ny, nx, 0.45, 2), 8)
    dj, di = shift
    Bs = np.full((ny, nx), -1, dtype=np.int64)                         # B read at the shift, -1 outside
    j0, j1, i0, i1 = max(0, -dj), min(ny, ny - dj), max(0, -di), min(nx, nx - di)
    Bs[j0:j1, i0:i1] = B[j0 + dj:j1 + dj, i0 + di:i1 + di]
    both = (A >= 0) & (Bs >= 0)
    ab, cnt = np.unique(np.stack([A[both], Bs[both]]), axis=1, return_counts=True)
    pairs, nhit = match_ref(A, B, 0, dj, di)
    assert len(pairs) > 20 and np.array_equal(pairs[:, :2].T, ab) and np.array_equal(pairs[:, 2], cnt) and nhit == both.sum()
    swapped, _ = match_ref(B, A, 0, -dj, -di)                          # symmetric under swapping the maps and negating the shift
    back = swapped[np.lexsort((swapped[:, 0], swapped[:, 1]))]
    assert np.array_equal(back[:, [1, 0, 2]], pairs)


def test_self_match_gives_every_feature_its_own_pixels():
    for mask, conn in ((random_mask(40, 31, 0.5, 4), 8), (serpentine(9, 12), 4), (checkerboard(6, 7), 4)):
        lab = label_ref(mask, conn)
        tab, _, nact = table_ref(lab)
        pairs, nhit = match_ref(lab, lab)
        assert np.array_equal(pairs, np.stack([tab[:, 0], tab[:, 0], tab[:, 1]], axis=1)) and nhit == nact
    lab = label_ref(checkerboard(6, 7), 4)                            # dust: within one pixel every other pixel of the 3 x 3 window
    pairs, nhit = match_ref(lab, lab, reach=1)
    inner = lab[2, 2]
    assert pairs[pairs[:, 0] == inner][:, 1].tolist() == [lab[1, 1], lab[1, 3], inner, lab[3, 1], lab[3, 3]] and nhit == 21
    assert (pairs[:, 2] == 1).all()


def test_match_ref_counts_a_feature_once_per_pixel_and_nothing_outside():
    A = np.full((4, 6), -1, dtype=np.int32)
    A[1, 1:5] = 7                                                      # a bar of four pixels
    B = np.full((4, 6), -1, dtype=np.int32)
    B[2, 0:3] = 3                                                      # below its left half
    B[0, 5] = 9                                                        # off its right end, one row up
    assert match_ref(A, B, 0)[0].shape == (0, 3) and match_ref(A, B, 0)[1] == 0
    pairs, nhit = match_ref(A, B, 1)
    assert pairs.tolist() == [[7, 3, 3], [7, 9, 1]] and nhit == 4      # columns 1..3 see the 3, column 4 the 9
    pairs, nhit = match_ref(A, B, 2)
    assert pairs.tolist() == [[7, 3, 4], [7, 9, 2]] and nhit == 4
    assert match_ref(A, B, 2, dj=-4)[0].shape == (0, 3)                 # everything outside the raster
    assert match_ref(A, B, 0, dj=1, di=-1)[0].tolist() == [[7, 3, 3]]       # B[2, 0..3] under the bar


def test_advect_ref_and_the_host_helpers_agree():
    rng = np.random.default_rng(5)
    nQ = 40
    o0, o1 = rng.integers(-1, nQ, (23, 17)).astype(np.int32), rng.integers(-1, nQ, (23, 17)).astype(np.int32)
    L = kept_ref(label_ref(random_mask(23, 17, 0.5, 6), 8), 2)
    M, ncells, ncarried = advect_ref(L, o0, o1, nQ)
    got, cellfeat = ft.advect_labels(L, o0, o1, nQ)
    assert np.array_equal(got, M) and got.dtype == np.int32 and (cellfeat >= 0).sum() == ncells and 0 < ncarried == (got >= 0).sum()
    q = int(o0[L >= 0][0])
    assert cellfeat[q] == L[(o0 == q) & (L >= 0)].min()
    assert np.array_equal(ft.kept_labels(label_ref(random_mask(23, 17, 0.5, 6), 8), 2), L)
    empty, none = ft.advect_labels(L, np.full_like(o0, -1), np.full_like(o1, -1), 0)
    assert (empty == -1).all() and none.shape == (0,)
    with pytest.raises(ValueError, match="one shape"):
        ft.advect_labels(L, o0[:-1], o1, nQ)


# ------------------------------------------------------------------------------------------------ the linker
def tab(*labels):
    return np.array([[l, 1] for l in labels], dtype=np.int64).reshape(-1, 2)


def test_link_features_merge_split_tie_and_truncation():
    # a merge: 0 and 5 both go into 1; a split: 9 goes into 4 and 7 with equal counts -- the tie goes to the lowest label
    tA, tB = tab(0, 5, 9), tab(1, 4, 7)
    pairs = np.array([[0, 1, 10], [5, 1, 20], [9, 4, 3], [9, 7, 3]], dtype=np.int64)
    l = sit.link_features(pairs, tA, tB)
    assert l["parent"].tolist() == [1, 2, 2] and l["child"].tolist() == [0, 0, 1]
    assert l["nparents"].tolist() == [2, 1, 1] and l["nchildren"].tolist() == [1, 1, 2] and l["dropped"] == 0
    assert all(l[k].dtype == np.int64 for k in ("parent", "child", "nparents", "nchildren"))
    # a tie on the parent side: the lowest label
    l = sit.link_features(np.array([[0, 1, 7], [5, 1, 7]]), tA, tB)
    assert l["parent"].tolist() == [0, -1, -1] and l["child"].tolist() == [0, 0, -1]
    # min_overlap takes the weak links out
    l = sit.link_features(pairs, tA, tB, min_overlap=4)
    assert l["parent"].tolist() == [1, -1, -1] and l["child"].tolist() == [0, 0, -1] and l["nchildren"].tolist() == [1, 1, 0]
    # truncated tables: the pairs that name a label they lack are ignored and counted
    l = sit.link_features(pairs, tA[:2], tB[:2])
    assert l["parent"].tolist() == [1, -1] and l["child"].tolist() == [0, 0] and l["dropped"] == 2
    l = sit.link_features(np.zeros((0, 3), dtype=np.int64), tA, tab())
    assert l["parent"].shape == (0,) and l["child"].tolist() == [-1, -1, -1] and l["dropped"] == 0
    for bad in ((np.zeros((2, 2), dtype=np.int64), tA, tB), (pairs.astype(float), tA, tB), (pairs, tA[::-1], tB), (pairs, tA[:, 0], tB)):
        with pytest.raises(ValueError, match="link_features"):
            sit.link_features(*bad)


def test_feature_tracks_continue_only_through_mutual_links():
    tA, tB, tC = tab(0, 5, 9), tab(1, 4, 7), tab(2, 3)
    l0 = sit.link_features(np.array([[0, 1, 10], [5, 1, 20], [9, 4, 3], [9, 7, 3]]), tA, tB)
    l1 = sit.link_features(np.array([[1, 2, 5], [7, 3, 1]]), tB, tC)
    track, age = sit.feature_tracks([l0, l1], [3, 3, 2])
    # window 1: row 0 continues 5 (its parent, whose child it is), row 1 continues 9, row 2 is 9's second child: a new track
    assert [t.tolist() for t in track] == [[0, 1, 2], [1, 2, 3], [1, 3]]
    assert [a.tolist() for a in age] == [[0, 0, 0], [1, 1, 0], [2, 1]]
    assert ft.track_events(l0, track[0], track[1]) == (2, 1, 1, 1, 1) and ft.track_events(l1, track[1], track[2]) == (2, 0, 1, 0, 0)
    one, zero = sit.feature_tracks([], [4])
    assert one[0].tolist() == [0, 1, 2, 3] and zero[0].tolist() == [0, 0, 0, 0]
    assert sit.feature_tracks([], []) == ([], [])
    with pytest.raises(ValueError, match="links"):
        sit.feature_tracks([l0], [3, 3, 2])
    with pytest.raises(ValueError, match="does not fit"):
        sit.feature_tracks([l0, l1], [3, 2, 2])


# ------------------------------------------------------------------------------------------------ the binding and the wrappers
NEW = {"sitrk_mesh_features_keep": 21, "sitrk_keep_put": 7, "sitrk_keep_get": 7, "sitrk_keep_free": 2, "sitrk_mesh_features_advect": 12,
       "sitrk_features_match": 10, "sitrk_match_kernel_ms": 4, "sitrk_advect_kernel_ms": 2}


def test_the_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sitrk.h")).read()
    for name, nargs in NEW.items():
        assert "int %s(sitrk_t *h" % name in hdr and name in _lib._SIGNATURES, name
        assert len(_lib._SIGNATURES[name][1]) == nargs and hasattr(_lib.lib(), name), name
    assert "#define SITRK_KEEP_MAX %d" % _lib.KEEP_MAX in hdr and _lib.KEEP_MAX == 16
    assert "#define SITRK_MATCH_MAXREACH %d" % _lib.MATCH_MAXREACH in hdr and _lib.MATCH_MAXREACH == 2
    assert _lib._SIGNATURES["sitrk_mesh_features_keep"][1][2:] == _lib._SIGNATURES["sitrk_mesh_features"][1][1:]
    for name in ("mesh_features_keep", "keep_put", "keep_get", "keep_free", "mesh_features_advect", "features_match", "match_kernel_ms"):
        assert callable(getattr(_lib.Context, name)), name
    for name in ("features_advect", "features_match", "mesh_features"):
        assert callable(getattr(sit.IceTracker, name)), name
    assert sit.MatchLabels is ft.MatchLabels and sit.link_features is ft.link_features and sit.feature_tracks is ft.feature_tracks
    src = open(os.path.join(ROOT, "sitrack_amd", "csrc", "Makefile")).read()
    assert "sitrk_track.o" in src and os.path.exists(os.path.join(ROOT, "sitrack_amd", "csrc", "sitrk_track.hip"))


def test_wrappers_refuse_bad_arguments_before_any_device_work():
    ok = np.zeros((4, 5), dtype=np.int32)
    for args, kw in (((ok, np.zeros((4, 6), dtype=np.int32)), {}), ((ok, ok), {"reach": 3}), ((ok, ok), {"reach": -1}), ((ok, ok), {"reach": 1.5}),
                     ((ok, ok), {"dj": 32769}), ((ok, ok), {"di": -32769}), ((ok, ok), {"maxpair": -1}), ((None, ok), {}), ((ok, None), {}),
                     ((ok.astype(float), ok), {}), ((ok[0], ok[0]), {}), ((np.zeros((0, 5), dtype=np.int32),) * 2, {}),
                     ((np.zeros((1, 32769), dtype=np.int32),) * 2, {})):
        with pytest.raises(ValueError, match="MatchLabels"):
            sit.MatchLabels(*args, **kw)
    trk = object.__new__(sit.IceTracker)                               # refuses before it reaches its context
    G = (0., 0., 1., 6, 7)
    for kw in ({"keepA": 16}, {"keepB": -1}, {"keepA": 1.5}, {"reach": 3}, {"dj": -40000}, {"maxpair": -2}):
        with pytest.raises(ValueError, match="features_match"):
            sit.IceTracker.features_match(trk, kw.pop("keepA", 0), kw.pop("keepB", 1), **kw)
    for frm, to, grid in ((16, 0, G), (0, -1, G), (0, 1, (0., 0., 0., 4, 4)), ("x", 1, G)):
        with pytest.raises(ValueError, match="features_advect"):
            sit.IceTracker.features_advect(trk, 5, grid, frm, to)
    for keep in (16, -1, 2.5):
        with pytest.raises(ValueError, match="mesh_features"):
            sit.IceTracker.mesh_features(trk, 5, G, keep=keep)
    assert ft.check_match_args(2, -32768, 32768, 0) == (2, -32768, 32768, 0) and ft.check_keep(15) == 15


# ------------------------------------------------------------------------------------------------ the command line
def test_deform_track_flag_parser_and_its_three_refusals(capsys):
    base = ["-i", "a", "-m", "b", "-s", "c"]
    feat = base + ["--deform", "10", "--deform-grid", "12.5", "--deform-features", "tot@1e-6"]
    assert drv.parse_args(base).deform_track is None and drv.parse_args(feat).deform_track is None
    assert drv.parse_args(feat + ["--deform-track"]).deform_track == 1
    assert drv.parse_args(["--deform-track"] + feat).deform_track == 1
    for reach in (0, 1, 2):
        assert drv.parse_args(feat + ["--deform-track", str(reach)]).deform_track == reach
    for bad in ("3", "-1", "1.5", "x", ""):
        with pytest.raises(SystemExit):
            drv.parse_args(feat + ["--deform-track", bad])
    capsys.readouterr()
    t1 = base + ["--deform", "10", "--deform-grid", "12.5@t1", "--deform-features", "tot@1e-6", "--deform-track"]
    for argv, msg in ((base + ["--deform", "10", "--deform-grid", "12.5", "--deform-track"], "--deform-features"), (t1, "@t1")):
        with pytest.raises(SystemExit):
            drv.parse_args(argv)
        err = capsys.readouterr().err
        assert "--deform-track" in err and msg in err
    assert drv.parse_args([a.replace("@t1", "@t0") for a in t1]).deform_track == 1
    f, g = ("tot", 1, 1e-6, 1, 8), (12.5, "t0")
    assert drv.deform_track_refusal(None, None, None, 9) is None and drv.deform_track_refusal(1, f, g, 8) is None
    assert "at most 8 meshes" in drv.deform_track_refusal(1, f, g, 9)
    assert "--deform-features" in drv.deform_track_refusal(1, None, g, 1) and "@t1" in drv.deform_track_refusal(0, f, (12.5, "t1"), 1)
    assert ft.track_arg("2") == 2
    with pytest.raises(ValueError, match="--track"):
        ft.track_arg("3", "--track")


def test_tool_refuses_track_without_features(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import deformation as tool
    with pytest.raises(SystemExit, match="--track.*--features"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--grid", "5", "--track"])
    with pytest.raises(SystemExit, match="REACH"):
        tool.main(["-i", str(tmp_path / "none.nc"), "-c", "auto", "--grid", "5", "--features", "tot@1e-6", "--track", "3"])
