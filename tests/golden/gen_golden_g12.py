"""Golden set G12: sub-stepped advection (sitrk_set_substeps) from the reference's own functions.

Run from the repository root where the reference is available: `python tests/golden/gen_golden_g12.py`.  The reference is
imported through refload.load_reference(); only numeric outputs are written.  The loop below restates the per-buoy body of
the reference driver (si3_part_tracker.py:378-490) -- velocity pick with the reference's intersect2Seg, Euler update,
IsInsideQuadrangle, CrossedEdge / NewHostCell / UpdtInd4NewCell, Survive -- and runs it `n` times per model record with
dt = rdt / n and that record's fields: the contract of include/sitrk.h for nsub = n.

Case: the G6b fast-flow case (tests/conftest.py::g6b_case: 120 x 140 warped grid, islands, drifting open water), every 5th
of its 1 500 buoys, (rdt, n) = (21600, 6) and (86400, 24), velocity rules 0 and 1, with and without per-buoy record windows.
Stored per case: per-record positions and masks (the record's output: the position after the buoy's last sub-step in that
record), host cells and alive flags after every record, kill records."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "g12_substep.npz")
FILL = -9999.0
CASES = ((21600., 6, 8), (86400., 24, 5))        # (rdt, nsub, records)
STRIDE = 5                                        # every 5th buoy of G6b


def substep_loop(ref, g, tmask, u, v, sic, yx0, jiT0, rec_first, rec_last, kstrt, Nt, rdt, nsub, strategy):
    """The reference loop body, nsub sub-steps of rdt/nsub per model record (record jrec uses slab jrec % K)."""
    util, locate, tracking = ref
    Yf, Xf, Yu, Xu, Yv, Xv = (g[k] for k in ("Yf", "Xf", "Yu", "Xu", "Yv", "Xv"))
    dt = rdt / nsub
    K = u.shape[0]
    nP = yx0.shape[0]
    alive = np.ones(nP, dtype="i1")
    pos = np.zeros((Nt + 1, nP, 2)) + FILL
    msk = np.zeros((Nt + 1, nP), dtype="i1")
    jit_rec = np.zeros((Nt + 1, nP, 2), dtype=np.int32)
    alive_rec = np.zeros((Nt + 1, nP), dtype="i1")
    kill_rec = np.full(nP, -1, dtype=np.int32)
    mesh = np.zeros((nP, 4, 2))
    still = np.zeros(nP, dtype=bool)
    cur = yx0.copy()
    jiT = jiT0.astype(np.int64).copy()
    vert = np.zeros((nP, 2, 4), dtype=np.int64)
    for b in range(nP):
        j, i = jiT[b]
        vert[b] = [[j - 1, j - 1, j, j], [i - 1, i, i, i - 1]]
    for b in range(nP):
        k0 = rec_first[b] - kstrt
        pos[k0, b] = yx0[b]
        msk[k0, b] = 1
    jit_rec[0] = jiT; alive_rec[0] = alive
    for jt in range(Nt):
        jrec = jt + kstrt
        xIC, xU, xV = sic[jrec % K], u[jrec % K], v[jrec % K]
        for b in range(nP):
            if not (alive[b] == 1 and rec_first[b] <= jrec <= rec_last[b]):
                continue
            for s in range(nsub):
                ry, rx = cur[b]
                if not still[b]:
                    vj, vi = vert[b]
                    mesh[b] = [[Yf[vj[c], vi[c]], Xf[vj[c], vi[c]]] for c in range(4)]
                jT, iT = jiT[b]
                if strategy == 0:
                    zU = 0.5 * (xU[jT, iT] + xU[jT, iT - 1])
                    zV = 0.5 * (xV[jT, iT] + xV[jT - 1, iT])
                else:
                    F = [Yf[jT, iT], Xf[jT, iT]]
                    um1 = tracking.intersect2Seg([ry, rx], F, [Yv[jT - 1, iT], Xv[jT - 1, iT]], [Yv[jT, iT], Xv[jT, iT]])
                    vm1 = tracking.intersect2Seg([ry, rx], F, [Yu[jT, iT - 1], Xu[jT, iT - 1]], [Yu[jT, iT], Xu[jT, iT]])
                    zU = xU[jT, iT - 1] if um1 else xU[jT, iT]
                    zV = xV[jT - 1, iT] if vm1 else xV[jT, iT]
                dx = zU * dt
                dy = zV * dt
                rxn = rx + dx / 1000.
                ryn = ry + dy / 1000.
                cur[b] = [ryn, rxn]
                pos[jt + 1, b] = [ryn, rxn]
                msk[jt + 1, b] = 1
                lin = locate.IsInsideQuadrangle(ryn, rxn, mesh[b])
                still[b] = lin
                if not lin:
                    ic = tracking.CrossedEdge([ry, rx], [ryn, rxn], vert[b], Yf, Xf)
                    nh = tracking.NewHostCell(ic, [ry, rx], [ryn, rxn], vert[b], Yf, Xf)
                    vert[b], jiT[b] = tracking.UpdtInd4NewCell(nh, vert[b], jiT[b])
                    if tracking.Survive(0, jiT[b], tmask, pIceC=xIC) > 0:
                        alive[b] = 0
                        kill_rec[b] = jrec
                        break
        jit_rec[jt + 1] = jiT; alive_rec[jt + 1] = alive
    return pos, msk, jit_rec, alive_rec, kill_rec


def main():
    from refload import load_reference
    from conftest import g6b_case, load_golden
    ref = load_reference()
    g6b = load_golden("g6b_traj_fast.npz")
    grid, u, v, sic = g6b_case(g6b)
    sel = np.arange(0, g6b["yx0"].shape[0], STRIDE)
    yx0, jiT0 = g6b["yx0"][sel], g6b["jiT0"][sel].astype(np.int64)
    nP = len(sel)
    kstrt = 2
    out = {"sel": sel.astype(np.int32), "kstrt": np.int64(kstrt), "cases": np.array([[r, n, t] for r, n, t in CASES])}
    rng = np.random.default_rng(1212)
    for (rdt, nsub, Nt) in CASES:
        full_first, full_last = np.full(nP, kstrt, dtype=np.int64), np.full(nP, kstrt + Nt - 1, dtype=np.int64)
        wf, wl = full_first.copy(), full_last.copy()
        late = rng.choice(nP, nP // 6, replace=False)
        wf[late] = kstrt + rng.integers(1, Nt, late.size)
        early = rng.choice(nP, nP // 6, replace=False)
        wl[early] = np.maximum(wf[early], kstrt + Nt - 1 - rng.integers(1, Nt, early.size))
        for win, (rf, rl) in (("all", (full_first, full_last)), ("win", (wf, wl))):
            tag = "n%d_%s" % (nsub, win)
            out["rec_first_" + tag], out["rec_last_" + tag] = rf.astype(np.int32), rl.astype(np.int32)
            for strat in (1, 0):
                with contextlib.redirect_stdout(io.StringIO()):
                    pos, msk, jit, alv, kr = substep_loop(ref, grid, grid["tmask"], u.astype(np.float64), v.astype(np.float64),
                                                          sic.astype(np.float64), yx0, jiT0, rf, rl, kstrt, Nt, rdt, nsub, strat)
                key = "%s_s%d" % (tag, strat)
                out["pos_" + key], out["msk_" + key], out["jiT_" + key] = pos, msk, jit
                out["alive_" + key], out["kill_rec_" + key] = alv, kr
                print("   G12 %-10s strat %d: dead %d/%d, cells moved %d" % (tag, strat, int((alv[-1] == 0).sum()), nP,
                                                                             int(np.abs(jit[-1] - jit[0]).sum())))
    np.savez_compressed(OUT, **out)
    print("%-28s %8.1f KB" % (os.path.basename(OUT), os.path.getsize(OUT) / 1024.))


if __name__ == "__main__":
    main()
