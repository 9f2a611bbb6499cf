/*
 * sitrk.h -- C ABI of libsitrk.so: MI355X (gfx950) per-buoy advection for the
 * `sitrack` Lagrangian sea-ice tracker.
 *
 * The reference (stephanieleroux/sitrack) is pure Python and has no FFI of its
 * own; the boundary this library replaces is the body of the record loop of
 * si3_part_tracker.py:361-496 and the `sit.*` calls made from it.  Each entry
 * point below cites the reference code it stands for.  Plain pointers and
 * sizes only; host arrays are C-contiguous, order [j,i] / [y,x] / [lat,lon]
 * like the reference.  A maintainer binds it from Python with ctypes (see
 * INTEGRATION.md); sitrack_amd/_lib.py is that binding.
 *
 * Conventions
 *   - every function returns 0 on success or a negative SITRK_E* code; the
 *     text is available from sitrk_last_error().  The library never prints
 *     and never exits (the reference's `print(...); exit(0)` convention,
 *     e.g. sitrack/tracking.py:18-20,301-303, becomes an error return).
 *   - one context = one GPU = one host thread at a time (not re-entrant per
 *     handle, no global state).  Multi-GPU = one process per GPU, each with
 *     its own context and its own contiguous range of buoys.
 *   - the caller owns all host buffers; no host pointer is retained after a
 *     call returns: inputs are copied into device memory or into the library's
 *     own pinned staging before the call comes back (a C caller may free or
 *     overwrite them at once), outputs are complete on return.  Device pointers
 *     passed to *_dev entry points must stay valid until the next sitrk_sync()/fetch.
 *   - threading: one compute stream and one copy stream per context (+ an ingest
 *     stream for the opt-in asynchronous Survive derivation).  Record uploads
 *     (sitrk_push_record*, sitrk_stage_submit*) run on the copy stream out of
 *     double-buffered pinned staging and are ordered against the kernels by
 *     events only, so the next records travel while the current ones are
 *     stepped with (SURVEY 8b "async, double-buffered").
 *   - there is NO CPU fallback: without a usable HIP device sitrk_create()
 *     fails with SITRK_EHIP.
 */
#ifndef SITRK_H
#define SITRK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SITRK_VERSION 100          /* 0.1.0 */

#define SITRK_OK        0
#define SITRK_EINVAL  (-1)         /* bad argument / call order                        */
#define SITRK_EINDEX  (-2)         /* index the reference would fault on (IndexError)  */
#define SITRK_EHIP    (-3)         /* HIP runtime error (text in sitrk_last_error)     */
#define SITRK_ENOMEM  (-4)

#define SITRK_F32 0                /* field record element types */
#define SITRK_F64 1

#define SITRK_FILL (-9999.0)       /* sitrack/ncio.py:19 FillValue */

typedef struct sitrk_ctx sitrk_t;

/* ---- context ----------------------------------------------------------- */
int         sitrk_version(void);
int         sitrk_create(sitrk_t **h, int device);
int         sitrk_destroy(sitrk_t *h);
const char *sitrk_last_error(sitrk_t *h);           /* h may be NULL: last create() error */
int         sitrk_sync(sitrk_t *h);                 /* wait for all queued work          */
/* adopt an external compute stream (hipStream_t as void*), e.g. the caller's
 * torch stream; NULL restores the library's own stream */
int         sitrk_set_stream(sitrk_t *h, void *hip_stream);

/* ---- static model grid -------------------------------------------------
 * The arrays GetModelGrid / GetModelUVGrid hand to the loop
 * (sitrack/ncio.py:22-92; si3_part_tracker.py:192,196): F-, U-, V-point plane
 * coordinates [km] and the T-point land-sea mask.  Copied to the device once and
 * re-laid out as one 48-byte record per cell.  4 <= Nj <= 32767, 4 <= Ni <= 65535, Nj*Ni <= 2^29. */
int sitrk_set_grid(sitrk_t *h, int Nj, int Ni,
                   const double *Yf, const double *Xf,
                   const double *Yu, const double *Xu,
                   const double *Yv, const double *Xv,
                   const int8_t *tmask);

/* module-level constants of the reference, same defaults:
 * rdt = 3600 (si3_part_tracker.py:31), iUVstrategy = 1 (:37; 0 = cell mean, 1 = nearest U/V point),
 * rmin_conc = 0.1 (sitrack/tracking.py:4).
 * uv_strategy = 2 is an EXTRA the reference does not have (no parity claim against it): u is interpolated linearly
 * between the cell's left and right U-points and v between its lower and upper V-points, at the buoy's clamped
 * projection on the segment joining them. */
int sitrk_set_params(sitrk_t *h, double rdt, int uv_strategy, double rmin_conc);

/* Sub-stepped advection (an EXTRA the reference does not have: it does one Euler step per model record, which is right only
 * while a buoy crosses less than one cell per record, i.e. for hourly output).  1 <= nsub <= 1024 (else SITRK_EINVAL), default
 * 1; may be called before or after sitrk_set_params, in any order.  With nsub = n and period rdt:
 *   - one model record jrec advances every buoy its gate admits (alive, jrec inside [rec_first, rec_last]) by n sub-steps;
 *   - each sub-step is EXACTLY one reference step (the per-buoy body of si3_part_tracker.py:382-484) with dt = rdt / n, one
 *     rounded fp64 division done once on the host at launch: velocity pick at the buoy's current position and host cell,
 *     Euler update, IsInsideQuadrangle, CrossedEdge / NewHostCell / UpdtInd4NewCell, Survive -- all with that record's u, v
 *     and siconc (its Survive bytes);
 *   - all sub-steps of a record are gated by the same jrec; a buoy killed in sub-step s takes no further sub-step and its
 *     kill_rec is jrec.
 * Equivalently: the reference loop body run n times per record with rdt/n and the same record fields.
 * Per-record output (sitrk_fetch_record): the position after the buoy's last sub-step in that record, mask 1, if it took at
 * least one sub-step there (a buoy killed mid-record keeps its death position with mask 1); FillValue and mask 0 otherwise.
 * With nsub > 1, sitrk_run and sitrk_step launch advect_substep_kernel (counted as fused launches by sitrk_launch_stats;
 * sitrk_step = one launch of one record).  Where the fused kernels do not apply (buoys set in the two outermost rows or
 * columns, meshes beyond 2^32 bytes of geometry) the one-record kernel is launched n times per record with dt = rdt / n
 * (counted as n one-record launches).  nsub = 1 launches exactly what it launched before.
 * A host cell moves up to nsub cells per record: see the row-band and box rules below (D). */
int sitrk_set_substeps(sitrk_t *h, int nsub);

/* performance knobs; they never change results.  "xcd_remap" (0/1): each XCD walks a
 * contiguous chunk of the cell-sorted buoys; "nt_state" (0/1): non-temporal loads/stores for
 * the once-per-step position/cell streams; "sort_tile" (tile_j*256 + tile_i, 0 = row-major):
 * order of the cell sort, tile-major tiles of tile_j x tile_i cells; "locate_bruteforce" (0/1):
 * SeedInit scans the whole grid per seed like the reference instead of the bounding-sphere search; "survive_tile" (0/1): derive a
 * record's Survive bytes with the LDS-tile kernel even where the register-rolling one applies (meshes with Ni % 4 == 0);
 * "async_survive" (0/1, default 0): an uploaded record's Survive bytes are derived on the compute stream (0) or on the library's
 * ingest stream, next to the stepping of the resident records (1: measured slower under the fused loop, kept as a knob);
 * "fill_threads" (1..16, default 8): host threads that copy a pushed record of 8 MB or more into the pinned staging;
 * "patch_kb" (0..63, default 16) / "patch_margin" (0..64, default 8): KB of LDS per workgroup that the fused kernel may fill with
 * the F-points of the cells around its buoys (0 = none: every geometry read goes to global memory), and the widest margin of
 * cells it takes around their bounding box; "xcd_group" (0..4096, default 16): runs of that many consecutive workgroups of the
 * fused kernel share an XCD (its L2); "step_block" (256/512/1024): workgroup size of the one-record kernel; "fuse" (1..32):
 * consecutive resident records advanced per launch by sitrk_run (loop interchange: the buoys are independent, each lane keeps
 * its buoy in registers across the records); "subsample_block" (256..4096, powers of two, default 1024): points per workgroup of
 * sitrk_subsample_cloud's resolve kernel; "coast_bin" (1..64, default 4): bin side of the next sitrk_coast_build, in quarters of
 * sqrt(bounding-box area / segments); "delaunay_bin" (1..4, default 3): cells per reach of the next sitrk_delaunay;
 * "skeleton_batch" (1..8, default 8): sub-iterations per launch of the thinning kernel of the next skeleton call;
 * "dist_aggregate" (0/1, default 0): per-wave aggregation in the digit passes of the next distribution call;
 * "lanes" (1/2, default 2) / "lane_min_wg" (>= 1, default 7168): with lanes = 2, sitrk_run splits the cell-sorted buoys into two
 * contiguous lanes (cut at a multiple of 256 * 8 * xcd_group buoys) and queues each lane's fused launches on a stream of its own
 * -- lane 0 on the compute stream, lane 1 on the ingest stream, its first launch half as long, so that the lanes' launch
 * boundaries alternate and the chip does not drain at them -- wherever the records up to the next re-sort or the end of the call
 * hold two full launches per lane behind that short one (2.5 * fuse records), the shorter lane keeps lane_min_wg workgroups of 256
 * buoys, and the ingest stream has no Survive derivation queued.  Everywhere else, and always with lanes = 1, the launch
 * sequence is the one-lane one.  The lanes fork from and join the compute stream by events inside sitrk_run (no host wait):
 * outside it all buoy state is ordered on the compute stream as before.  sitrk_launch_stats counts record batches, whatever the
 * number of lanes; sitrk_lane_stats counts the lanes' own launches. */
int sitrk_set_tuning(sitrk_t *h, const char *knob, int value);

/* ---- model records (u_ice, v_ice, siconc) -------------------------------
 * si3_part_tracker.py:372-374 reads one (Nj,Ni) slab of each per record.
 * `nslots` records are resident on the device; a slot is one contiguous slab
 * [u | v | siconc] of 3*Nj*Ni elements of `dtype` (what one RCCL broadcast moves). */
int   sitrk_alloc_records(sitrk_t *h, int nslots, int dtype);
/* Host arrays -> slot.  Asynchronous and double-buffered: the three fields are copied into the library's pinned staging
 * (so u, v, sic may be freed or reused as soon as the call returns), the DMA into the slot is queued on the copy stream
 * behind the last kernel that reads the slot, and the record's Survive mask is queued on the compute stream behind the
 * DMA.  A second push proceeds while the first one's DMA is in flight; a third waits for the first buffer to drain. */
int   sitrk_push_record(sitrk_t *h, int slot, const void *u, const void *v, const void *sic);   /* host pointers   */
/* The same without the intermediate copy, for callers that can READ INTO pinned memory (a NetCDF reader):
 * sitrk_stage_acquire hands out the next staging buffer as three arrays of nrows x Ni elements of the records' dtype
 * (blocks until the upload that last used the buffer has drained); the caller fills them and sitrk_stage_submit queues
 * them as rows [j0, j0 + nrows) of `slot` exactly like sitrk_push_record_rows (whole record: nrows = Nj, j0 = 0).
 * The pointers belong to the library and are valid until the submit (or the release); sitrk_alloc_records and
 * sitrk_destroy free the buffers, so nothing handed out before them may be touched afterwards.
 * sitrk_stage_release gives an acquired buffer back WITHOUT uploading it (a reader that failed half-way): the next
 * acquire hands out the same buffer again.  Releasing when nothing is acquired is not an error. */
int   sitrk_stage_acquire(sitrk_t *h, int nrows, void **u, void **v, void **sic);
int   sitrk_stage_submit(sitrk_t *h, int slot, int j0, int j1);
int   sitrk_stage_release(sitrk_t *h);
int   sitrk_push_record_dev(sitrk_t *h, int slot, const void *slab_dev);                        /* device pointer: [u|v|sic] */
void *sitrk_record_ptr(sitrk_t *h, int slot);   /* device address of a slot's slab (broadcast target); NULL on error */
/* A slot whose slab was (re)written in place through sitrk_record_ptr must be committed before it is
 * stepped with: this derives the record's Survive mask (sitrack/tracking.py:62-93 evaluated once per cell:
 * rim, 5-point tmask sum, 5-point siconc mean < rmin_conc) on the library's stream.  push_record* commit
 * by themselves; a slot handed out by sitrk_record_ptr and never committed is committed by the next step. */
int   sitrk_commit_record(sitrk_t *h, int slot);

/* Row-band ingest.  A step of a buoy hosted by row jT reads u,v in rows jT-1..jT and Survive bytes in rows jT-1..jT+1,
 * which derive from siconc rows jT-2..jT+2; and a host cell moves by at most one row per record (UpdtInd4NewCell,
 * sitrack/tracking.py:257-300).  So with [jmin,jmax] = sitrk_buoy_rows() (rows of the buoys still alive; jmin > jmax
 * when none) the next step can only touch rows [jmin-2, jmax+3) of a record, and only those need to be uploaded:
 * sitrk_push_record_rows copies rows [j0,j1) of the (Nj,Ni) fields (host arrays holding just those rows) into the slot
 * and derives the Survive bytes they determine (rows j0+1..j1-2 and the domain rim); other rows keep what they held.
 * Each rank of a multi-GPU run can thus ingest only the band of its own buoys: no collective at all.
 * The library remembers which rows of a slot are valid and checks every step against them: stepping with a partly
 * uploaded slot needs sitrk_buoy_rows() to have been evaluated since sitrk_set_buoys(), and fails with SITRK_EINVAL when
 * [jmin-2-D, jmax+3+D) is not inside the uploaded rows, where a = records stepped since that evaluation (record r of a fused
 * sitrk_run counts a+r) and D = (a+1)*nsub - 1 (sitrk_set_substeps: a host cell moves by at most one row per SUB-step;
 * nsub = 1 gives D = a).  Slots are allocated with every Survive byte = kill and every field value = NaN. */
int sitrk_buoy_rows(sitrk_t *h, int32_t *jmin, int32_t *jmax);
int sitrk_push_record_rows(sitrk_t *h, int slot, int j0, int j1, const void *u_rows, const void *v_rows, const void *sic_rows);
/* same derivation for rows [j0,j1) that the caller wrote in place through sitrk_record_ptr (device-side copies) */
int sitrk_commit_record_rows(sitrk_t *h, int slot, int j0, int j1);

/* Box ingest (rows AND columns).  The same argument in both directions: a step of a buoy hosted by (jT,iT) reads u,v in
 * rows jT-1..jT / columns iT-1..iT and Survive bytes of the cells (jT-1..jT+1, iT-1..iT+1), which derive from siconc in
 * (jT-2..jT+2, iT-2..iT+2); UpdtInd4NewCell moves a host cell by at most one row and one column per record.  With
 * (jmin,jmax,imin,imax) = sitrk_buoy_box() the next step can only touch the box rows [jmin-2, jmax+3) x columns
 * [imin-2, imax+3) of a record (36 % of the cells of BASELINE config 3, whose buoys fill the central 60 % x 60 %):
 *   sitrk_push_record_box     host arrays -> slot (gathered into the library's pinned staging by a few threads, then three
 *                             strided DMAs), + the Survive bytes the box determines.  u_box, v_box, sic_box address element
 *                             (j0,i0); consecutive rows of the box are `ld` elements apart in the caller's arrays: ld = i1-i0
 *                             for arrays that hold exactly the box, ld = Ni for pointers into whole (Nj,Ni) fields
 *   sitrk_stage_acquire_box / sitrk_stage_submit_box   the same for a reader that fills the pinned staging itself
 *                             (a NetCDF hyperslab read of si3_part_tracker.py:372-374 restricted to the box)
 *   sitrk_commit_record_box   the slab already sits in device memory (written through sitrk_record_ptr: an RCCL broadcast, a
 *                             device-side producer): derive the Survive bytes of the box only, and treat the slot as holding
 *                             that box from now on
 * The library remembers the box a slot holds and checks every step against it exactly like the row bands: a records after
 * sitrk_buoy_box() the slot must hold rows [jmin-2-D, jmax+3+D) and columns [imin-2-D, imax+3+D), D = (a+1)*nsub - 1 (= a
 * without sub-steps), else SITRK_EINVAL.  The *age of sitrk_buoy_box_end counts records, not sub-steps.
 * sitrk_buoy_rows() evaluates the columns too (a row band is a box of full width). */
int sitrk_buoy_box(sitrk_t *h, int32_t *jmin, int32_t *jmax, int32_t *imin, int32_t *imax);
int sitrk_push_record_box(sitrk_t *h, int slot, int j0, int j1, int i0, int i1, const void *u_box, const void *v_box, const void *sic_box,
                          int64_t ld);
/* sitrk_buoy_box without stalling the stream: _begin queues the reduction behind the work already queued on the compute stream,
 * _end waits for that point only (launches queued after the begin keep the GPU busy) and adopts the result -- the box then
 * counts as evaluated at the begin; *age (optional) = records stepped since the begin.  One evaluation in flight at a time. */
int sitrk_buoy_box_begin(sitrk_t *h);
int sitrk_buoy_box_end(sitrk_t *h, int32_t *jmin, int32_t *jmax, int32_t *imin, int32_t *imax, int32_t *age);
int sitrk_stage_acquire_box(sitrk_t *h, int nrows, int ncols, void **u, void **v, void **sic);
int sitrk_stage_submit_box(sitrk_t *h, int slot, int j0, int j1, int i0, int i1);
int sitrk_commit_record_box(sitrk_t *h, int slot, int j0, int j1, int i0, int i1);
/* the same box of the nrec records in slots (slot0 + k) % nslots, k < nrec (the slots a sitrk_run of nrec records from slot0
 * steps with), derived by ONE launch: a box of a record is ~10 us of memory traffic, of the order of a dependent dispatch */
int sitrk_commit_records_box(sitrk_t *h, int slot0, int nrec, int j0, int j1, int i0, int i1);
/* the same on the library's INGEST stream instead of the compute stream: the derivation runs next to the launches that step with
 * OTHER slots -- behind the last launch that read these slots' bytes, in front of the first one that will (knob "async_survive": the
 * same for uploaded records).  For slabs that are COMPLETE in device memory when the call is made: nothing may still be writing them.
 * Measured (bench.py --fresh-overlap): slower than the plain call under the fused loop -- an option, not the default path. */
int sitrk_commit_records_box_async(sitrk_t *h, int slot0, int nrec, int j0, int j1, int i0, int i1);

/* ---- buoys ---------------------------------------------------------------
 * State of si3_part_tracker.py:324-330 reduced to what the loop reads:
 * yx = xPosC[jt] (nP,2) km; jiT = vJIt (nP,2); rec_first/rec_last =
 * z1stModelRec/zLstModelRec (:264-265), NULL = every record.  VRTCS is a pure
 * function of vJIt (sitrack/locate.py:320-321, tracking.py:257-300) and is not
 * stored.  All buoys start alive.  Requires 1 <= jT <= Nj-2, 1 <= iT <= Ni-2
 * (outside it the reference indexes out of range) -> SITRK_EINDEX. */
int sitrk_set_buoys(sitrk_t *h, int64_t nP, const double *yx, const int32_t *jiT,
                    const int32_t *rec_first, const int32_t *rec_last);

/* Buoys that arrive with a history (handed over by another rank when the ranks' latitude bands are re-balanced): right after
 * sitrk_set_buoys, mark the buoys with alive[k] == 0 as dead and give every DEAD buoy its kill record back (kill_rec[k]), so
 * that sitrk_fetch / sitrk_fetch_record answer as they did on the rank that stepped them before.  Invariant of the library:
 * a buoy is alive exactly when its kill record is -1 -- kill_rec[k] of a buoy with alive[k] != 0 is ignored (stored as -1). */
int sitrk_restore_state(sitrk_t *h, const int8_t *alive, const int32_t *kill_rec);

/* re-order the device-resident buoys by host cell (coalescing); results are
 * always returned in the caller's original order.  resort_every > 0 re-sorts
 * automatically every that many steps (default 512; 0 = never). */
int sitrk_sort_buoys(sitrk_t *h);
int sitrk_set_resort(sitrk_t *h, int resort_every);

/* One model record for every buoy: the body of `for jP in range(nP)`
 * (si3_part_tracker.py:378-490): gate (:380), velocity pick (:423-441,
 * sitrack/tracking.py:44-58), Euler update (:452-458), IsInsideQuadrangle
 * (:466, locate.py:49-78), CrossedEdge / NewHostCell / UpdtInd4NewCell / Survive
 * (:474-484, tracking.py:62-93,182-305).  `slot` = resident record used as
 * model record `jrec`.  Asynchronous. */
int sitrk_step(sitrk_t *h, int slot, int jrec);

/* nsteps records jrec0, jrec0+1, ... using slots (slot0 + k) % nslots; consecutive resident records go into one launch
 * (knob "fuse"; never across a re-sort or the slot ring).  Buoy sets with per-buoy record windows run the kernel form
 * without the window test for every launch whose records lie inside all windows. */
int sitrk_run(sitrk_t *h, int slot0, int jrec0, int nsteps);
/* What sitrk_run / sitrk_step really launched since the last reset: fused launches of advect_run_kernel (or, with
 * nsub > 1, of advect_substep_kernel), the records they advanced in total (a launch is cut short at a re-sort and at the end of a run), and one-record launches of
 * advect_step_kernel.  Any pointer may be NULL.  bench.py prices its roofline per launch from these. */
int sitrk_launch_stats(sitrk_t *h, int reset, int64_t *fused_launches, int64_t *fused_records, int64_t *step_launches);
/* ... and, of those, what went on two lanes (knob "lanes"): segments (runs of records between two joins) and the kernel
 * launches the two lanes queued for them.  Both stay 0 with lanes = 1.  Any pointer may be NULL. */
int sitrk_lane_stats(sitrk_t *h, int reset, int64_t *lane_segments, int64_t *lane_launches);

/* ---- sub-stepped advection with the fields interpolated in time -------------------
 * An EXTRA the reference does not have.  sitrk_run advances every sub-step of a record with that record's u, v: a velocity
 * that is piecewise constant in time.  sitrk_run_tlerp steps the same records jrec0 + k, k < nsteps, from the same slots
 * (slot0 + k) % nslots with the current nsub = n >= 1 and dt = rdt / n (the same single rounded division), but blends the
 * velocity candidates of every sub-step linearly in time between the record and its neighbour.
 * `phase` in [0,1] = the fraction of its step interval at which a record is valid: 0.5 for time means centred on the interval
 * (what NEMO writes), 0 for snapshots at its start.  For sub-step s of a record, in fp64, one rounded operation per symbol,
 * no FMA:
 *     tau   = (double)(2s+1) / (double)(2n)
 *     theta = tau - phase
 *     theta < 0 : the partner is record jrec-1 in slot (slot-1+nslots) % nslots, w = -theta
 *     theta > 0 : the partner is record jrec+1 in slot (slot+1) % nslots,        w =  theta
 *     theta == 0: no partner
 * and no partner either for the record before k == 0 unless have_prev, nor for the record behind k == nsteps-1 unless
 * have_next.  Each of the four candidates u[jT,iT-1], u[jT,iT], v[jT-1,iT], v[jT,iT] of the buoy's current host cell becomes
 *     F = (double)f_cur + w * ((double)f_partner - (double)f_cur)
 * and F = (double)f_cur exactly where there is no partner (no arithmetic: a non-finite value of an unused partner cannot leak
 * in).  The sub-step is then the sub-step of sitrk_set_substeps with F in place of the record's values: uv_strategy 0 / 1 / 2
 * (the pick of strategy 1 is geometric, so pick and blend commute), P + (F*dt)/1000., inside test, crossing, re-hosting.
 * Never interpolated: the Survive bytes (always record jrec's own), the record-window gate (jrec) and kill_rec.
 * Equivalently: the reference loop body run n times per record with rdt/n, the blended fields u_s, v_s and siconc of record
 * jrec.  Bit for bit: with no partner anywhere the result is sitrk_run's with the same nsub; so it is with phase = 0.5, n = 1.
 * sitrk_fetch_record, sitrk_sample_*, sitrk_deform_* and sitrk_coast_dist_buoys behave after it exactly as after sitrk_run.
 * Host rules: nsteps + (have_prev?1:0) + (have_next?1:0) <= nslots.  A partner slot that the sub-steps read (a phase can
 * leave one side unused: phase 0 never looks back) is checked like the slot of the record it serves -- the same age, hence
 * the same D of the row-band / box rule: a box that holds record jrec-1 for its own step is nsub cells too small as a partner
 * of jrec -- made ready like it, and counts as read by the launch: a later upload into it waits for the kernel.  The periodic
 * re-sort is honoured as in sitrk_run; launches are counted as fused launches / fused records; one lane only
 * (sitrk_lane_stats does not move).  One call and record-by-record calls give the same bits.
 * SITRK_EINVAL: phase outside [0,1] (NaN included), nsteps < 0, a bad slot, missing buoys or records, too few slots, and a buoy
 * set to which the fused kernels do not apply (buoys in the two outermost rows/columns, geometry beyond 2^32 bytes: the
 * one-record kernel cannot blend); the handle stays usable. */
int sitrk_run_tlerp(sitrk_t *h, int slot0, int jrec0, int nsteps, double phase, int have_prev, int have_next);

/* Current state in the caller's buoy order (any pointer may be NULL):
 * yx (nP,2) current position; jiT (nP,2) = vJIt; alive (nP) = iAlive;
 * kill_rec (nP) = model record at which the buoy was killed, -1 if alive. */
int sitrk_fetch(sitrk_t *h, double *yx, int32_t *jiT, int8_t *alive, int32_t *kill_rec);

/* What the reference stores for the record that followed model record `jrec`
 * (xPosC[jt+1], xmask[jt+1], si3_part_tracker.py:459-460): the position where
 * the buoy stepped at `jrec`, FillValue and mask 0 elsewhere.  Valid right
 * after the step of `jrec`.  latlon (optional) = CartNPSkm2Geo1D of yx_rec
 * (:493; dead buoys' -9999 km are converted too, like the reference). */
int sitrk_fetch_record(sitrk_t *h, int jrec, double *yx_rec, int8_t *mask, double *latlon);

/* ---- model fields along the trajectories ----------------------------------
 * An EXTRA the reference does not have (its files hold positions only): the value of a 2-D field X on the T-grid at the
 * host cell of every buoy, for a model record jrec.
 *   mode SITRK_SAMPLE_AFTER  valid right after the step of jrec, like sitrk_fetch_record: out[k] = X[jT_k, iT_k], the buoy's
 *                            host cell after the step (with nsub > 1: after its last sub-step in jrec), for exactly the buoys
 *                            for which sitrk_fetch_record(jrec) gives mask 1 -- those that stepped at jrec, a buoy killed by
 *                            jrec included: it is sampled in the cell that killed it.  The same device code decides both.
 *   mode SITRK_SAMPLE_ENTER  valid before the step of jrec: out[k] = X[cell_k] for the buoys that are alive and, in sets
 *                            with record windows, have rec_first == jrec (without windows: every alive buoy) -- the seeds,
 *                            sampled in the record they start in (row 0 of the output files).
 * Every other buoy gets SITRK_FILL.  No interpolation and no land masking: the value is the bit pattern found in the field,
 * whatever a land point holds (NaN payloads included).  out has the fields' element type (f4 -> f4, f8 -> f8) and the
 * caller's buoy order.  Both calls are queued on the compute stream behind the stepping already queued and return with out
 * filled; they wait for the compute stream only and use none of the ingest's pinned staging, so a record upload in flight
 * (sitrk_stage_submit*, sitrk_push_record*) goes on undisturbed.
 * A buoy that must be sampled and whose host cell lies outside the box the field covers -> SITRK_EINVAL, their number in
 * sitrk_last_error, out unspecified.  SITRK_EINVAL also for a bad mode, field, nf or dtype, an empty or out-of-range box, no
 * buoys, and a slot that holds no record. */
#define SITRK_SAMPLE_AFTER 0
#define SITRK_SAMPLE_ENTER 1
#define SITRK_SAMPLE_MAX_FIELDS 8  /* design limit: the field pointers travel as kernel arguments */
/* a field of a RESIDENT record: field = 0 u, 1 v, 2 siconc -- the raw slab value at [jT,iT] (u, v: the U-/V-point east /
 * north of the T-point; not the velocity the pick chose).  Checked against the box the library remembers for the slot (box
 * ingest): a slot is never read outside it, so stale rows and columns cannot be sampled just because they hold numbers.
 * Waits for an upload of the slot still in flight.  out: nP elements of the records' dtype. */
int sitrk_sample_slot(sitrk_t *h, int slot, int jrec, int mode, int field, void *out);
/* 1 <= nf <= SITRK_SAMPLE_MAX_FIELDS host fields of `dtype` (SITRK_F32 / SITRK_F64, independent of the records') given as
 * boxes rows [j0,j1) x columns [i0,i1): boxes[f] addresses element (j0,i0), consecutive rows are ld elements apart (ld =
 * i1-i0 for arrays that hold exactly the box, ld = Ni for pointers into whole (Nj,Ni) fields).  One pass over the buoys
 * samples all nf fields.  out: (nf, nP) of dtype.  The device copies of the boxes live in the context's transient scratch
 * (never read by the stepping) and are reused by the next call: resident memory grows by no more than the boxes. */
int sitrk_sample_fields(sitrk_t *h, int jrec, int mode, int nf, int dtype, int j0, int j1, int i0, int i1,
                        const void *const *boxes, int64_t ld, void *out);

/* ---- deformation rates of buoy triangles and quadrangles ---------------------
 * An EXTRA the reference does not have (its tracking12 file is written for the RGPS-style deformation scripts of another
 * project): divergence, shear and vorticity of cells whose vertices are buoys, from the buoys' positions at two times.  No
 * parity claim is made against any other code; the contract below is this library's own.
 * A cell is nv = 3 or 4 buoy indices in the caller's buoy order, in either orientation; cells is (nC, nv) int32.
 * Per cell, with the t0 positions (y_k, x_k) and the t1 positions (Y_k, X_k) of its vertices in km, the elapsed time T in
 * seconds and k' = (k+1) mod nv, everything in fp64, one rounded operation per symbol, no fused multiply-add, this order:
 *     dx_k = x_k - x_0 ; dy_k = y_k - y_0                  (t0, relative to vertex 0)
 *     u_k  = (X_k - x_k) / T ; v_k = (Y_k - y_k) / T       [km/s]
 *     A2 = Suy = Sux = Svy = Svx = 0.0 ; then for k = 0 .. nv-1 in this order:
 *       A2  = A2  + (dx_k*dy_k' - dx_k'*dy_k)
 *       Suy = Suy + (u_k' + u_k)*(dy_k' - dy_k) ;  Sux = Sux + (u_k' + u_k)*(dx_k' - dx_k)
 *       Svy = Svy + (v_k' + v_k)*(dy_k' - dy_k) ;  Svx = Svx + (v_k' + v_k)*(dx_k' - dx_k)
 *     u_x = Suy/A2 ; u_y = -(Sux/A2) ; v_x = Svy/A2 ; v_y = -(Svx/A2)        [1/s]
 *     div = u_x + v_y ; vor = v_x - u_y ; shr = sqrt((u_x - v_y)*(u_x - v_y) + (u_y + v_x)*(u_y + v_x))
 *     area0 = 0.5*|A2| ; area1 = 0.5*|A2'|   (A2' = the same shoelace sum on the t1 positions relative to (Y_0, X_0))   [km^2]
 * This is the line-integral (Green) estimate on the t0 contour: exact for a velocity field that is linear in space, and, A2
 * being signed, independent of the orientation.  out (5, nC) fp64 = div, shr, vor, area0, area1; valid (nC) int8.
 * A cell is INVALID -- valid = 0 and all five values SITRK_FILL -- if a vertex is invalid at t0 or at t1, if any of its
 * 4 nv coordinates is not finite, if A2 == 0 or if A2 is not finite.  No filter on the cells' shape: area0 and area1 are there
 * for the caller's.  *nvalid (may be NULL) = number of valid cells.
 * A vertex index outside [0, nP) is an error, not an invalid cell: SITRK_EINDEX with the number of offending cells in
 * sitrk_last_error (out and valid unspecified); such an index is never dereferenced and the handle stays usable.
 * Only + - * / are bit-reproducible from the order above; sqrt is the device's.
 *
 * sitrk_deform_cells: host arrays yx0, yx1 (nP,2) [y,x] km, mask0 / mask1 (nP) int8, 0 = invalid vertex at t0 / t1 (NULL:
 * every buoy valid).  Synchronous on the handle's stream; nC == 0 is valid.  Uses the context's transient scratch only (never
 * read by the stepping): the grid, buoys and records of a tracker on the same handle are left as they were.  SITRK_EINVAL
 * for nv not in {3,4}, T not finite or <= 0 and missing pointers. */
int sitrk_deform_cells(sitrk_t *h, int64_t nP, const double *yx0, const double *yx1, const int8_t *mask0, const int8_t *mask1,
                       int64_t nC, int nv, const int32_t *cells, double T, double *out, int8_t *valid, int64_t *nvalid);
/* The same without moving a position to the host.  sitrk_deform_mark is queued on the compute stream behind the stepping
 * already queued and snapshots the current fp64 positions of all buoys, in the caller's order, into a device buffer of 16
 * bytes per buoy that belongs to the context: allocated at the first mark, overwritten by the next one, freed by
 * sitrk_set_buoys and sitrk_destroy, which both cancel the mark.  jrec0 = the model record that will be stepped next.
 * sitrk_deform_since_mark is valid right after the step of jrec1 >= jrec0: t0 = the snapshot, t1 = the current positions,
 * T = (jrec1 - jrec0 + 1) * rdt (one rounded product).  A buoy is a valid vertex iff it is alive now and, in sets with record
 * windows, rec_first <= jrec0 && rec_last >= jrec1: it was stepped at every record of the span.  The snapshot is in the
 * caller's order, so a re-sort between the two calls changes nothing.  Only cells go up and out / valid come back.
 * SITRK_EINVAL without a mark, for jrec1 < jrec0 and for no buoys; otherwise as sitrk_deform_cells. */
int sitrk_deform_mark(sitrk_t *h, int jrec0);
int sitrk_deform_since_mark(sitrk_t *h, int jrec1, int64_t nC, int nv, const int32_t *cells, double *out, int8_t *valid,
                            int64_t *nvalid);
/* measurement: GPU time [ms] of the kernels of the last sitrk_deform_cells / sitrk_deform_since_mark on this handle, from HIP
 * events around them -- the pass over the points, the cell kernel; either pointer may be NULL */
int sitrk_deform_kernel_ms(sitrk_t *h, float *points_ms, float *cells_ms);

/* ---- quadrangles from a triangulated buoy cloud --------------------------------
 * An EXTRA the reference does not have: adjacent triangles of a triangulation (sitrk_delaunay below, scipy's Delaunay on the
 * host, or any (nT,3) list) are paired into strictly convex, near-rectangular quadrangles, the cells sitrk_deform_* takes with nv = 4.  The pairing
 * is a deterministic greedy matching of maximum quality.  No parity claim is made against any other code; the contract below
 * is this library's own.  Everything in fp64, one rounded operation per symbol in the order written, no fused
 * multiply-add, no square root and no trigonometry.
 * Points are (nP,2) [y,x] km; a point is a VALID vertex iff it is not masked and both coordinates are finite.  tris is (nT,3)
 * int32 in either orientation.  A triangle is DEAD if a vertex is not valid, if two of its indices are equal, or if its signed
 * shoelace sum A2 (the expression of sitrk_deform_cells, nv = 3) is 0 or not finite.  A vertex index outside [0, nP) is an
 * error, not a dead triangle: SITRK_EINDEX with the number of offending triangles in sitrk_last_error (outputs unspecified);
 * such an index is never dereferenced and the handle stays usable.
 * A CANDIDATE is an undirected edge (p,q), p < q, that belongs to exactly two live triangles; an edge of three or more live
 * triangles is no candidate.  With r and s the two apexes (r == s, the same triangle listed twice: no candidate) its quadrangle
 * is the cycle r,p,s,q in CANONICAL form: started at its smallest index with the smaller of that vertex's two neighbours
 * second, A2 evaluated (sitrk_deform_cells' expression, nv = 4, relative to vertex 0), and where A2 < 0 the second and fourth
 * vertex exchanged and A2 evaluated again.  No candidate unless this A2 is > 0 and finite: the form is counter-clockwise with
 * x to the right and y up.  Both triangles of a pair get the same form, so everything below has the same bits for both.
 * With v_0..v_3 the canonical vertices, e_k = v_{k+1} - v_k (indices mod 4), L_k = e_k.x*e_k.x + e_k.y*e_k.y and at corner k
 *     cr_k = e_{k-1}.x*e_k.y - e_{k-1}.y*e_k.x ;  d_k = (-e_{k-1}.x)*e_k.x + (-e_{k-1}.y)*e_k.y ;  n_k = L_{k-1}*L_k
 *     s_k = d_k*|d_k| ;  q_k = (d_k*d_k)/n_k
 * a candidate is ACCEPTABLE iff
 *   1. cr_k > 0 at all four corners (strictly convex and simple),
 *   2. s_k <= (cos_lo*|cos_lo|)*n_k and s_k >= (cos_hi*|cos_hi|)*n_k at all four corners (the signed square of the cosine is
 *      monotone, so no root is needed; cos_lo >= cos_hi are the cosines of the smallest and the largest interior angle allowed),
 *   3. min_k L_k >= (ratio_min*ratio_min) * max_k L_k,
 *   4. area_min <= 0.5*A2 <= area_max  [km^2],
 *   5. its score is finite.
 * The SCORE is q = max_k q_k (q_0, then replaced by every q_k that compares greater): 0 for a rectangle, lower is better.
 * MATCHING: the acceptable candidates are taken in ascending order of (q, p, q-index); a candidate is taken iff neither of its
 * triangles has been taken.  The device reaches the same result in rounds: every untaken triangle picks the best remaining
 * candidate among its edges whose other triangle is untaken, and a candidate picked from both sides is taken; the first round
 * that takes nothing ends the matching (the globally best remaining candidate is always mutual).
 * OUTPUT: quads (nQ,4) int32 in canonical form, ordered by the smaller triangle id of each pair; tri_quad (nT) int32 = the row
 * of the quadrangle a triangle went into, -1 if it stayed single, -2 if it is dead; *nQ; *rounds = rounds run, the last, empty
 * one included (0 for nT == 0).  quads has room for cap rows; cap < nT/2 -> SITRK_EINVAL before any device work, as are
 * cosines outside [-1,1] or cos_lo < cos_hi, ratio_min outside [0,1], area_min > area_max (NaN included) and missing
 * pointers.  More than nT/2 + 1 rounds cannot happen and would be SITRK_EINVAL.
 *
 * sitrk_tri2quad: host arrays yx (nP,2), mask (nP) int8 with 0 = no valid vertex (NULL: none masked).  Synchronous on the
 * handle's stream; nT == 0 is valid.  Uses the context's transient scratch only: the grid, buoys and records of a tracker on
 * the same handle are left as they were. */
int sitrk_tri2quad(sitrk_t *h, int64_t nP, const double *yx, const int8_t *mask, int64_t nT, const int32_t *tris, double cos_lo,
                   double cos_hi, double ratio_min, double area_min, double area_max, int64_t cap, int32_t *quads,
                   int32_t *tri_quad, int64_t *nQ, int *rounds);
/* The same on the device-resident buoys of sitrk_set_buoys at their current positions, indices in the caller's buoy order; a
 * buoy is a valid vertex iff it is alive now.  Only tris go up and the result comes back; a re-sort changes nothing.
 * SITRK_EINVAL without buoys. */
int sitrk_tri2quad_buoys(sitrk_t *h, int64_t nT, const int32_t *tris, double cos_lo, double cos_hi, double ratio_min,
                         double area_min, double area_max, int64_t cap, int32_t *quads, int32_t *tri_quad, int64_t *nQ,
                         int *rounds);
/* measurement: GPU time [ms] of the phases of the last sitrk_tri2quad / sitrk_tri2quad_buoys that ran to its end on this
 * handle, from HIP events -- the triangle pass with the adjacency table, the scores, the rounds (their host read-backs
 * included), the compaction; any pointer may be NULL */
int sitrk_tri2quad_kernel_ms(sitrk_t *h, float *adjacency_ms, float *score_ms, float *rounds_ms, float *compact_ms);

/* ---- bounded Delaunay triangulation of a buoy cloud ------------------------------
 * An EXTRA the reference does not have: the triangles sitrk_tri2quad pairs, made on the device.  Every Delaunay triangle of the
 * cloud whose circumradius is at most rmax_km -- the full triangulation without the hull triangles that span open water and
 * land.  Such a triangle is decided by the points within 2*rmax_km of its vertices, so there is no global structure.  No parity
 * claim is made against any other code; the contract below is this library's own, pure integer mathematics.
 * Points are (nP,2) [y,x] km.  A point is a VERTEX iff it is not masked, both coordinates are finite, and no lower-indexed
 * vertex has the same integer coordinates Y = rint(y*2^20), X = rint(x*2^20) (int64; the scaling is exact, the rounding to
 * nearest-even).  |coordinate| > 2^30 km on an unmasked finite point is SITRK_EINVAL, the first such index named in
 * sitrk_last_error.  All predicates act on integer differences and are evaluated EXACTLY:
 *     orient(a,b,c)     = (Xb-Xa)*(Yc-Ya) - (Yb-Ya)*(Xc-Xa)        > 0: counter-clockwise with x to the right and y up
 *     incircle(a,b,c,d) = the 3x3 determinant of the rows (dx, dy, dx*dx+dy*dy) of a, b, c relative to d
 *                                                                   > 0: d strictly inside the circle of the ccw triangle abc
 * A row (p,q,r) of vertices is a triangle of the result iff
 *   1. p < q, p < r and orient(p,q,r) > 0;
 *   2. SIZE: with ux,uy = q-p, vx,vy = r-p, wx,wy = r-q (int64), la, lb, lc the three dx*dx+dy*dy, each exact in int64 and then
 *      converted to fp64 once, A2 = (double)orient(p,q,r), ru = rmax_km*1048576.0 and R4 = 4.0*(ru*ru):
 *      (la*lb)*lc <= (R4*A2)*A2, one rounded fp64 operation per symbol, no fused multiply-add (circumradius <= rmax_km without
 *      a root or a division);
 *   3. REACH: la <= R4, lb <= R4 and lc <= R4 (implied by 2 up to rounding; stated so that the candidates are exactly bounded);
 *   4. EMPTY CIRCLE: no vertex s has incircle(p,q,r,s) > 0;
 *   5. TIES: every vertex s outside {p,q,r} with incircle(p,q,r,s) == 0 has p < s and orient(q,r,s) > 0: a cocircular empty
 *      polygon is triangulated as the fan from its lowest index, and q->r is an edge of that polygon.
 * OUTPUT: tris (nT,3) int32, rows as above in ascending order of (p,q) -- a pair (p,q) has at most one r; *nT; vertex (nP)
 * int8, may be NULL: 1 for a vertex, 0 for a masked or non-finite point, 2 for a duplicate of a lower index.
 * nT <= max(0, 2*nV - 5) with nV the number of vertices.  tris has room for cap rows: cap < *nT writes only *nT (and vertex)
 * and returns SITRK_OK, the convention of sitrk_coast_segments.  rmax_km must be finite and in (0, 500], which keeps every
 * difference the predicates see below 2^30; NaN and values outside are SITRK_EINVAL before any device work, as are a missing
 * nT, a missing tris with cap > 0 and a missing yx.  The result never depends on the knob "delaunay_bin" (1..4, default 3:
 * square cells of side reach/delaunay_bin, 2*delaunay_bin+1 cells a side searched).
 *
 * sitrk_delaunay: host arrays yx (nP,2), mask (nP) int8 with 0 = masked (NULL: none).  Synchronous on the handle's stream;
 * nP == 0 is valid.  Uses the context's transient scratch only: the grid, buoys and records of a tracker on the same handle are
 * left as they were. */
int sitrk_delaunay(sitrk_t *h, int64_t nP, const double *yx, const int8_t *mask, double rmax_km, int64_t cap, int32_t *tris,
                   int64_t *nT, int8_t *vertex);
/* The same on the device-resident buoys of sitrk_set_buoys at their current fp64 positions, indices in the caller's buoy order;
 * a buoy can be a vertex iff it is alive now.  Nothing but the result comes down; a re-sort changes nothing.  SITRK_EINVAL
 * without buoys. */
int sitrk_delaunay_buoys(sitrk_t *h, double rmax_km, int64_t cap, int32_t *tris, int64_t *nT, int8_t *vertex);
/* measurement: GPU time [ms] of the phases of the last sitrk_delaunay / sitrk_delaunay_buoys that ran its kernels on this
 * handle, from HIP events -- binning (quantisation with the host's read of the bounding box, keys, sort, duplicates), the
 * triangle kernel, the compaction (sort of the rows by (p,q)); any pointer may be NULL */
int sitrk_delaunay_kernel_ms(sitrk_t *h, float *bin_ms, float *tri_ms, float *compact_ms);
/* ... and the in-circle tests of that call: all of them, and those whose sign the fp64 filter left to the 128-bit form */
int sitrk_delaunay_stats(sitrk_t *h, int64_t *incircle_tests, int64_t *exact_tests);

/* ---- device-resident quadrangle meshes ------------------------------------------
 * An EXTRA the reference does not have: the chain sitrk_delaunay_buoys -> sitrk_tri2quad_buoys -> sitrk_deform_mark /
 * sitrk_deform_since_mark without a triangle, a quadrangle or a position moving to the host.  A context holds
 * up to SITRK_MESH_MAX meshes, addressed by mesh in 0 .. SITRK_MESH_MAX-1.  A mesh is nQ quadrangles of buoy indices in the
 * caller's order, (nQ,4) int32, the t0 positions of their vertices (64 B per quadrangle, in cell order), the model record jrec0
 * those positions belong to and the pairing parameters it was built with, all in device allocations of the context's own:
 * neither the transient scratch nor the record slots.  sitrk_set_buoys and sitrk_destroy free every mesh (the indices belong
 * to the buoy set), sitrk_mesh_free frees one; a re-sort, sitrk_restore_state and every stepping entry point leave them alone.
 *
 * sitrk_mesh_build acts on the device-resident buoys at their current fp64 positions.  mask: host array (nP) int8 in the
 * caller's order, NULL = all; a buoy is a point of the mesh iff it is alive now and its mask byte is not 0.  The quadrangles
 * are, as integers and in the same order, what sitrk_tri2quad returns for the rows of sitrk_delaunay on (current positions,
 * alive and mask, rmax_km) with the same five parameters; *nT and *rounds are the values those two calls give (any of nT, nQ,
 * rounds may be NULL).  The t0 positions are the current ones; jrec0 = the model record that will be stepped next.  It replaces
 * whatever the slot held; nQ == 0 is a valid, empty mesh.  Argument checks are those of sitrk_delaunay_buoys and
 * sitrk_tri2quad_buoys, made before any device work, plus mesh out of range; SITRK_EINVAL without buoys.  Only the mask goes up;
 * only the counters come back that the two host functions read too: the bounding box, the triangle count, one word per round.
 * A call that fails leaves the slot as it was.
 * sitrk_mesh_cells returns the (nQ,4) rows; cells has room for cap rows, cap < nQ writes only *nQ and returns SITRK_OK.
 * sitrk_mesh_mark takes the t0 positions again for the same cells at the current positions, with a new jrec0; a vertex that is
 * not alive now gets NaN, and its cells are invalid from then on.
 * sitrk_mesh_deform is valid right after the step of jrec1 >= jrec0: t1 = the current positions, T = (jrec1 - jrec0 + 1) * rdt,
 * a buoy is a valid vertex under the rule of sitrk_deform_since_mark.  out (5,nQ) fp64 = div, shr, vor, area0, area1: the
 * contract of sitrk_deform_cells with nv = 4, the same bits as sitrk_deform_since_mark gives for the same cells after a
 * sitrk_deform_mark at the same moment.  status (nQ) int8: 0 = invalid in that contract's sense, all five values SITRK_FILL;
 * 1 = valid and acceptable at t1; 2 = valid, not acceptable at t1.  ACCEPTABLE AT t1 = the tests of sitrk_tri2quad on the four
 * vertices in their stored order at their t1 positions with the mesh's own parameters: the t1 shoelace sum relative to vertex 0
 * is > 0 and finite, tests 1-4 hold and the score is finite.  The stored order is canonical at t0 and is not made canonical
 * again: a cell that has turned inside out fails the first test.
 * stats is SITRK_MESH_NSTATS fp64: n0, n1, n2 = the number of cells of each status, then over the status-1 cells only
 * sum(area0), sum(area1), sum(area0*div), sum(area0*shr) and sum(area0*tot^q) for q = 1, 2, 3, with tot = sqrt(div*div +
 * shr*shr) and the terms formed as a*tot, (a*tot)*tot, ((a*tot)*tot)*tot: one rounded fp64 operation per symbol, no fused
 * multiply-add.  The order of the sums is the implementation's but fixed (no floating-point atomics): two calls on the same
 * state return the same bits.  Any of out, status, stats may be NULL, not all three; with only stats, 80 bytes come back and
 * nothing else.  SITRK_EINVAL for an empty slot (never built, or freed), jrec1 < jrec0 and no buoys; an empty mesh (nQ == 0)
 * returns zeros in stats. */
#define SITRK_MESH_MAX 8
#define SITRK_MESH_NSTATS 10
int sitrk_mesh_build(sitrk_t *h, int mesh, int jrec0, double rmax_km, const int8_t *mask, double cos_lo, double cos_hi,
                     double ratio_min, double area_min, double area_max, int64_t *nT, int64_t *nQ, int *rounds);
int sitrk_mesh_cells(sitrk_t *h, int mesh, int64_t cap, int32_t *cells, int64_t *nQ);
int sitrk_mesh_mark(sitrk_t *h, int mesh, int jrec0);
int sitrk_mesh_deform(sitrk_t *h, int mesh, int jrec1, double *out, int8_t *status, double *stats);
int sitrk_mesh_free(sitrk_t *h, int mesh);
/* measurement: GPU time [ms] from HIP events of the last sitrk_mesh_build (its whole device chain, the host's reads of the
 * counters included) and of the last sitrk_mesh_deform -- the pass over the buoys, the cell kernel, the final sum; any pointer
 * may be NULL, SITRK_EINVAL for a phase that has not run */
int sitrk_mesh_kernel_ms(sitrk_t *h, float *build_ms, float *points_ms, float *cells_ms, float *stats_ms);

/* ---- buoy cells rasterised onto a regular grid -----------------------------------
 * An EXTRA the reference does not have: which cell each point of a regular grid lies in, and for a device-resident mesh the
 * deformation of that cell -- the map of a mesh without its per-cell results moving to the host.  No parity
 * claim is made against any other code; the contract below is this library's own.  Everything in fp64, one rounded operation
 * per symbol in the order written, no fused multiply-add; only + - * and comparisons, so nothing is unpinned.
 * THE GRID is (y0_km, x0_km, d_km, ny, nx) in the polar-stereographic plane the tracker works in: square pixels of side d_km,
 * pixel (j,i) with j along y and i along x, its centre at
 *     cy_j = y0 + ((double)j + 0.5) * d ; cx_i = x0 + ((double)i + 0.5) * d        (one rounded product and one rounded sum each)
 * SITRK_EINVAL before any device work unless y0, x0, d are finite, d > 0, ny, nx >= 1 and ny*nx <= 2^28.
 * A CELL is nv = 3 or 4 vertices (y_k, x_k), k' = (k+1) mod nv, in either orientation.  A2 = the shoelace sum relative to
 * vertex 0, the expression of sitrk_deform_cells.  The cell is DRAWABLE iff all 2 nv coordinates are finite, A2 is finite and
 * A2 != 0; s = +1 if A2 > 0, else -1.
 * THE INSIDE TEST: for each edge
 *     o_k = (x_k' - x_k)*(cy - y_k) - (y_k' - y_k)*(cx - x_k)
 * and a centre lies IN the cell iff s*o_k >= 0 for every k: the boundary counts as inside.  For a quadrangle that is not convex
 * this is the part of it seen from all four edges; the cells of a mesh are strictly convex by the acceptance tests of
 * sitrk_tri2quad, at t0 always and at t1 where their status is 1.
 * THE OWNER: owner (ny,nx) int32 = the LOWEST index among the drawn cells the pixel's centre lies in, -1 for none.  A centre on a
 * shared edge or vertex, or in several overlapping cells (at t1, after convergence), goes to the lowest index whatever order
 * the cells are processed in: two calls on the same state return the same bits.  *nowned (may be NULL) = the number of pixels
 * with owner >= 0.  A cell's bounding box only bounds the pixels that are tested (its index range widened by one pixel each way,
 * the centre arithmetic not being exactly invertible, and checked against the centres themselves); the result is that of testing
 * every pixel against every cell.
 *
 * sitrk_raster_cells: host arrays yx (nP,2) [y,x] km, cells (nC,nv) int32, draw (nC) int8 (NULL: all): a cell is drawn iff its
 * byte is not 0 and it is drawable.  A vertex index outside [0, nP) is SITRK_EINDEX with the number of offending cells in
 * sitrk_last_error (owner unspecified); such an index is never dereferenced and the handle stays usable.  nC == 0 is valid:
 * every pixel -1.  Synchronous on the handle's stream.  Uses the context's transient scratch only (never read by the stepping):
 * the grid, buoys, records and meshes of a tracker on the same handle are left as they were.  SITRK_EINVAL for nv not in {3,4}
 * and missing pointers.
 * sitrk_mesh_raster is valid wherever sitrk_mesh_deform(mesh, jrec1, ...) is, and runs the same pass over the buoys and the same
 * cell kernel; the statuses and rates stay on the device.  at_t1 == 0: the geometry is the mesh's stored t0 positions and the
 * cells of status 1 or 2 are drawn (the most deformed cells are the ones a map is made for).  at_t1 == 1: the geometry is the
 * current positions and only the cells of status 1 are drawn (a cell of status 2 may have turned inside out).  fields (may be
 * NULL) is (5,ny,nx) fp64: the bits of div, shr, vor, area0, area1 of the pixel's owner as sitrk_mesh_deform returns them,
 * SITRK_FILL where owner == -1.  owner may be NULL when fields is not; both NULL is SITRK_EINVAL, as is at_t1 outside {0,1}.
 * The other errors are those of sitrk_mesh_deform, plus the grid's.  An empty mesh gives -1 and SITRK_FILL everywhere.  Only the
 * raster comes down: 4 (+ 40) bytes per pixel.
 * sitrk_raster_kernel_ms: GPU time [ms] of the last of the two calls on this handle, from HIP events -- the fill of the raster
 * with the cell kernel, the gather kernel; either pointer may be NULL, SITRK_EINVAL before any such call.
 * sitrk_raster_stats, measurement only: with the knob "raster_count" set to 1 (default 0; it never changes a result) the cell
 * kernel also counts *claims = the (centre, drawn cell) pairs that passed the inside test, each of which is one integer atomic;
 * claims over *nowned is 1 where no two drawn cells share a centre.  Of the last call that ran with the knob set, SITRK_EINVAL
 * if there is none. */
int sitrk_raster_cells(sitrk_t *h, int64_t nP, const double *yx, int64_t nC, int nv, const int32_t *cells, const int8_t *draw,
                       double y0_km, double x0_km, double d_km, int ny, int nx, int32_t *owner, int64_t *nowned);
int sitrk_mesh_raster(sitrk_t *h, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny, int nx,
                      int32_t *owner, double *fields, int64_t *nowned);
int sitrk_raster_kernel_ms(sitrk_t *h, float *cells_ms, float *gather_ms);
int sitrk_raster_stats(sitrk_t *h, int64_t *claims);

/* ---- coarse-grained deformation of buoy cells: the spatial scaling curve -------------
 * An EXTRA the reference does not have: the cells' velocity gradients box-averaged on a pyramid over a regular grid, and per
 * level the area-weighted moments of the total deformation of the boxes -- one point of the curve <tot^q>(L) per level, L =
 * d*2^l, from one mesh and one call (the spatial scaling analysis of Marsan et al. 2004).  No parity claim is
 * made against any other code; the contract below is this library's own.  Everything in fp64, one rounded operation per symbol
 * in the order written, no fused multiply-add.  The level sums use only + - * /, so every bit of `boxes` is pinned; the one
 * unpinned operation is the device's sqrt, in the moments table.
 * THE GRID is (y0_km, x0_km, d_km, ny, nx) as for sitrk_raster_cells, and 1 <= nlev <= SITRK_COARSE_MAXLEV.  Level l has
 *     ny_l = (ny + 2^l - 1) >> l  by  nx_l = (nx + 2^l - 1) >> l  boxes of side L_l = d*2^l (an exact scaling);
 * box (J,I) of level l+1 has the children (2J,2I), (2J,2I+1), (2J+1,2I), (2J+1,2I+1) of level l; the levels above the one that
 * reaches 1 x 1 stay 1 x 1.  SITRK_EINVAL before any device work unless y0, x0, d are finite, d > 0, ny, nx >= 1, ny*nx <= 2^24
 * (the pyramid holds 48 bytes per box), nlev is in range and fmin is finite and >= 0.
 * A CELL'S TERMS: with a = area0 and u_x, u_y, v_x, v_y of the sitrk_deform_cells contract, the five terms a, a*u_x, a*u_y,
 * a*v_x, a*v_y.
 * WHERE A CELL GOES: by its t0 centroid,
 *     nv = 4:  cy = 0.25*((y_0 + y_1) + (y_2 + y_3))        nv = 3:  cy = ((y_0 + y_1) + y_2)/3.0         cx likewise
 *     fy = (cy - y0)/d ; fx = (cx - x0)/d
 * The cell is IN THE GRID iff fy >= 0 && fy < ny && fx >= 0 && fx < nx, compared in fp64, and its pixel is (floor(fy),
 * floor(fx)): a centroid exactly on a pixel line belongs to the upper pixel.  A cell goes whole to that pixel.
 * LEVEL 0: each pixel has six values n, A, AUx, AUy, AVx, AVy.  n = the number of contributing cells of the pixel, as fp64.
 * Each of the five sums starts at +0.0 and the terms of the pixel's contributing cells are added IN ASCENDING CELL INDEX,
 * S = S + t.
 * LEVEL l+1: each of the six values is (c00 + c01) + (c10 + c11) of the children, a child beyond the edge counting as +0.0.
 * No floating-point atomics anywhere: two calls return the same bits, and a permutation of the cell rows returns the bits of
 * this contract evaluated on the permuted rows.
 * THE TABLE is (nlev, SITRK_COARSE_NCOLS) fp64, per level: [0] the number of boxes with n >= 1; [1] the number of FILLED boxes,
 * those with n >= 1, A > 0 and A >= fmin*(L_l*L_l); then sums over the filled boxes only: [2] A, [3] A*div, [4] A*shr,
 * [5] A*tot, [6] (A*tot)*tot, [7] ((A*tot)*tot)*tot, where per filled box
 *     UX = AUx/A ; UY = AUy/A ; VX = AVx/A ; VY = AVy/A
 *     div = UX + VY ; e1 = UX - VY ; e2 = UY + VX ; shr = sqrt(e1*e1 + e2*e2) ; tot = sqrt(div*div + shr*shr)
 * The order of these eight sums is the implementation's, fixed by the level's size alone (columns 0 and 1 are exact).
 * OUTPUTS: boxes (may be NULL) is the whole pyramid, level-major, each level (6, ny_l, nx_l) fp64; table as above; *nin and
 * *nout (may be NULL) = the contributing cells inside and outside the grid.
 *
 * sitrk_coarse_cells: host arrays with the argument rules of sitrk_deform_cells -- yx0, yx1 (nP,2), mask0 / mask1 (nP) or NULL,
 * cells (nC,nv), T finite and > 0 -- and use (nC) int8 (NULL: all).  A cell CONTRIBUTES iff its use byte is not 0 and it is valid
 * in the sense of sitrk_deform_cells.  A vertex index outside [0, nP) is SITRK_EINDEX with the number of offending cells in
 * sitrk_last_error (outputs unspecified); such an index is never dereferenced and the handle stays usable.  nC == 0 is valid:
 * zeros.  Synchronous on the handle's stream.  Uses the context's transient scratch only: the grid, buoys, records and meshes of
 * a tracker on the same handle are left as they were.
 * sitrk_mesh_coarse is valid wherever sitrk_mesh_deform(mesh, jrec1, ...) is, and runs the same pass over the buoys and the same
 * cell kernel; the statuses stay on the device.  The cells of status 1 contribute; their t0 geometry is the mesh's stored t0
 * positions, T that of sitrk_mesh_deform.  The result is that of sitrk_coarse_cells on those positions, the mesh's cells and
 * use = (status == 1).  An empty mesh gives zeros.  The errors are those of sitrk_mesh_deform plus the grid's.  Only the table
 * (64 bytes per level) and, when asked for, the pyramid come down.
 * sitrk_coarse_kernel_ms: GPU time [ms] of the phases of the last of the two calls on this handle, from HIP events -- the cells'
 * terms and keys, the sort, level 0, the levels above it, the table; any pointer may be NULL, SITRK_EINVAL before any such
 * call. */
#define SITRK_COARSE_MAXLEV 16
#define SITRK_COARSE_NCOLS 8
int sitrk_coarse_cells(sitrk_t *h, int64_t nP, const double *yx0, const double *yx1, const int8_t *mask0, const int8_t *mask1,
                       int64_t nC, int nv, const int32_t *cells, const int8_t *use, double T, double y0_km, double x0_km,
                       double d_km, int ny, int nx, int nlev, double fmin, double *boxes, double *table, int64_t *nin, int64_t *nout);
int sitrk_mesh_coarse(sitrk_t *h, int mesh, int jrec1, double y0_km, double x0_km, double d_km, int ny, int nx, int nlev,
                      double fmin, double *boxes, double *table, int64_t *nin, int64_t *nout);
int sitrk_coarse_kernel_ms(sitrk_t *h, float *terms_ms, float *sort_ms, float *level0_ms, float *pyramid_ms, float *table_ms);

/* ---- features of a map: connected components of a mask on a regular grid ---------------
 * An EXTRA the reference does not have: the connected bands of pixels of a raster that pass a test -- the leads, ridges and
 * linear kinematic features of a deformation map -- labelled on the device, and one row of integers per feature brought down
 * instead of the map.  No parity claim is made against any other code; the contract below is this library's
 * own.  Everything is integer, so nothing is unpinned.
 * THE RASTER is (ny, nx) with 1 <= ny, nx <= 32768 and ny*nx <= 2^28 (the side keeps the sum of j*j below 2^63); the linear
 * index of pixel (j,i) is p = j*nx + i.  THE MASK active (ny,nx) int8: a pixel is active iff its byte is not 0.
 * CONNECTIVITY conn is 4 (the neighbours across a pixel's four sides) or 8 (those and the four across its corners); anything
 * else is SITRK_EINVAL.  A component is a maximal set of active pixels joined by chains of neighbours.
 * THE LABELS: labels (ny,nx) int32, may be NULL: -1 for a pixel that is not active, else THE LOWEST LINEAR INDEX OF THE PIXEL'S
 * COMPONENT.  That is canonical: it does not depend on the tiling, the launch geometry or which lane gets where first, and two
 * calls return the same bits.
 * THE TABLE: table (maxfeat, SITRK_FEAT_NCOLS) int64, one row per component with npix >= min_pix (min_pix >= 1), the rows in
 * ascending label; only the first maxfeat of them are written (maxfeat >= 0; table may be NULL iff maxfeat == 0) and the rest of
 * `table` is left as it was.  Columns: [0] the label; [1] npix; [2] jmin, [3] jmax, [4] imin, [5] imax; the sums over the
 * component's pixels [6] j, [7] i, [8] j*j, [9] i*i, [10] j*i; [11] the perimeter = the number of sides of the component's
 * pixels whose other pixel is not active, the raster's rim counting as not active (an active pixel across a side belongs to the
 * same component for conn 4 and 8 alike).
 * THE COUNTS, each may be NULL: *nfeat = the components with npix >= min_pix, which may exceed maxfeat -- that is how the caller
 * learns that the table is truncated; *ncomp = all components; *nactive = the active pixels.
 *
 * sitrk_label_raster: a host mask.  Synchronous on the handle's stream.  Uses the context's transient scratch only: the grid,
 * buoys, records and meshes of a tracker on the same handle are left as they were.  A mask of zeros is valid: every label -1,
 * the counts 0.  SITRK_EINVAL before any device work for a raster, conn, min_pix or maxfeat out of range and missing pointers.
 * sitrk_mesh_features is valid wherever sitrk_mesh_raster(mesh, jrec1, at_t1, grid, ...) is, and runs the same pass over the
 * buoys, the same cell kernel and the same rasteriser; owner and rates stay on the device, where the mask is made, and only what
 * was asked for comes down: with labels == NULL the rows of the table and the three counts.  Its result is DEFINED BY THE
 * EXISTING CONTRACTS: that of sitrk_label_raster on the mask  owner >= 0 && test(out[:, owner]),  owner being what
 * sitrk_mesh_raster returns and out what sitrk_mesh_deform returns for the same arguments.  THE TEST: `what` selects f -- 0: div,
 * 1: shr, 2: vor -- and the pixel is active iff  sgn*f >= thr  with sgn +1 or -1, compared in fp64, a NaN never active.
 * what == 3, the total deformation: active iff  div*div + shr*shr >= thr*thr  (one rounded operation per symbol, no fused
 * multiply-add), which needs sgn == +1 and thr >= 0: no second square root, so the test adds nothing unpinned.  thr is finite,
 * in the unit of out.  (shr itself ends in the device's sqrt: DESIGN.md 3.14.)  The errors are those of sitrk_mesh_raster plus
 * the ones above, all raised before any device work.
 * Should a union-find loop of the kernels ever reach its bound -- the number of pixels, which a chain of strictly falling
 * indices cannot -- the call returns SITRK_EHIP with a text in sitrk_last_error instead of spinning; the outputs are unspecified.
 * sitrk_features_kernel_ms: GPU time [ms] of the phases of the last of the two calls on this handle, from HIP events -- the mask
 * (its kernel, or for sitrk_label_raster its upload), the labels (tiles, merge levels, flattening), the table (counts, scan,
 * rows); any pointer may be NULL, SITRK_EINVAL before any such call. */
#define SITRK_FEAT_NCOLS 12
#define SITRK_LABEL_TILE 64        /* side of the tiles the labelling starts from; never changes a result */
int sitrk_label_raster(sitrk_t *h, int ny, int nx, const int8_t *active, int conn, int64_t min_pix, int64_t maxfeat,
                       int32_t *labels, int64_t *table, int64_t *nfeat, int64_t *ncomp, int64_t *nactive);
int sitrk_mesh_features(sitrk_t *h, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny, int nx,
                        int what, int sgn, double thr, int conn, int64_t min_pix, int64_t maxfeat,
                        int32_t *labels, int64_t *table, int64_t *nfeat, int64_t *ncomp, int64_t *nactive);
int sitrk_features_kernel_ms(sitrk_t *h, float *mask_ms, float *label_ms, float *table_ms);

/* ---- features from window to window: kept label maps, carried by the ice, matched by overlap ---------------
 * An EXTRA the reference does not have: which feature of one window is which feature of the next.  A tracker
 * builds a new mesh per window, so cell identities do not survive a window; the buoys do.  A label map made on the t0 draw of
 * window k is carried by the cells of that window's mesh to the window's end, which is the instant the t0 draw of window k+1 is
 * made at: two maps at the same physical time on the same grid compare by plain pixel overlap.  No parity claim is made against
 * any other code; the contract below is this library's own.  Everything is integer and no result depends on an order, so
 * nothing is unpinned and two calls return the same bits.
 * KEPT MAPS.  A context holds up to SITRK_KEEP_MAX kept maps, addressed by keep in 0..SITRK_KEEP_MAX-1.  Each is a shape
 * (ny, nx) within the limits of sitrk_label_raster, an int32 map of that shape whose every value is -1 or in [0, ny*nx), and the
 * conn and min_pix it was made with.  A kept map is a device allocation of the context's own, 4 bytes per pixel: neither the
 * transient scratch nor a mesh.  Kept maps are freed by sitrk_keep_free and sitrk_destroy; stepping, re-sorts, sitrk_set_buoys,
 * mesh calls and every call that uses the transient scratch leave them alone; a call that fails leaves every slot as it was.
 * SITRK_EINVAL for a slot out of range and for reading an empty slot.
 * sitrk_mesh_features_keep: every argument behind `keep` is one of sitrk_mesh_features, with the same validity, the same errors
 * and the same bits in labels, table, *nfeat, *ncomp, *nactive.  It also fills slot keep with  K[p] = labels[p]  where the
 * pixel's component has npix >= min_pix, else -1; a truncation of the table by maxfeat does not affect K.
 * sitrk_keep_put: uploads the host map (ny,nx) into a slot, with conn in {4, 8} and min_pix >= 1 as its record of origin.  The
 * map need not be a canonical labelling.  A value outside [-1, ny*nx) is SITRK_EINDEX with the number of offending values in
 * sitrk_last_error; it is checked before the slot is replaced.
 * sitrk_keep_get: any pointer may be NULL; with map == NULL nothing comes down but the four numbers.
 * CARRYING A MAP WITH THE ICE.  sitrk_mesh_features_advect is valid wherever sitrk_mesh_raster(mesh, jrec1, ., grid) is; slot
 * keep_from must hold a map of shape (ny, nx); keep_to may equal keep_from.  Its result is DEFINED BY THE EXISTING CONTRACTS: let
 * o0 and o1 be the owner that sitrk_mesh_raster returns for the same arguments with at_t1 = 0 and at_t1 = 1, L the map of
 * keep_from and nQ the cells of the mesh; then
 *     cellfeat[q] = min { L[p] : o0[p] == q and L[p] >= 0 },  -1 when the set is empty          (q = 0 .. nQ-1)
 *     M[p]        = o1[p] >= 0 ? cellfeat[o1[p]] : -1
 * and slot keep_to becomes M, with keep_from's conn and min_pix.  *ncells = the cells with cellfeat >= 0, *ncarried = the pixels
 * with M >= 0; either may be NULL.  The call does not ask whether L was made from this mesh.  A cell of status 2 is drawn at t0
 * and not at t1 (the rasteriser's rule: it may have turned inside out), so what it carried is dropped.  Nothing but the two
 * counts comes down.  The errors are those of sitrk_mesh_raster plus the slots'.
 * MATCHING TWO KEPT MAPS.  sitrk_features_match needs both slots filled and of equal shape (keepA == keepB is allowed),
 * 0 <= reach <= SITRK_MATCH_MAXREACH, |dj|, |di| <= 32768, maxpair >= 0 and pairs NULL iff maxpair == 0; else SITRK_EINVAL before
 * any device work.  For a pixel p = (j,i) with a = A[j,i] >= 0, S(p) is the set of distinct values b >= 0 among
 * B[j+dj+s, i+di+t] for |s|, |t| <= reach, positions outside the raster contributing nothing, and
 *     count(a,b) = #{ p : A[p] == a and b in S(p) }.
 * pairs (maxpair, 3) int64 holds the rows (a, b, count) with count >= 1 in ascending (a, b); only the first maxpair rows are
 * written and the rest of `pairs` is left as it was.  *npair counts all such rows and may exceed maxpair; *nhit = the pixels of A
 * with a non-empty S; either may be NULL.  With reach == 0 the table is the pixel overlap, symmetric under swapping the slots and
 * negating the shift; with reach > 0 it is the A-side count, and the caller swaps the slots for the other side.  E = the sum of
 * |S(p)| over the pixels is counted first: E > 2^31 - 1 is SITRK_EINVAL with a text, before anything is sized from it.
 * sitrk_match_kernel_ms / sitrk_advect_kernel_ms: GPU time [ms] of the last such call on this handle, from HIP events -- the keys
 * (counts, scan, emission), their sort, the rows (bounds, scan, rows); the kernels of the advection behind its two rasters; any
 * pointer may be NULL, SITRK_EINVAL before any such call. */
#define SITRK_KEEP_MAX 16
#define SITRK_MATCH_MAXREACH 2
int sitrk_mesh_features_keep(sitrk_t *h, int keep, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny,
                             int nx, int what, int sgn, double thr, int conn, int64_t min_pix, int64_t maxfeat,
                             int32_t *labels, int64_t *table, int64_t *nfeat, int64_t *ncomp, int64_t *nactive);
int sitrk_keep_put(sitrk_t *h, int keep, int ny, int nx, const int32_t *map, int conn, int64_t min_pix);
int sitrk_keep_get(sitrk_t *h, int keep, int *ny, int *nx, int *conn, int64_t *min_pix, int32_t *map);
int sitrk_keep_free(sitrk_t *h, int keep);
int sitrk_mesh_features_advect(sitrk_t *h, int keep_from, int keep_to, int mesh, int jrec1, double y0_km, double x0_km, double d_km,
                               int ny, int nx, int64_t *ncells, int64_t *ncarried);
int sitrk_features_match(sitrk_t *h, int keepA, int keepB, int dj, int di, int reach, int64_t maxpair, int64_t *pairs, int64_t *npair,
                         int64_t *nhit);
int sitrk_match_kernel_ms(sitrk_t *h, float *emit_ms, float *sort_ms, float *rows_ms);
int sitrk_advect_kernel_ms(sitrk_t *h, float *advect_ms);

/* ---- skeletons of a label map: thinning, a table per feature, end points and junctions ---------------
 * An EXTRA the reference does not have: the features of a label map thinned to lines one pixel wide on the device, so that a
 * feature's length along itself, its number of arms and the places where arms meet come down instead of the map (DESIGN.md
 * 3.19).  No parity claim is made against any other code; the contract below is this library's own.  Everything is integer and
 * nothing is defined by an order of evaluation, so nothing is unpinned and two calls return the same bits.
 * INPUT.  A label map L (ny,nx) int32 within the limits of sitrk_label_raster, every value -1 or in [0, ny*nx): whatever
 * sitrk_keep_put accepts; it need not be a canonical labelling.  The mask is L >= 0; p = j*nx + i.
 * THINNING: Guo and Hall's two-sub-iteration algorithm (A1, 1989) on the mask, pixels outside the raster counting as 0.  For pixel
 * (j,i) of the current state S name its neighbours  p2 = S[j-1,i], p3 = S[j-1,i+1], p4 = S[j,i+1], p5 = S[j+1,i+1], p6 = S[j+1,i],
 * p7 = S[j+1,i-1], p8 = S[j,i-1], p9 = S[j-1,i-1]  and define
 *     C = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2))
 *     N = min((p9|p2)+(p3|p4)+(p5|p6)+(p7|p8), (p2|p3)+(p4|p5)+(p6|p7)+(p8|p9))
 *     m = (p6|p7|!p9) & p8  for sub-iteration k = 0, 2, 4, ...;   m = (p2|p3|!p5) & p4  for k = 1, 3, 5, ...
 * Sub-iteration k removes, all at once and from the state before it, every set pixel with  C == 1 && 2 <= N <= 3 && m == 0.
 * The device applies sub-iterations 0 .. max_sub-1 with 1 <= max_sub <= 2^20; those behind the fixpoint change nothing, so it
 * may stop early.  *nsub = 1 + the index of the last sub-iteration that removed a pixel, 0 if none did; *converged = 1 iff
 * max_sub >= nsub + 2: one quiet sub-iteration of each kind has then been seen.  THE SKELETON K is the state after those
 * sub-iterations.  The labels play no part in the thinning: features that touch are thinned as one.
 * CLASSIFICATION.  With the ring r0..r7 = p2, p3, p4, p5, p6, p7, p8, p9 taken from K, X(p) = the number of k with r[k] == 0 and
 * r[(k+1)%8] == 1.  A skeleton pixel is an END iff X == 1 and a JUNCTION iff X >= 3.
 * LINKS.  A link joins two skeleton pixels of one label.  An orthogonal link is (j,i)-(j,i+1) or (j,i)-(j+1,i).  A diagonal link
 * is (j,i)-(j+1,i+1) with neither (j,i+1) nor (j+1,i) in K, or (j,i)-(j+1,i-1) with neither (j,i-1) nor (j+1,i) in K; the blocking
 * pixels count whatever their label.  Each link is attributed once, to its first pixel.  A straight row of n pixels has n-1 links.
 * THE TABLE: table (maxfeat, SITRK_SKEL_NCOLS) int64, one row per distinct value >= 0 of L in ascending value; only the first
 * maxfeat rows are written (maxfeat >= 0; table may be NULL iff maxfeat == 0), the rest is left as it was.  Columns: [0] the value;
 * [1] the pixels of L with it; [2] nskel, its skeleton pixels; [3] nend; [4] njunc; [5] north; [6] ndiag.  *nfeat counts all rows.
 * THE NODES: nodes (maxnode, 3) int64, the rows (p, L[p], X(p)) of every skeleton pixel with X != 2 -- isolated pixels, X == 0,
 * included -- in ascending p; only the first maxnode rows are written (nodes may be NULL iff maxnode == 0).  *nnode counts all.
 * skel (ny,nx) int8, 1 on K and 0 elsewhere, may be NULL: nothing of raster size comes down then.  *nskel = the pixels of K.  Any
 * count pointer may be NULL.
 * sitrk_skeleton_raster: a host map.  Synchronous on the handle's stream; uses the context's transient scratch only.  A value
 * outside [-1, ny*nx) is SITRK_EINDEX with the number of offending values in sitrk_last_error, as in sitrk_keep_put.
 * sitrk_keep_skeleton: the kept map of slot keep, which it leaves as it was; SITRK_EINVAL for a slot out of range or empty.  With a
 * slot filled by sitrk_mesh_features_keep the rows of the table carry the labels and npix of that call's feature table in the
 * same order, given an equal maxfeat.
 * SITRK_EINVAL before any device work for a raster, max_sub, maxfeat or maxnode out of range and for missing pointers.  The
 * result never depends on the knob "skeleton_batch".
 * sitrk_skeleton_kernel_ms: GPU time [ms] of the phases of the last of the two calls on this handle, from HIP events -- the
 * thinning (its launches and the waits for their counters), the table (classification, counts, scan, rows), the nodes; any
 * pointer may be NULL, SITRK_EINVAL before any such call. */
#define SITRK_SKEL_NCOLS 7
int sitrk_skeleton_raster(sitrk_t *h, int ny, int nx, const int32_t *map, int max_sub, int64_t maxfeat, int64_t maxnode,
                          int8_t *skel, int64_t *table, int64_t *nodes, int64_t *nfeat, int64_t *nnode, int64_t *nskel,
                          int *nsub, int *converged);
int sitrk_keep_skeleton(sitrk_t *h, int keep, int max_sub, int64_t maxfeat, int64_t maxnode,
                        int8_t *skel, int64_t *table, int64_t *nodes, int64_t *nfeat, int64_t *nnode, int64_t *nskel,
                        int *nsub, int *converged);
int sitrk_skeleton_kernel_ms(sitrk_t *h, float *thin_ms, float *table_ms, float *nodes_ms);

/* ---- dispersion of buoy pairs: strain moments by separation class ----------------------
 * An EXTRA the reference does not have: for every pair of points that lie r0 apart at t0, how much their separation has changed
 * at t1, and per class of r0 the moments of that strain -- the buoy-dispersion analysis of sea-ice deformation (Rampal et al.
 * 2008).  It needs no triangulation, no quadrangle test and no grid.  No parity claim is made against any other
 * code; the contract below is this library's own.  Everything in fp64, one rounded operation per symbol in the order written, no
 * fused multiply-add.
 * POINTS: yx0, yx1 are (nP,2) [y,x] in km, in the tracker's polar-stereographic plane, at t0 and t1.  A point is VALID iff its
 * mask0 and mask1 bytes are not 0 (NULL: all) and its four coordinates are finite.
 * PAIRS: a pair is an unordered i < j of valid points; each pair counts once.
 *     dy = y_j - y_i ; dx = x_j - x_i ; q0 = dy*dy + dx*dx      on the t0 positions;  q1 the same on the t1 positions
 * CLASSES: edges_km holds nc + 1 finite, strictly increasing values with edges[0] >= 0, 1 <= nc <= SITRK_PAIRS_MAXCLASS.
 *     E_c = edges[c]*edges[c]   (one rounded product)
 * A pair is in class c iff E_c <= q0 && q0 < E_{c+1}, compared in fp64, and it CONTRIBUTES iff it is in a class and q0 > 0.
 * Only + - * and comparisons decide this: the class of every pair, and so every count, is pinned bit for bit.
 * A PAIR'S TERMS:
 *     r0 = sqrt(q0) ; r1 = sqrt(q1) ; d = (q1 - q0)/(r0 + r1) ; e = d/r0
 * d is r1 - r0 formed without cancelling two square roots: q1 - q0 is pinned, the only unpinned operations are the device's two
 * sqrt.  e is the pair's strain over the interval.  The elapsed time does not enter: rates are e/T on the host.
 * THE TABLE is (nc, SITRK_PAIRS_NCOLS) fp64, one row per class: [0] n, the number of contributing pairs (exact, below 2^53);
 * [1] sum r0; [2] sum e; [3] sum |e|; [4] sum e*e; [5] sum (e*e)*|e|; [6] sum d*d.  The order of the sums is the
 * implementation's but fixed by the points and the edges alone: no floating-point atomics, two calls on the same state return
 * the same bits.  *npts (may be NULL) = the number of valid points.
 *
 * sitrk_pairs_points: host arrays; mask0 / mask1 (nP) int8 or NULL.  Synchronous on the handle's stream.  Uses the context's
 * transient scratch only: the grid, buoys, records, meshes and marks of a tracker on the same handle are left as they were.
 * nP of 0 or 1 is valid: zeros.  SITRK_EINVAL, before any device work, for nc out of range, edges that are not finite, not
 * strictly increasing or start below 0, and missing pointers.
 * COST: the work is the number of pairs within edges[nc] of each other, about nP * rho * pi * edges[nc]^2 / 2 for a cloud of rho
 * points per km^2, and nothing caps it: it is the caller's to bound, through the mask or a coarsened cloud.
 * sitrk_pairs_mark is queued on the compute stream behind the stepping already queued and snapshots the current fp64 positions
 * of all buoys, in the caller's order, with a validity byte each -- alive now and, with a mask (nP, caller's order, may be
 * NULL), its byte not 0 -- into a device buffer of 17 bytes per buoy that belongs to the context: allocated at the first mark,
 * overwritten by the next one, freed by sitrk_pairs_free, sitrk_set_buoys and sitrk_destroy, which all cancel the mark.  It is
 * independent of sitrk_deform_mark and of the meshes.  jrec0 = the model record that will be stepped next.
 * sitrk_pairs_since_mark is valid right after the step of jrec1 >= jrec0: t0 = the snapshot, t1 = the current positions.  A buoy
 * is valid iff it was valid at the mark and is a valid vertex under the rule of sitrk_deform_since_mark: alive now and, in sets
 * with record windows, rec_first <= jrec0 && rec_last >= jrec1.  The table has the bits of sitrk_pairs_points on (the snapshot,
 * the current positions, those two validities); the snapshot is in the caller's order, so a re-sort between the calls changes
 * nothing.  It may be called any number of times after one mark, each later jrec1 one more interval from the same t0.  Only
 * edges_km goes up and 56 bytes per class come down.  SITRK_EINVAL without a mark, for jrec1 < jrec0, without buoys, and as
 * sitrk_pairs_points for nc, the edges and the pointers.
 * sitrk_pairs_free: frees the snapshot and cancels the mark; valid at any time.
 * sitrk_pairs_kernel_ms: GPU time [ms] of the phases of the last table on this handle, from HIP events -- the binning (box, keys,
 * sort, gather, bin starts), the pairs kernel, the table; any pointer may be NULL, SITRK_EINVAL before any such call.
 * sitrk_pairs_stats: *tests = the pairs that last table's pairs kernel formed q0 for, all class passes together. */
#define SITRK_PAIRS_MAXCLASS 16
#define SITRK_PAIRS_NCOLS 7
int sitrk_pairs_points(sitrk_t *h, int64_t nP, const double *yx0, const double *yx1, const int8_t *mask0, const int8_t *mask1,
                       int nc, const double *edges_km, double *table, int64_t *npts);
int sitrk_pairs_mark(sitrk_t *h, int jrec0, const int8_t *mask);
int sitrk_pairs_since_mark(sitrk_t *h, int jrec1, int nc, const double *edges_km, double *table, int64_t *npts);
int sitrk_pairs_free(sitrk_t *h);
int sitrk_pairs_kernel_ms(sitrk_t *h, float *bin_ms, float *pairs_ms, float *table_ms);
int sitrk_pairs_stats(sitrk_t *h, int64_t *tests);

/* ---- distribution of values: counts between edges, exact order statistics ----------------------
 * An EXTRA the reference does not have: the probability distribution of the deformation rates -- how many cells fall between
 * explicit edges, the PDF with its power-law tail -- and their order statistics -- the percentile a feature threshold is stated
 * as -- taken on the device, for a host array or for the cells of a device-resident mesh whose per-cell rates never move to the
 * host.  No parity claim is made against any other code; the contract below is this library's own.  It has only
 * comparisons in fp64, counts, and a selection on the bits of the values, so nothing is unpinned.
 * THE SAMPLE.  sitrk_dist_values: x (n) fp64, use (n) int8 or NULL; the sample is x[i] for every i with use == NULL or
 * use[i] != 0.  sitrk_mesh_dist: the cells of status 1 of sitrk_mesh_deform(mesh, jrec1) -- the population its ten stats are
 * summed over --, and their value is f = div, shr or vor for what = 0, 1, 2, taken as f, -f or |f| for sgn = +1, -1, 0.  what = 3
 * is the total deformation squared,  t2 = div*div + shr*shr  (one rounded operation per symbol, no fused multiply-add): the
 * square, as in sitrk_mesh_features, so that no second square root enters; it needs sgn == +1.  A NaN is not part of the sample
 * and is counted in *nnan; *m is the sample's size (either may be NULL).  -0.0 is taken as +0.0 (v + 0.0).  Infinities are
 * ordinary values.
 * THE HISTOGRAM.  nb in 0 .. SITRK_DIST_MAXBINS; edges (nb+1) finite and strictly ascending.  counts (nb+2) int64: counts[c] =
 * the number of sample values v with exactly c of the edges <= v, compared in fp64.  So counts[0] lies below edges[0], counts[c]
 * for 1 <= c <= nb in [edges[c-1], edges[c]) and counts[nb+1] at or above edges[nb]; the counts add up to m.  nb == 0 skips the
 * histogram; edges and counts may then be NULL.
 * ORDER STATISTICS.  nq in 0 .. SITRK_DIST_MAXQ, every q[t] in [0,1].  The rank of target t is
 *     k_t = min(m - 1, (int64)floor(q[t] * (double)m))            (one rounded product)
 * formed ON THE DEVICE from the counted m, so that no round trip is needed to learn m first.  qval[t] = the value at position k_t
 * of the sample in ascending order, BIT FOR BIT ONE OF THE SAMPLE'S VALUES (after -0.0 -> +0.0); qrank[t] = k_t.  With m == 0
 * qval[t] is NaN and qrank[t] is -1.  The order is that of the usual monotone 64-bit key of an fp64: with b its bits,
 *     key = b ^ (b >> 63 ? ~0 : 1 << 63)
 * which for the values of a sample is the order of <.  nq == 0 skips the selection; q, qval and qrank may then be NULL.
 * BYTES.  Only the nb+2 counts, the nq pairs and the two integers come down; sitrk_dist_values sends x and use up, sitrk_mesh_dist
 * sends the edges and q: nothing per cell crosses to the host in either direction.
 * sitrk_dist_values is synchronous on the handle's stream and uses the context's transient scratch only: the grid, buoys,
 * records, meshes, marks and kept maps of a tracker on the same handle are left as they were.  n == 0 is valid: zeros, m = 0.
 * sitrk_mesh_dist is valid wherever sitrk_mesh_deform is, runs the same pass over the buoys and the same cell kernel, and leaves
 * the mesh, buoys, records and kept maps as they were.  An empty mesh (nQ == 0) returns zeros, m = 0.
 * Two calls return the same bits, and the result does not depend on the launch geometry or on the knob "dist_aggregate" (0/1,
 * default 0; 1: in the selection a wave whose matching keys share their digit adds their number once).  Measured no faster.
 * SITRK_EINVAL, before any device work: nb or nq out of range, edges that are not finite or not strictly ascending, a q outside
 * [0,1] (a NaN included), missing pointers, n < 0, what or sgn out of range, what == 3 with sgn != +1, and for sitrk_mesh_dist
 * what sitrk_mesh_deform refuses: an empty slot, jrec1 < jrec0, no buoys.
 * sitrk_dist_kernel_ms: GPU time [ms] of the phases of the last of the two calls on this handle, from HIP events -- the keys (key
 * kernel, the sum of m and the ranks; for the mesh form the deformation itself is under sitrk_mesh_kernel_ms), the histogram
 * (counts, sum of the rows), the selection (eight digit passes, each a count and a pick); any pointer may be NULL, SITRK_EINVAL
 * before any such call.
 * sitrk_dist_stats, measurement only: *passes = the digit passes that call's selection ran (8, or 0 with nq == 0), *top_pass_ms =
 * the GPU time of the first of them, the top digit, where the keys of one sign and exponent crowd one counter; either may be
 * NULL. */
#define SITRK_DIST_MAXBINS 1024
#define SITRK_DIST_MAXQ    16
int sitrk_dist_values(sitrk_t *h, int64_t n, const double *x, const int8_t *use,
                      int nb, const double *edges, int64_t *counts,
                      int nq, const double *q, double *qval, int64_t *qrank,
                      int64_t *m, int64_t *nnan);
int sitrk_mesh_dist(sitrk_t *h, int mesh, int jrec1, int what, int sgn,
                    int nb, const double *edges, int64_t *counts,
                    int nq, const double *q, double *qval, int64_t *qrank,
                    int64_t *m, int64_t *nnan);
int sitrk_dist_kernel_ms(sitrk_t *h, float *keys_ms, float *hist_ms, float *select_ms);
int sitrk_dist_stats(sitrk_t *h, int *passes, float *top_pass_ms);

/* ---- distance to the model coastline ------------------------------------------
 * An EXTRA the reference does not have: its coastal cleaning of a seed cloud (`ldo_coastal_clean`, mojito's MaskCoastal,
 * util.Dist2Coast) reads a rasterised dist2coast file.  Here the coast is the model's own: the edges between a sea T-cell
 * and a land T-cell, and the distance is exact geometry in the plane the tracker works in.  No parity claim is made against
 * any other code; the contract below is this library's own.
 * Coast segments.  T-cell (j,i) has the corners F(j-1,i-1), F(j-1,i), F(j,i), F(j,i-1) (tracking.vertices_of).  Edge k of it:
 *     k = 0   shared by T(j,i) and T(j,i+1), defined for j >= 1 and i+1 < Ni:   a = F(j-1,i), b = F(j,i)
 *     k = 1   shared by T(j,i) and T(j+1,i), defined for i >= 1 and j+1 < Nj:   a = F(j,i-1), b = F(j,i)
 * An edge is a coast segment iff exactly one of its two cells has tmask == 0; the domain rim is no coast.  Its id is
 * 2*(j*Ni+i) + k (int32: Nj*Ni <= 2^29).  A coast edge with a non-finite endpoint coordinate is dropped and counted.
 * Distance of a point p to segment (a,b), [y,x] order, plane km, fp64, one rounded operation per symbol, no fused
 * multiply-add:
 *     ey = yb - ya ; ex = xb - xa ; py = yp - ya ; px = xp - xa
 *     len2 = ey*ey + ex*ex ; dot = py*ey + px*ex
 *     t = (len2 > 0) ? dot / len2 : 0 ; t = t < 0 ? 0 : (t > 1 ? 1 : t)
 *     cy = py - t*ey ; cx = px - t*ex ; d2 = cy*cy + cx*cx
 * d2min[p] = the minimum of d2 over ALL coast segments, seg[p] = the lowest id that attains it, dist[p] = sqrt(d2min[p]).
 * The index behind the queries only prunes with conservative bounds: what is reported is this minimum, which does not
 * depend on any order, so d2min and seg are reproducible bit for bit (sqrt is the device's).
 * rmax_km: finite and > 0 bounds the search: with r2 = rmax_km*rmax_km (rounded), a point with d2min > r2 reports
 * dist = +inf, seg = -1, every other point the unbounded answer.  rmax_km <= 0 or +inf: unbounded.  NaN: SITRK_EINVAL.
 * No coast (every cell sea, or every cell land): every point reports +inf, -1, and the calls return SITRK_OK.
 * A query with a non-finite coordinate reports NaN, -1 (when there is a coast) and is no error.
 * Units: kilometres in the polar-stereographic plane of sitrk_geo2cart, true at 70 N.  Against distances on the sphere the
 * plane's scale is (1 + sin 70) / (1 + sin lat): about +4 % at 60 N, -3 % at the pole.  It is not corrected for.
 *
 * sitrk_coast_build: extracts the segments on the device and builds the search index over them, from the host arrays Yf, Xf
 * (Nj,Ni) fp64 km and tmask (Nj,Ni) int8 -- or, with all three NULL, from the device copy of the grid of sitrk_set_grid
 * (Nj, Ni then 0 or that grid's; SITRK_EINVAL without a grid).  Segments and results are bit-identical either way.  The
 * index lives in device buffers of its own (68 bytes per segment + 4 per bin; not the transient scratch), is replaced by the
 * next build, freed by sitrk_destroy, and, when it was built from the context's grid, dropped by a later sitrk_set_grid.
 * *nseg / *ndropped (either may be NULL): coast segments kept / dropped for a non-finite endpoint.  The bin side is read from
 * the knob "coast_bin" (1..64, default 4: quarters of sqrt(bounding-box area / nseg)) at build time; results never depend
 * on it.  Needs Nj, Ni >= 2 and Nj*Ni <= 2^29. */
int sitrk_coast_build(sitrk_t *h, int Nj, int Ni, const double *Yf, const double *Xf, const int8_t *tmask, int64_t *nseg,
                      int64_t *ndropped);
/* Probe for tests and plots: *n = number of segments; when cap >= *n, ids (n) and ab (n,2,2) = [a|b][y,x] in id order (either
 * may be NULL); with cap < *n only *n is written. */
int sitrk_coast_segments(sitrk_t *h, int64_t cap, int32_t *ids, double *ab, int64_t *n);
/* dist (n) fp64 km and seg (n) int32 (may be NULL) of the host points yx (n,2) [y,x] km.  Synchronous on the handle's stream;
 * n == 0 is valid.  The points and results pass through the transient scratch only: the grid, buoys and records of a tracker
 * on the same handle are left as they were.  SITRK_EINVAL without an index. */
int sitrk_coast_dist(sitrk_t *h, int64_t n, const double *yx, double rmax_km, double *dist, int32_t *seg);
/* The same for every buoy of sitrk_set_buoys, alive or not, at its current fp64 position on the device, in the caller's
 * order: nothing but the result leaves the device; buoys, records and stepping state are only read.  SITRK_EINVAL without
 * buoys or without an index. */
int sitrk_coast_dist_buoys(sitrk_t *h, double rmax_km, double *dist, int32_t *seg);
/* measurement: GPU time [ms] of the query kernel of the last sitrk_coast_dist / sitrk_coast_dist_buoys on this handle, from
 * HIP events around it */
int sitrk_coast_kernel_ms(sitrk_t *h, float *query_ms);

/* ---- locate / seeding ----------------------------------------------------
 * FindContainingCell (sitrack/locate.py:280-330) for n points: from the guess
 * T-point tries centre, i+1, j+1, i-1, j-1.  found[k] 1/0; jiT_out = centre of
 * the found cell (last candidate tried when not found).  Needs set_grid. */
int sitrk_find_cells(sitrk_t *h, int64_t n, const double *yx, const int32_t *jiT_guess,
                     int32_t *jiT_out, int8_t *found);

/* SeedInit (sitrack/tracking.py:98-178), per-seed part: nearest T-point by
 * Haversine (locate.py:222-276, util.py:85-103) with the acceptance test of
 * NearestPoint as called there (rd_found_km = rFoundKM = 2.5, max_itr = 10, 2-D
 * resolkm), Survive on that T-point, FindContainingCell.  Outputs are NOT
 * compacted: keep[k] in {0,1}, why[k] (optional) 0 kept / 1 no nearest point /
 * 2 Survive / 3 no containing cell; the caller compacts with where(keep==1)
 * exactly like tracking.py:166-178.  sic: (Nj,Ni) fp64 ice concentration at
 * the seeding record (si3_part_tracker.py:228-229). */
int sitrk_seed_init(sitrk_t *h, int64_t nP, const double *latlon, const double *yx,
                    const double *latT, const double *lonT, const double *resolkm,
                    const double *sic, int32_t *jiT_out, int8_t *keep, int8_t *why);

/* NearestPoint alone (sitrack/locate.py:222-276, whole-domain form with find_ji_of_min :13-20 and Haversine
 * util.py:85-103): for each of nP points latlon (nP,2) [lat,lon] the (j,i) of the nearest T-point of the current grid's
 * latT/lonT (Nj,Ni), or (-1,-1) when the acceptance loop gives up (distance >= 0.5*resolkm[j,i] * 1.2^(max_itr-2), or
 * rd_found_km * 1.2^(max_itr-2) when resolkm is NULL).  SeedInit calls it with rd_found_km = 2.5, max_itr = 10.
 * dmin (nP) may be NULL: Haversine distance to that T-point in km (+inf for points rejected without a search). */
int sitrk_nearest_point(sitrk_t *h, int64_t nP, const double *latlon, const double *latT, const double *lonT,
                        const double *resolkm, double rd_found_km, int max_itr, int32_t *ji, double *dmin);

/* Idealised seeding on the model grid: nemoSeed (sitrack/tracking.py:365-442) + Geo2CartNPSkm1D (util.py:394-410), i.e. what
 * tools/generate_idealized_seeding.py computes (:201-386), on the device.  Every khss-th T-point of the (Nj,Ni) mesh
 * whose tmask x rmask (rmask may be NULL) is 1, whose latitude is not below 55 and whose ice concentration is not below
 * 0.9 carries a seed; with latF/lonF (both or neither) also every interior sub-sampled F-point whose four sub-sampled
 * T-neighbours carry one.  Outputs in the reference's order -- T-seeds in C order of the sub-sampled mesh, then F-seeds
 * -- as latlon (n,2) [lat,lon] and, if yx != NULL, yx (n,2) [y,x] km in the polar-stereographic plane (lat0, lon0).
 * Call once with capacity = 0 to learn the counts (*nT, *nF), then with arrays of nT + nF rows. */
int sitrk_nemo_seed(sitrk_t *h, int Nj, int Ni, int khss, const int8_t *tmask, const int8_t *rmask,
                    const double *latT, const double *lonT, const double *sic, const double *latF, const double *lonF,
                    double lat0, double lon0, int64_t capacity, double *latlon, double *yx, int64_t *nT, int64_t *nF);

/* ---- seed-cloud coarsening -------------------------------------------------
 * SubSampCloud (sitrack/util.py:345-370), i.e. gudhi.subsampling.sparsify_point_set(yx, min_squared_dist=rd_km**2) on the
 * seeds' polar-stereographic [y,x] km: n points yx (n,2) in the given order, keep[k] 1/0, *nkeep = number kept.
 * Contract: d2(i,j) = (y_i-y_j)*(y_i-y_j) + (x_i-x_j)*(x_i-x_j), two rounded fp64 products and one rounded sum, no FMA,
 * compared with r2 = rd_km*rd_km (rounded fp64).  Point i is kept iff no kept j < i has d2(i,j) < r2: pairs at exactly
 * d2 == r2 are both kept, duplicates collapse to the first.  This is the lexicographically-first maximal independent set
 * of the graph with edges d2 < r2 -- the greedy loop of gudhi's sparsify_point_set, whose documented guarantee is
 * "squared distance between any two output points >= min_squared_dist".  The boundary rule and the rounding are taken
 * from that documented behaviour and loop; gudhi itself is not available to this project, so bit parity with gudhi is
 * UNPINNED.  Result independent of the knob "subsample_block" (points per workgroup, 256..4096, powers of two).
 * Host arrays, synchronous on the handle's stream like sitrk_nemo_seed; n == 0 is valid.  *launches (may be NULL) =
 * launches of the resolve kernel.  Uses the context's transient scratch only (never read by the stepping): the grid,
 * buoys and records of a tracker on the same handle are left as they were.  SITRK_EINVAL when rd_km is not finite or
 * <= 0, when a coordinate is not finite (the first such index is named in sitrk_last_error) or a pointer is missing. */
int sitrk_subsample_cloud(sitrk_t *h, int64_t n, const double *yx, double rd_km, int8_t *keep, int64_t *nkeep, int32_t *launches);

/* ---- overlap cleaning of a tracked cloud ---------------------------------------
 * CancelTooClose (sitrack/util.py:520-565) at one record krec: n buoys at lat/lon (degrees, the record's positions), valid[b]
 * = pmsk[krec,b] != 0 (NULL: every buoy valid), nrec_all[b] = sum_t pmsk[t,b], nrec_before[b] = sum_{t<krec} pmsk[t,b].
 * Contract: d(j,k) = the reference Haversine(lat[j], lon[j], lat[k], lon[k]) (util.py:85-103, R = 6360 km, its operation
 * order); nn[j] = the valid k != j of smallest d(j,k), lowest index on ties, dmin[j] = that distance.  The reference's scan
 * (util.py:536-556) then runs over j in index order: if j is still alive and dmin[j] < rd_km, the one of j and nn[j] with
 * the smaller count goes (on equal counts nn[j]), where the count of a buoy already dropped is nrec_before (its records >= krec
 * were zeroed) and that of a live one nrec_all.  Distances are measured to dropped buoys too.  Every pass of the reference
 * starts afresh, so NbPass >= 1 does not change the result and this runs it once.  keep[b] = 1 for the buoys kept (valid and
 * not dropped), *nkeep their number, *nclose (may be NULL) the number of valid buoys with dmin < rd_km.
 * Extension (the reference raises IndexError there): a buoy with valid[b] == 0 takes no part -- never examined, nobody's
 * neighbour, not kept; with every buoy valid the result is the reference's.  The device sin/cos/asin may differ from numpy's
 * in the last ulp (the convention of sitrk_eval_haversine), so a dmin within ~1e-12 relative of rd_km, or two distinct
 * distances within ~1e-12 of each other, are unpinned; exact duplicates (distance 0) are exact.
 * Host arrays, synchronous on the handle's stream; n == 0 is valid.  Uses the context's transient scratch only (never read by
 * the stepping): the grid, buoys and records of a tracker on the same handle are left as they were.  SITRK_EINVAL when rd_km is
 * not finite or outside (0, 9999] (above 9999 the reference's self-mask would win), when a coordinate of a valid buoy is not
 * finite (the first such index is named in sitrk_last_error) or a pointer is missing. */
int sitrk_cancel_too_close(sitrk_t *h, int64_t n, const double *lat, const double *lon, const int8_t *valid, const int32_t *nrec_all,
                           const int32_t *nrec_before, double rd_km, int8_t *keep, int64_t *nkeep, int64_t *nclose);

/* Probe of the first stage of sitrk_cancel_too_close: for every valid buoy j, nn[j] and dmin[j] as defined there when
 * dmin[j] < rd_km, else nn[j] = -1 and dmin[j] = +inf (also for the buoys with valid[j] == 0).  Same arguments, limits and
 * errors as sitrk_cancel_too_close. */
int sitrk_nearest_buoy(sitrk_t *h, int64_t n, const double *lat, const double *lon, const int8_t *valid, double rd_km, int32_t *nn,
                       double *dmin);

/* ---- predicate probes ------------------------------------------------------
 * The device-side predicates of the hot path evaluated on plain arrays, so that each one can be held
 * against the reference function it restates (parity tests):
 *   sitrk_eval_inside    IsInsideQuadrangle (sitrack/locate.py:49-78): pts (n,2) [y,x], quads (n,4,2).  Evaluated in the
 *                        division-free form of the hot loop AND in the plain form: 0/1, +2 if the two ever disagreed
 *   sitrk_eval_euler     r + (vel * rdt) / 1000. (si3_part_tracker.py:452-458) as the hot loop evaluates it
 *   sitrk_eval_intersect intersect2Seg and _ccw_(A,B,C) (sitrack/tracking.py:44-58): segs (n,4,2) = A,B,C,D; ccw_abc may be NULL
 *   sitrk_eval_crossing  CrossedEdge + NewHostCell + UpdtInd4NewCell (tracking.py:182-305) on the current grid for a
 *                        move P1 -> P2 out of host cell jiT (n,2): new vJIt and, if codes != NULL, (n,2) = the return
 *                        values of CrossedEdge (1..4) and NewHostCell (1..8)
 *   sitrk_survive_mask   Survive (tracking.py:62-93) for every cell of the current grid with the given (Nj,Ni) fp64
 *                        ice concentration and the current rmin_conc: 1 = kill */
int sitrk_eval_inside(sitrk_t *h, int64_t n, const double *pts, const double *quads, int8_t *inside);
int sitrk_eval_euler(sitrk_t *h, int64_t n, const double *r, const double *vel, double rdt, double *out);
/* Haversine (sitrack/util.py:85-103, R = 6360 km) element by element: dist[k] between (plat[k],plon[k]) and (xlat[k],xlon[k]) */
int sitrk_eval_haversine(sitrk_t *h, int64_t n, const double *plat, const double *plon, const double *xlat,
                         const double *xlon, double *dist);
int sitrk_eval_intersect(sitrk_t *h, int64_t n, const double *segs, int8_t *intersect, int8_t *ccw_abc);
int sitrk_eval_crossing(sitrk_t *h, int64_t n, const double *P1, const double *P2, const int32_t *jiT, int32_t *jiT_new,
                        int32_t *codes);
int sitrk_survive_mask(sitrk_t *h, const double *sic, int8_t *mask);

/* ---- projection -----------------------------------------------------------
 * CartNPSkm2Geo1D / Geo2CartNPSkm1D (sitrack/util.py:394-429): WGS84 polar
 * stereographic, lat_ts = lat0, lon_0 = lon0 (defaults 70, -45 in the
 * reference), km <-> degrees, arrays (n,2) [y,x] <-> [lat,lon]. */
int sitrk_cart2geo(sitrk_t *h, int64_t n, const double *yx, double lat0, double lon0, double *latlon);
int sitrk_geo2cart(sitrk_t *h, int64_t n, const double *latlon, double lat0, double lon0, double *yx);

/* ---- measurement ----------------------------------------------------------
 * HIP events on the library's compute stream (torch.cuda.Event would only see
 * torch's stream).  timer_stop waits for the stop event and returns the elapsed ms. */
int sitrk_timer_start(sitrk_t *h);
int sitrk_timer_stop(sitrk_t *h, float *ms);
/* iAlive.sum() -- the per-record "current number of buoys alive" line of the
 * reference driver (si3_part_tracker.py:376) */
int sitrk_count_alive(sitrk_t *h, int64_t *nalive);

#ifdef __cplusplus
}
#endif
#endif /* SITRK_H */
