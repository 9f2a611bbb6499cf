// sitrk_internal.h -- context layout and host-side helpers shared by the translation units of libsitrk.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/sitrk.h"
#include "sitrk_geom.h"
#include "sitrk_launch.h"

namespace sitrk {

// The timing events of one timed range of a module's last call -- event k and k + 1 lie around phase k -- and whether that call
// recorded them all.  The sitrk_*_kernel_ms entry points refuse to read a timer that is not complete.
template <int N>
struct PhaseTimer {
    hipEvent_t ev[N] = {};
    bool complete = false;
    int create(sitrk_ctx *h);                           // creates the events at the first use
    int begin(sitrk_ctx *h);                            // ... and clears the flag
    int mark(sitrk_ctx *h, int k);                      // records event k on the compute stream
    void done() { complete = true; }
    int elapsed(sitrk_ctx *h, int k, float *ms);        // phase k in ms; a null ms is skipped
    void release();                                     // destroys the events, clears the flag
};

hipError_t sort_pairs_u32(void *tmp, size_t *tmp_bytes, const uint32_t *kin, uint32_t *kout,
                          const int32_t *vin, int32_t *vout, size_t n, unsigned end_bit, hipStream_t s);
hipError_t sort_keys_u64(void *tmp, size_t *tmp_bytes, const uint64_t *kin, uint64_t *kout, size_t n, unsigned end_bit, hipStream_t s);

// Seed-cloud coarsening (sitrk_subsample.hip): cells of side 1/inv_h, ny x nx of them, from (ymin, xmin)
struct SubGrid {
    double ymin = 0.0, xmin = 0.0, inv_h = 0.0;
    int ny = 1, nx = 1;
};
constexpr int kSubMaxPpt = 16;          // points per thread of resolve_kernel: knob subsample_block = 256 * ppt, 256..4096
struct SubResolveArgs {
    SubGrid g;
    int64_t n = 0;
    double r2 = 0.0;
    int ppt = 4;
    const pt *yx = nullptr;             // sorted by cell, index order inside a cell
    const int32_t *perm = nullptr;      // perm[s] = input index of sorted point s
    const int32_t *cstart = nullptr, *cend = nullptr;
    uint8_t *state = nullptr;           // 0 undecided, 1 kept, 2 dropped (sorted order)
    int32_t *cur_q = nullptr;           // pull cursor: sorted position (-1: start of the cell) ...
    uint8_t *cur_k = nullptr;           // ... inside neighbour cell cur_k (0..8)
    uint8_t *done = nullptr;            // per workgroup: all its points decided
    unsigned long long *undecided = nullptr;   // optional: += points still undecided at each workgroup's exit
};
// cells of side `side` over the extents hi[c] - lo[c], c < dims: the side is doubled while the grid exceeds max_cells cells or 2^20
// cells a side (a coarser grid is only slower).  false: no grid fits; else *inv_h = 1 / side and ncell[c] cells along c
bool fit_cell_grid(int dims, const double *lo, const double *hi, double side, int64_t max_cells, double *inv_h, int64_t *ncell);

// Overlap cleaning of a tracked cloud (sitrk_overlap.hip): cubic cells of side 1/inv_h over the unit vectors' bounding box,
// nx x ny x nz of them from (x0, y0, z0); key = (cz * ny + cy) * nx + cx, ncells = nx * ny * nz (the key of an invalid buoy)
struct __attribute__((aligned(16))) V3 { double x, y, z, w; };
struct OvGrid {
    double x0 = 0.0, y0 = 0.0, z0 = 0.0, inv_h = 0.0;
    int nx = 1, ny = 1, nz = 1;
    uint32_t ncells = 1;
};

// Distance to the model coastline (sitrk_coast.hip): the coast segments in id order (what sitrk_coast_segments returns) and the
// same segments ordered by the square bin of their midpoint, with the offset of every bin's first segment.  Device buffers of their
// own: a tracker queries again and again, so none of this lives in the transient scratch.
struct CoastIndex {
    int64_t nseg = 0;
    const pt *seg = nullptr;            // (2 nseg) endpoints a, b in BIN order, id order inside a bin
    const int32_t *sid = nullptr;       // (nseg) segment ids in bin order
    const int32_t *start = nullptr;     // (ny*nx + 1) first segment of bin by*nx + bx; a run of bins of one row is one run of segments
    double y0 = 0.0, x0 = 0.0, h = 1.0, inv_h = 1.0;   // bins of side h from (y0, x0), ny x nx of them
    int ny = 1, nx = 1;
    double pad = 0.0;                   // >= half the longest segment, plus what the index's own rounding can amount to [km]
};
struct CoastState {
    bool built = false;
    bool from_grid = false;             // built from the context's grid: a later sitrk_set_grid invalidates it
    int64_t ndropped = 0;
    int32_t *ids = nullptr;             // (nseg) id order
    pt *ab = nullptr;                   // (2 nseg) id order
    pt *seg = nullptr;                  // the arrays of CoastIndex
    int32_t *sid = nullptr, *start = nullptr;
    CoastIndex ix;
    PhaseTimer<2> timer;                // around the query kernel of the last distance call
};

// Quadrangles from triangles (sitrk_quadmesh.hip): the acceptance parameters as the kernels take them
struct QuadParams {
    double c_lo2, c_hi2;        // cos_lo*|cos_lo|, cos_hi*|cos_hi|
    double ratio2;              // ratio_min*ratio_min
    double area_min, area_max;
};

// A device-resident quadrangle mesh (sitrk_mesh.hip): allocations of their own, neither the transient scratch nor the record slots
struct Mesh {
    bool built = false;                 // false: the slot is empty (never built, or freed)
    int64_t nQ = 0;
    int32_t *quads = nullptr;           // (nQ,4) buoy indices in the caller's order, canonical at t0
    pt *t0 = nullptr;                   // (nQ,4) t0 positions of the vertices in cell order, 64 B per quadrangle; NaN in y: no valid vertex
    int jrec0 = 0;                      // the model record those positions belong to (stepped next when they were taken)
    double rmax_km = 0.0;
    QuadParams par = {0.0, 0.0, 0.0, 0.0, 0.0};
};

// A kept label map (sitrk_track.hip): a device allocation of its own, neither the transient scratch nor a mesh
struct KeptMap {
    int32_t *map = nullptr;             // (ny*nx) -1 or a label in [0, ny*nx); null: the slot is empty
    size_t cap = 0;                     // pixels the allocation holds
    int ny = 0, nx = 0, conn = 0;
    int64_t min_pix = 0;
};

// Device-resident buoy state, structure of arrays, in SORTED slot order.
// perm[s] = index of slot s in the caller's order.
struct BuoyState {
    pt      *pos      = nullptr;   // (y,x) km, current position           16 B
    int32_t *cell     = nullptr;   // packed (jT,iT) | dead bit              4 B
    int32_t *kill_rec = nullptr;   // model record of the kill, -1 alive     4 B
    int2    *win      = nullptr;   // (z1stModelRec, zLstModelRec), only when windowed: one 8-byte word, so that the
                                   // re-sort gathers it with one request                          8 B
    int32_t *perm     = nullptr;   //                                        4 B
};

// THE per-record output rule (xmask[jt+1] of si3_part_tracker.py:459-460), shared by fetch_record_kernel and
// sample_fields_kernel: slot s, whose packed cell is c, stepped at jrec  <=>  jrec lies in its window and it was alive before
// that record: still alive, or killed by this very record
__device__ __forceinline__ bool stepped_at(BuoyState st, int64_t s, int32_t c, int jrec, bool windowed)
{
    bool in_window = true;
    if (windowed) { const int2 w = st.win[s]; in_window = (jrec >= w.x) && (jrec <= w.y); }
    return in_window && (c >= 0 || st.kill_rec[s] == jrec);
}

}  // namespace sitrk

struct sitrk_ctx {
    int device = 0;
    char err[512] = {0};

    hipStream_t own_stream = nullptr;   // created by the library
    hipStream_t stream = nullptr;       // compute stream in use (own or adopted)
    hipStream_t copy_stream = nullptr;  // host -> device record uploads (overlap with stepping)
    hipStream_t sv_stream = nullptr;    // Survive derivation of records that just arrived (round 4): ingest work -- the DMA on copy_stream,
                                        // then the record's Survive bytes here -- runs NEXT TO the stepping of the resident records;
                                        // the compute stream waits for a slot's event right before the first launch that reads the slot
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // record ingest: library-owned pinned staging, double-buffered (sitrk_stage_acquire / sitrk_stage_submit).
    // The caller's buffers are copied (or read by the caller) into pinned memory before a push returns, the DMA into
    // the slot runs on copy_stream, ordered against the compute stream by events only.
    static constexpr int kStage = 2;
    void *stage[kStage] = {nullptr, nullptr};
    size_t stage_bytes = 0;                     // capacity of each buffer (= one whole slab)
    hipEvent_t stage_done[kStage] = {nullptr, nullptr};   // recorded on copy_stream behind the last DMA out of the buffer
    int stage_next = 0;                         // buffer the next acquire hands out
    int stage_rows = -1;                        // rows of the buffer handed out by acquire and not submitted yet (-1: none)
    int stage_cols = 0;                         // ... and its columns (Ni for the row-band entry points)

    // grid
    int Nj = 0, Ni = 0;
    sitrk::CellGeo *geo = nullptr;      // (Nj*Ni) 48-byte records
    sitrk::pt *geoF = nullptr;          // (Nj*Ni) F-points alone: the fused kernel fills its LDS patches from contiguous rows of it
    int8_t *orient = nullptr;           // (Nj*Ni) orientation bits of the velocity pick (cell_orient_kernel)
    int8_t *tmask = nullptr;

    // parameters
    double rdt = 3600.0;
    int nsub = 1;                       // Euler sub-steps per record (sitrk_set_substeps); dt_sub = rdt / nsub at launch
    int uv_strategy = 1;
    double rmin_conc = 0.1;
    double eps_mg = 0.0;                // 2^-48 * max |Yf|,|Xf| (inside_quad_hot)
    // performance knobs and their measured defaults (tools/ab_tune.py on MI355X, C3):
    // non-temporal state streams -2 %, tile-major 8x16 cell order -8 %, XCD-chunked block order +5 % (off)
    int tune = sitrk::TUNE_NT_STATE;    // TUNE_* bits
    int step_block = 512;               // workgroup size of advect_step_kernel (512: -3.6 % vs 256, 1024: +1.8 %)
    int fuse = 32;                      // sitrk_run: consecutive resident records advanced per launch, <= nslots (1 = one launch per record)
    int tile_j = 8, tile_i = 16;        // sort order: 0 = row-major cells, else tile-major tiles of tile_j x tile_i cells
    int patch_kb = 16;                  // fused kernel: LDS bytes per workgroup for its geometry patch (0 = none, all reads global)
    int xcd_group = 16;                 // fused kernel: runs of that many consecutive workgroups on one XCD (0/1 = hardware order)
    int patch_margin = 8;               // ... and the widest margin of cells around the buoys' bounding box it may take
    int lanes = 2;                      // sitrk_run: 2 = the sorted buoys split into two lanes whose fused launches overlap, lane 1 on
                                        // sv_stream and half a launch behind lane 0 (1 = one stream, one launch at a time)
    int lane_min_wg = 7168;             // ... where the shorter lane keeps that many workgroups (4 rounds of 256 CUs x 7 workgroups)
    hipEvent_t lane_fork = nullptr, lane_join = nullptr;
    int coast_bin = 4;                  // sitrk_coast_build: bin side in quarters of sqrt(bounding-box area / segments), 1..64 (never changes results)
    int delaunay_bin = 3;               // sitrk_delaunay: cells per reach (side = reach / delaunay_bin, 2*delaunay_bin+1 cells a side searched), 1..4 (never changes results)
    int subsample_block = 1024;         // sitrk_subsample_cloud: points per workgroup of its resolve kernel (never changes results)
    int fill_threads = 8;               // host threads copying a pushed record (>= 8 MB) into the pinned staging (2 / 4 / 8: 26 / 36 / 47 GB/s on the box rows of C3)

    // records
    int nslots = 0, dtype = 0;
    size_t slab_bytes = 0;
    void *slabs = nullptr;              // nslots * [u|v|sic]
    uint8_t *kill9 = nullptr;           // nslots * (Nj*Ni): per cell the Survive bytes (tmask, sic, rmin_conc) of its 8 neighbours, one bit each
    unsigned char slot_dirty[4096] = {0};   // slab (re)written since its mask was derived
    // per slot: upload still in flight on copy_stream (the compute stream waits for slot_ready before it reads the
    // slot; events are created on first use), and the sequence number of the last launch that reads the slot (an upload
    // into it waits for that launch's event in the ring below, not for the whole compute stream)
    unsigned char slot_pending[4096] = {0};
    hipEvent_t slot_ready[4096] = {nullptr};
    // ... and a Survive derivation in flight on sv_stream: slot_sv[k] is recorded behind it (created on first use); the compute stream
    // waits for it before it reads the slot's bytes (slot_sv_pending), an upload into the slot before it overwrites the siconc it reads
    hipEvent_t slot_sv[4096] = {nullptr};
    unsigned char slot_sv_pending[4096] = {0};
    int async_survive = 0;              // knob: uploads derive their Survive bytes on sv_stream (1) or on the compute stream (0, default:
                                        // next to the fused loop, which needs its seven waves per SIMD, the co-running kernel costs more
                                        // than it hides -- profiles/r04r_*; behind a PCIe upload there is nothing to hide)
    long long slot_used_seq[4096];
    static constexpr int kLaunchRing = 64;
    hipEvent_t launch_ev[kLaunchRing] = {nullptr};
    long long launch_seq = 0;
    // rows [row_lo,row_hi) of the slot's u,v hold this record (whole record: 0..Nj); everything else is stale.
    // Survive bytes are valid for rows (row_lo, row_hi-1) and the domain rim.
    int slot_row_lo[4096] = {0}, slot_row_hi[4096] = {0};
    // the same for the columns (box ingest, round 4): columns [col_lo,col_hi) of those rows hold this record
    int slot_col_lo[4096] = {0}, slot_col_hi[4096] = {0};
    // host rows and columns of the live buoys at the last sitrk_buoy_rows() / sitrk_buoy_box(), and the records stepped
    // since (a host cell moves at most one row and one column per record): what a partly uploaded slot is checked against
    int band_jmin = 0, band_jmax = -1, band_age = -1;      // band_age < 0: not evaluated since sitrk_set_buoys
    int band_imin = 0, band_imax = -1;
    // asynchronous evaluation (sitrk_buoy_box_begin / _end): the reduction is queued on the compute stream, its result lands in
    // pinned host memory behind an event; records stepped after the begin are counted separately until the end adopts the result
    int *box_host = nullptr;            // 4 ints, pinned
    hipEvent_t box_ev = nullptr;
    bool box_pending = false;
    int box_pending_age = 0;
    // launch accounting (sitrk_launch_stats)
    long long n_fused_launches = 0, n_fused_records = 0, n_step_launches = 0;
    long long n_lane_segments = 0, n_lane_launches = 0;     // (sitrk_lane_stats)
    // sitrk_run_tlerp: theta[s] = (2s+1)/(2 nsub) - phase of every sub-step, on the device (1024 doubles, allocated at the first
    // call), and the (nsub, phase) it was filled for
    double *tlerp_theta = nullptr;
    int tlerp_nsub = 0;
    double tlerp_phase = -1.0;

    // buoys
    int64_t nP = 0;
    bool windowed = false;
    int32_t win_first_max = 0, win_last_min = 0;   // over all buoys: a launch whose records lie in [first_max, last_min] steps
                                                   // every live buoy at every record -> the form without the window test
    bool rim_buoys = false;             // some buoy was set in a cell with jT < 2 or iT < 2 (numpy negative-index wrap possible)
    sitrk::BuoyState st[2];             // double buffer for the sort
    int cur = 0;
    uint32_t *keys[2] = {nullptr, nullptr};
    int32_t *vals[2] = {nullptr, nullptr};
    void *sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    int resort_every = 512;             // re-sort cadence in steps (0 = never); measured best over 6000 steps at C3
    int steps_since_sort = 0;
    bool sorted_once = false;

    // deformation (sitrk_deform.hip): the positions of all buoys at sitrk_deform_mark, caller order, 16 B per buoy.  Allocated at
    // the first mark, freed -- and the mark cancelled -- with the buoys (sitrk_set_buoys, sitrk_destroy)
    sitrk::pt *deform_t0 = nullptr;
    bool deform_marked = false;
    int deform_jrec0 = 0;
    sitrk::PhaseTimer<3> deform_timer;  // around the scatter pass and the cell kernel of the last deform call

    // pair dispersion (sitrk_pairs.hip): the positions of all buoys at sitrk_pairs_mark and a validity byte each, caller order, 17 B
    // per buoy.  Allocated at the first mark, freed -- and the mark cancelled -- by sitrk_pairs_free and with the buoys.  Events
    // around the three phases of the last call -- binning, pairs, table --, and its candidate tests
    sitrk::pt *pairs_t0 = nullptr;
    int8_t *pairs_v0 = nullptr;
    bool pairs_marked = false;
    int pairs_jrec0 = 0;
    sitrk::PhaseTimer<4> pairs_timer;
    unsigned long long pairs_tests = 0;

    sitrk::CoastState coast;            // distance to the coastline (sitrk_coast.hip)

    // quadrangles from triangles (sitrk_quadmesh.hip): events around the phases of the last call -- adjacency, scores, rounds, compaction
    sitrk::PhaseTimer<5> quad_timer;

    // bounded Delaunay triangulation (sitrk_delaunay.hip): events around the phases of the last call -- binning, triangles,
    // compaction -- and its in-circle tests, all of them / those that took the 128-bit path
    sitrk::PhaseTimer<4> dl_timer;
    unsigned long long dl_tests = 0, dl_exact = 0;

    // device-resident quadrangle meshes (sitrk_mesh.hip): freed with the buoys, whose indices they hold.  Events around the device
    // chain of the last build, and around the pass over the buoys, the cell kernel and the final sum of the last deform
    sitrk::Mesh mesh[SITRK_MESH_MAX];
    sitrk::PhaseTimer<2> mesh_build_timer;
    sitrk::PhaseTimer<4> mesh_deform_timer;

    // rasterised cells (sitrk_raster.hip): events around the fill with the cell kernel and around the gather kernel of the last
    // call; with the knob raster_count its centres found inside a drawn cell (= the atomics issued)
    sitrk::PhaseTimer<3> raster_timer;
    int raster_count = 0;               // knob: count them (a measurement build of the cell kernel; never changes results)
    bool raster_counted = false;
    unsigned long long raster_claims = 0;

    // coarse-grained deformation (sitrk_coarse.hip): events around the five phases of the last call -- terms, sort, level 0,
    // pyramid, table
    sitrk::PhaseTimer<6> coarse_timer;

    // labelled features (sitrk_label.hip): events around the three phases of the last call -- mask, labels, table
    sitrk::PhaseTimer<4> label_timer;

    // features from window to window (sitrk_track.hip): the kept label maps, which outlive the buoys and the meshes, and the
    // allocation the last replaced map left behind, taken again by the next call that fills a slot.  Events around the three
    // phases of the last match -- keys, sort, rows --, and around the kernels of the last advect behind its rasters
    sitrk::KeptMap keep[SITRK_KEEP_MAX];
    int32_t *keep_spare = nullptr;
    size_t keep_spare_cap = 0;
    sitrk::PhaseTimer<4> match_timer;
    sitrk::PhaseTimer<2> advect_timer;

    // skeletons of a label map (sitrk_skeleton.hip): events around the three phases of the last call -- thinning, table, nodes
    sitrk::PhaseTimer<4> skel_timer;
    int skeleton_batch = 0;             // knob: sub-iterations per launch of the thinning kernel, 1..8; 0 = as shipped (never changes results)

    // distribution of values (sitrk_dist.hip): events around the phases of the last call -- keys, histogram, the top-digit pass
    // of the selection, its other passes -- and the digit passes it ran
    sitrk::PhaseTimer<5> dist_timer;
    int dist_passes = 0;
    int dist_aggregate = 0;             // knob: a wave whose matching keys share the digit adds their number once (measured no faster:
                                        // DESIGN.md 3.21; never changes results)

    // scratch for fetch / locate
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    unsigned long long *counter = nullptr;   // device scalar for reductions
};

// --------------------------------------------------------------------------- host side shared by the translation units
#define SITRK_API extern "C" __attribute__((visibility("default")))

namespace sitrk {

int fail(sitrk_ctx *h, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
int ensure_scratch(sitrk_ctx *h, size_t bytes);
// sitrk_sample.hip reads a resident slot: the compute stream ordered behind an upload of `slot` still in flight on the copy
// stream (sitrk.hip); *field = device address of field 0 u / 1 v / 2 siconc of the slot's slab
int slot_order_read(sitrk_ctx *h, int slot, int field, const void **field_dev);
// sitrk_deform.hip: frees the snapshot of sitrk_deform_mark and cancels the mark (free_buoys of sitrk.hip); destroy = the timer
// too
void deform_release(sitrk_ctx *h, bool destroy);
// ... and queues its pass over the buoys on the compute stream: out (nP) = every buoy's position in the caller's order, NaN in y
// for a buoy that is not alive now (sitrk_quadmesh.hip)
int deform_points_now(sitrk_ctx *h, pt *out);
// ... and the pass of sitrk_deform_since_mark: NaN in y also for a buoy whose record window does not cover [jrec0, jrec1] (sitrk_mesh.hip)
int deform_points_span(sitrk_ctx *h, int jrec0, int jrec1, pt *out);
// sitrk_pairs.hip: frees the snapshot of sitrk_pairs_mark and cancels the mark (free_buoys of sitrk.hip); destroy = the timer too
void pairs_release(sitrk_ctx *h, bool destroy);
// sitrk_mesh.hip: frees every mesh (free_buoys of sitrk.hip); destroy = the timers too
void mesh_release(sitrk_ctx *h, bool destroy);
// ... and the body of sitrk_mesh_deform behind its argument checks (mesh_deform_check), everything left in the transient scratch:
// the pass over the buoys, the cell kernel and, when asked for, the final sum are queued on the compute stream and the pointers
// of MeshDeformDev say where their results lie.  `extra` bytes of the same scratch layout come with them for the caller's own
// buffers (sitrk_raster.hip, sitrk_coarse.hip).  An empty mesh queues nothing and returns null pointers next to `extra`.
struct MeshDeformDev {
    int64_t nQ = 0;
    const int32_t *quads = nullptr;     // (nQ,4) the mesh's own
    const pt *t0 = nullptr;             // (nQ,4) the mesh's own
    const pt *p1 = nullptr;             // (nP) current positions in the caller's order, NaN in y = no valid vertex
    const double *out = nullptr;        // (5,nQ)
    const int8_t *status = nullptr;     // (nQ)
    const double *stats = nullptr;      // (SITRK_MESH_NSTATS)
    char *extra = nullptr;
};
int mesh_deform_check(sitrk_ctx *h, const char *fn, int mesh, int jrec1);
int mesh_deform_core(sitrk_ctx *h, int mesh, int jrec1, bool want_out, bool want_status, bool want_stats, size_t extra,
                     MeshDeformDev *r);
// sitrk_raster.hip: the device side of its entry points, for a caller that goes on with the raster on the device (sitrk_label.hip):
// the grid's checks, and the fill, cell and gather kernels queued on the compute stream.  cnt: three counters -- cells with a bad
// index, owned pixels, and with the knob raster_count the centres inside a drawn cell.  out (5,nC) may be null when fields is
struct RasterGrid {
    double y0, x0, d;
    int ny, nx;
};
struct RasterJob {
    int64_t nC = 0, nP = 0;
    int nv = 4;
    bool block = false;                 // pts is (nC,nv) in cell order, no indices
    const int32_t *cells = nullptr;
    const pt *pts = nullptr;
    const int8_t *flag = nullptr;
    bool only_status1 = false;
    const double *out = nullptr;
    int32_t *owner = nullptr;
    double *fields = nullptr;
    unsigned long long *cnt = nullptr;
};
int raster_check_grid(sitrk_ctx *h, const char *fn, double y0, double x0, double d, int ny, int nx);
int raster_run(sitrk_ctx *h, const RasterJob &j, const RasterGrid &g);
// ... and the shape of a raster that is labelled, kept or thinned: ny, nx in 1..32768 and at most 2^28 pixels
int check_raster_shape(sitrk_ctx *h, const char *fn, int ny, int nx);
// sitrk_label.hip: the temporary storage, a multiple of 256 bytes, of a rocprim::exclusive_scan over n int32 values
int scan_i32_bytes(sitrk_ctx *h, int64_t n, size_t *bytes);
// ... and the body of sitrk_mesh_features behind the handle's check, for sitrk_mesh_features_keep (sitrk_track.hip): keep_map (ny*nx
// on the device, may be null) receives the labels of the components of at least min_pix pixels, -1 elsewhere
int mesh_features_body(sitrk_ctx *h, const char *fn, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny,
                       int nx, int what, int sgn, double thr, int conn, int64_t min_pix, int64_t maxfeat, int32_t *labels, int64_t *table,
                       int64_t *nfeat, int64_t *ncomp, int64_t *nactive, int32_t *keep_map);
// sitrk_track.hip: queues the kernel behind keep_map on the compute stream and synchronises; frees the kept maps and releases the
// timers (sitrk_destroy)
int keep_from_labels(sitrk_ctx *h, int64_t npix, const int32_t *labels, const int32_t *flag, int32_t *keep_map);
void track_release(sitrk_ctx *h);
// sitrk_skeleton.hip: the knob skeleton_batch behind its range check (sitrk_set_tuning)
int skeleton_set_batch(sitrk_ctx *h, int value);
// sitrk_dist.hip: the knob dist_aggregate behind its range check (sitrk_set_tuning)
int dist_set_aggregate(sitrk_ctx *h, int value);
// sitrk_coast.hip: frees the coast index (sitrk_destroy: the timer too); grid_changed = only an index that was built from
// the context's grid (sitrk_set_grid)
void coast_release(sitrk_ctx *h, bool grid_changed, bool destroy);

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace sitrk

#define HIPCHK(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) return sitrk::fail(h, SITRK_EHIP, "%s -> %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define NEED(cond, msg)                                \
    do {                                               \
        if (!(cond)) return sitrk::fail(h, SITRK_EINVAL, msg); \
    } while (0)

// a step of the library's own that returns a SITRK_* code
#define RCCHK(call)              \
    do {                         \
        int rc_ = (call);        \
        if (rc_) return rc_;     \
    } while (0)

namespace sitrk {

template <int N>
int PhaseTimer<N>::create(sitrk_ctx *h)
{
    for (hipEvent_t &e : ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    return SITRK_OK;
}

template <int N>
int PhaseTimer<N>::begin(sitrk_ctx *h)
{
    RCCHK(create(h));
    complete = false;
    return SITRK_OK;
}

template <int N>
int PhaseTimer<N>::mark(sitrk_ctx *h, int k)
{
    HIPCHK(hipEventRecord(ev[k], h->stream));
    return SITRK_OK;
}

template <int N>
int PhaseTimer<N>::elapsed(sitrk_ctx *h, int k, float *ms)
{
    if (ms) HIPCHK(hipEventElapsedTime(ms, ev[k], ev[k + 1]));
    return SITRK_OK;
}

template <int N>
void PhaseTimer<N>::release()
{
    for (hipEvent_t &e : ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    complete = false;
}

// Scratch carver: hands out typed pieces of one allocation in order, each rounded up to 256 bytes.  A layout is a callable that
// takes its pieces from the Carver it is given; carve_scratch() runs it twice -- over a null base, where only the offsets add up,
// to size h->scratch, then over h->scratch to place the pointers -- so the total requested and the placement come out of the
// same statements and cannot disagree.  Every entry point that stages arrays in h->scratch goes through it.
struct Carver {
    char *base = nullptr;
    size_t off = 0;
    template <typename T>
    void take(T *&p, size_t count, size_t round = 256)
    {
        p = base ? (T *)(base + off) : nullptr;
        off += (count * sizeof(T) + round - 1) / round * round;
    }
};

template <typename Layout>
static int carve_scratch(sitrk_ctx *h, Layout &&layout)
{
    Carver size;
    layout(size);
    RCCHK(ensure_scratch(h, size.off));
    Carver place;
    place.base = (char *)h->scratch;
    layout(place);
    return SITRK_OK;
}

// The same two passes for a layout that lies behind the buffers of a mesh's deformation: the layout is sized, mesh_deform_core
// carves that many bytes behind its own buffers and queues its kernels, and the layout is placed at m->extra
template <typename Layout>
static int carve_behind_mesh(sitrk_ctx *h, int mesh, int jrec1, bool want_out, bool want_status, bool want_stats, Layout &&layout,
                             MeshDeformDev *m)
{
    Carver size;
    layout(size);
    RCCHK(mesh_deform_core(h, mesh, jrec1, want_out, want_status, want_stats, size.off, m));
    Carver place;
    place.base = m->extra;
    layout(place);
    return SITRK_OK;
}

// Copies on the compute stream between a host array and a typed device array of `count` elements: the device pointer's type
// gives the element size (the host side of the ABI is plain double / int arrays, e.g. 2 doubles per pt)
template <typename T>
static hipError_t upload(sitrk_ctx *h, T *dst_dev, const void *src_host, size_t count)
{
    return hipMemcpyAsync(dst_dev, src_host, count * sizeof(T), hipMemcpyHostToDevice, h->stream);
}

template <typename T>
static hipError_t download(sitrk_ctx *h, void *dst_host, const T *src_dev, size_t count)
{
    return hipMemcpyAsync(dst_host, src_dev, count * sizeof(T), hipMemcpyDeviceToHost, h->stream);
}

// ---- the cores of sitrk_delaunay.hip and sitrk_quadmesh.hip: everything behind the points, rows left on the device.  The entry
// points of those files add the download; sitrk_mesh_build runs both back to back out of one scratch layout.
struct __attribute__((aligned(16))) ipt { int64_t y, x; };     // a point snapped to 2^-20 km
struct DlBuffers {
    ipt *xy, *xys, *xyv;
    uint32_t *k0, *k1;
    int32_t *v0, *perm, *cbeg, *rval0, *rval1, *tris;          // tris: (nT,3) rows of the result
    int8_t *vertex;
    unsigned long long *rkey0, *rkey1;
    long long *red;
    char *sort_tmp;
    size_t sort_bytes;
};
int dl_check_rmax(sitrk_ctx *h, const char *fn, double rmax_km);
int dl_sort_bytes(sitrk_ctx *h, int64_t nP, size_t *bytes);
void dl_carve(Carver &c, DlBuffers &b, int64_t nP);
// d_pts (nP; masked by d_mask when given) is on the device and the stream is behind what made it; *nT rows in b.tris, b.vertex filled
int dl_core(sitrk_ctx *h, const char *fn, int64_t nP, const pt *d_pts, const int8_t *d_mask, const DlBuffers &b, double rmax_km,
            int64_t *nT);

struct EdgeTable {
    unsigned long long *key;    // all ones or p << 32 | q
    unsigned long long *val;    // low 32 bits: triangles on the edge; high 32 bits: sum of their ids mod 2^32
    uint64_t mask;              // slots - 1, slots a power of two
};
struct QuadBuffers {
    int32_t *tris, *nbr, *mate, *pick, *quads, *tri_quad;      // quads (nQ,4), tri_quad (nT): the result
    int8_t *live;
    double *score;
    unsigned *block_count;
    int64_t *block_off;
    EdgeTable tab;
    uint64_t slots;
};
int quad_check_params(sitrk_ctx *h, const char *fn, double cos_lo, double cos_hi, double ratio_min, double area_min, double area_max);
QuadParams quad_params(double cos_lo, double cos_hi, double ratio_min, double area_min, double area_max);
void quad_carve(Carver &c, QuadBuffers &b, int64_t nT);        // room for nT triangles; the core takes any count up to it
// d_pts (nP, NaN in y = no valid vertex) and the triangles d_tris (nT,3) are on the device and the stream is behind what made
// them; *nQ rows in b.quads, b.tri_quad filled
int quad_core(sitrk_ctx *h, const char *fn, int64_t nP, const pt *d_pts, int64_t nT, const int32_t *d_tris, const QuadBuffers &b,
              const QuadParams &c, int64_t *nQ, int *rounds);

}  // namespace sitrk
