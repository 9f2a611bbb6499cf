// sitrk_track.hip -- features from window to window (sitrk_mesh_features_keep, sitrk_keep_*, sitrk_mesh_features_advect,
// sitrk_features_match): an EXTRA the reference does not have.  A label map is kept on the device, carried to the end of its
// window by the cells of the mesh it was drawn from, and compared pixel by pixel with the map of the next window, which is made
// at the same instant on the same grid.  What comes down is one row (a, b, count) per pair of features that meet.  The contract
// is in include/sitrk.h and DESIGN.md 3.18: all integer, so every bit is pinned.
//
// Kernels, wave64, 256 lanes per workgroup, no scratch memory, no LDS but the few words of a workgroup's counts:
//   keep_labels_kernel    one pixel per lane: its label where the label's component was flagged (npix >= min_pix), else -1
//   keep_range_kernel     (sitrk_keep_put) at most 2048 workgroups: the values outside [-1, npix) counted by ballot
//   advect_fill_kernel    one cell per lane: INT32_MAX
//   advect_min_kernel     one pixel per lane: the pixel's label into the cell that owns it at t0, one integer atomicMin without a
//                         return value
//   advect_cells_kernel   at most 2048 workgroups: the cells that received a label counted by ballot
//   advect_gather_kernel  at most 2048 workgroups, a later launch on the same stream: the label of the cell that owns the pixel at
//                         t1, INT32_MAX and no owner -> -1; the carried pixels counted by ballot
//   match_scan_kernel<REACH, EMIT>   at most 2048 workgroups, one pixel per lane and trip: the (2 REACH + 1)^2 values of B around
//                         the shifted pixel are read through the cache in a fixed order into registers (the loops are unrolled, so
//                         every index is a constant and nothing goes to scratch); a value counts where it is >= 0 and no earlier
//                         one of the scan equals it.  EMIT = false: the number of such values per pixel, and over the launch their
//                         sum E and the pixels with at least one.  EMIT = true: the keys a << nb | b at the pixel's offset
//   (rocprim::exclusive_scan)   counts -> offsets; (rocprim::radix_sort_keys) on the 2 nb bits a key has
//   match_bounds_kernel   one key per lane: 1 where the key differs from the one in front of it
//   (rocprim::exclusive_scan)   flags -> the row of every run of equal keys
//   match_rows_kernel     one key per lane: the first key of a run whose row is below maxpair stores (a, b), the first and the last
//                         add -index and index + 1 to the row's count by one integer atomic each; the last key stores npair
// No kernel depends on a plain load seeing what another workgroup stored in the same launch, and no lane waits for another
// workgroup: the phases are kernel boundaries on the handle's stream.  Every loop is bounded by a count fixed before it starts.
// Vector stores only, integer atomics only.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include "sitrk_internal.h"

namespace sitrk {

namespace {

constexpr int kTrThreads = 256;
constexpr unsigned kTrBlocks = 2048;               // 256 CUs x 8 resident workgroups
constexpr int32_t kTrNone = INT32_MAX;
constexpr int64_t kTrMaxKeys = ((int64_t)1 << 31) - 1;
constexpr int kTrMaxShift = 32768;

// counters of one call on the device
enum { kTrE = 0, kTrHit = 1, kTrPair = 2, kTrBad = 3, kTrN = 4 };

// the counts a, b of the waves of a workgroup (the same in all lanes of a wave) into two counters, one atomic each
__device__ __forceinline__ void block_add2(long long a, long long b, unsigned long long *ca, unsigned long long *cb)
{
    __shared__ long long sm[kTrThreads / 64][2];
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long x = sm[0][0], y = sm[0][1];
#pragma unroll
        for (int w = 1; w < kTrThreads / 64; w++) { x += sm[w][0]; y += sm[w][1]; }
        if (x && ca) atomicAdd(ca, (unsigned long long)x);
        if (y && cb) atomicAdd(cb, (unsigned long long)y);
    }
}

__global__ __launch_bounds__(kTrThreads) void keep_labels_kernel(int64_t npix, const int32_t *__restrict__ labels,
                                                                 const int32_t *__restrict__ flag, int32_t *__restrict__ map)
{
    const int64_t p = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (p >= npix) return;
    const int32_t l = labels[p];
    map[p] = l >= 0 && flag[l] ? l : -1;
}

__global__ __launch_bounds__(kTrThreads) void keep_range_kernel(int64_t npix, int trips, const int32_t *__restrict__ map,
                                                                unsigned long long *__restrict__ tot)
{
    const int64_t stride = (int64_t)gridDim.x * kTrThreads;
    int64_t p = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    long long bad = 0;
    for (int t = 0; t < trips; t++, p += stride) {
        bool b = false;
        if (p < npix) {
            const int32_t v = map[p];
            b = v < -1 || (int64_t)v >= npix;
        }
        bad += __popcll(__ballot(b));
    }
    block_add2(bad, 0, tot + kTrBad, nullptr);
}

__global__ __launch_bounds__(kTrThreads) void advect_fill_kernel(int64_t nQ, int32_t *__restrict__ cellfeat)
{
    const int64_t q = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (q < nQ) cellfeat[q] = kTrNone;
}

__global__ __launch_bounds__(kTrThreads) void advect_min_kernel(int64_t npix, int64_t nQ, const int32_t *__restrict__ owner0,
                                                                const int32_t *__restrict__ map, int32_t *cellfeat)
{
    const int64_t p = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (p >= npix) return;
    const int32_t q = owner0[p], l = map[p];
    if (q >= 0 && (int64_t)q < nQ && l >= 0) (void)__hip_atomic_fetch_min(cellfeat + q, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kTrThreads) void advect_cells_kernel(int64_t nQ, int trips, const int32_t *__restrict__ cellfeat,
                                                                  unsigned long long *__restrict__ tot)
{
    const int64_t stride = (int64_t)gridDim.x * kTrThreads;
    int64_t q = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    long long n = 0;
    for (int t = 0; t < trips; t++, q += stride) n += __popcll(__ballot(q < nQ && cellfeat[q] != kTrNone));
    block_add2(n, 0, tot + 0, nullptr);
}

__global__ __launch_bounds__(kTrThreads) void advect_gather_kernel(int64_t npix, int trips, int64_t nQ, const int32_t *__restrict__ owner1,
                                                                   const int32_t *__restrict__ cellfeat, int32_t *__restrict__ out,
                                                                   unsigned long long *__restrict__ tot)
{
    const int64_t stride = (int64_t)gridDim.x * kTrThreads;
    int64_t p = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    long long n = 0;
    for (int t = 0; t < trips; t++, p += stride) {
        int32_t v = -1;
        if (p < npix) {
            const int32_t q = owner1[p];
            if (q >= 0 && (int64_t)q < nQ) {
                const int32_t f = cellfeat[q];
                v = f == kTrNone ? -1 : f;
            }
            out[p] = v;
        }
        n += __popcll(__ballot(v >= 0));
    }
    block_add2(n, 0, tot + 1, nullptr);
}

// The distinct values >= 0 of B in the window of (2 REACH + 1)^2 pixels around (j + dj, i + di), scanned row by row; f(b) is
// called once per such value, in the order of the scan.  Returns how many there are.
template <int REACH, typename F>
__device__ __forceinline__ int scan_window(const int32_t *__restrict__ B, int ny, int nx, int j, int i, F &&f)
{
    constexpr int W = 2 * REACH + 1;
    int32_t v[W * W];
#pragma unroll
    for (int s = 0; s < W; s++) {
        const int jj = j + s - REACH;
#pragma unroll
        for (int t = 0; t < W; t++) {
            const int ii = i + t - REACH;
            v[s * W + t] = jj >= 0 && jj < ny && ii >= 0 && ii < nx ? B[(int64_t)jj * nx + ii] : -1;
        }
    }
    int n = 0;
#pragma unroll
    for (int k = 0; k < W * W; k++) {
        bool fresh = v[k] >= 0;
#pragma unroll
        for (int m = 0; m < k; m++) fresh = fresh && v[m] != v[k];
        if (fresh) { f(v[k]); n++; }
    }
    return n;
}

template <int REACH, bool EMIT>
__global__ __launch_bounds__(kTrThreads) void match_scan_kernel(int ny, int nx, int dj, int di, int trips, int nb, const int32_t *__restrict__ A,
                                                                const int32_t *__restrict__ B, int32_t *__restrict__ cnt,
                                                                const int32_t *__restrict__ off, unsigned long long *__restrict__ keys,
                                                                unsigned long long *__restrict__ tot)
{
    const int64_t npix = (int64_t)ny * nx;
    const int64_t stride = (int64_t)gridDim.x * kTrThreads;
    int64_t p = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    long long sum = 0, hit = 0;
    for (int t = 0; t < trips; t++, p += stride) {
        int n = 0;
        if (p < npix) {
            const int32_t a = A[p];
            if (a >= 0) {
                const int j = (int)(p / nx), i = (int)(p - (int64_t)j * nx);
                if (EMIT) {
                    unsigned long long *dst = keys + off[p];
                    const unsigned long long hi = (unsigned long long)a << nb;
                    n = scan_window<REACH>(B, ny, nx, j + dj, i + di, [&](int32_t b) { *dst++ = hi | (unsigned long long)b; });
                } else {
                    n = scan_window<REACH>(B, ny, nx, j + dj, i + di, [](int32_t) {});
                }
            }
            if (!EMIT && cnt) cnt[p] = n;
        }
        if (!EMIT) {
            int s = n;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            sum += s;
            hit += __popcll(__ballot(n > 0));
        }
    }
    if (!EMIT) block_add2(sum, hit, tot + kTrE, tot + kTrHit);
}

__global__ __launch_bounds__(kTrThreads) void match_bounds_kernel(int64_t E, const unsigned long long *__restrict__ keys, int32_t *__restrict__ flag)
{
    const int64_t k = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (k >= E) return;
    flag[k] = k == 0 || keys[k - 1] != keys[k] ? 1 : 0;
}

__global__ __launch_bounds__(kTrThreads) void match_rows_kernel(int64_t E, int64_t maxpair, int nb, const unsigned long long *__restrict__ keys,
                                                                const int32_t *__restrict__ flag, const int32_t *__restrict__ row,
                                                                long long *pairs, unsigned long long *__restrict__ tot)
{
    const int64_t k = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (k >= E) return;
    const unsigned long long key = keys[k];
    const bool head = flag[k] != 0;
    const bool tail = k == E - 1 || keys[k + 1] != key;
    const int64_t r = (int64_t)row[k] + (head ? 1 : 0) - 1;            // the run this key belongs to
    if (k == E - 1) tot[kTrPair] = (unsigned long long)(r + 1);
    if (r >= maxpair || !(head || tail)) return;
    long long *t = pairs + r * 3;
    if (head) {
        t[0] = (long long)(key >> nb);
        t[1] = (long long)(key & (((unsigned long long)1 << nb) - 1));
    }
    const long long d = (tail ? k + 1 : 0) - (head ? k : 0);           // over the run's first and last key: its length
    __hip_atomic_fetch_add(t + 2, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------ the slots
int keep_check_slot(sitrk_ctx *h, const char *fn, const char *name, int keep, bool filled)
{
    if (keep < 0 || keep >= SITRK_KEEP_MAX) return fail(h, SITRK_EINVAL, "%s: %s must be in 0..%d (got %d)", fn, name, SITRK_KEEP_MAX - 1, keep);
    if (filled && !h->keep[keep].map) return fail(h, SITRK_EINVAL, "%s: kept map %d is empty", fn, keep);
    return SITRK_OK;
}

int keep_check_shape(sitrk_ctx *h, const char *fn, int ny, int nx, int conn, int64_t min_pix)
{
    RCCHK(check_raster_shape(h, fn, ny, nx));
    if (conn != 4 && conn != 8) return fail(h, SITRK_EINVAL, "%s: conn must be 4 (edge neighbours) or 8 (edge and corner neighbours), got %d", fn, conn);
    if (min_pix < 1) return fail(h, SITRK_EINVAL, "%s: min_pix must be >= 1 (got %lld)", fn, (long long)min_pix);
    return SITRK_OK;
}

// an allocation of npix pixels for a map that is not in a slot yet: the spare one where it is large enough
int keep_take(sitrk_ctx *h, size_t npix, int32_t **map, size_t *cap)
{
    if (h->keep_spare && h->keep_spare_cap >= npix) {
        *map = h->keep_spare; *cap = h->keep_spare_cap;
        h->keep_spare = nullptr; h->keep_spare_cap = 0;
        return SITRK_OK;
    }
    *map = nullptr;
    HIPCHK(hipMalloc((void **)map, npix * sizeof(int32_t)));
    *cap = npix;
    return SITRK_OK;
}

// ... and what becomes of an allocation no slot holds any more: it is the spare one, the smaller of the two is freed
void keep_give(sitrk_ctx *h, int32_t *map, size_t cap)
{
    if (!map) return;
    if (h->keep_spare && h->keep_spare_cap >= cap) { (void)hipFree(map); return; }
    if (h->keep_spare) (void)hipFree(h->keep_spare);
    h->keep_spare = map; h->keep_spare_cap = cap;
}

void keep_commit(sitrk_ctx *h, int keep, int32_t *map, size_t cap, int ny, int nx, int conn, int64_t min_pix)
{
    KeptMap &k = h->keep[keep];
    int32_t *old = k.map;
    const size_t old_cap = k.cap;
    k.map = map; k.cap = cap; k.ny = ny; k.nx = nx; k.conn = conn; k.min_pix = min_pix;
    keep_give(h, old, old_cap);
}

template <bool EMIT>
int launch_scan(sitrk_ctx *h, int reach, int ny, int nx, int dj, int di, int nb, const int32_t *A, const int32_t *B, int32_t *cnt,
                const int32_t *off, unsigned long long *keys, unsigned long long *tot)
{
    const Strided s((int64_t)ny * nx, kTrThreads, kTrBlocks);
    if (reach == 0)
        hipLaunchKernelGGL((match_scan_kernel<0, EMIT>), dim3(s.blocks), dim3(kTrThreads), 0, h->stream, ny, nx, dj, di, s.trips, nb, A, B, cnt, off, keys, tot);
    else if (reach == 1)
        hipLaunchKernelGGL((match_scan_kernel<1, EMIT>), dim3(s.blocks), dim3(kTrThreads), 0, h->stream, ny, nx, dj, di, s.trips, nb, A, B, cnt, off, keys, tot);
    else
        hipLaunchKernelGGL((match_scan_kernel<2, EMIT>), dim3(s.blocks), dim3(kTrThreads), 0, h->stream, ny, nx, dj, di, s.trips, nb, A, B, cnt, off, keys, tot);
    HIPCHK(hipGetLastError());
    return SITRK_OK;
}

}  // namespace

int keep_from_labels(sitrk_ctx *h, int64_t npix, const int32_t *labels, const int32_t *flag, int32_t *keep_map)
{
    hipLaunchKernelGGL(keep_labels_kernel, dim3(nblk(npix, kTrThreads)), dim3(kTrThreads), 0, h->stream, npix, labels, flag, keep_map);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

void track_release(sitrk_ctx *h)
{
    for (KeptMap &k : h->keep) {
        if (k.map) (void)hipFree(k.map);
        k = KeptMap();
    }
    if (h->keep_spare) (void)hipFree(h->keep_spare);
    h->keep_spare = nullptr; h->keep_spare_cap = 0;
    h->match_timer.release();
    h->advect_timer.release();
}

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_mesh_features_keep(sitrk_t *h, int keep, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny,
                                       int nx, int what, int sgn, double thr, int conn, int64_t min_pix, int64_t maxfeat, int32_t *labels,
                                       int64_t *table, int64_t *nfeat, int64_t *ncomp, int64_t *nactive)
{
    const char *fn = "sitrk_mesh_features_keep";
    NEED(h, "null handle");
    RCCHK(keep_check_slot(h, fn, "keep", keep, false));
    // the body refuses a bad raster before any device work, with the message of its first failing check; the allocation is sized
    // from a checked shape only
    if (check_raster_shape(h, fn, ny, nx))
        return mesh_features_body(h, fn, mesh, jrec1, at_t1, y0_km, x0_km, d_km, ny, nx, what, sgn, thr, conn, min_pix, maxfeat, labels, table,
                                  nfeat, ncomp, nactive, nullptr);
    HIPCHK(hipSetDevice(h->device));
    int32_t *map; size_t cap;
    RCCHK(keep_take(h, (size_t)ny * nx, &map, &cap));
    const int rc = mesh_features_body(h, fn, mesh, jrec1, at_t1, y0_km, x0_km, d_km, ny, nx, what, sgn, thr, conn, min_pix, maxfeat, labels,
                                      table, nfeat, ncomp, nactive, map);
    if (rc) { keep_give(h, map, cap); return rc; }                     // the slot is what it was
    keep_commit(h, keep, map, cap, ny, nx, conn, min_pix);
    return SITRK_OK;
}

SITRK_API int sitrk_keep_put(sitrk_t *h, int keep, int ny, int nx, const int32_t *map, int conn, int64_t min_pix)
{
    const char *fn = "sitrk_keep_put";
    NEED(h, "null handle");
    RCCHK(keep_check_slot(h, fn, "keep", keep, false));
    RCCHK(keep_check_shape(h, fn, ny, nx, conn, min_pix));
    if (!map) return fail(h, SITRK_EINVAL, "%s: null map", fn);
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)ny * nx;
    unsigned long long *d_tot;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_tot, kTrN); }));
    int32_t *d_map; size_t cap;
    RCCHK(keep_take(h, (size_t)npix, &d_map, &cap));
    unsigned long long tot[kTrN] = {0, 0, 0, 0};
    const Strided s(npix, kTrThreads, kTrBlocks);
    hipError_t e = hipMemsetAsync(d_tot, 0, kTrN * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = upload(h, d_map, map, (size_t)npix);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(keep_range_kernel, dim3(s.blocks), dim3(kTrThreads), 0, h->stream, npix, s.trips, d_map, d_tot);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = download(h, tot, d_tot, kTrN);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        keep_give(h, d_map, cap);
        return fail(h, SITRK_EHIP, "%s: %s", fn, hipGetErrorString(e));
    }
    if (tot[kTrBad]) {
        keep_give(h, d_map, cap);
        return fail(h, SITRK_EINDEX, "%s: %llu value(s) of the map lie outside [-1, %lld)", fn, tot[kTrBad], (long long)npix);
    }
    keep_commit(h, keep, d_map, cap, ny, nx, conn, min_pix);
    return SITRK_OK;
}

SITRK_API int sitrk_keep_get(sitrk_t *h, int keep, int *ny, int *nx, int *conn, int64_t *min_pix, int32_t *map)
{
    const char *fn = "sitrk_keep_get";
    NEED(h, "null handle");
    RCCHK(keep_check_slot(h, fn, "keep", keep, true));
    const KeptMap &k = h->keep[keep];
    if (map) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(download(h, map, k.map, (size_t)k.ny * k.nx));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (ny) *ny = k.ny;
    if (nx) *nx = k.nx;
    if (conn) *conn = k.conn;
    if (min_pix) *min_pix = k.min_pix;
    return SITRK_OK;
}

SITRK_API int sitrk_keep_free(sitrk_t *h, int keep)
{
    NEED(h, "null handle");
    RCCHK(keep_check_slot(h, "sitrk_keep_free", "keep", keep, false));
    KeptMap &k = h->keep[keep];
    if (k.map) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipFree(k.map));
    }
    k = KeptMap();
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_features_advect(sitrk_t *h, int keep_from, int keep_to, int mesh, int jrec1, double y0_km, double x0_km, double d_km,
                                         int ny, int nx, int64_t *ncells, int64_t *ncarried)
{
    const char *fn = "sitrk_mesh_features_advect";
    NEED(h, "null handle");
    RCCHK(keep_check_slot(h, fn, "keep_from", keep_from, false));
    RCCHK(keep_check_slot(h, fn, "keep_to", keep_to, false));
    RCCHK(mesh_deform_check(h, fn, mesh, jrec1));
    RCCHK(raster_check_grid(h, fn, y0_km, x0_km, d_km, ny, nx));
    RCCHK(keep_check_slot(h, fn, "keep_from", keep_from, true));
    const KeptMap from = h->keep[keep_from];
    if (from.ny != ny || from.nx != nx)
        return fail(h, SITRK_EINVAL, "%s: kept map %d is %d x %d, the grid %d x %d", fn, keep_from, from.ny, from.nx, ny, nx);
    if (ncells) *ncells = 0;
    if (ncarried) *ncarried = 0;
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)ny * nx;
    const int64_t nQ = h->mesh[mesh].nQ;
    int32_t *d_o0, *d_o1, *d_cellfeat; unsigned long long *d_cnt0, *d_cnt1, *d_tot;
    auto layout = [&](Carver &c) {
        c.take(d_o0, npix); c.take(d_o1, npix); c.take(d_cellfeat, nQ > 0 ? nQ : 1); c.take(d_cnt0, 3); c.take(d_cnt1, 3); c.take(d_tot, 2);
    };
    int32_t *d_map; size_t cap;
    RCCHK(keep_take(h, (size_t)npix, &d_map, &cap));
    unsigned long long cnt0[3] = {0, 0, 0}, cnt1[3] = {0, 0, 0}, tot[2] = {0, 0};
    // everything that can fail behind the allocation: the slot stays what it was
    auto run = [&]() -> int {
        MeshDeformDev m;
        RCCHK(carve_behind_mesh(h, mesh, jrec1, false, true, false, layout, &m));
        if (m.nQ != nQ) return fail(h, SITRK_EHIP, "%s: the mesh changed under the call", fn);
        const RasterGrid g = {y0_km, x0_km, d_km, ny, nx};
        RasterJob r0;                                                  // the two draws of sitrk_mesh_raster
        r0.nC = m.nQ; r0.nP = h->nP; r0.nv = 4; r0.flag = m.status; r0.owner = d_o0; r0.cnt = d_cnt0;
        r0.block = true; r0.pts = m.t0;
        RCCHK(raster_run(h, r0, g));
        RasterJob r1;
        r1.nC = m.nQ; r1.nP = h->nP; r1.nv = 4; r1.flag = m.status; r1.owner = d_o1; r1.cnt = d_cnt1;
        r1.cells = m.quads; r1.pts = m.p1; r1.only_status1 = true;
        RCCHK(raster_run(h, r1, g));
        RCCHK(h->advect_timer.begin(h));
        HIPCHK(hipMemsetAsync(d_tot, 0, 2 * sizeof(unsigned long long), h->stream));
        RCCHK(h->advect_timer.mark(h, 0));
        if (nQ > 0) {
            hipLaunchKernelGGL(advect_fill_kernel, dim3(nblk(nQ, kTrThreads)), dim3(kTrThreads), 0, h->stream, nQ, d_cellfeat);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(advect_min_kernel, dim3(nblk(npix, kTrThreads)), dim3(kTrThreads), 0, h->stream, npix, nQ, d_o0, from.map, d_cellfeat);
            HIPCHK(hipGetLastError());
            const Strided sc(nQ, kTrThreads, kTrBlocks);
            hipLaunchKernelGGL(advect_cells_kernel, dim3(sc.blocks), dim3(kTrThreads), 0, h->stream, nQ, sc.trips, d_cellfeat, d_tot);
            HIPCHK(hipGetLastError());
        }
        const Strided sp(npix, kTrThreads, kTrBlocks);
        hipLaunchKernelGGL(advect_gather_kernel, dim3(sp.blocks), dim3(kTrThreads), 0, h->stream, npix, sp.trips, nQ, d_o1, d_cellfeat, d_map, d_tot);
        HIPCHK(hipGetLastError());
        RCCHK(h->advect_timer.mark(h, 1));
        h->advect_timer.done();
        HIPCHK(download(h, cnt0, d_cnt0, 3));
        HIPCHK(download(h, cnt1, d_cnt1, 3));
        HIPCHK(download(h, tot, d_tot, 2));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (cnt0[0] || cnt1[0])
            return fail(h, SITRK_EINDEX, "%s: %llu cell(s) of the mesh have a vertex index outside [0, %lld)", fn, cnt0[0] > cnt1[0] ? cnt0[0] : cnt1[0],
                        (long long)h->nP);
        return SITRK_OK;
    };
    const int rc = run();
    if (rc) { keep_give(h, d_map, cap); return rc; }
    keep_commit(h, keep_to, d_map, cap, ny, nx, from.conn, from.min_pix);
    if (ncells) *ncells = (int64_t)tot[0];
    if (ncarried) *ncarried = (int64_t)tot[1];
    return SITRK_OK;
}

SITRK_API int sitrk_features_match(sitrk_t *h, int keepA, int keepB, int dj, int di, int reach, int64_t maxpair, int64_t *pairs, int64_t *npair,
                                   int64_t *nhit)
{
    const char *fn = "sitrk_features_match";
    NEED(h, "null handle");
    RCCHK(keep_check_slot(h, fn, "keepA", keepA, false));
    RCCHK(keep_check_slot(h, fn, "keepB", keepB, false));
    if (reach < 0 || reach > SITRK_MATCH_MAXREACH) return fail(h, SITRK_EINVAL, "%s: reach must be in 0..%d (got %d)", fn, SITRK_MATCH_MAXREACH, reach);
    if (dj < -kTrMaxShift || dj > kTrMaxShift || di < -kTrMaxShift || di > kTrMaxShift)
        return fail(h, SITRK_EINVAL, "%s: the shift must be within +-%d pixels (got %d, %d)", fn, kTrMaxShift, dj, di);
    if (maxpair < 0) return fail(h, SITRK_EINVAL, "%s: maxpair must be >= 0 (got %lld)", fn, (long long)maxpair);
    if (maxpair > 0 && !pairs) return fail(h, SITRK_EINVAL, "%s: null pairs with maxpair = %lld", fn, (long long)maxpair);
    RCCHK(keep_check_slot(h, fn, "keepA", keepA, true));
    RCCHK(keep_check_slot(h, fn, "keepB", keepB, true));
    const KeptMap &A = h->keep[keepA], &B = h->keep[keepB];
    if (A.ny != B.ny || A.nx != B.nx)
        return fail(h, SITRK_EINVAL, "%s: kept map %d is %d x %d, kept map %d is %d x %d", fn, keepA, A.ny, A.nx, keepB, B.ny, B.nx);
    if (npair) *npair = 0;
    if (nhit) *nhit = 0;
    HIPCHK(hipSetDevice(h->device));
    const int ny = A.ny, nx = A.nx;
    const int64_t npix = (int64_t)ny * nx;
    int nb = 1;                                                        // bits of a label: every value is below npix <= 2^28
    while (((int64_t)1 << nb) < npix) nb++;

    // E, the number of keys, first: nothing is sized from it before it is known to fit
    unsigned long long *d_tot;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_tot, kTrN); }));
    RCCHK(h->match_timer.begin(h));
    HIPCHK(hipMemsetAsync(d_tot, 0, kTrN * sizeof(unsigned long long), h->stream));
    RCCHK(launch_scan<false>(h, reach, ny, nx, dj, di, nb, A.map, B.map, nullptr, nullptr, nullptr, d_tot));
    unsigned long long tot[kTrN] = {0, 0, 0, 0};
    HIPCHK(download(h, tot, d_tot, kTrN));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (tot[kTrE] > (unsigned long long)kTrMaxKeys)
        return fail(h, SITRK_EINVAL, "%s: %llu (pixel, feature) pairs to sort, more than 2^31 - 1: match a smaller raster or with a smaller reach", fn,
                    tot[kTrE]);
    const int64_t E = (int64_t)tot[kTrE];
    const int64_t rows_cap = maxpair < E ? maxpair : E;

    int32_t *d_cnt, *d_off; unsigned long long *d_keys, *d_sorted; long long *d_pairs; char *d_scan, *d_sort;
    size_t scan_bytes = 0, scan2 = 0, sort_bytes = 0;
    RCCHK(scan_i32_bytes(h, npix, &scan_bytes));
    if (E > 0) {
        RCCHK(scan_i32_bytes(h, E, &scan2));
        HIPCHK(sort_keys_u64(nullptr, &sort_bytes, nullptr, nullptr, (size_t)E, (unsigned)(2 * nb), h->stream));
    }
    if (scan2 > scan_bytes) scan_bytes = scan2;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_tot, kTrN); c.take(d_cnt, npix); c.take(d_off, npix); c.take(d_keys, E); c.take(d_sorted, E); c.take(d_pairs, (size_t)rows_cap * 3);
        c.take(d_scan, scan_bytes); c.take(d_sort, sort_bytes);
    }));
    // (the scratch may have moved: the counters are set again)
    HIPCHK(hipMemsetAsync(d_tot, 0, kTrN * sizeof(unsigned long long), h->stream));
    RCCHK(h->match_timer.mark(h, 0));
    if (E > 0) {
        RCCHK(launch_scan<false>(h, reach, ny, nx, dj, di, nb, A.map, B.map, d_cnt, nullptr, nullptr, d_tot));
        size_t tb = scan_bytes;
        HIPCHK(rocprim::exclusive_scan(d_scan, tb, d_cnt, d_off, 0, (size_t)npix, rocprim::plus<int32_t>(), h->stream));
        RCCHK(launch_scan<true>(h, reach, ny, nx, dj, di, nb, A.map, B.map, nullptr, d_off, d_keys, d_tot));
    }
    RCCHK(h->match_timer.mark(h, 1));
    if (E > 0) {
        size_t sb = sort_bytes;
        HIPCHK(sort_keys_u64(d_sort, &sb, (const uint64_t *)d_keys, (uint64_t *)d_sorted, (size_t)E, (unsigned)(2 * nb), h->stream));
    }
    RCCHK(h->match_timer.mark(h, 2));
    if (E > 0) {
        int32_t *d_flag = (int32_t *)d_keys, *d_row = d_flag + E;      // over the unsorted keys, which are dead
        hipLaunchKernelGGL(match_bounds_kernel, dim3(nblk(E, kTrThreads)), dim3(kTrThreads), 0, h->stream, E, d_sorted, d_flag);
        HIPCHK(hipGetLastError());
        size_t tb = scan_bytes;
        HIPCHK(rocprim::exclusive_scan(d_scan, tb, d_flag, d_row, 0, (size_t)E, rocprim::plus<int32_t>(), h->stream));
        if (rows_cap > 0) HIPCHK(hipMemsetAsync(d_pairs, 0, (size_t)rows_cap * 3 * sizeof(long long), h->stream));
        hipLaunchKernelGGL(match_rows_kernel, dim3(nblk(E, kTrThreads)), dim3(kTrThreads), 0, h->stream, E, rows_cap, nb, d_sorted, d_flag, d_row, d_pairs,
                           d_tot);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->match_timer.mark(h, 3));
    h->match_timer.done();
    unsigned long long end[kTrN] = {0, 0, 0, 0};
    HIPCHK(download(h, end, d_tot, kTrN));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t np = (int64_t)end[kTrPair];
    const int64_t rows = np < maxpair ? np : maxpair;
    if (rows > 0) {
        HIPCHK(download(h, pairs, d_pairs, (size_t)rows * 3));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (npair) *npair = np;
    if (nhit) *nhit = (int64_t)tot[kTrHit];
    return SITRK_OK;
}

SITRK_API int sitrk_match_kernel_ms(sitrk_t *h, float *emit_ms, float *sort_ms, float *rows_ms)
{
    NEED(h, "null handle");
    NEED(h->match_timer.complete, "sitrk_match_kernel_ms: no sitrk_features_match has run its kernels yet");
    float *out[3] = {emit_ms, sort_ms, rows_ms};
    for (int k = 0; k < 3; k++) RCCHK(h->match_timer.elapsed(h, k, out[k]));
    return SITRK_OK;
}

SITRK_API int sitrk_advect_kernel_ms(sitrk_t *h, float *advect_ms)
{
    NEED(h, "null handle");
    NEED(h->advect_timer.complete, "sitrk_advect_kernel_ms: no sitrk_mesh_features_advect has run its kernels yet");
    return h->advect_timer.elapsed(h, 0, advect_ms);
}
