// sitrk_deform.hip -- deformation rates of buoy triangles and quadrangles (sitrk_deform_cells, sitrk_deform_mark,
// sitrk_deform_since_mark): an EXTRA the reference does not have.  Kept in its own translation unit so that the device code of
// sitrk.hip stays as it is.  The contract (operation order, validity, fill) is in include/sitrk.h.
//
// Two kernels, both memory bound, no LDS and no cross-lane work:
//   deform_points_kernel   one buoy per lane over the CELL-SORTED state: coalesced reads of pos, cell, perm (and win), one
//                          16-byte point written per buoy in the caller's order.  A buoy that is no valid vertex gets NaN in y, so
//                          the cell kernel needs no second gather for validity.  With check = false it is the plain snapshot of
//                          sitrk_deform_mark.
//   deform_cells_kernel<NV>  one cell per lane: its NV indices, then all 2 NV 16-byte gathers before any arithmetic, the contract (deform_rates of
//                          sitrk_cellmath.h, which the cell kernel of sitrk_mesh.hip calls too),
//                          5 fp64 stores and 1 byte store.  A vertex index outside [0, nP) is counted through a vector atomic and
//                          never dereferenced; the drivers turn a non-zero count into SITRK_EINDEX.
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_cellmath.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kDefThreads = 256;

__global__ __launch_bounds__(kDefThreads) void deform_points_kernel(int64_t n, BuoyState st, bool windowed, bool check, int jrec0, int jrec1,
                                                                    pt *__restrict__ out)
{
    const int64_t s = (int64_t)blockIdx.x * kDefThreads + threadIdx.x;
    if (s >= n) return;
    const int32_t o = st.perm[s];
    pt p = st.pos[s];
    if (check) {
        bool ok = st.cell[s] >= 0;                                   // alive now
        if (windowed) { const int2 w = st.win[s]; ok = ok && w.x <= jrec0 && w.y >= jrec1; }     // stepped at every record of the span
        if (!ok) p.y = quiet_nan();
    }
    out[o] = p;
}

// host arrays of sitrk_deform_cells: a buoy with mask 0 is no valid vertex
__global__ __launch_bounds__(kDefThreads) void deform_mask_kernel(int64_t n, const int8_t *__restrict__ mask, pt *__restrict__ p)
{
    const int64_t k = (int64_t)blockIdx.x * kDefThreads + threadIdx.x;
    if (k >= n) return;
    if (mask[k] == 0) p[k].y = quiet_nan();
}

template <int NV>
__global__ __launch_bounds__(kDefThreads) void deform_cells_kernel(int64_t nC, int64_t nP, const int32_t *__restrict__ cells,
                                                                   const pt *__restrict__ p0, const pt *__restrict__ p1, double T,
                                                                   double *__restrict__ out, int8_t *__restrict__ valid,
                                                                   unsigned long long *__restrict__ bad_index)
{
    const int64_t c = (int64_t)blockIdx.x * kDefThreads + threadIdx.x;
    if (c >= nC) return;
    int32_t idx[NV];
    bool in_range = true;
#pragma unroll
    for (int k = 0; k < NV; k++) {
        idx[k] = cells[c * NV + k];
        in_range = in_range && (uint64_t)(int64_t)idx[k] < (uint64_t)nP;
    }
    if (!in_range) {
        atomicAdd(bad_index, 1ull);
#pragma unroll
        for (int k = 0; k < NV; k++) idx[k] = 0;                      // buoy 0 stands in: the offending index is never dereferenced
    }
    pt a[NV], b[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) a[k] = p0[idx[k]];
#pragma unroll
    for (int k = 0; k < NV; k++) b[k] = p1[idx[k]];

    double r[5];
    const bool ok = deform_rates<NV>(a, b, T, r) && in_range;          // the contract: sitrk_cellmath.h
    const double fill = SITRK_FILL;
#pragma unroll
    for (int k = 0; k < 5; k++) out[k * nC + c] = ok ? r[k] : fill;
    valid[c] = ok ? 1 : 0;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kDefThreads - 1) / kDefThreads); }

}  // namespace

void deform_release(sitrk_ctx *h, bool destroy)
{
    if (h->deform_t0) (void)hipFree(h->deform_t0);
    h->deform_t0 = nullptr;
    h->deform_marked = false;
    if (destroy) h->deform_timer.release();
}

int deform_points_now(sitrk_ctx *h, pt *out)
{
    hipLaunchKernelGGL(deform_points_kernel, dim3(nblk(h->nP)), dim3(kDefThreads), 0, h->stream, h->nP, h->st[h->cur], false, true, 0, 0, out);
    HIPCHK(hipGetLastError());
    return SITRK_OK;
}

int deform_points_span(sitrk_ctx *h, int jrec0, int jrec1, pt *out)
{
    hipLaunchKernelGGL(deform_points_kernel, dim3(nblk(h->nP)), dim3(kDefThreads), 0, h->stream, h->nP, h->st[h->cur], h->windowed, true,
                       jrec0, jrec1, out);
    HIPCHK(hipGetLastError());
    return SITRK_OK;
}

}  // namespace sitrk

using namespace sitrk;

// what both compute entry points check first; nC == 0 is valid
static int deform_check(sitrk_ctx *h, const char *fn, int64_t nC, int nv, const int32_t *cells, const double *out, const int8_t *valid)
{
    if (nv != 3 && nv != 4) return fail(h, SITRK_EINVAL, "%s: nv must be 3 (triangles) or 4 (quadrangles), got %d", fn, nv);
    if (!(nC >= 0 && nC < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nC must be in 0..2^31-2", fn);
    if (nC > 0 && !(cells && out && valid)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    return SITRK_OK;
}

// the cell list goes up and the bad-index count is zeroed in front of the kernels; event 0 of the timer marks where the kernels start
static int deform_begin(sitrk_ctx *h, int32_t *d_cells, const int32_t *cells, size_t count)
{
    RCCHK(h->deform_timer.create(h));
    HIPCHK(upload(h, d_cells, cells, count));
    HIPCHK(hipMemsetAsync(h->counter, 0, sizeof(unsigned long long), h->stream));
    RCCHK(h->deform_timer.mark(h, 0));
    return SITRK_OK;
}

// The shared tail: the cell kernel over device points d_p0 / d_p1 (nP each, NaN in y = no valid vertex), results to the host.
// Behind deform_begin() and the caller's pass over the points.
static int deform_run(sitrk_ctx *h, const char *fn, int64_t nP, const pt *d_p0, const pt *d_p1, int64_t nC, int nv, const int32_t *d_cells,
                      double T, double *d_out, int8_t *d_valid, double *out, int8_t *valid, int64_t *nvalid)
{
    RCCHK(h->deform_timer.mark(h, 1));
    if (nv == 3)
        hipLaunchKernelGGL((deform_cells_kernel<3>), dim3(nblk(nC)), dim3(kDefThreads), 0, h->stream, nC, nP, d_cells, d_p0, d_p1, T, d_out,
                           d_valid, h->counter);
    else
        hipLaunchKernelGGL((deform_cells_kernel<4>), dim3(nblk(nC)), dim3(kDefThreads), 0, h->stream, nC, nP, d_cells, d_p0, d_p1, T, d_out,
                           d_valid, h->counter);
    HIPCHK(hipGetLastError());
    RCCHK(h->deform_timer.mark(h, 2));
    h->deform_timer.done();
    unsigned long long bad = 0;
    HIPCHK(download(h, &bad, h->counter, 1));
    HIPCHK(download(h, out, d_out, (size_t)5 * nC));
    HIPCHK(download(h, valid, d_valid, (size_t)nC));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (bad)
        return fail(h, SITRK_EINDEX, "%s: %llu cell(s) have a vertex index outside [0, %lld)", fn, bad, (long long)nP);
    if (nvalid) {
        int64_t nv_ok = 0;
        for (int64_t c = 0; c < nC; c++) nv_ok += valid[c];
        *nvalid = nv_ok;
    }
    return SITRK_OK;
}

SITRK_API int sitrk_deform_cells(sitrk_t *h, int64_t nP, const double *yx0, const double *yx1, const int8_t *mask0, const int8_t *mask1,
                                 int64_t nC, int nv, const int32_t *cells, double T, double *out, int8_t *valid, int64_t *nvalid)
{
    const char *fn = "sitrk_deform_cells";
    NEED(h, "null handle");
    RCCHK(deform_check(h, fn, nC, nv, cells, out, valid));
    if (!(nP >= 0 && nP < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nP must be in 0..2^31-2", fn);
    if (nP > 0 && !(yx0 && yx1)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    if (!std::isfinite(T) || !(T > 0.0)) return fail(h, SITRK_EINVAL, "%s: T must be finite and > 0 seconds (got %g)", fn, T);
    if (nvalid) *nvalid = 0;
    if (nC == 0) return SITRK_OK;
    if (nP == 0) return fail(h, SITRK_EINDEX, "%s: %lld cell(s) have a vertex index outside [0, 0)", fn, (long long)nC);
    HIPCHK(hipSetDevice(h->device));
    pt *d_p0, *d_p1; int8_t *d_m0, *d_m1, *d_valid; int32_t *d_cells; double *d_out;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_p0, nP); c.take(d_p1, nP); c.take(d_m0, nP); c.take(d_m1, nP);
        c.take(d_cells, (size_t)nC * nv); c.take(d_out, (size_t)5 * nC); c.take(d_valid, nC);
    }));
    HIPCHK(upload(h, d_p0, yx0, nP));
    HIPCHK(upload(h, d_p1, yx1, nP));
    if (mask0) HIPCHK(upload(h, d_m0, mask0, nP));
    if (mask1) HIPCHK(upload(h, d_m1, mask1, nP));
    RCCHK(deform_begin(h, d_cells, cells, (size_t)nC * nv));
    if (mask0) hipLaunchKernelGGL(deform_mask_kernel, dim3(nblk(nP)), dim3(kDefThreads), 0, h->stream, nP, d_m0, d_p0);
    if (mask1) hipLaunchKernelGGL(deform_mask_kernel, dim3(nblk(nP)), dim3(kDefThreads), 0, h->stream, nP, d_m1, d_p1);
    HIPCHK(hipGetLastError());
    return deform_run(h, fn, nP, d_p0, d_p1, nC, nv, d_cells, T, d_out, d_valid, out, valid, nvalid);
}

SITRK_API int sitrk_deform_mark(sitrk_t *h, int jrec0)
{
    const char *fn = "sitrk_deform_mark";
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    HIPCHK(hipSetDevice(h->device));
    if (!h->deform_t0) HIPCHK(hipMalloc((void **)&h->deform_t0, (size_t)h->nP * sizeof(pt)));
    hipLaunchKernelGGL(deform_points_kernel, dim3(nblk(h->nP)), dim3(kDefThreads), 0, h->stream, h->nP, h->st[h->cur], h->windowed, false,
                       jrec0, jrec0, h->deform_t0);
    HIPCHK(hipGetLastError());
    h->deform_marked = true;
    h->deform_jrec0 = jrec0;
    return SITRK_OK;
}

SITRK_API int sitrk_deform_since_mark(sitrk_t *h, int jrec1, int64_t nC, int nv, const int32_t *cells, double *out, int8_t *valid,
                                      int64_t *nvalid)
{
    const char *fn = "sitrk_deform_since_mark";
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    if (!h->deform_marked) return fail(h, SITRK_EINVAL, "%s: no mark (call sitrk_deform_mark first; sitrk_set_buoys cancels it)", fn);
    if (jrec1 < h->deform_jrec0) return fail(h, SITRK_EINVAL, "%s: jrec1 = %d lies before the mark at record %d", fn, jrec1, h->deform_jrec0);
    RCCHK(deform_check(h, fn, nC, nv, cells, out, valid));
    if (nvalid) *nvalid = 0;
    if (nC == 0) return SITRK_OK;
    const double T = (double)((int64_t)jrec1 - h->deform_jrec0 + 1) * h->rdt;        // one rounded product
    HIPCHK(hipSetDevice(h->device));
    const int64_t nP = h->nP;
    pt *d_p1; int8_t *d_valid; int32_t *d_cells; double *d_out;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_p1, nP); c.take(d_cells, (size_t)nC * nv); c.take(d_out, (size_t)5 * nC); c.take(d_valid, nC);
    }));
    RCCHK(deform_begin(h, d_cells, cells, (size_t)nC * nv));
    hipLaunchKernelGGL(deform_points_kernel, dim3(nblk(nP)), dim3(kDefThreads), 0, h->stream, nP, h->st[h->cur], h->windowed, true,
                       h->deform_jrec0, jrec1, d_p1);
    HIPCHK(hipGetLastError());
    return deform_run(h, fn, nP, h->deform_t0, d_p1, nC, nv, d_cells, T, d_out, d_valid, out, valid, nvalid);
}

SITRK_API int sitrk_deform_kernel_ms(sitrk_t *h, float *points_ms, float *cells_ms)
{
    NEED(h, "null handle");
    NEED(h->deform_timer.complete, "sitrk_deform_kernel_ms: no deformation call has run its kernels yet");
    RCCHK(h->deform_timer.elapsed(h, 0, points_ms));
    RCCHK(h->deform_timer.elapsed(h, 1, cells_ms));
    return SITRK_OK;
}
