// sitrk_coarse.hip -- coarse-grained deformation of buoy cells (sitrk_coarse_cells, sitrk_mesh_coarse): an EXTRA the reference
// does not have.  The cells' velocity gradients, weighted by their t0 area, are summed into the pixels of a regular grid and up a
// pyramid of 2x2 boxes, and a table of eight sums per level comes down: the spatial scaling curve <tot^q>(L) of one mesh from one
// call, its per-cell results never leaving the device.  The contract is in include/sitrk.h and DESIGN.md 3.16: the level sums
// use only + - * / in a fixed order, so every bit of them is pinned; the one unpinned operation is the sqrt of the table.
//
// Kernels, wave64, 256 lanes per workgroup, no scratch memory, LDS only for the reductions (256 B, 32 B):
//   coarse_mask_kernel    one point per lane: NaN in y where the mask byte is 0 (host arrays only)
//   coarse_terms_kernel<NV,SRC>  one cell per lane: its vertices at t0 and t1 (SRC = 0: 2 NV gathers through its indices; SRC = 1:
//                         the mesh's contiguous 64-byte t0 block and four t1 gathers), the use / status byte, the gradients of
//                         sitrk_cellmath.h, the t0 centroid and its pixel.  Writes key = pixel index, or the number of pixels for a
//                         cell that does not contribute or lies outside the grid, value = cell index, the five terms, and per
//                         workgroup the number of contributing cells inside and outside the grid (ballots, no atomic)
//   (sort_pairs_u32)      the stable radix sort of sitrk_sort.hip on (key, cell index): a pixel's cells become one run, in
//                         ascending cell index
//   coarse_bounds_kernel  one sorted position per lane: where the key differs from its neighbour's, the run's start / end
//   coarse_level0_kernel  one pixel per lane: the run summed sequentially in that order, the six values stored, the pixel's eight
//                         table terms reduced over the workgroup into one row of partials
//   coarse_up_kernel      one box of level l+1 per lane: (c00 + c01) + (c10 + c11) of six values, the same table terms and row
//   coarse_table_kernel   one workgroup per level: lane i sums the rows i, i+256, ... in order, then the same reduction; and
//   coarse_count_kernel   one workgroup: the integer counts of the terms kernel
// Every loop is bounded by a count read before it starts, no lane waits for another, vector stores only, no floating-point
// atomics: the order of every sum is fixed by the contract or by the launch geometry alone.
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_bins.h"
#include "sitrk_cellmath.h"
#include "sitrk_internal.h"
#include "sitrk_reduce.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kCoThreads = 256;
constexpr int kCoCols = SITRK_COARSE_NCOLS;
constexpr int64_t kCoMaxPixels = (int64_t)1 << 24;

struct CoarseGrid {
    double y0, x0, d;
    int ny, nx;
};

__global__ __launch_bounds__(kCoThreads) void coarse_mask_kernel(int64_t n, const int8_t *__restrict__ mask, pt *__restrict__ p)
{
    const int64_t k = (int64_t)blockIdx.x * kCoThreads + threadIdx.x;
    if (k >= n) return;
    if (mask[k] == 0) p[k].y = quiet_nan();
}

template <int NV, int SRC>
__global__ __launch_bounds__(kCoThreads) void coarse_terms_kernel(int64_t nC, int64_t nP, const int32_t *__restrict__ cells,
                                                                  const pt *__restrict__ p0, const pt *__restrict__ p1,
                                                                  const int8_t *__restrict__ flag, bool only_status1, double T, CoarseGrid g,
                                                                  uint32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                                  double *__restrict__ terms, uint2 *__restrict__ counts,
                                                                  unsigned long long *__restrict__ bad_index)
{
    __shared__ unsigned sm[kCoThreads / 64][2];
    const int64_t c0 = (int64_t)blockIdx.x * kCoThreads + threadIdx.x;
    const bool live = c0 < nC;                                         // a lane behind the last cell reads the last cell and writes nothing
    const int64_t c = live ? c0 : nC - 1;
    bool use = live;
    int32_t idx[NV];
    if (NV == 4) {
        const int4 q = ((const int4 *)cells)[c];
        idx[0] = q.x; idx[1] = q.y; idx[2] = q.z; idx[NV - 1] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < NV; k++) idx[k] = cells[c * NV + k];
    }
    pt a[NV], b[NV];
    if (SRC == 0) {
        bool in_range = true;
#pragma unroll
        for (int k = 0; k < NV; k++) in_range = in_range && (uint64_t)(int64_t)idx[k] < (uint64_t)nP;
        if (!in_range) {
            if (live) atomicAdd(bad_index, 1ull);
            use = false;
#pragma unroll
            for (int k = 0; k < NV; k++) idx[k] = 0;                  // point 0 stands in: the offending index is never dereferenced
        }
#pragma unroll
        for (int k = 0; k < NV; k++) a[k] = p0[idx[k]];
    } else {
#pragma unroll
        for (int k = 0; k < NV; k++) a[k] = p0[NV * c + k];
    }
#pragma unroll
    for (int k = 0; k < NV; k++) b[k] = p1[idx[k]];
    if (flag != nullptr) {                                             // wave-uniform
        const int8_t f = flag[c];
        use = use && (only_status1 ? f == 1 : f != 0);
    }

    double t[5];
    use = deform_gradient_terms<NV>(a, b, T, t) && use;                // the contract: sitrk_cellmath.h

    // the t0 centroid and its pixel
    double cy, cx;
    if (NV == 4) {
        cy = 0.25 * ((a[0].y + a[1].y) + (a[2].y + a[NV - 1].y));
        cx = 0.25 * ((a[0].x + a[1].x) + (a[2].x + a[NV - 1].x));
    } else {
        cy = ((a[0].y + a[1].y) + a[2].y) / 3.0;
        cx = ((a[0].x + a[1].x) + a[2].x) / 3.0;
    }
    const double fy = (cy - g.y0) / g.d, fx = (cx - g.x0) / g.d;
    const bool in = fy >= 0.0 && fy < (double)g.ny && fx >= 0.0 && fx < (double)g.nx;     // a NaN is outside
    const uint32_t npix = (uint32_t)g.ny * (uint32_t)g.nx;
    uint32_t key = npix;
    if (use && in) key = (uint32_t)(int)floor(fy) * (uint32_t)g.nx + (uint32_t)(int)floor(fx);
    if (live) {
        keys[c] = key;
        vals[c] = (int32_t)c;
#pragma unroll
        for (int k = 0; k < 5; k++) terms[k * nC + c] = t[k];
    }

    const unsigned n_in = __popcll(__ballot(use && in)), n_out = __popcll(__ballot(use && !in));
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = n_in; sm[threadIdx.x >> 6][1] = n_out; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 s = make_uint2(sm[0][0], sm[0][1]);
#pragma unroll
        for (int w = 1; w < kCoThreads / 64; w++) { s.x += sm[w][0]; s.y += sm[w][1]; }
        counts[blockIdx.x] = s;
    }
}

// start / end (npix each, zeroed before) of every pixel's run in the sorted keys
__global__ __launch_bounds__(kCoThreads) void coarse_bounds_kernel(int64_t n, uint32_t npix, const uint32_t *__restrict__ keys,
                                                                   int32_t *__restrict__ start, int32_t *__restrict__ end)
{
    const int64_t s = (int64_t)blockIdx.x * kCoThreads + threadIdx.x;
    if (s >= n) return;
    const uint32_t k = keys[s];
    if (k >= npix) return;
    if (s == 0 || keys[s - 1] != k) start[k] = (int32_t)s;
    if (s == n - 1 || keys[s + 1] != k) end[k] = (int32_t)(s + 1);
}

// the eight table terms of one box v = n, A, AUx, AUy, AVx, AVy; amin = fmin*(L*L) of its level; all zero for a lane without a box
__device__ __forceinline__ void table_terms(bool live, const double (&v)[6], double amin, double (&t)[kCoCols])
{
    const bool some = live && v[0] >= 1.0;
    const bool filled = some && v[1] > 0.0 && v[1] >= amin;
    const double A = v[1];
    const double UX = v[2] / A, UY = v[3] / A, VX = v[4] / A, VY = v[5] / A;
    const double div = UX + VY, e1 = UX - VY, e2 = UY + VX;
    const double shr = sqrt(e1 * e1 + e2 * e2);
    const double tot = sqrt(div * div + shr * shr);
    const double m1 = A * tot, m2 = m1 * tot, m3 = m2 * tot;
    t[0] = some ? 1.0 : 0.0;
    t[1] = filled ? 1.0 : 0.0;
    t[2] = filled ? A : 0.0;
    t[3] = filled ? A * div : 0.0;
    t[4] = filled ? A * shr : 0.0;
    t[5] = filled ? m1 : 0.0;
    t[6] = filled ? m2 : 0.0;
    t[7] = filled ? m3 : 0.0;
}

__global__ __launch_bounds__(kCoThreads) void coarse_level0_kernel(int64_t npix, int64_t nC, const int32_t *__restrict__ start,
                                                                   const int32_t *__restrict__ end, const int32_t *__restrict__ vals,
                                                                   const double *__restrict__ terms, double amin, double *__restrict__ lev,
                                                                   double *__restrict__ partials)
{
    __shared__ double sm[kCoThreads / 64][kCoCols];
    const int64_t p = (int64_t)blockIdx.x * kCoThreads + threadIdx.x;
    const bool live = p < npix;
    int32_t s0 = 0, cnt = 0;
    if (live) { s0 = start[p]; cnt = end[p] - s0; }
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = 0.0;
    for (int32_t i = 0; i < cnt; i++) {                                // ascending cell index: the sort is stable
        const int64_t c = vals[s0 + i];
#pragma unroll
        for (int k = 0; k < 5; k++) v[1 + k] = v[1 + k] + terms[k * nC + c];
    }
    v[0] = (double)cnt;
    if (live) {
#pragma unroll
        for (int k = 0; k < 6; k++) lev[k * npix + p] = v[k];
    }
    double t[kCoCols];
    table_terms(live, v, amin, t);
    const double s = block_sum<kCoCols, kCoThreads>(t, sm);
    if (threadIdx.x < kCoCols) partials[(int64_t)blockIdx.x * kCoCols + threadIdx.x] = s;
}

__global__ __launch_bounds__(kCoThreads) void coarse_up_kernel(int nyc, int nxc, const double *__restrict__ child, int nyp, int nxp,
                                                               double amin, double *__restrict__ lev, double *__restrict__ partials)
{
    __shared__ double sm[kCoThreads / 64][kCoCols];
    const int64_t nbox = (int64_t)nyp * nxp, nch = (int64_t)nyc * nxc;
    const int64_t p = (int64_t)blockIdx.x * kCoThreads + threadIdx.x;
    const bool live = p < nbox;
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = 0.0;
    if (live) {
        const int J = (int)(p / nxp), I = (int)(p - (int64_t)J * nxp);
        const int j0 = 2 * J, i0 = 2 * I;                              // (j0, i0) is always a box of the level below
        const bool right = i0 + 1 < nxc, down = j0 + 1 < nyc;
        const int64_t q00 = (int64_t)j0 * nxc + i0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const double *f = child + k * nch;
            const double c00 = f[q00];
            const double c01 = right ? f[q00 + 1] : 0.0;
            const double c10 = down ? f[q00 + nxc] : 0.0;
            const double c11 = right && down ? f[q00 + nxc + 1] : 0.0;
            v[k] = (c00 + c01) + (c10 + c11);
            lev[k * nbox + p] = v[k];
        }
    }
    double t[kCoCols];
    table_terms(live, v, amin, t);
    const double s = block_sum<kCoCols, kCoThreads>(t, sm);
    if (threadIdx.x < kCoCols) partials[(int64_t)blockIdx.x * kCoCols + threadIdx.x] = s;
}

// rows (nlev, 2) int64: first row and number of rows of every level's partials
__global__ __launch_bounds__(kCoThreads) void coarse_table_kernel(const int64_t *__restrict__ rows, const double *__restrict__ partials,
                                                                  double *__restrict__ table)
{
    __shared__ double sm[kCoThreads / 64][kCoCols];
    const int64_t first = rows[2 * blockIdx.x], nrows = rows[2 * blockIdx.x + 1];
    double t[kCoCols];
#pragma unroll
    for (int k = 0; k < kCoCols; k++) t[k] = 0.0;
    for (int64_t row = threadIdx.x; row < nrows; row += kCoThreads) {
#pragma unroll
        for (int k = 0; k < kCoCols; k++) t[k] = t[k] + partials[(first + row) * kCoCols + k];
    }
    const double s = block_sum<kCoCols, kCoThreads>(t, sm);
    if (threadIdx.x < kCoCols) table[(int64_t)blockIdx.x * kCoCols + threadIdx.x] = s;
}

__global__ __launch_bounds__(kCoThreads) void coarse_count_kernel(int64_t nrows, const uint2 *__restrict__ counts,
                                                                  unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long sm[kCoThreads / 64][2];
    unsigned long long a = 0, b = 0;
    for (int64_t row = threadIdx.x; row < nrows; row += kCoThreads) {
        const uint2 c = counts[row];
        a += c.x; b += c.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kCoThreads / 64; w++) { a += sm[w][0]; b += sm[w][1]; }
        total[0] = a; total[1] = b;
    }
}

inline int64_t nblk(int64_t n) { return (n + kCoThreads - 1) / kCoThreads; }

// the levels of a grid: boxes, their first value in the pyramid and the rows of their partials
struct CoarseLevels {
    int nlev = 0;
    int ny[SITRK_COARSE_MAXLEV], nx[SITRK_COARSE_MAXLEV];
    int64_t off[SITRK_COARSE_MAXLEV + 1];       // first box of level l among all boxes; [nlev] = all boxes
    int64_t row[SITRK_COARSE_MAXLEV + 1];       // first row of level l's partials; [nlev] = all rows
    double amin[SITRK_COARSE_MAXLEV];           // fmin*(L_l*L_l), L_l = d*2^l
};

CoarseLevels coarse_levels(int ny, int nx, double d, int nlev, double fmin)
{
    CoarseLevels L;
    L.nlev = nlev;
    L.off[0] = 0; L.row[0] = 0;
    for (int l = 0; l < nlev; l++) {
        L.ny[l] = (int)(((int64_t)ny + ((int64_t)1 << l) - 1) >> l);
        L.nx[l] = (int)(((int64_t)nx + ((int64_t)1 << l) - 1) >> l);
        const int64_t nbox = (int64_t)L.ny[l] * L.nx[l];
        L.off[l + 1] = L.off[l] + nbox;
        L.row[l + 1] = L.row[l] + nblk(nbox);
        const double side = std::ldexp(d, l);                          // an exact scaling
        const double side2 = side * side;
        L.amin[l] = fmin * side2;
    }
    return L;
}

// the scratch of one call behind whatever holds its cells
struct CoarseBuf {
    uint32_t *k0, *k1;
    int32_t *v0, *v1, *start, *end;
    double *terms, *pyr, *partials, *table;
    uint2 *counts;
    int64_t *rows;
    unsigned long long *total;                  // contributing cells inside, outside, cells with a bad index
    char *sort_tmp;
    size_t sort_bytes;
};

void coarse_carve(Carver &c, CoarseBuf &b, int64_t nC, const CoarseLevels &L)
{
    const int64_t npix = L.off[1];
    c.take(b.k0, nC); c.take(b.k1, nC); c.take(b.v0, nC); c.take(b.v1, nC); c.take(b.terms, (size_t)5 * nC);
    c.take(b.start, npix); c.take(b.end, npix);
    c.take(b.pyr, (size_t)6 * L.off[L.nlev]); c.take(b.partials, (size_t)kCoCols * L.row[L.nlev]);
    c.take(b.table, (size_t)kCoCols * L.nlev); c.take(b.counts, nblk(nC)); c.take(b.rows, 2 * SITRK_COARSE_MAXLEV); c.take(b.total, 3);
    c.take(b.sort_tmp, b.sort_bytes);
}

struct CoarseJob {
    int64_t nC = 0, nP = 0;
    int nv = 4;
    bool block = false;                 // p0 is (nC,nv) in cell order; cells index p1 only
    const int32_t *cells = nullptr;
    const pt *p0 = nullptr, *p1 = nullptr;
    const int8_t *flag = nullptr;
    bool only_status1 = false;
    double T = 1.0;
};

int coarse_check(sitrk_ctx *h, const char *fn, double y0, double x0, double d, int ny, int nx, int nlev, double fmin, const double *table)
{
    if (!std::isfinite(y0) || !std::isfinite(x0)) return fail(h, SITRK_EINVAL, "%s: y0_km and x0_km must be finite (got %g, %g)", fn, y0, x0);
    if (!std::isfinite(d) || !(d > 0.0)) return fail(h, SITRK_EINVAL, "%s: d_km must be finite and > 0 (got %g)", fn, d);
    if (ny < 1 || nx < 1) return fail(h, SITRK_EINVAL, "%s: ny and nx must be >= 1 (got %d, %d)", fn, ny, nx);
    if ((int64_t)ny * nx > kCoMaxPixels) return fail(h, SITRK_EINVAL, "%s: ny*nx = %lld exceeds 2^24 pixels", fn, (long long)ny * nx);
    if (nlev < 1 || nlev > SITRK_COARSE_MAXLEV) return fail(h, SITRK_EINVAL, "%s: nlev must be in 1..%d (got %d)", fn, SITRK_COARSE_MAXLEV, nlev);
    if (!std::isfinite(fmin) || !(fmin >= 0.0)) return fail(h, SITRK_EINVAL, "%s: fmin must be finite and >= 0 (got %g)", fn, fmin);
    if (!table) return fail(h, SITRK_EINVAL, "%s: null table", fn);
    return SITRK_OK;
}

int coarse_sort_bytes(sitrk_ctx *h, int64_t nC, size_t *bytes)
{
    *bytes = 0;
    if (nC > 0) HIPCHK(sort_pairs_u32(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, (size_t)nC, 32, h->stream));
    *bytes = align256(*bytes);
    return SITRK_OK;
}

template <int NV, int SRC>
void launch_terms(sitrk_ctx *h, const CoarseJob &j, const CoarseGrid &g, const CoarseBuf &b)
{
    hipLaunchKernelGGL((coarse_terms_kernel<NV, SRC>), dim3((unsigned)nblk(j.nC)), dim3(kCoThreads), 0, h->stream, j.nC, j.nP, j.cells, j.p0,
                       j.p1, j.flag, j.only_status1, j.T, g, b.k0, b.v0, b.terms, b.counts, b.total + 2);
}

// everything behind the cells on the device: queues the kernels, the downloads and synchronises
int coarse_run(sitrk_ctx *h, const char *fn, const CoarseJob &j, const CoarseGrid &g, const CoarseLevels &L, const CoarseBuf &b,
               double *boxes, double *table, int64_t *nin, int64_t *nout)
{
    const int64_t npix = L.off[1];
    RCCHK(h->coarse_timer.begin(h));
    int64_t rows[2 * SITRK_COARSE_MAXLEV] = {0};
    for (int l = 0; l < L.nlev; l++) { rows[2 * l] = L.row[l]; rows[2 * l + 1] = L.row[l + 1] - L.row[l]; }
    HIPCHK(upload(h, b.rows, rows, 2 * SITRK_COARSE_MAXLEV));
    HIPCHK(hipMemsetAsync(b.total, 0, 3 * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemsetAsync(b.start, 0, (size_t)npix * sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(b.end, 0, (size_t)npix * sizeof(int32_t), h->stream));
    RCCHK(h->coarse_timer.mark(h, 0));
    if (j.nC > 0) {
        if (j.block) launch_terms<4, 1>(h, j, g, b);
        else if (j.nv == 3) launch_terms<3, 0>(h, j, g, b);
        else launch_terms<4, 0>(h, j, g, b);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->coarse_timer.mark(h, 1));
    if (j.nC > 0) {
        size_t tb = b.sort_bytes;                                      // the keys run 0 .. npix, npix <= 2^24
        HIPCHK(sort_pairs_u32(b.sort_tmp, &tb, b.k0, b.k1, b.v0, b.v1, (size_t)j.nC, key_bits((uint64_t)npix), h->stream));
    }
    RCCHK(h->coarse_timer.mark(h, 2));
    if (j.nC > 0) {
        hipLaunchKernelGGL(coarse_bounds_kernel, dim3((unsigned)nblk(j.nC)), dim3(kCoThreads), 0, h->stream, j.nC, (uint32_t)npix, b.k1, b.start,
                           b.end);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(coarse_level0_kernel, dim3((unsigned)nblk(npix)), dim3(kCoThreads), 0, h->stream, npix, j.nC, b.start, b.end, b.v1, b.terms,
                       L.amin[0], b.pyr, b.partials);
    HIPCHK(hipGetLastError());
    RCCHK(h->coarse_timer.mark(h, 3));
    for (int l = 1; l < L.nlev; l++) {
        const int64_t nbox = (int64_t)L.ny[l] * L.nx[l];
        hipLaunchKernelGGL(coarse_up_kernel, dim3((unsigned)nblk(nbox)), dim3(kCoThreads), 0, h->stream, L.ny[l - 1], L.nx[l - 1],
                           b.pyr + 6 * L.off[l - 1], L.ny[l], L.nx[l], L.amin[l], b.pyr + 6 * L.off[l], b.partials + kCoCols * L.row[l]);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->coarse_timer.mark(h, 4));
    hipLaunchKernelGGL(coarse_table_kernel, dim3((unsigned)L.nlev), dim3(kCoThreads), 0, h->stream, b.rows, b.partials, b.table);
    HIPCHK(hipGetLastError());
    if (j.nC > 0) {
        hipLaunchKernelGGL(coarse_count_kernel, dim3(1), dim3(kCoThreads), 0, h->stream, nblk(j.nC), b.counts, b.total);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->coarse_timer.mark(h, 5));
    h->coarse_timer.done();
    unsigned long long total[3] = {0, 0, 0};
    HIPCHK(download(h, total, b.total, 3));
    HIPCHK(download(h, table, b.table, (size_t)kCoCols * L.nlev));
    if (boxes) HIPCHK(download(h, boxes, b.pyr, (size_t)6 * L.off[L.nlev]));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (total[2]) return fail(h, SITRK_EINDEX, "%s: %llu cell(s) have a vertex index outside [0, %lld)", fn, total[2], (long long)j.nP);
    if (nin) *nin = (int64_t)total[0];
    if (nout) *nout = (int64_t)total[1];
    return SITRK_OK;
}

}  // namespace

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_coarse_cells(sitrk_t *h, int64_t nP, const double *yx0, const double *yx1, const int8_t *mask0, const int8_t *mask1,
                                 int64_t nC, int nv, const int32_t *cells, const int8_t *use, double T, double y0_km, double x0_km,
                                 double d_km, int ny, int nx, int nlev, double fmin, double *boxes, double *table, int64_t *nin,
                                 int64_t *nout)
{
    const char *fn = "sitrk_coarse_cells";
    NEED(h, "null handle");
    if (nv != 3 && nv != 4) return fail(h, SITRK_EINVAL, "%s: nv must be 3 (triangles) or 4 (quadrangles), got %d", fn, nv);
    if (!(nC >= 0 && nC < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nC must be in 0..2^31-2", fn);
    if (!(nP >= 0 && nP < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nP must be in 0..2^31-2", fn);
    if (!std::isfinite(T) || !(T > 0.0)) return fail(h, SITRK_EINVAL, "%s: T must be finite and > 0 seconds (got %g)", fn, T);
    RCCHK(coarse_check(h, fn, y0_km, x0_km, d_km, ny, nx, nlev, fmin, table));
    if ((nC > 0 && !cells) || (nP > 0 && !(yx0 && yx1))) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    if (nin) *nin = 0;
    if (nout) *nout = 0;
    if (nC > 0 && nP == 0) return fail(h, SITRK_EINDEX, "%s: %lld cell(s) have a vertex index outside [0, 0)", fn, (long long)nC);
    HIPCHK(hipSetDevice(h->device));
    const CoarseLevels L = coarse_levels(ny, nx, d_km, nlev, fmin);
    CoarseBuf b;
    RCCHK(coarse_sort_bytes(h, nC, &b.sort_bytes));
    pt *d_p0, *d_p1; int8_t *d_m0, *d_m1, *d_use; int32_t *d_cells;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_p0, nP); c.take(d_p1, nP); c.take(d_m0, mask0 ? (size_t)nP : 0); c.take(d_m1, mask1 ? (size_t)nP : 0);
        c.take(d_cells, (size_t)nC * nv); c.take(d_use, use ? (size_t)nC : 0);
        coarse_carve(c, b, nC, L);
    }));
    if (nC > 0) {
        HIPCHK(upload(h, d_p0, yx0, nP));
        HIPCHK(upload(h, d_p1, yx1, nP));
        HIPCHK(upload(h, d_cells, cells, (size_t)nC * nv));
        if (use) HIPCHK(upload(h, d_use, use, nC));
        if (mask0) {
            HIPCHK(upload(h, d_m0, mask0, nP));
            hipLaunchKernelGGL(coarse_mask_kernel, dim3((unsigned)nblk(nP)), dim3(kCoThreads), 0, h->stream, nP, d_m0, d_p0);
        }
        if (mask1) {
            HIPCHK(upload(h, d_m1, mask1, nP));
            hipLaunchKernelGGL(coarse_mask_kernel, dim3((unsigned)nblk(nP)), dim3(kCoThreads), 0, h->stream, nP, d_m1, d_p1);
        }
        HIPCHK(hipGetLastError());
    }
    CoarseJob j;
    j.nC = nC; j.nP = nP; j.nv = nv; j.cells = d_cells; j.p0 = d_p0; j.p1 = d_p1; j.flag = use ? d_use : nullptr; j.T = T;
    const CoarseGrid g = {y0_km, x0_km, d_km, ny, nx};
    return coarse_run(h, fn, j, g, L, b, boxes, table, nin, nout);
}

SITRK_API int sitrk_mesh_coarse(sitrk_t *h, int mesh, int jrec1, double y0_km, double x0_km, double d_km, int ny, int nx, int nlev,
                                double fmin, double *boxes, double *table, int64_t *nin, int64_t *nout)
{
    const char *fn = "sitrk_mesh_coarse";
    NEED(h, "null handle");
    RCCHK(mesh_deform_check(h, fn, mesh, jrec1));
    RCCHK(coarse_check(h, fn, y0_km, x0_km, d_km, ny, nx, nlev, fmin, table));
    if (nin) *nin = 0;
    if (nout) *nout = 0;
    HIPCHK(hipSetDevice(h->device));
    const int64_t nQ = h->mesh[mesh].nQ;
    const CoarseLevels L = coarse_levels(ny, nx, d_km, nlev, fmin);
    CoarseBuf b;
    RCCHK(coarse_sort_bytes(h, nQ, &b.sort_bytes));
    MeshDeformDev m;
    RCCHK(carve_behind_mesh(h, mesh, jrec1, false, true, false, [&](Carver &c) { coarse_carve(c, b, nQ, L); }, &m));
    CoarseJob j;
    j.nC = m.nQ; j.nP = h->nP; j.nv = 4; j.block = true; j.cells = m.quads; j.p0 = m.t0; j.p1 = m.p1; j.flag = m.status; j.only_status1 = true;
    j.T = (double)((int64_t)jrec1 - h->mesh[mesh].jrec0 + 1) * h->rdt;                 // one rounded product, as sitrk_mesh_deform
    const CoarseGrid g = {y0_km, x0_km, d_km, ny, nx};
    return coarse_run(h, fn, j, g, L, b, boxes, table, nin, nout);
}

SITRK_API int sitrk_coarse_kernel_ms(sitrk_t *h, float *terms_ms, float *sort_ms, float *level0_ms, float *pyramid_ms, float *table_ms)
{
    NEED(h, "null handle");
    NEED(h->coarse_timer.complete, "sitrk_coarse_kernel_ms: no coarse-graining call has run its kernels yet");
    float *out[5] = {terms_ms, sort_ms, level0_ms, pyramid_ms, table_ms};
    for (int k = 0; k < 5; k++) RCCHK(h->coarse_timer.elapsed(h, k, out[k]));
    return SITRK_OK;
}
