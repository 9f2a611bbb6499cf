// sitrk_pairs.hip -- dispersion of buoy pairs (sitrk_pairs_points, sitrk_pairs_mark, sitrk_pairs_since_mark): an EXTRA the
// reference does not have.  For every unordered pair of valid points whose t0 separation falls in a class [edges[c], edges[c+1])
// the strain e = (r1 - r0)/r0 of the pair over the interval, and per class a row of seven sums: the moments of |e| by separation,
// with no mesh.  The contract is in include/sitrk.h and DESIGN.md 3.20: the class of a pair is decided by + - * and comparisons
// alone, so every count is pinned; the unpinned operations are the two square roots of a pair's terms.
//
// Kernels, wave64, no scratch memory:
//   pairs_box_kernel     one point per lane: its validity, the bounding box of the valid t0 points (integer atomics on an order-
//                        preserving key of the double, one per wave) and their number
//   pairs_key_kernel     one point per lane: key = its bin on the uniform grid the host fitted to that box, or the number of bins
//                        for a point that is not valid; value = its index
//   (sort_pairs_u32)     the stable radix sort of sitrk_sort.hip: the valid points in (bin, index) order
//   pairs_gather_kernel  one sorted position per lane: the point's t0 and t1 positions as one 32-byte record
//   bin_start_kernel     (sitrk_bins.h) one bin per lane: the first sorted position of the bin, a binary search of a length fixed by
//                        the host
//   pairs_rows_kernel    one workgroup: a row of bins with n points is cut into ceil(n / kPairsTile) HOME CHUNKS of consecutive
//                        sorted positions; the exclusive scan of those numbers over the rows
//   pairs_kernel         one workgroup of one wave per (home chunk, class): lane i keeps home point i in registers; the rows of
//                        bins at and above the chunk's, cut to the columns within the class's outer edge of the chunk's, are runs
//                        of consecutive records and stream through LDS a tile of kPairsTile at a time.  A lane takes the streamed
//                        points behind its own sorted position, so every unordered pair is met once, and adds the terms of those
//                        in the class to seven sums of its own in the order they stream by; block_sum, one row of partials
//   pairs_table_kernel   one workgroup per class: lane i sums the rows i, i + kPairsTile, ... in order, then the same reduction
// One pass per class keeps the sums lane-private without 16 x 7 accumulators a lane: a pass costs the candidates of its own disc
// and geometric classes add up to about twice the outermost disc.
// Every loop is bounded by a count read before it starts, no lane waits for another, vector stores only, no floating-point
// atomics: the order of every sum is fixed by the sorted order and the launch geometry alone.
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_bins.h"
#include "sitrk_internal.h"
#include "sitrk_reduce.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kPairsThreads = 256;                  // the kernels with one point or bin per lane
constexpr int kPairsTile = 64;                      // home points of a workgroup = records staged in LDS at once = lanes of the table kernel
constexpr int kPairsCols = SITRK_PAIRS_NCOLS;
constexpr int kPairsSums = kPairsCols + 1;          // ... and the candidate tests behind them, for sitrk_pairs_stats
constexpr int kPairsMaxSide = 8192;                 // bins along one axis at most
constexpr int64_t kPairsMaxBins = (int64_t)1 << 22;
constexpr double kPairsBinFrac = 4.0;               // bin side = edges[nc] / kPairsBinFrac, doubled until the grid fits
constexpr double kPairsSlack = 1.0 + 1e-9, kPairsSlackAbs = 1e-9;   // what the reach in bins is widened by against its own roundings

struct __attribute__((aligned(16))) P4 { double y0, x0, y1, x1; };

struct PairsGrid {
    double ymin, xmin, inv_h, side;                 // inv_h = 0: one bin
    int ny, nx;
    int row_steps;                                  // trips of the search for a chunk's row
};

struct PairsEdges {
    double e[SITRK_PAIRS_MAXCLASS + 1];
    double e2[SITRK_PAIRS_MAXCLASS + 1];            // e[c]*e[c], one rounded product
};

__device__ __forceinline__ bool pairs_valid(int64_t k, const pt *__restrict__ p0, const pt *__restrict__ p1, const int8_t *__restrict__ m0,
                                            const int8_t *__restrict__ m1, pt &a, pt &b)
{
    a = p0[k]; b = p1[k];
    bool ok = isfinite(a.y) && isfinite(a.x) && isfinite(b.y) && isfinite(b.x);
    if (m0 != nullptr) ok = ok && m0[k] != 0;                            // wave-uniform
    if (m1 != nullptr) ok = ok && m1[k] != 0;
    return ok;
}

// red: ymin, ymax, xmin, xmax as order keys (set to all ones / 0 before), the number of valid points
__global__ __launch_bounds__(kPairsThreads) void pairs_box_kernel(int64_t n, const pt *__restrict__ p0, const pt *__restrict__ p1,
                                                                  const int8_t *__restrict__ m0, const int8_t *__restrict__ m1,
                                                                  unsigned long long *__restrict__ red)
{
    const int64_t k0 = (int64_t)blockIdx.x * kPairsThreads + threadIdx.x;
    const bool live = k0 < n;
    pt a, b;
    const bool ok = pairs_valid(live ? k0 : n - 1, p0, p1, m0, m1, a, b) && live;
    unsigned long long ylo = ok ? order_key(a.y) : ~0ull, yhi = ok ? order_key(a.y) : 0ull;
    unsigned long long xlo = ok ? order_key(a.x) : ~0ull, xhi = ok ? order_key(a.x) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a0 = __shfl_xor(ylo, o), a1 = __shfl_xor(yhi, o), a2 = __shfl_xor(xlo, o), a3 = __shfl_xor(xhi, o);
        ylo = a0 < ylo ? a0 : ylo; yhi = a1 > yhi ? a1 : yhi;
        xlo = a2 < xlo ? a2 : xlo; xhi = a3 > xhi ? a3 : xhi;
    }
    const unsigned long long cnt = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicMin(red + 0, ylo); atomicMax(red + 1, yhi); atomicMin(red + 2, xlo); atomicMax(red + 3, xhi);
        atomicAdd(red + 4, cnt);
    }
}

__global__ __launch_bounds__(kPairsThreads) void pairs_key_kernel(int64_t n, const pt *__restrict__ p0, const pt *__restrict__ p1,
                                                                  const int8_t *__restrict__ m0, const int8_t *__restrict__ m1, PairsGrid g,
                                                                  uint32_t *__restrict__ keys, int32_t *__restrict__ vals)
{
    const int64_t k = (int64_t)blockIdx.x * kPairsThreads + threadIdx.x;
    if (k >= n) return;
    pt a, b;
    const bool ok = pairs_valid(k, p0, p1, m0, m1, a, b);
    uint32_t key = (uint32_t)g.ny * (uint32_t)g.nx;
    if (ok) {
        // deliberately not cell_coord of sitrk_bins.h: (int) truncates, and the clamp compares in floating point before it converts
        int by = 0, bx = 0;
        if (g.inv_h > 0.0) {
            const double fy = (a.y - g.ymin) * g.inv_h, fx = (a.x - g.xmin) * g.inv_h;      // >= 0 and below the grid's side + 1
            by = fy < (double)(g.ny - 1) ? (int)fy : g.ny - 1;
            bx = fx < (double)(g.nx - 1) ? (int)fx : g.nx - 1;
        }
        key = (uint32_t)by * (uint32_t)g.nx + (uint32_t)bx;
    }
    keys[k] = key;
    vals[k] = (int32_t)k;
}

__global__ __launch_bounds__(kPairsThreads) void pairs_gather_kernel(int64_t nvalid, const int32_t *__restrict__ vals, const pt *__restrict__ p0,
                                                                     const pt *__restrict__ p1, P4 *__restrict__ pts)
{
    const int64_t s = (int64_t)blockIdx.x * kPairsThreads + threadIdx.x;
    if (s >= nvalid) return;
    const int32_t k = vals[s];
    const pt a = p0[k], b = p1[k];
    P4 r;
    r.y0 = a.y; r.x0 = a.x; r.y1 = b.y; r.x1 = b.x;
    pts[s] = r;
}

// chunk_off[r], r = 0 .. ny: the home chunks of the rows in front of row r
__global__ __launch_bounds__(kPairsThreads) void pairs_rows_kernel(int ny, int nx, const int32_t *__restrict__ start, int32_t *__restrict__ chunk_off)
{
    __shared__ int32_t sm[kPairsThreads];
    const int span = (ny + kPairsThreads - 1) / kPairsThreads;
    const int r0 = (int)threadIdx.x * span, r1 = r0 + span < ny ? r0 + span : ny;
    int32_t mine = 0;
    for (int r = r0; r < r1; r++) mine += (start[(int64_t)(r + 1) * nx] - start[(int64_t)r * nx] + kPairsTile - 1) / kPairsTile;
    sm[threadIdx.x] = mine;
    __syncthreads();
    int32_t run = 0;
    for (int t = 0; t < (int)threadIdx.x; t++) run += sm[t];
    for (int r = r0; r < r1; r++) {
        chunk_off[r] = run;
        run += (start[(int64_t)(r + 1) * nx] - start[(int64_t)r * nx] + kPairsTile - 1) / kPairsTile;
    }
    if (r0 < ny && r1 == ny) chunk_off[ny] = run;
}

__global__ __launch_bounds__(kPairsTile) void pairs_kernel(PairsGrid g, PairsEdges E, int64_t cap, const int32_t *__restrict__ chunk_off,
                                                           const int32_t *__restrict__ start, const uint32_t *__restrict__ keys,
                                                           const P4 *__restrict__ pts, double *__restrict__ partials)
{
    __shared__ P4 tile[kPairsTile];
    __shared__ double sm[1][kPairsSums];
    const int lane = threadIdx.x;
    const int c = blockIdx.y;
    const int32_t w = (int32_t)blockIdx.x;
    double acc[kPairsSums];
#pragma unroll
    for (int k = 0; k < kPairsSums; k++) acc[k] = 0.0;

    if (w < chunk_off[g.ny]) {                                          // workgroup-uniform
        int lo = 0, hi = g.ny;                                         // chunk_off[lo] <= w < chunk_off[hi]
        for (int it = 0; it < g.row_steps; it++) {
            if (hi - lo > 1) {
                const int mid = lo + ((hi - lo) >> 1);
                if (chunk_off[mid] <= w) lo = mid; else hi = mid;
            }
        }
        const int r = lo;
        const int64_t row0 = (int64_t)r * g.nx;
        const int32_t s_a = start[row0] + kPairsTile * (w - chunk_off[r]);
        const int32_t row_end = start[row0 + g.nx];
        const int32_t s_b = s_a + kPairsTile < row_end ? s_a + kPairsTile : row_end;
        const int32_t si = s_a + lane;
        const bool home = si < s_b;
        const P4 me = pts[home ? si : s_a];
        const int cmin = (int)((int64_t)keys[s_a] - row0), cmax = (int)((int64_t)keys[s_b - 1] - row0);
        const double Elo = E.e2[c], Ehi = E.e2[c + 1], R = E.e[c + 1];

        // rows and, per row, columns that can hold a point within R of a home point.  A point's bin index is the floor of a
        // difference times inv_h, two roundings on a value below 2^13: off by less than 1e-11.  So two points d apart along an
        // axis lie at most floor(d*inv_h + 1e-9) + 1 bins apart along it, and the reach below is at least that
        const double rows = R * g.inv_h * kPairsSlack + kPairsSlackAbs + 1.0;
        const int kmax = rows < (double)(g.ny - 1 - r) ? (int)rows : g.ny - 1 - r;
        for (int dy = 0; dy <= kmax; dy++) {
            const double gap = dy > 1 ? (double)(dy - 1) * g.side * 0.999999 : 0.0;      // the rows are at least that far apart
            if (gap > R) break;
            const double cols = sqrt(R * R - gap * gap) * g.inv_h * kPairsSlack + kPairsSlackAbs + 1.0;
            const int kx = cols < (double)g.nx ? (int)cols : g.nx;                    // a NaN takes the whole row
            const int ca = cmin - kx > 0 ? cmin - kx : 0, cb = cmax + kx < g.nx - 1 ? cmax + kx : g.nx - 1;
            const int64_t rowd = row0 + (int64_t)dy * g.nx;
            const int32_t t0 = dy == 0 ? s_a : start[rowd + ca];
            const int32_t t1 = start[rowd + cb + 1];
            for (int32_t t = t0; t < t1; t += kPairsTile) {
                __syncthreads();                                       // the tile of the trip before has been read
                if (t + lane < t1) tile[lane] = pts[t + lane];
                __syncthreads();
                const int m = t1 - t < kPairsTile ? t1 - t : kPairsTile;
                for (int j = 0; j < m; j++) {
                    const P4 o = tile[j];
                    const bool mine = home && t + j > si;
                    const double dy0 = o.y0 - me.y0, dx0 = o.x0 - me.x0;
                    const double q0 = dy0 * dy0 + dx0 * dx0;
                    if (mine) acc[kPairsCols] = acc[kPairsCols] + 1.0;
                    if (mine && Elo <= q0 && q0 < Ehi && q0 > 0.0) {
                        const double dy1 = o.y1 - me.y1, dx1 = o.x1 - me.x1;
                        const double q1 = dy1 * dy1 + dx1 * dx1;
                        const double r0 = sqrt(q0), r1 = sqrt(q1);
                        const double d = (q1 - q0) / (r0 + r1);
                        const double e = d / r0;
                        const double ae = fabs(e), ee = e * e;
                        acc[0] = acc[0] + 1.0;
                        acc[1] = acc[1] + r0;
                        acc[2] = acc[2] + e;
                        acc[3] = acc[3] + ae;
                        acc[4] = acc[4] + ee;
                        acc[5] = acc[5] + ee * ae;
                        acc[6] = acc[6] + d * d;
                    }
                }
            }
        }
    }
    __syncthreads();
    const double s = block_sum<kPairsSums, kPairsTile>(acc, sm);
    if (lane < kPairsSums) partials[((int64_t)c * cap + w) * kPairsSums + lane] = s;
}

__global__ __launch_bounds__(kPairsTile) void pairs_table_kernel(int ny, int64_t cap, const int32_t *__restrict__ chunk_off,
                                                                 const double *__restrict__ partials, double *__restrict__ table)
{
    __shared__ double sm[1][kPairsSums];
    const int64_t nrows = chunk_off[ny];
    const double *rows = partials + (int64_t)blockIdx.x * cap * kPairsSums;
    double t[kPairsSums];
#pragma unroll
    for (int k = 0; k < kPairsSums; k++) t[k] = 0.0;
    for (int64_t row = threadIdx.x; row < nrows; row += kPairsTile) {
#pragma unroll
        for (int k = 0; k < kPairsSums; k++) t[k] = t[k] + rows[row * kPairsSums + k];
    }
    const double s = block_sum<kPairsSums, kPairsTile>(t, sm);
    if (threadIdx.x < kPairsSums) table[(int64_t)blockIdx.x * kPairsSums + threadIdx.x] = s;
}

// the snapshot of sitrk_pairs_mark over the CELL-SORTED state: position and validity byte in the caller's order
__global__ __launch_bounds__(kPairsThreads) void pairs_mark_kernel(int64_t n, BuoyState st, const int8_t *__restrict__ mask, pt *__restrict__ t0,
                                                                   int8_t *__restrict__ v0)
{
    const int64_t s = (int64_t)blockIdx.x * kPairsThreads + threadIdx.x;
    if (s >= n) return;
    const int32_t o = st.perm[s];
    bool ok = st.cell[s] >= 0;                                         // alive now
    if (mask != nullptr) ok = ok && mask[o] != 0;
    t0[o] = st.pos[s];
    v0[o] = ok ? 1 : 0;
}

inline unsigned nblk(int64_t n) { return sitrk::nblk(n, kPairsThreads); }

inline int64_t max_bins(int64_t nP)
{
    const int64_t want = 8 * nP > 4096 ? 8 * nP : 4096;
    return want < kPairsMaxBins ? want : kPairsMaxBins;
}

inline int64_t max_chunks(int64_t n, int64_t rows) { return n / kPairsTile + (rows < n ? rows : n) + 1; }

// the scratch of one call behind whatever holds its points
struct PairsBuf {
    uint32_t *k0, *k1;
    int32_t *v0, *v1, *start, *chunk_off;
    P4 *pts;
    double *partials, *table;
    unsigned long long *red;
    char *sort_tmp;
    size_t sort_bytes;
};

void pairs_carve(Carver &c, PairsBuf &b, int64_t nP, int nc)
{
    c.take(b.k0, nP); c.take(b.k1, nP); c.take(b.v0, nP); c.take(b.v1, nP); c.take(b.pts, nP);
    c.take(b.start, max_bins(nP) + 1); c.take(b.chunk_off, kPairsMaxSide + 1);
    c.take(b.partials, (size_t)nc * max_chunks(nP, kPairsMaxSide) * kPairsSums);
    c.take(b.table, (size_t)kPairsSums * SITRK_PAIRS_MAXCLASS); c.take(b.red, 5);
    c.take(b.sort_tmp, b.sort_bytes);
}

int pairs_sort_bytes(sitrk_ctx *h, int64_t nP, size_t *bytes)
{
    *bytes = 0;
    if (nP > 0) HIPCHK(sort_pairs_u32(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, (size_t)nP, 32, h->stream));
    *bytes = align256(*bytes);
    return SITRK_OK;
}

// what the compute entry points check before any device work; fills E
int pairs_check(sitrk_ctx *h, const char *fn, int nc, const double *edges, const double *table, PairsEdges *E)
{
    if (nc < 1 || nc > SITRK_PAIRS_MAXCLASS) return fail(h, SITRK_EINVAL, "%s: nc must be in 1..%d (got %d)", fn, SITRK_PAIRS_MAXCLASS, nc);
    if (!edges || !table) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    for (int c = 0; c <= nc; c++) {
        if (!std::isfinite(edges[c])) return fail(h, SITRK_EINVAL, "%s: edges_km[%d] is not finite", fn, c);
        if (c == 0 ? !(edges[0] >= 0.0) : !(edges[c] > edges[c - 1]))
            return fail(h, SITRK_EINVAL, "%s: edges_km must start at >= 0 and increase strictly (edges_km[%d] = %g)", fn, c, edges[c]);
    }
    for (int c = 0; c <= SITRK_PAIRS_MAXCLASS; c++) {
        E->e[c] = edges[c < nc ? c : nc];
        E->e2[c] = E->e[c] * E->e[c];
    }
    return SITRK_OK;
}

// the grid over the box [ylo, yhi] x [xlo, xhi]: bins of side R / kPairsBinFrac, doubled until the grid fits its caps
PairsGrid pairs_grid(double ylo, double yhi, double xlo, double xhi, double R, int64_t bins_max)
{
    PairsGrid g;
    g.ymin = ylo; g.xmin = xlo; g.inv_h = 0.0; g.side = 0.0; g.ny = 1; g.nx = 1; g.row_steps = 1;
    double side = R / kPairsBinFrac;
    if (!(side > 0.0)) side = R;
    for (int it = 0; it < 2200; it++, side *= 2.0) {
        const double inv = 1.0 / side;
        const double ty = (yhi - ylo) * inv, tx = (xhi - xlo) * inv;
        if (!std::isfinite(side) || !(inv > 0.0)) break;
        if (!(ty < (double)kPairsMaxSide - 1.0) || !(tx < (double)kPairsMaxSide - 1.0)) continue;
        const int64_t ny = (int64_t)std::floor(ty) + 1, nx = (int64_t)std::floor(tx) + 1;
        if (ny * nx > bins_max) continue;
        g.inv_h = inv; g.side = side; g.ny = (int)ny; g.nx = (int)nx;
        break;
    }
    while (((int64_t)1 << g.row_steps) < g.ny) g.row_steps++;
    g.row_steps++;
    return g;
}

// everything behind the points on the device -- p0, p1 (nP), m0 / m1 (nP) or null -- : queues the kernels, waits once for the
// bounding box, downloads the table and synchronises
int pairs_run(sitrk_ctx *h, int64_t nP, const pt *p0, const pt *p1, const int8_t *m0, const int8_t *m1, int nc, const PairsEdges &E,
              const PairsBuf &b, double *table, int64_t *npts)
{
    for (int k = 0; k < nc * kPairsCols; k++) table[k] = 0.0;
    if (npts) *npts = 0;
    h->pairs_tests = 0;
    RCCHK(h->pairs_timer.begin(h));
    RCCHK(h->pairs_timer.mark(h, 0));
    unsigned long long red[5] = {~0ull, 0ull, ~0ull, 0ull, 0ull};
    if (nP > 0) {
        HIPCHK(upload(h, b.red, red, 5));
        hipLaunchKernelGGL(pairs_box_kernel, dim3(nblk(nP)), dim3(kPairsThreads), 0, h->stream, nP, p0, p1, m0, m1, b.red);
        HIPCHK(hipGetLastError());
        HIPCHK(download(h, red, b.red, 5));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    const int64_t nvalid = (int64_t)red[4];
    if (npts) *npts = nvalid;
    const bool work = nvalid >= 2;
    PairsGrid g = {};
    int64_t cap = 1;
    if (work) {
        g = pairs_grid(order_value(red[0]), order_value(red[1]), order_value(red[2]), order_value(red[3]), E.e[nc], max_bins(nP));
        const int64_t nbins = (int64_t)g.ny * g.nx;
        cap = max_chunks(nvalid, g.ny);
        hipLaunchKernelGGL(pairs_key_kernel, dim3(nblk(nP)), dim3(kPairsThreads), 0, h->stream, nP, p0, p1, m0, m1, g, b.k0, b.v0);
        HIPCHK(hipGetLastError());
        size_t tb = b.sort_bytes;                                      // the keys run 0 .. nbins, nbins <= 2^22
        HIPCHK(sort_pairs_u32(b.sort_tmp, &tb, b.k0, b.k1, b.v0, b.v1, (size_t)nP, key_bits((uint64_t)nbins), h->stream));
        hipLaunchKernelGGL(pairs_gather_kernel, dim3(nblk(nvalid)), dim3(kPairsThreads), 0, h->stream, nvalid, b.v1, p0, p1, b.pts);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(bin_start_kernel<kPairsThreads>, dim3(nblk(nbins + 1)), dim3(kPairsThreads), 0, h->stream, nbins, (int32_t)nvalid,
                           lower_bound_steps(nvalid), b.k1, b.start);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pairs_rows_kernel, dim3(1), dim3(kPairsThreads), 0, h->stream, g.ny, g.nx, b.start, b.chunk_off);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->pairs_timer.mark(h, 1));
    if (work) {
        hipLaunchKernelGGL(pairs_kernel, dim3((unsigned)cap, (unsigned)nc), dim3(kPairsTile), 0, h->stream, g, E, cap, b.chunk_off, b.start, b.k1,
                           b.pts, b.partials);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->pairs_timer.mark(h, 2));
    if (work) {
        hipLaunchKernelGGL(pairs_table_kernel, dim3((unsigned)nc), dim3(kPairsTile), 0, h->stream, g.ny, cap, b.chunk_off, b.partials, b.table);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->pairs_timer.mark(h, 3));
    h->pairs_timer.done();
    if (work) {
        double sums[kPairsSums * SITRK_PAIRS_MAXCLASS];
        HIPCHK(download(h, sums, b.table, (size_t)kPairsSums * nc));
        HIPCHK(hipStreamSynchronize(h->stream));
        double tests = 0.0;
        for (int c = 0; c < nc; c++) {
            for (int k = 0; k < kPairsCols; k++) table[c * kPairsCols + k] = sums[c * kPairsSums + k];
            tests += sums[c * kPairsSums + kPairsCols];
        }
        h->pairs_tests = (unsigned long long)tests;
    } else {
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return SITRK_OK;
}

}  // namespace

void pairs_release(sitrk_ctx *h, bool destroy)
{
    if (h->pairs_t0) (void)hipFree(h->pairs_t0);
    if (h->pairs_v0) (void)hipFree(h->pairs_v0);
    h->pairs_t0 = nullptr;
    h->pairs_v0 = nullptr;
    h->pairs_marked = false;
    if (destroy) h->pairs_timer.release();
}

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_pairs_points(sitrk_t *h, int64_t nP, const double *yx0, const double *yx1, const int8_t *mask0, const int8_t *mask1,
                                 int nc, const double *edges_km, double *table, int64_t *npts)
{
    const char *fn = "sitrk_pairs_points";
    NEED(h, "null handle");
    PairsEdges E;
    RCCHK(pairs_check(h, fn, nc, edges_km, table, &E));
    if (!(nP >= 0 && nP < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nP must be in 0..2^31-2", fn);
    if (nP > 0 && !(yx0 && yx1)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    HIPCHK(hipSetDevice(h->device));
    PairsBuf b;
    RCCHK(pairs_sort_bytes(h, nP, &b.sort_bytes));
    pt *d_p0, *d_p1; int8_t *d_m0, *d_m1;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_p0, nP); c.take(d_p1, nP); c.take(d_m0, mask0 ? (size_t)nP : 0); c.take(d_m1, mask1 ? (size_t)nP : 0);
        pairs_carve(c, b, nP, nc);
    }));
    if (nP > 0) {
        HIPCHK(upload(h, d_p0, yx0, nP));
        HIPCHK(upload(h, d_p1, yx1, nP));
        if (mask0) HIPCHK(upload(h, d_m0, mask0, nP));
        if (mask1) HIPCHK(upload(h, d_m1, mask1, nP));
    }
    return pairs_run(h, nP, d_p0, d_p1, mask0 ? d_m0 : nullptr, mask1 ? d_m1 : nullptr, nc, E, b, table, npts);
}

SITRK_API int sitrk_pairs_mark(sitrk_t *h, int jrec0, const int8_t *mask)
{
    const char *fn = "sitrk_pairs_mark";
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    HIPCHK(hipSetDevice(h->device));
    const int64_t nP = h->nP;
    int8_t *d_mask = nullptr;
    if (mask) {
        RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_mask, nP); }));
        HIPCHK(upload(h, d_mask, mask, nP));
    }
    if (!h->pairs_t0) HIPCHK(hipMalloc((void **)&h->pairs_t0, (size_t)nP * sizeof(pt)));
    if (!h->pairs_v0) HIPCHK(hipMalloc((void **)&h->pairs_v0, (size_t)nP));
    hipLaunchKernelGGL(pairs_mark_kernel, dim3(nblk(nP)), dim3(kPairsThreads), 0, h->stream, nP, h->st[h->cur], d_mask, h->pairs_t0, h->pairs_v0);
    HIPCHK(hipGetLastError());
    if (mask) HIPCHK(hipStreamSynchronize(h->stream));                 // the caller's mask may go once the call returns
    h->pairs_marked = true;
    h->pairs_jrec0 = jrec0;
    return SITRK_OK;
}

SITRK_API int sitrk_pairs_since_mark(sitrk_t *h, int jrec1, int nc, const double *edges_km, double *table, int64_t *npts)
{
    const char *fn = "sitrk_pairs_since_mark";
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    if (!h->pairs_marked) return fail(h, SITRK_EINVAL, "%s: no mark (call sitrk_pairs_mark first; sitrk_set_buoys and sitrk_pairs_free cancel it)", fn);
    if (jrec1 < h->pairs_jrec0) return fail(h, SITRK_EINVAL, "%s: jrec1 = %d lies before the mark at record %d", fn, jrec1, h->pairs_jrec0);
    PairsEdges E;
    RCCHK(pairs_check(h, fn, nc, edges_km, table, &E));
    HIPCHK(hipSetDevice(h->device));
    const int64_t nP = h->nP;
    PairsBuf b;
    RCCHK(pairs_sort_bytes(h, nP, &b.sort_bytes));
    pt *d_p1;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_p1, nP); pairs_carve(c, b, nP, nc); }));
    RCCHK(deform_points_span(h, h->pairs_jrec0, jrec1, d_p1));         // NaN in y: not alive now, or its window does not cover the span
    return pairs_run(h, nP, h->pairs_t0, d_p1, h->pairs_v0, nullptr, nc, E, b, table, npts);
}

SITRK_API int sitrk_pairs_free(sitrk_t *h)
{
    NEED(h, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));            // a mark or a table still queued reads the snapshot
    pairs_release(h, false);
    return SITRK_OK;
}

SITRK_API int sitrk_pairs_kernel_ms(sitrk_t *h, float *bin_ms, float *pairs_ms, float *table_ms)
{
    NEED(h, "null handle");
    NEED(h->pairs_timer.complete, "sitrk_pairs_kernel_ms: no pair-dispersion call has run its kernels yet");
    float *out[3] = {bin_ms, pairs_ms, table_ms};
    for (int k = 0; k < 3; k++) RCCHK(h->pairs_timer.elapsed(h, k, out[k]));
    return SITRK_OK;
}

SITRK_API int sitrk_pairs_stats(sitrk_t *h, int64_t *tests)
{
    NEED(h, "null handle");
    NEED(h->pairs_timer.complete, "sitrk_pairs_stats: no pair-dispersion call has run its kernels yet");
    if (tests) *tests = (int64_t)h->pairs_tests;
    return SITRK_OK;
}
