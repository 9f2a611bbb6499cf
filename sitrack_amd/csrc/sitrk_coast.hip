// sitrk_coast.hip -- distance to the model's own coastline (sitrk_coast_build, sitrk_coast_segments, sitrk_coast_dist,
// sitrk_coast_dist_buoys): an EXTRA the reference does not have (it reads a rasterised dist2coast file through mojito).  Kept in
// its own translation unit so that the device code of sitrk.hip stays as it is.  The contract (which edges are coast, the
// distance expression, ties, rmax) is in include/sitrk.h.
//
// Build (one-off, sitrk_coast_build):
//   coast_flag_kernel     one lane per candidate edge 2*(j*Ni+i)+k: 1 where exactly one of the two cells is land and all four
//                         endpoint coordinates are finite; coast edges with a non-finite endpoint are counted
//   rocPRIM exclusive scan of the flags, coast_compact_kernel: ids and endpoints in id order
//   coast_stats_kernel    bounding box of the segments' midpoints, the longest segment, the largest coordinate
//   coast_key_kernel      square bins over that box, key = bin of the midpoint (row-major), the radix sort of sitrk_sort.hip
//                         (stable: id order inside a bin), coast_gather_kernel, bin_start_kernel of sitrk_bins.h (first segment
//                         of every bin)
// Query (coast_query_kernel, one query per lane, no LDS, no cross-lane work).  With pad >= half the longest segment, a segment
// at distance <= d from p has its midpoint within d + pad of p, and the bin of a coordinate is a monotone function of it, so all
// such segments lie in bin rows bin(py - R) .. bin(py + R) and, in each row, in ONE run of the bin-sorted segments, bins
// bin(px - R) .. bin(px + R), for R = d + pad:
//   phase 1  boxes of 1, 2, 4, ... bins around the query's (clamped) bin until one holds a segment -- two offsets per row and
//            box, no segment is read -- which bounds d by the box's farthest corner + pad (with rmax: never beyond rmax + pad);
//   phase 2  rows from the query's row outwards, each row's run evaluated by the contract's expression; R shrinks with every
//            improvement and the walk ends when both next rows lie outside bin(py -+ R).
// What is reported is the minimum of the contract's d2 over every segment that can attain it or tie with it, so the result does
// not depend on the bin side, on the order of evaluation or on the placement of the queries.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include "sitrk_bins.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kCoastThreads = 256;

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double plus_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ bool finite64(double a) { return fabs(a) < plus_inf(); }

// F-points as two strided arrays: (Yf, Xf, 1) for the caller's arrays, (&geoF->y, &geoF->x, 2) for the context's grid
struct FPoints {
    const double *y, *x;
    int stride;
    __device__ __forceinline__ pt at(int64_t c) const { return make_pt(y[c * stride], x[c * stride]); }
};

// edge e = 2*c + k of T-cell c = j*Ni + i: the cell on its other side and its endpoints a, b (include/sitrk.h)
__device__ __forceinline__ bool edge_of(int64_t e, int Nj, int Ni, int64_t *c, int64_t *other, int64_t *ca)
{
    const int k = (int)(e & 1);
    *c = e >> 1;
    const int j = (int)(*c / Ni), i = (int)(*c % Ni);
    if (k == 0) {
        *other = *c + 1; *ca = *c - Ni;
        return j >= 1 && i + 1 < Ni;
    }
    *other = *c + Ni; *ca = *c - 1;
    return i >= 1 && j + 1 < Nj;
}

__global__ __launch_bounds__(kCoastThreads) void coast_flag_kernel(int Nj, int Ni, FPoints F, const int8_t *__restrict__ tmask,
                                                                   uint8_t *__restrict__ flag, unsigned long long *ndropped)
{
    const int64_t e = (int64_t)blockIdx.x * kCoastThreads + threadIdx.x;
    if (e >= (int64_t)2 * Nj * Ni) return;
    int64_t c, other, ca;
    uint8_t f = 0;
    if (edge_of(e, Nj, Ni, &c, &other, &ca) && (tmask[c] == 0) != (tmask[other] == 0)) {
        const pt a = F.at(ca), b = F.at(c);
        if (finite64(a.y) && finite64(a.x) && finite64(b.y) && finite64(b.x)) f = 1;
        else atomicAdd(ndropped, 1ull);
    }
    flag[e] = f;
}

__global__ __launch_bounds__(kCoastThreads) void coast_compact_kernel(int Nj, int Ni, FPoints F, const uint8_t *__restrict__ flag,
                                                                      const int32_t *__restrict__ pos, int32_t *__restrict__ ids,
                                                                      pt *__restrict__ ab)
{
    const int64_t e = (int64_t)blockIdx.x * kCoastThreads + threadIdx.x;
    if (e >= (int64_t)2 * Nj * Ni || !flag[e]) return;
    int64_t c, other, ca;
    (void)edge_of(e, Nj, Ni, &c, &other, &ca);
    const int32_t p = pos[e];
    ids[p] = (int32_t)e;
    ab[2 * (int64_t)p] = F.at(ca);
    ab[2 * (int64_t)p + 1] = F.at(c);
}

// the point a segment is binned by, and the longest segment is measured around
__device__ __forceinline__ pt midpoint(pt a, pt b) { return make_pt(0.5 * a.y + 0.5 * b.y, 0.5 * a.x + 0.5 * b.x); }

__global__ void coast_stats_init_kernel(unsigned long long *red)
{
    if (threadIdx.x < 6) red[threadIdx.x] = threadIdx.x < 2 ? ~0ull : 0ull;
}

// red[0..3] = keys of min y, min x, max y, max x of the midpoints; red[4] = key of the largest |b - a|^2; red[5] = key of the
// largest |coordinate|
__global__ __launch_bounds__(kCoastThreads) void coast_stats_kernel(int64_t nseg, const pt *__restrict__ ab, unsigned long long *red)
{
    unsigned long long r[6] = {~0ull, ~0ull, 0ull, 0ull, 0ull, 0ull};
    for (int64_t s = (int64_t)blockIdx.x * kCoastThreads + threadIdx.x; s < nseg; s += (int64_t)gridDim.x * kCoastThreads) {
        const pt a = ab[2 * s], b = ab[2 * s + 1], m = midpoint(a, b);
        const double ey = b.y - a.y, ex = b.x - a.x;
        const unsigned long long ky = order_key(m.y), kx = order_key(m.x);
        r[0] = min(r[0], ky); r[1] = min(r[1], kx); r[2] = max(r[2], ky); r[3] = max(r[3], kx);
        r[4] = max(r[4], order_key(ey * ey + ex * ex));
        r[5] = max(r[5], order_key(fmax(fmax(fabs(a.y), fabs(a.x)), fmax(fabs(b.y), fabs(b.x)))));
    }
    __shared__ unsigned long long sm[6][kCoastThreads];
#pragma unroll
    for (int q = 0; q < 6; q++) sm[q][threadIdx.x] = r[q];
    __syncthreads();
    block_reduce<kCoastThreads, Red::Min, Red::Min, Red::Max, Red::Max, Red::Max, Red::Max>(sm);
    if (threadIdx.x < 6) {
        if (threadIdx.x < 2) atomicMin(&red[threadIdx.x], sm[threadIdx.x][0]);
        else atomicMax(&red[threadIdx.x], sm[threadIdx.x][0]);
    }
}

// Deliberately not cell_coord of sitrk_bins.h: truncation by (int)t, not floor, and NaN / -inf go to bin 0, +inf to the last.
// THE bin of a coordinate: a monotone (non-decreasing) function of v, which is all the query relies on.  Coordinates outside the
// bins' extent, +-inf included, go to the first / last bin.
__device__ __forceinline__ int bin_of(double v, double v0, double inv_h, int n)
{
    const double t = (v - v0) * inv_h;
    if (!(t > 0.0)) return 0;
    if (t >= (double)n) return n - 1;
    return (int)t;
}

__global__ __launch_bounds__(kCoastThreads) void coast_key_kernel(CoastIndex ix, const pt *__restrict__ ab, uint32_t *__restrict__ key,
                                                                  int32_t *__restrict__ val)
{
    const int64_t s = (int64_t)blockIdx.x * kCoastThreads + threadIdx.x;
    if (s >= ix.nseg) return;
    const pt m = midpoint(ab[2 * s], ab[2 * s + 1]);
    key[s] = (uint32_t)bin_of(m.y, ix.y0, ix.inv_h, ix.ny) * (uint32_t)ix.nx + (uint32_t)bin_of(m.x, ix.x0, ix.inv_h, ix.nx);
    val[s] = (int32_t)s;
}

__global__ __launch_bounds__(kCoastThreads) void coast_gather_kernel(int64_t nseg, const int32_t *__restrict__ order,
                                                                     const int32_t *__restrict__ ids, const pt *__restrict__ ab,
                                                                     pt *__restrict__ seg, int32_t *__restrict__ sid)
{
    const int64_t s = (int64_t)blockIdx.x * kCoastThreads + threadIdx.x;
    if (s >= nseg) return;
    const int64_t o = order[s];
    seg[2 * s] = ab[2 * o];
    seg[2 * s + 1] = ab[2 * o + 1];
    sid[s] = ids[o];
}

// the contract's squared distance of p to segment (a, b): one rounded operation per symbol, no FMA
__device__ __forceinline__ double seg_d2(pt p, pt a, pt b)
{
    const double ey = b.y - a.y, ex = b.x - a.x, py = p.y - a.y, px = p.x - a.x;
    const double eyy = ey * ey, exx = ex * ex, len2 = eyy + exx;
    const double pey = py * ey, pex = px * ex, dot = pey + pex;
    double t = (len2 > 0.0) ? dot / len2 : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double ty = t * ey, tx = t * ex, cy = py - ty, cx = px - tx;
    const double cyy = cy * cy, cxx = cx * cx;
    return cyy + cxx;
}

// Search radius for the midpoints once the best distance is d: d + pad, widened by far more than the roundings of this sum, of
// the device's sqrt behind d and of py -+ R can amount to (a wider radius only costs time)
__device__ __forceinline__ double search_radius(double d, double pad, pt p)
{
    return (d + pad) * (1.0 + 0x1p-30) + (fabs(p.y) + fabs(p.x)) * 0x1p-40;
}

// perm == nullptr: query q is yx[q]; else yx is the cell-sorted buoy state and slot q reports at perm[q] (the caller's order)
__global__ __launch_bounds__(kCoastThreads) void coast_query_kernel(CoastIndex ix, int64_t n, const pt *__restrict__ yx,
                                                                    const int32_t *__restrict__ perm, double rmax, double r2,
                                                                    double *__restrict__ dist, int32_t *__restrict__ seg_out)
{
    const int64_t q = (int64_t)blockIdx.x * kCoastThreads + threadIdx.x;
    if (q >= n) return;
    const int64_t o = perm ? (int64_t)perm[q] : q;
    const pt p = yx[q];
    double d_out = plus_inf();
    int32_t s_out = -1;
    if (ix.nseg > 0 && !(finite64(p.y) && finite64(p.x))) d_out = quiet_nan();
    else if (ix.nseg > 0) {
        const bool bounded = rmax > 0.0;                        // the host passes 0 for "unbounded"
        const double r_cap = bounded ? search_radius(rmax, ix.pad, p) : plus_inf();
        const int cy = bin_of(p.y, ix.y0, ix.inv_h, ix.ny), cx = bin_of(p.x, ix.x0, ix.inv_h, ix.nx);
        // phase 1: the smallest box of 2w+1 bins a side, w = 1, 2, 4, ..., that holds a segment
        double R = r_cap;
        for (int w = 1;; w *= 2) {
            if ((double)w * ix.h >= r_cap) break;               // the box reaches beyond rmax + pad on every side it has bins on
            const int ylo = max(cy - w, 0), yhi = min(cy + w, ix.ny - 1), xlo = max(cx - w, 0), xhi = min(cx + w, ix.nx - 1);
            bool any = false;
            for (int by = ylo; by <= yhi && !any; by++) {
                const int64_t row = (int64_t)by * ix.nx;
                any = ix.start[row + xhi + 1] > ix.start[row + xlo];
            }
            if (any) {
                // some midpoint lies in the box: not further than its farthest corner
                const double fy = fmax(fabs(p.y - (ix.y0 + (double)ylo * ix.h)), fabs(p.y - (ix.y0 + (double)(yhi + 1) * ix.h)));
                const double fx = fmax(fabs(p.x - (ix.x0 + (double)xlo * ix.h)), fabs(p.x - (ix.x0 + (double)(xhi + 1) * ix.h)));
                R = fmin(r_cap, search_radius(sqrt(fy * fy + fx * fx), ix.pad, p));
                break;
            }
            if (ylo == 0 && yhi == ix.ny - 1 && xlo == 0 && xhi == ix.nx - 1) break;     // (cannot happen with nseg > 0)
        }
        // phase 2: rows outwards, every row's run of segments by the contract's expression
        double best = plus_inf();
        int32_t bid = INT32_MAX;
        for (int k = 0;; k++) {
            const int ylo = bin_of(p.y - R, ix.y0, ix.inv_h, ix.ny), yhi = bin_of(p.y + R, ix.y0, ix.inv_h, ix.ny);
            const bool down = cy - k >= ylo, up = k > 0 && cy + k <= yhi;
            if (!down && !up) break;
            for (int side = 0; side < 2; side++) {
                if (!(side ? up : down)) continue;
                const int64_t row = (int64_t)(side ? cy + k : cy - k) * ix.nx;
                const int xlo = bin_of(p.x - R, ix.x0, ix.inv_h, ix.nx), xhi = bin_of(p.x + R, ix.x0, ix.inv_h, ix.nx);
                const int32_t s1 = ix.start[row + xhi + 1];
                for (int32_t s = ix.start[row + xlo]; s < s1; s++) {
                    const double d2 = seg_d2(p, ix.seg[2 * (int64_t)s], ix.seg[2 * (int64_t)s + 1]);
                    if (d2 <= best) {
                        const int32_t id = ix.sid[s];
                        if (d2 < best || id < bid) {
                            best = d2; bid = id;
                            R = fmin(R, search_radius(sqrt(best), ix.pad, p));
                        }
                    }
                }
            }
        }
        if (bid != INT32_MAX && !(bounded && best > r2)) { d_out = sqrt(best); s_out = bid; }
    }
    dist[o] = d_out;
    if (seg_out) seg_out[o] = s_out;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kCoastThreads - 1) / kCoastThreads); }

void coast_free(sitrk_ctx *h)
{
    CoastState &c = h->coast;
    if (c.ids) (void)hipFree(c.ids);
    if (c.ab) (void)hipFree(c.ab);
    if (c.seg) (void)hipFree(c.seg);
    if (c.sid) (void)hipFree(c.sid);
    if (c.start) (void)hipFree(c.start);
    c.ids = nullptr; c.ab = nullptr; c.seg = nullptr; c.sid = nullptr; c.start = nullptr;
    c.ix = CoastIndex();
    c.built = false; c.from_grid = false; c.ndropped = 0;
}

}  // namespace

void coast_release(sitrk_ctx *h, bool grid_changed, bool destroy)
{
    if (!grid_changed || h->coast.from_grid) coast_free(h);
    if (destroy) h->coast.timer.release();
}

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_coast_build(sitrk_t *h, int Nj, int Ni, const double *Yf, const double *Xf, const int8_t *tmask, int64_t *nseg,
                                int64_t *ndropped)
{
    const char *fn = "sitrk_coast_build";
    NEED(h, "null handle");
    const bool from_grid = !Yf && !Xf && !tmask;
    if (!from_grid && !(Yf && Xf && tmask)) return fail(h, SITRK_EINVAL, "%s: Yf, Xf and tmask must be given together, or all three NULL", fn);
    if (from_grid) {
        if (!h->geoF || !h->tmask) return fail(h, SITRK_EINVAL, "%s: no grid (call sitrk_set_grid first, or pass Yf, Xf and tmask)", fn);
        if ((Nj || Ni) && (Nj != h->Nj || Ni != h->Ni))
            return fail(h, SITRK_EINVAL, "%s: Nj x Ni = %d x %d is not the grid of sitrk_set_grid (%d x %d)", fn, Nj, Ni, h->Nj, h->Ni);
        Nj = h->Nj; Ni = h->Ni;
    }
    if (Nj < 2 || Ni < 2 || (int64_t)Nj * Ni > ((int64_t)1 << 29))
        return fail(h, SITRK_EINVAL, "%s: grid %dx%d outside 2 <= Nj, Ni and Nj*Ni <= 2^29", fn, Nj, Ni);
    if (nseg) *nseg = 0;
    if (ndropped) *ndropped = 0;
    HIPCHK(hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    HIPCHK(hipStreamSynchronize(st));                           // no query of the previous index is in flight
    coast_free(h);
    CoastState &cs = h->coast;
    RCCHK(cs.timer.create(h));

    // ---- the segments, in id order
    const size_t ncell = (size_t)Nj * Ni, nedge = 2 * ncell;
    double *d_yf = nullptr, *d_xf = nullptr; int8_t *d_tm = nullptr; uint8_t *flag; int32_t *pos; char *scan_tmp;
    unsigned long long *red;
    size_t scan_bytes = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, scan_bytes, (uint8_t *)nullptr, (int32_t *)nullptr, (int32_t)0, nedge, rocprim::plus<int32_t>(), st));
    RCCHK(carve_scratch(h, [&](Carver &c) {
        if (!from_grid) { c.take(d_yf, ncell); c.take(d_xf, ncell); c.take(d_tm, ncell); }
        c.take(flag, nedge); c.take(pos, nedge); c.take(scan_tmp, scan_bytes); c.take(red, 8);
    }));
    FPoints F;
    const int8_t *tm;
    if (from_grid) {
        F.y = &h->geoF->y; F.x = &h->geoF->x; F.stride = 2;
        tm = h->tmask;
    } else {
        HIPCHK(upload(h, d_yf, Yf, ncell));
        HIPCHK(upload(h, d_xf, Xf, ncell));
        HIPCHK(upload(h, d_tm, tmask, ncell));
        F.y = d_yf; F.x = d_xf; F.stride = 1;
        tm = d_tm;
    }
    HIPCHK(hipMemsetAsync(red + 6, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(coast_flag_kernel, dim3(nblk((int64_t)nedge)), dim3(kCoastThreads), 0, st, Nj, Ni, F, tm, flag, red + 6);
    HIPCHK(hipGetLastError());
    size_t tb = align256(scan_bytes);
    HIPCHK(rocprim::exclusive_scan(scan_tmp, tb, flag, pos, (int32_t)0, nedge, rocprim::plus<int32_t>(), st));
    int32_t last_pos = 0; uint8_t last_flag = 0; unsigned long long ndrop = 0;
    HIPCHK(download(h, &last_pos, pos + (nedge - 1), 1));
    HIPCHK(download(h, &last_flag, flag + (nedge - 1), 1));
    HIPCHK(download(h, &ndrop, red + 6, 1));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t n = (int64_t)last_pos + last_flag;
    cs.ndropped = (int64_t)ndrop;
    cs.from_grid = from_grid;
    if (nseg) *nseg = n;
    if (ndropped) *ndropped = cs.ndropped;
    if (n == 0) {                                               // no coast: every query reports +inf, -1
        cs.built = true;
        return SITRK_OK;
    }
    HIPCHK(hipMalloc((void **)&cs.ids, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc((void **)&cs.ab, (size_t)2 * n * sizeof(pt)));
    hipLaunchKernelGGL(coast_compact_kernel, dim3(nblk((int64_t)nedge)), dim3(kCoastThreads), 0, st, Nj, Ni, F, flag, pos, cs.ids, cs.ab);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(coast_stats_init_kernel, dim3(1), dim3(64), 0, st, red);
    hipLaunchKernelGGL(coast_stats_kernel, dim3(std::min(nblk(n), 2048u)), dim3(kCoastThreads), 0, st, n, cs.ab, red);
    HIPCHK(hipGetLastError());
    unsigned long long r[6];
    HIPCHK(download(h, r, red, 6));
    HIPCHK(hipStreamSynchronize(st));                           // the scratch of this stage is free from here on

    // ---- the bins
    const double lo[2] = {order_value(r[0]), order_value(r[1])};
    const double hi[2] = {order_value(r[2]), order_value(r[3])};
    const double longest = std::sqrt(order_value(r[4])), cmax = order_value(r[5]);
    // side: coast_bin quarters of the spacing n segments would have if they filled the midpoints' bounding box evenly -- about
    // one segment per bin at the default, whatever the mesh; a coast on a line, or a single segment, gets the longest segment
    double side = 0.25 * h->coast_bin * std::sqrt((hi[0] - lo[0]) * (hi[1] - lo[1]) / (double)n);
    if (!(side > 0.0) || !std::isfinite(side)) side = longest > 0.0 && std::isfinite(longest) ? longest : 1.0;
    CoastIndex ix;
    ix.nseg = n; ix.y0 = lo[0]; ix.x0 = lo[1];
    int64_t nb[2] = {1, 1};
    const int64_t max_cells = std::min<int64_t>(16 * n + 1024, (int64_t)1 << 30);
    if (!fit_cell_grid(2, lo, hi, side, max_cells, &ix.inv_h, nb))
        return fail(h, SITRK_EINVAL, "%s: no bin grid fits the coast's extent", fn);
    ix.h = 1.0 / ix.inv_h;
    ix.ny = (int)nb[0]; ix.nx = (int)nb[1];
    // half the longest segment (rounded up), and what the bins' own arithmetic can be off by
    ix.pad = 0.5 * longest * (1.0 + 0x1p-20) + (ix.h + cmax) * 0x1p-30;
    const int64_t nbins = nb[0] * nb[1];
    const unsigned end_bit = key_bits((uint64_t)nbins - 1);
    size_t b_sort = 0;
    HIPCHK(sort_pairs_u32(nullptr, &b_sort, nullptr, nullptr, nullptr, nullptr, (size_t)n, 32, st));
    uint32_t *k0, *k1; int32_t *v0, *v1; char *sort_tmp;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(k0, n); c.take(k1, n); c.take(v0, n); c.take(v1, n); c.take(sort_tmp, b_sort);
    }));
    HIPCHK(hipMalloc((void **)&cs.seg, (size_t)2 * n * sizeof(pt)));
    HIPCHK(hipMalloc((void **)&cs.sid, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc((void **)&cs.start, (size_t)(nbins + 1) * sizeof(int32_t)));
    hipLaunchKernelGGL(coast_key_kernel, dim3(nblk(n)), dim3(kCoastThreads), 0, st, ix, cs.ab, k0, v0);
    HIPCHK(hipGetLastError());
    tb = align256(b_sort);
    HIPCHK(sort_pairs_u32(sort_tmp, &tb, k0, k1, v0, v1, (size_t)n, end_bit, st));
    hipLaunchKernelGGL(coast_gather_kernel, dim3(nblk(n)), dim3(kCoastThreads), 0, st, n, v1, cs.ids, cs.ab, cs.seg, cs.sid);
    hipLaunchKernelGGL(bin_start_kernel<kCoastThreads>, dim3(nblk(nbins + 1)), dim3(kCoastThreads), 0, st, nbins, (int32_t)n,
                       lower_bound_steps(n), k1, cs.start);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    ix.seg = cs.seg; ix.sid = cs.sid; ix.start = cs.start;
    cs.ix = ix;
    cs.built = true;
    return SITRK_OK;
}

SITRK_API int sitrk_coast_segments(sitrk_t *h, int64_t cap, int32_t *ids, double *ab, int64_t *n)
{
    const char *fn = "sitrk_coast_segments";
    NEED(h, "null handle");
    NEED(n, "sitrk_coast_segments: null n");
    if (!h->coast.built) return fail(h, SITRK_EINVAL, "%s: no coast index (call sitrk_coast_build first)", fn);
    const int64_t ns = h->coast.ix.nseg;
    *n = ns;
    if (cap < ns || ns == 0 || (!ids && !ab)) return SITRK_OK;  // the count alone
    HIPCHK(hipSetDevice(h->device));
    if (ids) HIPCHK(download(h, ids, h->coast.ids, (size_t)ns));
    if (ab) HIPCHK(download(h, ab, h->coast.ab, (size_t)2 * ns));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

// what both distance entry points check first
static int coast_check(sitrk_ctx *h, const char *fn, double rmax_km, double *rmax, double *r2)
{
    if (!h->coast.built) return fail(h, SITRK_EINVAL, "%s: no coast index (call sitrk_coast_build first; sitrk_set_grid drops one built from the grid)", fn);
    if (std::isnan(rmax_km)) return fail(h, SITRK_EINVAL, "%s: rmax_km is NaN", fn);
    const bool bounded = rmax_km > 0.0 && std::isfinite(rmax_km);
    *rmax = bounded ? rmax_km : 0.0;
    *r2 = bounded ? rmax_km * rmax_km : 0.0;
    return SITRK_OK;
}

// the query kernel between its two events, then the results to the host
static int coast_run(sitrk_ctx *h, int64_t n, const pt *d_yx, const int32_t *perm, double rmax, double r2, double *d_dist, int32_t *d_seg,
                     double *dist, int32_t *seg)
{
    CoastState &cs = h->coast;
    RCCHK(cs.timer.mark(h, 0));
    hipLaunchKernelGGL(coast_query_kernel, dim3(nblk(n)), dim3(kCoastThreads), 0, h->stream, cs.ix, n, d_yx, perm, rmax, r2, d_dist,
                       seg ? d_seg : (int32_t *)nullptr);
    HIPCHK(hipGetLastError());
    RCCHK(cs.timer.mark(h, 1));
    cs.timer.done();
    HIPCHK(download(h, dist, d_dist, (size_t)n));
    if (seg) HIPCHK(download(h, seg, d_seg, (size_t)n));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

SITRK_API int sitrk_coast_dist(sitrk_t *h, int64_t n, const double *yx, double rmax_km, double *dist, int32_t *seg)
{
    const char *fn = "sitrk_coast_dist";
    NEED(h, "null handle");
    double rmax, r2;
    RCCHK(coast_check(h, fn, rmax_km, &rmax, &r2));
    if (!(n >= 0 && n < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: n must be in 0..2^31-2", fn);
    if (n == 0) return SITRK_OK;
    if (!(yx && dist)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    HIPCHK(hipSetDevice(h->device));
    pt *d_yx; double *d_dist; int32_t *d_seg;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_yx, n); c.take(d_dist, n); c.take(d_seg, n); }));
    HIPCHK(upload(h, d_yx, yx, (size_t)n));
    return coast_run(h, n, d_yx, nullptr, rmax, r2, d_dist, d_seg, dist, seg);
}

SITRK_API int sitrk_coast_dist_buoys(sitrk_t *h, double rmax_km, double *dist, int32_t *seg)
{
    const char *fn = "sitrk_coast_dist_buoys";
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    double rmax, r2;
    RCCHK(coast_check(h, fn, rmax_km, &rmax, &r2));
    if (!dist) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->nP;
    double *d_dist; int32_t *d_seg;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_dist, n); c.take(d_seg, n); }));
    const BuoyState &b = h->st[h->cur];
    return coast_run(h, n, b.pos, b.perm, rmax, r2, d_dist, d_seg, dist, seg);
}

SITRK_API int sitrk_coast_kernel_ms(sitrk_t *h, float *query_ms)
{
    NEED(h, "null handle");
    NEED(h->coast.timer.complete, "sitrk_coast_kernel_ms: no distance call has run its kernel yet");
    return h->coast.timer.elapsed(h, 0, query_ms);
}
