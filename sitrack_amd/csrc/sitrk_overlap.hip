// sitrk_overlap.hip -- overlap cleaning of a tracked cloud (sitrk_cancel_too_close, sitrk_nearest_buoy): the reference's
// util.CancelTooClose (sitrack/util.py:520-565).  Kept in its own translation unit so that the device code of sitrk.hip
// stays as it is.
//
// Stage 1 (nearest other valid buoy within rd, per valid buoy), driven by overlap_stage1() at the end of this file:
//   1. unit_bbox_kernel  bounding box of the valid buoys' unit vectors and the first valid index with a non-finite coordinate
//   2. bin_key_kernel    cubic cells of side h >= chord(rd) (padded) over that box; key = cell (invalid buoys: ncells, sorted
//                        last); the rocPRIM radix sort of sitrk_sort.hip orders the buoys by cell
//   3. bin_gather_kernel sorted unit vectors and [lat,lon], and the [start,end) range of every cell
//   4. nearest_kernel    one thread per sorted buoy over the 27 neighbouring cells: pass 1 takes the minimum chord^2, pass 2
//                        evaluates the reference Haversine only on the candidates within the margin of that minimum and keeps
//                        the smallest distance, lowest index on ties (the bound is in DESIGN.md section 3.6)
// Stage 2 (close set, dmin < rd, in index order): flag_kernel, the rocPRIM exclusive scan below, close_scatter_kernel, with the
// neighbour remapped to its position in the compact list.  Stage 3, the sequential scan of the reference, runs on the host.
#include <algorithm>
#include <cmath>
#include <vector>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include "sitrk_bins.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kOvThreads = 256;

__device__ __forceinline__ V3 unit_vec(double lat, double lon)
{
    const double to_rad = 3.141592653589793 / 180.;
    double sl, cl, sp, cp;
    sincos(lon * to_rad, &sl, &cl);
    sincos(lat * to_rad, &sp, &cp);
    V3 v;
    v.x = cp * cl; v.y = cp * sl; v.z = sp; v.w = 0.0;
    return v;
}

// squared chord between two unit vectors: three rounded products, two rounded sums, no FMA
__device__ __forceinline__ double chord2(V3 a, V3 b)
{
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// Haversine   reference sitrack/util.py:85-103 (R = 6360 km), the operation order of sitrk_kernels.h's haversine: plat is the
// buoy the distances are measured from (the reference's Haversine(zlat[jb], zlon[jb], zlat, zlon)), cos_plat = cos(plat*to_rad)
__device__ __forceinline__ double haversine(double plat, double plon, double cos_plat, double xlat, double xlon)
{
    const double to_rad = 3.141592653589793 / 180.;
    const double R = 6360.;
    double a1 = sin(0.5 * ((xlat - plat) * to_rad));
    double a2 = sin(0.5 * ((xlon - plon) * to_rad));
    double a3 = cos(xlat * to_rad) * cos_plat;
    return 2. * R * asin(sqrt(a1 * a1 + a3 * a2 * a2));
}

__device__ __forceinline__ bool is_valid(const int8_t *valid, int64_t i) { return valid == nullptr || valid[i] != 0; }

__global__ void bbox_init_kernel(unsigned long long *red)
{
    if (threadIdx.x < 8) red[threadIdx.x] = (threadIdx.x < 3 || threadIdx.x == 6) ? ~0ull : 0ull;
}

// red[0..2] = keys of xmin, ymin, zmin; red[3..5] = keys of xmax, ymax, zmax (valid finite buoys); red[6] = first valid index with
// a non-finite coordinate (all-ones: none); red[7] = number of valid buoys
__global__ __launch_bounds__(kOvThreads) void unit_bbox_kernel(int64_t n, const double *__restrict__ lat, const double *__restrict__ lon,
                                                              const int8_t *__restrict__ valid, unsigned long long *red)
{
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0}, bad = ~0ull, cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * kOvThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kOvThreads) {
        if (!is_valid(valid, i)) continue;
        const double la = lat[i], lo_ = lon[i];
        if (!isfinite(la) || !isfinite(lo_)) {
            bad = min(bad, (unsigned long long)i);
            continue;
        }
        cnt++;
        const V3 v = unit_vec(la, lo_);
        const unsigned long long k[3] = {order_key(v.x), order_key(v.y), order_key(v.z)};
        for (int c = 0; c < 3; c++) { lo[c] = min(lo[c], k[c]); hi[c] = max(hi[c], k[c]); }
    }
    __shared__ unsigned long long sm[8][kOvThreads];
    for (int c = 0; c < 3; c++) { sm[c][threadIdx.x] = lo[c]; sm[3 + c][threadIdx.x] = hi[c]; }
    sm[6][threadIdx.x] = bad;
    sm[7][threadIdx.x] = cnt;
    __syncthreads();
    block_reduce<kOvThreads, Red::Min, Red::Min, Red::Min, Red::Max, Red::Max, Red::Max, Red::Min, Red::Add>(sm);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) { atomicMin(&red[c], sm[c][0]); atomicMax(&red[3 + c], sm[3 + c][0]); }
        atomicMin(&red[6], sm[6][0]);
        if (sm[7][0]) atomicAdd(&red[7], sm[7][0]);
    }
}

__device__ __forceinline__ uint32_t cell_of(const OvGrid &g, V3 v)
{
    const int cx = cell_coord(v.x, g.x0, g.inv_h, g.nx), cy = cell_coord(v.y, g.y0, g.inv_h, g.ny);
    const int cz = cell_coord(v.z, g.z0, g.inv_h, g.nz);
    return ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
}

// invalid buoys get key ncells: they sort after every cell and belong to none
__global__ __launch_bounds__(kOvThreads) void bin_key_kernel(OvGrid g, int64_t n, const double *__restrict__ lat,
                                                            const double *__restrict__ lon, const int8_t *__restrict__ valid,
                                                            uint32_t *key, int32_t *val)
{
    const int64_t i = (int64_t)blockIdx.x * kOvThreads + threadIdx.x;
    if (i >= n) return;
    key[i] = is_valid(valid, i) ? cell_of(g, unit_vec(lat[i], lon[i])) : g.ncells;
    val[i] = (int32_t)i;
}

__global__ __launch_bounds__(kOvThreads) void bin_gather_kernel(OvGrid g, int64_t n, const double *__restrict__ lat,
                                                               const double *__restrict__ lon, const uint32_t *__restrict__ key,
                                                               const int32_t *__restrict__ perm, V3 *uv_s, ll *ll_s, int32_t *cstart,
                                                               int32_t *cend)
{
    const int64_t s = (int64_t)blockIdx.x * kOvThreads + threadIdx.x;
    if (s >= n) return;
    const uint32_t k = key[s];
    if (k >= g.ncells) return;
    const int32_t i = perm[s];
    const double la = lat[i], lo = lon[i];
    uv_s[s] = unit_vec(la, lo);
    ll p; p.lat = la; p.lon = lo;
    ll_s[s] = p;
    mark_cell_run(key, s, n, cstart, cend);
}

// Results in input order: nn = input index of the nearest other valid buoy when its distance is < rd, else -1 (dmin +inf).
__global__ __launch_bounds__(kOvThreads) void nearest_kernel(OvGrid g, int64_t n, double rd_km, double cut2,
                                                            const uint32_t *__restrict__ key, const int32_t *__restrict__ perm,
                                                            const V3 *__restrict__ uv, const ll *__restrict__ lls,
                                                            const int32_t *__restrict__ cstart, const int32_t *__restrict__ cend,
                                                            int32_t *nn, double *dmin)
{
    const int64_t s = (int64_t)blockIdx.x * kOvThreads + threadIdx.x;
    if (s >= n) return;
    const int32_t me = perm[s];
    const uint32_t k = key[s];
    int32_t best_i = -1;
    double best = INFINITY;
    if (k < g.ncells) {
        const int cx = (int)(k % (uint32_t)g.nx), cy = (int)((k / (uint32_t)g.nx) % (uint32_t)g.ny);
        const int cz = (int)(k / ((uint32_t)g.nx * (uint32_t)g.ny));
        const V3 P = uv[s];
        // pass 1: minimum chord^2 to any other valid buoy of the 27 cells
        double cmin = INFINITY;
        for (int c = 0; c < 27; c++) {
            const int zz = cz + c / 9 - 1, yy = cy + (c / 3) % 3 - 1, xx = cx + c % 3 - 1;
            if (zz < 0 || zz >= g.nz || yy < 0 || yy >= g.ny || xx < 0 || xx >= g.nx) continue;
            const int64_t cc = ((int64_t)zz * g.ny + yy) * g.nx + xx;
            const int32_t e = cend[cc];
            for (int32_t q = cstart[cc]; q < e; q++)
                if (q != s) cmin = fmin(cmin, chord2(P, uv[q]));
        }
        // nothing within the chord of rd (with its slack) can be closer than rd: skip pass 2
        if (cmin <= cut2) {
            const double t = sqrt(cmin) * (1.0 + 1e-9) + 1e-13;
            const double thr = t * t;
            const ll L = lls[s];
            const double cos_plat = cos(L.lat * (3.141592653589793 / 180.));
            for (int c = 0; c < 27; c++) {
                const int zz = cz + c / 9 - 1, yy = cy + (c / 3) % 3 - 1, xx = cx + c % 3 - 1;
                if (zz < 0 || zz >= g.nz || yy < 0 || yy >= g.ny || xx < 0 || xx >= g.nx) continue;
                const int64_t cc = ((int64_t)zz * g.ny + yy) * g.nx + xx;
                const int32_t e = cend[cc];
                for (int32_t q = cstart[cc]; q < e; q++) {
                    if (q == s || !(chord2(P, uv[q]) <= thr)) continue;
                    const ll Q = lls[q];
                    const double d = haversine(L.lat, L.lon, cos_plat, Q.lat, Q.lon);
                    const int32_t qi = perm[q];
                    if (d < best || (d == best && qi < best_i)) { best = d; best_i = qi; }
                }
            }
        }
        if (!(best < rd_km)) { best = INFINITY; best_i = -1; }
    }
    nn[me] = best_i;
    dmin[me] = best;
}

__global__ __launch_bounds__(kOvThreads) void flag_kernel(int64_t n, const int32_t *__restrict__ nn, int32_t *flag)
{
    const int64_t i = (int64_t)blockIdx.x * kOvThreads + threadIdx.x;
    if (i < n) flag[i] = nn[i] >= 0 ? 1 : 0;
}

// pos = exclusive scan of the flags: close buoy i goes to position pos[i]; its neighbour nn[i] is close too,
// -1 flags a broken closure (the host reports it)
__global__ __launch_bounds__(kOvThreads) void close_scatter_kernel(int64_t n, const int32_t *__restrict__ nn, const int32_t *__restrict__ pos,
                                                                  int32_t *cidx, int32_t *cnn)
{
    const int64_t i = (int64_t)blockIdx.x * kOvThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t j = nn[i];
    if (j < 0) return;
    const int32_t p = pos[i];
    cidx[p] = (int32_t)i;
    cnn[p] = nn[j] >= 0 ? pos[j] : -1;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kOvThreads - 1) / kOvThreads); }

}  // namespace

}  // namespace sitrk

using namespace sitrk;

// Bounds in DESIGN.md section 3.6.  Everything lives in h->scratch, which the stepping never reads.  Stage 1 leaves, in input
// order, nn (nearest other valid buoy with Haversine < rd_km, else -1) and dmin.
struct OverlapScratch {
    int32_t *nn = nullptr, *flag = nullptr, *pos = nullptr, *cidx = nullptr, *cnn = nullptr;
    double *dmin = nullptr;
    char *scan_tmp = nullptr;
    size_t scan_bytes = 0;
    unsigned long long *red = nullptr;
};

static int overlap_stage1(sitrk_ctx *h, const char *fn, int64_t n, const double *lat, const double *lon, const int8_t *valid,
                          double rd_km, OverlapScratch &o)
{
    HIPCHK(hipSetDevice(h->device));
    const size_t un = (size_t)n;
    const hipStream_t st = h->stream;
    const int64_t max_cells = n + 1024;                 // the grid is known after the bounding box: size for the largest allowed
    size_t b_sort = 0;
    HIPCHK(sort_pairs_u32(nullptr, &b_sort, nullptr, nullptr, nullptr, nullptr, un, 32, st));
    HIPCHK(rocprim::exclusive_scan(nullptr, o.scan_bytes, o.flag, o.pos, 0, un, rocprim::plus<int32_t>(), st));
    o.scan_bytes = align256(o.scan_bytes);
    double *d_lat, *d_lon; int8_t *d_valid; uint32_t *k0, *k1; int32_t *v0, *perm, *cstart, *cend; V3 *uv_s; ll *ll_s;
    char *sort_tmp;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_lat, un); c.take(d_lon, un); c.take(o.dmin, un);
        c.take(d_valid, un);
        c.take(k0, un); c.take(k1, un);
        c.take(v0, un); c.take(perm, un);
        c.take(o.nn, un); c.take(o.flag, un); c.take(o.pos, un);
        c.take(o.cidx, un); c.take(o.cnn, un);
        c.take(uv_s, un); c.take(ll_s, un);
        c.take(cstart, max_cells); c.take(cend, max_cells);
        c.take(sort_tmp, b_sort); c.take(o.scan_tmp, o.scan_bytes);
        c.take(o.red, 8);          // [0..5] bbox keys, [6] first non-finite valid index, [7] valid count (one 256-byte block)
    }));

    HIPCHK(upload(h, d_lat, lat, un));
    HIPCHK(upload(h, d_lon, lon, un));
    if (valid) HIPCHK(upload(h, d_valid, valid, un));
    const int8_t *dv = valid ? d_valid : nullptr;
    hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, st, o.red);
    hipLaunchKernelGGL(unit_bbox_kernel, dim3(std::min(nblk(n), 2048u)), dim3(kOvThreads), 0, st, n, d_lat, d_lon, dv, o.red);
    HIPCHK(hipGetLastError());
    unsigned long long bb[8];
    HIPCHK(download(h, bb, o.red, 8));
    HIPCHK(hipStreamSynchronize(st));
    if (bb[6] != ~0ull) return fail(h, SITRK_EINVAL, "%s: non-finite coordinate of valid buoy at index %llu", fn, bb[6]);
    OvGrid g;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (bb[7]) {
        for (int c = 0; c < 3; c++) { lo[c] = order_value(bb[c]); hi[c] = order_value(bb[3 + c]); }
    }
    g.x0 = lo[0]; g.y0 = lo[1]; g.z0 = lo[2];
    // chord of rd (rd <= 9999 km: half-angle <= 0.79 rad, sin increasing); side h >= that chord, padded so that neither the
    // rounding of the Haversine (~1e-15 relative) nor that of the unit vectors (~1e-16) nor that of a cell coordinate
    // ((v - v0) * inv_h, < 2^20) can put a pair with Haversine < rd two cells apart
    const double chord = 2.0 * std::sin(rd_km / (2.0 * 6360.0));
    const double cut = chord * (1.0 + 1.0 / 1024.0) + 1e-12;
    int64_t ncell[3] = {1, 1, 1};
    if (!fit_cell_grid(3, lo, hi, cut, max_cells, &g.inv_h, ncell)) return fail(h, SITRK_EINVAL, "%s: no cell grid fits the cloud's extent", fn);
    g.nx = (int)ncell[0]; g.ny = (int)ncell[1]; g.nz = (int)ncell[2];
    const int64_t ncells = ncell[0] * ncell[1] * ncell[2];
    g.ncells = (uint32_t)ncells;
    const unsigned end_bit = key_bits((uint64_t)ncells);    // keys 0..ncells (ncells: invalid buoys)

    hipLaunchKernelGGL(bin_key_kernel, dim3(nblk(n)), dim3(kOvThreads), 0, st, g, n, d_lat, d_lon, dv, k0, v0);
    HIPCHK(hipGetLastError());
    size_t tb = align256(b_sort);
    HIPCHK(sort_pairs_u32(sort_tmp, &tb, k0, k1, v0, perm, un, end_bit, st));
    HIPCHK(hipMemsetAsync(cstart, 0, (size_t)ncells * sizeof(*cstart), st));
    HIPCHK(hipMemsetAsync(cend, 0, (size_t)ncells * sizeof(*cend), st));
    hipLaunchKernelGGL(bin_gather_kernel, dim3(nblk(n)), dim3(kOvThreads), 0, st, g, n, d_lat, d_lon, k1, perm, uv_s, ll_s, cstart, cend);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(nearest_kernel, dim3(nblk(n)), dim3(kOvThreads), 0, st, g, n, rd_km, cut * cut, k1, perm, uv_s, ll_s, cstart,
                       cend, o.nn, o.dmin);
    HIPCHK(hipGetLastError());
    return SITRK_OK;
}

static int overlap_check(sitrk_ctx *h, const char *fn, int64_t n, const double *lat, const double *lon, double rd_km)
{
    NEED(h, "null handle");
    if (!(n >= 0 && n < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: n must be in 0..2^31-2", fn);
    if (n > 0 && !(lat && lon)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    if (!std::isfinite(rd_km) || !(rd_km > 0.0) || rd_km > 9999.0)
        return fail(h, SITRK_EINVAL, "%s: rd_km must be finite and in (0, 9999] (got %g)", fn, rd_km);
    return SITRK_OK;
}

SITRK_API int sitrk_nearest_buoy(sitrk_t *h, int64_t n, const double *lat, const double *lon, const int8_t *valid, double rd_km,
                                 int32_t *nn, double *dmin)
{
    const char *fn = "sitrk_nearest_buoy";
    RCCHK(overlap_check(h, fn, n, lat, lon, rd_km));
    if (n > 0 && !(nn && dmin)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    if (n == 0) return SITRK_OK;
    OverlapScratch o;
    RCCHK(overlap_stage1(h, fn, n, lat, lon, valid, rd_km, o));
    HIPCHK(download(h, nn, o.nn, n));
    HIPCHK(download(h, dmin, o.dmin, n));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

SITRK_API int sitrk_cancel_too_close(sitrk_t *h, int64_t n, const double *lat, const double *lon, const int8_t *valid,
                                     const int32_t *nrec_all, const int32_t *nrec_before, double rd_km, int8_t *keep, int64_t *nkeep,
                                     int64_t *nclose)
{
    const char *fn = "sitrk_cancel_too_close";
    RCCHK(overlap_check(h, fn, n, lat, lon, rd_km));
    if (!nkeep) return fail(h, SITRK_EINVAL, "%s: null nkeep", fn);
    if (n > 0 && !(nrec_all && nrec_before && keep)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    *nkeep = 0;
    if (nclose) *nclose = 0;
    if (n == 0) return SITRK_OK;
    OverlapScratch o;
    RCCHK(overlap_stage1(h, fn, n, lat, lon, valid, rd_km, o));
    // stage 2: the close set (dmin < rd) in index order, neighbours as positions in it
    size_t tb = o.scan_bytes;
    hipLaunchKernelGGL(flag_kernel, dim3(nblk(n)), dim3(kOvThreads), 0, h->stream, n, o.nn, o.flag);
    HIPCHK(rocprim::exclusive_scan(o.scan_tmp, tb, o.flag, o.pos, 0, (size_t)n, rocprim::plus<int32_t>(), h->stream));
    hipLaunchKernelGGL(close_scatter_kernel, dim3(nblk(n)), dim3(kOvThreads), 0, h->stream, n, o.nn, o.pos, o.cidx, o.cnn);
    HIPCHK(hipGetLastError());
    int32_t last[2] = {0, 0};
    HIPCHK(download(h, &last[0], o.pos + (n - 1), 1));
    HIPCHK(download(h, &last[1], o.flag + (n - 1), 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t m = (int64_t)last[0] + last[1];
    std::vector<int32_t> cidx((size_t)m), cnn((size_t)m);
    if (m) {
        HIPCHK(download(h, cidx.data(), o.cidx, m));
        HIPCHK(download(h, cnn.data(), o.cnn, m));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    // stage 3: the reference's scan (util.py:536-556) over the close set in index order; a buoy dropped at krec loses its
    // records >= krec (zmsk[krec:,j2c] = 0), so its count becomes nrec_before; on equal counts the neighbour goes
    std::vector<uint8_t> dead((size_t)m, 0);
    for (int64_t p = 0; p < m; p++) {
        if (dead[p]) continue;
        const int32_t q = cnn[p];
        if (q < 0 || q >= m) return fail(h, SITRK_EHIP, "%s: nearest neighbour of buoy %d outside the close set", fn, cidx[p]);
        const int32_t i = cidx[p], k = cidx[q];
        const int64_t ci = nrec_all[i], ck = dead[q] ? nrec_before[k] : nrec_all[k];
        dead[ci < ck ? p : q] = 1;
    }
    int64_t nk = 0;
    for (int64_t i = 0; i < n; i++) {
        keep[i] = (valid == nullptr || valid[i] != 0) ? 1 : 0;
    }
    for (int64_t p = 0; p < m; p++)
        if (dead[p]) keep[cidx[p]] = 0;
    for (int64_t i = 0; i < n; i++) nk += keep[i];
    *nkeep = nk;
    if (nclose) *nclose = m;
    return SITRK_OK;
}
