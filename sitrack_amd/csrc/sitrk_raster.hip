// sitrk_raster.hip -- buoy cells rasterised onto a regular grid (sitrk_raster_cells, sitrk_mesh_raster): an EXTRA the reference
// does not have.  For every pixel of a regular grid in the tracker's plane the lowest-indexed drawn cell its centre lies in, and,
// for a device-resident mesh, the five values of that cell: the deformation map of a mesh without its per-cell results moving
// to the host.  The contract is in include/sitrk.h and DESIGN.md 3.15: only + - * and comparisons, so every bit is pinned.
//
// Kernels, wave64, 256 lanes per workgroup, no scratch memory, LDS only for the pixel count (16 B):
//   raster_fill_kernel      one pixel per lane: INT32_MAX
//   raster_cells_kernel<NV,SRC,COUNT>   one cell per lane: its indices (one dwordx4 for NV = 4) and NV 16-byte gathers (SRC = 0),
//                           or the mesh's contiguous 64-byte t0 block (SRC = 1); the draw / status byte, the drawable test, the
//                           cell's bounding box mapped to a pixel range, widened by one pixel each way, checked and clipped; two
//                           nested loops over that range whose trip counts are fixed before they start.  A centre that passes
//                           the NV edge tests issues one integer atomicMin without a return value.  (Reading the pixel first and
//                           skipping the atomic where a lower index is already there was measured and dropped: the cells of a mesh
//                           do not overlap, every owned pixel has one claimant, and the read cost 9-27 % of the kernel on fine
//                           rasters: DESIGN.md 3.15.)  COUNT: the measurement build behind the knob raster_count, which also
//                           sums the centres that passed -- the atomics issued -- over each wave, one integer atomic per wave
//   raster_gather_kernel    one pixel per lane and trip, at most 2048 workgroups whose lanes step a grid at a time, a later launch
//                           on the same stream (so the atomics need no fence inside a kernel): INT32_MAX -> -1, the five values
//                           of the owner from the device's `out` or SITRK_FILL, the owned pixels counted by ballot with one
//                           integer atomic per workgroup
// Every loop is bounded by a count read before it starts, no lane waits for another, vector stores only, no floating-point
// atomics: a pixel ends as the minimum over a set that the launch fixes, whichever lane gets there first.
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_cellmath.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kRasThreads = 256;
constexpr int64_t kRasMaxPixels = (int64_t)1 << 28;
constexpr int kRasMaxSide = 32768;                 // of a raster that is labelled, kept or thinned (check_raster_shape)
constexpr int32_t kRasNone = INT32_MAX;
constexpr unsigned kRasGatherBlocks = 2048;        // 256 CUs x 8 resident workgroups

__global__ __launch_bounds__(kRasThreads) void raster_fill_kernel(int64_t npix, int32_t *__restrict__ owner)
{
    const int64_t p = (int64_t)blockIdx.x * kRasThreads + threadIdx.x;
    if (p < npix) owner[p] = kRasNone;
}

// centre of pixel k along an axis that starts at o: one rounded product and one rounded sum
__device__ __forceinline__ double centre(double o, int k, double d) { return o + ((double)k + 0.5) * d; }

// The pixels k of 0..n-1 whose centre can lie in [lo, hi]: *first and the count returned.  The box [lo, hi] maps to the index
// range ceil(f(lo)) .. floor(f(hi)) with f(c) = (c - o)/d - 0.5, which is widened by one pixel each way.  centre() never falls as
// k rises, so the range is complete if the centre of the pixel in front of it lies below lo (or it starts at 0) and that of the
// pixel behind it above hi (or it ends at n-1).  That holds unless the grid's origin is so large against d that a pixel of margin
// does not cover the rounding of centre(); then the whole axis is taken: the box is a shortcut, never the result.
__device__ __forceinline__ int pixel_range(double lo, double hi, double o, double d, int n, int *first)
{
    const double top = (double)(n - 1);
    double f0 = ceil((lo - o) / d - 0.5) - 1.0, f1 = floor((hi - o) / d - 0.5) + 1.0;
    f0 = f0 < 0.0 ? 0.0 : f0;                                          // the operands are finite or infinite, never NaN
    f1 = f1 > top ? top : f1;
    if (f0 > f1) { *first = 0; return 0; }
    int k0 = (int)f0, k1 = (int)f1;
    const bool below = k0 == 0 || centre(o, k0 - 1, d) < lo, above = k1 == n - 1 || centre(o, k1 + 1, d) > hi;
    if (!(below && above)) { k0 = 0; k1 = n - 1; }
    *first = k0;
    return k1 - k0 + 1;
}

template <int NV, int SRC, bool COUNT>
__global__ __launch_bounds__(kRasThreads) void raster_cells_kernel(int64_t nC, int64_t nP, const int32_t *__restrict__ cells,
                                                                   const pt *__restrict__ pts, const int8_t *__restrict__ flag,
                                                                   bool only_status1, RasterGrid g, int32_t *owner,
                                                                   unsigned long long *__restrict__ cnt)
{
    const int64_t c0 = (int64_t)blockIdx.x * kRasThreads + threadIdx.x;
    const bool live = c0 < nC;                                         // a lane behind the last cell reads the last cell and draws nothing
    const int64_t c = live ? c0 : nC - 1;
    bool drawn = live;
    pt a[NV];
    if (SRC == 0) {
        int32_t idx[NV];
        if (NV == 4) {
            const int4 q = ((const int4 *)cells)[c];
            idx[0] = q.x; idx[1] = q.y; idx[2] = q.z; idx[NV - 1] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < NV; k++) idx[k] = cells[c * NV + k];
        }
        bool in_range = true;
#pragma unroll
        for (int k = 0; k < NV; k++) in_range = in_range && (uint64_t)(int64_t)idx[k] < (uint64_t)nP;
        if (!in_range) {
            if (live) atomicAdd(cnt, 1ull);
            drawn = false;
#pragma unroll
            for (int k = 0; k < NV; k++) idx[k] = 0;                  // point 0 stands in: the offending index is never dereferenced
        }
#pragma unroll
        for (int k = 0; k < NV; k++) a[k] = pts[idx[k]];
    } else {
#pragma unroll
        for (int k = 0; k < NV; k++) a[k] = pts[NV * c + k];
    }
    if (flag != nullptr) {                                             // wave-uniform
        const int8_t f = flag[c];
        drawn = drawn && (only_status1 ? f == 1 : f != 0);
    }

    // DRAWABLE: the shoelace sum of the sitrk_deform_cells contract, relative to vertex 0
    double dx[NV], dy[NV], ex[NV], ey[NV];
    double ymin = a[0].y, ymax = a[0].y, xmin = a[0].x, xmax = a[0].x;
#pragma unroll
    for (int k = 0; k < NV; k++) {
        drawn = drawn && finite64(a[k].y) && finite64(a[k].x);
        dx[k] = a[k].x - a[0].x; dy[k] = a[k].y - a[0].y;
        const int q = (k + 1) % NV;
        ex[k] = a[q].x - a[k].x; ey[k] = a[q].y - a[k].y;
        ymin = a[k].y < ymin ? a[k].y : ymin; ymax = a[k].y > ymax ? a[k].y : ymax;
        xmin = a[k].x < xmin ? a[k].x : xmin; xmax = a[k].x > xmax ? a[k].x : xmax;
    }
    double A2 = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int q = (k + 1) % NV;
        A2 = A2 + (dx[k] * dy[q] - dx[q] * dy[k]);
    }
    drawn = drawn && A2 != 0.0 && finite64(A2);
    const bool ccw = A2 > 0.0;

    int jlo = 0, ilo = 0, nj = 0, ni = 0;
    if (drawn) {
        nj = pixel_range(ymin, ymax, g.y0, g.d, g.ny, &jlo);
        ni = pixel_range(xmin, xmax, g.x0, g.d, g.nx, &ilo);
    }
    const int32_t cell = (int32_t)c;
    unsigned n_in = 0;
    for (int jj = 0; jj < nj; jj++) {
        const int j = jlo + jj;
        const double cy = centre(g.y0, j, g.d);
        for (int ii = 0; ii < ni; ii++) {
            const int i = ilo + ii;
            const double cx = centre(g.x0, i, g.d);
            bool in = true;
#pragma unroll
            for (int k = 0; k < NV; k++) {
                const double o = ex[k] * (cy - a[k].y) - ey[k] * (cx - a[k].x);
                in = in && (ccw ? o >= 0.0 : o <= 0.0);               // s*o >= 0 with s = +-1; a NaN is outside either way
            }
            if (in) {
                atomicMin(owner + ((int64_t)j * g.nx + i), cell);
                if (COUNT) n_in++;
            }
        }
    }
    if (COUNT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_in += __shfl_xor(n_in, o);
        if ((threadIdx.x & 63) == 0 && n_in) atomicAdd(cnt + 2, (unsigned long long)n_in);
    }
}

__global__ __launch_bounds__(kRasThreads) void raster_gather_kernel(int64_t npix, int trips, int64_t nQ, int32_t *__restrict__ owner,
                                                                    const double *__restrict__ out, double *__restrict__ fields,
                                                                    unsigned long long *__restrict__ cnt)
{
    __shared__ int sm[kRasThreads / 64];
    const int64_t stride = (int64_t)gridDim.x * kRasThreads;
    int64_t p = (int64_t)blockIdx.x * kRasThreads + threadIdx.x;
    int n = 0;                                                         // owned pixels of this wave: the same in all its lanes
    for (int t = 0; t < trips; t++, p += stride) {
        bool owned = false;
        if (p < npix) {
            const int32_t v = owner[p];
            owned = v != kRasNone;
            if (!owned) owner[p] = -1;
            if (fields != nullptr) {                                   // wave-uniform
                const double fill = SITRK_FILL;
#pragma unroll
                for (int k = 0; k < 5; k++) fields[k * npix + p] = owned ? out[k * nQ + v] : fill;
            }
        }
        n += __popcll(__ballot(owned));
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = sm[0];
#pragma unroll
        for (int w = 1; w < kRasThreads / 64; w++) m += sm[w];
        if (m) atomicAdd(cnt + 1, (unsigned long long)m);
    }
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kRasThreads - 1) / kRasThreads); }

template <int NV, int SRC>
void launch_cells(sitrk_ctx *h, const RasterJob &j, const RasterGrid &g)
{
    if (h->raster_count)
        hipLaunchKernelGGL((raster_cells_kernel<NV, SRC, true>), dim3(nblk(j.nC)), dim3(kRasThreads), 0, h->stream, j.nC, j.nP, j.cells, j.pts,
                           j.flag, j.only_status1, g, j.owner, j.cnt);
    else
        hipLaunchKernelGGL((raster_cells_kernel<NV, SRC, false>), dim3(nblk(j.nC)), dim3(kRasThreads), 0, h->stream, j.nC, j.nP, j.cells, j.pts,
                           j.flag, j.only_status1, g, j.owner, j.cnt);
}

// the counters, behind the downloads of the results on the same stream; synchronises
int raster_finish(sitrk_ctx *h, const unsigned long long *d_cnt, unsigned long long (&cnt)[3], int64_t *nowned)
{
    HIPCHK(download(h, cnt, d_cnt, 3));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->raster_count) {
        h->raster_counted = true;
        h->raster_claims = cnt[2];
    }
    if (nowned) *nowned = (int64_t)cnt[1];
    return SITRK_OK;
}

}  // namespace

int raster_run(sitrk_ctx *h, const RasterJob &j, const RasterGrid &g)
{
    const int64_t npix = (int64_t)g.ny * g.nx;
    RCCHK(h->raster_timer.begin(h));
    h->raster_counted = false;
    HIPCHK(hipMemsetAsync(j.cnt, 0, 3 * sizeof(unsigned long long), h->stream));
    RCCHK(h->raster_timer.mark(h, 0));
    hipLaunchKernelGGL(raster_fill_kernel, dim3(nblk(npix)), dim3(kRasThreads), 0, h->stream, npix, j.owner);
    HIPCHK(hipGetLastError());
    if (j.nC > 0) {
        if (j.block) launch_cells<4, 1>(h, j, g);
        else if (j.nv == 3) launch_cells<3, 0>(h, j, g);
        else launch_cells<4, 0>(h, j, g);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->raster_timer.mark(h, 1));
    // at most kRasGatherBlocks workgroups, each lane `trips` pixels a grid apart: the atomics on the one counter serialise at the
    // memory side, and one per 256 pixels took longer than the pixels themselves (profiles/raster_bench.md)
    const Strided gs(npix, kRasThreads, kRasGatherBlocks);
    hipLaunchKernelGGL(raster_gather_kernel, dim3(gs.blocks), dim3(kRasThreads), 0, h->stream, npix, gs.trips, j.nC, j.owner, j.out, j.fields,
                       j.cnt);
    HIPCHK(hipGetLastError());
    RCCHK(h->raster_timer.mark(h, 2));
    h->raster_timer.done();
    return SITRK_OK;
}

int raster_check_grid(sitrk_ctx *h, const char *fn, double y0, double x0, double d, int ny, int nx)
{
    if (!std::isfinite(y0) || !std::isfinite(x0)) return fail(h, SITRK_EINVAL, "%s: y0_km and x0_km must be finite (got %g, %g)", fn, y0, x0);
    if (!std::isfinite(d) || !(d > 0.0)) return fail(h, SITRK_EINVAL, "%s: d_km must be finite and > 0 (got %g)", fn, d);
    if (ny < 1 || nx < 1) return fail(h, SITRK_EINVAL, "%s: ny and nx must be >= 1 (got %d, %d)", fn, ny, nx);
    if ((int64_t)ny * nx > kRasMaxPixels) return fail(h, SITRK_EINVAL, "%s: ny*nx = %lld exceeds 2^28 pixels", fn, (long long)ny * nx);
    return SITRK_OK;
}

int check_raster_shape(sitrk_ctx *h, const char *fn, int ny, int nx)
{
    if (ny < 1 || nx < 1 || ny > kRasMaxSide || nx > kRasMaxSide)
        return fail(h, SITRK_EINVAL, "%s: ny and nx must be in 1..%d (got %d, %d)", fn, kRasMaxSide, ny, nx);
    if ((int64_t)ny * nx > kRasMaxPixels) return fail(h, SITRK_EINVAL, "%s: ny*nx = %lld exceeds 2^28 pixels", fn, (long long)ny * nx);
    return SITRK_OK;
}

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_raster_cells(sitrk_t *h, int64_t nP, const double *yx, int64_t nC, int nv, const int32_t *cells, const int8_t *draw,
                                 double y0_km, double x0_km, double d_km, int ny, int nx, int32_t *owner, int64_t *nowned)
{
    const char *fn = "sitrk_raster_cells";
    NEED(h, "null handle");
    if (nv != 3 && nv != 4) return fail(h, SITRK_EINVAL, "%s: nv must be 3 (triangles) or 4 (quadrangles), got %d", fn, nv);
    if (!(nC >= 0 && nC < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nC must be in 0..2^31-2", fn);
    if (!(nP >= 0 && nP < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nP must be in 0..2^31-2", fn);
    RCCHK(raster_check_grid(h, fn, y0_km, x0_km, d_km, ny, nx));
    if (!owner || (nC > 0 && !cells) || (nP > 0 && !yx)) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    if (nowned) *nowned = 0;
    if (nC > 0 && nP == 0) return fail(h, SITRK_EINDEX, "%s: %lld cell(s) have a vertex index outside [0, 0)", fn, (long long)nC);
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)ny * nx;
    pt *d_pts; int32_t *d_cells, *d_owner; int8_t *d_draw; unsigned long long *d_cnt;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_pts, nP); c.take(d_cells, (size_t)nC * nv); c.take(d_draw, draw ? (size_t)nC : 0); c.take(d_owner, npix); c.take(d_cnt, 3);
    }));
    if (nC > 0) {
        HIPCHK(upload(h, d_pts, yx, nP));
        HIPCHK(upload(h, d_cells, cells, (size_t)nC * nv));
        if (draw) HIPCHK(upload(h, d_draw, draw, nC));
    }
    RasterJob j;
    j.nC = nC; j.nP = nP; j.nv = nv; j.cells = d_cells; j.pts = d_pts; j.flag = draw ? d_draw : nullptr;
    j.owner = d_owner; j.cnt = d_cnt;
    const RasterGrid g = {y0_km, x0_km, d_km, ny, nx};
    RCCHK(raster_run(h, j, g));
    HIPCHK(download(h, owner, d_owner, (size_t)npix));
    unsigned long long cnt[3];
    RCCHK(raster_finish(h, d_cnt, cnt, nullptr));
    if (cnt[0]) return fail(h, SITRK_EINDEX, "%s: %llu cell(s) have a vertex index outside [0, %lld)", fn, cnt[0], (long long)nP);
    if (nowned) *nowned = (int64_t)cnt[1];
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_raster(sitrk_t *h, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny, int nx,
                                int32_t *owner, double *fields, int64_t *nowned)
{
    const char *fn = "sitrk_mesh_raster";
    NEED(h, "null handle");
    RCCHK(mesh_deform_check(h, fn, mesh, jrec1));
    if (at_t1 != 0 && at_t1 != 1) return fail(h, SITRK_EINVAL, "%s: at_t1 must be 0 (t0 positions) or 1 (current positions), got %d", fn, at_t1);
    RCCHK(raster_check_grid(h, fn, y0_km, x0_km, d_km, ny, nx));
    if (!owner && !fields) return fail(h, SITRK_EINVAL, "%s: owner and fields are both null", fn);
    if (nowned) *nowned = 0;
    const int64_t npix = (int64_t)ny * nx;
    int32_t *d_owner; double *d_fields; unsigned long long *d_cnt;
    auto layout = [&](Carver &c) { c.take(d_owner, npix); c.take(d_fields, fields ? (size_t)5 * npix : 0); c.take(d_cnt, 3); };
    MeshDeformDev m;
    RCCHK(carve_behind_mesh(h, mesh, jrec1, fields != nullptr, true, false, layout, &m));
    RasterJob j;
    j.nC = m.nQ; j.nP = h->nP; j.nv = 4; j.flag = m.status; j.out = m.out; j.owner = d_owner; j.fields = fields ? d_fields : nullptr; j.cnt = d_cnt;
    if (at_t1) { j.cells = m.quads; j.pts = m.p1; j.only_status1 = true; }
    else { j.block = true; j.pts = m.t0; }
    const RasterGrid g = {y0_km, x0_km, d_km, ny, nx};
    RCCHK(raster_run(h, j, g));
    if (owner) HIPCHK(download(h, owner, d_owner, (size_t)npix));
    if (fields) HIPCHK(download(h, fields, d_fields, (size_t)5 * npix));
    unsigned long long cnt[3];
    RCCHK(raster_finish(h, d_cnt, cnt, nowned));
    if (cnt[0]) return fail(h, SITRK_EINDEX, "%s: %llu cell(s) of the mesh have a vertex index outside [0, %lld)", fn, cnt[0], (long long)h->nP);
    return SITRK_OK;
}

SITRK_API int sitrk_raster_kernel_ms(sitrk_t *h, float *cells_ms, float *gather_ms)
{
    NEED(h, "null handle");
    NEED(h->raster_timer.complete, "sitrk_raster_kernel_ms: no raster call has run its kernels yet");
    RCCHK(h->raster_timer.elapsed(h, 0, cells_ms));
    return h->raster_timer.elapsed(h, 1, gather_ms);
}

SITRK_API int sitrk_raster_stats(sitrk_t *h, int64_t *claims)
{
    NEED(h, "null handle");
    NEED(h->raster_counted, "sitrk_raster_stats: no raster call has run with the knob raster_count set");
    if (claims) *claims = (int64_t)h->raster_claims;
    return SITRK_OK;
}
