// sitrk_subsample.hip -- seed-cloud coarsening (sitrk_subsample_cloud): the greedy sparsification of the reference's
// util.SubSampCloud (gudhi.subsampling.sparsify_point_set).  Point i is kept iff no kept j < i has d2(i,j) < r2, i.e.
// the lexicographically-first maximal independent set of the graph with edges where d2 < r2.  Kept in its own
// translation unit so that the device code of sitrk.hip stays as it is.
//
// Steps (driven by sitrk_subsample_cloud() at the end of this file):
//   1. bbox_kernel      bounding box of the cloud and the first non-finite coordinate
//   2. bin_key_kernel   square cells of side h >= rd (padded); key = cell, value = index; the rocPRIM radix sort of
//                       sitrk_sort.hip orders the points by cell, stably, so each cell holds its points in index order
//   3. bin_gather_kernel sorted coordinates and the [start,end) range of every cell
//   4. resolve_kernel   the greedy result in rounds over a state array (undecided -> kept | dropped), see below
//   5. emit_kernel      keep mask in input order and the kept count
//
// All state lives in sorted position order.  Every decision is final and correct on its own:
//   - a point is dropped only when it sees a KEPT earlier neighbour (kept states are correct by induction);
//   - a point is kept only when it has seen every earlier neighbour DROPPED;
//   - a point that becomes kept marks its later neighbours dropped at once ("push"), cooperatively by its workgroup.
// So the result is the unique greedy set whatever the dispatch order, timing or placement.  A workgroup re-sweeps its
// own undecided points while it makes progress (at most kMaxSweeps times); what it reads of other workgroups' states
// is a hint (a stale "undecided" only delays a decision).  No workgroup ever waits for another.  The lowest-index
// undecided point at a launch's start has all its earlier neighbours decided and visible (kernel boundary), so its
// workgroup decides it in its first sweep: every launch decides at least one point.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_bins.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kSubThreads = 256;      // threads per workgroup of every kernel here
constexpr int kMaxSweeps = 256;       // bound of the in-launch re-sweeps of one workgroup
constexpr uint8_t kUndecided = 0, kKept = 1, kDropped = 2;

__device__ __forceinline__ uint8_t state_load(const uint8_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void state_store(uint8_t *p, uint8_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the contract's distance: two rounded products, one rounded sum, no FMA (contract(off) above and -ffp-contract=off)
__device__ __forceinline__ double d2of(pt a, pt b)
{
    const double dy = a.y - b.y, dx = a.x - b.x;
    const double yy = dy * dy, xx = dx * dx;
    return yy + xx;
}

__global__ void bbox_init_kernel(unsigned long long *red)
{
    if (threadIdx.x < 5) red[threadIdx.x] = threadIdx.x < 2 || threadIdx.x == 4 ? ~0ull : 0ull;
}

// red[0..3] = keys of ymin, xmin, ymax, xmax (finite points); red[4] = first non-finite index (all-ones: none)
__global__ __launch_bounds__(kSubThreads) void bbox_kernel(int64_t n, const pt *__restrict__ yx, unsigned long long *red)
{
    unsigned long long lo_y = ~0ull, lo_x = ~0ull, hi_y = 0, hi_x = 0, bad = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * kSubThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSubThreads) {
        const pt p = yx[i];
        if (!isfinite(p.y) || !isfinite(p.x)) {
            bad = min(bad, (unsigned long long)i);
            continue;
        }
        const unsigned long long ky = order_key(p.y), kx = order_key(p.x);
        lo_y = min(lo_y, ky); hi_y = max(hi_y, ky);
        lo_x = min(lo_x, kx); hi_x = max(hi_x, kx);
    }
    __shared__ unsigned long long sm[5][kSubThreads];
    sm[0][threadIdx.x] = lo_y; sm[1][threadIdx.x] = lo_x; sm[2][threadIdx.x] = hi_y; sm[3][threadIdx.x] = hi_x;
    sm[4][threadIdx.x] = bad;
    __syncthreads();
    block_reduce<kSubThreads, Red::Min, Red::Min, Red::Max, Red::Max, Red::Min>(sm);
    if (threadIdx.x == 0) {
        atomicMin(&red[0], sm[0][0]); atomicMin(&red[1], sm[1][0]);
        atomicMax(&red[2], sm[2][0]); atomicMax(&red[3], sm[3][0]);
        atomicMin(&red[4], sm[4][0]);
    }
}

__global__ __launch_bounds__(kSubThreads) void bin_key_kernel(SubGrid g, int64_t n, const pt *__restrict__ yx, uint32_t *key,
                                                             int32_t *val)
{
    const int64_t i = (int64_t)blockIdx.x * kSubThreads + threadIdx.x;
    if (i >= n) return;
    const pt p = yx[i];
    const int cy = cell_coord(p.y, g.ymin, g.inv_h, g.ny), cx = cell_coord(p.x, g.xmin, g.inv_h, g.nx);
    key[i] = (uint32_t)cy * (uint32_t)g.nx + (uint32_t)cx;
    val[i] = (int32_t)i;
}

__global__ __launch_bounds__(kSubThreads) void bin_gather_kernel(int64_t n, const pt *__restrict__ yx, const uint32_t *__restrict__ key,
                                                                const int32_t *__restrict__ perm, pt *yx_s, int32_t *cstart,
                                                                int32_t *cend)
{
    const int64_t s = (int64_t)blockIdx.x * kSubThreads + threadIdx.x;
    if (s >= n) return;
    yx_s[s] = yx[perm[s]];
    mark_cell_run(key, s, n, cstart, cend);
}

// Pull: walk the earlier neighbours of sorted point p from its cursor (cell slot 0..8 of the 3x3 neighbourhood, sorted
// position inside that cell).  The cursor only ever moves past non-neighbours and DROPPED neighbours, which are final,
// so a point blocked behind an undecided neighbour costs one re-check per sweep.  Returns the decision (or kUndecided).
__device__ uint8_t pull(const SubResolveArgs &a, int32_t p)
{
    const pt P = a.yx[p];
    const int32_t me = a.perm[p];
    const int cy = cell_coord(P.y, a.g.ymin, a.g.inv_h, a.g.ny), cx = cell_coord(P.x, a.g.xmin, a.g.inv_h, a.g.nx);
    int k = a.cur_k[p];
    int32_t q = a.cur_q[p];
    for (; k < 9; k++, q = -1) {
        const int yy = cy + k / 3 - 1, xx = cx + k % 3 - 1;
        if (yy < 0 || yy >= a.g.ny || xx < 0 || xx >= a.g.nx) continue;
        const int64_t c = (int64_t)yy * a.g.nx + xx;
        const int32_t e = a.cend[c];
        if (q < 0) q = a.cstart[c];
        for (; q < e; q++) {
            if (a.perm[q] >= me) break;              // a cell holds its points in index order: the rest are later
            if (d2of(P, a.yx[q]) < a.r2) {
                const uint8_t st = state_load(a.state + q);
                if (st == kKept) return kDropped;
                if (st == kUndecided) {
                    a.cur_k[p] = (uint8_t)k;
                    a.cur_q[p] = q;
                    return kUndecided;
                }
            }
        }
    }
    return kKept;
}

__global__ __launch_bounds__(kSubThreads) void resolve_kernel(SubResolveArgs a)
{
    const int wg = blockIdx.x;
    if (a.done[wg]) return;                          // every point of this workgroup decided in an earlier launch
    const int64_t base = (int64_t)wg * kSubThreads * a.ppt;
    __shared__ int32_t klist[kSubThreads * kSubMaxPpt];
    __shared__ int nk, progress, nund;
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        if (threadIdx.x == 0) { nk = 0; progress = 0; }
        __syncthreads();
        for (int t = 0; t < a.ppt; t++) {
            const int64_t p = base + (int64_t)t * kSubThreads + threadIdx.x;
            if (p >= a.n || state_load(a.state + p) != kUndecided) continue;
            const uint8_t d = pull(a, (int32_t)p);
            if (d == kUndecided) continue;
            state_store(a.state + p, d);
            if (d == kKept) klist[atomicAdd(&nk, 1)] = (int32_t)p;
            progress = 1;
        }
        __syncthreads();
        // both flags are read into registers here, between the two barriers: thread 0 resets them at the top of the next
        // sweep with no barrier in between, so a read after the second barrier could see the reset and leave the loop alone
        const int nkept = nk, prog = progress;
        // push: the whole workgroup drops the later neighbours of each point it has just kept
        for (int e = 0; e < nkept; e++) {
            const int32_t p = klist[e];
            const pt P = a.yx[p];
            const int32_t me = a.perm[p];
            const int cy = cell_coord(P.y, a.g.ymin, a.g.inv_h, a.g.ny), cx = cell_coord(P.x, a.g.xmin, a.g.inv_h, a.g.nx);
            for (int k = 0; k < 9; k++) {
                const int yy = cy + k / 3 - 1, xx = cx + k % 3 - 1;
                if (yy < 0 || yy >= a.g.ny || xx < 0 || xx >= a.g.nx) continue;
                const int64_t c = (int64_t)yy * a.g.nx + xx;
                const int32_t e1 = a.cend[c];
                for (int32_t q = a.cstart[c] + (int32_t)threadIdx.x; q < e1; q += kSubThreads)
                    if (a.perm[q] > me && d2of(P, a.yx[q]) < a.r2 && state_load(a.state + q) == kUndecided)
                        state_store(a.state + q, kDropped);
            }
        }
        __syncthreads();
        if (!prog) break;                            // uniform: every thread read the same value before the barrier
    }
    // what is left undecided here (an over-count at worst: another workgroup may have dropped some of these meanwhile)
    if (threadIdx.x == 0) nund = 0;
    __syncthreads();
    int mine = 0;
    for (int t = 0; t < a.ppt; t++) {
        const int64_t p = base + (int64_t)t * kSubThreads + threadIdx.x;
        if (p < a.n && state_load(a.state + p) == kUndecided) mine++;
    }
    if (mine) atomicAdd(&nund, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (nund == 0) a.done[wg] = 1;
        if (a.undecided && nund) atomicAdd(a.undecided, (unsigned long long)nund);
    }
}

__global__ __launch_bounds__(kSubThreads) void emit_kernel(int64_t n, const int32_t *__restrict__ perm, const uint8_t *__restrict__ state,
                                                          int8_t *keep, unsigned long long *nkeep)
{
    const int64_t s = (int64_t)blockIdx.x * kSubThreads + threadIdx.x;
    const int kept = s < n && state[s] == kKept;
    if (s < n) keep[perm[s]] = (int8_t)kept;
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    if (kept) atomicAdd(&cnt, 1);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(nkeep, (unsigned long long)cnt);
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kSubThreads - 1) / kSubThreads); }

}  // namespace

bool fit_cell_grid(int dims, const double *lo, const double *hi, double side, int64_t max_cells, double *inv_h, int64_t *ncell)
{
    for (int it = 0; it < 2100; it++, side *= 2.0) {
        *inv_h = 1.0 / side;
        bool ok = true;
        int64_t cells = 1;
        for (int c = 0; c < dims && ok; c++) {
            const double t = (hi[c] - lo[c]) * *inv_h;
            if (!(t < 1048576.0)) ok = false;
            else cells *= (ncell[c] = (int64_t)std::floor(t) + 1);
        }
        if (ok && cells <= max_cells) return *inv_h > 0.0;
    }
    return false;
}

}  // namespace sitrk

using namespace sitrk;

// Everything lives in h->scratch, which the stepping never reads.
SITRK_API int sitrk_subsample_cloud(sitrk_t *h, int64_t n, const double *yx, double rd_km, int8_t *keep, int64_t *nkeep,
                                    int32_t *launches)
{
    NEED(h, "null handle");
    NEED(n >= 0 && n < ((int64_t)1 << 31) - 1, "sitrk_subsample_cloud: n must be in 0..2^31-2");
    NEED(nkeep, "sitrk_subsample_cloud: null nkeep");
    NEED(n == 0 || (yx && keep), "sitrk_subsample_cloud: null array");
    if (!std::isfinite(rd_km) || !(rd_km > 0.0))
        return fail(h, SITRK_EINVAL, "sitrk_subsample_cloud: rd_km must be finite and > 0 (got %g)", rd_km);
    *nkeep = 0;
    if (launches) *launches = 0;
    if (n == 0) return SITRK_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t un = (size_t)n;
    // the cell grid is known after the bounding box; size the scratch for the largest grid allowed (cells <= n + 1024)
    const int64_t max_cells = n + 1024;
    size_t b_sort = 0;
    HIPCHK(sort_pairs_u32(nullptr, &b_sort, nullptr, nullptr, nullptr, nullptr, un, 32, h->stream));
    const hipStream_t st = h->stream;
    const int64_t nwg = (n + h->subsample_block - 1) / h->subsample_block;
    pt *d_yx, *d_yxs; uint32_t *k0, *k1; int32_t *v0, *perm, *cur_q, *cstart, *cend; uint8_t *state, *cur_k, *done;
    int8_t *d_keep; char *sort_tmp; unsigned long long *red;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_yx, un); c.take(d_yxs, un);
        c.take(k0, un); c.take(k1, un);
        c.take(v0, un); c.take(perm, un); c.take(cur_q, un);
        c.take(state, un); c.take(cur_k, un); c.take(d_keep, un);
        c.take(cstart, max_cells); c.take(cend, max_cells);
        c.take(sort_tmp, b_sort);
        c.take(red, 7);            // [0..4] bbox + first non-finite, [5] undecided, [6] kept (one 256-byte block)
        c.take(done, nwg);
    }));

    HIPCHK(upload(h, d_yx, yx, un));
    hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, st, red);
    hipLaunchKernelGGL(bbox_kernel, dim3(std::min(nblk(n), 2048u)), dim3(kSubThreads), 0, st, n, d_yx, red);
    HIPCHK(hipGetLastError());
    unsigned long long bb[5];
    HIPCHK(download(h, bb, red, 5));
    HIPCHK(hipStreamSynchronize(st));
    if (bb[4] != ~0ull)
        return fail(h, SITRK_EINVAL, "sitrk_subsample_cloud: non-finite coordinate at index %llu", bb[4]);
    const double lo[2] = {order_value(bb[0]), order_value(bb[1])};
    const double hi[2] = {order_value(bb[2]), order_value(bb[3])};
    // side h >= rd, padded so that the rounding of a cell coordinate ((v - v0) * inv_h, <= 2^20) can never put a pair with
    // d2 < r2 two cells apart
    SubGrid g;
    g.ymin = lo[0]; g.xmin = lo[1];
    int64_t ncell[2] = {1, 1};
    if (!fit_cell_grid(2, lo, hi, rd_km * (1.0 + 1.0 / 1024.0), max_cells, &g.inv_h, ncell))
        return fail(h, SITRK_EINVAL, "sitrk_subsample_cloud: no cell grid fits the cloud's extent");
    g.ny = (int)ncell[0]; g.nx = (int)ncell[1];
    const int64_t ncells = ncell[0] * ncell[1];
    const unsigned end_bit = key_bits((uint64_t)ncells - 1);

    // bin: key = cell, stable radix sort (index order inside a cell), sorted coordinates, cell ranges
    hipLaunchKernelGGL(bin_key_kernel, dim3(nblk(n)), dim3(kSubThreads), 0, st, g, n, d_yx, k0, v0);
    HIPCHK(hipGetLastError());
    size_t tb = align256(b_sort);
    HIPCHK(sort_pairs_u32(sort_tmp, &tb, k0, k1, v0, perm, un, end_bit, st));
    HIPCHK(hipMemsetAsync(cstart, 0, (size_t)ncells * sizeof(*cstart), st));
    HIPCHK(hipMemsetAsync(cend, 0, (size_t)ncells * sizeof(*cend), st));
    hipLaunchKernelGGL(bin_gather_kernel, dim3(nblk(n)), dim3(kSubThreads), 0, st, n, d_yx, k1, perm, d_yxs, cstart, cend);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(state, 0, un, st));
    HIPCHK(hipMemsetAsync(cur_k, 0, un, st));
    HIPCHK(hipMemsetAsync(cur_q, 0xff, un * sizeof(*cur_q), st));
    HIPCHK(hipMemsetAsync(done, 0, (size_t)nwg, st));

    SubResolveArgs a;
    a.g = g; a.n = n; a.r2 = rd_km * rd_km; a.ppt = h->subsample_block / 256;
    a.yx = d_yxs; a.perm = perm; a.cstart = cstart; a.cend = cend;
    a.state = state; a.cur_q = cur_q; a.cur_k = cur_k; a.done = done;
    // launches in batches; the last launch of a batch counts what it leaves undecided (an over-count at worst, and always
    // below the previous batch's count, since every launch decides the lowest undecided point): stop at 0, give up if it stalls
    unsigned long long prev = (unsigned long long)n + 1, und = 0;
    int64_t nl = 0;
    int batch = 4;
    for (;;) {
        for (int b = 0; b < batch; b++) {
            a.undecided = nullptr;
            if (b == batch - 1) {
                HIPCHK(hipMemsetAsync(red + 5, 0, sizeof(unsigned long long), st));
                a.undecided = red + 5;
            }
            hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)nwg), dim3(kSubThreads), 0, st, a);
            HIPCHK(hipGetLastError());
        }
        nl += batch;
        HIPCHK(download(h, &und, red + 5, 1));
        HIPCHK(hipStreamSynchronize(st));
        if (und == 0) break;
        if (und >= prev || nl > n + 64)
            return fail(h, SITRK_EHIP, "sitrk_subsample_cloud: undecided count stalled at %llu after %lld launches", und, (long long)nl);
        prev = und;
        batch = std::min(2 * batch, 64);
    }
    HIPCHK(hipMemsetAsync(red + 6, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(emit_kernel, dim3(nblk(n)), dim3(kSubThreads), 0, st, n, perm, state, d_keep, red + 6);
    HIPCHK(hipGetLastError());
    unsigned long long nk = 0;
    HIPCHK(download(h, keep, d_keep, un));
    HIPCHK(download(h, &nk, red + 6, 1));
    HIPCHK(hipStreamSynchronize(st));
    *nkeep = (int64_t)nk;
    if (launches) *launches = (int32_t)std::min<int64_t>(nl, INT32_MAX);
    return SITRK_OK;
}
