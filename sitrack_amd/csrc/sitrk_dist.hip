// sitrk_dist.hip -- the distribution of a set of values (sitrk_dist_values, sitrk_mesh_dist): an EXTRA the reference does not
// have.  The counts of the values between explicit edges -- the PDF of the deformation rates -- and exact order statistics --
// the percentile a feature threshold is stated as -- of a host array or of the status-1 cells of a device-resident mesh, without
// a per-cell result moving to the host.  The contract is in include/sitrk.h and DESIGN.md 3.21: comparisons, counts and a
// selection on the bits of the values, so every number is pinned and nothing depends on the launch geometry.
//
// Kernels, wave64, no scratch memory:
//   dist_keys_values_kernel  one value per lane: its order key (sitrk_bins.h) or the marker for "not in the sample"; the sample's
//   dist_keys_mesh_kernel    size and the NaNs from ballots, summed per workgroup into one row of partials
//   dist_setup_kernel        one workgroup: sums those rows (m, nnan), forms every target's rank from m and starts its prefix
//   dist_count_kernel        capped, strided: the edges and one u32 counter per class in LDS; the class of a value by a branch-free
//                            binary search of a length fixed by the host; integer LDS atomics; one row of partials per workgroup
//   dist_hist_sum_kernel     the rows summed in int64, 16 classes a workgroup
//   dist_select_kernel       capped, strided, one pass per 8-bit digit from the top: a key that matches a target's prefix adds 1 to
//                            that target's counter of the key's digit, 256 u32 counters per target in LDS.  Targets with one
//                            prefix share the counters of the first of them.  With the knob dist_aggregate (default 0: measured
//                            no faster; never changes a result), where every matching lane of a wave has the same
//                            digit -- the rule in the top passes, rates share their sign and most of their exponent -- one lane
//                            adds the number of them
//   dist_pick_kernel         one workgroup: sums the rows, scans the 256 digits of every target, extends its prefix by the digit
//                            its rank falls in and takes the digits below off the rank; behind the last pass the prefix is the key.
//                            Prefix, rank and group are read once in front of a barrier and stored by the one lane that extends
//                            the target: no lane reads what another stores in the same launch
// The host reads nothing between the passes.  Every loop is bounded by a count read before it starts, no lane waits for another,
// vector stores only, no floating-point atomics.
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_bins.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

typedef unsigned long long u64;

constexpr int kDistThreads = 256;                   // the key kernels, one value per lane, and the setup kernel
constexpr int kDistWide = 1024;                     // lanes of a workgroup of the capped count launches and of the pick kernel
constexpr unsigned kDistMaxBlocks = 256;            // workgroups of the capped count launches at most = rows of their partials
constexpr int kDistUnroll = 4;                      // keys a lane of those has in flight
constexpr int kDistRowLanes = 4;                    // rows the pick kernel reads side by side: kDistWide / 256
constexpr int kDistSumCols = 16, kDistSumRows = 16; // classes x rows a workgroup of the histogram's sum reads side by side
constexpr int kDistDigits = 256;
constexpr u64 kDistOut = ~0ull;                     // the key of no value of a sample: the order key of a NaN
static_assert(kDistRowLanes * kDistDigits == kDistWide, "pick kernel: one lane per (row lane, digit)");
static_assert(kDistSumCols * kDistSumRows == kDistThreads, "histogram sum: one lane per (row lane, class)");

// what comes down, int64 words: m, nnan, qval (nq, the bits of the doubles), qrank (nq), counts (nb + 2)
__host__ __device__ inline int down_qval(int) { return 2; }
__host__ __device__ inline int down_qrank(int nq) { return 2 + nq; }
__host__ __device__ inline int down_counts(int nq) { return 2 + 2 * nq; }

// the two ballots of a key kernel summed over the workgroup: row blockIdx.x of part = (in the sample, NaN)
__device__ __forceinline__ void dist_part_row(bool ok, bool isnan_, u64 *__restrict__ part)
{
    __shared__ unsigned sm[kDistThreads / 64][2];
    const unsigned a = __popcll(__ballot(ok)), b = __popcll(__ballot(isnan_));
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < kDistThreads / 64; w++) s += sm[w][threadIdx.x];
        part[(int64_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kDistThreads) void dist_keys_values_kernel(int64_t n, const double *__restrict__ x, const int8_t *__restrict__ use,
                                                                        u64 *__restrict__ keys, u64 *__restrict__ part)
{
    const int64_t i = (int64_t)blockIdx.x * kDistThreads + threadIdx.x;
    const bool live = i < n;
    const double v = live ? x[i] : 0.0;
    bool in = live;
    if (use != nullptr) in = in && use[live ? i : 0] != 0;             // wave-uniform
    const bool bad = in && v != v;
    const bool ok = in && !bad;
    if (live) keys[i] = ok ? order_key(v + 0.0) : kDistOut;
    dist_part_row(ok, bad, part);
}

// out (5,nQ) and status (nQ) of the mesh's deformation; f, -f or |f| of div, shr, vor, or t2 = div*div + shr*shr
__global__ __launch_bounds__(kDistThreads) void dist_keys_mesh_kernel(int64_t nQ, const double *__restrict__ out, const int8_t *__restrict__ status,
                                                                      int what, int sgn, u64 *__restrict__ keys, u64 *__restrict__ part)
{
    const int64_t i = (int64_t)blockIdx.x * kDistThreads + threadIdx.x;
    const bool live = i < nQ;
    const int64_t k = live ? i : 0;
    const bool in = live && status[k] == 1;
    double v;
    if (what == 3) {                                                   // wave-uniform
        const double d = out[k], s = out[nQ + k];
        const double dd = d * d, ss = s * s;
        v = dd + ss;
    } else {
        const double f = out[(int64_t)what * nQ + k];
        v = sgn > 0 ? f : sgn < 0 ? -f : fabs(f);
    }
    const bool bad = in && v != v;
    const bool ok = in && !bad;
    if (live) keys[i] = ok ? order_key(v + 0.0) : kDistOut;
    dist_part_row(ok, bad, part);
}

// state of the selection on the device: per target its prefix (the digits found so far, in place, zeros below), the rank that is
// left among the keys with that prefix (-1: an empty sample) and the first target with the same prefix
struct DistState {
    u64 *pre;
    int64_t *rnk;
    int32_t *grp;
};

__global__ __launch_bounds__(kDistThreads) void dist_setup_kernel(int64_t nrows, const u64 *__restrict__ part, int nq, const double *__restrict__ q,
                                                                  DistState st, int64_t *__restrict__ down)
{
    __shared__ u64 sm[kDistThreads / 64][2];
    u64 a = 0, b = 0;
    for (int64_t r = threadIdx.x; r < nrows; r += kDistThreads) { a += part[r * 2]; b += part[r * 2 + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    u64 m = 0, nn = 0;
#pragma unroll
    for (int w = 0; w < kDistThreads / 64; w++) { m += sm[w][0]; nn += sm[w][1]; }
    if (threadIdx.x == 0) { down[0] = (int64_t)m; down[1] = (int64_t)nn; }
    if ((int)threadIdx.x < nq) {
        const int t = threadIdx.x;
        int64_t k = -1;
        if (m > 0) {
            const double f = floor(q[t] * (double)(int64_t)m);       // one rounded product
            k = (int64_t)f;
            if (k > (int64_t)m - 1) k = (int64_t)m - 1;
        }
        st.pre[t] = 0; st.rnk[t] = k; st.grp[t] = 0;
        down[down_qrank(nq) + t] = k;
        down[down_qval(nq) + t] = (int64_t)0x7ff8000000000000ull;       // NaN until the last pass writes the value
    }
}

// keys of a lane of a capped launch: trip t of workgroup b covers (t * gridDim.x + b) * kDistWide + lane
__device__ __forceinline__ void dist_load(int64_t n, int trips, int t0, const u64 *__restrict__ keys, u64 (&k)[kDistUnroll])
{
#pragma unroll
    for (int u = 0; u < kDistUnroll; u++) {
        const int64_t i = ((int64_t)(t0 + u) * gridDim.x + blockIdx.x) * kDistWide + threadIdx.x;
        k[u] = (t0 + u < trips && i < n) ? keys[i] : kDistOut;
    }
}

// rows (gridDim.x, nb + 2) u32: the values of the workgroup's trips with exactly c of the nb + 1 edges <= v.  step0 = the largest
// power of two <= nb + 1
__global__ __launch_bounds__(kDistWide) void dist_count_kernel(int64_t n, int trips, const u64 *__restrict__ keys, int nb, int step0,
                                                               const double *__restrict__ edges, uint32_t *__restrict__ rows)
{
    __shared__ double sE[SITRK_DIST_MAXBINS + 1];
    __shared__ uint32_t sC[SITRK_DIST_MAXBINS + 2];
    const int ne = nb + 1;
    for (int c = threadIdx.x; c < ne; c += kDistWide) sE[c] = edges[c];
    for (int c = threadIdx.x; c < nb + 2; c += kDistWide) sC[c] = 0;
    __syncthreads();
    for (int t0 = 0; t0 < trips; t0 += kDistUnroll) {
        u64 k[kDistUnroll];
        dist_load(n, trips, t0, keys, k);
#pragma unroll
        for (int u = 0; u < kDistUnroll; u++) {
            if (k[u] != kDistOut) {
                const double v = order_value(k[u]);
                int lo = 0;                                            // edges known to be <= v
                for (int s = step0; s > 0; s >>= 1) {
                    const int t = lo + s;
                    const int at = (t < ne ? t : ne) - 1;
                    lo = (t <= ne && sE[at] <= v) ? t : lo;
                }
                atomicAdd(&sC[lo], 1u);
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nb + 2; c += kDistWide) rows[(int64_t)blockIdx.x * (nb + 2) + c] = sC[c];
}

__global__ __launch_bounds__(kDistThreads) void dist_hist_sum_kernel(int nrows, int nb2, const uint32_t *__restrict__ rows, int64_t *__restrict__ counts)
{
    __shared__ int64_t sm[kDistSumRows][kDistSumCols];
    const int cl = threadIdx.x % kDistSumCols, rl = threadIdx.x / kDistSumCols;
    const int c = blockIdx.x * kDistSumCols + cl;
    int64_t s = 0;
    if (c < nb2)
        for (int r = rl; r < nrows; r += kDistSumRows) s += rows[(int64_t)r * nb2 + c];
    sm[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < nb2) {
        int64_t tot = 0;
#pragma unroll
        for (int r = 0; r < kDistSumRows; r++) tot += sm[r][cl];
        counts[c] = tot;
    }
}

// rows (gridDim.x, nq, 256) u32.  shift = the digit's lowest bit; himask = the bits above the digit
__global__ __launch_bounds__(kDistWide) void dist_select_kernel(int64_t n, int trips, const u64 *__restrict__ keys, int nq, int shift, u64 himask,
                                                                int aggregate, DistState st, uint32_t *__restrict__ rows)
{
    __shared__ uint32_t sC[SITRK_DIST_MAXQ * kDistDigits];
    __shared__ u64 sPre[SITRK_DIST_MAXQ];
    __shared__ int32_t sLead[SITRK_DIST_MAXQ];
    for (int c = threadIdx.x; c < nq * kDistDigits; c += kDistWide) sC[c] = 0;
    if ((int)threadIdx.x < nq) { sPre[threadIdx.x] = st.pre[threadIdx.x]; sLead[threadIdx.x] = st.grp[threadIdx.x] == (int)threadIdx.x; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int t0 = 0; t0 < trips; t0 += kDistUnroll) {
        u64 k[kDistUnroll];
        dist_load(n, trips, t0, keys, k);
#pragma unroll
        for (int u = 0; u < kDistUnroll; u++) {
            const bool in = k[u] != kDistOut;
            const int digit = (int)((k[u] >> shift) & 255);
            for (int t = 0; t < nq; t++) {
                if (!sLead[t]) continue;                               // workgroup-uniform
                const bool match = in && ((k[u] ^ sPre[t]) & himask) == 0;
                const u64 mm = __ballot(match);
                if (mm == 0) continue;                                 // wave-uniform
                bool plain = true;
                if (aggregate) {
                    const int first = __ffsll((long long)mm) - 1;
                    const int d0 = __shfl(digit, first);
                    const u64 same = __ballot(match && digit == d0);
                    if (same == mm) {                                  // wave-uniform
                        plain = false;
                        if (lane == first) atomicAdd(&sC[t * kDistDigits + d0], (uint32_t)__popcll(mm));
                    }
                }
                if (plain && match) atomicAdd(&sC[t * kDistDigits + digit], 1u);
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nq * kDistDigits; c += kDistWide) rows[(int64_t)blockIdx.x * nq * kDistDigits + c] = sC[c];
}

__global__ __launch_bounds__(kDistWide) void dist_pick_kernel(int nrows, int nq, int shift, const uint32_t *__restrict__ rows, DistState st,
                                                              int64_t *__restrict__ down)
{
    __shared__ u64 sPart[kDistRowLanes][kDistDigits];
    __shared__ u64 sTot[SITRK_DIST_MAXQ][kDistDigits];
    __shared__ int32_t sGrp[SITRK_DIST_MAXQ];
    __shared__ u64 sNew[SITRK_DIST_MAXQ];
    __shared__ int64_t sRnk[SITRK_DIST_MAXQ];
    const int d = threadIdx.x & (kDistDigits - 1), rl = threadIdx.x / kDistDigits;
    // the state of every target is read once, here, in front of a barrier: the lane that extends a target below stores its new
    // prefix and rank to device memory while other waves of the same target may still be scanning, and none of them reads
    // device memory or sNew for it again -- what a lane decides never depends on how far another wave has got
    if ((int)threadIdx.x < nq) {
        sGrp[threadIdx.x] = st.grp[threadIdx.x]; sNew[threadIdx.x] = st.pre[threadIdx.x]; sRnk[threadIdx.x] = st.rnk[threadIdx.x];
    }
    __syncthreads();
    for (int g = 0; g < nq; g++) {                                     // the counters of every first target of a prefix
        if (sGrp[g] != g) continue;                                    // workgroup-uniform
        u64 s = 0;
        for (int r0 = rl; r0 < nrows; r0 += kDistRowLanes * kDistUnroll) {
            uint32_t a[kDistUnroll];
#pragma unroll
            for (int u = 0; u < kDistUnroll; u++) {
                const int r = r0 + u * kDistRowLanes;
                a[u] = r < nrows ? rows[((int64_t)r * nq + g) * kDistDigits + d] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kDistUnroll; u++) s += a[u];
        }
        sPart[rl][d] = s;
        __syncthreads();
        if (rl == 0) {
            u64 tot = 0;
#pragma unroll
            for (int r = 0; r < kDistRowLanes; r++) tot += sPart[r][d];
            sTot[g][d] = tot;
        }
        __syncthreads();
    }
    for (int t = rl; t < nq; t += kDistRowLanes) {                     // one run of 256 lanes per target
        const u64 *tot = sTot[sGrp[t]];
        const int64_t rank = sRnk[t];                                    // the rank this pass started with, for all four waves
        int64_t below = 0;
        for (int j = 0; j < d; j++) below += (int64_t)tot[j];
        if (below <= rank && rank < below + (int64_t)tot[d]) {           // one lane at most; none for rank -1
            const u64 p = sNew[t] | ((u64)d << shift);                 // that lane alone reads and writes sNew[t] in this loop
            sNew[t] = p;
            st.pre[t] = p;
            st.rnk[t] = rank - below;
            if (shift == 0) {
                const double v = order_value(p);
                int64_t bits;
                memcpy(&bits, &v, sizeof bits);
                down[down_qval(nq) + t] = bits;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nq) {
        const int t = threadIdx.x;
        int g = t;
        for (int j = t - 1; j >= 0; j--) g = sNew[j] == sNew[t] ? j : g;
        st.grp[t] = g;
    }
}

struct DistBuf {
    u64 *keys, *part;
    uint32_t *hrows, *srows;
    double *edges, *q;
    DistState st;
    int64_t *down;
};

void dist_carve(Carver &c, DistBuf &b, int64_t n, int nb, int nq)
{
    c.take(b.keys, n); c.take(b.part, (size_t)2 * nblk(n, kDistThreads));
    c.take(b.hrows, nb ? (size_t)kDistMaxBlocks * (nb + 2) : 0); c.take(b.srows, (size_t)kDistMaxBlocks * nq * kDistDigits);
    c.take(b.edges, nb ? nb + 1 : 0); c.take(b.q, nq);
    c.take(b.st.pre, SITRK_DIST_MAXQ); c.take(b.st.rnk, SITRK_DIST_MAXQ); c.take(b.st.grp, SITRK_DIST_MAXQ);
    c.take(b.down, 2 + 2 * SITRK_DIST_MAXQ + SITRK_DIST_MAXBINS + 2);
}

// what both entry points check before any device work
int dist_check(sitrk_ctx *h, const char *fn, int nb, const double *edges, const int64_t *counts, int nq, const double *q, const double *qval,
               const int64_t *qrank)
{
    if (nb < 0 || nb > SITRK_DIST_MAXBINS) return fail(h, SITRK_EINVAL, "%s: nb must be in 0..%d (got %d)", fn, SITRK_DIST_MAXBINS, nb);
    if (nq < 0 || nq > SITRK_DIST_MAXQ) return fail(h, SITRK_EINVAL, "%s: nq must be in 0..%d (got %d)", fn, SITRK_DIST_MAXQ, nq);
    if (nb > 0 && !(edges && counts)) return fail(h, SITRK_EINVAL, "%s: null edges or counts with nb = %d", fn, nb);
    if (nq > 0 && !(q && qval && qrank)) return fail(h, SITRK_EINVAL, "%s: null q, qval or qrank with nq = %d", fn, nq);
    for (int c = 0; nb > 0 && c <= nb; c++) {
        if (!std::isfinite(edges[c])) return fail(h, SITRK_EINVAL, "%s: edges[%d] is not finite", fn, c);
        if (c > 0 && !(edges[c] > edges[c - 1]))
            return fail(h, SITRK_EINVAL, "%s: edges must increase strictly (edges[%d] = %g)", fn, c, edges[c]);
    }
    for (int t = 0; t < nq; t++)
        if (!(q[t] >= 0.0 && q[t] <= 1.0)) return fail(h, SITRK_EINVAL, "%s: q[%d] = %g is not in [0, 1]", fn, t, q[t]);
    return SITRK_OK;
}

void dist_empty(int nb, int64_t *counts, int nq, double *qval, int64_t *qrank, int64_t *m, int64_t *nnan)
{
    for (int c = 0; nb > 0 && c < nb + 2; c++) counts[c] = 0;
    for (int t = 0; t < nq; t++) { qval[t] = std::nan(""); qrank[t] = -1; }
    if (m) *m = 0;
    if (nnan) *nnan = 0;
}

// everything behind the keys (n > 0) and their rows of partials: queues the kernels, downloads the result and synchronises
int dist_run(sitrk_ctx *h, int64_t n, const DistBuf &b, int nb, const double *edges, int64_t *counts, int nq, const double *q, double *qval,
             int64_t *qrank, int64_t *m, int64_t *nnan)
{
    if (nb > 0) HIPCHK(upload(h, b.edges, edges, (size_t)nb + 1));
    if (nq > 0) HIPCHK(upload(h, b.q, q, (size_t)nq));
    hipLaunchKernelGGL(dist_setup_kernel, dim3(1), dim3(kDistThreads), 0, h->stream, (int64_t)nblk(n, kDistThreads), b.part, nq, b.q, b.st, b.down);
    HIPCHK(hipGetLastError());
    RCCHK(h->dist_timer.mark(h, 1));
    const Strided L(n, kDistWide, kDistMaxBlocks);
    if (nb > 0) {
        int step0 = 1;
        while (step0 * 2 <= nb + 1) step0 *= 2;
        hipLaunchKernelGGL(dist_count_kernel, dim3(L.blocks), dim3(kDistWide), 0, h->stream, n, L.trips, b.keys, nb, step0, b.edges, b.hrows);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(dist_hist_sum_kernel, dim3(nblk(nb + 2, kDistSumCols)), dim3(kDistThreads), 0, h->stream, (int)L.blocks, nb + 2, b.hrows,
                           b.down + down_counts(nq));
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->dist_timer.mark(h, 2));
    if (nq > 0) {
        for (int shift = 56; shift >= 0; shift -= 8) {
            const u64 himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
            hipLaunchKernelGGL(dist_select_kernel, dim3(L.blocks), dim3(kDistWide), 0, h->stream, n, L.trips, b.keys, nq, shift, himask,
                               h->dist_aggregate, b.st, b.srows);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(dist_pick_kernel, dim3(1), dim3(kDistWide), 0, h->stream, (int)L.blocks, nq, shift, b.srows, b.st, b.down);
            HIPCHK(hipGetLastError());
            if (shift == 56) RCCHK(h->dist_timer.mark(h, 3));              // behind the top-digit pass
        }
    } else {
        RCCHK(h->dist_timer.mark(h, 3));
    }
    h->dist_passes = nq > 0 ? 8 : 0;
    RCCHK(h->dist_timer.mark(h, 4));
    h->dist_timer.done();
    int64_t host[2 + 2 * SITRK_DIST_MAXQ + SITRK_DIST_MAXBINS + 2];
    const size_t words = (size_t)down_counts(nq) + (nb > 0 ? nb + 2 : 0);
    HIPCHK(download(h, host, b.down, words));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (m) *m = host[0];
    if (nnan) *nnan = host[1];
    for (int t = 0; t < nq; t++) {
        memcpy(&qval[t], &host[down_qval(nq) + t], sizeof(double));
        qrank[t] = host[down_qrank(nq) + t];
    }
    for (int c = 0; nb > 0 && c < nb + 2; c++) counts[c] = host[down_counts(nq) + c];
    return SITRK_OK;
}

}  // namespace

int dist_set_aggregate(sitrk_ctx *h, int value)
{
    if (value < 0 || value > 1) return fail(h, SITRK_EINVAL, "sitrk_set_tuning: dist_aggregate must be 0 or 1");
    h->dist_aggregate = value;
    return SITRK_OK;
}

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_dist_values(sitrk_t *h, int64_t n, const double *x, const int8_t *use, int nb, const double *edges, int64_t *counts,
                                int nq, const double *q, double *qval, int64_t *qrank, int64_t *m, int64_t *nnan)
{
    const char *fn = "sitrk_dist_values";
    NEED(h, "null handle");
    RCCHK(dist_check(h, fn, nb, edges, counts, nq, q, qval, qrank));
    if (!(n >= 0 && n < ((int64_t)1 << 36))) return fail(h, SITRK_EINVAL, "%s: n must be in 0..2^36-1", fn);
    if (n > 0 && !x) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    dist_empty(nb, counts, nq, qval, qrank, m, nnan);
    if (n == 0) return SITRK_OK;
    HIPCHK(hipSetDevice(h->device));
    DistBuf b;
    double *d_x; int8_t *d_use;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_x, n); c.take(d_use, use ? (size_t)n : 0); dist_carve(c, b, n, nb, nq); }));
    HIPCHK(upload(h, d_x, x, n));
    if (use) HIPCHK(upload(h, d_use, use, n));
    RCCHK(h->dist_timer.begin(h));
    RCCHK(h->dist_timer.mark(h, 0));
    hipLaunchKernelGGL(dist_keys_values_kernel, dim3(nblk(n, kDistThreads)), dim3(kDistThreads), 0, h->stream, n, d_x, use ? d_use : nullptr, b.keys,
                       b.part);
    HIPCHK(hipGetLastError());
    return dist_run(h, n, b, nb, edges, counts, nq, q, qval, qrank, m, nnan);
}

SITRK_API int sitrk_mesh_dist(sitrk_t *h, int mesh, int jrec1, int what, int sgn, int nb, const double *edges, int64_t *counts, int nq,
                              const double *q, double *qval, int64_t *qrank, int64_t *m, int64_t *nnan)
{
    const char *fn = "sitrk_mesh_dist";
    NEED(h, "null handle");
    RCCHK(mesh_deform_check(h, fn, mesh, jrec1));
    if (what < 0 || what > 3) return fail(h, SITRK_EINVAL, "%s: what must be 0 (div), 1 (shr), 2 (vor) or 3 (tot), got %d", fn, what);
    if (sgn != 1 && sgn != -1 && sgn != 0) return fail(h, SITRK_EINVAL, "%s: sgn must be +1, -1 or 0 (the absolute value), got %d", fn, sgn);
    if (what == 3 && sgn != 1) return fail(h, SITRK_EINVAL, "%s: what = 3 (tot) needs sgn = +1, got %d", fn, sgn);
    RCCHK(dist_check(h, fn, nb, edges, counts, nq, q, qval, qrank));
    dist_empty(nb, counts, nq, qval, qrank, m, nnan);
    const int64_t nQ = h->mesh[mesh].nQ;
    if (nQ == 0) return SITRK_OK;
    HIPCHK(hipSetDevice(h->device));
    DistBuf b;
    MeshDeformDev d;
    RCCHK(carve_behind_mesh(h, mesh, jrec1, true, true, false, [&](Carver &c) { dist_carve(c, b, nQ, nb, nq); }, &d));
    RCCHK(h->dist_timer.begin(h));
    RCCHK(h->dist_timer.mark(h, 0));
    hipLaunchKernelGGL(dist_keys_mesh_kernel, dim3(nblk(nQ, kDistThreads)), dim3(kDistThreads), 0, h->stream, nQ, d.out, d.status, what, sgn, b.keys,
                       b.part);
    HIPCHK(hipGetLastError());
    return dist_run(h, nQ, b, nb, edges, counts, nq, q, qval, qrank, m, nnan);
}

SITRK_API int sitrk_dist_kernel_ms(sitrk_t *h, float *keys_ms, float *hist_ms, float *select_ms)
{
    NEED(h, "null handle");
    NEED(h->dist_timer.complete, "sitrk_dist_kernel_ms: no distribution call has run its kernels yet");
    float *out[2] = {keys_ms, hist_ms};
    for (int k = 0; k < 2; k++) RCCHK(h->dist_timer.elapsed(h, k, out[k]));
    float top = 0.0f, rest = 0.0f;
    RCCHK(h->dist_timer.elapsed(h, 2, &top));
    RCCHK(h->dist_timer.elapsed(h, 3, &rest));
    if (select_ms) *select_ms = top + rest;
    return SITRK_OK;
}

SITRK_API int sitrk_dist_stats(sitrk_t *h, int *passes, float *top_pass_ms)
{
    NEED(h, "null handle");
    NEED(h->dist_timer.complete, "sitrk_dist_stats: no distribution call has run its kernels yet");
    if (passes) *passes = h->dist_passes;
    RCCHK(h->dist_timer.elapsed(h, 2, top_pass_ms));
    return SITRK_OK;
}
