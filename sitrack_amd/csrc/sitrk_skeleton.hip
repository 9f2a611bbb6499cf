// sitrk_skeleton.hip -- skeletons of the features of a label map (sitrk_skeleton_raster, sitrk_keep_skeleton): an EXTRA the
// reference does not have.  The mask L >= 0 of a label map is thinned on the device by Guo and Hall's two-sub-iteration
// algorithm; what comes down is one row of seven integers per distinct label -- its pixels, skeleton pixels, ends, junctions and
// links -- and the list of the skeleton's end points and junctions, instead of the map.  The contract is in include/sitrk.h and
// all integer, defined without reference to any order of evaluation, so every bit is pinned.
//
// Kernels, wave64, 256 lanes per workgroup, no scratch memory:
//   skel_init_kernel      at most 2048 workgroups: a pixel's state byte L >= 0; the values outside [-1, npix) counted by ballot
//   skel_thin_kernel      THE HOT PATH.  One workgroup per tile of 64 x 64 pixels: the tile and a halo of kSkHalo pixels go from the
//                         source state into LDS, one byte per pixel (positions outside the raster are 0, which is their true
//                         value), up to kSkHalo sub-iterations run there between two LDS copies, and the tile alone is stored to
//                         the destination state.  A sub-iteration reads the 3 x 3 of the state before it, so what the missing
//                         pixels beyond the halo spoil moves inwards by one ring per sub-iteration and has not reached the tile
//                         after kSkHalo of them: a launch equals that many global sub-iterations exactly.  The deletions inside
//                         the tile are counted per sub-iteration, one integer atomic per workgroup and non-zero counter
//   skel_class_kernel     at most 2048 workgroups: X of every skeleton pixel (-1 elsewhere) from the eight bytes around it; the
//                         skeleton pixels counted by ballot
//   skel_count_kernel     one pixel per lane and trip, a wave on a span of pixels of its own: the pixels of every value of L,
//                         summed over the wave by ballot, the value with the most pixels carried in registers along the span
//   skel_flag_kernel      one value per lane: 1 where a value has pixels
//   (rocprim::exclusive_scan)   flag -> row of every value, in ascending value
//   skel_rows_kernel      one value per lane: a value whose row is below maxfeat initialises the row; the last stores nfeat
//   skel_table_kernel     the same spans: the five terms of a skeleton pixel -- itself, end, junction, orthogonal and diagonal
//                         links -- summed per row over the wave by ballot, the row with the most skeleton pixels carried in
//                         registers along the span; five int64 atomic adds bring a row's terms in
//   skel_nodeflag_kernel  one pixel per lane: 1 for a skeleton pixel with X != 2
//   (rocprim::exclusive_scan)   flag -> the row of every node, in ascending p
//   skel_nodes_kernel     one pixel per lane: a node whose row is below maxnode stores (p, L[p], X); the last pixel stores nnode
// No kernel depends on a plain load seeing what another workgroup stored in the same launch (the states ping-pong between
// launches), and no lane waits for another workgroup.  Every loop is bounded by a count fixed before it starts.  Vector stores
// only, integer atomics only.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include "sitrk_internal.h"

namespace sitrk {

namespace {

constexpr int kSkThreads = 256;
constexpr int kSkTile = 64;                        // side of a workgroup's tile; never changes a result
constexpr int kSkHalo = 8;                         // pixels around it in LDS = the most sub-iterations of one launch
constexpr int kSkBatch = 8;                        // sub-iterations per launch as shipped (knob skeleton_batch, 1..kSkHalo)
constexpr int kSkSide = kSkTile + 2 * kSkHalo;     // side of the patch in LDS
constexpr int kSkPitch = (kSkSide + 2 + 3) / 4 * 4;    // ... with a ring of zeros around it, rows of whole words
constexpr int kSkCols = SITRK_SKEL_NCOLS;
constexpr int kSkMaxSub = 1 << 20;
constexpr unsigned kSkBlocks = 2048;               // 256 CUs x 8 resident workgroups
constexpr int64_t kSkSpanWaves = 4 * 2048;         // ... and their waves, each with a span of pixels of its own
constexpr int kSkMinTrips = 4;                     // pieces of 64 pixels in a span, on small rasters too
static_assert(kSkBatch >= 1 && kSkBatch <= kSkHalo, "a launch runs at most as many sub-iterations as the halo is wide");
static_assert(kSkSide * kSkSide % kSkThreads == 0 && kSkTile * kSkTile % kSkThreads == 0, "whole trips over the patch and the tile");

// counters of one call on the device
enum { kSkFeat = 0, kSkNode = 1, kSkSkel = 2, kSkBad = 3, kSkN = 4 };

// the count n of the waves of a workgroup (the same in all lanes of a wave) into a counter, one atomic
__device__ __forceinline__ void block_add(long long n, unsigned long long *c)
{
    __shared__ long long sm[kSkThreads / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long x = sm[0];
#pragma unroll
        for (int w = 1; w < kSkThreads / 64; w++) x += sm[w];
        if (x) atomicAdd(c, (unsigned long long)x);
    }
}

__global__ __launch_bounds__(kSkThreads) void skel_init_kernel(int64_t npix, int trips, const int32_t *__restrict__ map,
                                                               int8_t *__restrict__ state, unsigned long long *__restrict__ tot)
{
    const int64_t stride = (int64_t)gridDim.x * kSkThreads;
    int64_t p = (int64_t)blockIdx.x * kSkThreads + threadIdx.x;
    long long bad = 0;
    for (int t = 0; t < trips; t++, p += stride) {
        bool b = false;
        if (p < npix) {
            const int32_t v = map[p];
            b = v < -1 || (int64_t)v >= npix;
            state[p] = v >= 0 ? 1 : 0;
        }
        bad += __popcll(__ballot(b));
    }
    block_add(bad, tot + kSkBad);
}

// nb sub-iterations k0, k0 + 1, ... of the state src -> dst; del[s] += the pixels sub-iteration k0 + s removed
__global__ __launch_bounds__(kSkThreads) void skel_thin_kernel(int ny, int nx, int k0, int nb, const int8_t *__restrict__ src,
                                                               int8_t *__restrict__ dst, unsigned *__restrict__ del)
{
    constexpr int kWords = (kSkSide + 2) * kSkPitch / 4;               // of one copy of the patch
    __shared__ uint32_t words[2 * kWords];
    __shared__ unsigned ndel[kSkHalo];
    uint8_t *const st0 = (uint8_t *)words, *const st1 = (uint8_t *)(words + kWords);
    const int tid = threadIdx.x;
    const int jt = (int)blockIdx.y * kSkTile, it = (int)blockIdx.x * kSkTile;

    for (int w = tid; w < 2 * kWords; w += kSkThreads) words[w] = 0;   // the rings of zeros, mostly
    if (tid < kSkHalo) ndel[tid] = 0;
    __syncthreads();
#pragma unroll 5
    for (int t = 0; t < kSkSide * kSkSide / kSkThreads; t++) {
        const int q = t * kSkThreads + tid, lj = q / kSkSide, li = q - lj * kSkSide;
        const int j = jt - kSkHalo + lj, i = it - kSkHalo + li;
        uint8_t v = 0;
        if (j >= 0 && j < ny && i >= 0 && i < nx) v = src[(int64_t)j * nx + i] != 0;
        st0[(lj + 1) * kSkPitch + li + 1] = v;
    }
    __syncthreads();

    const uint8_t *cur = st0;
    uint8_t *nxt = st1;
    for (int s = 0; s < nb; s++) {                                     // nb <= kSkHalo, the same in every lane
        const bool odd = (k0 + s) & 1;
        int n = 0;
#pragma unroll 5
        for (int t = 0; t < kSkSide * kSkSide / kSkThreads; t++) {
            const int q = t * kSkThreads + tid, lj = q / kSkSide, li = q - lj * kSkSide;
            const int c = (lj + 1) * kSkPitch + li + 1;
            uint8_t keep = cur[c];
            if (keep) {
                const int p2 = cur[c - kSkPitch], p3 = cur[c - kSkPitch + 1], p4 = cur[c + 1], p5 = cur[c + kSkPitch + 1];
                const int p6 = cur[c + kSkPitch], p7 = cur[c + kSkPitch - 1], p8 = cur[c - 1], p9 = cur[c - kSkPitch - 1];
                const int C = ((p2 ^ 1) & (p3 | p4)) + ((p4 ^ 1) & (p5 | p6)) + ((p6 ^ 1) & (p7 | p8)) + ((p8 ^ 1) & (p9 | p2));
                const int n1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8), n2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9);
                const int N = n1 < n2 ? n1 : n2;
                const int m = odd ? ((p2 | p3 | (p5 ^ 1)) & p4) : ((p6 | p7 | (p9 ^ 1)) & p8);
                if (C == 1 && N >= 2 && N <= 3 && m == 0) {
                    keep = 0;
                    n += lj >= kSkHalo && lj < kSkHalo + kSkTile && li >= kSkHalo && li < kSkHalo + kSkTile;
                }
            }
            nxt[c] = keep;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        if ((tid & 63) == 0 && n) atomicAdd(&ndel[s], (unsigned)n);
        __syncthreads();
        const uint8_t *was = cur;
        cur = nxt;
        nxt = (uint8_t *)was;
    }

#pragma unroll 4
    for (int t = 0; t < kSkTile * kSkTile / kSkThreads; t++) {
        const int q = t * kSkThreads + tid, lj = q / kSkTile, li = q - lj * kSkTile;
        const int j = jt + lj, i = it + li;
        if (j < ny && i < nx) dst[(int64_t)j * nx + i] = (int8_t)cur[(lj + kSkHalo + 1) * kSkPitch + li + kSkHalo + 1];
    }
    if (tid < nb && ndel[tid]) atomicAdd(del + tid, ndel[tid]);
}

__global__ __launch_bounds__(kSkThreads) void skel_class_kernel(int64_t npix, int trips, int ny, int nx, const int8_t *__restrict__ K,
                                                                int8_t *__restrict__ xc, unsigned long long *__restrict__ tot)
{
    const int64_t stride = (int64_t)gridDim.x * kSkThreads;
    int64_t p = (int64_t)blockIdx.x * kSkThreads + threadIdx.x;
    long long nsk = 0;
    for (int t = 0; t < trips; t++, p += stride) {
        bool sk = false;
        if (p < npix) {
            int x = -1;
            sk = K[p] != 0;
            if (sk) {
                const int j = (int)(p / nx), i = (int)(p - (int64_t)j * nx);
                const bool up = j > 0, dn = j < ny - 1, lf = i > 0, rt = i < nx - 1;
                int r[8];                                              // p2 .. p9
                r[0] = up && K[p - nx]; r[1] = up && rt && K[p - nx + 1]; r[2] = rt && K[p + 1]; r[3] = dn && rt && K[p + nx + 1];
                r[4] = dn && K[p + nx]; r[5] = dn && lf && K[p + nx - 1]; r[6] = lf && K[p - 1]; r[7] = up && lf && K[p - nx - 1];
                x = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) x += !r[k] && r[(k + 1) & 7];
            }
            xc[p] = (int8_t)x;
        }
        nsk += __popcll(__ballot(sk));
    }
    block_add(nsk, tot + kSkSkel);
}

// A wave of the two kernels below takes `trips` pieces of 64 pixels that follow each other.  In a piece the lanes of one key are
// summed over the wave by ballot, and the key with the most pixels so far is carried in registers from piece to piece: a key costs
// a wave its atomics once, or once per piece while a larger one holds the registers (an address takes its atomics
// one at a time).
__global__ __launch_bounds__(kSkThreads) void skel_count_kernel(int32_t npix, int trips, const int32_t *__restrict__ map, int32_t *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kSkThreads / 64) + (threadIdx.x >> 6);
    int64_t p = wave * trips * 64 + lane;
    int32_t carry_r = -1;
    int carry_n = 0;
    for (int t = 0; t < trips; t++, p += 64) {
        const int32_t r = p < npix ? map[p] : -1;
        unsigned long long todo = __ballot(r >= 0);
        for (int it = 0; it < 64 && todo; it++) {                      // one trip per value among the piece's pixels: at most 64
            const int src = __ffsll((long long)todo) - 1;
            const int32_t k = __shfl(r, src);
            const unsigned long long mine = __ballot(r == k);
            todo &= ~mine;
            const int sum = __popcll(mine);
            if (k == carry_r) {
                carry_n += sum;
            } else if (carry_r < 0 || sum > carry_n) {                 // the larger of the two stays in registers
                if (lane == 0 && carry_r >= 0) atomicAdd(cnt + carry_r, carry_n);
                carry_r = k; carry_n = sum;
            } else if (lane == 0) {
                atomicAdd(cnt + k, sum);
            }
        }
    }
    if (lane == 0 && carry_r >= 0) atomicAdd(cnt + carry_r, carry_n);
}

__global__ __launch_bounds__(kSkThreads) void skel_flag_kernel(int64_t npix, const int32_t *__restrict__ cnt, int32_t *__restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * kSkThreads + threadIdx.x;
    if (v < npix) flag[v] = cnt[v] > 0 ? 1 : 0;
}

__global__ __launch_bounds__(kSkThreads) void skel_rows_kernel(int64_t npix, int64_t maxfeat, const int32_t *__restrict__ cnt,
                                                               const int32_t *__restrict__ row, long long *__restrict__ table,
                                                               unsigned long long *__restrict__ tot)
{
    const int64_t v = (int64_t)blockIdx.x * kSkThreads + threadIdx.x;
    if (v >= npix) return;
    const int32_t n = cnt[v], r = row[v];
    if (v == npix - 1) tot[kSkFeat] = (unsigned long long)(r + (n > 0));
    if (n <= 0 || r >= maxfeat) return;
    long long *t = table + (int64_t)r * kSkCols;
    t[0] = v; t[1] = n;
#pragma unroll
    for (int k = 2; k < kSkCols; k++) t[k] = 0;
}

__device__ __forceinline__ void skel_flush(long long *table, int32_t r, const int (&s)[5])
{
    long long *t = table + (int64_t)r * kSkCols + 2;
#pragma unroll
    for (int k = 0; k < 5; k++)
        if (s[k]) __hip_atomic_fetch_add(t + k, (long long)s[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kSkThreads) void skel_table_kernel(int32_t npix, int trips, int ny, int nx, int64_t maxfeat,
                                                                const int32_t *__restrict__ map, const int8_t *__restrict__ xc,
                                                                const int32_t *__restrict__ row, long long *table)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kSkThreads / 64) + (threadIdx.x >> 6);
    int64_t p = wave * trips * 64 + lane;
    int32_t carry_r = -1;                                              // the row carried from piece to piece, and its terms so far
    int carry_s[5] = {0, 0, 0, 0, 0};                                  // a span has fewer than 2^31 links
    for (int t = 0; t < trips; t++, p += 64) {
        int32_t r = -1;
        bool end = false, junc = false, right = false, down = false, dr = false, dl = false;
        if (p < npix) {
            const int x = xc[p];
            if (x >= 0) {                                              // a skeleton pixel: its label is >= 0
                const int32_t l = map[p];
                r = row[l];
                if (r >= maxfeat) r = -1;
                if (r >= 0) {
                    const int j = (int)(p / nx), i = (int)(p - (int64_t)j * nx);
                    const bool dn = j < ny - 1, lf = i > 0, rt = i < nx - 1;
                    const bool kr = rt && xc[p + 1] >= 0, kd = dn && xc[p + nx] >= 0, kl = lf && xc[p - 1] >= 0;
                    end = x == 1; junc = x >= 3;
                    right = kr && map[p + 1] == l;
                    down = kd && map[p + nx] == l;
                    dr = dn && rt && !kr && !kd && xc[p + nx + 1] >= 0 && map[p + nx + 1] == l;
                    dl = dn && lf && !kl && !kd && xc[p + nx - 1] >= 0 && map[p + nx - 1] == l;
                }
            }
        }
        unsigned long long todo = __ballot(r >= 0);
        for (int it = 0; it < 64 && todo; it++) {                      // one trip per row among the piece's pixels: at most 64
            const int src = __ffsll((long long)todo) - 1;
            const int32_t k = __shfl(r, src);
            const bool mine = r == k;
            const unsigned long long all = __ballot(mine);
            todo &= ~all;
            int v[5];
            v[0] = __popcll(all);
            v[1] = __popcll(__ballot(mine && end));
            v[2] = __popcll(__ballot(mine && junc));
            v[3] = __popcll(__ballot(mine && right)) + __popcll(__ballot(mine && down));
            v[4] = __popcll(__ballot(mine && dr)) + __popcll(__ballot(mine && dl));
            if (k == carry_r) {
#pragma unroll
                for (int q = 0; q < 5; q++) carry_s[q] += v[q];
            } else if (carry_r < 0 || v[0] > carry_s[0]) {             // the larger of the two stays in registers
                if (lane == 0 && carry_r >= 0) skel_flush(table, carry_r, carry_s);
                carry_r = k;
#pragma unroll
                for (int q = 0; q < 5; q++) carry_s[q] = v[q];
            } else if (lane == 0) {
                skel_flush(table, k, v);
            }
        }
    }
    if (lane == 0 && carry_r >= 0) skel_flush(table, carry_r, carry_s);
}

__global__ __launch_bounds__(kSkThreads) void skel_nodeflag_kernel(int64_t npix, const int8_t *__restrict__ xc, int32_t *__restrict__ flag)
{
    const int64_t p = (int64_t)blockIdx.x * kSkThreads + threadIdx.x;
    if (p >= npix) return;
    const int x = xc[p];
    flag[p] = x >= 0 && x != 2 ? 1 : 0;
}

__global__ __launch_bounds__(kSkThreads) void skel_nodes_kernel(int64_t npix, int64_t maxnode, const int32_t *__restrict__ map,
                                                                const int8_t *__restrict__ xc, const int32_t *__restrict__ flag,
                                                                const int32_t *__restrict__ row, long long *__restrict__ nodes,
                                                                unsigned long long *__restrict__ tot)
{
    const int64_t p = (int64_t)blockIdx.x * kSkThreads + threadIdx.x;
    if (p >= npix) return;
    const int32_t f = flag[p], r = row[p];
    if (p == npix - 1) tot[kSkNode] = (unsigned long long)(r + f);
    if (!f || r >= maxnode) return;
    long long *t = nodes + (int64_t)r * 3;
    t[0] = p; t[1] = map[p]; t[2] = xc[p];
}

struct SkelArgs {
    int ny, nx, max_sub;
    int64_t maxfeat, maxnode;
    int8_t *skel;
    int64_t *table, *nodes, *nfeat, *nnode, *nskel;
    int *nsub, *converged;
};

struct SkelBuf {
    int32_t *map;                       // the raster entry point's upload; null where the map is a kept one
    int8_t *st[2], *xc;
    int32_t *cnt, *flag, *row;
    long long *table, *nodes;
    unsigned long long *tot;
    unsigned *del;
    char *scan_tmp;
    size_t scan_bytes;
};

int skel_check(sitrk_ctx *h, const char *fn, int ny, int nx, const SkelArgs &a)
{
    RCCHK(check_raster_shape(h, fn, ny, nx));
    if (a.max_sub < 1 || a.max_sub > kSkMaxSub) return fail(h, SITRK_EINVAL, "%s: max_sub must be in 1..%d (got %d)", fn, kSkMaxSub, a.max_sub);
    if (a.maxfeat < 0) return fail(h, SITRK_EINVAL, "%s: maxfeat must be >= 0 (got %lld)", fn, (long long)a.maxfeat);
    if (a.maxnode < 0) return fail(h, SITRK_EINVAL, "%s: maxnode must be >= 0 (got %lld)", fn, (long long)a.maxnode);
    if (a.maxfeat > 0 && !a.table) return fail(h, SITRK_EINVAL, "%s: null table with maxfeat = %lld", fn, (long long)a.maxfeat);
    if (a.maxnode > 0 && !a.nodes) return fail(h, SITRK_EINVAL, "%s: null nodes with maxnode = %lld", fn, (long long)a.maxnode);
    return SITRK_OK;
}

// everything behind the checks.  host_map: uploaded and range-checked (sitrk_skeleton_raster); else dev_map is a kept map
int skel_core(sitrk_ctx *h, const char *fn, const SkelArgs &a, const int32_t *host_map, const int32_t *dev_map)
{
    const int ny = a.ny, nx = a.nx;
    const int64_t npix = (int64_t)ny * nx;
    if (a.nfeat) *a.nfeat = 0;
    if (a.nnode) *a.nnode = 0;
    if (a.nskel) *a.nskel = 0;
    if (a.nsub) *a.nsub = 0;
    if (a.converged) *a.converged = 0;
    HIPCHK(hipSetDevice(h->device));
    const int64_t frows = a.maxfeat < npix ? a.maxfeat : npix, nrows = a.maxnode < npix ? a.maxnode : npix;
    SkelBuf b;
    RCCHK(scan_i32_bytes(h, npix, &b.scan_bytes));
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(b.map, host_map ? (size_t)npix : 0); c.take(b.st[0], npix); c.take(b.st[1], npix); c.take(b.xc, npix);
        c.take(b.cnt, npix); c.take(b.flag, npix); c.take(b.row, npix);
        c.take(b.table, (size_t)frows * kSkCols); c.take(b.nodes, (size_t)nrows * 3); c.take(b.tot, kSkN); c.take(b.del, kSkHalo);
        c.take(b.scan_tmp, b.scan_bytes);
    }));
    RCCHK(h->skel_timer.begin(h));
    const int32_t *map = dev_map;
    if (host_map) {
        HIPCHK(upload(h, b.map, host_map, (size_t)npix));
        map = b.map;
    }
    HIPCHK(hipMemsetAsync(b.tot, 0, kSkN * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemsetAsync(b.cnt, 0, (size_t)npix * sizeof(int32_t), h->stream));
    const Strided sp(npix, kSkThreads, kSkBlocks);
    hipLaunchKernelGGL(skel_init_kernel, dim3(sp.blocks), dim3(kSkThreads), 0, h->stream, npix, sp.trips, map, b.st[0], b.tot);
    HIPCHK(hipGetLastError());
    unsigned long long tot[kSkN] = {0, 0, 0, 0};
    if (host_map) {                                                    // before anything is indexed by a value of the map
        HIPCHK(download(h, tot, b.tot, kSkN));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (tot[kSkBad]) return fail(h, SITRK_EINDEX, "%s: %llu value(s) of the map lie outside [-1, %lld)", fn, tot[kSkBad], (long long)npix);
    }

    // the thinning: batches of `batch` sub-iterations, the last one cut to what max_sub leaves; a batch's counters are the only
    // download in the loop, which stops behind two sub-iterations in a row that removed nothing
    RCCHK(h->skel_timer.mark(h, 0));
    const dim3 tiles((unsigned)((nx + kSkTile - 1) / kSkTile), (unsigned)((ny + kSkTile - 1) / kSkTile));
    const int batch = h->skeleton_batch > 0 ? h->skeleton_batch : kSkBatch;
    int cur = 0, done = 0, nsub = 0, quiet = 0;
    while (done < a.max_sub && quiet < 2) {
        const int nb = a.max_sub - done < batch ? a.max_sub - done : batch;
        unsigned del[kSkHalo];
        HIPCHK(hipMemsetAsync(b.del, 0, kSkHalo * sizeof(unsigned), h->stream));
        hipLaunchKernelGGL(skel_thin_kernel, tiles, dim3(kSkThreads), 0, h->stream, ny, nx, done, nb, b.st[cur], b.st[cur ^ 1], b.del);
        HIPCHK(hipGetLastError());
        HIPCHK(download(h, del, b.del, kSkHalo));
        HIPCHK(hipStreamSynchronize(h->stream));
        cur ^= 1;
        for (int s = 0; s < nb; s++) {
            if (del[s]) { nsub = done + s + 1; quiet = 0; }
            else if (quiet < 2) quiet++;
        }
        done += nb;
    }
    const int8_t *K = b.st[cur];
    RCCHK(h->skel_timer.mark(h, 1));

    // the table
    hipLaunchKernelGGL(skel_class_kernel, dim3(sp.blocks), dim3(kSkThreads), 0, h->stream, npix, sp.trips, ny, nx, K, b.xc, b.tot);
    HIPCHK(hipGetLastError());
    const WaveSpans ws(npix, kSkThreads, kSkSpanWaves, kSkMinTrips);
    hipLaunchKernelGGL(skel_count_kernel, dim3(ws.blocks), dim3(kSkThreads), 0, h->stream, (int32_t)npix, ws.trips, map, b.cnt);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(skel_flag_kernel, dim3(nblk(npix, kSkThreads)), dim3(kSkThreads), 0, h->stream, npix, b.cnt, b.flag);
    HIPCHK(hipGetLastError());
    size_t tb = b.scan_bytes;
    HIPCHK(rocprim::exclusive_scan(b.scan_tmp, tb, b.flag, b.row, 0, (size_t)npix, rocprim::plus<int32_t>(), h->stream));
    hipLaunchKernelGGL(skel_rows_kernel, dim3(nblk(npix, kSkThreads)), dim3(kSkThreads), 0, h->stream, npix, frows, b.cnt, b.row, b.table, b.tot);
    HIPCHK(hipGetLastError());
    if (frows > 0) {
        hipLaunchKernelGGL(skel_table_kernel, dim3(ws.blocks), dim3(kSkThreads), 0, h->stream, (int32_t)npix, ws.trips, ny, nx, frows, map, b.xc,
                           b.row, b.table);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->skel_timer.mark(h, 2));

    // the nodes: their flags lie over the counters and their rows over the values' flags, both dead by now
    int32_t *nflag = b.cnt, *nrow = b.flag;
    hipLaunchKernelGGL(skel_nodeflag_kernel, dim3(nblk(npix, kSkThreads)), dim3(kSkThreads), 0, h->stream, npix, b.xc, nflag);
    HIPCHK(hipGetLastError());
    tb = b.scan_bytes;
    HIPCHK(rocprim::exclusive_scan(b.scan_tmp, tb, nflag, nrow, 0, (size_t)npix, rocprim::plus<int32_t>(), h->stream));
    hipLaunchKernelGGL(skel_nodes_kernel, dim3(nblk(npix, kSkThreads)), dim3(kSkThreads), 0, h->stream, npix, nrows, map, b.xc, nflag, nrow, b.nodes, b.tot);
    HIPCHK(hipGetLastError());
    RCCHK(h->skel_timer.mark(h, 3));
    h->skel_timer.done();

    HIPCHK(download(h, tot, b.tot, kSkN));
    if (a.skel) HIPCHK(download(h, a.skel, K, (size_t)npix));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int64_t nf = (int64_t)tot[kSkFeat], nn = (int64_t)tot[kSkNode];
    const int64_t tr = nf < frows ? nf : frows, nr = nn < nrows ? nn : nrows;
    if (tr > 0) HIPCHK(download(h, a.table, b.table, (size_t)tr * kSkCols));
    if (nr > 0) HIPCHK(download(h, a.nodes, b.nodes, (size_t)nr * 3));
    if (tr > 0 || nr > 0) HIPCHK(hipStreamSynchronize(h->stream));
    if (a.nfeat) *a.nfeat = nf;
    if (a.nnode) *a.nnode = nn;
    if (a.nskel) *a.nskel = (int64_t)tot[kSkSkel];
    if (a.nsub) *a.nsub = nsub;
    if (a.converged) *a.converged = a.max_sub >= nsub + 2 ? 1 : 0;
    return SITRK_OK;
}

}  // namespace

int skeleton_set_batch(sitrk_ctx *h, int value)
{
    if (value < 1 || value > kSkHalo) return fail(h, SITRK_EINVAL, "sitrk_set_tuning: skeleton_batch must be 1..%d", kSkHalo);
    h->skeleton_batch = value;
    return SITRK_OK;
}

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_skeleton_raster(sitrk_t *h, int ny, int nx, const int32_t *map, int max_sub, int64_t maxfeat, int64_t maxnode,
                                    int8_t *skel, int64_t *table, int64_t *nodes, int64_t *nfeat, int64_t *nnode, int64_t *nskel,
                                    int *nsub, int *converged)
{
    const char *fn = "sitrk_skeleton_raster";
    NEED(h, "null handle");
    const SkelArgs a = {ny, nx, max_sub, maxfeat, maxnode, skel, table, nodes, nfeat, nnode, nskel, nsub, converged};
    RCCHK(skel_check(h, fn, ny, nx, a));
    if (!map) return fail(h, SITRK_EINVAL, "%s: null map", fn);
    return skel_core(h, fn, a, map, nullptr);
}

SITRK_API int sitrk_keep_skeleton(sitrk_t *h, int keep, int max_sub, int64_t maxfeat, int64_t maxnode, int8_t *skel, int64_t *table,
                                  int64_t *nodes, int64_t *nfeat, int64_t *nnode, int64_t *nskel, int *nsub, int *converged)
{
    const char *fn = "sitrk_keep_skeleton";
    NEED(h, "null handle");
    if (keep < 0 || keep >= SITRK_KEEP_MAX) return fail(h, SITRK_EINVAL, "%s: keep must be in 0..%d (got %d)", fn, SITRK_KEEP_MAX - 1, keep);
    if (!h->keep[keep].map) return fail(h, SITRK_EINVAL, "%s: kept map %d is empty", fn, keep);
    const KeptMap &k = h->keep[keep];
    const SkelArgs a = {k.ny, k.nx, max_sub, maxfeat, maxnode, skel, table, nodes, nfeat, nnode, nskel, nsub, converged};
    RCCHK(skel_check(h, fn, k.ny, k.nx, a));
    return skel_core(h, fn, a, nullptr, k.map);
}

SITRK_API int sitrk_skeleton_kernel_ms(sitrk_t *h, float *thin_ms, float *table_ms, float *nodes_ms)
{
    NEED(h, "null handle");
    NEED(h->skel_timer.complete, "sitrk_skeleton_kernel_ms: no skeleton call has run its kernels yet");
    float *out[3] = {thin_ms, table_ms, nodes_ms};
    for (int k = 0; k < 3; k++) RCCHK(h->skel_timer.elapsed(h, k, out[k]));
    return SITRK_OK;
}
