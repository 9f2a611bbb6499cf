// sitrk_label.hip -- connected components of a mask on a regular grid (sitrk_label_raster, sitrk_mesh_features): an EXTRA the
// reference does not have.  The features of a deformation map -- the connected bands of pixels that pass a threshold -- labelled
// on the device, and one row of twelve integers per feature brought down instead of the map.  The contract is in include/sitrk.h
// and DESIGN.md 3.17: all integer, so every bit is pinned.
//
// Kernels, wave64, 256 lanes per workgroup, no scratch memory:
//   label_mask_kernel     (mesh path) one pixel per lane: its owner, the owner's rates from the device's `out`, the test, the byte
//   label_tile_kernel     one workgroup per tile of 64 x 64 pixels, one wave per row and trip: the row's mask by ballot, every pixel
//                         starts at the first pixel of its row run, the runs of two rows are united by atomicMin in LDS (16 KB of
//                         int32 parents + 512 B of row masks), every pixel chases its root and stores it as a linear index of the
//                         raster, -1 for an inactive pixel
//   label_merge_kernel    one launch per level, ONE workgroup per 2 x 2 group of the regions of the level below: its lanes unite
//                         the pixel pairs along the two borders inside the group.  The workgroups of a launch touch disjoint sets
//                         of parents; inside a workgroup every parent is read by an agent-scope atomic load and linked by an
//                         atomicMin on a root, the larger root under the smaller, so a root is the minimum of its set
//   label_flatten_kernel  one pixel per lane and trip, a wave on a span of pixels of its own: a read-only chase to the root ->
//                         labels; the pixels of a root are counted over the wave, the largest root's count stays in registers
//                         along the span, and a count reaches the root's counter by one integer atomic
//   label_flag_kernel     at most 2048 workgroups: flag = root && npix >= min_pix; the roots and the active pixels counted by
//                         ballot, one integer atomic per workgroup and counter
//   (rocprim::exclusive_scan)   flag -> row of every feature, in ascending label
//   label_rows_kernel     one pixel per lane: a flagged root whose row is below maxfeat initialises that row; the last pixel stores
//                         the number of features
//   label_table_kernel    one pixel per lane and trip, the same spans: its eleven terms, reduced over the lanes that follow each
//                         other with one row, then over the wave's runs of that row; the largest row stays in registers along
//                         the span; seven integer atomic adds and four atomic min / max bring a row's terms in
// No kernel depends on a plain load seeing what another workgroup stored in the same launch, and no lane waits for another
// workgroup: the phases are kernel boundaries on the handle's stream.  Every loop is bounded by a count fixed before it starts;
// a chase or a retry loop that reaches its bound -- the number of pixels, which no chain of strictly falling indices can reach --
// sets the give-up word, which the host turns into an error.  Vector stores only, integer atomics only.
#include <cmath>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kLbThreads = 256;
constexpr int kLbTile = SITRK_LABEL_TILE;
constexpr int kLbRowsPerWave = kLbTile / (kLbThreads / 64);
constexpr int kLbCols = SITRK_FEAT_NCOLS;
constexpr unsigned kLbFlagBlocks = 2048;           // 256 CUs x 8 resident workgroups
constexpr int64_t kLbSpanWaves = 4 * 2048;         // ... and their waves, each with a span of pixels of its own
constexpr int kLbMinTrips = 4;                     // pieces of 64 pixels in a span, on small rasters too
constexpr long long kLbBig = (long long)1 << 40;   // above every coordinate
static_assert(kLbTile == 64, "one wave per row of a tile");

// counters of one call on the device: components, active pixels, features, give-up word
enum { kTotComp = 0, kTotActive = 1, kTotFeat = 2, kTotGiveUp = 3, kTotN = 4 };

template <bool GLOBAL>
__device__ __forceinline__ int32_t parent_load(const int32_t *P, int32_t x)
{
    if (GLOBAL) return __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool GLOBAL>
__device__ __forceinline__ int32_t parent_min(int32_t *P, int32_t x, int32_t v)
{
    if (GLOBAL) return __hip_atomic_fetch_min(P + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __hip_atomic_fetch_min(P + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the root of x, or -1 after `bound` steps.  A parent is never above its child, so a chain has fewer than `bound` links
template <bool GLOBAL>
__device__ __forceinline__ int32_t find_root(const int32_t *P, int32_t x, int32_t bound)
{
    for (int32_t k = 0; k < bound; k++) {
        const int32_t up = parent_load<GLOBAL>(P, x);
        if (up == x) return x;
        if (up < 0) return -1;                                         // never on an active pixel: nothing is read through it
        x = up;
    }
    return -1;
}

// The sets of a and b become one.  The larger root is linked under the smaller by atomicMin; where the minimum found another
// parent there already (another lane linked that root first), the three are united from there: the larger of the two indices in
// hand falls with every trip, so there are fewer than `bound` of them.  false: a bound was reached
template <bool GLOBAL>
__device__ __forceinline__ bool unite(int32_t *P, int32_t a, int32_t b, int32_t bound)
{
    for (int32_t k = 0; k < bound; k++) {
        a = find_root<GLOBAL>(P, a, bound);
        b = find_root<GLOBAL>(P, b, bound);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = parent_min<GLOBAL>(P, hi, lo);
        if (old == hi) return true;
        a = old; b = lo;
    }
    return false;
}

__global__ __launch_bounds__(kLbThreads) void label_mask_kernel(int64_t npix, int64_t nQ, const int32_t *__restrict__ owner,
                                                                const double *__restrict__ out, int what, double sgn, double thr,
                                                                double thr2, int8_t *__restrict__ mask)
{
    const int64_t p = (int64_t)blockIdx.x * kLbThreads + threadIdx.x;
    if (p >= npix) return;
    const int32_t v = owner[p];
    bool a = false;
    if (v >= 0) {
        if (what == 3) {
            const double div = out[v], shr = out[nQ + v];
            a = div * div + shr * shr >= thr2;                         // a NaN is never active
        } else {
            const double f = out[(int64_t)what * nQ + v];
            a = sgn * f >= thr;
        }
    }
    mask[p] = a ? 1 : 0;
}

__global__ __launch_bounds__(kLbThreads) void label_tile_kernel(int ny, int nx, int conn8, const int8_t *__restrict__ active,
                                                                int32_t *__restrict__ parent, unsigned long long *__restrict__ tot)
{
    __shared__ int32_t lab[kLbTile * kLbTile];
    __shared__ unsigned long long rows[kLbTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (int)blockIdx.x * kLbTile + lane, jt = (int)blockIdx.y * kLbTile;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;

#pragma unroll
    for (int k = 0; k < kLbRowsPerWave; k++) {
        const int lj = wave + k * (kLbThreads / 64), j = jt + lj;
        const bool a = j < ny && i < nx && active[(int64_t)j * nx + i] != 0;
        const unsigned long long m = __ballot(a);
        if (lane == 0) rows[lj] = m;
        const unsigned long long gap = ~m & below;                     // the inactive pixels of the row in front of this one
        const int start = gap ? 64 - __clzll((long long)gap) : 0;
        lab[lj * kLbTile + lane] = a ? lj * kLbTile + start : -1;
    }
    __syncthreads();

    // a run meets the row above: where the pixel above is active, the first pixel of the overlap unites the two (the others
    // would repeat it); with corner neighbours also the pixel above to the left of a run's first and to the right of its last
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kLbRowsPerWave; k++) {
        const int lj = wave + k * (kLbThreads / 64);
        const unsigned long long m = rows[lj], u = lj > 0 ? rows[lj - 1] : 0;
        if (!((m >> lane) & 1)) continue;
        const bool up = (u >> lane) & 1;
        const bool left = lane > 0 && ((m >> (lane - 1)) & 1), upleft = lane > 0 && ((u >> (lane - 1)) & 1);
        const bool right = lane < 63 && ((m >> (lane + 1)) & 1), upright = lane < 63 && ((u >> (lane + 1)) & 1);
        const int32_t q = lj * kLbTile + lane;
        if (up) {
            if (!(left && upleft)) ok = unite<false>(lab, q, q - kLbTile, kLbTile * kLbTile) && ok;
        } else if (conn8) {
            if (upleft && !left) ok = unite<false>(lab, q, q - kLbTile - 1, kLbTile * kLbTile) && ok;
            if (upright && !right) ok = unite<false>(lab, q, q - kLbTile + 1, kLbTile * kLbTile) && ok;
        }
    }
    __syncthreads();

#pragma unroll
    for (int k = 0; k < kLbRowsPerWave; k++) {
        const int lj = wave + k * (kLbThreads / 64), j = jt + lj;
        const int32_t q = lj * kLbTile + lane;
        int32_t v = -1;
        if ((rows[lj] >> lane) & 1) {
            const int32_t r = find_root<false>(lab, q, kLbTile * kLbTile);
            if (r < 0) ok = false;
            else v = (jt + (r >> 6)) * nx + ((int)blockIdx.x * kLbTile + (r & 63));
        }
        if (j < ny && i < nx) parent[(int64_t)j * nx + i] = v;
    }
    if (!ok) atomicOr(tot + kTotGiveUp, 1ull);
}

// `half` = the side of a region of the level below; the group of this workgroup is rows j0..j1-1 by columns i0..i1-1
__global__ __launch_bounds__(kLbThreads) void label_merge_kernel(int ny, int nx, int conn8, int half, const int8_t *__restrict__ active,
                                                                 int32_t *parent, int32_t bound, unsigned long long *__restrict__ tot)
{
    const int side = 2 * half;
    const int j0 = (int)blockIdx.y * side, i0 = (int)blockIdx.x * side;
    const int j1 = j0 + side < ny ? j0 + side : ny, i1 = i0 + side < nx ? i0 + side : nx;
    const int y = j0 + half, x = i0 + half;                            // the first row / column behind the two borders
    bool ok = true;
    auto act = [&](int j, int i) { return active[(int64_t)j * nx + i] != 0; };
    auto pix = [&](int j, int i) { return (int32_t)(j * nx + i); };    // ny*nx <= 2^28

    if (x < i1) {                                                      // pairs (j, x-1) -- (j', x)
        const int trips = (j1 - j0 + kLbThreads - 1) / kLbThreads;
        for (int t = 0; t < trips; t++) {
            const int j = j0 + t * kLbThreads + (int)threadIdx.x;
            if (j >= j1 || !act(j, x - 1)) continue;
            const int32_t a = pix(j, x - 1);
            if (act(j, x)) {
                // the pair above, where both its pixels are active and it lies on the same side of the other border, implies this one
                const bool implied = j > j0 && j != y && act(j - 1, x - 1) && act(j - 1, x);
                if (!implied) ok = unite<true>(parent, a, pix(j, x), bound) && ok;
            } else if (conn8) {                                        // (with (j, x) active its neighbours above and below are joined to it)
                if (j > j0 && act(j - 1, x)) ok = unite<true>(parent, a, pix(j - 1, x), bound) && ok;
                if (j + 1 < j1 && act(j + 1, x)) ok = unite<true>(parent, a, pix(j + 1, x), bound) && ok;
            }
        }
    }
    if (y < j1) {                                                      // pairs (y-1, i) -- (y, i')
        const int trips = (i1 - i0 + kLbThreads - 1) / kLbThreads;
        for (int t = 0; t < trips; t++) {
            const int i = i0 + t * kLbThreads + (int)threadIdx.x;
            if (i >= i1 || !act(y - 1, i)) continue;
            const int32_t a = pix(y - 1, i);
            if (act(y, i)) {
                const bool implied = i > i0 && i != x && act(y - 1, i - 1) && act(y, i - 1);
                if (!implied) ok = unite<true>(parent, a, pix(y, i), bound) && ok;
            } else if (conn8) {
                if (i > i0 && act(y, i - 1)) ok = unite<true>(parent, a, pix(y, i - 1), bound) && ok;
                if (i + 1 < i1 && act(y, i + 1)) ok = unite<true>(parent, a, pix(y, i + 1), bound) && ok;
            }
        }
    }
    if (!ok) atomicOr(tot + kTotGiveUp, 1ull);
}

// the lanes of a wave that follow each other with one key form a run: *first = this lane starts one; the mask of all such lanes
__device__ __forceinline__ unsigned long long wave_run_heads(int32_t key, bool *first)
{
    const int32_t prev = __shfl_up(key, 1);
    *first = (threadIdx.x & 63) == 0 || prev != key;
    return __ballot(*first);
}

// A wave of the two kernels below takes `trips` pieces of 64 pixels that follow each other.  In a piece the runs of one key are
// summed over the wave, and the key with the most pixels so far is carried in registers from piece to piece: a component costs a
// wave its atomics once, or once per piece while a larger one holds the registers.  (One set of atomics per run put a component
// of 10^7 pixels on one address 5 x 10^6 times over, and an address takes them one at a time: 376 ms of a 380 ms call)
__global__ __launch_bounds__(kLbThreads) void label_flatten_kernel(int32_t npix, int trips, const int32_t *__restrict__ parent,
                                                                   int32_t *__restrict__ labels, int32_t *__restrict__ cnt,
                                                                   unsigned long long *__restrict__ tot)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kLbThreads / 64) + (threadIdx.x >> 6);
    int64_t p = wave * trips * 64 + lane;
    bool ok = true;
    int32_t carry_r = -1;
    int carry_n = 0;
    for (int t = 0; t < trips; t++, p += 64) {
        int32_t r = -1;
        if (p < npix) {
            const int32_t v = parent[p];
            if (v >= 0) {
                int32_t x = v;
                r = -2;
                for (int32_t k = 0; k < npix; k++) {                   // plain loads: nothing is stored to `parent` in this launch
                    const int32_t up = parent[x];
                    if (up == x) { r = x; break; }
                    if (up < 0) break;                                 // never on an active pixel: nothing is read through it
                    x = up;
                }
                if (r == -2) { ok = false; r = -1; }
            }
            labels[p] = r;
        }
        bool first;
        const unsigned long long heads = wave_run_heads(r, &first);
        const unsigned long long next = heads & ~(((unsigned long long)2 << lane) - 1);    // lane 63: the shift leaves 0, none
        const int n = (next ? __ffsll((long long)next) - 1 : 64) - lane;                   // of a lane that starts a run: its pixels
        unsigned long long todo = __ballot(first && r >= 0);
        for (int it = 0; it < 64 && todo; it++) {                      // one trip per root among the piece's runs: at most 64
            const int src = __ffsll((long long)todo) - 1;
            const int32_t k = __shfl(r, src);
            const bool mine = first && r == k;
            const unsigned long long runs = __ballot(mine);
            todo &= ~runs;
            int sum = __shfl(n, src);
            if (__popcll(runs) > 1) {                                  // wave-uniform
                sum = mine ? n : 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            }
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
    if (!ok) atomicOr(tot + kTotGiveUp, 1ull);
}

__global__ __launch_bounds__(kLbThreads) void label_flag_kernel(int64_t npix, int trips, int64_t min_pix, const int32_t *__restrict__ labels,
                                                                const int32_t *__restrict__ cnt, int32_t *__restrict__ flag,
                                                                unsigned long long *__restrict__ tot)
{
    __shared__ int sm[kLbThreads / 64][2];
    const int64_t stride = (int64_t)gridDim.x * kLbThreads;
    int64_t p = (int64_t)blockIdx.x * kLbThreads + threadIdx.x;
    int nroot = 0, nact = 0;                                           // of this wave: the same in all its lanes
    for (int t = 0; t < trips; t++, p += stride) {
        bool root = false, act = false;
        if (p < npix) {
            const int32_t l = labels[p];
            act = l >= 0;
            root = (int64_t)l == p;
            flag[p] = root && (int64_t)cnt[p] >= min_pix ? 1 : 0;
        }
        nroot += __popcll(__ballot(root));
        nact += __popcll(__ballot(act));
    }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = nroot; sm[threadIdx.x >> 6][1] = nact; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = sm[0][0], b = sm[0][1];
#pragma unroll
        for (int w = 1; w < kLbThreads / 64; w++) { a += sm[w][0]; b += sm[w][1]; }
        if (a) atomicAdd(tot + kTotComp, (unsigned long long)a);
        if (b) atomicAdd(tot + kTotActive, (unsigned long long)b);
    }
}

__global__ __launch_bounds__(kLbThreads) void label_rows_kernel(int64_t npix, int64_t maxfeat, const int32_t *__restrict__ flag,
                                                                const int32_t *__restrict__ row, long long *__restrict__ table,
                                                                unsigned long long *__restrict__ tot)
{
    const int64_t p = (int64_t)blockIdx.x * kLbThreads + threadIdx.x;
    if (p >= npix) return;
    const int32_t f = flag[p], r = row[p];
    if (p == npix - 1) tot[kTotFeat] = (unsigned long long)(r + f);
    if (!f || r >= maxfeat) return;
    long long *t = table + (int64_t)r * kLbCols;
    t[0] = p; t[1] = 0;
    t[2] = kLbBig; t[3] = -1; t[4] = kLbBig; t[5] = -1;
#pragma unroll
    for (int k = 6; k < kLbCols; k++) t[k] = 0;
}

// the eleven terms of a run into its row: seven sums, four bounds
__device__ __forceinline__ void table_flush(long long *table, int32_t r, const long long (&s)[7], int lo_j, int hi_j, int lo_i, int hi_i)
{
    long long *t = table + (int64_t)r * kLbCols;
    __hip_atomic_fetch_add(t + 1, s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(t + 2, (long long)lo_j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(t + 3, (long long)hi_j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(t + 4, (long long)lo_i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(t + 5, (long long)hi_i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 1; k < 7; k++) __hip_atomic_fetch_add(t + 5 + k, s[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kLbThreads) void label_table_kernel(int32_t npix, int trips, int ny, int nx, int64_t maxfeat,
                                                                 const int32_t *__restrict__ labels, const int32_t *__restrict__ flag,
                                                                 const int32_t *__restrict__ row, long long *table)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kLbThreads / 64) + (threadIdx.x >> 6);
    int64_t p = wave * trips * 64 + lane;
    int32_t carry_r = -1;                                              // the row carried from piece to piece, and its terms so far
    long long carry_s[7] = {0, 0, 0, 0, 0, 0, 0};
    int carry_lo_j = 0, carry_hi_j = 0, carry_lo_i = 0, carry_hi_i = 0;
    for (int t = 0; t < trips; t++, p += 64) {
        int32_t r = -1;
        long long s[7] = {0, 0, 0, 0, 0, 0, 0};                        // npix, j, i, j*j, i*i, j*i, perimeter
        int lo_j = 0, hi_j = 0, lo_i = 0, hi_i = 0;
        if (p < npix) {
            const int32_t l = labels[p];
            if (l >= 0 && flag[l]) {
                r = row[l];
                if (r >= maxfeat) r = -1;
            }
            if (r >= 0) {
                const int j = (int)(p / nx), i = (int)(p - (int64_t)j * nx);
                int per = 0;                                           // sides whose other pixel is not active; the rim is not
                per += j == 0 || labels[p - nx] < 0;
                per += j == ny - 1 || labels[p + nx] < 0;
                per += i == 0 || labels[p - 1] < 0;
                per += i == nx - 1 || labels[p + 1] < 0;
                s[0] = 1; s[1] = j; s[2] = i; s[3] = (long long)j * j; s[4] = (long long)i * i; s[5] = (long long)j * i; s[6] = per;
                lo_j = hi_j = j; lo_i = hi_i = i;
            }
        }
        bool first;
        const unsigned long long heads = wave_run_heads(r, &first);    // lane 0 always starts a run
        const int run = __popcll(heads & (((unsigned long long)2 << lane) - 1));         // lane 63: the shift leaves 0, all ones
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                             // after the step o a lane holds its run's lanes [lane, lane + 2o)
            const bool same = __shfl_down(run, o) == run && lane + o < 64;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const long long v = __shfl_down(s[k], o);
                if (same) s[k] += v;
            }
            const int a = __shfl_down(lo_j, o), b = __shfl_down(hi_j, o), c = __shfl_down(lo_i, o), d = __shfl_down(hi_i, o);
            if (same) {
                lo_j = a < lo_j ? a : lo_j; hi_j = b > hi_j ? b : hi_j;
                lo_i = c < lo_i ? c : lo_i; hi_i = d > hi_i ? d : hi_i;
            }
        }
        unsigned long long todo = __ballot(first && r >= 0);
        for (int it = 0; it < 64 && todo; it++) {                      // one trip per row among the piece's runs: at most 64
            const int src = __ffsll((long long)todo) - 1;
            const int32_t k = __shfl(r, src);
            const bool mine = first && r == k;
            const unsigned long long runs = __ballot(mine);
            todo &= ~runs;
            long long v[7];
            int a, b, c, d;
            if (__popcll(runs) > 1) {                                  // wave-uniform: the runs of this row, summed over the wave
#pragma unroll
                for (int q = 0; q < 7; q++) v[q] = mine ? s[q] : 0;
                a = mine ? lo_j : INT32_MAX; b = mine ? hi_j : -1; c = mine ? lo_i : INT32_MAX; d = mine ? hi_i : -1;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                    for (int q = 0; q < 7; q++) v[q] += __shfl_xor(v[q], o);
                    const int a2 = __shfl_xor(a, o), b2 = __shfl_xor(b, o), c2 = __shfl_xor(c, o), d2 = __shfl_xor(d, o);
                    a = a2 < a ? a2 : a; b = b2 > b ? b2 : b; c = c2 < c ? c2 : c; d = d2 > d ? d2 : d;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 7; q++) v[q] = __shfl(s[q], src);
                a = __shfl(lo_j, src); b = __shfl(hi_j, src); c = __shfl(lo_i, src); d = __shfl(hi_i, src);
            }
            if (k == carry_r) {
#pragma unroll
                for (int q = 0; q < 7; q++) carry_s[q] += v[q];
                carry_lo_j = a < carry_lo_j ? a : carry_lo_j; carry_hi_j = b > carry_hi_j ? b : carry_hi_j;
                carry_lo_i = c < carry_lo_i ? c : carry_lo_i; carry_hi_i = d > carry_hi_i ? d : carry_hi_i;
            } else if (carry_r < 0 || v[0] > carry_s[0]) {             // the larger of the two stays in registers
                if (lane == 0 && carry_r >= 0) table_flush(table, carry_r, carry_s, carry_lo_j, carry_hi_j, carry_lo_i, carry_hi_i);
                carry_r = k;
#pragma unroll
                for (int q = 0; q < 7; q++) carry_s[q] = v[q];
                carry_lo_j = a; carry_hi_j = b; carry_lo_i = c; carry_hi_i = d;
            } else if (lane == 0) {
                table_flush(table, k, v, a, b, c, d);
            }
        }
    }
    if (lane == 0 && carry_r >= 0) table_flush(table, carry_r, carry_s, carry_lo_j, carry_hi_j, carry_lo_i, carry_hi_i);
}

// the scratch of one call behind whatever makes its mask.  `flag` lies over `parent` and `row` over `cnt`: the parents are dead
// once the labels are flat, the counters once the flags are set
struct LabelBuf {
    int8_t *mask;
    int32_t *parent, *labels, *cnt;
    long long *table;
    unsigned long long *tot;
    char *scan_tmp;
    size_t scan_bytes;
};

struct LabelJob {
    int ny = 0, nx = 0, conn = 8;
    int64_t min_pix = 1, maxfeat = 0;
};

void label_carve(Carver &c, LabelBuf &b, const LabelJob &j)
{
    const size_t npix = (size_t)j.ny * (size_t)j.nx;
    c.take(b.mask, npix); c.take(b.parent, npix); c.take(b.labels, npix); c.take(b.cnt, npix);
    c.take(b.table, (size_t)j.maxfeat * kLbCols); c.take(b.tot, kTotN); c.take(b.scan_tmp, b.scan_bytes);
}

int label_check(sitrk_ctx *h, const char *fn, int ny, int nx, int conn, int64_t min_pix, int64_t maxfeat, const int64_t *table)
{
    RCCHK(check_raster_shape(h, fn, ny, nx));
    if (conn != 4 && conn != 8) return fail(h, SITRK_EINVAL, "%s: conn must be 4 (edge neighbours) or 8 (edge and corner neighbours), got %d", fn, conn);
    if (min_pix < 1) return fail(h, SITRK_EINVAL, "%s: min_pix must be >= 1 (got %lld)", fn, (long long)min_pix);
    if (maxfeat < 0) return fail(h, SITRK_EINVAL, "%s: maxfeat must be >= 0 (got %lld)", fn, (long long)maxfeat);
    if (maxfeat > 0 && !table) return fail(h, SITRK_EINVAL, "%s: null table with maxfeat = %lld", fn, (long long)maxfeat);
    return SITRK_OK;
}

// everything behind the mask on the device, phases 1 and 2 of the label timer (the caller has begun it and marked the mask's
// phase): queues the kernels and the downloads, synchronises
int label_run(sitrk_ctx *h, const char *fn, const LabelJob &j, const LabelBuf &b, int32_t *labels, int64_t *table, int64_t *nfeat,
              int64_t *ncomp, int64_t *nactive)
{
    const int64_t npix = (int64_t)j.ny * j.nx;
    const int conn8 = j.conn == 8;
    int32_t *flag = b.parent, *row = b.cnt;
    HIPCHK(hipMemsetAsync(b.tot, 0, kTotN * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemsetAsync(b.cnt, 0, (size_t)npix * sizeof(int32_t), h->stream));
    RCCHK(h->label_timer.mark(h, 1));
    const dim3 tiles((unsigned)((j.nx + kLbTile - 1) / kLbTile), (unsigned)((j.ny + kLbTile - 1) / kLbTile));
    hipLaunchKernelGGL(label_tile_kernel, tiles, dim3(kLbThreads), 0, h->stream, j.ny, j.nx, conn8, b.mask, b.parent, b.tot);
    HIPCHK(hipGetLastError());
    const int longest = j.ny > j.nx ? j.ny : j.nx;
    for (int half = kLbTile; half < longest; half *= 2) {              // at most 9 levels: 64 * 2^9 = 32768
        const int side = 2 * half;
        const dim3 groups((unsigned)((j.nx + side - 1) / side), (unsigned)((j.ny + side - 1) / side));
        hipLaunchKernelGGL(label_merge_kernel, groups, dim3(kLbThreads), 0, h->stream, j.ny, j.nx, conn8, half, b.mask, b.parent, (int32_t)npix,
                           b.tot);
        HIPCHK(hipGetLastError());
    }
    const WaveSpans ws(npix, kLbThreads, kLbSpanWaves, kLbMinTrips);   // the waves of the flatten and table kernels
    hipLaunchKernelGGL(label_flatten_kernel, dim3(ws.blocks), dim3(kLbThreads), 0, h->stream, (int32_t)npix, ws.trips, b.parent, b.labels,
                       b.cnt, b.tot);
    HIPCHK(hipGetLastError());
    RCCHK(h->label_timer.mark(h, 2));
    const Strided fs(npix, kLbThreads, kLbFlagBlocks);
    hipLaunchKernelGGL(label_flag_kernel, dim3(fs.blocks), dim3(kLbThreads), 0, h->stream, npix, fs.trips, j.min_pix, b.labels, b.cnt, flag,
                       b.tot);
    HIPCHK(hipGetLastError());
    size_t tb = b.scan_bytes;
    HIPCHK(rocprim::exclusive_scan(b.scan_tmp, tb, flag, row, 0, (size_t)npix, rocprim::plus<int32_t>(), h->stream));
    hipLaunchKernelGGL(label_rows_kernel, dim3(nblk(npix, kLbThreads)), dim3(kLbThreads), 0, h->stream, npix, j.maxfeat, flag, row, b.table, b.tot);
    HIPCHK(hipGetLastError());
    if (j.maxfeat > 0) {
        hipLaunchKernelGGL(label_table_kernel, dim3(ws.blocks), dim3(kLbThreads), 0, h->stream, (int32_t)npix, ws.trips, j.ny, j.nx, j.maxfeat,
                           b.labels, flag, row, b.table);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->label_timer.mark(h, 3));
    h->label_timer.done();
    unsigned long long tot[kTotN] = {0, 0, 0, 0};
    HIPCHK(download(h, tot, b.tot, kTotN));
    if (labels) HIPCHK(download(h, labels, b.labels, (size_t)npix));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (tot[kTotGiveUp])
        return fail(h, SITRK_EHIP, "%s: a union-find loop reached its bound of %lld steps and gave up; the labels are not valid", fn,
                    (long long)npix);
    const int64_t rows = (int64_t)tot[kTotFeat] < j.maxfeat ? (int64_t)tot[kTotFeat] : j.maxfeat;
    if (rows > 0) {
        HIPCHK(download(h, table, b.table, (size_t)rows * kLbCols));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (nfeat) *nfeat = (int64_t)tot[kTotFeat];
    if (ncomp) *ncomp = (int64_t)tot[kTotComp];
    if (nactive) *nactive = (int64_t)tot[kTotActive];
    return SITRK_OK;
}

}  // namespace

int scan_i32_bytes(sitrk_ctx *h, int64_t n, size_t *bytes)
{
    *bytes = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, *bytes, (int32_t *)nullptr, (int32_t *)nullptr, 0, (size_t)n, rocprim::plus<int32_t>(), h->stream));
    *bytes = align256(*bytes);
    return SITRK_OK;
}

}  // namespace sitrk

using namespace sitrk;

SITRK_API int sitrk_label_raster(sitrk_t *h, int ny, int nx, const int8_t *active, int conn, int64_t min_pix, int64_t maxfeat,
                                 int32_t *labels, int64_t *table, int64_t *nfeat, int64_t *ncomp, int64_t *nactive)
{
    const char *fn = "sitrk_label_raster";
    NEED(h, "null handle");
    RCCHK(label_check(h, fn, ny, nx, conn, min_pix, maxfeat, table));
    if (!active) return fail(h, SITRK_EINVAL, "%s: null mask", fn);
    if (nfeat) *nfeat = 0;
    if (ncomp) *ncomp = 0;
    if (nactive) *nactive = 0;
    HIPCHK(hipSetDevice(h->device));
    LabelJob j;
    j.ny = ny; j.nx = nx; j.conn = conn; j.min_pix = min_pix; j.maxfeat = maxfeat;
    LabelBuf b;
    RCCHK(scan_i32_bytes(h, (int64_t)ny * nx, &b.scan_bytes));
    RCCHK(carve_scratch(h, [&](Carver &c) { label_carve(c, b, j); }));
    RCCHK(h->label_timer.begin(h));
    RCCHK(h->label_timer.mark(h, 0));
    HIPCHK(upload(h, b.mask, active, (size_t)ny * nx));
    return label_run(h, fn, j, b, labels, table, nfeat, ncomp, nactive);
}

// the body of sitrk_mesh_features behind the handle's check; keep_map (npix, may be null: sitrk_mesh_features_keep of
// sitrk_track.hip) receives the labels of the components that passed min_pix, -1 elsewhere, once everything else has succeeded
int sitrk::mesh_features_body(sitrk_ctx *h, const char *fn, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny,
                              int nx, int what, int sgn, double thr, int conn, int64_t min_pix, int64_t maxfeat, int32_t *labels,
                              int64_t *table, int64_t *nfeat, int64_t *ncomp, int64_t *nactive, int32_t *keep_map)
{
    RCCHK(mesh_deform_check(h, fn, mesh, jrec1));
    if (at_t1 != 0 && at_t1 != 1) return fail(h, SITRK_EINVAL, "%s: at_t1 must be 0 (t0 positions) or 1 (current positions), got %d", fn, at_t1);
    RCCHK(raster_check_grid(h, fn, y0_km, x0_km, d_km, ny, nx));
    RCCHK(label_check(h, fn, ny, nx, conn, min_pix, maxfeat, table));
    if (what < 0 || what > 3) return fail(h, SITRK_EINVAL, "%s: what must be 0 (div), 1 (shr), 2 (vor) or 3 (tot), got %d", fn, what);
    if (sgn != 1 && sgn != -1) return fail(h, SITRK_EINVAL, "%s: sgn must be +1 or -1 (got %d)", fn, sgn);
    if (!std::isfinite(thr)) return fail(h, SITRK_EINVAL, "%s: thr must be finite (got %g)", fn, thr);
    if (what == 3 && (sgn != 1 || !(thr >= 0.0)))
        return fail(h, SITRK_EINVAL, "%s: what = 3 (total deformation) needs sgn = +1 and thr >= 0 (got %d, %g)", fn, sgn, thr);
    if (nfeat) *nfeat = 0;
    if (ncomp) *ncomp = 0;
    if (nactive) *nactive = 0;
    const int64_t npix = (int64_t)ny * nx;
    LabelJob j;
    j.ny = ny; j.nx = nx; j.conn = conn; j.min_pix = min_pix; j.maxfeat = maxfeat;
    LabelBuf b;
    HIPCHK(hipSetDevice(h->device));
    RCCHK(scan_i32_bytes(h, npix, &b.scan_bytes));
    int32_t *d_owner; unsigned long long *d_cnt;
    auto layout = [&](Carver &c) { c.take(d_owner, npix); c.take(d_cnt, 3); label_carve(c, b, j); };
    MeshDeformDev m;
    RCCHK(carve_behind_mesh(h, mesh, jrec1, true, true, false, layout, &m));
    RasterJob r;
    r.nC = m.nQ; r.nP = h->nP; r.nv = 4; r.flag = m.status; r.owner = d_owner; r.cnt = d_cnt;
    if (at_t1) { r.cells = m.quads; r.pts = m.p1; r.only_status1 = true; }
    else { r.block = true; r.pts = m.t0; }
    const RasterGrid g = {y0_km, x0_km, d_km, ny, nx};
    RCCHK(raster_run(h, r, g));
    RCCHK(h->label_timer.begin(h));
    RCCHK(h->label_timer.mark(h, 0));
    const double thr2 = thr * thr;
    hipLaunchKernelGGL(label_mask_kernel, dim3(nblk(npix, kLbThreads)), dim3(kLbThreads), 0, h->stream, npix, m.nQ, d_owner, m.out, what, (double)sgn, thr,
                       thr2, b.mask);
    HIPCHK(hipGetLastError());
    unsigned long long cnt[3] = {0, 0, 0};
    HIPCHK(download(h, cnt, d_cnt, 3));                                // lands with the synchronisation of label_run
    RCCHK(label_run(h, fn, j, b, labels, table, nfeat, ncomp, nactive));
    if (cnt[0]) return fail(h, SITRK_EINDEX, "%s: %llu cell(s) of the mesh have a vertex index outside [0, %lld)", fn, cnt[0], (long long)h->nP);
    if (keep_map) RCCHK(keep_from_labels(h, npix, b.labels, b.parent, keep_map));     // the flags lie over the parents (label_run)
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_features(sitrk_t *h, int mesh, int jrec1, int at_t1, double y0_km, double x0_km, double d_km, int ny, int nx,
                                  int what, int sgn, double thr, int conn, int64_t min_pix, int64_t maxfeat, int32_t *labels,
                                  int64_t *table, int64_t *nfeat, int64_t *ncomp, int64_t *nactive)
{
    NEED(h, "null handle");
    return mesh_features_body(h, "sitrk_mesh_features", mesh, jrec1, at_t1, y0_km, x0_km, d_km, ny, nx, what, sgn, thr, conn, min_pix, maxfeat,
                              labels, table, nfeat, ncomp, nactive, nullptr);
}

SITRK_API int sitrk_features_kernel_ms(sitrk_t *h, float *mask_ms, float *label_ms, float *table_ms)
{
    NEED(h, "null handle");
    NEED(h->label_timer.complete, "sitrk_features_kernel_ms: no labelling call has run its kernels yet");
    float *out[3] = {mask_ms, label_ms, table_ms};
    for (int k = 0; k < 3; k++) RCCHK(h->label_timer.elapsed(h, k, out[k]));
    return SITRK_OK;
}
