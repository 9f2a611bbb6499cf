// sitrk_bins.h -- what the point-cloud modules (subsample, overlap, coast, delaunay, pairs) share when they bin points into cells:
// the order key of a double, the bits of a radix sort, cell marks and offsets, the box reduction of a workgroup.  The first part is
// plain C++, nothing of HIP: a host program can include it alone (tests/c/bins_check.cpp).  Each module keeps its own cell formula.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SITRK_BINS_HD __host__ __device__ __forceinline__
#else
#define SITRK_BINS_HD inline
#endif

namespace sitrk {

// order-preserving map of a double to an unsigned 64-bit key (min/max by integer atomics): a < b  <=>  key(a) < key(b)
SITRK_BINS_HD unsigned long long order_key(double v)
{
    unsigned long long b;
    memcpy(&b, &v, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// ... and its inverse
SITRK_BINS_HD double order_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

// bits a radix sort of the keys 0 .. max_key has to look at: the smallest e in 1..32 with 2^e > max_key.  Keys 0 .. ncells - 1 pass
// ncells - 1; a module that parks its invalid points at key ncells passes ncells
inline unsigned key_bits(uint64_t max_key)
{
    unsigned e = 1;
    while (e < 32 && ((uint64_t)1 << e) <= max_key) e++;
    return e;
}

// trips of bin_start_kernel's search over n sorted keys: a range of n halves to nothing in floor(log2 n) + 1 steps (n < 2^32)
inline int lower_bound_steps(int64_t n) { return (int)key_bits((uint64_t)n); }

#ifdef __HIPCC__

// cell of coordinate v on a grid of nc cells of side 1 / inv_h from v0 (subsample, overlap)
__device__ __forceinline__ int cell_coord(double v, double v0, double inv_h, int nc)
{
    const double t = (v - v0) * inv_h;               // same expression as the host's cell count: t <= nc - 1 by monotonicity
    int c = (int)floor(t);
    return c < 0 ? 0 : (c >= nc ? nc - 1 : c);
}

// sorted slot s of n opens and / or closes the run of its key.  cstart/cend zeroed by the caller: empty cells keep [0,0)
__device__ __forceinline__ void mark_cell_run(const uint32_t *__restrict__ key, int64_t s, int64_t n, int32_t *cstart, int32_t *cend)
{
    const uint32_t k = key[s];
    if (s == 0 || key[s - 1] != k) cstart[k] = (int32_t)s;
    if (s == n - 1 || key[s + 1] != k) cend[k] = (int32_t)(s + 1);
}

// start[b], b = 0 .. nbins: the first of the n sorted positions whose key is >= b (start[nbins] = n when no key exceeds nbins - 1);
// steps = lower_bound_steps(n), so no lane loops on a condition of its own
template <int THREADS>
__global__ __launch_bounds__(THREADS) void bin_start_kernel(int64_t nbins, int32_t n, int steps, const uint32_t *__restrict__ keys,
                                                            int32_t *__restrict__ start)
{
    const int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (b > nbins) return;
    int32_t lo = 0, hi = n;                                            // keys[lo - 1] < b <= keys[hi]
    for (int it = 0; it < steps; it++) {
        if (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < (uint32_t)b) lo = mid + 1; else hi = mid;
        }
    }
    start[b] = lo;
}

// The tree over the columns sm[c][0 .. THREADS) of a workgroup's LDS, column c by operation OPS[c], each exact in any order.  Every
// lane has stored its sm[c][threadIdx.x] and a __syncthreads() lies behind the stores; the result is sm[c][0], visible to every lane
// on return.  Every lane of the workgroup must call it.  T: unsigned long long or long long
enum class Red { Min, Max, Add };

template <int THREADS, Red... OPS, typename T>
__device__ __forceinline__ void block_reduce(T (&sm)[sizeof...(OPS)][THREADS])
{
    constexpr int N = sizeof...(OPS);
    constexpr Red op[N] = {OPS...};
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int c = 0; c < N; c++) {
                const T u = sm[c][threadIdx.x], v = sm[c][threadIdx.x + s];
                sm[c][threadIdx.x] = op[c] == Red::Min ? min(u, v) : (op[c] == Red::Max ? max(u, v) : u + v);
            }
        }
        __syncthreads();
    }
}

#endif  // __HIPCC__

}  // namespace sitrk
