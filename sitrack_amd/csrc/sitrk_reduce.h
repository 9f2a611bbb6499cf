// sitrk_reduce.h -- the reduction over a workgroup of THREADS lanes (wave64) that the kernels of sitrk_mesh.hip and sitrk_coarse.hip share
#pragma once
#include <hip/hip_runtime.h>

namespace sitrk {

// t[k] over all lanes of the workgroup in a fixed order: the xor butterfly inside a wave, then the waves in order.  Lane k < N
// returns sum k, every other lane 0.  Every lane of the workgroup must call it.
template <int N, int THREADS>
__device__ __forceinline__ double block_sum(double (&t)[N], double (*sm)[N])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; k++) t[k] = t[k] + __shfl_xor(t[k], o);                   // both partners form the same sum
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) sm[wave][k] = t[k];
    }
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x < N) {
        s = sm[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < THREADS / 64; w++) s = s + sm[w][threadIdx.x];
    }
    return s;
}

}  // namespace sitrk
