// reduce.h -- fixed-order wave / workgroup sums (deterministic: no atomics) and the LDS-only synchronisations.
#pragma once
#include <hip/hip_runtime.h>
namespace mcml {
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;   // lane 0
}
// result valid in thread 0; sh holds blockDim.x/64 doubles
__device__ __forceinline__ double block_sum(double v, double* sh)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
    __syncthreads();
    return r;
}
// the lanes of ONE wave exchange data through LDS: LDS operations of a wave complete in issue order, so only the
// compiler has to be kept from moving them across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// workgroup barrier for LDS traffic only.  __syncthreads() also waits for vmcnt(0): in a kernel that stores to global
// memory as it goes, every barrier would wait for those stores to be acknowledged (~1-2 us each)
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
}  // namespace mcml
