// sload.h -- scalar loads of wave-uniform, read-only metadata.
// hipcc keeps such loads on the vector pipe (64 lanes fetching one address) because it cannot prove that the kernel's
// stores do not alias them; these issue them on the scalar pipe, a batch at a time with one wait.  The pointers must be
// wave-uniform (SGPR operands).  Outputs are early-clobber: an output must not reuse a pointer's registers.  On the host
// pass of the compiler each helper is the plain load.
#pragma once
#include <hip/hip_runtime.h>

namespace mcml {

typedef int cp_i8 __attribute__((ext_vector_type(8)));
typedef double cp_d8 __attribute__((ext_vector_type(8)));

// eight ints and eight doubles.  Alignment: 4 bytes each (dword / dwordx2 loads)
__device__ __forceinline__ void sload8(const int* ip, const double* dp, int (&iv)[8], double (&dv)[8])
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dword %0, %16, 0x0\n\ts_load_dword %1, %16, 0x4\n\ts_load_dword %2, %16, 0x8\n\ts_load_dword %3, %16, 0xc\n\t"
                 "s_load_dword %4, %16, 0x10\n\ts_load_dword %5, %16, 0x14\n\ts_load_dword %6, %16, 0x18\n\ts_load_dword %7, %16, 0x1c\n\t"
                 "s_load_dwordx2 %8, %17, 0x0\n\ts_load_dwordx2 %9, %17, 0x8\n\ts_load_dwordx2 %10, %17, 0x10\n\ts_load_dwordx2 %11, %17, 0x18\n\t"
                 "s_load_dwordx2 %12, %17, 0x20\n\ts_load_dwordx2 %13, %17, 0x28\n\ts_load_dwordx2 %14, %17, 0x30\n\ts_load_dwordx2 %15, %17, 0x38\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(iv[0]), "=&s"(iv[1]), "=&s"(iv[2]), "=&s"(iv[3]), "=&s"(iv[4]), "=&s"(iv[5]), "=&s"(iv[6]), "=&s"(iv[7]),
                   "=&s"(dv[0]), "=&s"(dv[1]), "=&s"(dv[2]), "=&s"(dv[3]), "=&s"(dv[4]), "=&s"(dv[5]), "=&s"(dv[6]), "=&s"(dv[7])
                 : "s"(ip), "s"(dp) : "memory");
#else
    for (int u = 0; u < 8; ++u) { iv[u] = ip[u]; dv[u] = dp[u]; }
#endif
}
// one double from each of two addresses.  Alignment: 4 bytes (dwordx2)
__device__ __forceinline__ void sload_f64x2(const double* a, const double* b, double& x, double& y)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx2 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(x), "=&s"(y) : "s"(a), "s"(b) : "memory");
#else
    x = *a; y = *b;
#endif
}
// one double.  Alignment: 4 bytes (dwordx2)
__device__ __forceinline__ double sload_f64(const double* a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double x;
    asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(x) : "s"(a) : "memory");
    return x;
#else
    return *a;
#endif
}
// one record of the component plan: 32 + 64 bytes.  Alignment: natural, 32 and 64 bytes (dwordx8 / dwordx16; the records are
// hipMalloc'ed arrays with strides of 32 and 64 bytes)
__device__ __forceinline__ void sload_slot(const int* ip, const double* dp, cp_i8& iv, cp_d8& dv)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx16 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(iv), "=&s"(dv) : "s"(ip), "s"(dp) : "memory");
#else
    for (int u = 0; u < 8; ++u) { iv[u] = ip[u]; dv[u] = dp[u]; }
#endif
}
// two consecutive ints.  Alignment: 4 bytes (two dword loads)
__device__ __forceinline__ void sload_i32x2(const int* p, int& a, int& b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dword %0, %2, 0x0\n\ts_load_dword %1, %2, 0x4\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b) : "s"(p) : "memory");
#else
    a = p[0]; b = p[1];
#endif
}
// one int.  Alignment: 4 bytes
__device__ __forceinline__ int sload_i32(const int* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int a;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a) : "s"(p) : "memory");
    return a;
#else
    return *p;
#endif
}

}  // namespace mcml
