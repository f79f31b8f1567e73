// vecops.hip -- see vecops.h
#include "vecops.h"
#include "reduce.h"

namespace mcml {

// out[0] = (accumulate ? out[0] : 0) + sum(partials[0..n))
__global__ __launch_bounds__(256) void k_sum_partials(const double* partials, int n, double* out, int accumulate)
{
    __shared__ double sh[4];
    double v = 0;
    for (int i = threadIdx.x; i < n; i += 256) v += partials[i];
    double r = block_sum(v, sh);
    if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.0) + r;
}

__global__ __launch_bounds__(256) void k_sumsq(const double* U, int ldu, int rows, int cols, double* partials)
{
    __shared__ double sh[4];
    int i = blockIdx.x * 256 + threadIdx.x;
    double acc = 0;
    if (i < rows)
        for (int j = blockIdx.y; j < cols; j += gridDim.y) {
            double u = U[i + (size_t)j * ldu];
            acc += u * u;
        }
    double r = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = r;
}

// scal[1] = logdet = sum 2 log L_ii (mcmldmatrix.h:67-70)
__global__ __launch_bounds__(256) void k_logdet(const double* A, int lda, int n, double* out)
{
    __shared__ double sh[4];
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += 2 * log(A[i + (size_t)i * lda]);
    double r = block_sum(acc, sh);
    if (threadIdx.x == 0) out[0] = r;
}

// y = A x  (A rows x cols, column-major): one thread per row
__global__ __launch_bounds__(256) void k_gemv_n(const double* A, int lda, int rows, int cols, const double* x,
                                                double* y)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double s = 0;
    for (int j = 0; j < cols; ++j) s += A[i + (size_t)j * lda] * x[j];
    y[i] = s;
}

// y[j] = beta y[j] + alpha sum_i A[i + j lda] x[i]  (A' x): one wave per column
__global__ __launch_bounds__(256) void k_gemv_t(const double* A, int lda, int rows, int cols, const double* x,
                                                double* y, double alpha, double beta)
{
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= cols) return;
    double s = 0;
    for (int i = lane; i < rows; i += 64) s += A[i + (size_t)j * lda] * x[i];
    s = wave_sum(s);
    if (lane == 0) y[j] = (beta != 0.0 ? beta * y[j] : 0.0) + alpha * s;
}

__global__ void k_axpy(double* y, const double* x, double a, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += a * x[i];
}

__global__ void k_copy(double* dst, const double* src, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// AT (cols x rows) = A' through a 32 x 33 LDS tile
__global__ __launch_bounds__(256) void k_transpose_in(const double* A, int lda, int rows, int cols, double* AT, int ldt,
                                                      size_t bsT = 0)
{
    AT += (size_t)blockIdx.z * bsT;            // the same samples under every candidate's matrix
    __shared__ double tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int i = bx + tx, j = by + r;
        tile[r][tx] = (i < rows && j < cols) ? A[i + (size_t)j * lda] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int j = by + tx, i = bx + r;
        if (i < rows && j < cols) AT[j + (size_t)i * ldt] = tile[tx][r];
    }
}

// ------------------------------------------------------------------ launchers
#define VEC_LAUNCH(kernel, grid, block, ...)                                          \
    do {                                                                              \
        hipLaunchKernelGGL(kernel, grid, block, 0, c.stream, __VA_ARGS__);            \
        MCML_HIP(hipGetLastError());                                                  \
        return MCML_OK;                                                               \
    } while (0)

int dev_sum(Ctx& c, const double* x, int n, double* out, bool accumulate)
{
    VEC_LAUNCH(k_sum_partials, dim3(1), dim3(256), x, n, out, accumulate ? 1 : 0);
}

int dev_sumsq_partials(Ctx& c, const double* A, int lda, int rows, int cols, int gx, int gy, double* partials)
{
    VEC_LAUNCH(k_sumsq, dim3(gx, gy), dim3(256), A, lda, rows, cols, partials);
}

int dev_logdet_chol(Ctx& c, const double* A, int lda, int n, double* out)
{
    VEC_LAUNCH(k_logdet, dim3(1), dim3(256), A, lda, n, out);
}

int dev_gemv_n(Ctx& c, const double* A, int lda, int rows, int cols, const double* x, double* y)
{
    VEC_LAUNCH(k_gemv_n, dim3((rows + 255) / 256), dim3(256), A, lda, rows, cols, x, y);
}

int dev_gemv_t(Ctx& c, const double* A, int lda, int rows, int cols, const double* x, double* y, double alpha, double beta)
{
    VEC_LAUNCH(k_gemv_t, dim3((cols + 3) / 4), dim3(256), A, lda, rows, cols, x, y, alpha, beta);
}

int dev_axpy(Ctx& c, double* y, const double* x, double a, int n)
{
    VEC_LAUNCH(k_axpy, dim3((n + 255) / 256), dim3(256), y, x, a, n);
}

int dev_copy(Ctx& c, double* dst, const double* src, int n)
{
    VEC_LAUNCH(k_copy, dim3((n + 127) / 128), dim3(128), dst, src, n);
}

int dev_transpose(Ctx& c, const double* A, int lda, int rows, int cols, double* AT, int ldt, int nbatch, size_t bsT)
{
    VEC_LAUNCH(k_transpose_in, dim3((rows + 31) / 32, (cols + 31) / 32, nbatch), dim3(256), A, lda, rows, cols, AT, ldt, bsT);
}

}  // namespace mcml
