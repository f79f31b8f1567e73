// cov_block.h -- what the kernels that work on a whole covariance block share, on the device:
//   small_block_factor     a block of dim <= SMALL_BLOCK built by cov_entry and factorised in LDS by one wave: k_small_ll
//                          (mvn.hip), k_small_grad (mvn_grad.h), k_pred_small (predict.hip)
//   small_block_forward    a lane's forward substitution against that factor: the sample columns of the same three kernels and
//                          the rows of the cross-covariance in k_pred_small
//   lower_inverse_column   a column of the inverse of a lower triangle in LDS: k_small_grad, k_ti_comp (theta_info.hip)
//   lower_tile_walk        the (i, j) of a workgroup's 64 x 16 tile of a lower triangle: build_dense_body (mvn.hip),
//                          k_grad_reduce_large (mvn_grad.h), k_ti_build_dD (theta_info.hip)
// The library is compiled without contraction and without fast-math: a kernel that calls a helper performs the helper's
// floating-point operations in the helper's order, so the kernels that share one agree to the bit.
#pragma once
#include <cmath>
#include "chol.h"
#include "cov_entry.h"

namespace mcml {

constexpr double LOG_2PI = 1.8378770664093454835606594728112;   // log(2*M_PI), mcmldmatrix.h:63,75
constexpr int SMALL_LS = SMALL_BLOCK + 1;                       // row stride of a small block in LDS

// ------------------------------------------------------------------ a small block in LDS, one wave of 64 lanes
// S (SMALL_BLOCK x SMALL_LS, lower triangle) = the Cholesky factor of block blk: built entry by entry, then the left-looking
// column Cholesky in the operation order of the CPU oracle.  A pivot that is not positive raises errflag and counts as 1.  Ends
// with a barrier
__device__ __forceinline__ void small_block_factor(double* S, const CovBlock& blk, const int32_t* cov, int rows, const double* bd,
                                                   const ThetaArg& th, int* errflag)
{
    constexpr int LS = SMALL_LS;
    const int dim = blk.dim, lane = threadIdx.x;
    for (int e = lane; e < dim * dim; e += 64) {
        int i = e % dim, j = e / dim;
        if (i >= j) S[i * LS + j] = cov_entry(blk, cov, rows, bd, th, i, j);
    }
    __syncthreads();
    for (int j = 0; j < dim; ++j) {
        if (lane == j) {
            double d = S[j * LS + j];
            for (int k = 0; k < j; ++k) d -= S[j * LS + k] * S[j * LS + k];
            if (!(d > 0.0)) { atomicExch(errflag, 1); d = 1.0; }
            S[j * LS + j] = sqrt(d);
        }
        __syncthreads();
        if (lane > j && lane < dim) {
            double s = S[lane * LS + j];
            for (int k = 0; k < j; ++k) s -= S[lane * LS + k] * S[j * LS + k];
            S[lane * LS + j] = s / S[j * LS + j];
        }
        __syncthreads();
    }
}

// z = inv(L) rhs for the lane's own right-hand side, L the factor in S: Z[i * 64 + lane] = z_i = (rhs(i) - sum_{j < i} L_ij z_j) /
// L_ii (algo::forward_sub, moremaths.h:166-179); returns sum_i z_i^2
template <class Rhs>
__device__ __forceinline__ double small_block_forward(const double* S, int dim, double* Z, int lane, Rhs rhs)
{
    constexpr int LS = SMALL_LS;
    double quad = 0;
    for (int i = 0; i < dim; ++i) {
        double lsum = 0;
        for (int j = 0; j < i; ++j) lsum += S[i * LS + j] * Z[j * 64 + lane];
        double z = (rhs(i) - lsum) / S[i * LS + i];
        Z[i * 64 + lane] = z;
        quad += z * z;
    }
    return quad;
}

// column j of the inverse of the n x n lower triangle T into X, both in LDS with row stride ls: forward substitution, the
// thread reading back what it wrote itself
__device__ __forceinline__ void lower_inverse_column(const double* T, double* X, int ls, int n, int j)
{
    for (int i = j; i < n; ++i) {
        double s = (i == j) ? 1.0 : 0.0;
        for (int k = j; k < i; ++k) s -= T[i * ls + k] * X[k * ls + j];
        X[i * ls + j] = s / T[i * ls + i];
    }
}

// ------------------------------------------------------------------ the lower triangle of a large block, tile by tile
// A workgroup of 256 = 64 rows x 16 columns of a grid (ceil(n / 64), ceil(n / 16)), a wave = the 64 rows of four columns, so
// every load or store of a wave along a column is 512 contiguous bytes (16 x 16 tiles with 128-byte row groups ran 71 us for
// the 5000 x 5000 lower triangle).  f(i, j) for the thread's four entries; a tile strictly above the diagonal returns at once.
// Entries past the matrix and above the diagonal inside a tile are the caller's to skip
template <class F>
__device__ __forceinline__ void lower_tile_walk(F f)
{
    if ((int)blockIdx.x * 64 + 63 < (int)blockIdx.y * 16) return;
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
#pragma unroll
    for (int u = 0; u < 4; ++u) f(i, (int)(blockIdx.y * 16 + (threadIdx.x >> 6) * 4 + u));
}

}  // namespace mcml
