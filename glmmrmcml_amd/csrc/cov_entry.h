// cov_entry.h -- one entry of a covariance block from the table of covspec.h, on the device: between two observed rows
// (mvn.hip builds and factorises D with it) and between a new point and an observed row (predict.hip).  Every form
// multiplies the block's terms in the order of the cov rows, each term by cov_term.
#pragma once
#include "covspec.h"

namespace mcml {

// D_b[i, j]: bd is the block's dim x ncol data matrix, column-major
__device__ __forceinline__ double cov_entry(const CovBlock& blk, const int32_t* cov, int rows,
                                            const double* bd, const ThetaArg& th, int i, int j)
{
    double val = 1.0;
    int coff = 0;
    for (int r = blk.r0; r < blk.r1; ++r) {
        const int fn = cov[r + 2 * rows], nv = cov[r + 3 * rows], pi = cov[r + 4 * rows];
        double d2 = 0.0;
        for (int p = 0; p < nv; ++p) {
            double df = bd[i + (size_t)(coff + p) * blk.dim] - bd[j + (size_t)(coff + p) * blk.dim];
            d2 += df * df;
        }
        val = cov_term(fn, sqrt(d2), &th.v[pi], val);
        coff += nv;
    }
    return val;
}

// C_b[i, j]: new point i (row i of xn, knew x ncol column-major, the columns of bd) against observed row j
__device__ __forceinline__ double cov_cross_entry(const CovBlock& blk, const int32_t* cov, int rows, const double* bd,
                                                  const double* xn, int knew, const ThetaArg& th, int i, int j)
{
    double val = 1.0;
    int coff = 0;
    for (int r = blk.r0; r < blk.r1; ++r) {
        const int fn = cov[r + 2 * rows], nv = cov[r + 3 * rows], pi = cov[r + 4 * rows];
        double d2 = 0.0;
        for (int p = 0; p < nv; ++p) {
            double df = xn[i + (size_t)(coff + p) * knew] - bd[j + (size_t)(coff + p) * blk.dim];
            d2 += df * df;
        }
        val = cov_term(fn, sqrt(d2), &th.v[pi], val);
        coff += nv;
    }
    return val;
}

// the same product at distance 0: the prior variance of any point of the block
__device__ __forceinline__ double cov_prior_variance(const CovBlock& blk, const int32_t* cov, int rows, const ThetaArg& th)
{
    double val = 1.0;
    for (int r = blk.r0; r < blk.r1; ++r) val = cov_term(cov[r + 2 * rows], 0.0, &th.v[cov[r + 4 * rows]], val);
    return val;
}

}  // namespace mcml
