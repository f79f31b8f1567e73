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

// d log(term) / d t[q], t = the term's parameters (gr: where dist == 0; the term, and so the product, is 0 elsewhere): the
// derivative of a term is the term times this factor (the score of mvn_grad.h, the information of theta_info.hip)
__device__ __forceinline__ double cov_term_dlog(int fn, double dist, const double* g, int q)
{
    switch (fn) {
    case 1: return 2.0 / g[0];
    case 2: return dist / (g[0] * g[0]);
    case 3: return dist / g[0];
    case 4: return q == 0 ? 1.0 / g[0] : 2.0 * dist * dist / (g[1] * g[1] * g[1]);
    case 7: return q == 0 ? 1.0 / g[0] : dist / (g[1] * g[1]);
    case 14: return 2.0 * dist * dist / (g[0] * g[0] * g[0]);
    }
    return 0.0;
}

// (d D_b / d theta_par)[i, j] = D_b[i, j] * the sum of cov_term_dlog over the slots of the block that read parameter `par` --
// slots numbered term by term, a term's parameters in order, as grad_entry (mvn_grad.h) walks them; a parameter may be read by
// several terms.  An all-gr block is the diagonal matrix mvn.hip makes of it
__device__ __forceinline__ double cov_dentry(const CovBlock& blk, const int32_t* cov, int rows, const double* bd,
                                             const ThetaArg& th, int i, int j, int par)
{
    if (blk.all_gr && i != j) return 0.0;
    double val = 1.0, dl = 0.0;
    int coff = 0;
    for (int r = blk.r0; r < blk.r1; ++r) {
        const int fn = cov[r + 2 * rows], nv = cov[r + 3 * rows], pi = cov[r + 4 * rows];
        double d2 = 0.0;
        if (!blk.all_gr)
            for (int p = 0; p < nv; ++p) {
                double df = bd[i + (size_t)(coff + p) * blk.dim] - bd[j + (size_t)(coff + p) * blk.dim];
                d2 += df * df;
            }
        const double dist = sqrt(d2);
        val = cov_term(fn, dist, &th.v[pi], val);
        const int np = (fn == 4 || fn == 7) ? 2 : 1;
        for (int q = 0; q < np; ++q)
            if (pi + q == par) dl += cov_term_dlog(fn, dist, &th.v[pi], q);
        coff += nv;
    }
    return val * dl;
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
