// cov_entry.h -- one entry of a covariance block from the table of covspec.h, on the device.  cov_walk holds the only loop over
// a block's cov rows: the product of the block's terms in the order of the rows, each term by cov_term at the Euclidean distance
// of two points in the term's data columns.  Every form is that walk with its own two points and its own visitor:
//   cov_entry           D_b[i, j], two observed rows: build_dense_body (mvn.hip: mvn_ll, genD, mvn_build_block for predict.hip),
//                       small_block_factor (cov_block.h: k_small_ll, k_small_grad, k_pred_small)
//   cov_cross_entry     C_b[i, j], a new point against an observed row: k_pred_diag, k_pred_small, k_build_cross (predict.hip)
//   cov_prior_variance  the product at distance 0: the variance of a row of an all-gr block (k_diag_prep in mvn_grad.h,
//                       k_diag_fill in mvn.hip) and of a new point (k_pred_diag, k_pred_small, k_pred_cvar)
//   cov_dentry          (d D_b / d theta_par)[i, j]: k_ti_build_dD, k_ti_comp (theta_info.hip)
//   cov_d2entry         (d^2 D_b / d theta_r d theta_s)[i, j]: k_ss_apply (small_sample.hip)
//   grad_entry          (mvn_grad.h) h D_b[i, j] dlog of a window of the block's slots: k_small_grad, k_grad_reduce_large
#pragma once
#include "covspec.h"

namespace mcml {

// the product of the block's terms; diff(c): the difference of the two points in data column c of the block; visit(fn, pi,
// dist) is called after every term, in the order of the rows
template <class Diff, class Visit>
__device__ __forceinline__ double cov_walk(const CovBlock& blk, const int32_t* cov, int rows, const ThetaArg& th, Diff diff,
                                           Visit visit)
{
    double val = 1.0;
    int coff = 0;
    for (int r = blk.r0; r < blk.r1; ++r) {
        const int fn = cov[r + 2 * rows], nv = cov[r + 3 * rows], pi = cov[r + 4 * rows];
        double d2 = 0.0;
        for (int p = 0; p < nv; ++p) {
            double df = diff(coff + p);
            d2 += df * df;
        }
        const double dist = sqrt(d2);
        val = cov_term(fn, dist, &th.v[pi], val);
        visit(fn, pi, dist);
        coff += nv;
    }
    return val;
}

// D_b[i, j]: bd is the block's dim x ncol data matrix, column-major
__device__ __forceinline__ double cov_entry(const CovBlock& blk, const int32_t* cov, int rows,
                                            const double* bd, const ThetaArg& th, int i, int j)
{
    return cov_walk(blk, cov, rows, th, [&](int c) { return bd[i + (size_t)c * blk.dim] - bd[j + (size_t)c * blk.dim]; },
                    [](int, int, double) {});
}

// C_b[i, j]: new point i (row i of xn, knew x ncol column-major, the columns of bd) against observed row j
__device__ __forceinline__ double cov_cross_entry(const CovBlock& blk, const int32_t* cov, int rows, const double* bd,
                                                  const double* xn, int knew, const ThetaArg& th, int i, int j)
{
    return cov_walk(blk, cov, rows, th, [&](int c) { return xn[i + (size_t)c * knew] - bd[j + (size_t)c * blk.dim]; },
                    [](int, int, double) {});
}

// the same product at distance 0: the prior variance of any point of the block, the variance of a row of an all-gr block
// (prod_k theta^2, mcmldmatrix.h:61-65)
__device__ __forceinline__ double cov_prior_variance(const CovBlock& blk, const int32_t* cov, int rows, const ThetaArg& th)
{
    return cov_walk(blk, cov, rows, th, [](int) { return 0.0; }, [](int, int, double) {});
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
    double dl = 0.0;
    const double val = cov_walk(
        blk, cov, rows, th,
        [&](int c) { return blk.all_gr ? 0.0 : bd[i + (size_t)c * blk.dim] - bd[j + (size_t)c * blk.dim]; },   // all gr: not read
        [&](int fn, int pi, double dist) {
            for (int q = 0; q < CovSpec::fn_npar(fn); ++q)
                if (pi + q == par) dl += cov_term_dlog(fn, dist, &th.v[pi], q);
        });
    return val * dl;
}

// d^2 log(term) / d t[q]^2 of the same terms; between two parameters of one term, and between two terms, the second
// log-derivative is 0 (the log of every term is a sum of functions of one parameter each)
__device__ __forceinline__ double cov_term_d2log(int fn, double dist, const double* g, int q)
{
    switch (fn) {
    case 1: return -2.0 / (g[0] * g[0]);
    case 2: return -2.0 * dist / (g[0] * g[0] * g[0]);
    case 3: return -dist / (g[0] * g[0]);
    case 4: return q == 0 ? -1.0 / (g[0] * g[0]) : -6.0 * dist * dist / (g[1] * g[1] * g[1] * g[1]);
    case 7: return q == 0 ? -1.0 / (g[0] * g[0]) : -2.0 * dist / (g[1] * g[1] * g[1]);
    case 14: return -6.0 * dist * dist / (g[0] * g[0] * g[0] * g[0]);
    }
    return 0.0;
}

// (d^2 D_b / d theta_r d theta_s)[i, j] = D_b[i, j] (dl_r dl_s + [r == s] the sum of cov_term_d2log over the slots that read r),
// dl_p the sum of cov_dentry; one walk yields all three.  An all-gr block is diagonal, as in cov_dentry
__device__ __forceinline__ double cov_d2entry(const CovBlock& blk, const int32_t* cov, int rows, const double* bd,
                                              const ThetaArg& th, int i, int j, int r, int s)
{
    if (blk.all_gr && i != j) return 0.0;
    double dlr = 0.0, dls = 0.0, d2 = 0.0;
    const double val = cov_walk(
        blk, cov, rows, th,
        [&](int c) { return blk.all_gr ? 0.0 : bd[i + (size_t)c * blk.dim] - bd[j + (size_t)c * blk.dim]; },
        [&](int fn, int pi, double dist) {
            for (int q = 0; q < CovSpec::fn_npar(fn); ++q) {
                if (pi + q == r) { dlr += cov_term_dlog(fn, dist, &th.v[pi], q); d2 += cov_term_d2log(fn, dist, &th.v[pi], q); }
                if (pi + q == s) dls += cov_term_dlog(fn, dist, &th.v[pi], q);
            }
        });
    return val * (dlr * dls + (r == s ? d2 : 0.0));
}

}  // namespace mcml
