/*
 * glmmr_mcml_predict.h -- conditional (kriging) prediction of the random effects at new locations (csrc/predict.hip): part
 * of the C ABI, included by glmmr_mcml_c.h (include that header; this one relies on its types and error codes).  Beyond the
 * reference's exports: the reference stops at the samples of the observed random effects.
 */
#ifndef GLMMR_MCML_PREDICT_H
#define GLMMR_MCML_PREDICT_H
#ifndef GLMMR_MCML_C_H
#error "include glmmr_mcml_c.h, which includes this header"
#endif

/* Block b of D(theta) gets nnew[b] >= 0 new points: the rows of a nnew[b] x ncol_b matrix with the columns of the block's
 * data matrix (the `gr` columns included: a new point names its group).  newdata: those matrices, column-major, concatenated
 * in block order, newdata_len values in all.  With C_b the cross-covariance of the new points and the block's random effects,
 * p the prior variance (the block's product at distance 0) and U_b the block's rows of the context's sample columns:
 *   means (nullable; K x mcols, leading dimension ldm, K = sum of nnew)   C_b D_b^-1 U_b, the conditional mean per sample column
 *   summary (K x 3, leading dimension lds)   column 0: the mean of a row of means; column 1: the conditional (kriging)
 *     variance max(p - C_b D_b^-1 C_b', 0); column 2: the variance of that row across the sample columns with divisor
 *     mcols - 1, NaN for one column.  The predictive variance is column 1 + column 2.
 * All-gr blocks are diagonal: a new point that matches a level returns that level's samples to the bit with variance 0, one
 * that matches none 0 and p.  Every sum has a fixed order: two calls, and two contexts, return the same bits.  The locally
 * held sample columns are used and no collective is issued.  A query: nothing a later sampler, fit, mvn_ll, mvn_ll_grad,
 * Laplace call or information query reads is changed.  GLMMR_MCML_EINVAL without samples, for a negative count, for K = 0
 * and for a newdata_len that is not sum_b nnew[b] ncol_b; GLMMR_MCML_ENOTPD for a failed pivot: nothing is written.
 * GLMMR_MCML_PREDICT_CHUNK (environment, read per call) lowers the number of new points worked on at a time. */
int glmmr_mcml_ctx_predict_re(glmmr_mcml_ctx* ctx, const double* theta, const int* nnew, const double* newdata,
                              long long newdata_len, double* summary, int lds, double* means, int ldm);
/* the same on a context made for the call from the covariance and the Q x m sample columns u, as glmmr_mcml_mvn_ll */
int glmmr_mcml_predict_re(const int32_t* cov, int cov_rows, const double* data, int data_len, const double* eff_range,
                          int eff_len, const double* gamma, int ngamma, const double* u, int Q, int m, const int* nnew,
                          const double* newdata, long long newdata_len, double* summary, int lds, double* means, int ldm);
/* test hook (csrc/ctx_hooks.hip): out8 = what the last prediction on this context did: [blocks served by the diagonal path, by
 * the small path, by the large path, K, chunks of new points run, factorisations run by the large path, bytes of the query's
 * workspace, sample columns] */
int glmmr_mcml_dbg_predict_plan(glmmr_mcml_ctx* ctx, long long* out8);

#endif
