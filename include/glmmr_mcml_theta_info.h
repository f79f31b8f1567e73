/*
 * glmmr_mcml_theta_info.h -- the GLS information of the covariance parameters of libglmmr_mcml_hip.so (csrc/theta_info.hip):
 * part of the C ABI, included by glmmr_mcml_c.h (include that header; this one relies on its types and error codes).  Beyond
 * the reference's exports: the reference leaves the standard errors of the covariance parameters to glmmrBase.
 */
#ifndef GLMMR_MCML_THETA_INFO_H
#define GLMMR_MCML_THETA_INFO_H
#ifndef GLMMR_MCML_C_H
#error "include glmmr_mcml_c.h, which includes this header"
#endif

/* The expected (GLS) information of the covariance parameters,
 *     I[r, s] = 1/2 tr(Sigma^-1 d_r Sigma  Sigma^-1 d_s Sigma),   Sigma = W^-1 + Z D(theta) Z',   d_r Sigma = Z (d_r D) Z',
 * on the device -> out (nout x nout, column-major, symmetric to the bit; two calls return the same bits).  W^-1 = diag(w) with
 * the weights of glmmr_mcml_ctx_information at beta / var_par: no random-effect term in the linear predictor, neither y nor
 * the samples are read.  For gaussian / identity W^-1 = sigma^2 I, sigma = var_par is a fitted parameter and the result is the
 * information of (theta, sigma), sigma last: *nout = R + 1; for every other family *nout = R, R = the covariance's
 * parameter count.  Computed in its Q x Q form: with D = L L', M = I + ZL' V ZL = R R', B = I - M^-1 and
 * E_r = L^-1 (d_r D) L^-T, I[r, s] = 1/2 sum_ij (B E_r)_ij (B E_s)_ji.
 * theta is required (a factor installed by set_L carries no parameter values): the context is left as update_L with that
 * theta leaves it, and the query changes nothing that a later sampler, fit, mvn_ll or information query reads.
 * op: 0 = the component operator (one workgroup per connected component of ZL's coupling graph, nothing of size Q x Q built)
 * where the context's operator is the sparse one, no component has more than 64 variables and every covariance block lies
 * inside one component, else the dense operator; 1 = dense (on a sparse context the dense ZL / ZL' are built beside the
 * sparse operator); 2 = component, GLMMR_MCML_EUNSUPPORTED where it does not apply.  A weight that is not finite is
 * GLMMR_MCML_EINVAL; a failed pivot of M, or a D(theta) that is not positive definite, GLMMR_MCML_ENOTPD: out is not written.
 * ldo >= R + 1 always suffices.  No collective: every rank of a sharded job answers locally. */
int glmmr_mcml_ctx_theta_information(glmmr_mcml_ctx* ctx, const double* beta, double var_par, const double* theta, int op,
                                     double* out, int ldo, int* nout);
/* the same on a context made for the call (prob->y may be any n values: it is not read); theta holds ntheta >= the
 * covariance's parameter count values */
int glmmr_mcml_theta_information(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta,
                                 double var_par, int op, double* out, int ldo, int* nout);
/* test hook (csrc/ctx_hooks.hip): out8 = what the last query of the covariance parameters' information on this context was
 * asked for and did: [op requested, operator run (0 dense, 1 component), components, most variables in one, launches of the
 * query's own kernels, bytes of the dense matrices the call built (0 component), R, rows returned] */
int glmmr_mcml_dbg_theta_information_plan(glmmr_mcml_ctx* ctx, long long* out8);

#endif
