/*
 * glmmr_mcml_info.h -- the GLS information query of libglmmr_mcml_hip.so (csrc/info.hip): part of the C ABI, included by
 * glmmr_mcml_c.h (include that header; this one relies on its types and error codes).  Beyond the reference's exports: the
 * reference leaves information_matrix() to glmmrBase.
 */
#ifndef GLMMR_MCML_INFO_H
#define GLMMR_MCML_INFO_H
#ifndef GLMMR_MCML_C_H
#error "include glmmr_mcml_c.h, which includes this header"
#endif

/* The GLS information matrix of the fixed effects, X' (W^-1 + Z D Z')^-1 X (the caller layer's information_matrix), on the
 * device -> out (P x P, column-major, symmetric to the bit; two calls return the same bits).  W^-1 = diag(w),
 * w_i = dhdmu(x_i' beta) times sigma^2 (gaussian), sigma (gamma), 1 + sigma (beta) or 1, sigma = var_par: NO random-effect
 * term in the linear predictor, y is not read.  By Woodbury with D = L L', V = W: X'VX - S'S, S = R^-1 ZL' V X,
 * R R' = I + ZL' V ZL.
 * theta (nullable): given, the context is first left as update_L with that theta leaves it; null, the resident L is used and
 * the context is left untouched.  Either way the query changes nothing that a later sampler, fit or mvn_ll reads.
 * op: 0 = the component operator (M factorised one connected component of ZL's coupling graph at a time, nothing of size
 * Q x Q or Q x n built) where the context's operator is the sparse one and no component has more than 128 variables, else
 * the dense operator; 1 = dense (on a sparse context the dense ZL / ZL' are built beside the sparse operator);
 * 2 = component, GLMMR_MCML_EUNSUPPORTED where it does not apply.  A weight that is not finite is GLMMR_MCML_EINVAL, a
 * failed pivot GLMMR_MCML_ENOTPD: out is not written.  No collective: every rank of a sharded job answers locally. */
int glmmr_mcml_ctx_information(glmmr_mcml_ctx* ctx, const double* beta, double var_par, const double* theta, int op,
                               double* out, int ldo);
/* the same on a context made for the call (prob->y may be any n values: it is not read); theta holds ntheta >= the
 * covariance's parameter count values */
int glmmr_mcml_information(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta,
                           double var_par, int op, double* out, int ldo);
/* test hook (csrc/ctx_hooks.hip): out8 = what the last information query on this context was asked for and did: [op
 * requested, operator run (0 dense, 1 component: work items of several components per wave, 2 component-wide: a wave per
 * component), components, most variables in one, waves per component of the factor kernel (0 dense, 1, 4), k_lac_factor* +
 * k_comp_solve launches (0 dense), bytes of the dense Q x Q / Q x n matrices the call built -- M, ZLTW, and ZL + ZL' on a
 * sparse context -- (0 component), P] */
int glmmr_mcml_dbg_information_plan(glmmr_mcml_ctx* ctx, long long* out8);

#endif
