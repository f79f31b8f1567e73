/*
 * glmmr_mcml_small_sample.h -- the ingredients of the Kenward-Roger / Satterthwaite small-sample corrections of the fixed
 * effects of libglmmr_mcml_hip.so (csrc/small_sample.hip): part of the C ABI, included by glmmr_mcml_c.h (include that header;
 * this one relies on its types and error codes).  Beyond the reference's exports: the reference leaves the corrections to
 * glmmrBase.
 */
#ifndef GLMMR_MCML_SMALL_SAMPLE_H
#define GLMMR_MCML_SMALL_SAMPLE_H
#ifndef GLMMR_MCML_C_H
#error "include glmmr_mcml_c.h, which includes this header"
#endif

/* With Sigma = W^-1 + Z D(theta) Z', the weights of glmmr_mcml_ctx_information at beta / var_par, and no = R (the covariance's
 * parameter count), or R + 1 with sigma = var_par last for gaussian / identity (d_sigma Sigma = 2 sigma I), one call returns
 *     info   (P x P, leading dimension ldi)     X' Sigma^-1 X, the bits of glmmr_mcml_ctx_information on the same operator;
 *     tinfo  (no x no, leading dimension ldt)   the bits of glmmr_mcml_ctx_theta_information;
 *     Pm     (no matrices, P x P each)          P_r  = -X' Sigma^-1 d_r Sigma Sigma^-1 X;
 *     Qm     (no x no matrices, index r + no s) Q_rs =  X' Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma Sigma^-1 X;
 *     Rm     (no x no matrices, index r + no s) R_rs =  X' Sigma^-1 d2_rs Sigma Sigma^-1 X,
 * every matrix column-major, the stacks contiguous; P_r, Q_rr and R_rs are symmetric to the bit, Q_sr is Q_rs transposed, two
 * calls return the same bits; *nout = no.  Pm holds (R + 1) P P doubles at most, Qm and Rm (R + 1)^2 P P.  Computed in the
 * Q x Q form (csrc/small_sample.hip); neither y nor the samples are read.  theta is required and the context is left as
 * update_L with that theta leaves it; the query changes nothing that a later sampler, fit, mvn_ll or information query reads.
 * op and the errors: as glmmr_mcml_ctx_theta_information (0 auto, 1 dense, 2 component or GLMMR_MCML_EUNSUPPORTED; a weight that
 * is not finite GLMMR_MCML_EINVAL; a failed pivot GLMMR_MCML_ENOTPD); on an error no output is written.  No collective. */
int glmmr_mcml_ctx_small_sample(glmmr_mcml_ctx* ctx, const double* beta, double var_par, const double* theta, int op,
                                double* info, int ldi, double* tinfo, int ldt, double* Pm, double* Qm, double* Rm, int* nout);
/* the same on a context made for the call (prob->y may be any n values: it is not read); theta holds ntheta >= the
 * covariance's parameter count values */
int glmmr_mcml_small_sample(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta, double var_par,
                            int op, double* info, int ldi, double* tinfo, int ldt, double* Pm, double* Qm, double* Rm, int* nout);
/* test hook (csrc/ctx_hooks.hip): out8 = what the last small-sample query on this context was asked for and did: [op requested,
 * operator run (0 dense, 1 component), components, most variables in one, launches of the query's own kernels, bytes of the
 * matrices the new part allocated (none of them Q x Q), R, rows returned] */
int glmmr_mcml_dbg_small_sample_plan(glmmr_mcml_ctx* ctx, long long* out8);

#endif
