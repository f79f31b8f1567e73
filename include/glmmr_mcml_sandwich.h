/*
 * glmmr_mcml_sandwich.h -- the cluster-robust (sandwich) covariance query of libglmmr_mcml_hip.so (csrc/sandwich.hip): part of
 * the C ABI, included by glmmr_mcml_c.h (include that header; this one relies on its types and error codes).  Beyond the
 * reference's exports: the reference accepts se.method = "robust" and computes what "lik" computes.
 */
#ifndef GLMMR_MCML_SANDWICH_H
#define GLMMR_MCML_SANDWICH_H
#ifndef GLMMR_MCML_C_H
#error "include glmmr_mcml_c.h, which includes this header"
#endif

/* With eta = X beta (no random-effect term), the weights w and Sigma = diag(w) + Z D(theta) Z' of glmmr_mcml_ctx_information:
 *   e_i = (y_i - h(eta_i)) (d eta / d mu)(eta_i)      the working residual; y as the problem gave it (gaussian / log too, where
 *                                                     the samplers and fits read log y as the reference does)
 *   a   = Sigma^-1 e
 *   scores (nullable; ncl x P, leading dimension lds)  G[c, p] = sum over the observations i of cluster c, ascending, of X[i, p] a_i
 *   meat (P x P, leading dimension ldm)                B = G' G, symmetric to the bit
 *   info (P x P, leading dimension ldi)                the bread X' Sigma^-1 X: glmmr_mcml_ctx_information's matrix to the bit
 * The robust covariance is info^-1 meat info^-1, left to the caller (P is small).  Column-major; every sum has a fixed order:
 * two calls return the same bits.
 * cluster: n ids in [0, ncluster), any partition of the observations (Sigma need not be block diagonal over it); null (ncluster
 * is then not read): the connected components of ZL's coupling graph, GLMMR_MCML_EINVAL -- with a message that asks for
 * explicit ids -- where the context does not run the sparse operator (there is no component plan) or some observation has no
 * entry of ZL.  ncluster_out (nullable): the number of clusters, i.e. the component count when cluster is null; with cluster null
 * and scores given, lds must be at least that count.
 * theta and op: as glmmr_mcml_ctx_information (theta null: the resident L, the context is left untouched; given: it is left as
 * update_L(theta) leaves it; op 0 auto, 1 dense, 2 component or GLMMR_MCML_EUNSUPPORTED).  GLMMR_MCML_EINVAL for a null pointer,
 * an id outside [0, ncluster), ncluster < 1, a residual or a weight that is not finite; GLMMR_MCML_ENOTPD for a failed pivot:
 * no output is written.  A query: nothing a later sampler, fit, mvn_ll, information or prediction query reads is changed; no
 * collective is issued.  GLMMR_MCML_SAND_SCORES = wave | wg (environment, read per call) forces the form of the score kernel. */
int glmmr_mcml_ctx_sandwich(glmmr_mcml_ctx* ctx, const double* beta, double var_par, const double* theta, int op,
                            const int* cluster, int ncluster, double* info, int ldi, double* meat, int ldm, double* scores,
                            int lds, int* ncluster_out);
/* the same on a context made for the call (prob->y IS read); theta holds ntheta >= the covariance's parameter count values */
int glmmr_mcml_sandwich(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta, double var_par,
                        int op, const int* cluster, int ncluster, double* info, int ldi, double* meat, int ldm, double* scores,
                        int lds, int* ncluster_out);
/* test hook (csrc/ctx_hooks.hip): out8 = what the last sandwich query on this context was asked for and did: [op requested,
 * operator run (as the information plan: 0 dense, 1 component, 2 component-wide), clusters, rows of the largest cluster, 1 if
 * the default clusters were used, launches of csrc/sandwich.hip's kernels, bytes of the dense matrices (the information
 * plan's), P] */
int glmmr_mcml_dbg_sandwich_plan(glmmr_mcml_ctx* ctx, long long* out8);

#endif
