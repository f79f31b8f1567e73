// entry.h -- the host entry points one translation unit defines and another calls: the samplers (hmc.hip), the drivers
// (drivers.hip, laplace.hip), the queries (info.hip, sandwich.hip, predict.hip, theta_info.hip, small_sample.hip) and the launch counters (hmc.hip, component.hip) behind the extern "C" layer (cabi.hip,
// ctx_hooks.hip).  The defining
// files include this header, so a signature that drifts is a compile error, not a wrong link.
#pragma once
#include "../../include/glmmr_mcml_c.h"
#include "ctx.h"
#include <random>

namespace mcml {

// ---- hmc.hip (nuts_sample: nuts.h, part of the same translation unit) ----
int hmc_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed,
               uint32_t iter_idx, const double* inj_init, const double* inj_mom, uint8_t* flags_out,
               double* probs_out, glmmr_mcml_hmc_diag* diag, int* ncols_out);
int nuts_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_nuts_opts* o, uint64_t seed, uint32_t iter_idx,
                int* depth_out, int* nleap_out, double* eps_out, double* accept_out, glmmr_mcml_nuts_diag* diag,
                int* ncols_out);
bool hmc_exact_applicable(const Ctx& c);
int hmc_exact_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed, uint32_t iter_idx,
                     const double* inj_z, glmmr_mcml_hmc_diag* diag, int* ncols_out);
bool hmc_exact_component_applicable(const Ctx& c);
int hmc_exact_component_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed,
                               uint32_t iter_idx, const double* inj_z, glmmr_mcml_hmc_diag* diag, int* ncols_out);
void hmc_exact_component_sizes(const Ctx& c, long long* out3);
long long cm_traj_launch_count();

// ---- drivers.hip ----
int drv_optim(Ctx& c, const double* start, int nstart, int trace, int mcnr, const glmmr_mcml_ext* e,
              double* beta, double* theta, double* sigma);
int drv_simlik(Ctx& c, const double* start, int nstart, int trace, const glmmr_mcml_ext* e, double* beta,
               double* theta, double* sigma);
int drv_hess(Ctx& c, const double* start, int nstart, double tol, int trace, double* H);
int drv_theta_round(Ctx& c, const double* thetas, int k, double* out);
int drv_aic(Ctx& c, const double* beta_par, int nbeta, const double* cov_par, int ncov, double* out);
int drv_full(Ctx& c, const double* start, int nstart, int mcnr, int m, int maxiter, int warmup, double tol,
             int verbose, double lambda, int trace, int refresh, int maxsteps, double target_accept,
             const glmmr_mcml_ext* e, double* beta_out, double* theta_out, double* sigma_out,
             int* converged_out, int* iters_out, glmmr_mcml_hmc_diag* last_diag);

// ---- laplace.hip ----
int drv_la(Ctx& c, const double* start, int nstart, int nr, int usehess, double tol, int verbose, int trace,
           int maxiter, const glmmr_mcml_ext* e, double* beta, double* theta, double* sigma, double* se, double* u,
           int* converged, int* iters);
int drv_la_probe(Ctx& c, const double* start, int nstart, int kind, const double* v, double var_par,
                 const double* par, int npar, double* out, double* v_out, double* beta_out, double* sigma_out);

// ---- component.hip ----
long long la_component_launch_count();

// ---- info.hip ----
// X' (W^-1 + Z D Z')^-1 X at beta / var_par with the context's resident L -> out (P x P, column-major, symmetric to the bit).
// op: 0 the component operator where comp_operator_ready (component.h), else the dense one; 1 dense; 2 component or MCML_EUNSUPPORTED
int info_matrix(Ctx& c, const double* beta, double var_par, int op, double* out, int ldo);
// the dense operator on a context whose operator is the sparse one: the dense ZL / ZL' beside it, built as the Laplace fits' dense
// operator builds them; the sparse pair and the records are not written, so the context's operator is the sparse one again on every exit
struct InfoDenseScope {
    Ctx& c;
    bool on = false;
    explicit InfoDenseScope(Ctx& ctx) : c(ctx) {}
    int build()
    {
        on = true;
        c.no_sparse_zl = true;
        return model_update_L(c);
    }
    ~InfoDenseScope() { if (on) { c.no_sparse_zl = false; c.sp.active = true; } }
};
// the front half the queries on Sigma = diag(w) + Z D Z' share: the weights (c.info.v, c.info.bad) and the factor of
// M = I + ZL' V ZL -- comp: every M_c in c.info.f; else c.info.M factorised on the dense ZL / ZL', which `dense` builds where the
// context's operator is the sparse one.  rhs: info_matrix's right-hand sides ZL' V X into c.info.S on the way
int info_front(Ctx& c, const double* beta, double var_par, bool comp, bool rhs, InfoDenseScope& dense);
// what info_matrix launches behind info_front(rhs): S = R^-1 (ZL' V X) in c.info.S on the operator info_front ran, then gram_launch
// -> c.info.res (P x P and the two flags).  dense_built: `dense` built the dense ZL / ZL' (the plan's byte count)
int info_solve_gram(Ctx& c, bool comp, bool dense_built);
// the chunked Gram reduction, two launches: out[a, b] = out[b, a] = sum_i U[i, a] W[i, b] - sum_q S[q, a] S[q, b], a >= b, over n
// and Q rows in chunks of 2048, the partials in `part`, each sum in a fixed order (Q = 0: no second sum, S is not read); behind
// the P x P matrix ride the two flags of the call: out[P P] = the context's "not positive definite" flag, out[P P + 1] = *bad
int gram_launch(Ctx& c, const double* U, int ldu, const double* W, int ldw, int n, const double* S, int lds, int Q, int P,
                DevBuf& part, const int* bad, double* out);
// the tail of a query whose result gram_launch wrote: h <- the P P + 2 + extra doubles of res, the stream synchronised.  A
// raised not-PD flag is cleared in the context; *bad raised: "<who>: <bad_what> is not finite", MCML_EINVAL; else not-PD:
// MCML_ENOTPD.  The caller copies out only after MCML_OK, so nothing is written on an error
int query_download(Ctx& c, const DevBuf& res, int P, size_t extra, const char* who, const char* bad_what, std::vector<double>& h);
inline void copy_columns(double* dst, int ldd, const double* src, int rows, int cols)
{
    for (int b = 0; b < cols; ++b) memcpy(dst + (size_t)b * ldd, src + (size_t)b * rows, sizeof(double) * (size_t)rows);
}

// ---- sandwich.hip ----
// the bread X' Sigma^-1 X (info_matrix's, to the bit), the meat G' G and, where scores is not null, the ncl x P cluster scores G
// of the working residuals at beta / var_par with the resident L.  cluster: n ids in [0, ncluster), or null for the components of
// the plan (MCML_EINVAL where there is none or an observation has no entry of ZL).  op: as info_matrix.  On an error nothing is written
int sandwich_matrices(Ctx& c, const double* beta, double var_par, int op, const int* cluster, int ncluster, double* info, int ldi,
                      double* meat, int ldm, double* scores, int lds, int* ncluster_out);

// ---- theta_info.hip ----
// the GLS information of the covariance parameters, 1/2 tr(Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma), at beta / var_par / theta with
// the resident L = L(theta) -> out (nout x nout, column-major, symmetric to the bit), *nout = npar, or npar + 1 with the sigma row
// of gaussian / identity.  op: as info_matrix, the component operator where theta_info_component_ok.  On an error nothing is written
int theta_info(Ctx& c, const double* beta, double var_par, const double* theta, int op, double* out, int ldo, int* nout);
// its two halves, for a query that needs I_theta with more (small_sample.hip).  theta_info_begin: the operator for `op` (comp),
// the kernels' theta and every block's parameter mask, c.tinfo.plan started; MCML_EUNSUPPORTED, in `who`'s name, where op = 2
// does not apply.  theta_info_compute, after info_front on the same operator: every launch of the query -> c.tinfo.res (no x no
// and the two flags); B = M^-1 N (c.tinfo.B, dense operator) and the inverted diagonal blocks of L in c.chol.linv stay behind it
constexpr int TI_COMP_MAX_VARS = 64;              // variables of a component the component operator takes
struct ThetaInfoCall {
    ThetaArg th;
    std::vector<unsigned> mask;                   // bit p: block b has a slot that reads parameter p
    int R = 0, sigma_row = 0, no = 0;
    bool comp = false, sparse_ctx = false;
};
bool theta_info_component_ok(const Ctx& c);
int theta_info_begin(Ctx& c, const char* who, const double* theta, int op, ThetaInfoCall& k);
int theta_info_compute(Ctx& c, const ThetaInfoCall& k, double var_par);

// ---- small_sample.hip ----
// I_beta and I_theta (information_matrix's and theta_info's, to the bit) and the P x P matrices of the Kenward-Roger /
// Satterthwaite corrections, P_r (no of them), Q_rs and R_rs (no x no each, index r + no s), at beta / var_par / theta with the
// resident L = L(theta); no = npar, or npar + 1 with sigma last for gaussian / identity.  op: as theta_info.  On an error nothing
// is written
int small_sample(Ctx& c, const double* beta, double var_par, const double* theta, int op, double* info, int ldi, double* tinfo,
                 int ldt, double* Pm, double* Qm, double* Rm, int* nout);

// ---- predict.hip ----
// conditional mean and variance of the random effects at nnew[b] new points per covariance block (newdata: every block's
// k_b x ncol_b matrix, column-major, concatenated) given the resident samples -> summary (K x 3: mean over the samples,
// conditional variance, variance between the samples) and, where means is not null, the K x mcols conditional means
int predict_re(Ctx& c, const double* theta, const int* nnew, const double* newdata, long long newdata_len, double* summary,
               int lds, double* means, int ldm);

// the seed of a sampler run: the caller's, or one from std::random_device as the reference draws it (mhmcmc.h:55)
inline uint64_t default_seed(const glmmr_mcml_ext* e)
{
    if (e && e->seed) return e->seed;
    std::random_device rd;
    return ((uint64_t)rd() << 32) | rd();
}

}  // namespace mcml
