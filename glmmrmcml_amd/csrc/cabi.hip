// cabi.hip -- the extern "C" boundary (include/glmmr_mcml_c.h).
// Lifecycle, samples, queries, model state, samplers, drivers, the opt-in modes, the profile and the host-buffer mirrors of
// the Rcpp exports.  The test hooks (glmmr_mcml_dbg_*) are ctx_hooks.hip and debug_hooks.hip.
#include "entry.h"
#include "hmc_chain.h"
#include <atomic>

using namespace mcml;

// One of the three opt-in modes of a context: its process-wide default, -1 until first asked, then the environment variable
// (read once, at the first get(); a value that is none of `names`, or none at all, is mode 0), and the range check of the
// setters.  names[0] is the mode every context had before the mode existed.
struct Mode {
    int Ctx::*field;
    const char* env;
    const char* names[4];       // names[mode], null after the last
    const char* valid;          // the valid modes as a refusal lists them
    std::atomic<int> dflt{-1};

    int get()
    {
        if (dflt.load() < 0) {
            const char* e = getenv(env);
            int unset = -1, m = 0;
            for (int i = 1; e && names[i]; ++i) if (!strcmp(e, names[i])) m = i;
            dflt.compare_exchange_strong(unset, m);     // a set_default that raced us wins
        }
        return dflt.load();
    }
    int check(const char* fn, bool ok, int mode) const
    {
        int n = 0;
        while (names[n]) ++n;
        MCML_REQUIRE(ok && mode >= 0 && mode < n, "%s: mode must be %s", fn, valid);
        return MCML_OK;
    }
    int set_default(const char* fn, int mode) { MCML_TRY(check(fn, true, mode)); dflt.store(mode); return MCML_OK; }
    int set(const char* fn, glmmr_mcml_ctx* h, int mode) { MCML_TRY(check(fn, h, mode)); h->c.*field = mode; return MCML_OK; }
};
static Mode g_traj{&Ctx::traj_mode, "GLMMR_MCML_TRAJ", {"step", "component"}, "0 (per step) or 1 (component)"};
static Mode g_draws{&Ctx::draws_mode, "GLMMR_MCML_DRAWS", {"hmc", "exact", "exact_component"}, "0 (hmc), 1 (exact) or 2 (exact_component)"};
static Mode g_la{&Ctx::la_mode, "GLMMR_MCML_LA", {"dense", "component", "component_wide"}, "0 (dense), 1 (component) or 2 (component_wide)"};

extern "C" int glmmr_mcml_set_default_trajectory(int mode) { return g_traj.set_default("set_default_trajectory", mode); }
extern "C" int glmmr_mcml_get_default_trajectory(void) { return g_traj.get(); }
extern "C" int glmmr_mcml_ctx_set_trajectory(glmmr_mcml_ctx* h, int mode) { return g_traj.set("set_trajectory", h, mode); }
extern "C" int glmmr_mcml_set_default_draws(int mode) { return g_draws.set_default("set_default_draws", mode); }
extern "C" int glmmr_mcml_get_default_draws(void) { return g_draws.get(); }
extern "C" int glmmr_mcml_ctx_set_draws(glmmr_mcml_ctx* h, int mode) { return g_draws.set("set_draws", h, mode); }
extern "C" int glmmr_mcml_set_default_la_operator(int mode) { return g_la.set_default("set_default_la_operator", mode); }
extern "C" int glmmr_mcml_get_default_la_operator(void) { return g_la.get(); }
extern "C" int glmmr_mcml_ctx_set_la_operator(glmmr_mcml_ctx* h, int mode) { return g_la.set("set_la_operator", h, mode); }

static int flink_of(const char* family, const char* link)
{
    // mcmlmodel.h:74-87 string_to_case
    static const char* tab[12][2] = {
        {"poisson", "log"}, {"poisson", "identity"}, {"binomial", "logit"},
        {"binomial", "log"}, {"binomial", "identity"}, {"binomial", "probit"},
        {"gaussian", "identity"}, {"gaussian", "log"}, {"gamma", "log"},
        {"gamma", "inverse"}, {"gamma", "identity"}, {"beta", "logit"}};
    for (int i = 0; i < 12; i++)
        if (!strcmp(family, tab[i][0]) && !strcmp(link, tab[i][1])) return i + 1;
    return 0;
}

static int link_code_of(const char* link)
{
    // moremaths.h:123-129
    if (!strcmp(link, "log")) return 1;
    if (!strcmp(link, "identity")) return 2;
    if (!strcmp(link, "logit")) return 3;
    if (!strcmp(link, "probit")) return 4;
    if (!strcmp(link, "inverse")) return 5;
    return 0;
}

static int require_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: libglmmr_mcml_hip has no CPU fallback");
        return MCML_ENODEVICE;
    }
    MCML_REQUIRE(device >= 0 && device < ndev, "device %d out of range (%d visible)", device, ndev);
    MCML_HIP(hipSetDevice(device));
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_create(const glmmr_mcml_problem* p, const glmmr_mcml_dev_opts* o,
                                     glmmr_mcml_ctx** out)
{
    MCML_REQUIRE(p && out, "ctx_create: null argument");
    *out = nullptr;
    MCML_TRY(require_device(o ? o->device : 0));
    auto* h = new (std::nothrow) glmmr_mcml_ctx();
    MCML_REQUIRE(h, "out of host memory");
    Ctx& c = h->c;
    auto fail = [&](int rc) { delete h; return rc; };
    c.device = o ? o->device : 0;
    if (o && o->stream) { c.stream = (hipStream_t)o->stream; c.own_stream = false; }
    else {
        hipError_t e = hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking);
        if (e != hipSuccess) { set_error("hipStreamCreate: %s", hipGetErrorString(e)); return fail(MCML_EHIP); }
        c.own_stream = true;
    }
    for (Mode* m : {&g_traj, &g_la, &g_draws}) c.*m->field = m->get();
    c.rank = o ? o->rank : 0;
    c.world = (o && o->world > 0) ? o->world : 1;
    c.reduce = o ? (reduce_fn)o->reduce : nullptr;
    c.reduce_user = o ? o->reduce_user : nullptr;
    int rc = MCML_OK;
    if (p->cov) {
        rc = c.cov.parse(p->cov, p->cov_rows, p->data, p->data_len, p->eff_range, p->eff_len);
        if (rc) return fail(rc);
    } else {
        // no covariance description (export mcmc_sample receives L itself, mcml_full.cpp:315)
        if (p->Q <= 0) { set_error("ctx_create: neither cov nor Q given"); return fail(MCML_EINVAL); }
        c.cov.N = p->Q;
    }
    c.Q = c.cov.N;
    if (p->Q > 0 && p->Q != c.cov.N) {
        set_error("Z has %d columns but the covariance blocks sum to %d", p->Q, c.cov.N);
        return fail(MCML_EINVAL);
    }
    c.n = p->n; c.P = p->P;
    if (p->n > 0) {
        if (!(p->Z && p->X && p->y && p->family && p->link && p->P > 0)) {
            set_error("ctx_create: n > 0 needs Z, X, y, family, link");
            return fail(MCML_EINVAL);
        }
        c.flink = flink_of(p->family, p->link);
        c.link_code = link_code_of(p->link);
        if (!c.flink) {
            set_error("family '%s' with link '%s' is not a known combination", p->family, p->link);
            return fail(MCML_EUNSUPPORTED);
        }
        if ((rc = model_setup(c, p->Z, p->X, p->y))) return fail(rc);
    }
    if ((rc = mvn_setup(c))) return fail(rc);
    *out = h;
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_destroy(glmmr_mcml_ctx* h)
{
    if (!h) return MCML_OK;
    (void)hipSetDevice(h->c.device);
    if (h->c.stream) (void)hipStreamSynchronize(h->c.stream);
    hipStream_t s = h->c.own_stream ? h->c.stream : nullptr;
    delete h;
    if (s) (void)hipStreamDestroy(s);
    return MCML_OK;
}

extern "C" int glmmr_mcml_set_u(glmmr_mcml_ctx* h, const double* u, int Q, int ncols, int niter)
{
    MCML_REQUIRE(h && u, "set_u: null argument");
    Ctx& c = h->c;
    MCML_REQUIRE(Q == c.Q && ncols > 0 && niter > 0 && niter <= ncols, "set_u: bad shape %d x %d (niter %d)", Q, ncols, niter);
    MCML_HIP(hipSetDevice(c.device));
    MCML_TRY(upload_matrix(c.U, u, Q, ncols, Q, c.stream));
    c.mcols = ncols; c.niter = niter;
    c.m_global = ncols; c.niter_global = niter;
    c.zu_valid = false; c.uall_valid = false;
    return c.sync();
}

extern "C" int glmmr_mcml_get_u(glmmr_mcml_ctx* h, double* u, int ldu)
{
    MCML_REQUIRE(h && u, "get_u: null argument");
    Ctx& c = h->c;
    MCML_REQUIRE(c.mcols > 0 && ldu >= c.Q, "get_u: no samples / bad ldu");
    MCML_HIP(hipSetDevice(c.device));
    return download_matrix(u, ldu, c.U.d(), c.U.ld, c.Q, c.mcols, c.stream);
}

extern "C" int glmmr_mcml_get_u_all(glmmr_mcml_ctx* h, double* u, int ldu, int* ncols_out)
{
    MCML_REQUIRE(h && u, "get_u_all: null argument");
    Ctx& c = h->c;
    MCML_REQUIRE(c.mcols > 0 && ldu >= c.Q, "get_u_all: no samples / bad ldu");
    MCML_HIP(hipSetDevice(c.device));
    if (comm_world(c) <= 1) {
        if (ncols_out) *ncols_out = c.mcols;
        return download_matrix(u, ldu, c.U.d(), c.U.ld, c.Q, c.mcols, c.stream);
    }
    MCML_TRY(gather_samples(c));
    if (ncols_out) *ncols_out = c.Uall.cols;
    return download_matrix(u, ldu, c.Uall.d(), c.Uall.ld, c.Q, c.Uall.cols, c.stream);
}

extern "C" int glmmr_mcml_ctx_last_kernels(glmmr_mcml_ctx* h, int* fwd, int* bwd)
{
    MCML_REQUIRE(h, "last_kernels: null context");
    if (fwd) *fwd = h->c.last_kernel[0];
    if (bwd) *bwd = h->c.last_kernel[1];
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_exact_sample(glmmr_mcml_ctx* h, const double* beta, double var_par,
                                           const glmmr_mcml_hmc_opts* opts, uint64_t seed, uint32_t iter_idx,
                                           const double* inj_z, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    MCML_REQUIRE(h && beta && opts, "exact_sample: null argument");
    MCML_HIP(hipSetDevice(h->c.device));
    return hmc_exact_sample(h->c, beta, var_par, opts, seed, iter_idx, inj_z, diag, ncols_out);
}

extern "C" int glmmr_mcml_ctx_exact_component_sample(glmmr_mcml_ctx* h, const double* beta, double var_par,
                                                     const glmmr_mcml_hmc_opts* opts, uint64_t seed, uint32_t iter_idx,
                                                     const double* inj_z, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    MCML_REQUIRE(h && beta && opts, "exact_component_sample: null argument");
    MCML_HIP(hipSetDevice(h->c.device));
    return hmc_exact_component_sample(h->c, beta, var_par, opts, seed, iter_idx, inj_z, diag, ncols_out);
}

extern "C" int glmmr_mcml_ctx_shard_stats(glmmr_mcml_ctx* h, long long* out6)
{
    MCML_REQUIRE(h && out6, "shard_stats: null argument");
    const Ctx& c = h->c;
    out6[0] = c.gather_calls; out6[1] = c.gather_doubles; out6[2] = c.theta_rounds; out6[3] = c.theta_evals_own;
    out6[4] = c.theta_evals_all; out6[5] = c.theta_factorised;
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_mvn_ll(glmmr_mcml_ctx* h, const double* theta, double* out)
{
    MCML_REQUIRE(h && theta && out, "mvn_ll: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    double s = 0;
    MCML_TRY(mvn_loglik_sum(c, theta, &s));
    double tot[2] = {s, (double)c.mcols};
    MCML_TRY(allreduce_host(c, tot, 2));
    *out = tot[0] / tot[1];        // loglV / ncols, mcmldmatrix.h:40
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_mvn_ll_grad(glmmr_mcml_ctx* h, const double* theta, const double* weights, double* value,
                                          double* grad)
{
    MCML_REQUIRE(h && theta && value && grad, "mvn_ll_grad: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    return mvn_loglik_grad(c, theta, weights, value, grad);
}

// conditional prediction at new points (predict.hip): the locally held sample columns, no collective
extern "C" int glmmr_mcml_ctx_predict_re(glmmr_mcml_ctx* h, const double* theta, const int* nnew, const double* newdata,
                                         long long newdata_len, double* summary, int lds, double* means, int ldm)
{
    MCML_REQUIRE(h && theta && nnew && newdata && summary, "predict_re: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    return predict_re(c, theta, nnew, newdata, newdata_len, summary, lds, means, ldm);
}

extern "C" int glmmr_mcml_ctx_mvn_ll_batch(glmmr_mcml_ctx* h, const double* thetas, int k, double* out)
{
    MCML_REQUIRE(h && thetas && out && k >= 1 && k <= 64, "mvn_ll_batch: bad argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_REQUIRE(c.mcols > 0 && c.U.d(), "mvn_ll: no samples set");
    std::vector<double> tot(k + 1, 0.0);
    std::vector<int> rcs(k, 0);
    MCML_TRY(mvn_loglik_batch(c, thetas, k, c.U.d(), c.U.ld, c.mcols, tot.data(), rcs.data()));
    for (int j = 0; j < k; ++j) if (rcs[j] == MCML_ENOTPD) tot[j] = NAN;          // a sum with NaN stays NaN on every rank
    tot[k] = (double)c.mcols;
    MCML_TRY(allreduce_host(c, tot.data(), k + 1));
    for (int j = 0; j < k; ++j) out[j] = tot[j] / tot[k];
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_gen_D(glmmr_mcml_ctx* h, const double* theta, int chol, double* out, int ldo)
{
    MCML_REQUIRE(h && theta && out, "gen_D: null argument");
    Ctx& c = h->c;
    MCML_REQUIRE(ldo >= c.Q, "gen_D: ldo too small");
    MCML_HIP(hipSetDevice(c.device));
    // a query: built in a matrix of its own (off the hot path), the context's L and what was made from it stay in force
    DevMat D;
    MCML_TRY(mvn_gen_D(c, theta, chol != 0, D));
    return download_matrix(out, ldo, D.d(), D.ld, c.Q, c.Q, c.stream);
}

extern "C" int glmmr_mcml_ctx_loglik(glmmr_mcml_ctx* h, const double* beta, double var_par, double* out)
{
    MCML_REQUIRE(h && beta && out, "loglik: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_TRY(model_update_beta(c, beta));
    double s = 0;
    MCML_TRY(model_loglik_sum(c, var_par, &s));
    double tot[2] = {s, (double)c.niter};
    MCML_TRY(allreduce_host(c, tot, 2));
    *out = tot[0] / tot[1];        // ll.mean(), mcmlmodel.h:303
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_mcnr(glmmr_mcml_ctx* h, const double* beta, double var_par,
                                   double* beta_out, double* sigma_out, double* stats_out)
{
    MCML_REQUIRE(h && beta && beta_out && sigma_out, "mcnr: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_TRY(model_update_beta(c, beta));
    std::vector<double> st((size_t)c.P * c.P + c.P + 2);
    MCML_TRY(model_mcnr_stats(c, var_par, st.data()));
    if (stats_out) memcpy(stats_out, st.data(), sizeof(double) * ((size_t)c.P * c.P + c.P + 1));
    return mcnr_finish(c.P, st.data(), beta, beta_out, sigma_out);
}

// c.L is new: the operator made from it (ZL, ZL' or the sparse pair).  If that fails the context holds a new L beside the
// old operator, so it holds no L: the consumers refuse until the next successful update_L / set_L
static int install_L(Ctx& c)
{
    int rc = model_update_L(c);
    if (rc == MCML_OK) rc = c.sync();
    if (rc != MCML_OK) c.have_L = false;
    return rc;
}

extern "C" int glmmr_mcml_ctx_update_L(glmmr_mcml_ctx* h, const double* theta)
{
    MCML_REQUIRE(h && theta, "update_L: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_TRY(mvn_gen_L(c, theta, true));
    return install_L(c);
}

extern "C" int glmmr_mcml_ctx_set_L(glmmr_mcml_ctx* h, const double* L, int ldl)
{
    MCML_REQUIRE(h && L, "set_L: null argument");
    Ctx& c = h->c;
    MCML_REQUIRE(ldl >= c.Q, "set_L: ldl too small");
    MCML_HIP(hipSetDevice(c.device));
    c.have_L = false;
    MCML_TRY(upload_matrix(c.L, L, c.Q, c.Q, ldl, c.stream));
    c.have_L = true;
    // a caller-supplied L need not have the block pattern the sparse ZL operator assumes (entries outside the
    // covariance blocks would be dropped): the dense products take whatever L holds
    c.l_foreign = true;
    return install_L(c);
}

// the GLS information of the fixed effects (info.hip).  theta: the context is first brought to where update_L(theta) leaves it
extern "C" int glmmr_mcml_ctx_information(glmmr_mcml_ctx* h, const double* beta, double var_par, const double* theta, int op,
                                          double* out, int ldo)
{
    MCML_REQUIRE(h && beta && out, "information: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    if (theta) {
        MCML_REQUIRE(c.n > 0 && c.cov.npar > 0, "information: the context has no model / covariance");
        MCML_TRY(mvn_gen_L(c, theta, true));
        MCML_TRY(install_L(c));
    }
    return info_matrix(c, beta, var_par, op, out, ldo);
}

// the GLS information of the covariance parameters (theta_info.hip).  theta is required: the query needs the parameter values,
// and the context is left as update_L(theta) leaves it
extern "C" int glmmr_mcml_ctx_theta_information(glmmr_mcml_ctx* h, const double* beta, double var_par, const double* theta, int op,
                                                double* out, int ldo, int* nout)
{
    MCML_REQUIRE(h && beta && theta && out && nout, "theta_information: null argument (theta is required)");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_REQUIRE(c.n > 0 && c.cov.npar > 0, "theta_information: the context has no model / covariance");
    MCML_TRY(mvn_gen_L(c, theta, true));
    MCML_TRY(install_L(c));
    return theta_info(c, beta, var_par, theta, op, out, ldo, nout);
}

// the ingredients of the small-sample corrections (small_sample.hip).  theta is required, as for the query above
extern "C" int glmmr_mcml_ctx_small_sample(glmmr_mcml_ctx* h, const double* beta, double var_par, const double* theta, int op,
                                           double* info, int ldi, double* tinfo, int ldt, double* Pm, double* Qm, double* Rm,
                                           int* nout)
{
    MCML_REQUIRE(h && beta && theta && info && tinfo && Pm && Qm && Rm && nout, "small_sample: null argument (theta is required)");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_REQUIRE(c.n > 0 && c.cov.npar > 0, "small_sample: the context has no model / covariance");
    MCML_TRY(mvn_gen_L(c, theta, true));
    MCML_TRY(install_L(c));
    return small_sample(c, beta, var_par, theta, op, info, ldi, tinfo, ldt, Pm, Qm, Rm, nout);
}

// the cluster-robust sandwich of the fixed effects (sandwich.hip).  theta: as glmmr_mcml_ctx_information
extern "C" int glmmr_mcml_ctx_sandwich(glmmr_mcml_ctx* h, const double* beta, double var_par, const double* theta, int op,
                                       const int* cluster, int ncluster, double* info, int ldi, double* meat, int ldm,
                                       double* scores, int lds, int* ncluster_out)
{
    MCML_REQUIRE(h && beta && info && meat, "sandwich: null argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    if (theta) {
        MCML_REQUIRE(c.n > 0 && c.cov.npar > 0, "sandwich: the context has no model / covariance");
        MCML_TRY(mvn_gen_L(c, theta, true));
        MCML_TRY(install_L(c));
    }
    return sandwich_matrices(c, beta, var_par, op, cluster, ncluster, info, ldi, meat, ldm, scores, lds, ncluster_out);
}

extern "C" int glmmr_mcml_ctx_hmc_sample(glmmr_mcml_ctx* h, const double* beta, double var_par,
                                         const glmmr_mcml_hmc_opts* opts, uint64_t seed, uint32_t iter_idx,
                                         const double* inj_init, const double* inj_mom, uint8_t* flags_out,
                                         double* probs_out, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    MCML_REQUIRE(h && beta && opts, "hmc_sample: null argument");
    MCML_HIP(hipSetDevice(h->c.device));
    return hmc_sample(h->c, beta, var_par, opts, seed, iter_idx, inj_init, inj_mom, flags_out, probs_out,
                      diag, ncols_out);
}

extern "C" int glmmr_mcml_ctx_nuts_sample(glmmr_mcml_ctx* h, const double* beta, double var_par,
                                          const glmmr_mcml_nuts_opts* opts, uint64_t seed, uint32_t iter_idx,
                                          int* depth_out, int* nleap_out, double* eps_out, double* accept_out,
                                          glmmr_mcml_nuts_diag* diag, int* ncols_out)
{
    MCML_REQUIRE(h && beta && opts, "nuts_sample: null argument");
    MCML_HIP(hipSetDevice(h->c.device));
    return nuts_sample(h->c, beta, var_par, opts, seed, iter_idx, depth_out, nleap_out, eps_out, accept_out, diag,
                       ncols_out);
}

// ------------------------------------------------------------------------- drivers
extern "C" int glmmr_mcml_sample_cols(int m, int chains)
{
    return m <= 0 ? 0 : sample_shape(m, 0, chains).ncols;
}

// kernel timing (HIP events on the context's stream).
// out8: [fwd_ms, fwd_count, bwd_ms, bwd_count, executed flops per forward launch, per backward
// launch, dense flops per launch (2 n Q C), operator kind (0 dense GEMM, 1 banded GEMM, 2 sparse)]
extern "C" int glmmr_mcml_ctx_profile(glmmr_mcml_ctx* h, int enable, int reset, double* out8)
{
    MCML_REQUIRE(h, "profile: null context");
    Ctx& c = h->c;
    KernelProf& p = c.prof;
    if (out8) {
        out8[0] = p.ms[0]; out8[1] = (double)p.cnt[0]; out8[2] = p.ms[1]; out8[3] = (double)p.cnt[1];
        const double C = (double)c.hmc.C, dense = 2.0 * c.n * (double)c.Q * C;
        double ff = dense, fb = dense, kind = 0;
        if (c.sp.active) { ff = fb = 2.0 * (double)c.sp.nnz * C; kind = 2; }
        else {
            // the MFMAs issued (band_plan.h: inside the row-tile extents), 2 * 16 * 16 * 4 flop each, C / 16 strips
            const bool rt = band_rowtiles_enabled();
            if (c.band_fwd) { ff = 2.0 * 16.0 * 4.0 * (double)c.plan_fwd.issued(rt) * C; kind = 1; }
            if (c.band_bwd) { fb = 2.0 * 16.0 * 4.0 * (double)c.plan_bwd.issued(rt) * C; kind = 1; }
        }
        out8[4] = ff; out8[5] = fb; out8[6] = dense; out8[7] = kind;
    }
    if (reset) for (int i = 0; i < 4; ++i) { p.ms[i] = 0; p.cnt[i] = 0; p.seen[i] = 0; }
    if (enable && !p.on) {
        // the markers' events are made HERE, not at their first use inside whatever is being timed: a sampler call of
        // 100 proposals records ~1000 of them, and creating those on the fly cost the first timed MCML iteration of a
        // small configuration 20-75 ms (config 4 in bench.py: 45 or 70 ms per iteration from one process to the next)
        MCML_HIP(hipSetDevice(c.device));
        while (p.ev.size() < 4096) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); break; } p.ev.push_back(e); }
    }
    p.on = enable != 0;
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_profile_launches(glmmr_mcml_ctx* h, long long* fwd, long long* bwd)
{
    MCML_REQUIRE(h, "profile_launches: null context");
    if (fwd) *fwd = h->c.prof.seen[0];
    if (bwd) *bwd = h->c.prof.seen[1];
    return MCML_OK;
}

extern "C" int glmmr_mcml_ctx_ncols(glmmr_mcml_ctx* h) { return h ? h->c.mcols : 0; }
extern "C" int glmmr_mcml_ctx_npar(glmmr_mcml_ctx* h) { return h ? h->c.cov.npar : 0; }

extern "C" int glmmr_mcml_ctx_optim(glmmr_mcml_ctx* h, const double* start, int nstart, int trace, int mcnr,
                                    const glmmr_mcml_ext* ext, double* beta, double* theta, double* sigma)
{
    MCML_REQUIRE(h && start && beta && theta && sigma, "optim: null argument");
    MCML_REQUIRE(h->c.n > 0, "optim: context has no model");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_optim(h->c, start, nstart, trace, mcnr, ext, beta, theta, sigma);
}

extern "C" int glmmr_mcml_ctx_simlik(glmmr_mcml_ctx* h, const double* start, int nstart, int trace,
                                     const glmmr_mcml_ext* ext, double* beta, double* theta, double* sigma)
{
    MCML_REQUIRE(h && start && beta && theta && sigma, "simlik: null argument");
    MCML_REQUIRE(h->c.n > 0, "simlik: context has no model");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_simlik(h->c, start, nstart, trace, ext, beta, theta, sigma);
}

extern "C" int glmmr_mcml_ctx_hess(glmmr_mcml_ctx* h, const double* start, int nstart, double tol, int trace,
                                   double* H)
{
    MCML_REQUIRE(h && start && H, "hess: null argument");
    MCML_REQUIRE(h->c.n > 0 && tol > 0, "hess: context has no model / bad tol");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_hess(h->c, start, nstart, tol, trace, H);
}

extern "C" int glmmr_mcml_ctx_aic(glmmr_mcml_ctx* h, const double* beta_par, int nbeta, const double* cov_par,
                                  int ncov, double* out)
{
    MCML_REQUIRE(h && beta_par && cov_par && out, "aic: null argument");
    MCML_REQUIRE(h->c.n > 0, "aic: context has no model");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_aic(h->c, beta_par, nbeta, cov_par, ncov, out);
}

extern "C" int glmmr_mcml_ctx_full(glmmr_mcml_ctx* h, const double* start, int nstart, int mcnr, int m,
                                   int maxiter, int warmup, double tol, int verbose, double lambda, int trace,
                                   int refresh, int maxsteps, double target_accept, const glmmr_mcml_ext* ext,
                                   double* beta, double* theta, double* sigma, int* converged, int* iters,
                                   glmmr_mcml_hmc_diag* diag)
{
    MCML_REQUIRE(h && start && beta && theta && sigma, "mcml_full: null argument");
    MCML_REQUIRE(h->c.n > 0, "mcml_full: context has no model");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_full(h->c, start, nstart, mcnr, m, maxiter, warmup, tol, verbose, lambda, trace, refresh, maxsteps,
                    target_accept, ext, beta, theta, sigma, converged, iters, diag);
}

// Laplace-approximation fits (src/mcml_la.cpp): nr = 0 mcml_la, 1 mcml_la_nr
extern "C" int glmmr_mcml_ctx_la(glmmr_mcml_ctx* h, const double* start, int nstart, int nr, int usehess, double tol,
                                 int verbose, int trace, int maxiter, const glmmr_mcml_ext* ext, double* beta,
                                 double* theta, double* sigma, double* se, double* u, int* converged, int* iters)
{
    MCML_REQUIRE(h && start && beta && theta && sigma, "mcml_la: null argument");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_la(h->c, start, nstart, nr, usehess, tol, verbose, trace, maxiter, ext, beta, theta, sigma, se, u,
                  converged, iters);
}

// ---- host-buffer mirrors of the Rcpp exports: each on a context made for the call ----
namespace {
struct CtxGuard {
    glmmr_mcml_ctx* h = nullptr;
    ~CtxGuard() { if (h) glmmr_mcml_ctx_destroy(h); }
};
int open_ctx(const glmmr_mcml_problem* prob, const glmmr_mcml_ext* ext, CtxGuard& g)
{
    glmmr_mcml_dev_opts o{};
    o.device = ext ? ext->device : 0; o.world = 1;
    return glmmr_mcml_ctx_create(prob, &o, &g.h);
}
// the sparse exports pass the CSC pattern (Ap, Ai) of D (R6ModelExtMCML.R:193-195); D is
// block diagonal, so the pattern must fit inside the blocks the cov matrix describes
struct Pattern { const int32_t *Ap, *Ai; int nnz; };
int check_pattern(const Ctx& c, const Pattern& s)
{
    const int32_t *Ap = s.Ap, *Ai = s.Ai;
    MCML_REQUIRE(Ap && Ai && s.nnz >= 0, "sparse: null pattern");
    std::vector<int> blk(c.Q);
    for (int b = 0; b < c.cov.B; ++b) for (int k = 0; k < c.cov.blocks[b].dim; ++k) blk[c.cov.blocks[b].matstart + k] = b;
    MCML_REQUIRE(Ap[0] == 0 && Ap[c.Q] == s.nnz, "sparse: Ap does not describe %d columns / %d entries", c.Q, s.nnz);
    for (int j = 0; j < c.Q; ++j)
        for (int p = Ap[j]; p < Ap[j + 1]; ++p) {
            MCML_REQUIRE(Ai[p] >= 0 && Ai[p] < c.Q, "sparse: row index out of range");
            MCML_REQUIRE(blk[Ai[p]] == blk[j], "sparse: entry (%d,%d) lies outside the covariance blocks", Ai[p], j);
        }
    return MCML_OK;
}
// the fit mirrors: the problem on ext's device with the samples u; pattern: the _sparse exports, checked before u goes down
int open_fit(const glmmr_mcml_problem* prob, const glmmr_mcml_ext* ext, const Pattern* pattern, const double* u, int ucols,
             CtxGuard& g)
{
    MCML_TRY(open_ctx(prob, ext, g));
    if (pattern) MCML_TRY(check_pattern(g.h->c, *pattern));
    return glmmr_mcml_set_u(g.h, u, prob->Q, ucols, ucols);
}
// mvn_ll / mvn_ll_grad (`fn`): the covariance alone, no model, with the m sample columns u
int open_cov(const char* fn, const int32_t* cov, int cov_rows, const double* data, int data_len, const double* eff_range,
             int eff_len, int ngamma, const double* u, int Q, int m, CtxGuard& g)
{
    glmmr_mcml_problem p{};
    p.cov = cov; p.cov_rows = cov_rows; p.data = data; p.data_len = data_len;
    p.eff_range = eff_range; p.eff_len = eff_len; p.Q = Q;
    MCML_TRY(open_ctx(&p, nullptr, g));
    const int npar = g.h->c.cov.npar;
    MCML_REQUIRE(ngamma >= npar, "%s: %d covariance parameters given, the functions need %d", fn, ngamma, npar);
    return glmmr_mcml_set_u(g.h, u, Q, m, m);
}
// mcmc_sample / gen_u_samples: the model with the caller's L in place of a covariance, and the seed of the run
int open_sampler(const double* Z, const double* L, const double* X, const double* y, int n, int Q, int P, const char* family,
                 const char* link, const glmmr_mcml_ext* ext, CtxGuard& g, uint64_t* seed)
{
    glmmr_mcml_problem p{};
    p.Z = Z; p.X = X; p.y = y; p.n = n; p.Q = Q; p.P = P; p.family = family; p.link = link;
    MCML_TRY(open_ctx(&p, ext, g));
    MCML_TRY(glmmr_mcml_ctx_set_L(g.h, L, Q));
    *seed = default_seed(ext);
    return MCML_OK;
}
}  // namespace

extern "C" int glmmr_mcml_mvn_ll(const int32_t* cov, int cov_rows, const double* data, int data_len,
                                 const double* eff_range, int eff_len, const double* gamma, int ngamma,
                                 const double* u, int Q, int m, double* out)
{
    CtxGuard g;
    MCML_TRY(open_cov("mvn_ll", cov, cov_rows, data, data_len, eff_range, eff_len, ngamma, u, Q, m, g));
    return glmmr_mcml_ctx_mvn_ll(g.h, gamma, out);
}

extern "C" int glmmr_mcml_mvn_ll_grad(const int32_t* cov, int cov_rows, const double* data, int data_len,
                                      const double* eff_range, int eff_len, const double* gamma, int ngamma,
                                      const double* u, int Q, int m, const double* weights, double* value, double* grad)
{
    CtxGuard g;
    MCML_TRY(open_cov("mvn_ll_grad", cov, cov_rows, data, data_len, eff_range, eff_len, ngamma, u, Q, m, g));
    MCML_TRY(glmmr_mcml_ctx_mvn_ll_grad(g.h, gamma, weights, value, grad));
    for (int k = g.h->c.cov.npar; k < ngamma; ++k) grad[k] = 0.0;
    return MCML_OK;
}

extern "C" int glmmr_mcml_predict_re(const int32_t* cov, int cov_rows, const double* data, int data_len,
                                     const double* eff_range, int eff_len, const double* gamma, int ngamma, const double* u,
                                     int Q, int m, const int* nnew, const double* newdata, long long newdata_len,
                                     double* summary, int lds, double* means, int ldm)
{
    MCML_REQUIRE(cov && data && gamma && u && nnew && newdata && summary, "predict_re: null argument");
    CtxGuard g;
    MCML_TRY(open_cov("predict_re", cov, cov_rows, data, data_len, eff_range, eff_len, ngamma, u, Q, m, g));
    return glmmr_mcml_ctx_predict_re(g.h, gamma, nnew, newdata, newdata_len, summary, lds, means, ldm);
}

extern "C" int glmmr_mcml_optim(const glmmr_mcml_problem* prob, const double* u, int ucols, const double* start,
                                int nstart, int trace, int mcnr, const glmmr_mcml_ext* ext, double* beta,
                                double* theta, double* sigma)
{
    CtxGuard g;
    MCML_TRY(open_fit(prob, ext, nullptr, u, ucols, g));
    return glmmr_mcml_ctx_optim(g.h, start, nstart, trace, mcnr, ext, beta, theta, sigma);
}

extern "C" int glmmr_mcml_simlik(const glmmr_mcml_problem* prob, const double* u, int ucols, const double* start,
                                 int nstart, int trace, const glmmr_mcml_ext* ext, double* beta, double* theta,
                                 double* sigma)
{
    CtxGuard g;
    MCML_TRY(open_fit(prob, ext, nullptr, u, ucols, g));
    return glmmr_mcml_ctx_simlik(g.h, start, nstart, trace, ext, beta, theta, sigma);
}

// LDL' factor of the block-diagonal D(theta) in the layout SparseChol hands back
// (mcml_optim.cpp:180-182: chol_->L->{Ap,Ai,Ax}, chol_->D): L unit lower triangular stored
// column-compressed WITHOUT its diagonal, D the pivots; chol(D) = L * diag(sqrt(D)).
// From the dense block factors: L_ldl = L_chol * diag(1 / diag(L_chol)), D = diag(L_chol)^2.
static int sparse_factor_nnz(const CovSpec& cs)
{
    long nnz = 0;
    for (const auto& b : cs.blocks) if (!b.all_gr) nnz += (long)b.dim * (b.dim - 1) / 2;
    return (int)nnz;
}

extern "C" int glmmr_mcml_sparse_factor_nnz(const int32_t* cov, int cov_rows, const double* data, int data_len)
{
    CovSpec cs;
    return cs.parse(cov, cov_rows, data, data_len, nullptr, 0) ? -1 : sparse_factor_nnz(cs);
}

static int sparse_factor(Ctx& c, const double* theta, int32_t* Lp, int32_t* Li, double* Lx, double* D)
{
    MCML_TRY(mvn_gen_L(c, theta, true));
    std::vector<double> blk;
    int nz = 0;
    for (const auto& b : c.cov.blocks) {
        blk.assign((size_t)b.dim * b.dim, 0.0);
        MCML_TRY(download_matrix(blk.data(), b.dim, c.L.at(b.matstart, b.matstart), c.L.ld, b.dim, b.dim, c.stream));
        for (int j = 0; j < b.dim; ++j) {
            const double d = blk[j + (size_t)j * b.dim];
            Lp[b.matstart + j] = nz;
            D[b.matstart + j] = d * d;
            if (!b.all_gr)
                for (int i = j + 1; i < b.dim; ++i) { Li[nz] = b.matstart + i; Lx[nz] = blk[i + (size_t)j * b.dim] / d; ++nz; }
        }
    }
    Lp[c.Q] = nz;
    return MCML_OK;
}

extern "C" int glmmr_mcml_optim_sparse(const glmmr_mcml_problem* prob, const int32_t* Ap, const int32_t* Ai,
                                       int nnz, const double* u, int ucols, const double* start, int nstart,
                                       int trace, int mcnr, const glmmr_mcml_ext* ext, double* beta, double* theta,
                                       double* sigma, int32_t* Lp, int32_t* Li, double* Lx, double* D, int lcap)
{
    CtxGuard g;
    const Pattern pattern{Ap, Ai, nnz};
    MCML_TRY(open_fit(prob, ext, &pattern, u, ucols, g));
    MCML_TRY(glmmr_mcml_ctx_optim(g.h, start, nstart, trace, mcnr, ext, beta, theta, sigma));
    if (Lp && Li && Lx && D) {
        const int need = sparse_factor_nnz(g.h->c.cov);
        MCML_REQUIRE(lcap >= need, "optim_sparse: factor needs %d entries, %d given", need, lcap);
        MCML_TRY(sparse_factor(g.h->c, theta, Lp, Li, Lx, D));
    }
    return MCML_OK;
}

extern "C" int glmmr_mcml_simlik_sparse(const glmmr_mcml_problem* prob, const int32_t* Ap, const int32_t* Ai,
                                        int nnz, const double* u, int ucols, const double* start, int nstart,
                                        int trace, const glmmr_mcml_ext* ext, double* beta, double* theta,
                                        double* sigma)
{
    CtxGuard g;
    const Pattern pattern{Ap, Ai, nnz};
    MCML_TRY(open_fit(prob, ext, &pattern, u, ucols, g));
    return glmmr_mcml_ctx_simlik(g.h, start, nstart, trace, ext, beta, theta, sigma);
}

extern "C" int glmmr_mcml_hess(const glmmr_mcml_problem* prob, const double* u, int ucols, const double* start,
                               int nstart, double tol, int trace, const glmmr_mcml_ext* ext, double* H)
{
    CtxGuard g;
    MCML_TRY(open_fit(prob, ext, nullptr, u, ucols, g));
    return glmmr_mcml_ctx_hess(g.h, start, nstart, tol, trace, H);
}

extern "C" int glmmr_mcml_hess_sparse(const glmmr_mcml_problem* prob, const int32_t* Ap, const int32_t* Ai,
                                      int nnz, const double* u, int ucols, const double* start, int nstart,
                                      double tol, int trace, const glmmr_mcml_ext* ext, double* H)
{
    CtxGuard g;
    const Pattern pattern{Ap, Ai, nnz};
    MCML_TRY(open_fit(prob, ext, &pattern, u, ucols, g));
    return glmmr_mcml_ctx_hess(g.h, start, nstart, tol, trace, H);
}

extern "C" int glmmr_mcml_aic(const glmmr_mcml_problem* prob, const double* u, int ucols, const double* beta_par,
                              int nbeta, const double* cov_par, int ncov, const glmmr_mcml_ext* ext, double* out)
{
    CtxGuard g;
    MCML_TRY(open_fit(prob, ext, nullptr, u, ucols, g));
    return glmmr_mcml_ctx_aic(g.h, beta_par, nbeta, cov_par, ncov, out);
}

extern "C" int glmmr_mcml_full(const glmmr_mcml_problem* prob, const double* start, int nstart, int mcnr, int m,
                               int maxiter, int warmup, double tol, int verbose, double lambda, int trace,
                               int refresh, int maxsteps, double target_accept, const glmmr_mcml_ext* ext,
                               double* beta, double* theta, double* sigma, int* converged, double* u, int ldu,
                               int* ucols)
{
    CtxGuard g;
    MCML_TRY(open_ctx(prob, ext, g));
    int iters = 0;
    MCML_TRY(glmmr_mcml_ctx_full(g.h, start, nstart, mcnr, m, maxiter, warmup, tol, verbose, lambda, trace, refresh,
                                 maxsteps, target_accept, ext, beta, theta, sigma, converged, &iters, nullptr));
    if (ucols) *ucols = g.h->c.mcols;
    if (u) MCML_TRY(glmmr_mcml_get_u(g.h, u, ldu));
    return MCML_OK;
}

extern "C" int glmmr_mcml_la(const glmmr_mcml_problem* prob, const double* start, int nstart, int usehess, double tol,
                             int verbose, int trace, int maxiter, const glmmr_mcml_ext* ext, double* beta,
                             double* theta, double* sigma, double* se, double* u)
{
    CtxGuard g;
    MCML_TRY(open_ctx(prob, ext, g));
    return glmmr_mcml_ctx_la(g.h, start, nstart, 0, usehess, tol, verbose, trace, maxiter, ext, beta, theta, sigma, se,
                             u, nullptr, nullptr);
}

extern "C" int glmmr_mcml_la_nr(const glmmr_mcml_problem* prob, const double* start, int nstart, int usehess,
                                double tol, int verbose, int trace, int maxiter, const glmmr_mcml_ext* ext,
                                double* beta, double* theta, double* sigma, double* se, double* u)
{
    CtxGuard g;
    MCML_TRY(open_ctx(prob, ext, g));
    return glmmr_mcml_ctx_la(g.h, start, nstart, 1, usehess, tol, verbose, trace, maxiter, ext, beta, theta, sigma, se,
                             u, nullptr, nullptr);
}

extern "C" int glmmr_mcml_information(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta,
                                      double var_par, int op, double* out, int ldo)
{
    MCML_REQUIRE(prob && beta && theta && out, "information: null argument");
    CtxGuard g;
    MCML_TRY(open_ctx(prob, nullptr, g));
    MCML_REQUIRE(ntheta >= g.h->c.cov.npar, "information: %d covariance parameters given, the covariance needs %d", ntheta,
                 g.h->c.cov.npar);
    return glmmr_mcml_ctx_information(g.h, beta, var_par, theta, op, out, ldo);
}

extern "C" int glmmr_mcml_theta_information(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta,
                                            double var_par, int op, double* out, int ldo, int* nout)
{
    MCML_REQUIRE(prob && beta && theta && out && nout, "theta_information: null argument");
    CtxGuard g;
    MCML_TRY(open_ctx(prob, nullptr, g));
    MCML_REQUIRE(ntheta >= g.h->c.cov.npar, "theta_information: %d covariance parameters given, the covariance needs %d", ntheta,
                 g.h->c.cov.npar);
    return glmmr_mcml_ctx_theta_information(g.h, beta, var_par, theta, op, out, ldo, nout);
}

extern "C" int glmmr_mcml_small_sample(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta,
                                       double var_par, int op, double* info, int ldi, double* tinfo, int ldt, double* Pm,
                                       double* Qm, double* Rm, int* nout)
{
    MCML_REQUIRE(prob && beta && theta && info && tinfo && Pm && Qm && Rm && nout, "small_sample: null argument");
    CtxGuard g;
    MCML_TRY(open_ctx(prob, nullptr, g));
    MCML_REQUIRE(ntheta >= g.h->c.cov.npar, "small_sample: %d covariance parameters given, the covariance needs %d", ntheta,
                 g.h->c.cov.npar);
    return glmmr_mcml_ctx_small_sample(g.h, beta, var_par, theta, op, info, ldi, tinfo, ldt, Pm, Qm, Rm, nout);
}

extern "C" int glmmr_mcml_sandwich(const glmmr_mcml_problem* prob, const double* beta, const double* theta, int ntheta,
                                   double var_par, int op, const int* cluster, int ncluster, double* info, int ldi, double* meat,
                                   int ldm, double* scores, int lds, int* ncluster_out)
{
    MCML_REQUIRE(prob && beta && theta && info && meat, "sandwich: null argument");
    CtxGuard g;
    MCML_TRY(open_ctx(prob, nullptr, g));
    MCML_REQUIRE(ntheta >= g.h->c.cov.npar, "sandwich: %d covariance parameters given, the covariance needs %d", ntheta,
                 g.h->c.cov.npar);
    return glmmr_mcml_ctx_sandwich(g.h, beta, var_par, theta, op, cluster, ncluster, info, ldi, meat, ldm, scores, lds,
                                   ncluster_out);
}

extern "C" int glmmr_mcml_mcmc_sample(const double* Z, const double* L, const double* X, const double* y, int n,
                                      int Q, int P, const double* beta, const char* family, const char* link,
                                      int warmup, int nsamp, double lambda, double var_par, int trace, int refresh,
                                      int maxsteps, double target_accept, const glmmr_mcml_ext* ext,
                                      double* samples, int lds, int* ncols)
{
    (void)trace; (void)refresh;
    MCML_REQUIRE(Z && L && X && y && beta && samples, "mcmc_sample: null argument");
    CtxGuard g;
    uint64_t seed = 0;
    MCML_TRY(open_sampler(Z, L, X, y, n, Q, P, family, link, ext, g, &seed));
    glmmr_mcml_hmc_opts ho{};
    ho.warmup = warmup; ho.nsamp = nsamp; ho.adapt = 100; ho.lambda = lambda; ho.max_steps = maxsteps;
    ho.target_accept = target_accept; ho.chains = (ext && ext->chains > 0) ? ext->chains : 1; ho.chain_offset = 0;
    MCML_TRY(glmmr_mcml_ctx_hmc_sample(g.h, beta, var_par, &ho, seed, 0, nullptr, nullptr, nullptr, nullptr, nullptr, ncols));
    return glmmr_mcml_get_u(g.h, samples, lds);
}

extern "C" int glmmr_mcml_gen_u_samples(const double* Z, const double* L, const double* X, const double* y, int n, int Q,
                                        int P, const double* beta, const char* family, const char* link, double sigma,
                                        int warmup_iter, int m, const glmmr_mcml_nuts_opts* opts, const glmmr_mcml_ext* ext,
                                        double* samples, int lds, int* ncols)
{
    MCML_REQUIRE(Z && L && X && y && beta && samples, "gen_u_samples: null argument");
    CtxGuard g;
    uint64_t seed = 0;
    MCML_TRY(open_sampler(Z, L, X, y, n, Q, P, family, link, ext, g, &seed));
    glmmr_mcml_nuts_opts no{};
    if (opts) no = *opts;
    no.warmup = warmup_iter; no.nsamp = m;
    if (no.chains <= 0) no.chains = (ext && ext->chains > 0) ? ext->chains : 1;      // gen_u_samples.R:59: chains = 1
    MCML_TRY(glmmr_mcml_ctx_nuts_sample(g.h, beta, sigma, &no, seed, 0, nullptr, nullptr, nullptr, nullptr, nullptr, ncols));
    return glmmr_mcml_get_u(g.h, samples, lds);
}
