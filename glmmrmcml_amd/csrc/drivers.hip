// drivers.hip -- the algorithm objects and drivers above the kernels:
//   objective functors D_/L_/F_likelihood        likelihood.h:31-110
//   mcmloptim::{d_optim,l_optim,f_optim,mcnr,f_hess}   mcmloptim.h:56-113,198-236,333-355
//   drivers mcml_full, mcmc_sample                src/mcml_full.cpp:41-148,314-338
//   mcml_optim, mcml_simlik, mcml_hess, aic_mcml  src/mcml_optim.cpp:35-392
// Host code; every objective evaluation runs on the device with u, Z, X, y
// resident and returns one scalar.  The MVN term has two forms: eval_mvn (one
// theta) and eval_theta_round (a round of candidates).  The spaces the steps
// search are parspace.h's; a round's values cross the ranks in comm.hip.
//
// Deliberate departures from the reference:
//   D4  the importance ratio exp(ll+logl)/exp(denom) underflows to NaN for any
//       realistic n (likelihood.h:101-105): evaluated as -(ll + logl - denom).
//   D3  mcnr's OpenMP race on W_/zu_: the statistics here are those of the
//       serial loop.
//   D11 the sampler is re-initialised every MCML iteration exactly as the
//       reference does (mhmcmc.h:127), with seeds derived from (seed, iteration).
#include "entry.h"
#include "glm.h"
#include "optim.h"
#include "parspace.h"
#include "theta_scale.h"
#include "trace.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>

namespace mcml {

// ---- device-backed scalar evaluations (all-reduced over ranks) ----
static int eval_loglik(Ctx& c, const double* beta, double var_par, double* ll)
{
    MCML_TRY(model_update_beta(c, beta));
    double s = 0;
    MCML_TRY(model_loglik_sum(c, var_par, &s));
    double tot[2] = {s, (double)c.niter};
    MCML_TRY(allreduce_host(c, tot, 2));
    *ll = tot[0] / tot[1];
    return MCML_OK;
}

// A theta at which some block is not positive definite has no likelihood: the
// reference would return NaN from its unchecked Cholesky; the optimiser is told
// "infinitely bad" so that it backs away instead of aborting the fit.
static const double LOGL_NO_VALUE = -HUGE_VAL;

// tests (ctx.h theta_log): one MVN objective evaluation
static void log_theta(Ctx& c, const double* theta, double logl)
{
    if (c.theta_log_on) { c.theta_log.insert(c.theta_log.end(), theta, theta + c.cov.npar); c.theta_log.push_back(logl); }
}

// the single-candidate form
static int eval_mvn(Ctx& c, const double* theta, double* logl)
{
    double s = 0;
    int rc = mvn_loglik_sum(c, theta, &s);
    if (rc == MCML_ENOTPD) { *logl = LOGL_NO_VALUE; return MCML_OK; }
    MCML_TRY(rc);
    double tot[2] = {s, (double)c.mcols};
    MCML_TRY(allreduce_host(c, tot, 2));
    *logl = tot[0] / tot[1];
    log_theta(c, theta, *logl);
    return MCML_OK;
}

// D is large dense blocks only (the geospatial configs): a round of candidate thetas is evaluated in ONE pass of the
// factorisation's schedule (mvn.hip mvn_loglik_batch), so rounds of candidates are the schedule there
static bool dense_only(const Ctx& c) { return c.maxdim_large > 0 && c.n_small == 0 && c.n_diag_rows == 0; }

// Candidates that differ in a pure scale parameter only share a factorisation (theta_scale.h): where rounds of candidates
// are the schedule and the specification proves a scale.  GLMMR_MCML_THETA_SCALE=0: one factorisation per candidate.
static bool scale_active(const Ctx& c) { return dense_only(c) && theta_scale_any(c.theta_scale_p) && theta_scale_enabled(); }

// One round of candidate thetas on the m columns of Us, the only place that does any of it: cand[j] -> the R coordinates of
// candidate j as the optimiser holds them (theta or log theta: sp); logl[j] = sum_j / m, LOGL_NO_VALUE where rcs[j] is not
// MCML_OK; returns the batch call's code, which rcs[j] may not show; (log) logs the candidates that have a value.  With a
// memo (ts, alive for one theta-step: the samples are fixed in it) only the first member of every group not seen before is
// factorised, the others are rescaled on the host; a round of ONE new candidate runs the single evaluation, leaves no entry.
static int eval_theta_round(Ctx& c, const ParSpace& sp, ThetaScaleMemo* ts, const std::vector<const double*>& cand,
                            const double* Us, int ldu, int m, bool log, std::vector<double>* logl, std::vector<int>* rcs)
{
    const int R = c.cov.npar, k = (int)cand.size();
    std::vector<double> X((size_t)R * k), ths((size_t)R * k), sums(k, 0.0);
    for (int j = 0; j < k; ++j) for (int i = 0; i < R; ++i) { X[(size_t)j * R + i] = cand[j][i]; ths[(size_t)j * R + i] = sp.theta_at(cand[j][i]); }
    rcs->assign(k, 0);
    int brc = MCML_OK;
    const std::vector<int> reps = ts ? ts->plan(X.data(), R, k) : std::vector<int>();
    const int nr = (int)reps.size();
    if (!ts || (k == 1 && nr == 1)) {
        c.theta_factorised += k;
        brc = mvn_loglik_batch(c, ths.data(), k, Us, ldu, m, sums.data(), rcs->data());
    } else {
        std::vector<double> rth((size_t)R * nr), rsums(nr, 0.0), parts((size_t)2 * nr, 0.0);
        std::vector<int> rrcs(nr, 0);
        for (int q = 0; q < nr; ++q) memcpy(&rth[(size_t)q * R], &ths[(size_t)reps[q] * R], sizeof(double) * R);
        if (nr > 0) brc = mvn_loglik_batch_parts(c, rth.data(), nr, k, Us, ldu, m, rsums.data(), rrcs.data(), parts.data());
        if (brc != MCML_OK) rcs->assign(k, brc);
        else {
            c.theta_factorised += nr;
            ts->finish(X.data(), R, k, reps, rsums.data(), parts.data(), rrcs.data(), c.cov.N, m, sums.data(), rcs->data());
        }
    }
    logl->assign(k, LOGL_NO_VALUE);
    for (int j = 0; j < k; ++j)
        if (brc == MCML_OK && (*rcs)[j] == MCML_OK) { (*logl)[j] = sums[j] / m; if (log) log_theta(c, &ths[(size_t)j * R], (*logl)[j]); }
    return brc;
}

// mcmloptim<T> (mcmloptim.h:16-369)
struct McmlOptim {
    Ctx& c;
    int P, R;
    std::vector<double> beta, theta, cov_par_fix;
    double sigma;
    int trace, maxfun;
    int theta_batch = 0;      // candidates per rank and round of the sharded theta-step (glmmr_mcml_ext.theta_batch)
    double model_var_par;     // M_->var_par_

    McmlOptim(Ctx& ctx, const double* start, int trace_, int maxfun_, double var_par0)
        : c(ctx), P(ctx.P), R(ctx.cov.npar), trace(trace_), maxfun(maxfun_), model_var_par(var_par0)
    {
        parse_start(start, P, R, glm_is_gaussian(c.flink), &beta, &theta, &sigma);
        cov_par_fix = theta;
    }
    int result(double* b, double* t, double* s) const { std::copy(beta.begin(), beta.end(), b); std::copy(theta.begin(), theta.end(), t); *s = sigma; return MCML_OK; }

    // d_optim of a chain-sharded job (no reference counterpart: the reference is one process).  The
    // factorisation of D(theta) does not shard -- replicated, it was 43 % of a rank's step at 8 GPUs -- but the
    // optimiser's EVALUATIONS do: the sample columns are all-gathered once per iteration (every rank then holds all of
    // u), the optimiser proposes `width` candidate thetas per round (optim.h bobyqa_batch), candidate j is evaluated on
    // ALL columns by rank j mod world, and one all-reduce per round carries the values (each slot is nonzero on one
    // rank).  Same objective (mcmloptim.h:56-68, likelihood.h:31-46, mcmldmatrix.h:23-41), sequential depth = rounds.
    // The search runs over log(theta): the parameters are positive scales (lower bound 1e-6, mcmloptim.h:35-38) and
    // the MVN log-likelihood is far closer to a quadratic there, which is what a round of simultaneous points needs.
    // Every rank runs the same deterministic optimiser on the same values: no further agreement is needed.
    int d_optim_sharded(int width)
    {
        MCML_TRY(gather_samples(c));
        const int wr = comm_world(c), mall = c.mcols * wr;
        // one memo per rank whose share is evaluated here, alive for this theta-step only (the samples are fixed in it):
        // a rank groups inside its own share of a round, candidates are never re-dealt between ranks
        std::vector<ThetaScaleMemo> memos(scale_active(c) ? wr : 0);
        for (ThetaScaleMemo& ts : memos) ts.reset(c.theta_scale_p, true);
        const ParSpace sp(0, R, false, true);
        batch_objective_fn fb = [&](const std::vector<std::vector<double>>& Zs, std::vector<double>* F) -> int {
            const int nc = (int)Zs.size();
            std::vector<double> vals(nc, 0.0);
            int first_rc = MCML_OK;
            // this rank's candidates of the round, factorised side by side (mvn.hip mvn_loglik_batch).  Rank emulation in
            // recording mode evaluates every rank's share here, one rank's share at a time -- exactly the batches the
            // ranks of the real job would run, so that the replay reproduces the recorded values to the bit
            const bool all_shares = comm_emulated(c) && c.emu_mode == 1;
            for (int rr = all_shares ? 0 : c.rank; rr < (all_shares ? wr : c.rank + 1); ++rr) {
                std::vector<const double*> cand;                 // candidates rr, rr + wr, ...
                for (int j = rr; j < nc; j += wr) cand.push_back(Zs[j].data());
                if (cand.empty()) continue;
                std::vector<double> logl;
                std::vector<int> rcs;
                const int brc = eval_theta_round(c, sp, memos.empty() ? nullptr : &memos[rr], cand, c.Uall.d(), c.Uall.ld, mall,
                                                 true, &logl, &rcs);
                for (size_t q = 0; q < cand.size(); ++q) {
                    const int j = rr + (int)q * wr;
                    const int rc = (rcs[q] == MCML_OK && brc != MCML_OK) ? brc : rcs[q];
                    if (rc != MCML_OK && getenv("GLMMR_MCML_BOBYQA_TRACE")) fprintf(stderr, "theta-step: candidate %d (theta %.6g %.6g) rc %d brc %d: %s\n", j, sp.theta_at(Zs[j][0]), R > 1 ? sp.theta_at(Zs[j][1]) : 0.0, rcs[q], brc, last_error());
                    if (rc == MCML_OK || rc == MCML_ENOTPD) vals[j] = -1 * logl[q];     // no value: infinitely bad, not an error
                    else { vals[j] = NAN; if (first_rc == MCML_OK) first_rc = rc; }
                    if (rr == c.rank) ++c.theta_evals_own;
                }
            }
            c.theta_rounds += 1; c.theta_evals_all += nc;
            MCML_TRY(exchange_round(c, vals));
            if (first_rc != MCML_OK) return first_rc;
            for (double v : vals)         // a rank that failed put NaN in its slot: every rank stops here, together
                if (v != v) { set_error("theta-step: a rank failed to evaluate its candidate"); return MCML_EHIP; }
            *F = vals;
            return MCML_OK; };
        BobyqaOpts o = bopts(trace, maxfun); o.rhobeg = 0.25; o.rhoend = 1e-7;
        return sp.minimise(fb, o, width, &beta, &theta, &sigma);
    }

    // d_optim (mcmloptim.h:56-68), D_likelihood (likelihood.h:40-45)
    int d_optim()
    {
        static const bool shard = !(getenv("GLMMR_MCML_THETA_SHARD") && !strcmp(getenv("GLMMR_MCML_THETA_SHARD"), "0"));
        const int wr = comm_world(c);
        // candidates per rank and round.  For a dense-only model (dense_only()) the batch schedule is the default even
        // for a single process, 8 candidates per round (batch_width()); glmmr_mcml_ext.theta_batch wins, 1 = the
        // reference's sequential BOBYQA.
        // a sharded job: rounds of about eight candidates in all -- 8 / world per rank for a dense-block model (at 2 ranks
        // four candidates per rank factorised side by side: 6 rounds of 8.7 ms instead of 20 of 3.6 ms), one otherwise
        const int k = wr > 1 ? (theta_batch > 0 ? theta_batch : dense_only(c) ? std::max(1, 8 / wr) : 1) : batch_width();
        if ((wr > 1 && shard) || k > 1) return d_optim_sharded(wr * std::max(1, k));
        objective_fn f = [&](const std::vector<double>& par, double* v) {
            double logl; MCML_TRY(eval_mvn(c, par.data(), &logl)); *v = -1 * logl; return (int)MCML_OK; };
        return ParSpace(0, R, false).minimise(f, bopts(trace, maxfun), 0, &beta, &theta, &sigma);
    }

    // l_optim (mcmloptim.h:71-88), L_likelihood (likelihood.h:57-64)
    int l_optim()
    {
        if (c.flink == 12) { set_error("l_optim: beta family is not built (reference reads par[P] out of range, defect D8)"); return MCML_EUNSUPPORTED; }
        objective_fn f = [&](const std::vector<double>& par, double* v) {
            model_var_par = glm_has_var_par(c.flink) ? par[P] : 0.0;   // fix_var_ = false, fix_var_par_ = 0
            double ll; MCML_TRY(eval_loglik(c, par.data(), model_var_par, &ll)); *v = -1 * ll; return (int)MCML_OK; };
        return ParSpace(P, 0, glm_is_gaussian(c.flink)).minimise(f, bopts(trace, maxfun), 0, &beta, &theta, &sigma);
    }

    // mcnr (mcmloptim.h:198-236)
    int mcnr()
    {
        MCML_TRY(model_update_beta(c, beta.data()));
        std::vector<double> st((size_t)P * P + P + 2), nb(P);
        MCML_TRY(model_mcnr_stats(c, model_var_par, st.data()));
        double s = 0;
        MCML_TRY(mcnr_finish(P, st.data(), beta.data(), nb.data(), &s));
        beta = nb; sigma = s;
        return MCML_OK;
    }

    // F_likelihood::operator() (likelihood.h:88-109) with fix_var = true
    // memo: the MVN term depends on theta alone.  The central differences of f_hess move one or two coordinates at a time,
    // so about half of its 4 (P + R)^2 points repeat a theta already factorised (19 distinct of 36 at P = 1, R = 2): those
    // reuse the value (same bits) instead of another build + Cholesky + solve.
    typedef std::map<std::vector<double>, double> ThetaMemo;
    objective_fn make_F(bool importance, double fix_var_par, double denomD, bool memoise = false,
                        std::shared_ptr<ThetaMemo> memo = std::make_shared<ThetaMemo>())
    {
        return [this, importance, fix_var_par, denomD, memoise, memo](const std::vector<double>& par, double* v) {
            model_var_par = fix_var_par;
            double ll, logl;
            MCML_TRY(eval_loglik(c, par.data(), model_var_par, &ll));
            if (memoise) {
                const std::vector<double> th(par.begin() + P, par.begin() + P + R);
                auto it = memo->find(th);
                if (it != memo->end()) logl = it->second;
                else { MCML_TRY(eval_mvn(c, th.data(), &logl)); (*memo)[th] = logl; }
            } else
            MCML_TRY(eval_mvn(c, par.data() + P, &logl));
            *v = importance ? -1.0 * (ll + logl - denomD) : -1.0 * (ll + logl);
            return (int)MCML_OK; };
    }

    // candidates per round of the batch schedule for this model in a single process (see d_optim): 8 when D consists of
    // large dense blocks only, else 1 = the sequential optimiser; glmmr_mcml_ext.theta_batch / GLMMR_MCML_THETA_BATCH override
    int batch_width() const
    {
        if (theta_batch > 0) return theta_batch;
        static const int envk = getenv("GLMMR_MCML_THETA_BATCH") ? atoi(getenv("GLMMR_MCML_THETA_BATCH")) : 0;
        if (envk > 0) return envk;
        return dense_only(c) ? 8 : 1;
    }

    // f_optim on the batch schedule (single process, dense-block models): a round's candidates (beta, log theta[, sigma])
    // get their MVN terms from ONE pass of the factorisation (mvn_loglik_batch) and their log-likelihood terms one after
    // the other (cheap: n m log-pdf evaluations on the cached Z u).  Same objective (likelihood.h:88-109), same optimum.
    // (For the gaussian family the reference lets BOBYQA carry sigma as a variable the objective never reads,
    // mcmloptim.h:102-105 -- a flat direction whose final value is whatever the trust region left it at; here it simply stays
    // at its start value.)
    int f_optim_batch(int width, double denomD)
    {
        const double fix_var_par = sigma;
        ThetaScaleMemo memo;                                     // this call's: the samples are fixed in it
        const bool scale = scale_active(c);
        if (scale) memo.reset(c.theta_scale_p, true);
        const ParSpace sp(P, R, false, true);
        batch_objective_fn fb = [&](const std::vector<std::vector<double>>& Zs, std::vector<double>* F) -> int {
            const int nc = (int)Zs.size();
            std::vector<const double*> cand;
            for (const std::vector<double>& z : Zs) cand.push_back(z.data() + P);
            std::vector<double> logl;
            std::vector<int> rcs;
            MCML_TRY(eval_theta_round(c, sp, scale ? &memo : nullptr, cand, c.U.d(), c.U.ld, c.mcols, true, &logl, &rcs));
            F->assign(nc, 0.0);
            for (int j = 0; j < nc; ++j) {
                model_var_par = fix_var_par;
                double ll = 0;
                MCML_TRY(eval_loglik(c, Zs[j].data(), model_var_par, &ll));
                (*F)[j] = -1.0 * (ll + logl[j] - denomD);
            }
            return MCML_OK; };
        BobyqaOpts o = bopts(trace, maxfun); o.rhobeg = 0.25; o.rhoend = 1e-7;
        return sp.minimise(fb, o, width, &beta, &theta, &sigma);
    }

    // f_optim (mcmloptim.h:91-113)
    int f_optim()
    {
        const bool g = glm_is_gaussian(c.flink);
        double denomD = 0;
        MCML_TRY(eval_mvn(c, cov_par_fix.data(), &denomD));      // constant in the parameters
        if (comm_world(c) == 1 && batch_width() > 1) return f_optim_batch(batch_width(), denomD);
        objective_fn f = make_F(true, sigma, denomD);
        // 2n + 1 interpolation points, not the n + 2 the other steps take over from minqa: in the P + R dimensions of this
        // objective, whose curvatures differ by a factor of a hundred and more, a model on n + 2 points is all but linear --
        // the run crept along the weak directions in steps of its final radius and stopped 2e-6 to 4e-6 from the optimum
        // after 350 to 490 evaluations, where 2n + 1 points end within 4e-7 after 110 to 190
        BobyqaOpts o = bopts(trace, maxfun);
        o.npt = 2 * (P + R + (g ? 1 : 0)) + 1;
        return ParSpace(P, R, g).minimise(f, o, 0, &beta, &theta, &sigma);
    }

    // f_hess (mcmloptim.h:333-355)
    int f_hess(double tol, double* H)
    {
        auto memo = std::make_shared<ThetaMemo>();
        objective_fn f = make_F(false, sigma, 0.0, true, memo);
        const int nv = P + R;
        const ParSpace sp(P, R, false);
        const ParSpace::Point p = sp.pack(beta, theta, sigma);
        std::vector<double> nd(nv, tol), h;
        // The points of the finite differences do not depend on the values: a dry pass lists the thetas they will ask
        // for, and (single process) those are factorised side by side, a round at a time, before the real pass runs
        if (comm_world(c) == 1 && c.maxdim_large > 0) {
            std::vector<std::vector<double>> want;
            objective_fn dry = [&](const std::vector<double>& par, double* v) {
                std::vector<double> th(par.begin() + P, par.begin() + P + R);
                if (std::find(want.begin(), want.end(), th) == want.end()) want.push_back(th);
                *v = 0.0; return (int)MCML_OK; };
            std::vector<double> hdry;
            MCML_TRY(fd_hessian(dry, p.x, nd, true, p.lower, p.upper, &hdry));
            std::vector<const double*> cand;
            for (const std::vector<double>& th : want) cand.push_back(th.data());
            // the points move one or two coordinates at a time: those that differ in a scale parameter only share a matrix
            ThetaScaleMemo ts;
            const bool scale = scale_active(c);
            if (scale) ts.reset(c.theta_scale_p, false);         // these coordinates are theta itself
            std::vector<double> logl;
            std::vector<int> rcs;
            MCML_TRY(eval_theta_round(c, sp, scale ? &ts : nullptr, cand, c.U.d(), c.U.ld, c.mcols, true, &logl, &rcs));
            for (size_t q = 0; q < want.size(); ++q) (*memo)[want[q]] = logl[q];
        }
        MCML_TRY(fd_hessian(f, p.x, nd, true, p.lower, p.upper, &h));
        memcpy(H, h.data(), sizeof(double) * (size_t)nv * nv);
        return MCML_OK;
    }
};

// ---------------------------------------------------------------- ctx-level drivers
int drv_optim(Ctx& c, const double* start, int nstart, int trace, int mcnr, const glmmr_mcml_ext* e,
              double* beta, double* theta, double* sigma)
{
    const int P = c.P, R = c.cov.npar;
    MCML_REQUIRE(start && nstart >= P + R + (glm_is_gaussian(c.flink) ? 1 : 0), "start has %d values, need %d", nstart, P + R + (glm_is_gaussian(c.flink) ? 1 : 0));
    MCML_REQUIRE(c.mcols > 0, "no samples u set");
    McmlOptim mc(c, start, trace, e ? e->maxfun : 0, 1.0);      // model built with var_par = 1 (mcml_optim.cpp:51)
    mc.theta_batch = e ? e->theta_batch : 0;
    {
        PhaseRange r("mcml:beta-step");
        if (!mcnr) MCML_TRY(mc.l_optim()); else MCML_TRY(mc.mcnr());
    }
    PhaseRange r("mcml:theta-step");
    MCML_TRY(mc.d_optim());
    return mc.result(beta, theta, sigma);
}

int drv_simlik(Ctx& c, const double* start, int nstart, int trace, const glmmr_mcml_ext* e, double* beta,
               double* theta, double* sigma)
{
    const int P = c.P, R = c.cov.npar;
    MCML_REQUIRE(start && nstart >= P + R + (glm_is_gaussian(c.flink) ? 1 : 0), "start too short");
    MCML_REQUIRE(c.mcols > 0, "no samples u set");
    McmlOptim mc(c, start, trace, e ? e->maxfun : 0, 1.0);
    mc.theta_batch = e ? e->theta_batch : 0;
    MCML_TRY(mc.f_optim());
    return mc.result(beta, theta, sigma);
}

int drv_hess(Ctx& c, const double* start, int nstart, double tol, int trace, double* H)
{
    const int P = c.P, R = c.cov.npar;
    MCML_REQUIRE(start && nstart >= P + R + (glm_is_gaussian(c.flink) ? 1 : 0), "start too short");
    MCML_REQUIRE(c.mcols > 0, "no samples u set");
    McmlOptim mc(c, start, trace, 0, 1.0);
    return mc.f_hess(tol, H);
}

// One round of k candidate thetas (R x k) exactly as a theta-step evaluates it, with a memo of its own: out[j] =
// log-likelihood at candidate j, NaN where D is not positive definite (tests: glmmr_mcml_dbg_theta_round)
int drv_theta_round(Ctx& c, const double* thetas, int k, double* out)
{
    MCML_REQUIRE(thetas && out && k >= 1 && k <= 64, "theta_round: bad argument");
    MCML_REQUIRE(c.mcols > 0 && c.U.d(), "theta_round: no samples set");
    ThetaScaleMemo ts;
    const bool scale = scale_active(c);
    if (scale) ts.reset(c.theta_scale_p, false);
    std::vector<const double*> cand;
    for (int j = 0; j < k; ++j) cand.push_back(thetas + (size_t)j * c.cov.npar);
    std::vector<double> logl;
    std::vector<int> rcs;
    MCML_TRY(eval_theta_round(c, ParSpace(0, c.cov.npar, false), scale ? &ts : nullptr, cand, c.U.d(), c.U.ld, c.mcols, false,
                              &logl, &rcs));
    for (int j = 0; j < k; ++j) out[j] = rcs[j] == MCML_OK ? logl[j] : NAN;
    return MCML_OK;
}

// aic_mcml (mcml_optim.cpp:356-392)
int drv_aic(Ctx& c, const double* beta_par, int nbeta, const double* cov_par, int ncov, double* out)
{
    const int P = c.P;
    const bool var = glm_has_var_par(c.flink);
    MCML_REQUIRE(nbeta >= P + (var ? 1 : 0) && ncov >= c.cov.npar, "aic_mcml: parameter vectors too short");
    MCML_REQUIRE(c.mcols > 0, "no samples u set");
    const double var_par = var ? beta_par[P] : 0;
    const int dof = nbeta + ncov;
    double dmv, ll;
    MCML_TRY(eval_mvn(c, cov_par, &dmv));
    MCML_TRY(eval_loglik(c, beta_par, var_par, &ll));
    *out = (-2 * (ll + dmv) + 2 * dof);
    return MCML_OK;
}

// mcml_full (mcml_full.cpp:41-148)
int drv_full(Ctx& c, const double* start, int nstart, int mcnr, int m, int maxiter, int warmup, double tol,
             int verbose, double lambda, int trace, int refresh, int maxsteps, double target_accept,
             const glmmr_mcml_ext* e, double* beta_out, double* theta_out, double* sigma_out,
             int* converged_out, int* iters_out, glmmr_mcml_hmc_diag* last_diag)
{
    (void)refresh;
    const int P = c.P, R = c.cov.npar;
    MCML_REQUIRE(start && nstart >= P + R + 1, "mcml_full: start needs c(beta, theta, sigma|1) = %d values", P + R + 1);
    MCML_REQUIRE(m > 0 && maxiter >= 1, "mcml_full: bad m / maxiter");
    std::vector<double> theta(start + P, start + P + R), beta(start, start + P);
    double var_par = glm_is_gaussian(c.flink) ? start[nstart - 1] : 1;          // :65
    const uint64_t seed = default_seed(e);
    const int chains = (e && e->chains > 0) ? e->chains : 1;
    MCML_TRY(mvn_gen_L(c, theta.data(), true));                               // :66-68
    MCML_TRY(model_update_beta(c, beta.data()));
    MCML_TRY(model_update_L(c));
    McmlOptim mc(c, start, trace, e ? e->maxfun : 0, var_par);                // :71
    mc.theta_batch = e ? e->theta_batch : 0;
    double maxdiff = 1;
    int iter = 1;
    bool converged = false;
    glmmr_mcml_hmc_opts ho{};
    ho.warmup = warmup; ho.nsamp = m; ho.adapt = 100; ho.lambda = lambda; ho.max_steps = maxsteps;
    ho.target_accept = target_accept; ho.chains = chains; ho.chain_offset = c.rank * chains;
    while (maxdiff > tol && iter <= maxiter) {                                 // :83
        glmmr_mcml_hmc_diag dg{};
        {
            PhaseRange r("mcml:sample");
            MCML_TRY(hmc_sample(c, beta.data(), var_par, &ho, seed, (uint32_t)iter, nullptr, nullptr, nullptr,
                                nullptr, &dg, nullptr));                       // :92
        }
        if (last_diag) *last_diag = dg;
        mc.model_var_par = var_par;
        {
            PhaseRange r("mcml:beta-step");
            if (!mcnr) MCML_TRY(mc.l_optim()); else MCML_TRY(mc.mcnr());       // :95-99
        }
        {
            PhaseRange r("mcml:theta-step");
            MCML_TRY(mc.d_optim());                                            // :101
        }
        const std::vector<double>& nb = mc.beta; const std::vector<double>& nt = mc.theta;
        double new_var_par = 1;
        if (glm_is_gaussian(c.flink)) new_var_par = mc.sigma;                      // :105
        else new_var_par = var_par;
        maxdiff = 0;
        for (int i = 0; i < P; ++i) maxdiff = std::max(maxdiff, std::fabs(beta[i] - nb[i]));
        for (int i = 0; i < R; ++i) maxdiff = std::max(maxdiff, std::fabs(theta[i] - nt[i]));
        maxdiff = std::max(maxdiff, std::fabs(var_par - new_var_par));
        if (maxdiff < tol) converged = true;                                   // :113
        beta = nb; theta = nt; var_par = new_var_par;
        if (!converged) {                                                      // :119-126
            PhaseRange r("mcml:refresh");
            MCML_TRY(mvn_gen_L(c, theta.data(), true));
            MCML_TRY(model_update_beta(c, beta.data()));
            MCML_TRY(model_update_L(c));
        }
        if (verbose && c.rank == 0) {
            printf("Iter %d  beta:", iter);
            for (double b : beta) printf(" %.6g", b);
            printf("  theta:");
            for (double t : theta) printf(" %.6g", t);
            if (glm_is_gaussian(c.flink)) printf("  sigma: %.6g", var_par);
            printf("  max diff %.4g  accept %.3f%s\n", maxdiff, dg.accept_rate, converged ? "  CONVERGED" : "");
            fflush(stdout);
        }
        ++iter;
    }
    memcpy(beta_out, beta.data(), sizeof(double) * P);
    memcpy(theta_out, theta.data(), sizeof(double) * R);
    *sigma_out = var_par;
    if (converged_out) *converged_out = converged ? 1 : 0;
    if (iters_out) *iters_out = iter - 1;
    return MCML_OK;
}

}  // namespace mcml

extern "C" int glmmr_mcml_dbg_phase_ms(int enable, int reset, double* out8)
{
    mcml::PhaseClock& pc = mcml::phase_clock();
    std::lock_guard<std::mutex> g(pc.mu);
    if (out8) for (int i = 0; i < 4; ++i) { out8[i] = pc.ms[i]; out8[4 + i] = (double)pc.n[i]; }
    if (reset) for (int i = 0; i < 4; ++i) { pc.ms[i] = 0; pc.n[i] = 0; }
    pc.on.store(enable != 0, std::memory_order_relaxed);
    return 0;
}
