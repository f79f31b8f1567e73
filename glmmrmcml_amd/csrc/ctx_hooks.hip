// ctx_hooks.hip -- the test / bench hooks of include/glmmr_mcml_c.h that take a context, and the two process-wide launch
// counters that tell what the contexts of the one-shot exports ran.  The public API is cabi.hip; the hooks that need no
// context (GEMM, RNG, optimiser, copies) are debug_hooks.hip.
#include "entry.h"
#include "sparse_plan.h"
#include <algorithm>

using namespace mcml;

extern "C" int glmmr_mcml_dbg_theta_log(glmmr_mcml_ctx* h, int enable, double* out, int cap_rows, int* nrows)
{
    MCML_REQUIRE(h, "theta_log: null context");
    Ctx& c = h->c;
    const int w = c.cov.npar + 1;
    const int have = (int)(c.theta_log.size() / (size_t)w);
    if (nrows) *nrows = have;
    if (out) {
        const int take = have < cap_rows ? have : cap_rows;       // the LAST `take` rows
        memcpy(out, c.theta_log.data() + (size_t)(have - take) * w, sizeof(double) * (size_t)take * w);
        if (nrows) *nrows = take;
    }
    if (enable >= 0) { c.theta_log_on = enable != 0; if (enable) c.theta_log.clear(); }
    return MCML_OK;
}

// read-only: the banded kernel's decomposition for `chains` columns of the forward (which = 0) or backward (1)
// product -- the plan a product has built for that column-tile count, or the same decomposition computed on the host
extern "C" int glmmr_mcml_dbg_band_plan(glmmr_mcml_ctx* h, int which, int chains, int* out10)
{
    MCML_REQUIRE(h && (which == 0 || which == 1) && chains >= 1 && out10, "dbg_band_plan: bad argument");
    const Ctx& c = h->c;
    const BandPlan& bp = which ? c.plan_bwd : c.plan_fwd;
    const int gn = (chains + BD_BN - 1) / BD_BN;
    if (c.sp.active) {         // the operator is the sparse one: the plans of an earlier dense L (set_L) are kept but not in use
        for (int i = 0; i < 10; ++i) out10[i] = 0;
        out10[3] = gn;
        return MCML_OK;
    }
    int nempty = 0;
    for (int b = 0; b < bp.nbands; ++b) nempty += bp.kr[2 * b] == bp.kr[2 * b + 1];
    int nwg = 0, nred = 0, nslots = 0, paired = 0, built = 0;
    auto it = bp.by_gn.find(gn);
    if (it != bp.by_gn.end()) {
        const BandPlanDev& d = *it->second;
        nwg = d.nwg; nred = d.nred; nslots = d.nslots; paired = d.paired; built = 1;
    } else if (bp.nbands > 0) {
        std::vector<BandItem> items; std::vector<int> wg_ptr; std::vector<BandRed> red;
        paired = BandPlan::decompose(bp.kr, bp.nbands, gn, 256, items, wg_ptr, red, nslots) ? 1 : 0;
        nwg = (int)wg_ptr.size() - 1; nred = (int)red.size();
    }
    const int v[10] = {(which ? c.band_bwd : c.band_fwd) ? 1 : 0, bp.nbands, (int)bp.tiles, gn, nwg, nred, nslots,
                       paired, nempty, built};
    for (int i = 0; i < 10; ++i) out10[i] = v[i];
    return MCML_OK;
}

// read-only: the host copy of the row-tile extents of the forward (which = 0) or backward (1) operand, 10 ints per band
// (band_plan.h), as many bands as fit `cap` ints; out3 = [bands, MFMAs per 16-column strip inside the extents, MFMAs per
// strip of the whole K tiles]
extern "C" int glmmr_mcml_dbg_band_extents(glmmr_mcml_ctx* h, int which, int* ext, int cap, long long* out3)
{
    MCML_REQUIRE(h && (which == 0 || which == 1) && out3 && (ext || cap == 0), "dbg_band_extents: bad argument");
    const Ctx& c = h->c;
    const BandPlan& bp = which ? c.plan_bwd : c.plan_fwd;
    const int nb = c.sp.active ? 0 : bp.nbands;
    out3[0] = nb; out3[1] = nb ? bp.issued(true) : 0; out3[2] = nb ? bp.issued(false) : 0;
    for (int i = 0; i < cap && i < BD_EXT * nb; ++i) ext[i] = bp.ext[i];
    return MCML_OK;
}

// read-only: the form of the sparse (chain-major) ZL operator and the kernels the HMC sampler launches on it for `chains`
// chains (ncb follows `chains`; nuts.h launches on the width of its active set) -- the decisions are the functions of sparse_plan.h that hmc.hip launches by
extern "C" int glmmr_mcml_dbg_sparse_plan(glmmr_mcml_ctx* h, int chains, long long* out12)
{
    MCML_REQUIRE(h && chains >= 1 && out12, "dbg_sparse_plan: bad argument");
    const Ctx& c = h->c;
    const SparseZL& sp = c.sp;
    for (int i = 0; i < 12; ++i) out12[i] = 0;
    out12[0] = sp.active ? 1 : 0;
    out12[10] = cm_qrows(c.Q); out12[11] = cm_chain_blocks(chains);
    if (!sp.active) return MCML_OK;
    out12[1] = sp.factored ? 1 : 0; out12[2] = sp.W; out12[3] = sp.nnz; out12[4] = sp.nnz_z; out12[5] = sp.nnz_l;
    out12[6] = sp.nblk; out12[7] = sp.max_blk; out12[8] = cm_long_rows(c) ? 1 : 0; out12[9] = cm_fuse_width(c);
    return MCML_OK;
}

extern "C" long long glmmr_mcml_dbg_traj_launches(void) { return cm_traj_launch_count(); }

// read-only: the component-local trajectory path as the next hmc_sample call with `chains` chains would take it
extern "C" int glmmr_mcml_dbg_component_plan(glmmr_mcml_ctx* h, int chains, long long* out11)
{
    MCML_REQUIRE(h && chains >= 1 && out11, "dbg_component_plan: bad argument");
    const Ctx& c = h->c;
    const ComponentPlan& p = c.cp.plan;
    for (int i = 0; i < 11; ++i) out11[i] = 0;
    out11[0] = c.traj_mode; out11[9] = CP_MAX_VARS;
    if (!c.sp.active) return MCML_OK;
    const bool feasible = c.cp.ready && p.feasible;
    out11[1] = feasible ? 1 : 0; out11[2] = (feasible && c.traj_mode == 1) ? 1 : 0;
    out11[3] = p.ncomp; out11[4] = p.max_vars; out11[5] = p.max_rows; out11[6] = p.empty_comps;
    if (!feasible) return MCML_OK;
    const int waves = cp_waves(p, cp_forced_waves(CP_TRAJ_WAVES_ENV));
    out11[7] = p.nitems(); out11[8] = waves; out11[10] = cp_lds_bytes(p.max_vars, waves);
    return MCML_OK;
}

// read-only: the exact path as the next hmc_sample call would (not) take it
extern "C" int glmmr_mcml_dbg_draws_plan(glmmr_mcml_ctx* h, int* out4)
{
    MCML_REQUIRE(h && out4, "dbg_draws_plan: null argument");
    const Ctx& c = h->c;
    const long long bytes = (long long)sizeof(double) * pad_ld(c.Q) * c.Q;
    out4[0] = c.draws_mode; out4[1] = hmc_exact_applicable(c) ? 1 : 0; out4[2] = c.Q;
    out4[3] = bytes > 0x7fffffffLL ? 0x7fffffff : (int)bytes;
    return MCML_OK;
}

// read-only: the component path as the next hmc_sample call would (not) take it
extern "C" int glmmr_mcml_dbg_exact_component_plan(glmmr_mcml_ctx* h, long long* out8)
{
    MCML_REQUIRE(h && out8, "dbg_exact_component_plan: null argument");
    const Ctx& c = h->c;
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    out8[0] = c.draws_mode;
    if (!hmc_exact_component_applicable(c)) return MCML_OK;
    const ComponentPlan& p = c.cp.plan;
    out8[1] = 1; out8[2] = p.ncomp; out8[3] = p.max_vars; out8[4] = p.max_rows;
    hmc_exact_component_sizes(c, out8 + 5);
    return MCML_OK;
}

extern "C" int glmmr_mcml_dbg_exact_component_phases(glmmr_mcml_ctx* h, int enable, double* out4)
{
    MCML_REQUIRE(h, "dbg_exact_component_phases: null context");
    if (out4) for (int i = 0; i < 4; ++i) out4[i] = h->c.exact_comp.ms[i];
    h->c.exact_comp.prof = enable != 0;
    return MCML_OK;
}

extern "C" int glmmr_mcml_dbg_exact_phases(glmmr_mcml_ctx* h, int enable, double* out5)
{
    MCML_REQUIRE(h, "dbg_exact_phases: null context");
    if (out5) for (int i = 0; i < 5; ++i) out5[i] = h->c.exact.ms[i];
    h->c.exact.prof = enable != 0;
    return MCML_OK;
}

// scripts/time_exact_gaussian.py: HIP-event time (median of `reps`) of the transposed solve and / or of the forward solve of
// the factor the last exact call left, on a copy of the context's m sample columns
extern "C" int glmmr_mcml_dbg_trsm_compare(glmmr_mcml_ctx* h, int m, int reps, double* trans_ms, double* fwd_ms)
{
    MCML_REQUIRE(h && m > 0 && reps > 0 && reps <= 64, "dbg_trsm_compare: bad argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_REQUIRE(c.last_kernel[0] == KERNEL_EXACT && c.exact.M.d() && c.exact.M.rows == c.Q && c.U.d() && c.mcols >= m,
                 "dbg_trsm_compare: the last sampler call on this context must be an exact one with at least %d columns", m);
    DevMat T;
    MCML_TRY(T.alloc(c.Q, m));
    hipEvent_t e0, e1;
    MCML_HIP(hipEventCreate(&e0)); MCML_HIP(hipEventCreate(&e1));
    int rc = MCML_OK;
    for (int which = 0; which < 2 && rc == MCML_OK; ++which) {
        double* out = which ? fwd_ms : trans_ms;
        if (!out) continue;
        std::vector<float> ms;
        for (int r = 0; r < reps && rc == MCML_OK; ++r) {
            if (hipMemcpy2DAsync(T.d(), sizeof(double) * T.ld, c.U.d(), sizeof(double) * c.U.ld, sizeof(double) * c.Q, m,
                                 hipMemcpyDeviceToDevice, c.stream) != hipSuccess) { rc = MCML_EHIP; break; }
            (void)hipEventRecord(e0, c.stream);
            rc = which ? trsm_left_lower(c, c.exact.M.d(), c.exact.M.ld, c.Q, T.d(), T.ld, m)
                       : trsm_left_lower_trans(c, c.exact.M.d(), c.exact.M.ld, c.Q, T.d(), T.ld, m);
            (void)hipEventRecord(e1, c.stream);
            if (hipEventSynchronize(e1) != hipSuccess) rc = MCML_EHIP;
            float t = 0;
            if (rc == MCML_OK && hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms.push_back(t);
        }
        if (rc == MCML_OK && !ms.empty()) { std::sort(ms.begin(), ms.end()); *out = ms[ms.size() / 2]; }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc == MCML_EHIP) set_error("dbg_trsm_compare: HIP call failed");
    return rc;
}

extern "C" long long glmmr_mcml_dbg_la_component_launches(void) { return la_component_launch_count(); }

// read-only: what was asked for and what the last Laplace call on this context did
extern "C" int glmmr_mcml_dbg_la_plan(glmmr_mcml_ctx* h, long long* out8)
{
    MCML_REQUIRE(h && out8, "dbg_la_plan: null argument");
    const Ctx& c = h->c;
    const ComponentPlan& p = c.cp.plan;
    const long long v[8] = {c.la_mode, c.la_last_op, p.ncomp, p.max_vars, p.max_rows, c.la_launches, c.la_dense_bytes, c.la_waves};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return MCML_OK;
}

// read-only: what the last glmmr_mcml_ctx_predict_re on this context did (predict.hip)
extern "C" int glmmr_mcml_dbg_predict_plan(glmmr_mcml_ctx* h, long long* out8)
{
    MCML_REQUIRE(h && out8, "dbg_predict_plan: null argument");
    std::copy(h->c.predict.plan, h->c.predict.plan + 8, out8);
    return MCML_OK;
}

// read-only: what the last glmmr_mcml_ctx_sandwich on this context was asked for and did (sandwich.hip)
extern "C" int glmmr_mcml_dbg_sandwich_plan(glmmr_mcml_ctx* h, long long* out8)
{
    MCML_REQUIRE(h && out8, "dbg_sandwich_plan: null argument");
    std::copy(h->c.sand.plan, h->c.sand.plan + 8, out8);
    return MCML_OK;
}

// read-only: what the last glmmr_mcml_ctx_information on this context was asked for and did (info.hip)
extern "C" int glmmr_mcml_dbg_information_plan(glmmr_mcml_ctx* h, long long* out8)
{
    MCML_REQUIRE(h && out8, "dbg_information_plan: null argument");
    std::copy(h->c.info.plan, h->c.info.plan + 8, out8);
    return MCML_OK;
}

// read-only: what the last glmmr_mcml_ctx_theta_information on this context was asked for and did (theta_info.hip)
extern "C" int glmmr_mcml_dbg_theta_information_plan(glmmr_mcml_ctx* h, long long* out8)
{
    MCML_REQUIRE(h && out8, "dbg_theta_information_plan: null argument");
    std::copy(h->c.tinfo.plan, h->c.tinfo.plan + 8, out8);
    return MCML_OK;
}

// read-only: what the last glmmr_mcml_ctx_small_sample on this context was asked for and did (small_sample.hip)
extern "C" int glmmr_mcml_dbg_small_sample_plan(glmmr_mcml_ctx* h, long long* out8)
{
    MCML_REQUIRE(h && out8, "dbg_small_sample_plan: null argument");
    std::copy(h->c.ss.plan, h->c.ss.plan + 8, out8);
    return MCML_OK;
}

extern "C" int glmmr_mcml_dbg_emulate_world(glmmr_mcml_ctx* h, int world, int mode)
{
    MCML_REQUIRE(h, "emulate_world: null context");
    Ctx& c = h->c;
    MCML_REQUIRE(c.world <= 1 && !c.comm, "emulate_world: the context is rank %d of a real group of %d", c.rank, c.world);
    MCML_REQUIRE(world <= 1 || mode == 1 || mode == 2, "emulate_world: mode must be 1 (record) or 2 (replay)");
    if (world <= 1) { c.emu_world = 0; c.emu_mode = 0; c.emu_trace.clear(); c.emu_pos = 0; c.uall_valid = false; return MCML_OK; }
    if (c.emu_world != world) { c.emu_trace.clear(); c.uall_valid = false; }
    c.emu_world = world; c.emu_mode = mode; c.emu_pos = 0;
    if (mode == 1) c.emu_trace.clear();
    return MCML_OK;
}

extern "C" int glmmr_mcml_dbg_log_prob_grad(glmmr_mcml_ctx* h, const double* beta, double var_par,
                                            const double* V, int ncols, double* lp, double* G)
{
    MCML_REQUIRE(h && beta && V && lp && G && ncols > 0, "log_prob_grad: bad argument");
    MCML_HIP(hipSetDevice(h->c.device));
    return hmc_dbg_log_prob_grad(h->c, beta, var_par, V, ncols, lp, G);
}

extern "C" int glmmr_mcml_dbg_theta_round(glmmr_mcml_ctx* h, const double* thetas, int k, double* out)
{
    MCML_REQUIRE(h, "theta_round: null context");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_theta_round(h->c, thetas, k, out);
}

extern "C" int glmmr_mcml_dbg_leaf_profile(glmmr_mcml_ctx* h, unsigned long long* out10)
{
    MCML_REQUIRE(h && out10, "leaf_profile: null argument");
    return potrf_leaf_profile(h->c, out10);
}

extern "C" int glmmr_mcml_dbg_la_probe(glmmr_mcml_ctx* h, const double* start, int nstart, int kind, const double* v,
                                       double var_par, const double* par, int npar, double* out, double* v_out,
                                       double* beta_out, double* sigma_out)
{
    MCML_REQUIRE(h && start, "la_probe: null argument");
    MCML_REQUIRE(kind >= 0 && kind <= 3, "la_probe: kind %d", kind);
    MCML_REQUIRE(kind == 3 ? (v_out && beta_out && sigma_out) : (par && out && npar > 0), "la_probe: null output");
    MCML_HIP(hipSetDevice(h->c.device));
    return drv_la_probe(h->c, start, nstart, kind, v, var_par, par, npar, out, v_out, beta_out, sigma_out);
}

// ------------------------------------------------------------------------- test hooks of the dense Cholesky stack
// The n x n host array A goes to the device AS GIVEN (upper triangle included), potrf_lower_checked factorises it, then every
// solve runs on a fresh copy of B (n x m) against that factor: trsm_left_lower -> Xfwd, trsm_left_lower_trans -> Ytrans,
// potrs_lower_vec column by column -> Zpotrs (each n x m with leading dimension ldb; null: skipped).  A receives the whole
// array as the device left it, Linv (nullable) the ceil(n / 128) inverted 128 x 128 diagonal blocks of c.chol.linv.
extern "C" int glmmr_mcml_dbg_chol(glmmr_mcml_ctx* h, int n, double* A, int lda, int m, const double* B, int ldb,
                                   double* Xfwd, double* Ytrans, double* Zpotrs, double* Linv)
{
    MCML_REQUIRE(h && A && n > 0 && lda >= n && m >= 0, "dbg_chol: bad argument");
    MCML_REQUIRE(m == 0 || (B && ldb >= n), "dbg_chol: bad right-hand sides");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    MCML_REQUIRE(c.scalars.d(), "dbg_chol: the context has no covariance set up");
    DevMat dA, dB, T;
    DevBuf tmp;
    MCML_TRY(upload_matrix(dA, A, n, n, lda, c.stream));
    MCML_TRY(potrf_lower_checked(c, dA.d(), n, dA.ld));
    MCML_TRY(download_matrix(A, lda, dA.d(), dA.ld, n, n, c.stream));
    if (Linv) {
        MCML_TRY(copy_d2h(Linv, c.chol.linv.d(), sizeof(double) * (size_t)((n + CHOL_NB - 1) / CHOL_NB) * CHOL_NB * CHOL_NB, c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
    }
    if (m == 0) return MCML_OK;
    MCML_TRY(upload_matrix(dB, B, n, m, ldb, c.stream));
    MCML_TRY(T.alloc(n, m));
    MCML_TRY(tmp.ensure(sizeof(double) * CHOL_NB));
    for (int which = 0; which < 3; ++which) {
        double* out = which == 0 ? Xfwd : which == 1 ? Ytrans : Zpotrs;
        if (!out) continue;
        MCML_HIP(hipMemcpyAsync(T.d(), dB.d(), sizeof(double) * (size_t)dB.ld * m, hipMemcpyDeviceToDevice, c.stream));
        if (which == 0) MCML_TRY(trsm_left_lower(c, dA.d(), dA.ld, n, T.d(), T.ld, m));
        else if (which == 1) MCML_TRY(trsm_left_lower_trans(c, dA.d(), dA.ld, n, T.d(), T.ld, m));
        else for (int j = 0; j < m; ++j) MCML_TRY(potrs_lower_vec(c, dA.d(), dA.ld, n, T.d() + (size_t)j * T.ld, tmp.d()));
        MCML_TRY(download_matrix(out, ldb, T.d(), T.ld, n, m, c.stream));
    }
    return MCML_OK;
}

// What the last mvn_ll call (cand = -1: c.Dwork) or the last mvn_ll_batch call (cand >= 0: matrix `cand` of c.Dbatch) left in
// its workspace for the context's last large block: the d x d array holding the factor -> L, the m x d solved sample rows
// below it -> X (either may be null); dims = {d, round_up(d, 16), m, the workspace's leading dimension}.
extern "C" int glmmr_mcml_dbg_mvn_workspace(glmmr_mcml_ctx* h, int cand, double* L, int ldl, double* X, int ldx, int* dims)
{
    MCML_REQUIRE(h && dims && cand >= -1, "dbg_mvn_workspace: bad argument");
    Ctx& c = h->c;
    MCML_HIP(hipSetDevice(c.device));
    const Ctx::MvnWs& w = c.mvn_ws[cand >= 0];
    const DevMat& W = cand >= 0 ? c.Dbatch : c.Dwork;
    MCML_REQUIRE(w.kb > 0 && W.d(), "dbg_mvn_workspace: no %s call on this context before it", cand >= 0 ? "mvn_ll_batch" : "mvn_ll");
    MCML_REQUIRE(cand < w.kb, "dbg_mvn_workspace: candidate %d of %d", cand, w.kb);
    dims[0] = w.d; dims[1] = w.dp; dims[2] = w.m; dims[3] = w.ld;
    MCML_HIP(hipStreamSynchronize(c.stream));
    const double* Wj = W.d() + (cand > 0 ? (size_t)cand * w.ld * round_up(c.maxdim_large, 16) : 0);
    if (L) {
        MCML_REQUIRE(ldl >= w.d, "dbg_mvn_workspace: ldl %d < %d", ldl, w.d);
        MCML_TRY(download_matrix(L, ldl, Wj, w.ld, w.d, w.d, c.stream));
    }
    if (X) {
        MCML_REQUIRE(ldx >= w.m, "dbg_mvn_workspace: ldx %d < %d", ldx, w.m);
        MCML_TRY(download_matrix(X, ldx, Wj + w.dp, w.ld, w.m, w.d, c.stream));
    }
    return MCML_OK;
}
