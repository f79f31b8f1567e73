// ctx.h -- the device-resident MCML problem: everything the hot path needs
// stays in HBM between calls (Z, X, y, the samples u, L, ZL, workspaces); only
// parameter vectors go down and scalars / small statistics come back.
#pragma once
#include "common.h"
#include "chol.h"
#include "covspec.h"
#include "band_plan.h"
#include "component_plan.h"
#include "step_ahead.h"

namespace mcml {

// cross-rank reduction hook (sum, f64, in place on a device buffer).  Single
// process: null.  bench.py / the distributed front end install a callback that
// all-reduces the buffer with torch.distributed (backend "nccl" = RCCL).
typedef int (*reduce_fn)(void* user, double* dev_buf, int n);

// kernel family that served an HMC product (glmmr_mcml_ctx_last_kernels)
enum { KERNEL_SKINNY = 0, KERNEL_BAND = 1, KERNEL_DLDS = 2, KERNEL_REG = 3, KERNEL_SPARSE = 4, KERNEL_COMPONENT = 5,
       KERNEL_EXACT = 6,     // 6: no product pair at all, the exact conditional draw (hmc_exact.h)
       KERNEL_EXACT_COMPONENT = 7 };   // 7: the same, component by component on the sparse operator (hmc_exact_comp.h)

// the sampler's step-count read-back (hmc.hip hmc_sample): a ring of host memory mapped into the device, written by
// k_max_steps with (proposal sequence number << 32 | count), read by the host with plain loads (StepAhead, step_ahead.h);
// lives as long as the context
struct StepRing {
    static constexpr int SLOTS = StepAhead::SLOTS;
    unsigned long long* h = nullptr;    // host address
    unsigned long long* d = nullptr;    // the same memory as the device sees it
    unsigned seq = 0;                   // sequence number of the last proposal launched
    StepRing() = default;
    StepRing(const StepRing&) = delete;
    StepRing& operator=(const StepRing&) = delete;
    ~StepRing() { if (h) (void)hipHostFree(h); }
};

struct HmcState {
    StepRing ring;
    int C = 0;                  // chains resident
    int Cw = 0;                 // columns the two products and the log-density kernels process (= C; the No-U-Turn
                                // sampler packs the chains whose trees still grow into the first Cw columns)
    DevMat V, R, UP, GRAD, GRADP;   // Q x C
    DevMat MU, S;               // n x C
    DevBuf chain;               // per-chain scalars, see hmc_chain.h
    DevBuf partial;             // per-(row slot, chain) partial sums
    int partial_slots = 0;
    bool cm = false;            // chain-major state (sparse ZL operator, hmc_cm.h): element (c, r) at c + r * ld
    DevBuf cm_part, cm_acc;     // chain-major path: partial sums (ll | lp | kin | ss), accept flags
    DevBuf cm_part_fwd;         // ... and the log-density partials the last forward product of a trajectory leaves (one per workgroup)
    DevMat LX, ZS;              // factored operator (SparseZL::factored): L X and Z' S, C x Q
    DevBuf cp_part;             // component-local trajectories (hmc_traj.h): K0 | ll | lp | kin, one per (work item, chain)
};

// No-U-Turn sampler (nuts.h): edges, tree, node under construction and one stored node per tree level (Q x C each),
// per-chain scalars, partial sums
constexpr int NUTS_MAXD = 12;                       // deepest tree supported (Stan's default max_treedepth: 10)
struct NutsState {
    DevMat vecs[16 + 4 * (NUTS_MAXD + 1)];
    DevBuf chain, part;
};

// ZL = Z L held as padded-CSR (ELL) rows plus its transpose in CSR: used by the sampler (chain-major state, hmc_cm.h)
// instead of the dense n x Q products when Z is indicator-like and every covariance block is
// diagonal or small, so that a row of ZL has only a few nonzeros (configs 1, 4, 5): the two
// products are then gathers bound by HBM bandwidth, not n x Q x C GEMMs.
struct SparseZL {
    bool possible = false, active = false, built = false;
    int W = 0;                       // ELL width
    long nnz = 0;
    DevBuf ell_col, ell_src, ell_z, ell_val;   // n x W (column-major): column of ZL, flat index into L, Z value, value
    DevBuf csr_ptr, csr_i, csr_pos, csr_val;   // rows of ZL' : q -> (observation, position in ell_val, value)
    DevBuf row_start;                          // first column of row q of the block-diagonal L (U = L V, hmc.hip)
    // factored form ZL = Z * L (hmc_cm.h): chosen when a row of ZL mostly repeats a row of L, i.e. when gathering
    // through Z and applying the blocks of L separately touches far fewer entries than nnz(ZL)
    bool factored = false;
    long nnz_z = 0, nnz_l = 0;
    DevBuf zcsr_ptr, zcsr_i, zcsr_val;         // rows of Z' : q -> (observation, value)
    DevBuf row_end;                            // one past the last row of column q of L (= end of q's block)
    DevBuf blk_ptr;                            // first row of every covariance block, B + 1 entries (k_cm_Lcol_Lrow)
    int nblk = 0, max_blk = 0;
};

// the components of ZL's coupling graph, their records and the work items of the trajectory kernel (component_plan.h;
// component.h describes a record and gives the kernels their view): the pattern is fixed per model (comp_setup, from
// sparse_zl_setup), the values follow L (comp_fill_val, from model_update_L) and beta (comp_fill_xy)
struct ComponentDev {
    ComponentPlan plan;
    bool ready = false;                        // the device copies below are there
    DevBuf item_ptr, var_ptr, vars, slot_ptr, slot_quarter, slot_i, slot_src, slot_d;
};

// the Cholesky factors of every M_c as lac_factor_launch leaves them, for whoever applies them afterwards (component.h,
// comp_factors_ensure): sum_c nv_c^2 doubles, at most Q * 128, where each starts, and the factor kernels' log-determinants
// (not read); kept between calls
struct CompFactors {
    DevBuf fac, fac_ptr, logdet;
    long long doubles = 0;              // 0: fac_ptr not uploaded yet
};

// HIP-event timing of the dominant kernels, on the stream they are launched on
// (bench.py's roofline line).  kind 0 = HMC forward GEMM, 1 = HMC backward GEMM.
struct KernelProf {
    bool on = false;
    bool skip = false;                          // on, but this launch is only counted (the sampler times one proposal in four)
    long long seen[4] = {0, 0, 0, 0};           // launches since the last reset, timed or not
    std::vector<hipEvent_t> ev;                 // pool
    std::vector<int> kind, e0, e1;              // per timed launch: kind, start / stop event index
    size_t used = 0, nev = 0;
    int last_stop = -1;                         // event recorded right after the previous timed launch
    double ms[4] = {0, 0, 0, 0};
    long long cnt[4] = {0, 0, 0, 0};
    int fresh() {
        if (nev >= ev.size())
            for (int i = 0; i < 512; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return -1; ev.push_back(e); }
        return (int)nev++;
    }
    // chain = true: this launch directly follows the previous timed launch on the same stream, so that
    // launch's stop marker doubles as this one's start (one marker per kernel instead of two: every
    // marker costs a few microseconds of idle GPU between dependent kernels)
    int begin(hipStream_t s, int k, bool chain = false) {
        if (!on) return -1;
        ++seen[k];
        if (skip) return -1;
        int st = (chain && last_stop >= 0) ? last_stop : fresh();
        if (st < 0) return -1;
        if (!(chain && last_stop >= 0)) (void)hipEventRecord(ev[st], s);
        if (used >= kind.size()) { kind.resize(used + 512); e0.resize(used + 512); e1.resize(used + 512); }
        kind[used] = k; e0[used] = st; e1[used] = -1;
        return (int)used++;
    }
    void end(hipStream_t s, int slot) {
        if (slot < 0) return;
        const int sp = fresh();
        if (sp < 0) return;
        (void)hipEventRecord(ev[sp], s);
        e1[slot] = sp; last_stop = sp;
    }
    void unchain() { last_stop = -1; }          // something else was launched in between
    void collect() {       // call after the stream has been synchronised
        for (size_t i = 0; i < used; ++i) {
            float t = 0;
            if (e1[i] >= 0 && hipEventElapsedTime(&t, ev[e0[i]], ev[e1[i]]) == hipSuccess) { ms[kind[i]] += t; cnt[kind[i]] += 1; }
        }
        used = 0; nev = 0; last_stop = -1;
    }
    ~KernelProf() { for (auto e : ev) (void)hipEventDestroy(e); }
};

// exact conditional draws (hmc_exact.h): M = I + ZL' ZL / sigma^2 and its factor, the Q x ncols right-hand sides / draws, the
// Q-vector b -> w; kept between calls (Q x Q: 200 MB at Q = 5000).  prof: HIP events around the phases of the next calls
struct ExactState {
    DevMat M, T;
    DevBuf b;
    bool prof = false;
    double ms[5] = {0, 0, 0, 0, 0};   // M build | factorisation | right-hand side + fill | transposed solve | L V, of the last call
};

// component-wise exact draws (hmc_exact_comp.h): the factors of every M_c, b -> mu*, the draws chain-major and transposed;
// kept between calls
struct ExactCompState {
    CompFactors f;
    DevBuf b, mu, CM;
    DevMat T;
    bool prof = false;
    double ms[5] = {0, 0, 0, 0, 0};     // factor + mean | draw kernel | transpose | L V | 0, of the last call
};

// the GLS information query (info.hip): beta, the reciprocal weights v, XV = diag(v) X, the right-hand sides / S (Q x P), the
// Gram partials and the result with its two flags; the dense operator's M and ZLTW, the component operator's factors; kept
// between calls.  plan: what the last call did (glmmr_mcml_dbg_information_plan)
struct InfoState {
    DevBuf beta, v, bad, part, res;
    CompFactors f;
    DevMat XV, S, M, ZLTW;
    int waves = 0;                      // of the factor kernel of the last component front half (info_front)
    long long plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// the information of the covariance parameters (theta_info.hip).  Dense operator: B = M^-1 N, the matrix at hand d_r D -> E_r, its
// transposition, and one G_r = B E_r per parameter (Q x Q each); component operator: the block of every variable and the
// per-component partials; the contraction's partials and the result with its two flags; kept between calls.  plan: what the last
// call did (glmmr_mcml_dbg_theta_information_plan)
struct ThetaInfoState {
    DevMat B, E, T;
    std::vector<DevMat> G;
    DevBuf gptr, blk_of_var, part, tr, res;
    long long plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// the small-sample query (small_sample.hip): c = M^-1 ZL' V X and d = L^-T c (Q x P), W = every U_r and V_rs side by side
// (Q x (R + the pairs of parameters a block reads together) P), T / Y = the columns on their way to (Z' Sigma^-1 Z) U_r; gaussian / identity: A = Sigma^-1 X,
// V A, A2 = Sigma^-1 A, ZL c (n x P), c2, d2 (Q x P); the work items of k_ss_apply, the jobs and partials of k_ss_gram and the
// result I_beta | 2 flags | I_theta | P | Q | R; kept between calls.  plan: what the last call did
// (glmmr_mcml_dbg_small_sample_plan)
struct SmallSampleState {
    DevMat C, Dm, W, T, Y, A, VA, A2, ZC, C2, D2;
    DevBuf work, jobs, part, res;
    long long plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// the sandwich query (sandwich.hip): the residual flag, the working residual e, v o e, a = Sigma^-1 e, the right-hand side / t (Q),
// ZL t (dense operator), the clusters' CSR, the meat's partials and the result B | 2 flags | G; kept between calls.  plan: what
// the last call did (glmmr_mcml_dbg_sandwich_plan)
struct SandwichState {
    DevBuf bad, e, ve, a, t, zt, cl_ptr, cl_rows, part, res;
    long long plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// the prediction query (predict.hip): the new points' data, the K x 3 summary, the large block at hand -- its matrix / factor D,
// the solved samples Y, the chunk of C_b' / W' -- and the means of the chunks not yet flushed; allocated by the first call, kept
// between calls.  plan: what the last call did (glmmr_mcml_dbg_predict_plan)
struct PredictState {
    DevBuf nd, sum;
    DevMat D, Y, CT, M;
    long long plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;

    // problem
    int n = 0, Q = 0, P = 0, flink = 0, link_code = 0;
    int z_width = 0;            // > 0: Z also held as padded-CSR rows of this width
    DevBuf z_idx, z_val;        // n x z_width (column-major)
    std::vector<int> h_zidx; std::vector<double> h_zval;   // host copy of the same
    SparseZL sp;
    ComponentDev cp;
    int traj_mode = 0;          // 0: a launch per leapfrog step; 1: component-local trajectories where feasible (hmc_traj.h)
    int draws_mode = 0;         // hmc_sample: 0 HMC trajectories; 1 exact conditional draws where the target is Gaussian (hmc_exact.h);
                                // 2 the same, and component by component where the sparse operator runs (hmc_exact_comp.h)
    ExactState exact;
    ExactCompState exact_comp;
    InfoState info;
    ThetaInfoState tinfo;
    SmallSampleState ss;
    SandwichState sand;
    PredictState predict;
    bool no_sparse_zl = false;  // the Laplace path works on the dense ZL / ZLT
    int la_mode = 0;            // Laplace fits: 0 dense ZL and M; 1 the component operator where feasible (component.hip); 2 the same up
                                // to CP_WIDE_MAX_VARS variables per component, a wave or a workgroup each
    int la_last_op = 0;         // what the last Laplace call ran (0 dense, 1 component, 2 component_wide), its waves per
    int la_waves = 0;           // component (0 dense, 1, 4), its k_lac_factor / k_lac_factor_wg launches and the
    long long la_launches = 0, la_dense_bytes = 0;   // bytes of M + ZLTW + ZL + ZLT it allocated / worked on (dbg_la_plan)
    bool l_foreign = false;     // L came from the caller (set_L), not from theta: it need not have the block pattern the
                                // sparse ZL operator assumes; cleared as soon as L is regenerated from theta (mvn_gen_L)
    CovSpec cov;
    DevMat Z, X;                // n x Q, n x P
    DevBuf y;                   // n
    DevBuf y_given;             // n, gaussian / log only: y before model_setup took its logarithm (sandwich.hip)
    DevBuf d_cov, d_data, d_blocks, d_rowblock;   // covariance spec on the device

    // samples
    DevMat U;                   // Q x mcols (u = L v)
    int mcols = 0;              // columns held (theta-step uses all: mcmldmatrix.h:24)
    int niter = 0;              // columns the beta-step uses (mcmlmodel.h:73,296)
    int m_global = 0, niter_global = 0;   // across ranks (== local when single rank)
    DevMat ZU;                  // n x mcols, cached Z u
    bool zu_valid = false;

    // model state
    DevMat L, ZL, ZLT;          // Q x Q lower factor of D; n x Q; Q x n
    BandPlan plan_fwd, plan_bwd;   // nonzero K-tile range and row-tile extents of every 80-row band of ZL / ZLT + the work decomposition (dgemm_band.h)
    DevBuf kr_scratch;
    bool band_fwd = false, band_bwd = false;   // the structural zeros are worth skipping
    DevBuf xb;                  // n
    bool have_L = false;

    // MVN workspaces
    DevMat Dwork;               // maxdim x maxdim
    DevBuf partials;            // reduction partials
    DevBuf scalars;             // 64 small device scalars (doubles): [0..3] mvn_ll, [4] model log-likelihood, [8..15] sampler
                                // diagnostics, [16] the "not positive definite" flag (int), [17..] sampler step counts (ints)
    int* errflag() const { return reinterpret_cast<int*>(scalars.d() + 16); }
    int maxdim_large = 0;       // largest block that takes the blocked (dense) path
    int n_small = 0, n_diag_rows = 0;
    DevBuf small_ids;                           // ids of the small dense blocks (mvn_setup), for k_small_ll

    // sampler
    int last_kernel[2] = {-1, -1};   // kernel family of the last forward / backward product (KERNEL_*)
    HmcState hmc;
    NutsState nuts;
    KernelProf prof;

    // distribution
    int rank = 0, world = 1;
    reduce_fn reduce = nullptr;
    void* reduce_user = nullptr;
    void* comm = nullptr;       // ncclComm_t of the native RCCL path (comm.hip); null = hook or single process
    long long coll_calls = 0, coll_doubles = 0;   // collectives issued / doubles summed (tests, bench)
    long long gather_calls = 0, gather_doubles = 0;   // all-gathers issued / doubles received
    // every rank's sample columns (comm.hip allgather_dev): rank r's mcols columns at column r * mcols.  Valid until the
    // samples change.  The theta-step of a sharded job reads these (drivers.hip::d_optim).
    DevMat Uall;
    bool uall_valid = false;
    bool theta_log_on = false;          // tests: every MVN objective evaluation as (theta..., log-likelihood)
    std::vector<double> theta_log;
    long long theta_rounds = 0, theta_evals_own = 0, theta_evals_all = 0;   // sharded theta-step: exchanges, evaluations here / everywhere
    long long theta_factorised = 0;     // ... and the matrices this rank actually factorised for them (theta_scale.h)
    std::vector<int> theta_scale_p;     // scale exponents of the covariance parameters (theta_scale.h), set by mvn_setup
    // rank emulation on one GPU (bench.py --as-rank-of N, include/glmmr_mcml_c.h glmmr_mcml_dbg_emulate_world): the
    // other ranks are copies of this one -- a sum is `emu_world` times the local value, a gather `emu_world` copies of
    // the local block; the candidate thetas of the other ranks are evaluated here too (mode 1, values recorded) or taken
    // from that record (mode 2: only this rank's share runs, which is what a rank of the real job executes)
    int emu_world = 0, emu_mode = 0;
    std::vector<std::vector<double>> emu_trace; size_t emu_pos = 0;
    DevBuf reduce_buf;          // doubles handed to the collective
    DevBuf scratch;             // short-lived per-call scratch

    DevMat Dbatch;                                   // mvn_loglik_batch: the candidates' matrices side by side
    DevBuf bscal;                                    // ... and their result scalars (4 per candidate)
    // tests (glmmr_mcml_dbg_mvn_workspace): what mvn_large_blocks last left in Dwork [0] / Dbatch [1] -- the block's
    // dimension d, round_up(d, 16), the sample rows m, the leading dimension, the number of matrices (0: no call yet)
    struct MvnWs { int d = 0, dp = 0, m = 0, ld = 0, kb = 0; } mvn_ws[2];
    // the analytic score of mvn_ll (mvn_grad.h): everything is allocated by the first gradient call, so a context that never
    // asks pays nothing; Dwork and chol.linv are only read.  S / T: X' diag(w) X - (sum w) I and H of the large block at hand,
    // Xw: the weighted copy of its solved sample rows; a dense block's parameters are slots [slot_base, + slot_count) of
    // slot_par (the parameter index each adds to), small blocks first
    struct MvnGrad {
        bool ready = false;
        DevMat S, T, Xw;
        DevBuf w, diag, part, part_small, small_tab, res;
        std::vector<int> slot_base, slot_count, slot_par;
        std::vector<int> slot_scale;     // per slot: c where dlog is the constant c / theta over the whole block (0: it is not)
        int n_small_slots = 0, res_len = 0;
    } grad;
    // the dense Cholesky stack (chol.h): inverted diagonal blocks, side streams + events, graph cache.  Last member: it is
    // torn down first, right after the communicator
    CholState chol;
    ~Ctx() { comm_release_hook(); }

    int sync() { MCML_HIP(hipStreamSynchronize(stream)); return MCML_OK; }
    void comm_release_hook();
};

// ---- comm.hip ----
void comm_release(Ctx& c);
int allreduce_dev(Ctx& c, double* dev, int n);              // in place on device memory, on c.stream
int allgather_dev(Ctx& c, const double* send, double* recv, size_t count);
int gather_samples(Ctx& c);                                  // c.Uall <- all ranks' sample columns
inline int comm_world(const Ctx& c) { return c.emu_world > 1 ? c.emu_world : c.world; }
inline bool comm_emulated(const Ctx& c) { return !c.comm && c.world <= 1 && c.emu_world > 1; }   // rank emulation is on
inline void Ctx::comm_release_hook() { comm_release(*this); }

// ---- mvn.hip ----
int mvn_setup(Ctx& c);
// sum over the locally held columns of sum_b log N(u_b; 0, D_b(theta))
int mvn_loglik_sum(Ctx& c, const double* theta, double* sum_out);
// the same over the m columns of any resident sample matrix (Q x m, leading dimension ldu)
int mvn_loglik_sum_on(Ctx& c, const double* theta, const double* U, int ldu, int m, double* sum_out);
// k candidate thetas (npar x k, column-major) factorised side by side: sums[j], rcs[j] = MCML_OK | MCML_ENOTPD
int mvn_loglik_batch(Ctx& c, const double* thetas, int k, const double* U, int ldu, int m, double* sums, int* rcs);
// the k representatives of a round of `round` > 1 candidates, dense-block models only: as mvn_loglik_batch, and
// parts[2 j], parts[2 j + 1] = candidate j's log-determinant and sum of squares (theta_scale.h)
int mvn_loglik_batch_parts(Ctx& c, const double* thetas, int k, int round, const double* U, int ldu, int m, double* sums,
                           int* rcs, double* parts);
// c.L = genD(0, chol=true, upper=false) (mcml_full.cpp:68): block-diagonal lower factor; have_L = chol.  A build that
// fails (a block that is not positive definite) leaves have_L false: c.L is overwritten in place
int mvn_gen_L(Ctx& c, const double* theta, bool chol);
// value = sum_j w_j sum_b log N(u_bj; 0, D_b(theta)) over the locally held columns and grad[k] = d value / d theta_k, k < npar
// (mvn_grad.h).  weights: mcols host values, or null for 1 each -- value is then mvn_loglik_sum's to the bit.  A query
int mvn_loglik_grad(Ctx& c, const double* theta, const double* weights, double* value, double* grad);
// the same matrix as a query: built into `out` (allocated here), no state of the context changes
int mvn_gen_D(Ctx& c, const double* theta, bool chol, DevMat& out);
// block b's matrix alone, lower triangle with an identity border up to dpad, into A (enqueued; no state changes)
int mvn_build_block(Ctx& c, double* A, int lda, int b, const double* theta, int dpad);

// ---- chol.hip: see chol.h; vecops.hip (the vector-sized kernels): see vecops.h; component.hip: see component.h ----

// ---- laplace.hip ----
// M (Q x Q) = ZL' diag(W) ZL + I from the current c.ZL / c.ZLT.  W null: W = w0 for every observation, ZLT is multiplied as it
// is (ZLTW is not touched).  lower_only: the tiles strictly above the diagonal are left zero
int build_M_dense(Ctx& c, const double* W, double w0, DevMat& M, DevMat& ZLTW, bool lower_only);

// ---- model.hip ----
int model_setup(Ctx& c, const double* Z, const double* X, const double* y);
int allreduce_host(Ctx& c, double* vals, int n);             // comm.hip
int exchange_round(Ctx& c, std::vector<double>& vals);      // comm.hip: a round's candidate values, each set on its owner
int model_update_beta(Ctx& c, const double* beta);          // xb = X beta
int model_update_zu(Ctx& c);                                // ZU = Z U (cached)
int model_update_L(Ctx& c);                                 // ZL = Z L, ZLT (dense) or the ELL/CSR pair (sparse)
int model_sparse_setup(Ctx& c);                             // the sparse ZL pattern and the component plan, if not built yet
int model_loglik_sum(Ctx& c, double var_par, double* sum_out);
int model_mcnr_stats(Ctx& c, double var_par, double* stats /* P*P + P + 2 */);
int mcnr_finish(int P, const double* stats, const double* beta, double* beta_out, double* sigma_out);

// ---- hmc.hip (the samplers: entry.h) ----
int hmc_dbg_log_prob_grad(Ctx& c, const double* beta, double var_par, const double* V, int ncols, double* lp,
                          double* G);

}  // namespace mcml

// the opaque handle of include/glmmr_mcml_c.h
struct glmmr_mcml_ctx { mcml::Ctx c; };
