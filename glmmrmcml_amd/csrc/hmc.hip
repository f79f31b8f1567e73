// hmc.hip -- the random-effects HMC sampler, mcmcRunHMC (mhmcmc.h:16-160), run as
// C independent chains at once.
//
// The reference runs ONE chain whose every leapfrog step is two n x Q GEMVs that
// stream ZL (200 MB at n = Q = 5000) and are strictly sequential.  Here the
// chains are the columns of Q x C state matrices, so one leapfrog step of all
// chains is two FP64-MFMA GEMMs that read ZL once:
//     forward   MU = xb + ZL * UP ,  S = s(y, MU)          (n x Q x C)
//     backward  g  = -UP + post * ZL' * S                   (Q x n x C)
// with the score and the leapfrog update fused into the GEMM epilogues.  Each
// chain keeps its own step size / dual-averaging state (mhmcmc.h:107-116), its
// own minstd accept stream (:27,55,85) and its own number of steps; chains that
// have finished their trajectory are masked in the backward epilogue.
// log_prob(u) and log_grad(u) of the current state are cached from the step that
// produced it instead of being recomputed (the reference recomputes them,
// :64,82): same numbers, 2*steps GEMMs per proposal instead of 2*steps + 4.
#include <algorithm>
#include <atomic>
#include <chrono>
#include "entry.h"
#include "dgemm_mfma.h"
#include "dgemm_dlds.h"
#include "dgemm_band.h"
#include "dgemm_skinny.h"
#include "glm.h"
#include "reduce.h"
#include "rng.h"
#include "hmc_chain.h"
#include "hmc_cm.h"
#include "hmc_traj.h"

namespace mcml {

// ------------------------------------------------------------------ GEMM epilogues
// forward: MU = xb + acc ; S = score(y, MU)          (mcmlmodel.h:160-162,169-276)
// store_mu = 0: inside a leapfrog trajectory only the score feeds the next product; the linear
// predictor itself is read (by k_hmc_accept) after the LAST step only, so its 8 n C bytes per
// launch are not written
// FL: the family / link code as a compile-time constant (12 = beta/logit, whose digamma score is its own function,
// glm.h; 1, 3, 7 = poisson/log, binomial/logit, gaussian/identity), 0 = run-time code: the epilogue evaluates the score
// 20 times per lane, unrolled -- with a run-time code that is twenty copies of glm_score's switch
template <int FL>
struct EpiForwardT {
    double* MU; double* S; int ld; const double* xb; const double* y; int flink; int store_mu; double var_par;
    __device__ __forceinline__ double score(double yv, double mu) const {
        if constexpr (FL == 12) return glm_score_beta(yv, mu, var_par);
        else return glm_score(yv, mu, FL ? FL : flink);
    }
    __device__ __forceinline__ void elem(int m, int n, double accv) const {
        const double mu = xb[m] + accv;
        if (store_mu) MU[m + (size_t)n * ld] = mu;
        S[m + (size_t)n * ld] = score(y[m], mu);
    }
    // Three phases -- all loads, all arithmetic, all stores -- with no use of a loaded register after the first
    // store.  The compiler's waitcnt insertion cannot count stores issued under divergent control flow, so any
    // such use gets `s_waitcnt vmcnt(0)`, and vector memory completes in order: that wait also drains every store
    // issued so far (one memory round trip per row group, ~1-2 us each with every CU storing at once).
    template <int TM, int TN>
    __device__ __forceinline__ void operator()(d4 (&acc)[TM][TN], int mB, int nB, int lane, int M, int N,
                                               int) const {
        double xbv[TM], yv[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = mB + 16 * i + (lane & 15);
            const int mm = m < M ? m : 0;
            xbv[i] = xb[mm]; yv[i] = y[mm];
        }
        double sc[TM][TN][4];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double mu = xbv[i] + acc[i][j][r];
                    acc[i][j][r] = mu;
                    sc[i][j][r] = score(yv[i], mu);
                }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nB + 16 * j + (lane >> 4) + 4 * r;
                if (n >= N) continue;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int m = mB + 16 * i + (lane & 15);
                    if (m < M) {
                        if (store_mu) MU[m + (size_t)n * ld] = acc[i][j][r];
                        S[m + (size_t)n * ld] = sc[i][j][r];
                    }
                }
            }
    }
};

// backward: g = -x + post*acc.  mode 0: GRAD = g (initial state).
// mode 1 (leapfrog step s): for chains with s < steps: GRADP = g; R += e/2 g;
// and, unless it was the chain's last step, R += e/2 g; UP += e R   (mhmcmc.h:73-78)
struct EpiBackward {
    const double* Xs; double* G; double* R; double* UP; int ld;
    const double* e; const int* steps; int s; double post; int mode;
    __device__ __forceinline__ void elem(int m, int n, double accv) const {
        int st = 0; double en = 0.0;
        if (mode == 1) { st = steps[n]; en = e[n]; if (s >= st) return; }
        const size_t off = m + (size_t)n * ld;
        const double x = Xs[off];
        double g = -1.0 * x;
        g = g + post * accv;
        if (mode != 1 || s + 1 >= st) G[off] = g;     // mid-trajectory gradients are never read
        if (mode == 1) {
            double rr = R[off];
            rr = rr + (en / 2) * g;
            if (s + 1 < st) {
                rr = rr + (en / 2) * g;
                UP[off] = x + en * rr;
            }
            R[off] = rr;
        }
    }
    // Per 16-column group: all loads (from clamped, always valid addresses), then all arithmetic into
    // registers, then all stores, and no use of a loaded register after the first store (see EpiForwardT: such a
    // use costs `s_waitcnt vmcnt(0)`, which drains the stores issued so far -- one memory round trip per
    // element group).  Arithmetic order per element is elem()'s; the choices it makes with branches are selects.
    template <int TM, int TN>
    __device__ __forceinline__ void operator()(d4 (&acc)[TM][TN], int mB, int nB, int lane, int M, int N,
                                               int) const {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int stv[4]; double env[4]; bool inN[4]; size_t cb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nB + 16 * j + (lane >> 4) + 4 * r;
                inN[r] = n < N;
                const int nn = inN[r] ? n : 0;
                stv[r] = mode == 1 ? steps[nn] : 0;
                env[r] = mode == 1 ? e[nn] : 0.0;
                cb[r] = (size_t)nn * ld;
            }
            double xv[TM][4], rv[TM][4];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mB + 16 * i + (lane & 15);
                const int mm = m < M ? m : 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    xv[i][r] = Xs[mm + cb[r]];
                    rv[i][r] = mode == 1 ? R[mm + cb[r]] : 0.0;
                }
            }
            // g -> acc, new R -> rv, new UP -> xv
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double en = env[r];
                const bool more = s + 1 < stv[r];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const double x = xv[i][r];
                    double g = -1.0 * x;
                    g = g + post * acc[i][j][r];
                    acc[i][j][r] = g;
                    double rr = rv[i][r];
                    rr = rr + (en / 2) * g;
                    const double rr2 = rr + (en / 2) * g;
                    rr = more ? rr2 : rr;
                    rv[i][r] = rr;
                    xv[i][r] = x + en * rr;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool act = inN[r] && (mode != 1 || s < stv[r]);
                if (!act) continue;
                const bool more = s + 1 < stv[r];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int m = mB + 16 * i + (lane & 15);
                    if (m >= M) continue;
                    const size_t off = m + cb[r];
                    if (mode != 1 || !more) G[off] = acc[i][j][r];       // mid-trajectory gradients are never read
                    if (mode == 1) {
                        if (more) UP[off] = xv[i][r];
                        R[off] = rv[i][r];
                    }
                }
            }
        }
    }
};

// The banded products run the feeder form of the kernel (dgemm_band.h) with the epilogues whose instantiation of it
// compiles without scratch
template <> struct BandFeed<EpiBackward> { static constexpr bool ok = true; };
template <> struct BandFeed<EpiForwardT<1>> { static constexpr bool ok = true; };
template <> struct BandFeed<EpiForwardT<3>> { static constexpr bool ok = true; };
template <> struct BandFeed<EpiForwardT<7>> { static constexpr bool ok = true; };

// ------------------------------------------------------------------ sparse ZL products
// The forward / backward products of the sparse operator and the per-chain kernels that go with them live in
// hmc_cm.h: with a sparse ZL the whole sampler state is chain-major.

// U = L V for a block-diagonal L with small blocks (the sparse-ZL configurations): row q of L has entries in
// columns start(q) .. q only.  Dense, this product is Q x Q x m (22 ms at config 5 for what is a diagonal scaling).
__global__ __launch_bounds__(256) void k_blockdiag_LV(int Q, int ncols, const int* start, const double* L, int ldl,
                                                      const double* V, int ldv, double* U, int ldu)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int s0 = start[q];
    for (int c = blockIdx.y; c < ncols; c += gridDim.y) {
        const double* v = V + (size_t)c * ldv;
        double acc = 0.0;
        for (int t = s0; t <= q; ++t) acc += L[q + (size_t)t * ldl] * v[t];
        U[q + (size_t)c * ldu] = acc;
    }
}

// ------------------------------------------------------------------ per-chain kernels
__global__ __launch_bounds__(256) void k_hmc_init(double* V, int ld, int Q, ChainArrays ca, uint64_t seed,
                                                  uint32_t chain_offset, uint32_t iter_idx, const double* inj_init)
{
    const int c = blockIdx.x;
    const uint32_t gid = chain_offset + (uint32_t)c;
    for (int q = threadIdx.x; q < Q; q += 256)
        V[q + (size_t)c * ld] = inj_init ? inj_init[q + (size_t)c * Q]
                                         : rng_normal(seed, (uint32_t)q, gid, 0u, 16u * iter_idx + 0u);
    if (threadIdx.x == 0) chain_reset(ca, c, seed, gid, iter_idx);
}

// log_prob of column c: sum_i logf(y_i | MU_ic) + sum_k logN(x_k; 0, 1)   (mcmlmodel.h:138-153)
// FL != 0: the family / link is a compile-time constant -- the 12-way switch of glm_logpdf with its lgamma / tgamma / erfc
// bodies inlined costs 302 VGPRs (one wave per SIMD) in every kernel that calls it with a run-time code
template <int FL>
__device__ __forceinline__ double chain_log_prob(const double* MU, int ldm, int n, const double* X, int ldx,
                                                 int Q, const double* y, double var_par, int flink_rt, int c,
                                                 double* sh)
{
    const int flink = FL ? FL : flink_rt;
    // loads batched four deep (the kernel is latency-bound: 4 workgroups per CU); each thread still adds its
    // own elements in index order, so the sums are bit-identical to the plain loop
    double ll = 0, lp = 0;
    for (int i0 = threadIdx.x; i0 < n; i0 += 1024) {
        double m4[4], y4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 256 * u;
            m4[u] = i < n ? MU[i + (size_t)c * ldm] : 0.0;
            y4[u] = i < n ? y[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + 256 * u < n) ll += glm_logpdf(y4[u], m4[u], var_par, flink);
    }
    for (int k0 = threadIdx.x; k0 < Q; k0 += 1024) {
        double x4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int k = k0 + 256 * u; x4[u] = k < Q ? X[k + (size_t)c * ldx] : 0.0; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k0 + 256 * u < Q) lp += glm_logpdf(x4[u], 0, 1, 7);
    }
    double a = block_sum(ll, sh);
    double b = block_sum(lp, sh);
    return a + b;    // valid in thread 0
}

template <int FL>
__global__ __launch_bounds__(256) void k_hmc_lp0(const double* MU, int ldm, int n, const double* V, int ld, int Q,
                                                 const double* y, double var_par, int flink, double* lpcur)
{
    __shared__ double sh[4];
    double v = chain_log_prob<FL>(MU, ldm, n, V, ld, Q, y, var_par, flink, blockIdx.x, sh);
    if (threadIdx.x == 0) lpcur[blockIdx.x] = v;
}

// new_proposal, first part (mhmcmc.h:62-75): momentum, K0, steps, first half step + position
__global__ __launch_bounds__(256) void k_hmc_propose(const double* V, const double* GRAD, double* R, double* UP,
                                                     int ld, int Q, ChainArrays ca, double lambda, int max_steps,
                                                     uint64_t seed, uint32_t chain_offset, uint32_t iter_idx,
                                                     int it, const double* inj_mom, int C)
{
    __shared__ double sh[4];
    const int c = blockIdx.x;
    const uint32_t gid = chain_offset + (uint32_t)c;
    const double e = ca.e[c];
    double ss = 0;
    for (int q = threadIdx.x; q < Q; q += 256) {
        const size_t off = q + (size_t)c * ld;
        double r = inj_mom ? inj_mom[q + ((size_t)it * C + c) * Q]
                           : rng_normal(seed, (uint32_t)q, gid, (uint32_t)it, 16u * iter_idx + 2u);
        ss += r * r;
        const double g = GRAD[off], v = V[off];
        r = r + (e / 2) * g;
        R[off] = r;
        UP[off] = v + e * r;
    }
    double tot = block_sum(ss, sh);
    if (threadIdx.x == 0) chain_begin_proposal(ca, c, tot, lambda, max_steps);
}

// slot (nullable): host memory mapped into the device -- the count goes there too, tagged with the proposal's sequence number,
// as one 64-bit system-scope store (hmc_sample reads it back with plain loads)
__global__ void k_max_steps(const int* steps, int C, int* out, unsigned long long* slot = nullptr, unsigned seq = 0)
{
    __shared__ int sh[256];
    int v = 0;
    for (int i = threadIdx.x; i < C; i += 256) v = max(v, steps[i]);
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + o]); __syncthreads(); }
    if (threadIdx.x == 0) {
        out[0] = sh[0];
        if (slot) __hip_atomic_store(slot, ((unsigned long long)seq << 32) | (unsigned)sh[0], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// new_proposal, second part (mhmcmc.h:80-117)
template <int FL>
__global__ __launch_bounds__(256) void k_hmc_accept(double* V, double* GRAD, const double* R, const double* UP,
                                                    const double* GRADP, int ld, int Q, const double* MU, int ldm,
                                                    int n, const double* y, double var_par, int flink,
                                                    ChainArrays ca, double target_accept, int adapt, int it,
                                                    int C, uint8_t* flags, double* probs)
{
    __shared__ double sh[4];
    __shared__ int acc_s;
    const int c = blockIdx.x;
    double l2 = chain_log_prob<FL>(MU, ldm, n, UP, ld, Q, y, var_par, flink, c, sh);
    double kin = 0;
    for (int k0 = threadIdx.x; k0 < Q; k0 += 1024) {
        double r4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int k = k0 + 256 * u; r4[u] = k < Q ? R[k + (size_t)c * ld] : 0.0; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k0 + 256 * u < Q) kin += r4[u] * r4[u];
    }
    kin = block_sum(kin, sh);
    if (threadIdx.x == 0) acc_s = chain_decide(ca, c, l2, kin, target_accept, adapt, it, C, flags, probs);
    __syncthreads();
    const int acc = acc_s;
    if (acc)
        for (int k0 = threadIdx.x; k0 < Q; k0 += 1024) {
            double u4[4], g4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 256 * u;
                const size_t off = (k < Q ? k : 0) + (size_t)c * ld;
                u4[u] = UP[off]; g4[u] = GRADP[off];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 256 * u;
                if (k < Q) { const size_t off = k + (size_t)c * ld; V[off] = u4[u]; GRAD[off] = g4[u]; }
            }
        }
}

// store the current state of every chain as sample columns c*stride + col
__global__ __launch_bounds__(256) void k_hmc_store(const double* V, int ld, int Q, double* SAMP, int lds,
                                                   int stride, int col)
{
    const int c = blockIdx.x;
    for (int k = threadIdx.x; k < Q; k += 256) SAMP[k + (size_t)(c * stride + col) * lds] = V[k + (size_t)c * ld];
}

__global__ void k_hmc_diag(ChainArrays ca, int C, double* out)
{
    // out: [0] sum accept, [1] sum e, [2] min e, [3] max e, [4] max steps, [5] sum leapfrog
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sa = 0, se = 0, mn = 1e300, mx = 0, ms = 0, sl = 0;
    for (int c = 0; c < C; ++c) {
        sa += ca.acc[c]; se += ca.e[c];
        mn = fmin(mn, ca.e[c]); mx = fmax(mx, ca.e[c]);
        ms = fmax(ms, (double)ca.steps[c]); sl += (double)ca.leap[c];
    }
    out[0] = sa; out[1] = se; out[2] = mn; out[3] = mx; out[4] = ms; out[5] = sl;
}

// ------------------------------------------------------------------ host
// component-local trajectories (hmc_traj.h): asked for, the sparse operator is active and every component fits the kernel
static bool cm_traj_used(const Ctx& c) { return c.traj_mode == 1 && c.sp.active && c.cp.ready && c.cp.plan.feasible; }

// k_cm_traj launches of this process, over all contexts (glmmr_mcml_dbg_traj_launches: the contexts the one-shot exports
// create cannot be asked which kernels they ran)
static std::atomic<long long> g_traj_launches{0};
long long cm_traj_launch_count() { return g_traj_launches.load(); }

// one proposal's trajectories of every (component, chain): ONE launch whatever the step counts
static int cm_traj_launch(Ctx& c, const TrajArgs& a)
{
    const CompView m = comp_view(c);
    const int waves = cp_waves(c.cp.plan, cp_forced_waves(CP_TRAJ_WAVES_ENV));
    const int lds = cp_lds_bytes(m.max_vars, waves);
    const dim3 grid(m.nitems, cm_chain_blocks(a.C));
    MCML_TRY((dispatch_flink<1, 3, 7, 12>(c.flink, [&](auto FL) {
        if (waves == 4) {
            MCML_TRY(ensure_dynamic_lds((const void*)k_cm_traj<FL(), 4>, cp_lds_bytes(CP_MAX_VARS, 4)));
            hipLaunchKernelGGL((k_cm_traj<FL(), 4>), grid, dim3(256), lds, c.stream, m, a);
        } else {
            MCML_TRY(ensure_dynamic_lds((const void*)k_cm_traj<FL(), 1>, cp_lds_bytes(CP_MAX_VARS, 1)));
            hipLaunchKernelGGL((k_cm_traj<FL(), 1>), grid, dim3(64), lds, c.stream, m, a);
        }
        return (int)MCML_OK;
    })));
    MCML_HIP(hipGetLastError());
    ++g_traj_launches;                           // launches that were actually enqueued
    return MCML_OK;
}

static int hmc_alloc(Ctx& c, int C)
{
    HmcState& h = c.hmc;
    h.C = C; h.Cw = C;
    h.cm = c.sp.active;
    // chain-major state (sparse operator, hmc_cm.h): the "rows" of a DevMat are the chains
    auto mat = [&](DevMat& m, int len) { return h.cm ? m.alloc(C, len) : m.alloc(len, C); };
    for (DevMat* m : {&h.V, &h.R, &h.UP, &h.GRAD, &h.GRADP}) MCML_TRY(mat(*m, c.Q));
    MCML_TRY(mat(h.MU, c.n)); MCML_TRY(mat(h.S, c.n));
    MCML_TRY(h.chain.ensure(sizeof(double) * (size_t)round_up(C, 16) * 8));
    if (h.cm) {
        const size_t nchn = (size_t)(c.n + CM_ROWS - 1) / CM_ROWS, nchq = (size_t)(c.Q + cm_qrows(c.Q) - 1) / cm_qrows(c.Q);
        MCML_TRY(h.cm_part.ensure(sizeof(double) * (nchn + 3 * nchq + 4) * (size_t)h.V.ld));
        MCML_TRY(h.cm_acc.ensure(sizeof(int) * (size_t)round_up(C, 64)));
        if (c.sp.factored) { MCML_TRY(h.LX.alloc(C, c.Q)); MCML_TRY(h.ZS.alloc(C, c.Q)); }
        if (cm_traj_used(c)) MCML_TRY(h.cp_part.ensure(sizeof(double) * 4 * (size_t)c.cp.plan.nitems() * h.V.ld));
        return MCML_OK;
    }
    // padding rows of the operands the GEMMs read must hold finite values
    MCML_HIP(hipMemsetAsync(h.V.d(), 0, sizeof(double) * (size_t)h.V.ld * C, c.stream));
    MCML_HIP(hipMemsetAsync(h.UP.d(), 0, sizeof(double) * (size_t)h.UP.ld * C, c.stream));
    MCML_HIP(hipMemsetAsync(h.S.d(), 0, sizeof(double) * (size_t)h.S.ld * C, c.stream));
    return MCML_OK;
}

// direct-to-LDS GEMM (dgemm_dlds.h) unless GLMMR_MCML_GEMM=reg asks for the register-staged one
static bool use_dlds()
{
    static int v = -1;
    if (v < 0) { const char* e = getenv("GLMMR_MCML_GEMM"); v = (e && !strcmp(e, "reg")) ? 0 : 1; }
    return v == 1;
}

static bool use_skinny()                       // GLMMR_MCML_SKINNY=0: the MFMA kernels whatever the column count
{                                              // (read per call: the parity tests run both paths in one process)
    const char* e = getenv("GLMMR_MCML_SKINNY");
    return !(e && !strcmp(e, "0"));
}

// The dense product of one direction (dir 0: forward, A = ZL; 1: backward, A = ZL') with the h.Cw columns of B, by the
// first kernel family that applies.
struct DenseOp { BandPlan& plan; bool band; int M, K; const DevMat& A; };
template <class Epi>
static int dense_product(Ctx& c, int dir, const DenseOp& a, const double* B, int ldb, const Epi& epi)
{
    const int N = c.hmc.Cw, lda = a.A.ld;
    const double* A = a.A.d();
    // at most 16 chains (chains = 1: the reference's layout; the tail of a NUTS doubling): an HBM-bound stream, not an MFMA tile
    // c.last_kernel[]: which kernel family served the product (tests assert the path they mean to compare)
    if (use_skinny() && skinny_applicable(a.plan, a.M, a.K, N, lda)) {
        c.last_kernel[dir] = KERNEL_SKINNY;
        return launch_skinny(c.stream, a.plan, N, A, lda, B, ldb, epi);
    }
    if (a.band && dlds_applicable(a.M, N, a.K, A, lda, a.A.cols_alloc, B, ldb)) {
        c.last_kernel[dir] = KERNEL_BAND;
        return launch_gemm_band(c.stream, a.plan, N, A, lda, B, ldb, epi);
    }
    if (use_dlds() && dlds_applicable(a.M, N, a.K, A, lda, a.A.cols_alloc, B, ldb)) {
        c.last_kernel[dir] = KERNEL_DLDS;
        return launch_gemm_dlds(c.stream, a.M, N, a.K, A, lda, B, ldb, epi);
    }
    c.last_kernel[dir] = KERNEL_REG;
    return launch_gemm<false>(c.stream, a.M, N, a.K, A, lda, B, ldb, epi);
}

// what a product of the sampler is asked for besides its operands
enum : unsigned {
    PROD_STORE_MU = 1,   // forward: write the linear predictor MU too (see EpiForwardT)
    PROD_CHAIN = 2,      // the launch depends on the one before it (profiler: no marker in between)
    PROD_WANT_LL = 4,    // forward, sparse operator only: leave the per-chain partial sums of log f(y | MU) in h.cm_part_fwd instead of MU
    PROD_LX_READY = 8,   // forward, factored sparse operator only: LX = L X is already there, left by k_cm_Lcol_Lrow of the previous leapfrog step
};

// MU = xb + ZL * X ; S = score
static int hmc_forward(Ctx& c, const double* X, int ldx, double var_par, unsigned flags = PROD_STORE_MU)
{
    HmcState& h = c.hmc;
    const int store_mu = (flags & PROD_STORE_MU) ? 1 : 0;
    const int slot = c.prof.begin(c.stream, 0, (flags & PROD_CHAIN) != 0);
    int rc;
    if (h.cm) {
        c.last_kernel[0] = KERNEL_SPARSE;
        const int rpw = CM_FR;
        dim3 grid((c.n + 4 * rpw - 1) / (4 * rpw), (h.Cw + 63) / 64);
        // factored operator: LX = L X first, then the rows of Z gather from LX
        int W = c.sp.W; const int* col = c.sp.ell_col.as<int>(); const double* val = c.sp.ell_val.d(); const double* Xin = X;
        if (c.sp.factored) {
            if (!(flags & PROD_LX_READY))
            hipLaunchKernelGGL(k_cm_Lrow, dim3((c.Q + 3) / 4, (h.Cw + 63) / 64), dim3(256), 0, c.stream, c.Q, h.Cw, h.V.ld,
                               c.sp.row_start.as<int>(), c.L.d(), c.L.ld, X, h.LX.d());
            W = c.z_width; col = c.z_idx.as<int>(); val = c.z_val.d(); Xin = h.LX.d();
        }
        double* pll = nullptr;
        if (flags & PROD_WANT_LL) {
            MCML_TRY(h.cm_part_fwd.ensure(sizeof(double) * (size_t)grid.x * h.V.ld));
            pll = h.cm_part_fwd.d();
        }
        dispatch_flink<1, 3, 7, 12>(c.flink, [&](auto FL) {
            hipLaunchKernelGGL((k_cm_forward<FL()>), grid, dim3(256), 0, c.stream, c.n, h.Cw, h.V.ld, W, col, val, Xin, c.xb.d(),
                               c.y.d(), c.flink, var_par, store_mu, h.MU.d(), h.S.d(), rpw, pll, h.V.ld);
        });
        rc = (hipGetLastError() == hipSuccess) ? MCML_OK : MCML_EHIP;
    } else
        rc = dispatch_flink<1, 3, 7, 12>(c.flink, [&](auto FL) {
            return dense_product(c, 0, DenseOp{c.plan_fwd, c.band_fwd, c.n, c.Q, c.ZL}, X, ldx,
                                 EpiForwardT<FL()>{h.MU.d(), h.S.d(), h.MU.ld, c.xb.d(), c.y.d(), c.flink, store_mu, var_par});
        });
    c.prof.end(c.stream, slot);
    return rc;
}

// flags: PROD_CHAIN only
// next_lx (factored sparse operator, inside a trajectory; cm_fuse_width's 8 or 16, else 0): also leave LX = L * UP for the
// next step's forward product, by k_cm_Lcol_Lrow of that width
static int hmc_backward(Ctx& c, const double* Xs, double* G, int s, double var_par, int mode, unsigned flags = 0,
                        int next_lx = 0)
{
    HmcState& h = c.hmc;
    ChainArrays ca = chain_arrays(h);
    EpiBackward epi{Xs, G, h.R.d(), h.UP.d(), h.V.ld, ca.e, ca.steps, s, glm_score_post(var_par, c.flink), mode};
    const int slot = c.prof.begin(c.stream, 1, (flags & PROD_CHAIN) != 0);
    int rc;
    if (h.cm) {
        // factored operator: T = Z' S (mode 2: the raw sums), then g = -x + post * L' T with the leapfrog update
        const bool f = c.sp.factored;
        const int* ptr = f ? c.sp.zcsr_ptr.as<int>() : c.sp.csr_ptr.as<int>();
        const int* ci = f ? c.sp.zcsr_i.as<int>() : c.sp.csr_i.as<int>();
        const double* cv = f ? c.sp.zcsr_val.d() : c.sp.csr_val.d();
        double* out = f ? h.ZS.d() : G;
        const int m1 = f ? 2 : mode;
        const double post = glm_score_post(var_par, c.flink);
        if (cm_long_rows(c)) {                                   // long rows: a workgroup per (random effect, 64 chains)
            const int ncb = cm_chain_blocks(h.Cw);
            hipLaunchKernelGGL(k_cm_backward_long, dim3((c.Q * ncb + 7) / 8 * 8), dim3(256), 0, c.stream, c.Q, h.Cw, h.V.ld,
                               ptr, ci, cv, h.S.d(), Xs, out, h.R.d(), h.UP.d(), ca.e, ca.steps, s, post, m1, ncb);
        } else {
            const int rpw = 2;
            dim3 grid((c.Q + 4 * rpw - 1) / (4 * rpw), (h.Cw + 63) / 64);
            hipLaunchKernelGGL(k_cm_backward, grid, dim3(256), 0, c.stream, c.Q, h.Cw, h.V.ld, ptr, ci, cv, h.S.d(), Xs, out,
                               h.R.d(), h.UP.d(), ca.e, ca.steps, s, post, m1, rpw);
        }
        if (f && next_lx && mode == 1) {
            const dim3 grid((c.sp.nblk + 3) / 4, (h.Cw + 63) / 64);
            hipLaunchKernelGGL(next_lx == 8 ? k_cm_Lcol_Lrow<8> : k_cm_Lcol_Lrow<16>, grid, dim3(256), 0, c.stream, c.sp.nblk, h.Cw,
                               h.V.ld, c.sp.blk_ptr.as<int>(), c.L.d(), c.L.ld, h.ZS.d(), Xs, G, h.R.d(), h.UP.d(), ca.e, ca.steps, s,
                               post, h.LX.d());
        } else if (f)
            hipLaunchKernelGGL(k_cm_Lcol, dim3((c.Q + 3) / 4, (h.Cw + 63) / 64), dim3(256), 0, c.stream, c.Q, h.Cw, h.V.ld,
                               c.sp.row_end.as<int>(), c.L.d(), c.L.ld, h.ZS.d(), Xs, G, h.R.d(), h.UP.d(), ca.e, ca.steps, s,
                               post, mode);
        rc = (hipGetLastError() == hipSuccess) ? MCML_OK : MCML_EHIP;
        c.last_kernel[1] = KERNEL_SPARSE;
    } else
        rc = dense_product(c, 1, DenseOp{c.plan_bwd, c.band_bwd, c.Q, c.n, c.ZLT}, h.S.d(), h.S.ld, epi);
    c.prof.end(c.stream, slot);
    return rc;
}

// ---- chain-major helpers (sparse ZL operator, hmc_cm.h) ----
static int cm_fwd_chunks(const Ctx& c) { return (c.n + 4 * CM_FR - 1) / (4 * CM_FR); }     // workgroups of k_cm_forward = its ll partials
struct CmParts { double *ll, *lp, *kin, *ss; int nchn, nchq, ldp; };
static CmParts cm_parts(const Ctx& c)
{
    const HmcState& h = c.hmc;
    CmParts p;
    p.nchn = (c.n + CM_ROWS - 1) / CM_ROWS; p.nchq = (c.Q + cm_qrows(c.Q) - 1) / cm_qrows(c.Q); p.ldp = h.V.ld;
    p.ll = h.cm_part.d(); p.lp = p.ll + (size_t)p.nchn * p.ldp; p.kin = p.lp + (size_t)p.nchq * p.ldp;
    p.ss = p.kin + (size_t)p.nchq * p.ldp;
    return p;
}
// partial sums of log f(y | MU) + log N(X; 0, 1) (+ R^2) of every chain
// skip_ll: the observation part came out of the last forward product (PROD_WANT_LL); only the prior / kinetic part runs
static int cm_logprob_partials(Ctx& c, const double* X, const double* R, double var_par, bool skip_ll = false)
{
    HmcState& h = c.hmc;
    const CmParts p = cm_parts(c);
    const int nchn = skip_ll ? 0 : p.nchn;
    const dim3 grid((h.Cw + 63) / 64, nchn + p.nchq);
    dispatch_flink<1, 3, 7>(c.flink, [&](auto FL) {
        hipLaunchKernelGGL((k_cm_logprob_partials<FL()>), grid, dim3(256), 0, c.stream, h.MU.d(), X, R, h.V.ld, c.n, c.Q, h.Cw,
                           c.y.d(), var_par, c.flink, nchn, p.ll, p.lp, p.kin, p.ldp);
    });
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

// column-major state: lp[c] = log_prob of column c of X with the linear predictor in h.MU, for the first ncols columns
static void hmc_lp0_launch(Ctx& c, const DevMat& X, int ncols, double var_par, double* lp)
{
    const HmcState& h = c.hmc;
    dispatch_flink<1, 3, 7>(c.flink, [&](auto FL) {
        hipLaunchKernelGGL((k_hmc_lp0<FL()>), dim3(ncols), dim3(256), 0, c.stream, h.MU.d(), h.MU.ld, c.n, X.d(), X.ld, c.Q,
                           c.y.d(), var_par, c.flink, lp);
    });
}

// log_prob and log_grad of every column of the current V
static int hmc_eval_state(Ctx& c, double var_par)
{
    HmcState& h = c.hmc;
    ChainArrays ca = chain_arrays(h);
    // sparse operator: the observation part of the log density comes out of the forward product (MU is not stored)
    MCML_TRY(hmc_forward(c, h.V.d(), h.V.ld, var_par, h.cm ? PROD_WANT_LL : PROD_STORE_MU));
    if (h.cm) {
        const CmParts p = cm_parts(c);
        MCML_TRY(cm_logprob_partials(c, h.V.d(), nullptr, var_par, true));
        hipLaunchKernelGGL(k_cm_lp0_fin, dim3((h.C + 63) / 64), dim3(256), 0, c.stream, h.cm_part_fwd.d(), p.lp,
                           cm_fwd_chunks(c), p.nchq, p.ldp, h.C, ca.lpcur);
    } else
        hmc_lp0_launch(c, h.V, h.C, var_par, ca.lpcur);
    MCML_HIP(hipGetLastError());
    return hmc_backward(c, h.V.d(), h.GRAD.d(), 0, var_par, 0);
}

// ---- pieces the two samplers (hmc_sample here, nuts_sample in nuts.h) share ----
// initialise_u (mhmcmc.h:47-59): the state V (init, Q x C column-major on the device, or fresh normal draws) and the per-chain arrays
static int sampler_init_state(Ctx& c, uint64_t seed, uint32_t chain_offset, uint32_t iter_idx, const double* init)
{
    HmcState& h = c.hmc;
    const ChainArrays ca = chain_arrays(h);
    if (h.cm)
        hipLaunchKernelGGL(k_cm_init, dim3((h.C + 63) / 64, cm_parts(c).nchq), dim3(256), 0, c.stream, h.V.d(), h.V.ld, c.Q, h.C,
                           ca, seed, chain_offset, iter_idx, init);
    else
        hipLaunchKernelGGL(k_hmc_init, dim3(h.C), dim3(256), 0, c.stream, h.V.d(), h.V.ld, c.Q, ca, seed, chain_offset, iter_idx,
                           init);
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

// the current state of every chain c becomes sample column c * stride + col
static void store_columns(Ctx& c, const DevMat& samp, int stride, int col)
{
    const HmcState& h = c.hmc;
    if (h.cm)      // SAMP[k + (c * stride + col) * lds] = V[c + k * ldc]
        hipLaunchKernelGGL(k_cm_transpose, dim3((c.Q + 31) / 32, (h.C + 31) / 32), dim3(256), 0, c.stream, h.V.d(), h.V.ld, c.Q,
                           h.C, samp.d(), (size_t)samp.ld, (size_t)(stride > 0 ? stride : 1), col);
    else
        hipLaunchKernelGGL(k_hmc_store, dim3(h.C), dim3(256), 0, c.stream, h.V.d(), h.V.ld, c.Q, samp.d(), samp.ld, stride, col);
}

// c.U = L * samples  (mhmcmc.h:155; gen_u_samples.R:66); the caller sets c.niter
static int samples_to_U(Ctx& c, const DevMat& samp, int ncols)
{
    const int Q = c.Q;
    MCML_TRY(c.U.alloc(Q, ncols));
    MCML_HIP(hipMemsetAsync(c.U.d(), 0, sizeof(double) * (size_t)c.U.ld * ncols, c.stream));
    if (c.sp.active && c.sp.row_start.p) {
        int gy = ncols < 1024 ? ncols : 1024;
        hipLaunchKernelGGL(k_blockdiag_LV, dim3((Q + 255) / 256, gy), dim3(256), 0, c.stream, Q, ncols,
                           c.sp.row_start.as<int>(), c.L.d(), c.L.ld, samp.d(), samp.ld, c.U.d(), c.U.ld);
        MCML_HIP(hipGetLastError());
    } else {
        EpiAxpby epi{c.U.d(), c.U.ld, 1.0, 0.0};
        MCML_TRY(launch_gemm<false>(c.stream, Q, ncols, Q, c.L.d(), c.L.ld, samp.d(), samp.ld, epi));
    }
    c.mcols = ncols;
    c.zu_valid = false; c.uall_valid = false;
    return MCML_OK;
}

}  // namespace mcml

#include "hmc_exact.h"      // exact conditional draws (gaussian / identity): ends in samples_to_U like the samplers here
#include "hmc_exact_comp.h" // the same, component by component on the sparse operator

namespace mcml {

// the exact path from outside this file (entry.h; cabi.hip: the direct entry point, ctx_hooks.hip: the plan hook)
bool hmc_exact_applicable(const Ctx& c) { return exact_applicable(c); }
int hmc_exact_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed, uint32_t iter_idx,
                     const double* inj_z, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    return exact_gaussian_sample(c, beta, var_par, o, seed, iter_idx, inj_z, nullptr, nullptr, diag, ncols_out);
}

bool hmc_exact_component_applicable(const Ctx& c) { return exact_component_applicable(c); }
int hmc_exact_component_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed,
                               uint32_t iter_idx, const double* inj_z, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    return exact_component_sample(c, beta, var_par, o, seed, iter_idx, inj_z, nullptr, nullptr, diag, ncols_out);
}
// glmmr_mcml_dbg_exact_component_plan: waves of the factor kernel, LDS bytes of the draw kernel, bytes of the factor scratch
void hmc_exact_component_sizes(const Ctx& c, long long* out3)
{
    const ComponentPlan& p = c.cp.plan;
    const int waves = cp_waves(p, cp_forced_waves(CP_LA_WAVES_ENV));
    out3[0] = waves; out3[1] = exc_lds_bytes(p.max_vars); out3[2] = 8LL * comp_factor_doubles(c);
}

// ---- hmc_sample in parts ----
// GLMMR_MCML_HMC_TIMING=1: host wall-clock of a call's segments on stderr (set-up | proposals | tail), and of the slowest
// proposal's enqueue -- to tell a slow call's cause from outside (run-to-run jitter)
struct HmcTiming {
    using Clock = std::chrono::steady_clock;
    enum { PROPOSE, LOOK_AHEAD, TRAJECTORY, ACCEPT, NSEG };     // the segments of a proposal's enqueue
    const bool on = enabled();
    Clock::time_point t_phase = Clock::now(), t_mark = t_phase, t_prop = t_phase;
    double setup = 0, loop = 0, sync = 0, slowest = 0, seg[NSEG] = {};   // seg: the slowest enqueue of each segment
    int n_sync = 0, nprop = 0;

    static bool enabled() { static const bool v = getenv("GLMMR_MCML_HMC_TIMING") != nullptr; return v; }
    static double since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }
    static double now_ms() { return std::chrono::duration<double, std::milli>(Clock::now().time_since_epoch()).count(); }
    double phase_end() { const double d = since(t_phase); t_phase = Clock::now(); return d; }   // set-up -> loop -> tail
    void proposal()                                 // a proposal's enqueue begins (and the one before it has ended)
    {
        if (!on) return;
        if (nprop++ > 0) slowest = std::max(slowest, since(t_prop));
        t_prop = t_mark = Clock::now();
    }
    void start() { if (on) t_mark = Clock::now(); }                                // a segment begins ...
    void mark(int k) { if (on) { seg[k] = std::max(seg[k], since(t_mark)); t_mark = Clock::now(); } }   // ... ends, the next begins
    void waited() { if (on) { sync += since(t_mark); ++n_sync; } }                 // ... was a stream synchronisation
    void print(int total) const
    {
        if (on)
            fprintf(stderr, "hmc_sample: set-up %.2f ms | %d proposals %.2f ms enqueue (%d synchronous, %.2f ms waiting; slowest proposal %.2f ms: propose %.2f, count look-ahead %.2f, trajectory %.2f, accept %.2f) | tail %.2f ms\n",
                    setup, total, loop, n_sync, sync, slowest, seg[PROPOSE], seg[LOOK_AHEAD], seg[TRAJECTORY], seg[ACCEPT], since(t_phase));
    }
};

// what the proposals of one hmc_sample call share; constant over the call but for pending_commit
struct HmcCall {
    const glmmr_mcml_hmc_opts* o; double var_par; uint64_t seed; uint32_t iter_idx;
    SampleShape sh;                       // chains, draws per chain, proposals, columns
    ChainArrays ca;
    const double* mom; uint8_t* flags; double* probs;   // device, or null: injected momenta; accept flags / probabilities out
    const DevMat* samp;                   // the draws
    int lf;                               // factored operator: the backward pass of step s leaves LX for step s + 1 (cm_fuse_width)
    double* tpart; size_t tstride;        // component trajectories: K0 | ll | lp | kin partial sums, tstride doubles each
    StepRing* ring; int* d_maxs;          // the step-count read-back
    bool pending_commit;                  // sparse operator: the last decisions are applied by the next proposal's first kernel
    int adapt(int it) const { return (it < o->warmup) && (it < o->adapt); }     // mhmcmc.h:131-136
};

// sparse operator: the accepted chains' V <- UP, GRAD <- GRADP: folded into the next proposal's first pass unless V is read
// before that (a draw is stored after this proposal, or it is the last one)
static void commit_cm(Ctx& c, HmcCall& k, int it)
{
    HmcState& h = c.hmc;
    int stride;
    const bool stores_now = k.sh.column_of(it, &stride) >= 0;
    if (it + 1 < k.sh.total && !stores_now) k.pending_commit = true;
    else hipLaunchKernelGGL(k_cm_commit, dim3((k.sh.C + 63) / 64, cm_parts(c).nchq), dim3(256), 0, c.stream, h.V.d(), h.GRAD.d(),
                            h.UP.d(), h.GRADP.d(), h.V.ld, c.Q, k.sh.C, h.cm_acc.as<int>());
}

static void store_draw(Ctx& c, const HmcCall& k, int it)
{
    int stride;
    const int col = k.sh.column_of(it, &stride);
    if (col >= 0) store_columns(c, *k.samp, stride, col);
}

// The proposal's first kernels are on the stream: the leapfrog steps of every chain.  As many iterations are launched as the
// read-ahead answers -- the cap while it speculates, else the largest step count over the chains, waited for; the chains'
// own counts mask the rest
static int leapfrog_steps(Ctx& c, const HmcCall& k, StepAhead& ahead, HmcTiming& t, int it)
{
    HmcState& h = c.hmc;
    StepRing& ring = *k.ring;
    const unsigned seq = ++ring.seq;
    const int slot = (int)(seq % StepRing::SLOTS);
    hipLaunchKernelGGL(k_max_steps, dim3(1), dim3(256), 0, c.stream, k.ca.steps, k.sh.C, k.d_maxs, ring.d + slot, seq);
    MCML_HIP(hipGetLastError());
    t.mark(HmcTiming::PROPOSE);
    int maxs = ahead.launched(seq, HmcTiming::now_ms);
    if (maxs != StepAhead::SYNCHRONISE) t.mark(HmcTiming::LOOK_AHEAD);
    else {
        t.start();
        MCML_HIP(hipStreamSynchronize(c.stream));
        t.waited();
        maxs = ahead.synchronised(seq);
        MCML_REQUIRE(maxs != StepAhead::NOT_ARRIVED, "hmc: the step count of proposal %d did not arrive (token %llx, expected sequence %u)", it, ring.h[slot], seq);
        MCML_REQUIRE(maxs != StepAhead::OUT_OF_ORDER, "hmc: step-count ring out of order");
    }
    MCML_REQUIRE(maxs >= 1 && maxs <= k.o->max_steps, "hmc: step count %d out of range", maxs);
    // kernel timing (bench.py's roofline): every marker between two dependent launches costs ~2.5 us of idle GPU,
    // so one proposal in four is timed -- still hundreds of launches per MCML iteration behind the average
    c.prof.skip = (it & 3) != 0;
    t.start();
    int rc = MCML_OK;
    for (int s = 0; s < maxs && rc == MCML_OK; ++s) {
        const bool last = s == maxs - 1;
        rc = hmc_forward(c, h.UP.d(), h.UP.ld, k.var_par, (s > 0 ? PROD_CHAIN : 0) | (last ? (h.cm ? PROD_WANT_LL : PROD_STORE_MU) : 0) |
                                                              (k.lf && s > 0 ? PROD_LX_READY : 0));
        if (rc == MCML_OK) rc = hmc_backward(c, h.UP.d(), h.GRADP.d(), s, k.var_par, 1, PROD_CHAIN, last ? 0 : k.lf);
    }
    c.prof.skip = false;
    t.mark(HmcTiming::TRAJECTORY);
    MCML_TRY(rc);
    c.prof.unchain();
    return MCML_OK;
}

// One proposal of every chain (new_proposal, mhmcmc.h:62-117), per back end.  dense ZL, column-major state:
static int propose_dense(Ctx& c, HmcCall& k, StepAhead& ahead, HmcTiming& t, int it)
{
    HmcState& h = c.hmc;
    const glmmr_mcml_hmc_opts* o = k.o;
    hipLaunchKernelGGL(k_hmc_propose, dim3(k.sh.C), dim3(256), 0, c.stream, h.V.d(), h.GRAD.d(), h.R.d(), h.UP.d(),
                       h.V.ld, c.Q, k.ca, o->lambda, o->max_steps, k.seed, (uint32_t)o->chain_offset, k.iter_idx, it,
                       k.mom, k.sh.C);
    MCML_TRY(leapfrog_steps(c, k, ahead, t, it));
    dispatch_flink<1, 3, 7>(c.flink, [&](auto FL) {
        hipLaunchKernelGGL((k_hmc_accept<FL()>), dim3(k.sh.C), dim3(256), 0, c.stream, h.V.d(), h.GRAD.d(), h.R.d(), h.UP.d(),
                           h.GRADP.d(), h.V.ld, c.Q, h.MU.d(), h.MU.ld, c.n, c.y.d(), k.var_par, c.flink, k.ca,
                           o->target_accept, k.adapt(it), it, k.sh.C, k.flags, k.probs);
    });
    store_draw(c, k, it);
    MCML_HIP(hipGetLastError());
    t.mark(HmcTiming::ACCEPT);
    return MCML_OK;
}

// sparse ZL operator, chain-major state (hmc_cm.h), a launch pair per leapfrog step:
static int propose_cm(Ctx& c, HmcCall& k, StepAhead& ahead, HmcTiming& t, int it)
{
    HmcState& h = c.hmc;
    const glmmr_mcml_hmc_opts* o = k.o;
    const CmParts p = cm_parts(c);
    const dim3 chains((k.sh.C + 63) / 64);
    hipLaunchKernelGGL(k_cm_propose, dim3(chains.x, p.nchq), dim3(256), 0, c.stream, h.V.d(), h.GRAD.d(), h.R.d(),
                       h.UP.d(), h.V.ld, c.Q, k.sh.C, k.ca, k.seed, (uint32_t)o->chain_offset, k.iter_idx, it, k.mom,
                       p.ss, p.ldp, k.pending_commit ? h.cm_acc.as<int>() : nullptr, h.GRADP.d());
    k.pending_commit = false;
    hipLaunchKernelGGL(k_cm_propose_fin, chains, dim3(256), 0, c.stream, p.ss, p.nchq, p.ldp, k.sh.C, k.ca, o->lambda, o->max_steps);
    MCML_TRY(leapfrog_steps(c, k, ahead, t, it));
    MCML_TRY(cm_logprob_partials(c, h.UP.d(), h.R.d(), k.var_par, true));
    hipLaunchKernelGGL((k_cm_accept_fin<false>), chains, dim3(256), 0, c.stream, h.cm_part_fwd.d(), p.lp, p.kin,
                       cm_fwd_chunks(c), p.nchq, p.ldp, k.sh.C, k.ca, o->target_accept, k.adapt(it), it, k.flags, k.probs,
                       h.cm_acc.as<int>(), (const double*)nullptr, 0, 0.0, 0);
    commit_cm(c, k, it);
    store_draw(c, k, it);
    MCML_HIP(hipGetLastError());
    t.mark(HmcTiming::ACCEPT);
    return MCML_OK;
}

// component-local trajectories (hmc_traj.h): one launch instead of the loop over the steps, no step count to read
static int propose_component(Ctx& c, HmcCall& k, int it)
{
    HmcState& h = c.hmc;
    const glmmr_mcml_hmc_opts* o = k.o;
    double* const tpart = k.tpart; const size_t tstride = k.tstride;
    TrajArgs a{h.V.d(), h.GRAD.d(), h.UP.d(), h.GRADP.d(), h.V.ld, k.sh.C, c.Q, k.ca, k.seed, (uint32_t)o->chain_offset,
               k.iter_idx, it, k.mom, k.pending_commit ? h.cm_acc.as<int>() : nullptr, o->lambda, o->max_steps, c.flink,
               k.var_par, glm_score_post(k.var_par, c.flink), tpart, tpart + tstride, tpart + 2 * tstride,
               tpart + 3 * tstride, h.V.ld};
    k.pending_commit = false;
    c.prof.skip = (it & 3) != 0;
    const int slot = c.prof.begin(c.stream, 0);     // counted (and timed) under the forward product's slot
    const int rc = cm_traj_launch(c, a);
    c.prof.end(c.stream, slot);
    c.prof.skip = false;
    c.prof.unchain();
    MCML_TRY(rc);
    const int ni = c.cp.plan.nitems();
    hipLaunchKernelGGL((k_cm_accept_fin<true>), dim3((k.sh.C + 63) / 64), dim3(256), 0, c.stream, tpart + tstride, tpart + 2 * tstride,
                       tpart + 3 * tstride, ni, ni, h.V.ld, k.sh.C, k.ca, o->target_accept, k.adapt(it), it, k.flags, k.probs,
                       h.cm_acc.as<int>(), tpart, ni, o->lambda, o->max_steps);
    commit_cm(c, k, it);
    store_draw(c, k, it);
    MCML_HIP(hipGetLastError());
    c.last_kernel[0] = c.last_kernel[1] = KERNEL_COMPONENT;
    return MCML_OK;
}

int hmc_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed,
               uint32_t iter_idx, const double* inj_init, const double* inj_mom, uint8_t* flags_out,
               double* probs_out, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    MCML_REQUIRE(c.n > 0 && c.have_L && (c.ZL.d() || c.sp.active), "hmc: model / L not set (call update_L or set_L first)");
    MCML_REQUIRE(o && o->warmup >= 0 && o->nsamp > 0 && o->max_steps >= 1 && o->lambda > 0,
                 "hmc: bad options");
    MCML_REQUIRE(beta, "hmc: beta is null");
    // exact conditional draws: asked for (Ctx::draws_mode) and the target is the Gaussian hmc_exact.h draws from; anywhere else the
    // request changes nothing
    if ((c.draws_mode == 1 || c.draws_mode == 2) && exact_applicable(c))
        return exact_gaussian_sample(c, beta, var_par, o, seed, iter_idx, nullptr, flags_out, probs_out, diag, ncols_out);
    if (c.draws_mode == 2 && exact_component_applicable(c))      // the same target where M is block diagonal (hmc_exact_comp.h)
        return exact_component_sample(c, beta, var_par, o, seed, iter_idx, nullptr, flags_out, probs_out, diag, ncols_out);
    const SampleShape sh = sample_shape(o->nsamp, o->warmup, o->chains);
    const int C = sh.C, total = sh.total, ncols = sh.ncols;
    const int Q = c.Q;
    HmcState& h = c.hmc;
    HmcTiming t;
    MCML_TRY(model_update_beta(c, beta));
    MCML_TRY(hmc_alloc(c, C));
    DevMat samp;
    MCML_TRY(samp.alloc(Q, ncols));
    MCML_HIP(hipMemsetAsync(samp.d(), 0, sizeof(double) * (size_t)samp.ld * ncols, c.stream));

    DevBuf d_init, d_mom, d_flags, d_probs;
    if (inj_init) {
        MCML_TRY(d_init.ensure(sizeof(double) * (size_t)Q * C));
        MCML_TRY(copy_h2d(d_init.p, inj_init, sizeof(double) * (size_t)Q * C, c.stream));
    }
    if (inj_mom) {
        MCML_TRY(d_mom.ensure(sizeof(double) * (size_t)Q * C * total));
        MCML_TRY(copy_h2d(d_mom.p, inj_mom, sizeof(double) * (size_t)Q * C * total, c.stream));
    }
    if (flags_out) MCML_TRY(d_flags.ensure((size_t)C * total));
    if (probs_out) MCML_TRY(d_probs.ensure(sizeof(double) * (size_t)C * total));

    // the step-count read-back: step_ahead.h.  GLMMR_MCML_HMC_SPEC=0 disables the speculation
    static const bool spec_allowed = !(getenv("GLMMR_MCML_HMC_SPEC") && atoi(getenv("GLMMR_MCML_HMC_SPEC")) == 0);
    StepRing& ring = h.ring;
    if (!ring.h) {
        MCML_HIP(hipHostMalloc((void**)&ring.h, sizeof(unsigned long long) * StepRing::SLOTS, hipHostMallocMapped | hipHostMallocCoherent));
        memset(ring.h, 0, sizeof(unsigned long long) * StepRing::SLOTS);
        MCML_HIP(hipHostGetDevicePointer((void**)&ring.d, ring.h, 0));
    }
    StepAhead ahead(ring.h, ring.seq, o->max_steps, spec_allowed);

    // component-local trajectories: one launch per proposal instead of the loop over the steps
    const bool traj = h.cm && cm_traj_used(c);
    HmcCall k{o, var_par, seed, iter_idx, sh, chain_arrays(h), d_mom.d(), d_flags.as<uint8_t>(), d_probs.d(), &samp,
              h.cm ? cm_fuse_width(c) : 0, traj ? h.cp_part.d() : nullptr, traj ? (size_t)c.cp.plan.nitems() * h.V.ld : 0,
              &ring, c.scalars.as<int>() + 34, false};

    MCML_TRY(sampler_init_state(c, seed, (uint32_t)o->chain_offset, iter_idx, d_init.d()));
    MCML_TRY(hmc_eval_state(c, var_par));
    if (sh.single_chain_layout && o->warmup == 0) store_columns(c, samp, 0, 0);   // no warm-up: column 0 is the start value
    if (traj) MCML_TRY(comp_fill_xy(c));        // xb follows beta: the records' copy of it
    t.setup = t.phase_end();
    for (int it = 0; it < total; ++it) {
        t.proposal();
        if (traj) MCML_TRY(propose_component(c, k, it));
        else if (h.cm) MCML_TRY(propose_cm(c, k, ahead, t, it));
        else MCML_TRY(propose_dense(c, k, ahead, t, it));
    }
    t.loop = t.phase_end();
    MCML_TRY(samples_to_U(c, samp, ncols));     // return (L * samples)  (mhmcmc.h:155)
    c.niter = sh.niter;
    if (flags_out) MCML_TRY(copy_d2h(flags_out, d_flags.p, (size_t)C * total, c.stream));
    if (probs_out) MCML_TRY(copy_d2h(probs_out, d_probs.p, sizeof(double) * (size_t)C * total, c.stream));
    double dg[6] = {0, 0, 0, 0, 0, 0};
    hipLaunchKernelGGL(k_hmc_diag, dim3(1), dim3(64), 0, c.stream, k.ca, C, c.scalars.d() + 8);
    MCML_TRY(copy_d2h(dg, c.scalars.d() + 8, sizeof dg, c.stream));
    MCML_HIP(hipStreamSynchronize(c.stream));
    t.print(total);
    c.prof.collect();
    if (diag) {
        diag->accept_rate = dg[0] / ((double)C * total);
        diag->mean_e = dg[1] / C; diag->min_e = dg[2]; diag->max_e = dg[3];
        diag->max_steps_used = (int)dg[4]; diag->leapfrog_total = (long long)dg[5];
    }
    if (ncols_out) *ncols_out = ncols;
    return MCML_OK;
}

// test hook: log_prob (A4) and log_grad (A5) of every column of V
int hmc_dbg_log_prob_grad(Ctx& c, const double* beta, double var_par, const double* V, int ncols, double* lp,
                          double* G)
{
    MCML_REQUIRE(c.n > 0 && c.have_L && (c.ZL.d() || c.sp.active), "log_prob_grad: model / L not set");
    MCML_TRY(model_update_beta(c, beta));
    MCML_TRY(hmc_alloc(c, ncols));
    HmcState& h = c.hmc;
    ChainArrays ca = chain_arrays(h);
    if (h.cm) {
        DevMat tmp;                                   // Q x ncols column-major staging
        MCML_TRY(tmp.alloc(c.Q, ncols));
        MCML_TRY(copy_h2d_2d(tmp.d(), sizeof(double) * tmp.ld, V, sizeof(double) * c.Q, sizeof(double) * c.Q, ncols, c.stream));
        // V[c + q * ldc] = tmp[q + c * ld]
        hipLaunchKernelGGL(k_cm_transpose, dim3((ncols + 31) / 32, (c.Q + 31) / 32), dim3(256), 0, c.stream, tmp.d(), tmp.ld,
                           ncols, c.Q, h.V.d(), (size_t)h.V.ld, (size_t)1, 0);
        MCML_HIP(hipGetLastError());
        MCML_TRY(hmc_eval_state(c, var_par));
        hipLaunchKernelGGL(k_cm_transpose, dim3((c.Q + 31) / 32, (ncols + 31) / 32), dim3(256), 0, c.stream, h.GRAD.d(), h.GRAD.ld,
                           c.Q, ncols, tmp.d(), (size_t)tmp.ld, (size_t)1, 0);
        MCML_HIP(hipGetLastError());
        MCML_TRY(copy_d2h(lp, ca.lpcur, sizeof(double) * ncols, c.stream));
        MCML_TRY(download_matrix(G, c.Q, tmp.d(), tmp.ld, c.Q, ncols, c.stream));
        return c.sync();                              // tmp goes out of scope
    }
    MCML_TRY(copy_h2d_2d(h.V.d(), sizeof(double) * h.V.ld, V, sizeof(double) * c.Q, sizeof(double) * c.Q, ncols, c.stream));
    MCML_TRY(hmc_eval_state(c, var_par));
    MCML_TRY(copy_d2h(lp, ca.lpcur, sizeof(double) * ncols, c.stream));
    return download_matrix(G, c.Q, h.GRAD.d(), h.GRAD.ld, c.Q, ncols, c.stream);
}

}  // namespace mcml

#include "nuts.h"
