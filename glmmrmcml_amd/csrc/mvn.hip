// mvn.hip -- multivariate-normal log-likelihood of the random effects,
//   (1/m) sum_b sum_j log N(u_{b,j}; 0, D_b(theta)),
// i.e. MCMLDmatrix::loglik / logdet / loglik_block (mcmldmatrix.h:23-78), the
// D_likelihood functor (likelihood.h:31-46) and export mvn_ll
// (mcml_optim.cpp:406-414), plus DMatrix::genD(0,chol,false) (mcml_full.cpp:68).
//
// The reference rebuilds and refactorises each block once per sample column
// (defect D2); here every block is built and factorised once per theta:
//   * all-gr blocks (diagonal, mcmldmatrix.h:61-65): closed form, one streaming pass
//     over u (HBM-bound: 8 B per element);
//   * blocks of dim <= 32: one wave builds + factorises the block in LDS and
//     forward-substitutes 64 sample columns at a time;
//   * larger blocks: fused covariance build -> right-looking blocked Cholesky (chol.hip) whose
//     panel and trailing updates are FP64-MFMA GEMMs (dgemm_dl.h), 128-wide leaves
//     factorised and inverted in LDS; the m sample columns ride below the matrix
//     as extra rows, so the same GEMMs forward-substitute them -> Frobenius norm
//     + log-det.
// Reductions are two-stage with a fixed order, so the result is run-to-run
// bit-reproducible.  The analytic score of the same objective (beyond the reference's
// exports) lives in mvn_grad.h, one gradient path per block kind.
#include <cmath>
#include "ctx.h"
#include "cov_block.h"
#include "mvn_grad.h"
#include "reduce.h"
#include "theta_scale.h"
#include "vecops.h"

namespace mcml {

// ------------------------------------------------------------------ diagonal blocks
// the variance of a row and its constant: k_diag_prep (mvn_grad.h, whose diagonal rows read them too)
__global__ __launch_bounds__(256) void k_diag_ll(const double* U, int ldu, int Q, int mcols,
                                                 const int* rowblock, const double* dd,
                                                 const double* dc, double* partials)
{
    __shared__ double sh[4];
    int k = blockIdx.x * 256 + threadIdx.x;
    double acc = 0;
    if (k < Q && rowblock[k] >= 0) {
        const double idd = dd[k], c0 = dc[k];
        for (int col = blockIdx.y; col < mcols; col += gridDim.y) {
            double u = U[k + (size_t)col * ldu];
            acc += c0 - 0.5 * u * u / idd;
        }
    }
    double r = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = r;
}

// ------------------------------------------------------------------ small blocks
__global__ __launch_bounds__(64) void k_small_ll(const double* U, int ldu, int mcols,
                                                 const int* small_ids, const CovBlock* blocks,
                                                 const int32_t* cov, int rows, const double* data,
                                                 ThetaArg th, double* partials, int* errflag)
{
    constexpr int LS = SMALL_LS;
    __shared__ double S[SMALL_BLOCK * LS];
    __shared__ double Zs[SMALL_BLOCK * 64];
    const CovBlock blk = blocks[small_ids[blockIdx.x]];
    const int dim = blk.dim, lane = threadIdx.x;
    small_block_factor(S, blk, cov, rows, data + blk.doff, th, errflag);
    double logdet = 0;
    for (int i = 0; i < dim; ++i) logdet += 2 * log(S[i * LS + i]);
    double acc = 0;
    for (int col = blockIdx.y * 64 + lane; col < mcols; col += gridDim.y * 64) {
        const double* u = U + blk.matstart + (size_t)col * ldu;
        const double quad = small_block_forward(S, dim, Zs, lane, [&](int i) { return u[i]; });
        acc += (-0.5 * dim * LOG_2PI - 0.5 * logdet - 0.5 * quad);
    }
    acc = wave_sum(acc);
    if (lane == 0) partials[blockIdx.x * gridDim.y + blockIdx.y] = acc;
}

// ------------------------------------------------------------------ large blocks
// lower triangle (mirrored) of one block's covariance matrix
// (dpad > dim: rows / columns dim .. dpad are an identity border, so that an odd block can be factorised as an
// even one -- every panel pointer stays 16-byte aligned; the border does not change L, the log-determinant or
// the solves)
__device__ __forceinline__ void build_dense_body(double* A, int lda, int bidx, const CovBlock* blocks, const int32_t* cov,
                                                 int rows, const double* data, const ThetaArg& th, int mirror, int dpad)
{
    const CovBlock blk = blocks[bidx];
    lower_tile_walk([&](int i, int j) {
        if (i >= blk.dim && i < dpad && j <= i) { A[i + (size_t)j * lda] = (i == j) ? 1.0 : 0.0; return; }
        if (i >= blk.dim || j >= blk.dim || i < j) return;
        const double v = cov_entry(blk, cov, rows, data + blk.doff, th, i, j);
        A[i + (size_t)j * lda] = v;
        if (mirror && i != j) A[j + (size_t)i * lda] = v;
    });
}

// the candidate thetas of one round (mvn_loglik_batch): blockIdx.z picks the candidate and its matrix
constexpr int MVN_MAXBATCH = 8;
struct ThetaBatch { ThetaArg t[MVN_MAXBATCH]; };

__global__ __launch_bounds__(256) void k_build_dense_batch(double* A, int lda, size_t bsA, int bidx, const CovBlock* blocks,
                                                           const int32_t* cov, int rows, const double* data,
                                                           ThetaBatch tb, int dpad)
{
    build_dense_body(A + (size_t)blockIdx.z * bsA, lda, bidx, blocks, cov, rows, data, tb.t[blockIdx.z], 0, dpad);
}

__global__ __launch_bounds__(256) void k_build_dense(double* A, int lda, int bidx, const CovBlock* blocks,
                                                     const int32_t* cov, int rows, const double* data,
                                                     ThetaArg th, int mirror, int dpad)
{
    build_dense_body(A, lda, bidx, blocks, cov, rows, data, th, mirror, dpad);
}

__global__ void k_copy_block(double* dst, int ldd, const double* src, int lds, int rows, int cols)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    for (int j = blockIdx.y; j < cols; j += gridDim.y) dst[i + (size_t)j * ldd] = src[i + (size_t)j * lds];
}

// scal[0] += mcols*(-0.5 dim log 2pi - 0.5 logdet) - 0.5 sumsq   (mcmldmatrix.h:75)
__global__ void k_finish_large(double* scal, int dim, int mcols)
{
    scal[0] += (double)mcols * (-0.5 * dim * LOG_2PI - 0.5 * scal[1]) - 0.5 * scal[2];
}

// the two terms of the block at hand, added up per candidate for the host (mvn_loglik_batch_parts): thread j = candidate j
__global__ void k_accum_parts(const double* scal, int sstride, double* parts)
{
    const double* sj = scal + (size_t)threadIdx.x * sstride;
    parts[2 * threadIdx.x] += sj[1];
    parts[2 * threadIdx.x + 1] += sj[2];
}

__global__ void k_zero_upper(double* A, int lda, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int j = blockIdx.y;
    if (i < n && j < n && i < j) A[i + (size_t)j * lda] = 0.0;
}

// ------------------------------------------------------------------ setup
int mvn_setup(Ctx& c)
{
    const CovSpec& cs = c.cov;
    c.theta_scale_p = theta_scale_exponents(cs);
    MCML_TRY(c.d_cov.ensure(sizeof(int32_t) * cs.cov.size()));
    MCML_TRY(copy_h2d(c.d_cov.p, cs.cov.data(), sizeof(int32_t) * cs.cov.size(), c.stream));
    MCML_TRY(c.d_data.ensure(sizeof(double) * (cs.data.size() + 1)));
    if (!cs.data.empty())
        MCML_TRY(copy_h2d(c.d_data.p, cs.data.data(), sizeof(double) * cs.data.size(), c.stream));
    MCML_TRY(c.d_blocks.ensure(sizeof(CovBlock) * cs.blocks.size()));
    MCML_TRY(copy_h2d(c.d_blocks.p, cs.blocks.data(), sizeof(CovBlock) * cs.blocks.size(), c.stream));
    std::vector<int> rowblock(cs.N, -1), small;
    c.maxdim_large = 0; c.n_small = 0; c.n_diag_rows = 0;
    for (int b = 0; b < cs.B; ++b) {
        const CovBlock& blk = cs.blocks[b];
        if (blk.all_gr) {
            for (int k = 0; k < blk.dim; ++k) rowblock[blk.matstart + k] = b;
            c.n_diag_rows += blk.dim;
        } else if (blk.dim <= SMALL_BLOCK) {
            ++c.n_small;
            small.push_back(b);
        } else if (blk.dim > c.maxdim_large) {
            c.maxdim_large = blk.dim;
        }
    }
    MCML_TRY(c.d_rowblock.ensure(sizeof(int) * (size_t)(cs.N + 1)));
    MCML_TRY(copy_h2d(c.d_rowblock.p, rowblock.data(), sizeof(int) * cs.N, c.stream));
    MCML_TRY(c.scalars.ensure(sizeof(double) * 64));
    MCML_HIP(hipMemsetAsync(c.scalars.p, 0, sizeof(double) * 64, c.stream));
    if (c.n_small) {
        MCML_TRY(c.small_ids.ensure(sizeof(int) * small.size()));
        MCML_TRY(copy_h2d(c.small_ids.p, small.data(), sizeof(int) * small.size(), c.stream));
    }
    if (c.maxdim_large) {
        MCML_TRY(c.Dwork.alloc(c.maxdim_large, c.maxdim_large));
        MCML_HIP(hipMemsetAsync(c.Dwork.d(), 0, sizeof(double) * (size_t)c.Dwork.ld * c.maxdim_large, c.stream));
        // room for a whole round of candidates (mvn_loglik_batch) from the start: growing the buffer later would change
        // the pointer the single evaluation's captured graph is keyed on
        MCML_TRY(c.chol.linv.ensure(sizeof(double) * linv_size(round_up(c.maxdim_large, 16)) * MVN_MAXBATCH));
    }
    c.grad.ready = false;
    MCML_HIP(hipStreamSynchronize(c.stream));
    return MCML_OK;
}

// ------------------------------------------------------------------ loglik
int mvn_loglik_sum(Ctx& c, const double* theta, double* sum_out)
{
    MCML_REQUIRE(c.mcols > 0 && c.U.d(), "mvn_ll: no samples set");
    return mvn_loglik_sum_on(c, theta, c.U.d(), c.U.ld, c.mcols, sum_out);
}

// The large blocks of D for kb >= 1 candidate thetas th[0..kb), enqueued.  W holds the kb matrices side by side
// (matrix j = columns [j * dmax, (j + 1) * dmax), sized by the caller); the m sample columns ride below each matrix as
// m extra rows (U', one sample per row), so the forward substitution happens inside the factorisation (potrf_blocked).
// Candidate j's terms are added to scal[j * sstride] (scal[j * sstride + 1 .. 2]: log-determinant and sum of squares
// of the block at hand); a failed pivot raises flags[j].
//
// A batch (kb > 1) is launched EAGERLY with the two-stream fork-join of potrf_blocked (the leaf of step t+1 beside the
// bulk of step t): 13.4 ms per round of 8 at Q = 5000 and 1.95 ms at Q = 2000, against 14.4 / 2.21 ms for a
// one-chain graph (measured, then removed) -- a graph without a parallel branch cannot overlap the two, and one
// with a branch is subject to the executable lottery described at CholGraph.  The host keeps ahead easily (~250
// launches per round).  kb = 1 (a single evaluation, or the last round of k = 8 j + 1 candidates) takes the graph.
// round > 1: the kb matrices are the representatives of a round of `round` candidates (mvn_loglik_batch_parts); they
// take the batch's schedule whatever kb is.  parts (nullable): 2 doubles per candidate, += (log-determinant, sum of
// squares) of every block.  grad (nullable, kb = 1): the block's gradient terms follow its value terms (mvn_grad_large), while
// c.chol.linv still holds this block's inverted diagonal blocks.
static int mvn_large_blocks(Ctx& c, DevMat& W, int kb, const ThetaArg* th, const double* Us, int ldu, int m,
                            double* scal, int sstride, int* flags, int round = 0, double* parts = nullptr,
                            const GradJob* grad = nullptr)
{
    const bool batch = (round ? round : kb) > 1;
    const CovSpec& cs = c.cov;
    const int32_t* dcov = c.d_cov.as<int32_t>();
    const CovBlock* dblk = c.d_blocks.as<CovBlock>();
    const int ld = W.ld, dmax = round_up(c.maxdim_large, 16);
    Bat bt; bt.n = kb; bt.sA = (size_t)ld * dmax; bt.sL = linv_size(dmax); bt.err = flags; bt.round = round;
    ThetaBatch tb;
    memset(&tb, 0, sizeof tb);
    for (int j = 0; j < kb; ++j) tb.t[j] = th[j];
    for (int b = 0; b < cs.B; ++b) {
        const CovBlock& blk = cs.blocks[b];
        if (blk.all_gr || blk.dim <= SMALL_BLOCK) continue;
        const int d = blk.dim;
        // a multiple of 16 (identity border): the extra rows and every panel stay 16-byte aligned and the last, ragged
        // panel still has a K the LDS-DMA kernel takes (5000 = 39 x 128 + 8 would fall back to the register-staged one)
        const int dp = round_up(d, 16);
        c.mvn_ws[&W == &c.Dbatch] = Ctx::MvnWs{d, dp, m, ld, kb};
        const dim3 gb((dp + 63) / 64, (dp + 15) / 16, kb);
        if (!batch)
            hipLaunchKernelGGL(k_build_dense, gb, dim3(256), 0, c.stream, W.d(), ld, b, dblk, dcov, cs.rows, c.d_data.d(),
                               th[0], 0, dp);
        else
            hipLaunchKernelGGL(k_build_dense_batch, gb, dim3(256), 0, c.stream, W.d(), ld, bt.sA, b, dblk, dcov, cs.rows,
                               c.d_data.d(), tb, dp);
        MCML_HIP(hipGetLastError());
        MCML_TRY(dev_transpose(c, Us + blk.matstart, ldu, d, m, W.d() + dp, ld, kb, bt.sA));
        if (dp > d)          // the border columns of the sample rows must be finite: they meet zeros only
            for (int j = 0; j < kb; ++j)
                MCML_HIP(hipMemset2DAsync(W.d() + j * bt.sA + dp + (size_t)d * ld, sizeof(double) * ld, 0, sizeof(double) * m, dp - d, c.stream));
        MCML_TRY(leaf_prepare(c, dmax, kb));
        MCML_TRY(batch ? potrf_blocked(c, W.d(), ld, dp, m, bt) : potrf_graphed(c, W.d(), ld, dp, m, bt));
        // the solved samples: m rows x d columns below each factor
        const int gx = (m + 255) / 256, gy = d < 64 ? d : 64;
        MCML_TRY(c.partials.ensure(sizeof(double) * (size_t)(gx * gy + 16)));
        for (int j = 0; j < kb; ++j) {
            double* sj = scal + (size_t)j * sstride;
            const double* Aj = W.d() + j * bt.sA;
            MCML_TRY(dev_sumsq_partials(c, Aj + dp, ld, m, d, gx, gy, c.partials.d()));
            MCML_TRY(dev_sum(c, c.partials.d(), gx * gy, sj + 2));
            MCML_TRY(dev_logdet_chol(c, Aj, ld, d, sj + 1));
            hipLaunchKernelGGL(k_finish_large, dim3(1), dim3(1), 0, c.stream, sj, d, m);
        }
        if (parts) hipLaunchKernelGGL(k_accum_parts, dim3(1), dim3(kb), 0, c.stream, scal, sstride, parts);
        MCML_HIP(hipGetLastError());
        if (grad) MCML_TRY(mvn_grad_large(c, *grad, b, W, dp, m, scal + 1));
    }
    return MCML_OK;
}

static int mvn_loglik_enqueue(Ctx& c, const double* theta, const double* Us, int ldu, int m, const GradJob* grad = nullptr)
{
    MCML_REQUIRE(m > 0 && Us, "mvn_ll: no samples set");
    ThetaArg th;
    MCML_TRY(theta_arg(theta, c.cov.npar, th));
    const CovSpec& cs = c.cov;
    const int Q = cs.N;
    double* scal = c.scalars.d();
    const int32_t* dcov = c.d_cov.as<int32_t>();
    const CovBlock* dblk = c.d_blocks.as<CovBlock>();
    const int* drb = c.d_rowblock.as<int>();
    MCML_HIP(hipMemsetAsync(scal, 0, sizeof(double) * 4, c.stream));

    if (c.n_diag_rows > 0) {
        MCML_TRY(c.partials.ensure(sizeof(double) * (size_t)(2 * Q + 65536)));
        double* dd = c.partials.d();
        double* dc = dd + Q;
        double* part = dc + Q;
        hipLaunchKernelGGL(k_diag_prep, dim3((Q + 255) / 256), dim3(256), 0, c.stream, Q, drb, dblk, dcov,
                           cs.rows, th, dd, dc);
        dim3 grid((Q + 255) / 256, 1);
        int gy = 65536 / (int)grid.x; if (gy > m) gy = m; if (gy > 64) gy = 64; if (gy < 1) gy = 1;
        grid.y = gy;
        hipLaunchKernelGGL(k_diag_ll, grid, dim3(256), 0, c.stream, Us, ldu, Q, m, drb, dd, dc, part);
        MCML_HIP(hipGetLastError());
        MCML_TRY(dev_sum(c, part, (int)(grid.x * grid.y), scal, true));
    }
    if (c.n_small > 0) {
        // the block ids were uploaded once by mvn_setup: nothing here needs the host to wait
        int ny = (m + 63) / 64; if (ny > 16) ny = 16;
        DevBuf& wb = c.scratch;      // scratch that outlives the launch
        MCML_TRY(wb.ensure(sizeof(double) * (size_t)c.n_small * ny + 1024));
        double* part = wb.d();
        hipLaunchKernelGGL(k_small_ll, dim3((unsigned)c.n_small, ny), dim3(64), 0, c.stream, Us, ldu, m,
                           c.small_ids.as<int>(), dblk, dcov, cs.rows, c.d_data.d(), th, part, c.errflag());
        MCML_HIP(hipGetLastError());
        MCML_TRY(dev_sum(c, part, c.n_small * ny, scal, true));
    }
    if (c.maxdim_large > 0) {
        if (c.Dwork.rows < c.maxdim_large + 16 + m || c.Dwork.cols < c.maxdim_large + 16) {
            MCML_TRY(c.Dwork.alloc(c.maxdim_large + 16 + m, c.maxdim_large + 16));
            MCML_HIP(hipMemsetAsync(c.Dwork.d(), 0, sizeof(double) * (size_t)c.Dwork.ld * (c.maxdim_large + 16), c.stream));
        }
        MCML_TRY(mvn_large_blocks(c, c.Dwork, 1, &th, Us, ldu, m, scal, 4, c.errflag(), 0, nullptr, grad));
    }
    return MCML_OK;
}

int mvn_loglik_sum_on(Ctx& c, const double* theta, const double* Us, int ldu, int m, double* sum_out)
{
    MCML_TRY(mvn_loglik_enqueue(c, theta, Us, ldu, m));
    MCML_TRY(copy_d2h(sum_out, c.scalars.d(), sizeof(double), c.stream));
    MCML_TRY(check_errflag(c, "mvn_ll: covariance block is not positive definite"));
    return MCML_OK;
}

// The score (mvn_grad.h).  The value path runs exactly as mvn_loglik_sum_on enqueues it -- the same kernels in the same order,
// so the workspace, the graph cache and, with unit weights, the value are what that call leaves -- with each large block's
// gradient step after its value terms; the diagonal rows and the small blocks follow in buffers of their own.  One
// read-back at the end; the slots are added to their parameters on the host, block by block.
int mvn_loglik_grad(Ctx& c, const double* theta, const double* weights, double* value, double* grad)
{
    MCML_REQUIRE(c.mcols > 0 && c.U.d(), "mvn_ll: no samples set");
    MCML_REQUIRE(theta && value && grad, "mvn_ll_grad: null argument");
    const int m = c.mcols, R = c.cov.npar;
    GradJob gj;
    MCML_TRY(theta_arg(theta, c.cov.npar, gj.th));
    gj.sw = (double)m;
    if (weights) {
        gj.sw = 0;
        for (int j = 0; j < m; ++j) {
            MCML_REQUIRE(weights[j] >= 0.0 && std::isfinite(weights[j]), "mvn_ll_grad: weight %d is negative or not finite", j);
            gj.sw += weights[j];
        }
    }
    MCML_TRY(mvn_grad_setup(c));
    Ctx::MvnGrad& g = c.grad;
    if (weights) {
        MCML_TRY(g.w.ensure(sizeof(double) * (size_t)m));
        MCML_TRY(copy_h2d(g.w.p, weights, sizeof(double) * (size_t)m, c.stream));
        gj.w = g.w.d();
    }
    MCML_HIP(hipMemsetAsync(g.res.p, 0, sizeof(double) * g.res_len, c.stream));
    int rc = mvn_loglik_enqueue(c, theta, c.U.d(), c.U.ld, m, &gj);
    if (rc == MCML_OK) rc = mvn_grad_diag_small(c, gj, c.U.d(), c.U.ld, m);
    std::vector<double> res(g.res_len);
    double sum = 0;
    if (rc == MCML_OK) rc = copy_d2h(res.data(), g.res.p, sizeof(double) * g.res_len, c.stream);
    if (rc == MCML_OK) rc = copy_d2h(&sum, c.scalars.d(), sizeof(double), c.stream);
    const int rc_flag = check_errflag(c, "mvn_ll_grad: covariance block is not positive definite");   // clears a raised flag
    if (rc != MCML_OK) return rc;
    MCML_TRY(rc_flag);
    const CovSpec& cs = c.cov;
    // unit weights stand for 1 / m each: the sums are divided as glmmr_mcml_ctx_mvn_ll divides its own
    const double div = (double)m;
    *value = weights ? res[0] + res[1] + res[2 + R] : sum / div;
    for (int k = 0; k < R; ++k) grad[k] = res[2 + k];
    for (int b = 0; b < cs.B; ++b)
        for (int s = 0; s < g.slot_count[b]; ++s)
            grad[g.slot_par[g.slot_base[b] + s]] += 0.5 * res[3 + R + g.slot_base[b] + s];
    if (!weights) for (int k = 0; k < R; ++k) grad[k] /= div;
    return MCML_OK;
}

// k candidate thetas in ONE pass of the factorisation's schedule.  A single evaluation of a large dense block is a
// latency chain (40 steps of leaf + two single-block products, ~70 us each, on a handful of CUs; 0.24 of the FP64 MFMA
// peak at Q = 5000); with the k matrices side by side in one workspace every launch covers all of them, so the chain
// is paid once per round.  (Measured dead end: the k evaluations as k independent streams / graphs -- "lanes" -- do
// not overlap on this stack: 3.6 ms per evaluation alone, 4.1 / 4.8 / 5.0 ms each with 2 / 4 / 8 lanes, worse with
// more hardware queues.)  Models whose D has diagonal or small blocks besides, and k = 1, take the single path.
static bool mvn_batchable(const Ctx& c) { return c.maxdim_large > 0 && c.n_small == 0 && c.n_diag_rows == 0; }

// the side-by-side pass in chunks of MVN_MAXBATCH.  round / parts: see mvn_large_blocks (parts here: host, 2 per candidate)
static int mvn_batch_pass(Ctx& c, const double* thetas, int k, int round, const double* Us, int ldu, int m, double* sums,
                          int* rcs, double* parts)
{
    const int R = c.cov.npar;
    for (int j0 = 0; j0 < k; j0 += MVN_MAXBATCH) {
        const int kb = (k - j0 < MVN_MAXBATCH) ? k - j0 : MVN_MAXBATCH;
        ThetaArg th[MVN_MAXBATCH];
        for (int j = 0; j < kb; ++j) MCML_TRY(theta_arg(thetas + (size_t)(j0 + j) * R, R, th[j]));
        const int dmax = round_up(c.maxdim_large, 16);
        if (c.Dbatch.rows < dmax + m || c.Dbatch.cols < kb * dmax) {
            MCML_TRY(c.Dbatch.alloc(dmax + m, MVN_MAXBATCH * dmax));
            MCML_HIP(hipMemsetAsync(c.Dbatch.d(), 0, sizeof(double) * (size_t)c.Dbatch.ld * MVN_MAXBATCH * dmax, c.stream));
        }
        // results: 4 doubles per candidate, then one "not positive definite" flag (int) per candidate, then the two
        // summed terms per candidate -- a buffer of their own (c.scalars is shared with the sampler's diagnostics)
        MCML_TRY(c.bscal.ensure(sizeof(double) * 7 * MVN_MAXBATCH));
        MCML_HIP(hipMemsetAsync(c.bscal.p, 0, sizeof(double) * 7 * MVN_MAXBATCH, c.stream));
        int* bflags = reinterpret_cast<int*>(c.bscal.d() + 4 * MVN_MAXBATCH);
        double* bparts = c.bscal.d() + 5 * MVN_MAXBATCH;
        MCML_TRY(mvn_large_blocks(c, c.Dbatch, kb, th, Us, ldu, m, c.bscal.d(), 4, bflags, round, parts ? bparts : nullptr));
        double hs[4 * MVN_MAXBATCH]; int hf[MVN_MAXBATCH];
        MCML_TRY(copy_d2h(hs, c.bscal.p, sizeof(double) * 4 * kb, c.stream));
        MCML_TRY(copy_d2h(hf, bflags, sizeof(int) * kb, c.stream));
        if (parts) MCML_TRY(copy_d2h(parts + 2 * (size_t)j0, bparts, sizeof(double) * 2 * kb, c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
        for (int j = 0; j < kb; ++j) { sums[j0 + j] = hs[4 * j]; rcs[j0 + j] = hf[j] ? MCML_ENOTPD : MCML_OK; }
    }
    return MCML_OK;
}

int mvn_loglik_batch(Ctx& c, const double* thetas, int k, const double* Us, int ldu, int m, double* sums, int* rcs)
{
    MCML_REQUIRE(k >= 1 && thetas && sums && rcs && m > 0 && Us, "mvn_ll batch: bad arguments");
    const int R = c.cov.npar;
    const bool batchable = k > 1 && mvn_batchable(c);
    if (!batchable) {
        int first_rc = MCML_OK;
        for (int j = 0; j < k; ++j) {
            rcs[j] = mvn_loglik_sum_on(c, thetas + (size_t)j * R, Us, ldu, m, sums + j);
            if (rcs[j] != MCML_OK && rcs[j] != MCML_ENOTPD && first_rc == MCML_OK) first_rc = rcs[j];
        }
        return first_rc;
    }
    return mvn_batch_pass(c, thetas, k, 0, Us, ldu, m, sums, rcs, nullptr);
}

// The k REPRESENTATIVES of a round of `round` > 1 candidates (theta_scale.h: the others share a representative's
// factorisation up to a scale), dense-block models only.  As mvn_loglik_batch, and parts[2 j .. 2 j + 1] = candidate
// j's log-determinant and sum of squares summed over the blocks -- the two terms k_finish_large combines.
// What decides the two-level blocking: the size of the ROUND (potrf_blocked), so a round of 8 reduced to 5 matrices, or
// to one, regroups its sums exactly as the full round did; with k == round the sums are mvn_loglik_batch's to the bit.
// A chunk of one (k = 8 j + 1 representatives) therefore runs the eager two-level schedule here, not the single
// evaluation's graph mvn_loglik_batch gives such a chunk: a 1e-13 difference in that candidate's value.
int mvn_loglik_batch_parts(Ctx& c, const double* thetas, int k, int round, const double* Us, int ldu, int m, double* sums,
                           int* rcs, double* parts)
{
    MCML_REQUIRE(k >= 1 && round >= k && round > 1 && thetas && sums && rcs && parts && m > 0 && Us, "mvn_ll batch parts: bad arguments");
    MCML_REQUIRE(mvn_batchable(c), "mvn_ll batch parts: the model has blocks that are not factorised side by side");
    return mvn_batch_pass(c, thetas, k, round, Us, ldu, m, sums, rcs, parts);
}

// ------------------------------------------------------------------ genD
__global__ void k_diag_fill(double* L, int ldl, int Q, const int* rowblock, const CovBlock* blocks,
                            const int32_t* cov, int rows, ThetaArg th, int chol)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Q) return;
    int b = rowblock[k];
    if (b < 0) return;
    const double val = cov_prior_variance(blocks[b], cov, rows, th);
    L[k + (size_t)k * ldl] = chol ? sqrt(val) : val;
}

// D(theta) or its block-diagonal lower factor built into L, which may be any Q x Q matrix: the context's state is not touched
static int gen_D_into(Ctx& c, DevMat& L, const ThetaArg& th, bool chol)
{
    const CovSpec& cs = c.cov;
    const int Q = cs.N;
    MCML_TRY(L.alloc(Q, Q));
    MCML_HIP(hipMemsetAsync(L.d(), 0, sizeof(double) * (size_t)L.ld * Q, c.stream));
    const int32_t* dcov = c.d_cov.as<int32_t>();
    const CovBlock* dblk = c.d_blocks.as<CovBlock>();
    if (c.n_diag_rows > 0)
        hipLaunchKernelGGL(k_diag_fill, dim3((Q + 255) / 256), dim3(256), 0, c.stream, L.d(), L.ld, Q,
                           c.d_rowblock.as<int>(), dblk, dcov, cs.rows, th, chol ? 1 : 0);
    for (int b = 0; b < cs.B; ++b) {
        const CovBlock& blk = cs.blocks[b];
        if (blk.all_gr) continue;
        const int d = blk.dim;
        double* A = L.at(blk.matstart, blk.matstart);
        dim3 g((d + 63) / 64, (d + 15) / 16);
        hipLaunchKernelGGL(k_build_dense, g, dim3(256), 0, c.stream, A, L.ld, b, dblk, dcov, cs.rows,
                           c.d_data.d(), th, chol ? 0 : 1, d);
        MCML_HIP(hipGetLastError());
        if (chol) {
            // blocks start at arbitrary (possibly odd) offsets: factorise in the
            // aligned workspace when the view is not 16-byte aligned
            if (d <= CHOL_NB || (blk.matstart & 1) == 0) {
                MCML_TRY(potrf_lower(c, A, d, L.ld));
            } else {
                DevMat tmp;
                MCML_TRY(tmp.alloc(d, d));
                hipLaunchKernelGGL(k_copy_block, dim3((d + 255) / 256, d < 256 ? d : 256), dim3(256), 0, c.stream,
                                   tmp.d(), tmp.ld, A, L.ld, d, d);
                MCML_TRY(potrf_lower(c, tmp.d(), d, tmp.ld));
                hipLaunchKernelGGL(k_copy_block, dim3((d + 255) / 256, d < 256 ? d : 256), dim3(256), 0, c.stream,
                                   A, L.ld, tmp.d(), tmp.ld, d, d);
                MCML_HIP(hipStreamSynchronize(c.stream));
            }
            // the SYRK updates of diagonal tiles also touch their upper halves
            if (d > CHOL_NB)
                hipLaunchKernelGGL(k_zero_upper, dim3((d + 255) / 256, d), dim3(256), 0, c.stream, A, L.ld, d);
        }
    }
    MCML_HIP(hipGetLastError());
    return check_errflag(c, "genD: covariance block is not positive definite");
}

// block b's covariance matrix (lower triangle, identity border up to dpad) into the caller's array, enqueued: the build step
// of mvn_large_blocks for a caller with a workspace of its own (predict.hip)
int mvn_build_block(Ctx& c, double* A, int lda, int b, const double* theta, int dpad)
{
    ThetaArg th;
    MCML_TRY(theta_arg(theta, c.cov.npar, th));
    MCML_REQUIRE(b >= 0 && b < c.cov.B && A && dpad >= c.cov.blocks[b].dim && lda >= dpad, "mvn_build_block: bad argument");
    hipLaunchKernelGGL(k_build_dense, dim3((dpad + 63) / 64, (dpad + 15) / 16), dim3(256), 0, c.stream, A, lda, b,
                       c.d_blocks.as<CovBlock>(), c.d_cov.as<int32_t>(), c.cov.rows, c.d_data.d(), th, 0, dpad);
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

// A query (glmmr_mcml_ctx_gen_D): into the caller's matrix, so c.L, have_L and l_foreign stay as they are
int mvn_gen_D(Ctx& c, const double* theta, bool chol, DevMat& out)
{
    ThetaArg th;
    MCML_TRY(theta_arg(theta, c.cov.npar, th));
    return gen_D_into(c, out, th, chol);
}

// c.L is overwritten in place (its address keys captured graphs), so a build that fails half way -- a block that is not
// positive definite -- leaves no L at all: every consumer requires have_L and refuses until the next successful call
int mvn_gen_L(Ctx& c, const double* theta, bool chol)
{
    ThetaArg th;
    MCML_TRY(theta_arg(theta, c.cov.npar, th));
    c.have_L = false;
    MCML_TRY(gen_D_into(c, c.L, th, chol));
    if (chol) c.l_foreign = false;
    c.have_L = chol;
    return MCML_OK;
}

}  // namespace mcml
