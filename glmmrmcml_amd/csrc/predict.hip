// predict.hip -- conditional (kriging) prediction of the random effects at new locations (a query: DESIGN.md 5.10).
// Block b of D(theta) gets k_b new points (rows of a k_b x ncol_b matrix with the columns of the block's data matrix).  With
// C_b (k_b x dim_b) the cross-covariance, p the prior variance (the block's product at distance 0), D_b = L L',
// W' = L^-1 C_b' and Y = L^-1 U_b (U_b: the block's rows of the resident samples c.U):
//     means[i, j] = (W Y)[i, j] = (C_b D_b^-1 u_bj)[i]          cvar[i] = max(p - |W[i, :]|^2, 0)
// and the summary row of point i is (mean_j means[i, j], cvar[i], var_j means[i, j] with divisor m - 1, NaN at m = 1).
// One path per block kind, the three of mvn.hip:
//   k_pred_diag     all-gr blocks (diagonal): means[i, j] = sum_k (C_ik / D_kk) u_kj, cvar = max(p - sum_k C_ik (C_ik / D_kk), 0), k
//                   ascending; a point that matches one level has C_ik / D_kk = 1 there and 0 elsewhere: the level's sample to
//                   the bit and variance 0; one that matches none gets 0 and p
//   k_pred_small    dim <= 32: a wave builds and factorises D_b in LDS (small_block_factor, cov_block.h: k_small_ll's factor to
//                   the bit), forward-substitutes 64 rows of C_b and 64 sample columns (small_block_forward, a lane each), then
//                   forms the 64 x 64 tile of means; further new points and sample columns are the two grid dimensions
//   larger blocks   D_b by k_build_dense into the query's own workspace, the eager potrf_blocked (never the captured graphs of
//                   the theta-step: they are keyed by workspace pointer and stay where they are), Y by trsm_left_lower on a
//                   copy of U_b -- once per block; then per chunk of new points k_build_cross (C_b' stored d x kc), the same
//                   solve, k_pred_cvar (column sums of squares, a wave per column) and means = (W')' Y by the transposed-A
//                   MFMA GEMM.  The block is padded to a multiple of 16 with an identity border as mvn_large_blocks pads it,
//                   the border rows of C_b' and of Y are zero
// New points go through in chunks of at most kc rows: the means of the chunks collect in one buffer of PREDICT_CAP_BYTES at
// most (with C_b'), and a full buffer is flushed -- k_pred_summary (two-pass, j ascending, a thread per row), and the download
// of the rows where the caller wants the means -- so the workspace is bounded whatever K is.  GLMMR_MCML_PREDICT_CHUNK, read
// per call, forces a smaller kc.  Everything runs on c.stream, no atomics but the error flag, every sum in a fixed order: two
// calls and two contexts return the same bits.  Nothing that a sampler, a fit, mvn_ll, its score, a Laplace call or an
// information query reads is changed; c.chol.linv is overwritten, as by every factorisation.
#include "entry.h"
#include "cov_block.h"
#include "dgemm_mfma.h"
#include "reduce.h"
#include <algorithm>
#include <chrono>
#include <cmath>

namespace mcml {

constexpr size_t PREDICT_CAP_BYTES = (size_t)256 << 20;      // C_b' (d x kc) + the means buffer (rows x m), doubles

__global__ __launch_bounds__(256) void k_pred_diag(const double* U, int ldu, int m, int b, const CovBlock* blocks,
                                                   const int32_t* cov, int rows, const double* data, const double* xn,
                                                   int knew, ThetaArg th, double* Mn, int ldm, double* cvar)
{
    __shared__ double wsh[256];
    const CovBlock blk = blocks[b];
    const int i = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
    const double p = cov_prior_variance(blk, cov, rows, th);         // = D_kk of every level
    double acc = 0, q = 0;
    for (int k0 = 0; k0 < blk.dim; k0 += 256) {
        const int k = k0 + threadIdx.x;
        __syncthreads();
        wsh[threadIdx.x] = k < blk.dim ? cov_cross_entry(blk, cov, rows, data + blk.doff, xn, knew, th, i, k) : 0.0;
        __syncthreads();
        const int lim = blk.dim - k0 < 256 ? blk.dim - k0 : 256;
        for (int t = 0; t < lim; ++t) {
            const double cik = wsh[t];
            if (cik == 0.0) continue;                                // the level does not match: 0 to both sums
            const double w = cik / p;
            if (j < m) acc += w * U[blk.matstart + k0 + t + (size_t)j * ldu];
            q += cik * w;
        }
    }
    if (j < m) Mn[i + (size_t)j * ldm] = acc;
    if (blockIdx.y == 0 && threadIdx.x == 0) cvar[i] = fmax(p - q, 0.0);
}

// grid (ceil(kcur / 64), ceil(m / 64)), one wave; the cvar of a point is written by the wave of sample-column pass 0
__global__ __launch_bounds__(64) void k_pred_small(const double* U, int ldu, int m, int b, const CovBlock* blocks,
                                                   const int32_t* cov, int rows, const double* data, const double* xn,
                                                   int knew, int kcur, ThetaArg th, double* Mn, int ldm, double* cvar,
                                                   int* errflag)
{
    __shared__ double S[SMALL_BLOCK * SMALL_LS];
    __shared__ double Zs[SMALL_BLOCK * 64];
    __shared__ double Ws[SMALL_BLOCK * 64];
    const CovBlock blk = blocks[b];
    const int dim = blk.dim, lane = threadIdx.x;
    const double* bd = data + blk.doff;
    small_block_factor(S, blk, cov, rows, bd, th, errflag);
    const int i0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int cnt = kcur - i0 < 64 ? kcur - i0 : 64, ccnt = m - c0 < 64 ? m - c0 : 64;
    if (lane < cnt) {                                                // row i0 + lane of C_b: w = L^-1 c
        const double q = small_block_forward(S, dim, Ws, lane, [&](int k) {
            return cov_cross_entry(blk, cov, rows, bd, xn, knew, th, i0 + lane, k);
        });
        if (blockIdx.y == 0) cvar[i0 + lane] = fmax(cov_prior_variance(blk, cov, rows, th) - q, 0.0);
    }
    if (lane < ccnt) {                                               // sample column c0 + lane: y = L^-1 u
        const double* u = U + blk.matstart + (size_t)(c0 + lane) * ldu;
        small_block_forward(S, dim, Zs, lane, [&](int k) { return u[k]; });
    }
    __syncthreads();
    if (lane < cnt)
        for (int cj = 0; cj < ccnt; ++cj) {                          // a lane per new point: the stores of a column are contiguous
            double acc = 0;
            for (int k = 0; k < dim; ++k) acc += Ws[k * 64 + lane] * Zs[k * 64 + cj];
            Mn[i0 + lane + (size_t)(c0 + cj) * ldm] = acc;
        }
}

// dst (dp x m) = rows [0, d) of src, zero rows up to dp
__global__ __launch_bounds__(256) void k_pred_copy_rows(double* dst, int ldd, const double* src, int lds, int d, int dp, int m)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dp) return;
    for (int j = blockIdx.y; j < m; j += gridDim.y) dst[i + (size_t)j * ldd] = i < d ? src[i + (size_t)j * lds] : 0.0;
}

// C_b' (dp x kcur, zero border rows), rectangular: a 64 x 16 workgroup as lower_tile_walk's (cov_block.h), the 64 along the
// observed index, so every store of a wave is 512 contiguous bytes
__global__ __launch_bounds__(256) void k_build_cross(double* CT, int ld, int b, const CovBlock* blocks, const int32_t* cov,
                                                     int rows, const double* data, const double* xn, int knew, int kcur,
                                                     ThetaArg th, int dp)
{
    const CovBlock blk = blocks[b];
    const int k = blockIdx.x * 64 + (threadIdx.x & 63);
    if (k >= dp) return;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = blockIdx.y * 16 + (threadIdx.x >> 6) * 4 + u;
        if (i >= kcur) continue;
        CT[k + (size_t)i * ld] = k < blk.dim ? cov_cross_entry(blk, cov, rows, data + blk.doff, xn, knew, th, i, k) : 0.0;
    }
}

// cvar[i] = max(p - sum_k W'[k, i]^2, 0): a wave per column, lane l adds rows l, l + 64, ... in turn, then wave_sum
__global__ __launch_bounds__(256) void k_pred_cvar(const double* WT, int ld, int dp, int kcur, int b, const CovBlock* blocks,
                                                   const int32_t* cov, int rows, ThetaArg th, double* cvar)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= kcur) return;                                           // the whole wave
    const double* w = WT + (size_t)i * ld;
    double acc = 0;
    for (int k = lane; k < dp; k += 64) acc += w[k] * w[k];
    acc = wave_sum(acc);
    if (lane == 0) cvar[i] = fmax(cov_prior_variance(blocks[b], cov, rows, th) - acc, 0.0);
}

// rows [0, n) of the means buffer -> columns 0 and 2 of the summary at rows [g0, g0 + n): two passes, j ascending
__global__ __launch_bounds__(256) void k_pred_summary(const double* Mn, int ldm, int n, int m, double* sum, int K, int g0)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0;
    for (int j = 0; j < m; ++j) s += Mn[i + (size_t)j * ldm];
    const double mean = s / m;
    double ss = 0;
    for (int j = 0; j < m; ++j) { const double d = Mn[i + (size_t)j * ldm] - mean; ss += d * d; }
    sum[g0 + i] = mean;
    sum[g0 + i + 2 * (size_t)K] = m > 1 ? ss / (m - 1) : NAN;
}

// GLMMR_MCML_PREDICT_PHASES=1 (read per call; scripts/time_predict.py): the stream is synchronised after every phase and the
// host clock read; one line on stderr ends the call.  build | factor | solves | product | summary, the diagonal and the
// small kernels under product.  Off: lap() does nothing
struct PredictPhases {
    bool on;
    double ms[5] = {0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t;
    explicit PredictPhases(hipStream_t s) : on(getenv("GLMMR_MCML_PREDICT_PHASES") && atoi(getenv("GLMMR_MCML_PREDICT_PHASES")) > 0)
    {
        if (on) { (void)hipStreamSynchronize(s); t = std::chrono::steady_clock::now(); }
    }
    void lap(hipStream_t s, int k)
    {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        ms[k] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    }
    void print() const
    {
        if (on) fprintf(stderr, "predict_re phases ms: build %.4f factor %.4f solves %.4f product %.4f summary %.4f\n", ms[0], ms[1],
                        ms[2], ms[3], ms[4]);
    }
};

static int predict_chunk_rows(int cap_rows)
{
    const char* e = getenv("GLMMR_MCML_PREDICT_CHUNK");
    const int v = e ? atoi(e) : 0;
    return v > 0 && v < cap_rows ? v : cap_rows;
}

int predict_re(Ctx& c, const double* theta, const int* nnew, const double* newdata, long long newdata_len, double* summary,
               int lds, double* means, int ldm)
{
    MCML_REQUIRE(theta && nnew && newdata && summary, "predict_re: null argument");
    MCML_REQUIRE(c.mcols > 0 && c.U.d(), "predict_re: no samples set");
    const CovSpec& cs = c.cov;
    const int m = c.mcols;
    long long Kll = 0, need = 0;
    for (int b = 0; b < cs.B; ++b) {
        MCML_REQUIRE(nnew[b] >= 0, "predict_re: block %d has a negative number of new points", b);
        Kll += nnew[b];
        need += (long long)nnew[b] * cs.blocks[b].ncol;
    }
    MCML_REQUIRE(Kll > 0, "predict_re: no new points");
    MCML_REQUIRE(Kll < (1ll << 30), "predict_re: %lld new points, at most 2^30 - 1", Kll);
    MCML_REQUIRE(need == newdata_len, "predict_re: newdata holds %lld values, the counts need %lld", newdata_len, need);
    const int K = (int)Kll;
    MCML_REQUIRE(lds >= K && (!means || ldm >= K), "predict_re: leading dimension below the %d new points", K);
    ThetaArg th;
    MCML_TRY(theta_arg(theta, cs.npar, th));

    PredictState& x = c.predict;
    const int dmaxp = c.maxdim_large ? round_up(c.maxdim_large, 16) : SMALL_BLOCK;
    // rows of the means buffer: what the cap leaves beside a C_b' chunk of as many columns, in 64s, no more than K needs
    int cap_rows = (int)std::min<size_t>(PREDICT_CAP_BYTES / (sizeof(double) * ((size_t)dmaxp + m)) / 64 * 64, (size_t)round_up(K, 64));
    if (cap_rows < 64) cap_rows = 64;
    const int kc = predict_chunk_rows(cap_rows);
    MCML_TRY(x.nd.ensure(sizeof(double) * (size_t)need));
    MCML_TRY(copy_h2d(x.nd.p, newdata, sizeof(double) * (size_t)need, c.stream));
    MCML_TRY(x.sum.ensure(sizeof(double) * 3 * (size_t)K));
    MCML_TRY(x.M.alloc(cap_rows, m));
    long long plan[8] = {0, 0, 0, K, 0, 0, 0, m};
    std::vector<double> hm;                                           // the means are handed over only when the whole call succeeded
    if (means) hm.resize((size_t)K * m);

    const int32_t* dcov = c.d_cov.as<int32_t>();
    const CovBlock* dblk = c.d_blocks.as<CovBlock>();
    int fill = 0, g0 = 0;
    PredictPhases ph(c.stream);
    auto flush = [&]() -> int {
        if (!fill) return MCML_OK;
        hipLaunchKernelGGL(k_pred_summary, dim3((fill + 255) / 256), dim3(256), 0, c.stream, x.M.d(), x.M.ld, fill, m, x.sum.d(), K, g0);
        MCML_HIP(hipGetLastError());
        if (means) {
            MCML_TRY(copy_d2h_2d(hm.data() + g0, sizeof(double) * (size_t)K, x.M.d(), sizeof(double) * (size_t)x.M.ld,
                                 sizeof(double) * (size_t)fill, (size_t)m, c.stream));
            MCML_HIP(hipStreamSynchronize(c.stream));
        }
        g0 += fill; fill = 0;
        ph.lap(c.stream, 4);
        return MCML_OK;
    };

    size_t noff = 0;
    int koff = 0;
    for (int b = 0; b < cs.B; ++b) {
        const CovBlock& blk = cs.blocks[b];
        const int kb = nnew[b], d = blk.dim;
        if (!kb) continue;
        const double* xn = x.nd.d() + noff;
        const bool diag = blk.all_gr, small = !diag && d <= SMALL_BLOCK;
        ++plan[diag ? 0 : small ? 1 : 2];
        const int dp = round_up(d, 16);
        if (!diag && !small) {
            // ---- D_b, its factor, Y = L^-1 U_b: once per block
            MCML_TRY(x.D.alloc(dmaxp, dmaxp));
            MCML_TRY(x.Y.alloc(dmaxp, m));
            MCML_TRY(x.CT.alloc(dmaxp, kc));
            MCML_TRY(mvn_build_block(c, x.D.d(), x.D.ld, b, theta, dp));
            ph.lap(c.stream, 0);
            MCML_TRY(leaf_prepare(c, dp, 1));
            MCML_TRY(potrf_blocked(c, x.D.d(), x.D.ld, dp, 0));
            ph.lap(c.stream, 1);
            ++plan[5];
            hipLaunchKernelGGL(k_pred_copy_rows, dim3((dp + 255) / 256, m < 1024 ? m : 1024), dim3(256), 0, c.stream, x.Y.d(), x.Y.ld,
                               c.U.d() + blk.matstart, c.U.ld, d, dp, m);
            MCML_HIP(hipGetLastError());
            MCML_TRY(trsm_left_lower(c, x.D.d(), x.D.ld, dp, x.Y.d(), x.Y.ld, m));
            ph.lap(c.stream, 2);
        }
        for (int r0 = 0; r0 < kb; r0 += kc) {
            const int kcur = kb - r0 < kc ? kb - r0 : kc;
            if (fill + kcur > cap_rows) MCML_TRY(flush());
            double* Mn = x.M.d() + fill;
            double* cvar = x.sum.d() + K + koff + r0;
            if (diag) {
                hipLaunchKernelGGL(k_pred_diag, dim3(kcur, (m + 255) / 256), dim3(256), 0, c.stream, c.U.d(), c.U.ld, m, b, dblk, dcov,
                                   cs.rows, c.d_data.d(), xn + r0, kb, th, Mn, x.M.ld, cvar);
            } else if (small) {
                hipLaunchKernelGGL(k_pred_small, dim3((kcur + 63) / 64, (m + 63) / 64), dim3(64), 0, c.stream, c.U.d(), c.U.ld, m, b,
                                   dblk, dcov, cs.rows, c.d_data.d(), xn + r0, kb, kcur, th, Mn, x.M.ld, cvar, c.errflag());
            } else {
                hipLaunchKernelGGL(k_build_cross, dim3((dp + 63) / 64, (kcur + 15) / 16), dim3(256), 0, c.stream, x.CT.d(), x.CT.ld, b,
                                   dblk, dcov, cs.rows, c.d_data.d(), xn + r0, kb, kcur, th, dp);
                MCML_HIP(hipGetLastError());
                ph.lap(c.stream, 0);
                MCML_TRY(trsm_left_lower(c, x.D.d(), x.D.ld, dp, x.CT.d(), x.CT.ld, kcur));
                hipLaunchKernelGGL(k_pred_cvar, dim3((kcur + 3) / 4), dim3(256), 0, c.stream, x.CT.d(), x.CT.ld, dp, kcur, b, dblk, dcov,
                                   cs.rows, th, cvar);
                MCML_HIP(hipGetLastError());
                ph.lap(c.stream, 2);
                const EpiAxpby epi{Mn, x.M.ld, 1.0, 0.0};
                MCML_TRY(launch_gemm_at(c.stream, kcur, m, dp, x.CT.d(), x.CT.ld, x.Y.d(), x.Y.ld, epi));
            }
            MCML_HIP(hipGetLastError());
            ph.lap(c.stream, 3);
            fill += kcur;
            ++plan[4];
        }
        noff += (size_t)kb * blk.ncol;
        koff += kb;
    }
    MCML_TRY(flush());
    plan[6] = (long long)(x.nd.bytes + x.sum.bytes + x.M.buf.bytes + x.D.buf.bytes + x.Y.buf.bytes + x.CT.buf.bytes);
    std::copy(plan, plan + 8, x.plan);
    std::vector<double> hs(3 * (size_t)K);
    MCML_TRY(copy_d2h(hs.data(), x.sum.p, sizeof(double) * hs.size(), c.stream));
    MCML_TRY(check_errflag(c, "predict_re: covariance block is not positive definite"));   // synchronises; nothing written yet
    ph.lap(c.stream, 4);
    ph.print();
    for (int col = 0; col < 3; ++col) memcpy(summary + (size_t)col * lds, hs.data() + (size_t)col * K, sizeof(double) * (size_t)K);
    if (means)
        for (int j = 0; j < m; ++j) memcpy(means + (size_t)j * ldm, hm.data() + (size_t)j * K, sizeof(double) * (size_t)K);
    return MCML_OK;
}

}  // namespace mcml
