// mvn_grad.h -- the analytic score of the MVN log-likelihood mvn.hip evaluates: the score's kernels and its per-kind host
// steps, included by mvn.hip alone (mvn_large_blocks calls mvn_grad_large between two blocks):
//   value(theta) = sum_j w_j sum_b log N(u_bj; 0, D_b(theta)),     d value / d theta_k = sum_b 1/2 sum_ij (d_k D_b)_ij H_b,ij,
//   H_b = A diag(w) A' - (sum w) inv(D_b),  A = inv(D_b) U_b.
// Every function of covspec.h's table is a product of terms and the derivative of a term is the term times a closed-form
// factor (cov_term_dlog), so (d_k D)_ij = D_ij * that factor.  A block's parameters are numbered as SLOTS -- term by term, a
// term's parameters in order -- and the host adds the slots' sums to the parameter indices they read (a parameter may be shared
// by terms and blocks of every kind), block by block.  One gradient path per block kind of mvn_setup:
//   * all-gr rows: one streaming pass over U for q_k = sum_j w_j u_kj^2, then r_k = q_k / v_k - sum w and, per parameter p,
//     sum_k c(block(k), p) r_k / theta_p with c = the gr terms of the row's block that read p;
//   * blocks of dim <= 32: one wave per (block, slice of the columns, 64 at a time) builds and factorises the block
//     (small_block_factor, cov_block.h: k_small_ll's factor to the bit), inverts the factor (lower_inverse_column), solves A
//     for its columns (small_block_forward, then backwards), accumulates the lower triangle of H in LDS and contracts
//     it with D o dlog;
//   * large blocks: after the factorisation the workspace holds L and the m solved rows X = (inv(L) U)'.  S = X' diag(w) X -
//     (sum w) I (transposed-A GEMM, K = m, the weights on a copy of the rows), H = inv(L)' S inv(L) by two transposed solves
//     with a transposition between them, and a reduction over the lower 64 x 16 tiles of H (lower_tile_walk) that rebuilds
//     every entry's terms.
//     A slot whose dlog is constant over the block (a pure scale) is coef trace(S) in closed form (k_grad_scale_slot).
// All reductions are two-stage with a fixed order and there is no floating-point atomic: the result is run-to-run
// bit-reproducible and does not depend on what the context did before.
#pragma once
#include "ctx.h"
#include "cov_block.h"
#include "dgemm_mfma.h"
#include "reduce.h"
#include "vecops.h"

namespace mcml {

constexpr int GRAD_SLOTS = 8;        // slots a reduction carries in registers; a block with more takes another pass

// cov_term_dlog, the closed-form factor of a term's derivative: cov_entry.h

// acc[s] += h * D_ij * dlog of slot slot0 + s: cov_entry's walk (cov_walk), the dlog of the slots inside the window
// [slot0, slot0 + GRAD_SLOTS) collected on the way
__device__ __forceinline__ void grad_entry(const CovBlock& blk, const int32_t* cov, int rows, const double* bd,
                                           const ThetaArg& th, int i, int j, double h, int slot0, double (&acc)[GRAD_SLOTS])
{
    double dl[GRAD_SLOTS];
#pragma unroll
    for (int s = 0; s < GRAD_SLOTS; ++s) dl[s] = 0.0;
    int slot = -slot0;
    const double val = cov_walk(
        blk, cov, rows, th, [&](int c) { return bd[i + (size_t)c * blk.dim] - bd[j + (size_t)c * blk.dim]; },
        [&](int fn, int pi, double dist) {
            for (int q = 0; q < CovSpec::fn_npar(fn); ++q, ++slot) {
                if (slot < 0 || slot >= GRAD_SLOTS) continue;
                const double x = cov_term_dlog(fn, dist, &th.v[pi], q);
#pragma unroll
                for (int s = 0; s < GRAD_SLOTS; ++s) dl[s] = (s == slot) ? x : dl[s];
            }
        });
    const double hd = h * val;
#pragma unroll
    for (int s = 0; s < GRAD_SLOTS; ++s) acc[s] += hd * dl[s];
}

// out[x] = sum_{i < n} part[x * bstride + i * istride], one workgroup per output
__global__ __launch_bounds__(256) void k_grad_sum(const double* part, int n, size_t bstride, size_t istride, double* out)
{
    __shared__ double sh[4];
    double v = 0;
    for (int i = threadIdx.x; i < n; i += 256) v += part[blockIdx.x * bstride + i * istride];
    const double r = block_sum(v, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// ------------------------------------------------------------------ diagonal rows
// dd[k] = prod_k theta^2 ("dmat(k,k)*dmat(k,k)"), dc[k] = -0.5 log(dd) - 0.5 log(2 pi); rows of no all-gr block: 1 and 0.
// The value path of mvn.hip launches it as well: it is defined here, in the header that only mvn.hip includes, because a
// kernel in cov_block.h would be emitted into every translation unit that includes that header
__global__ void k_diag_prep(int Q, const int* rowblock, const CovBlock* blocks, const int32_t* cov, int rows, ThetaArg th,
                            double* dd, double* dc)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Q) return;
    int b = rowblock[k];
    if (b < 0) { dd[k] = 1.0; dc[k] = 0.0; return; }
    double d = sqrt(cov_prior_variance(blocks[b], cov, rows, th));   // the Cholesky factor of a diagonal block
    dd[k] = d * d;
    dc[k] = -0.5 * log(d * d) - 0.5 * LOG_2PI;
}

// qpart[by * Q + k] = sum over the columns by, by + gy, ... of w_j u_kj^2: the one pass over U
__global__ __launch_bounds__(256) void k_diag_gradq(const double* U, int ldu, int Q, int mcols, const double* w,
                                                    const int* rowblock, double* qpart)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Q) return;
    double acc = 0;
    if (rowblock[k] >= 0)
        for (int col = blockIdx.y; col < mcols; col += gridDim.y) {
            const double u = U[k + (size_t)col * ldu];
            acc += (w ? w[col] : 1.0) * u * u;
        }
    qpart[(size_t)blockIdx.y * Q + k] = acc;
}

// r[k] = q_k / v_k - sum w and the row's term of the value, sum w (-0.5 log v - 0.5 log 2 pi) - 0.5 q_k / v_k
__global__ void k_diag_gradr(int Q, int gy, const double* qpart, const int* rowblock, const double* dd, const double* dc,
                             double sw, double* r, double* vrow)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Q) return;
    if (rowblock[k] < 0) { r[k] = 0.0; vrow[k] = 0.0; return; }
    double q = 0;
    for (int y = 0; y < gy; ++y) q += qpart[(size_t)y * Q + k];
    r[k] = q / dd[k] - sw;
    vrow[k] = sw * dc[k] - 0.5 * q / dd[k];
}

// workgroup p < npar: out[p] = sum_k c(block(k), p) r_k / theta_p; workgroup npar: out[npar] = sum_k vrow[k]
__global__ __launch_bounds__(256) void k_diag_gradp(int Q, int npar, const int* rowblock, const CovBlock* blocks,
                                                    const int32_t* cov, int rows, ThetaArg th, const double* r,
                                                    const double* vrow, double* out)
{
    __shared__ double sh[4];
    const int p = blockIdx.x;
    double acc = 0;
    for (int k = threadIdx.x; k < Q; k += 256) {
        if (p == npar) { acc += vrow[k]; continue; }
        const int b = rowblock[k];
        if (b < 0) continue;
        int cnt = 0;
        for (int t = blocks[b].r0; t < blocks[b].r1; ++t) cnt += cov[t + 4 * rows] == p;
        if (cnt) acc += cnt * r[k];
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) out[p] = (p == npar) ? s : s / th.v[p];
}

// ------------------------------------------------------------------ small blocks
// gpart[(slot_base[block] + s) * gridDim.y + slice] = sum over the lower triangle of mult H_ij D_ij dlog_s (mult 1 on the
// diagonal, 2 below), H of the slice's columns; vpart[block * gridDim.y + slice] = the slice's weighted value
__global__ __launch_bounds__(64) void k_small_grad(const double* U, int ldu, int mcols, const double* w,
                                                   const int* small_ids, const int* slot_base, const int* nslots,
                                                   const CovBlock* blocks, const int32_t* cov, int rows, const double* data,
                                                   ThetaArg th, double* gpart, double* vpart, int* errflag)
{
    constexpr int LS = SMALL_LS;
    __shared__ double S[SMALL_BLOCK * LS], Li[SMALL_BLOCK * LS], Hs[SMALL_BLOCK * LS];
    __shared__ double Zs[SMALL_BLOCK * 64];
    __shared__ double Ws[64];
    const CovBlock blk = blocks[small_ids[blockIdx.x]];
    const int dim = blk.dim, lane = threadIdx.x;
    const double* bd = data + blk.doff;
    for (int e = lane; e < dim * dim; e += 64) {
        int i = e % dim, j = e / dim;
        if (i >= j) Hs[i * LS + j] = 0.0;
    }
    small_block_factor(S, blk, cov, rows, bd, th, errflag);
    if (lane < dim) lower_inverse_column(S, Li, LS, dim, lane);      // inv(L), lane j its column j
    __syncthreads();
    double logdet = 0;
    for (int i = 0; i < dim; ++i) logdet += 2 * log(S[i * LS + i]);
    double acc = 0, swc = 0;
    for (int col0 = blockIdx.y * 64; col0 < mcols; col0 += gridDim.y * 64) {
        const int col = col0 + lane;
        const bool active = col < mcols;
        const double wj = active ? (w ? w[col] : 1.0) : 0.0;
        if (active) {
            const double* u = U + blk.matstart + (size_t)col * ldu;
            const double quad = small_block_forward(S, dim, Zs, lane, [&](int i) { return u[i]; });   // z = inv(L) u
            acc += wj * (-0.5 * dim * LOG_2PI - 0.5 * logdet - 0.5 * quad);
            for (int i = dim - 1; i >= 0; --i) {                 // a = inv(L)' z, in place
                double lsum = 0;
                for (int k = i + 1; k < dim; ++k) lsum += S[k * LS + i] * Zs[k * 64 + lane];
                Zs[i * 64 + lane] = (Zs[i * 64 + lane] - lsum) / S[i * LS + i];
            }
        } else {
            for (int i = 0; i < dim; ++i) Zs[i * 64 + lane] = 0.0;
        }
        Ws[lane] = wj;
        swc += wj;
        __syncthreads();
        for (int e = lane; e < dim * dim; e += 64) {             // a lane owns entries and loops over the columns
            int i = e % dim, j = e / dim;
            if (i < j) continue;
            double h = 0;
            for (int cc = 0; cc < 64; ++cc) h += Ws[cc] * Zs[i * 64 + cc] * Zs[j * 64 + cc];
            Hs[i * LS + j] += h;
        }
        __syncthreads();
    }
    swc = __shfl(wave_sum(swc), 0);
    for (int e = lane; e < dim * dim; e += 64) {                 // - (sum w) inv(D), inv(D) = inv(L)' inv(L)
        int i = e % dim, j = e / dim;
        if (i < j) continue;
        double s = 0;
        for (int k = i; k < dim; ++k) s += Li[k * LS + i] * Li[k * LS + j];
        Hs[i * LS + j] -= swc * s;
    }
    __syncthreads();
    const int ns = nslots[blockIdx.x], sb = slot_base[blockIdx.x];
    for (int slot0 = 0; slot0 < ns; slot0 += GRAD_SLOTS) {
        double g[GRAD_SLOTS];
#pragma unroll
        for (int s = 0; s < GRAD_SLOTS; ++s) g[s] = 0.0;
        for (int e = lane; e < dim * dim; e += 64) {
            int i = e % dim, j = e / dim;
            if (i >= j) grad_entry(blk, cov, rows, bd, th, i, j, (i == j ? 1.0 : 2.0) * Hs[i * LS + j], slot0, g);
        }
#pragma unroll
        for (int s = 0; s < GRAD_SLOTS; ++s) {
            const double r = wave_sum(g[s]);
            if (lane == 0 && slot0 + s < ns) gpart[(size_t)(sb + slot0 + s) * gridDim.y + blockIdx.y] = r;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) vpart[blockIdx.x * gridDim.y + blockIdx.y] = acc;
}

// ------------------------------------------------------------------ large blocks
// Xw[j + i ldw] = w_j X[j + i ldx], j < m, and a zero pad row m where m is odd (the transposed-A GEMM's operand contract)
__global__ __launch_bounds__(256) void k_grad_weigh_rows(const double* X, int ldx, int m, int cols, const double* w,
                                                         double* Xw, int ldw)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m + (m & 1)) return;
    const double wj = j < m ? (w ? w[j] : 1.0) : 0.0;
    for (int i = blockIdx.y; i < cols; i += gridDim.y)
        Xw[j + (size_t)i * ldw] = j < m ? wj * X[j + (size_t)i * ldx] : 0.0;
}

// S_ii -= sum w, i < n, and v[0] += sum w (-0.5 d log 2 pi - 0.5 logdet) - 0.5 trace(X' diag(w) X): the block's weighted value;
// trs[0] = trace(X' diag(w) X) - d sum w, the trace of the block's S (k_grad_scale_slot)
__global__ __launch_bounds__(256) void k_grad_sdiag(double* S, int lds, int d, int n, double sw, const double* logdet, double* v,
                                                    double* trs)
{
    __shared__ double sh[4];
    double tr = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double s = S[i + (size_t)i * lds];
        if (i < d) tr += s;
        S[i + (size_t)i * lds] = s - sw;
    }
    const double t = block_sum(tr, sh);
    if (threadIdx.x == 0) {
        v[0] += sw * (-0.5 * d * LOG_2PI - 0.5 * logdet[0]) - 0.5 * t;
        trs[0] = t - sw * d;
    }
}

// A slot whose dlog is the constant coef over the whole block -- the scale of sqexp / fexp, a gr term of a dense block -- has
// sum_ij D_ij H_ij dlog = coef trace(D H) = coef trace(S), D = L L' and H = inv(L)' S inv(L): the trace taken BEFORE the two
// solves.  The contraction of H with D arrives at the same number through the solves against the inverted diagonal blocks and
// loses kappa_2(L_kk) on the way (two to four digits of the scale's gradient at kappa_2(D) = 1e9 .. 1e12,
// tests/illcond_cases.py); the slot is overwritten with the closed form.
__global__ void k_grad_scale_slot(const double* trs, double coef, double* out) { out[0] = coef * trs[0]; }

// partials[workgroup * GRAD_SLOTS + s] = the workgroup's sum of mult H_ij D_ij dlog_{slot0 + s} over its 64 x 16 tile of the
// lower triangle (mult 1 on the diagonal, 2 below; the identity border i >= dim is skipped)
__global__ __launch_bounds__(256) void k_grad_reduce_large(const double* H, int ldh, int bidx, const CovBlock* blocks,
                                                           const int32_t* cov, int rows, const double* data, ThetaArg th,
                                                           int slot0, double* partials)
{
    __shared__ double sh[4];
    double g[GRAD_SLOTS];
#pragma unroll
    for (int s = 0; s < GRAD_SLOTS; ++s) g[s] = 0.0;
    const CovBlock blk = blocks[bidx];
    lower_tile_walk([&](int i, int j) {
        if (i >= blk.dim || j > i) return;
        const double h = H[i + (size_t)j * ldh];
        grad_entry(blk, cov, rows, data + blk.doff, th, i, j, (i == j ? 1.0 : 2.0) * h, slot0, g);
    });
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int s = 0; s < GRAD_SLOTS; ++s) {
        const double r = block_sum(g[s], sh);
        if (threadIdx.x == 0) partials[wg * GRAD_SLOTS + s] = r;
    }
}

// ------------------------------------------------------------------ host
// one gradient evaluation under way: what the per-block step of mvn_large_blocks needs
struct GradJob {
    ThetaArg th;
    const double* w = nullptr;   // device weights, null: 1 each
    double sw = 0;               // their sum
};

// slots of the dense blocks (small ones first, then large ones, each in block order) and the device tables k_small_grad reads
static int mvn_grad_setup(Ctx& c)
{
    Ctx::MvnGrad& g = c.grad;
    if (g.ready) return MCML_OK;
    const CovSpec& cs = c.cov;
    g.slot_base.assign(cs.B, -1);
    g.slot_count.assign(cs.B, 0);
    g.slot_par.clear();
    g.slot_scale.clear();
    std::vector<int> sbase, scount;
    for (int pass = 0; pass < 2; ++pass)
        for (int b = 0; b < cs.B; ++b) {
            const CovBlock& blk = cs.blocks[b];
            if (blk.all_gr || (blk.dim <= SMALL_BLOCK) != (pass == 0)) continue;
            g.slot_base[b] = (int)g.slot_par.size();
            for (int r = blk.r0; r < blk.r1; ++r)
                for (int q = 0; q < CovSpec::fn_npar(cs.c(r, 2)); ++q) {
                    g.slot_par.push_back(cs.c(r, 4) + q);
                    // cov_term_dlog: gr 2 / t everywhere the product is not 0; sqexp and fexp 1 / t0
                    g.slot_scale.push_back(q == 0 ? CovSpec::fn_scale_exp(cs.c(r, 2)) : 0);
                }
            g.slot_count[b] = (int)g.slot_par.size() - g.slot_base[b];
            if (pass == 0) { sbase.push_back(g.slot_base[b]); scount.push_back(g.slot_count[b]); }
        }
    g.n_small_slots = 0;
    for (int n : scount) g.n_small_slots += n;
    if (!sbase.empty()) {
        MCML_TRY(g.small_tab.ensure(sizeof(int) * 2 * sbase.size()));
        MCML_TRY(copy_h2d(g.small_tab.p, sbase.data(), sizeof(int) * sbase.size(), c.stream));
        MCML_TRY(copy_h2d(g.small_tab.as<int>() + sbase.size(), scount.data(), sizeof(int) * scount.size(), c.stream));
    }
    // results: [0] weighted value of the large blocks, [1] of the small ones, [2 .. 2 + npar] the diagonal rows' sums per
    // parameter and their value, then one double per slot, then the trace of the large block at hand (k_grad_sdiag)
    g.res_len = 4 + cs.npar + (int)g.slot_par.size();
    MCML_TRY(g.res.ensure(sizeof(double) * g.res_len));
    MCML_HIP(hipStreamSynchronize(c.stream));
    g.ready = true;
    return MCML_OK;
}

static double* grad_slot_out(Ctx& c, int slot) { return c.grad.res.d() + 3 + c.cov.npar + slot; }

// The gradient terms of large block b, right after its factorisation: W holds L (dp x dp, identity border past the block's
// dimension) and the m solved sample rows below it; c.chol.linv holds this factor's inverted diagonal blocks, which is why
// the step cannot wait for the next block.  W and linv are only read.  logdet: the block's log-determinant on the device
static int mvn_grad_large(Ctx& c, const GradJob& gj, int b, const DevMat& W, int dp, int m, const double* logdet)
{
    Ctx::MvnGrad& g = c.grad;
    const CovSpec& cs = c.cov;
    const CovBlock& blk = cs.blocks[b];
    const int d = blk.dim, ld = W.ld, dmax = round_up(c.maxdim_large, 16);
    if (g.S.rows < dmax) {               // first gradient call of the context
        MCML_TRY(g.S.alloc(dmax, dmax));
        MCML_TRY(g.T.alloc(dmax, dmax));
    }
    if (g.Xw.rows < m + 1 || g.Xw.cols < dmax) MCML_TRY(g.Xw.alloc(m + 1, dmax));
    const double* X = W.d() + dp;
    hipLaunchKernelGGL(k_grad_weigh_rows, dim3((m + 1 + 255) / 256, dp < 1024 ? dp : 1024), dim3(256), 0, c.stream, X, ld, m,
                       dp, gj.w, g.Xw.d(), g.Xw.ld);
    MCML_HIP(hipGetLastError());
    {
        EpiAxpby epi{g.S.d(), g.S.ld, 1.0, 0.0};
        MCML_TRY(launch_gemm_at(c.stream, dp, dp, m, X, ld, g.Xw.d(), g.Xw.ld, epi));
    }
    hipLaunchKernelGGL(k_grad_sdiag, dim3(1), dim3(256), 0, c.stream, g.S.d(), g.S.ld, d, dp, gj.sw, logdet, g.res.d(),
                       g.res.d() + g.res_len - 1);
    MCML_HIP(hipGetLastError());
    // H = inv(L)' S inv(L): T1 = inv(L)' S in place, H = inv(L)' T1' (S is symmetric)
    MCML_TRY(trsm_left_lower_trans(c, W.d(), ld, dp, g.S.d(), g.S.ld, dp));
    MCML_TRY(dev_transpose(c, g.S.d(), g.S.ld, dp, dp, g.T.d(), g.T.ld));
    MCML_TRY(trsm_left_lower_trans(c, W.d(), ld, dp, g.T.d(), g.T.ld, dp));
    const dim3 gr((d + 63) / 64, (d + 15) / 16);
    const int nwg = (int)(gr.x * gr.y);
    MCML_TRY(g.part.ensure(sizeof(double) * (size_t)nwg * GRAD_SLOTS));
    for (int slot0 = 0; slot0 < g.slot_count[b]; slot0 += GRAD_SLOTS) {
        const int ns = g.slot_count[b] - slot0 < GRAD_SLOTS ? g.slot_count[b] - slot0 : GRAD_SLOTS;
        hipLaunchKernelGGL(k_grad_reduce_large, gr, dim3(256), 0, c.stream, g.T.d(), g.T.ld, b, c.d_blocks.as<CovBlock>(),
                           c.d_cov.as<int32_t>(), cs.rows, c.d_data.d(), gj.th, slot0, g.part.d());
        hipLaunchKernelGGL(k_grad_sum, dim3(ns), dim3(256), 0, c.stream, g.part.d(), nwg, (size_t)1, (size_t)GRAD_SLOTS,
                           grad_slot_out(c, g.slot_base[b] + slot0));
        MCML_HIP(hipGetLastError());
    }
    for (int s = 0; s < g.slot_count[b]; ++s) {
        const int slot = g.slot_base[b] + s;
        if (!g.slot_scale[slot]) continue;
        hipLaunchKernelGGL(k_grad_scale_slot, dim3(1), dim3(1), 0, c.stream, g.res.d() + g.res_len - 1,
                           g.slot_scale[slot] / gj.th.v[g.slot_par[slot]], grad_slot_out(c, slot));
        MCML_HIP(hipGetLastError());
    }
    return MCML_OK;
}

// the diagonal rows and the small blocks, enqueued
static int mvn_grad_diag_small(Ctx& c, const GradJob& gj, const double* Us, int ldu, int m)
{
    Ctx::MvnGrad& g = c.grad;
    const CovSpec& cs = c.cov;
    const int Q = cs.N;
    const int32_t* dcov = c.d_cov.as<int32_t>();
    const CovBlock* dblk = c.d_blocks.as<CovBlock>();
    const int* drb = c.d_rowblock.as<int>();
    double* res = g.res.d();
    if (c.n_diag_rows > 0) {
        const int gx = (Q + 255) / 256;
        int gy = 65536 / gx; if (gy > m) gy = m; if (gy > 64) gy = 64; if (gy < 1) gy = 1;
        MCML_TRY(g.diag.ensure(sizeof(double) * (size_t)Q * (gy + 4)));
        double* dd = g.diag.d();
        double* dc = dd + Q;
        double* r = dc + Q;
        double* vrow = r + Q;
        double* qpart = vrow + Q;
        hipLaunchKernelGGL(k_diag_prep, dim3(gx), dim3(256), 0, c.stream, Q, drb, dblk, dcov, cs.rows, gj.th, dd, dc);
        hipLaunchKernelGGL(k_diag_gradq, dim3(gx, gy), dim3(256), 0, c.stream, Us, ldu, Q, m, gj.w, drb, qpart);
        hipLaunchKernelGGL(k_diag_gradr, dim3(gx), dim3(256), 0, c.stream, Q, gy, qpart, drb, dd, dc, gj.sw, r, vrow);
        hipLaunchKernelGGL(k_diag_gradp, dim3(cs.npar + 1), dim3(256), 0, c.stream, Q, cs.npar, drb, dblk, dcov, cs.rows,
                           gj.th, r, vrow, res + 2);
        MCML_HIP(hipGetLastError());
    }
    if (c.n_small > 0) {
        int ny = (m + 63) / 64; if (ny > 16) ny = 16;
        MCML_TRY(g.part_small.ensure(sizeof(double) * (size_t)(g.n_small_slots + c.n_small) * ny));
        double* gpart = g.part_small.d();
        double* vpart = gpart + (size_t)g.n_small_slots * ny;
        const int* tab = g.small_tab.as<int>();
        hipLaunchKernelGGL(k_small_grad, dim3((unsigned)c.n_small, ny), dim3(64), 0, c.stream, Us, ldu, m, gj.w,
                           c.small_ids.as<int>(), tab, tab + c.n_small, dblk, dcov, cs.rows, c.d_data.d(), gj.th, gpart, vpart,
                           c.errflag());
        if (g.n_small_slots)
            hipLaunchKernelGGL(k_grad_sum, dim3(g.n_small_slots), dim3(256), 0, c.stream, gpart, ny, (size_t)ny, (size_t)1,
                               grad_slot_out(c, 0));
        hipLaunchKernelGGL(k_grad_sum, dim3(1), dim3(256), 0, c.stream, vpart, c.n_small * ny, (size_t)0, (size_t)1, res + 1);
        MCML_HIP(hipGetLastError());
    }
    return MCML_OK;
}

}  // namespace mcml
