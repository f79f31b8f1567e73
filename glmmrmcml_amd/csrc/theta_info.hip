// theta_info.hip -- the GLS (expected) information of the covariance parameters on the device (a query: DESIGN.md 5.12),
//     I[r, s] = 1/2 tr(Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma),   Sigma = V^-1 + Z D(theta) Z',   d_r Sigma = Z (d_r D) Z',
// with V = diag(1 / w) exactly as the information query of the fixed effects forms it (info.hip, info_front).  In its Q x Q form,
// with D = L L', N = ZL' V ZL, M = I + N = R R' and L' (Z' Sigma^-1 Z) L = I - M^-1 = M^-1 N = B:
//     E_r = L^-1 (d_r D) L^-T,   G_r = B E_r,   I[r, s] = 1/2 sum_ij G_r[i, j] G_s[j, i],
// and for gaussian / identity (V^-1 = sigma^2 I, sigma a fitted parameter) the row of sigma from traces of the same matrices:
//     I[r, sigma] = (tr G_r - tr(B G_r)) / sigma,   I[sigma, sigma] = 2 (n - 2 tr B + tr(B B)) / sigma^2.
// (d_r D)_ij = D_ij * the sum of cov_term_dlog over the slots that read parameter r (cov_dentry, cov_entry.h).
//
// Dense operator.  After info_front (x.M = R, its inverted diagonal blocks in c.chol.linv):
//   N, full, by the MFMA GEMM on the ZLTW build_M_dense left; B = M^-1 N by trsm_left_lower + trsm_left_lower_trans.  N is built
//   for this rather than B = I - M^-1: that difference cancels where the data are weak against the prior (N small);
//   k_ti_linv            the inverted 128 x 128 diagonal blocks of the resident L into c.chol.linv, where the blocked solves
//                        expect them (every factorisation overwrites them, as this does);
//   per parameter r      k_ti_build_dD (the dense block-diagonal d_r D), trsm_left_lower with L, a transposition, trsm_left_lower
//                        again (E_r), G_r = B E_r by the MFMA GEMM;
//   k_ti_contract        for every pair r >= s of the R (+ 1: B itself, for the sigma row) matrices, the 32 x 32 tile (I, J) of one
//                        against the tile (J, I) of the other through LDS -> one partial per (pair, tile);
//   k_ti_sum             the tiles' partials in a fixed order, and the traces.
// Component operator (theta_info_component_ok: the sparse operator runs, no component above TI_COMP_MAX_VARS variables, every
// covariance block inside one component): B, E_r and with them everything above are block diagonal by component.
//   k_ti_comp            one workgroup per component, four 64 x 64 matrices in LDS: N_c from the rows of ZL' and ZL, B_c = M_c^-1 N_c
//                        by the two substitutions with R_c, L_c^-1, T = B_c L_c^-1, A_c = L_c^-T T = (Z' Sigma^-1 Z)_c, A2_c = T' T; per parameter r that a block of the
//                        component reads, K_r = A_c (d_r D_c) A_c, and for s <= r the sum of K_r o (d_s D_c), d_s D_c rebuilt
//                        entry by entry from the spec: tr(G_r G_s) = tr(A d_r D A d_s D).  tr G_r = sum A o d_r D,
//                        tr(B G_r) = sum A2 o d_r D;
//   k_ti_comp_sum        adds the components in ascending order.
// k_ti_final writes the matrix (r >= s, mirrored) and the two flags behind it; query_download ends the call.  Everything runs on
// c.stream, there is no floating-point atomic and every sum has a fixed order: two calls give the same bits.  Neither y nor the
// samples are read, no collective is issued, and nothing a sampler, a fit, mvn_ll or the information query reads is changed.
// The call is two halves, declared in entry.h for the small-sample query (small_sample.hip), which needs I_theta with more:
// theta_info_begin (the operator, the kernels' theta, the blocks' parameter masks) and theta_info_compute (every launch above).
#include "entry.h"
#include "component.h"
#include "cov_block.h"
#include "dgemm_mfma.h"
#include "glm.h"
#include "reduce.h"
#include "vecops.h"
#include <algorithm>
#include <cmath>

namespace mcml {

constexpr int TI_LS = TI_COMP_MAX_VARS + 1;       // row stride of its LDS matrices
constexpr size_t TI_COMP_LDS = sizeof(double) * 4 * TI_COMP_MAX_VARS * TI_LS;   // 130 KB of the 160 KB: one workgroup per CU
constexpr int TI_TILE = 32;

// index of the pair (r, s), r >= s
__host__ __device__ __forceinline__ int ti_pair(int r, int s) { return r * (r + 1) / 2 + s; }

// where the reduced sums lie, R parameters, np = R (R + 1) / 2: [pair(r, s)] tr(G_r G_s) | np + r: tr G_r | np + R + r: tr(B G_r)
// | np + 2 R: tr B | np + 2 R + 1: tr(B B)
__host__ __device__ __forceinline__ int ti_red_len(int R) { return R * (R + 1) / 2 + 2 * R + 2; }

// ------------------------------------------------------------------ dense operator
// Linv[i + 128 j] of panel blockIdx.x = the inverse of L's diagonal block there, lower triangle (the layout k_potrf_leaf
// leaves); thread j its column j by forward substitution, reading back what it wrote itself
__global__ __launch_bounds__(CHOL_NB) void k_ti_linv(const double* L, int ldl, int Q, double* Linv)
{
    const int k0 = blockIdx.x * CHOL_NB, nb = Q - k0 < CHOL_NB ? Q - k0 : CHOL_NB, j = threadIdx.x;
    if (j >= nb) return;
    const double* A = L + k0 + (size_t)k0 * ldl;
    double* X = Linv + (size_t)blockIdx.x * CHOL_NB * CHOL_NB + (size_t)j * CHOL_NB;
    for (int i = j; i < nb; ++i) {
        double s = (i == j) ? 1.0 : 0.0;
        for (int k = j; k < i; ++k) s -= A[i + (size_t)k * ldl] * X[k];
        X[i] = s / A[i + (size_t)i * ldl];
    }
}

// block b's part of d_par D into the Q x Q matrix E (zero before): both triangles.  A dense block: the 64 x 16 tiles of its lower
// triangle (lower_tile_walk, cov_block.h); an all-gr block: its diagonal, 256 rows per workgroup
__global__ __launch_bounds__(256) void k_ti_build_dD(double* E, int lde, int bidx, const CovBlock* blocks, const int32_t* cov,
                                                     int rows, const double* data, ThetaArg th, int par)
{
    const CovBlock blk = blocks[bidx];
    double* A = E + blk.matstart + (size_t)blk.matstart * lde;
    const double* bd = data + blk.doff;
    if (blk.all_gr) {
        const int k = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (k < blk.dim) A[k + (size_t)k * lde] = cov_dentry(blk, cov, rows, bd, th, k, k, par);
        return;
    }
    lower_tile_walk([&](int i, int j) {
        if (i >= blk.dim || j > i) return;
        const double v = cov_dentry(blk, cov, rows, bd, th, i, j, par);
        A[i + (size_t)j * lde] = v;
        A[j + (size_t)i * lde] = v;
    });
}

// part[pair * gridDim.x + tile] = sum over the 32 x 32 tile (I, J) of G_r[i, j] G_s[j, i], pair = (r, s), r >= s, of the nm
// matrices G[0 .. nm) (Q x Q, leading dimension ld): tile (I, J) of G_r and tile (J, I) of G_s through LDS, both read along columns
__global__ __launch_bounds__(256) void k_ti_contract(const double* const* G, int ld, int Q, int nt, double* part)
{
    __shared__ double a[TI_TILE][TI_TILE + 1], b[TI_TILE][TI_TILE + 1];
    __shared__ double sh[4];
    int r = 0;
    while (ti_pair(r + 1, 0) <= (int)blockIdx.y) ++r;
    const int s = blockIdx.y - ti_pair(r, 0);
    const double *Gr = G[r], *Gs = G[s];
    const int I = blockIdx.x % nt, J = blockIdx.x / nt, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int jj = ty + 8 * u;
        const int gi = I * TI_TILE + tx, gj = J * TI_TILE + jj, hi = J * TI_TILE + tx, hj = I * TI_TILE + jj;
        a[jj][tx] = (gi < Q && gj < Q) ? Gr[gi + (size_t)gj * ld] : 0.0;
        b[jj][tx] = (hi < Q && hj < Q) ? Gs[hi + (size_t)hj * ld] : 0.0;
    }
    __syncthreads();
    double acc = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int jj = ty + 8 * u;
        acc += a[jj][tx] * b[tx][jj];
    }
    const double v = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
}

// workgroup x < npairs: the pair's tile partials, thread t the tiles t, t + 256, ... in turn, then block_sum; workgroup
// npairs + m: the trace of G[m].  nm = R: the R matrices G_r; nm = R + 1: B behind them.  -> red in the layout of ti_red_len
__global__ __launch_bounds__(256) void k_ti_sum(const double* part, int ntile, const double* const* G, int ld, int Q, int R, int nm,
                                                double* red)
{
    __shared__ double sh[4];
    const int npairs = ti_pair(nm, 0), np = ti_pair(R, 0), x = blockIdx.x;
    double acc = 0;
    int dst;
    if (x < npairs) {
        int r = 0;
        while (ti_pair(r + 1, 0) <= x) ++r;
        const int s = x - ti_pair(r, 0);
        for (int t = threadIdx.x; t < ntile; t += 256) acc += part[(size_t)x * ntile + t];
        dst = r < R ? x : (s < R ? np + R + s : np + 2 * R + 1);
    } else {
        const int m = x - npairs;
        const double* A = G[m];
        for (int i = threadIdx.x; i < Q; i += 256) acc += A[i + (size_t)i * ld];
        dst = m < R ? np + m : np + 2 * R;
    }
    const double v = block_sum(acc, sh);
    if (threadIdx.x == 0) red[dst] = v;
}

// ------------------------------------------------------------------ the result
// out (nout x nout, nout = R + sigma_row) from the reduced sums, r >= s and mirrored; the two flags of the call behind the matrix,
// as k_info_gram_final leaves them
__global__ __launch_bounds__(256) void k_ti_final(const double* red, int R, int sigma_row, double sigma, double n, const int* errflag,
                                                  const int* bad, double* out)
{
    const int nout = R + sigma_row, np = ti_pair(R, 0), t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0) { out[(size_t)nout * nout] = (double)*errflag; out[(size_t)nout * nout + 1] = (double)*bad; }
    if (t >= nout * nout) return;
    const int a = t % nout, b = t / nout;
    if (a < b) return;
    double val;
    if (a < R) val = 0.5 * red[ti_pair(a, b)];
    else if (b < R) val = (red[np + b] - red[np + R + b]) / sigma;
    else val = 2.0 * (n - 2.0 * red[np + 2 * R] + red[np + 2 * R + 1]) / (sigma * sigma);
    out[a + (size_t)b * nout] = val;
    out[b + (size_t)a * nout] = val;
}

// ------------------------------------------------------------------ component operator
// C (nv x nv) = X Y over the workgroup, entries dealt e = tid, tid + 256, ...; k runs over [klo(i, j), khi(i, j))
template <class FA, class FB, class FLO, class FHI>
__device__ __forceinline__ void ti_matmul(int nv, double* C, FA xa, FB yb, FLO klo, FHI khi)
{
    for (int e = threadIdx.x; e < nv * nv; e += 256) {
        const int i = e % nv, j = e / nv;
        double s = 0;
        for (int k = klo(i, j); k < khi(i, j); ++k) s += xa(i, k) * yb(k, j);
        C[i * TI_LS + j] = s;
    }
}

// One workgroup per component (file comment).  cpart[c * ti_red_len(R) + x]: the component's share of every reduced sum.
// blk_of_var: the covariance block of every variable; blk_mask: bit p set where the block reads parameter p; loc: the local
// index of every variable in its component; csr_* / ell_*: the rows of ZL' and of ZL (SparseZL), v the reciprocal weights
__global__ __launch_bounds__(256) void k_ti_comp(const int* var_ptr, const int* vars, const double* fac, const int* fac_ptr,
                                                 const double* L, int ldl, const int* blk_of_var, const unsigned* blk_mask,
                                                 const int* loc, const int* csr_ptr, const int* csr_i, const double* csr_val,
                                                 const int* ell_col, const double* ell_val, int n, int W, const double* v,
                                                 const CovBlock* blocks, const int32_t* cov, int rows, const double* data,
                                                 ThetaArg th, int R, double* cpart)
{
    extern __shared__ double lds[];
    double *S0 = lds, *S1 = S0 + TI_COMP_MAX_VARS * TI_LS, *S2 = S1 + TI_COMP_MAX_VARS * TI_LS, *S3 = S2 + TI_COMP_MAX_VARS * TI_LS;
    __shared__ double sh[4];
    __shared__ int gv[TI_COMP_MAX_VARS], gb[TI_COMP_MAX_VARS];
    __shared__ unsigned cmask;
    const int c = blockIdx.x, v0 = var_ptr[c], nv = var_ptr[c + 1] - v0, tid = threadIdx.x;
    const int np = ti_pair(R, 0);
    double* out = cpart + (size_t)c * ti_red_len(R);
    if (tid < nv) { gv[tid] = vars[v0 + tid]; gb[tid] = blk_of_var[gv[tid]]; }
    __syncthreads();
    if (tid == 0) {
        unsigned m = 0;
        for (int i = 0; i < nv; ++i) m |= blk_mask[gb[i]];
        cmask = m;
    }
    // S0 <- R_c, S1 <- L_c (lower triangles), S2, S3 <- 0
    const double* Rc = fac + fac_ptr[c];
    for (int e = tid; e < nv * nv; e += 256) {
        const int i = e % nv, j = e / nv;
        S0[i * TI_LS + j] = i >= j ? Rc[i + (size_t)j * nv] : 0.0;
        S1[i * TI_LS + j] = i >= j ? L[gv[i] + (size_t)gv[j] * ldl] : 0.0;
        S2[i * TI_LS + j] = 0.0;
        S3[i * TI_LS + j] = 0.0;
    }
    __syncthreads();
    // S2 <- N_c = ZL_c' V ZL_c, thread a its row a: the entries of row gv[a] of ZL', observations ascending, each against the ELL
    // row of its observation (the padding holds column 0 and value 0; a column of another component is never met)
    if (tid < nv) {
        const int q = gv[tid];
        for (int t = csr_ptr[q]; t < csr_ptr[q + 1]; ++t) {
            const int i = csr_i[t];
            const double w = csr_val[t] * v[i];
            for (int k = 0; k < W; ++k) {
                const int col = ell_col[i + (size_t)k * n], l = loc[col];
                if (l < nv && gv[l] == col) S2[tid * TI_LS + l] += w * ell_val[i + (size_t)k * n];
            }
        }
    }
    __syncthreads();
    // S2 <- B = M_c^-1 N_c: R_c y = N_c[:, j], then R_c' b = y, in place, threads 0 .. nv - 1 a column each;
    // S3 <- Li = L_c^-1, threads 64 .. 64 + nv - 1 a column each
    if (tid < nv) {
        const int j = tid;
        for (int i = 0; i < nv; ++i) {
            double s = S2[i * TI_LS + j];
            for (int k = 0; k < i; ++k) s -= S0[i * TI_LS + k] * S2[k * TI_LS + j];
            S2[i * TI_LS + j] = s / S0[i * TI_LS + i];
        }
        for (int i = nv - 1; i >= 0; --i) {
            double s = S2[i * TI_LS + j];
            for (int k = i + 1; k < nv; ++k) s -= S0[k * TI_LS + i] * S2[k * TI_LS + j];
            S2[i * TI_LS + j] = s / S0[i * TI_LS + i];
        }
    } else if (tid >= 64 && tid - 64 < nv) {
        lower_inverse_column(S1, S3, TI_LS, nv, tid - 64);
    }
    __syncthreads();
    // tr B and tr(B B)
    double trb = 0, bb = 0;
    for (int e = tid; e < nv * nv; e += 256) {
        const int i = e % nv, j = e / nv;
        if (i == j) trb += S2[i * TI_LS + i];
        bb += S2[i * TI_LS + j] * S2[j * TI_LS + i];
    }
    trb = block_sum(trb, sh);
    bb = block_sum(bb, sh);
    if (tid == 0) { out[np + 2 * R] = trb; out[np + 2 * R + 1] = bb; }
    // S0 <- T = B Li
    ti_matmul(nv, S0, [&](int i, int k) { return S2[i * TI_LS + k]; }, [&](int k, int j) { return S3[k * TI_LS + j]; },
              [](int, int j) { return j; }, [&](int, int) { return nv; });
    __syncthreads();
    // S1 <- A = Li' T, S2 <- A2 = T' T
    ti_matmul(nv, S1, [&](int i, int k) { return S3[k * TI_LS + i]; }, [&](int k, int j) { return S0[k * TI_LS + j]; },
              [](int i, int) { return i; }, [&](int, int) { return nv; });
    ti_matmul(nv, S2, [&](int i, int k) { return S0[k * TI_LS + i]; }, [&](int k, int j) { return S0[k * TI_LS + j]; },
              [](int, int) { return 0; }, [&](int, int) { return nv; });
    __syncthreads();
    const unsigned mask = cmask;
    // (d_p D_c)[i, j] of the component's local entry, 0 across blocks and where the block does not read p
    auto dentry = [&](int i, int j, int p) {
        const int b = gb[i];
        if (b != gb[j] || !((blk_mask[b] >> p) & 1u)) return 0.0;
        const CovBlock blk = blocks[b];
        return cov_dentry(blk, cov, rows, data + blk.doff, th, gv[i] - blk.matstart, gv[j] - blk.matstart, p);
    };
    for (int r = 0; r < R; ++r) {
        if (!((mask >> r) & 1u)) {                      // no block of the component reads r: the whole row is 0
            if (tid <= r) out[ti_pair(r, tid)] = 0.0;
            if (tid == 0) { out[np + r] = 0.0; out[np + R + r] = 0.0; }
            continue;
        }
        // S0 <- d_r D_c; tr G_r = sum A o d_r D, tr(B G_r) = sum A2 o d_r D on the way
        double tg = 0, tbg = 0;
        for (int e = tid; e < nv * nv; e += 256) {
            const int i = e % nv, j = e / nv;
            const double d = dentry(i, j, r);
            S0[i * TI_LS + j] = d;
            tg += S1[i * TI_LS + j] * d;
            tbg += S2[i * TI_LS + j] * d;
        }
        tg = block_sum(tg, sh);
        tbg = block_sum(tbg, sh);
        if (tid == 0) { out[np + r] = tg; out[np + R + r] = tbg; }
        // S3 <- A d_r D, S0 <- K_r = (A d_r D) A
        ti_matmul(nv, S3, [&](int i, int k) { return S1[i * TI_LS + k]; }, [&](int k, int j) { return S0[k * TI_LS + j]; },
                  [](int, int) { return 0; }, [&](int, int) { return nv; });
        __syncthreads();
        ti_matmul(nv, S0, [&](int i, int k) { return S3[i * TI_LS + k]; }, [&](int k, int j) { return S1[k * TI_LS + j]; },
                  [](int, int) { return 0; }, [&](int, int) { return nv; });
        __syncthreads();
        for (int s = 0; s <= r; ++s) {
            double acc = 0;
            if ((mask >> s) & 1u)
                for (int e = tid; e < nv * nv; e += 256) {
                    const int i = e % nv, j = e / nv;
                    acc += S0[i * TI_LS + j] * dentry(i, j, s);
                }
            acc = block_sum(acc, sh);
            if (tid == 0) out[ti_pair(r, s)] = acc;
        }
    }
}

// red[x] = sum_c cpart[c * len + x], c ascending
__global__ __launch_bounds__(256) void k_ti_comp_sum(const double* cpart, int ncomp, int len, double* red)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= len) return;
    double s = 0;
    for (int c = 0; c < ncomp; ++c) s += cpart[(size_t)c * len + x];
    red[x] = s;
}

// ------------------------------------------------------------------ host
// the component operator applies: the sparse operator runs (comp_operator_ready), no component has more than TI_COMP_MAX_VARS
// variables and every covariance block lies inside one component -- a variable with no observation is a component of its own and
// can split a block
bool theta_info_component_ok(const Ctx& c)
{
    if (!comp_operator_ready(c)) return false;
    const ComponentPlan& p = c.cp.plan;
    if (p.max_vars > TI_COMP_MAX_VARS || (int)p.comp_of_var.size() != c.cov.N) return false;
    for (const CovBlock& blk : c.cov.blocks)
        for (int k = 1; k < blk.dim; ++k)
            if (p.comp_of_var[blk.matstart + k] != p.comp_of_var[blk.matstart]) return false;
    return true;
}

// the Q x Q workspace of the dense operator: every column the GEMM's K padding touches is allocated, and all of it is zero
static int ti_alloc_zero(Ctx& c, DevMat& A, int Q)
{
    MCML_TRY(A.alloc(Q, Q, 32));
    MCML_HIP(hipMemsetAsync(A.d(), 0, sizeof(double) * (size_t)A.ld * A.cols_alloc, c.stream));
    return MCML_OK;
}

static int theta_info_dense(Ctx& c, const ThetaArg& th, int R, int sigma_row, const std::vector<unsigned>& mask, bool sparse_ctx)
{
    InfoState& x = c.info;
    ThetaInfoState& t = c.tinfo;
    const CovSpec& cs = c.cov;
    const int n = c.n, Q = c.Q, nm = R + sigma_row;
    long long launches = 0;
    if ((int)t.G.size() < R) t.G.resize(R);
    MCML_TRY(ti_alloc_zero(c, t.B, Q));
    MCML_TRY(ti_alloc_zero(c, t.T, Q));
    for (int r = 0; r < R; ++r) MCML_TRY(ti_alloc_zero(c, t.G[r], Q));
    // ---- N = ZL' V ZL in full, B = M^-1 N
    {
        const EpiAxpby epi{t.B.d(), t.B.ld, 1.0, 0.0};
        MCML_TRY(launch_gemm<false>(c.stream, Q, Q, n, x.ZLTW.d(), x.ZLTW.ld, c.ZL.d(), c.ZL.ld, epi));
    }
    MCML_TRY(trsm_left_lower(c, x.M.d(), x.M.ld, Q, t.B.d(), t.B.ld, Q));
    MCML_TRY(trsm_left_lower_trans(c, x.M.d(), x.M.ld, Q, t.B.d(), t.B.ld, Q));
    // ---- the inverted diagonal blocks of L where the blocked solves read them
    MCML_TRY(leaf_prepare(c, Q, 1));
    hipLaunchKernelGGL(k_ti_linv, dim3((Q + CHOL_NB - 1) / CHOL_NB), dim3(CHOL_NB), 0, c.stream, c.L.d(), c.L.ld, Q, c.chol.linv.d());
    MCML_HIP(hipGetLastError());
    ++launches;
    // ---- G_r = B L^-1 (d_r D) L^-T
    for (int r = 0; r < R; ++r) {
        MCML_TRY(ti_alloc_zero(c, t.E, Q));
        for (int b = 0; b < cs.B; ++b) {
            if (!((mask[b] >> r) & 1u)) continue;
            const int d = cs.blocks[b].dim;
            const dim3 g = cs.blocks[b].all_gr ? dim3((d + 255) / 256, 1) : dim3((d + 63) / 64, (d + 15) / 16);
            hipLaunchKernelGGL(k_ti_build_dD, g, dim3(256), 0, c.stream, t.E.d(), t.E.ld, b, c.d_blocks.as<CovBlock>(),
                               c.d_cov.as<int32_t>(), cs.rows, c.d_data.d(), th, r);
            ++launches;
        }
        MCML_HIP(hipGetLastError());
        MCML_TRY(trsm_left_lower(c, c.L.d(), c.L.ld, Q, t.E.d(), t.E.ld, Q));
        MCML_TRY(dev_transpose(c, t.E.d(), t.E.ld, Q, Q, t.T.d(), t.T.ld));
        MCML_TRY(trsm_left_lower(c, c.L.d(), c.L.ld, Q, t.T.d(), t.T.ld, Q));
        const EpiAxpby epi{t.G[r].d(), t.G[r].ld, 1.0, 0.0};
        MCML_TRY(launch_gemm<false>(c.stream, Q, Q, Q, t.B.d(), t.B.ld, t.T.d(), t.T.ld, epi));
    }
    // ---- the contraction, two stages
    std::vector<const double*> ptr(nm);
    for (int r = 0; r < R; ++r) ptr[r] = t.G[r].d();
    if (sigma_row) ptr[R] = t.B.d();
    MCML_TRY(t.gptr.ensure(sizeof(double*) * (size_t)nm));
    MCML_TRY(copy_h2d(t.gptr.p, ptr.data(), sizeof(double*) * (size_t)nm, c.stream));
    MCML_HIP(hipStreamSynchronize(c.stream));                       // ptr leaves scope
    const int nt = (Q + TI_TILE - 1) / TI_TILE, ntile = nt * nt, npairs = ti_pair(nm, 0);
    MCML_TRY(t.part.ensure(sizeof(double) * (size_t)npairs * ntile));
    hipLaunchKernelGGL(k_ti_contract, dim3(ntile, npairs), dim3(256), 0, c.stream, t.gptr.as<const double*>(), t.B.ld, Q, nt,
                       t.part.d());
    MCML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ti_sum, dim3(npairs + nm), dim3(256), 0, c.stream, t.part.d(), ntile, t.gptr.as<const double*>(), t.B.ld, Q,
                       R, nm, t.tr.d());
    MCML_HIP(hipGetLastError());
    launches += 2;
    size_t bytes = t.B.buf.bytes + t.E.buf.bytes + t.T.buf.bytes + x.M.buf.bytes + x.ZLTW.buf.bytes;
    for (int r = 0; r < R; ++r) bytes += t.G[r].buf.bytes;
    if (sparse_ctx) bytes += c.ZL.buf.bytes + c.ZLT.buf.bytes;
    t.plan[4] = launches; t.plan[5] = (long long)bytes;
    return MCML_OK;
}

static int theta_info_comp(Ctx& c, const ThetaArg& th, int R, const std::vector<unsigned>& mask)
{
    InfoState& x = c.info;
    ThetaInfoState& t = c.tinfo;
    const CovSpec& cs = c.cov;
    const ComponentPlan& p = c.cp.plan;
    const int Q = c.Q, len = ti_red_len(R);
    std::vector<int> bov(2 * (size_t)Q + cs.B);                    // the block of every variable | its local index | the blocks' masks
    for (int b = 0; b < cs.B; ++b) {
        for (int k = 0; k < cs.blocks[b].dim; ++k) bov[cs.blocks[b].matstart + k] = b;
        bov[2 * (size_t)Q + b] = (int)mask[b];
    }
    std::copy(p.local_of_var.begin(), p.local_of_var.end(), bov.begin() + Q);
    MCML_TRY(t.blk_of_var.ensure(sizeof(int) * bov.size()));
    MCML_TRY(copy_h2d(t.blk_of_var.p, bov.data(), sizeof(int) * bov.size(), c.stream));
    MCML_HIP(hipStreamSynchronize(c.stream));                       // bov leaves scope
    MCML_TRY(t.part.ensure(sizeof(double) * (size_t)p.ncomp * len));
    MCML_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&k_ti_comp), (int)TI_COMP_LDS));
    hipLaunchKernelGGL(k_ti_comp, dim3(p.ncomp), dim3(256), TI_COMP_LDS, c.stream, c.cp.var_ptr.as<int>(), c.cp.vars.as<int>(),
                       x.f.fac.d(), x.f.fac_ptr.as<int>(), c.L.d(), c.L.ld, t.blk_of_var.as<int>(),
                       t.blk_of_var.as<unsigned>() + 2 * (size_t)Q, t.blk_of_var.as<int>() + Q, c.sp.csr_ptr.as<int>(),
                       c.sp.csr_i.as<int>(), c.sp.csr_val.d(), c.sp.ell_col.as<int>(), c.sp.ell_val.d(), c.n, c.sp.W, x.v.d(),
                       c.d_blocks.as<CovBlock>(), c.d_cov.as<int32_t>(), cs.rows, c.d_data.d(), th,
                       R, t.part.d());
    MCML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ti_comp_sum, dim3((len + 255) / 256), dim3(256), 0, c.stream, t.part.d(), p.ncomp, len, t.tr.d());
    MCML_HIP(hipGetLastError());
    t.plan[4] = 2; t.plan[5] = 0;
    return MCML_OK;
}

int theta_info_begin(Ctx& c, const char* who, const double* theta, int op, ThetaInfoCall& k)
{
    const int R = c.cov.npar;
    k.R = R;
    k.sigma_row = c.flink == 7 ? 1 : 0;                             // gaussian / identity
    k.no = R + k.sigma_row;
    ThetaInfoState& t = c.tinfo;
    const ComponentPlan& p = c.cp.plan;
    const bool comp_ok = theta_info_component_ok(c);
    const long long plan0[8] = {op, 0, p.ncomp, p.max_vars, 0, 0, R, k.no};
    std::copy(plan0, plan0 + 8, t.plan);
    if (op == 2 && !comp_ok) {
        set_error("%s: the component operator needs the sparse ZL operator, no component above %d variables and "
                  "every covariance block inside one component", who, TI_COMP_MAX_VARS);
        return MCML_EUNSUPPORTED;
    }
    k.comp = op != 1 && comp_ok;
    MCML_TRY(theta_arg(theta, R, k.th));
    const CovSpec& cs = c.cov;
    k.mask.assign(cs.B, 0u);                                        // bit p: block b has a slot that reads parameter p
    for (int b = 0; b < cs.B; ++b)
        for (int r = cs.blocks[b].r0; r < cs.blocks[b].r1; ++r)
            for (int q = 0; q < CovSpec::fn_npar(cs.c(r, 2)); ++q) k.mask[b] |= 1u << (cs.c(r, 4) + q);
    k.sparse_ctx = c.sp.active;
    return MCML_OK;
}

int theta_info_compute(Ctx& c, const ThetaInfoCall& k, double var_par)
{
    ThetaInfoState& t = c.tinfo;
    const int R = k.R, no = k.no;
    MCML_TRY(t.tr.ensure(sizeof(double) * (size_t)ti_red_len(R)));
    MCML_HIP(hipMemsetAsync(t.tr.d(), 0, sizeof(double) * (size_t)ti_red_len(R), c.stream));
    if (k.comp) MCML_TRY(theta_info_comp(c, k.th, R, k.mask));
    else MCML_TRY(theta_info_dense(c, k.th, R, k.sigma_row, k.mask, k.sparse_ctx));
    t.plan[1] = k.comp ? 1 : 0;
    MCML_TRY(t.res.ensure(sizeof(double) * ((size_t)no * no + 2)));
    hipLaunchKernelGGL(k_ti_final, dim3((no * no + 255) / 256), dim3(256), 0, c.stream, t.tr.d(), R, k.sigma_row, var_par, (double)c.n,
                       c.errflag(), c.info.bad.as<int>(), t.res.d());
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

int theta_info(Ctx& c, const double* beta, double var_par, const double* theta, int op, double* out, int ldo, int* nout)
{
    const int n = c.n, P = c.P, R = c.cov.npar;
    MCML_REQUIRE(n > 0 && P > 0 && R > 0, "theta_information: the context has no model / covariance");
    MCML_REQUIRE(beta && theta && out && nout, "theta_information: null argument");
    MCML_REQUIRE(op >= 0 && op <= 2, "theta_information: op must be 0 (auto), 1 (dense) or 2 (component)");
    MCML_REQUIRE(c.have_L && !c.l_foreign, "theta_information: the context holds no L made from theta");
    MCML_REQUIRE(std::isfinite(var_par), "theta_information: var_par is not finite");
    const int no = R + (c.flink == 7 ? 1 : 0);
    MCML_REQUIRE(ldo >= no, "theta_information: ldo %d too small for %d rows", ldo, no);
    MCML_REQUIRE(c.flink != 7 || var_par != 0.0, "theta_information: sigma is 0");
    ThetaInfoCall k;
    MCML_TRY(theta_info_begin(c, "theta_information", theta, op, k));

    InfoDenseScope dense(c);
    MCML_TRY(info_front(c, beta, var_par, k.comp, false, dense));
    MCML_TRY(theta_info_compute(c, k, var_par));

    // ---- the one download
    std::vector<double> h;
    MCML_TRY(query_download(c, c.tinfo.res, no, 0, "theta_information", "a weight dhdmu(x' beta) * scale, or its reciprocal,", h));
    copy_columns(out, ldo, h.data(), no, no);
    *nout = no;
    return MCML_OK;
}

}  // namespace mcml
