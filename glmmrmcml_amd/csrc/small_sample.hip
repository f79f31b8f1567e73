// small_sample.hip -- the ingredients of the Kenward-Roger / Satterthwaite small-sample corrections of the fixed effects on the
// device (a query: DESIGN.md 5.13).  With Sigma = V^-1 + Z D(theta) Z' as info.hip and theta_info.hip form it, the P x P matrices
//     P_r  = -X' Sigma^-1 d_r Sigma Sigma^-1 X,
//     Q_rs =  X' Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma Sigma^-1 X,
//     R_rs =  X' Sigma^-1 d2_rs Sigma Sigma^-1 X
// beside I_beta = X' Sigma^-1 X (info.hip) and I_theta (theta_info.hip), which this query returns to the bit; the caller layer
// does the rest by P x P algebra (model.py small_sample).  In the Q x Q form, D = L L', N = ZL' V ZL, M = I + N = R R',
// b = ZL' V X:
//     c = M^-1 b = R^-T S (S = R^-1 b is what the information query leaves; no subtraction),   d = L^-T c = Z' Sigma^-1 X,
//     U_r = (d_r D) d,   V_rs = (d2_rs D) d,   Y_r = (Z' Sigma^-1 Z) U_r = L^-T M^-1 N L^-1 U_r   (N itself, not M - I),
//     P_r = -d' U_r,   Q_rs = U_r' Y_s,   R_rs = d' V_rs,
// and for gaussian / identity (sigma last, d_sigma Sigma = 2 sigma I): A = Sigma^-1 X = V (X - ZL c), c2 = M^-1 ZL' V A,
// A2 = Sigma^-1 A = V (A - ZL c2), d2 = L^-T c2,
//     P_sigma = -2 sigma A' A,   Q_sigma,sigma = 4 sigma^2 A' A2,   Q_r,sigma = 2 sigma U_r' d2,   R_sigma,sigma = 2 A' A,   R_r,sigma = 0.
//
// One call: info_front with the right-hand sides, info_solve_gram (I_beta), c (and A, c2, A2) while the factor of M is the one
// the solves read, theta_info_compute (I_theta), then
//   k_ss_apply       U_r and V_rs matrix-free: a workgroup per (block, 64 rows, parameter or pair), the entries of d_r D / d2_rs D
//                    from one cov_walk each (cov_dentry, cov_d2entry), d's rows staged in LDS 64 at a time, SS_PC columns a pass,
//                    four j-lanes a row summed in a fixed order; an all-gr block elementwise
//   Y_r              dense operator: trsm_left_lower with L, the MFMA GEMM with the resident B = M^-1 N (c.tinfo.B),
//                    trsm_left_lower_trans with L, all R P columns at once, after k_ti_linv; component operator: k_ss_comp_y
//   k_ss_gram        every P_r, Q_rs, R_rs and sigma entry: a cross-Gram per job, partials per (job, entry, 2048 rows) in
//                    block_sum's order, k_ss_gram_final sums them ascending, scales, mirrors (P_r, Q_rr, R_rs: a >= b) or
//                    transposes (Q_sr = Q_rs'); R_rs only where a block reads both parameters, else 0
// and one download (query_download).  Component operator (theta_info_component_ok): k_ss_comp_back (c = R_c^-T S_c,
// d = L_c^-T c) and k_ss_comp_y, a workgroup per component with R_c, L_c^-1 and N_c in LDS and a thread per column; k_ss_ell
// for ZL c; comp_rhs_csr_launch and comp_solve_launch for c2.  Nothing of size Q x Q or Q x n is built by this file, no
// floating-point atomic, every sum in a fixed order: two calls give the same bits.  y and the samples are not read; no collective.
#include "entry.h"
#include "component.h"
#include "cov_block.h"
#include "dgemm_mfma.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

namespace mcml {

constexpr int SS_ROWS = 64;                       // rows of a block a workgroup of k_ss_apply takes, and rows of d staged at a time
constexpr int SS_JL = 4;                          // threads a row: j = jl, jl + 4, ... of the staged rows
constexpr int SS_PC = 8;                          // columns of d a pass
constexpr int SS_CHUNK = 2048;                    // rows a partial of k_ss_gram
constexpr int SS_LS = TI_COMP_MAX_VARS + 1;       // row stride of the component kernels' LDS matrices
constexpr size_t SS_BACK_LDS = sizeof(double) * 3 * TI_COMP_MAX_VARS * SS_LS;
constexpr size_t SS_Y_LDS = sizeof(double) * 4 * TI_COMP_MAX_VARS * SS_LS;
static_assert(SS_Y_LDS + 1024 <= CP_LDS_BYTES_PER_CU && SS_BACK_LDS + 1024 <= CP_LDS_BYTES_PER_CU, "the component kernels fit a CU");

__host__ __device__ __forceinline__ int ss_pair(int r, int s) { return r * (r + 1) / 2 + s; }   // r >= s

// ------------------------------------------------------------------ U_r, V_rs
// work[5 x]: block, row tile, r, s, slot (s = -1: U_r = (d_r D) d into column block slot = r of W; else V_rs = (d2_rs D) d into
// column block slot = R + the pair's rank among the pairs some block reads together).  Dm: d (Q x P).  Every entry of W is
// written by one thread of one workgroup, or not at all (W is zero)
__global__ __launch_bounds__(256) void k_ss_apply(const int* work, const CovBlock* blocks, const int32_t* cov, int rows,
                                                  const double* data, ThetaArg th, const double* Dm, int ldd, int P,
                                                  double* W, int ldw)
{
    __shared__ double dt[SS_ROWS][SS_PC];
    __shared__ double red[SS_JL][SS_ROWS][SS_PC + 1];
    const int* w = work + 5 * (size_t)blockIdx.x;
    const int r = w[2], s = w[3], tid = threadIdx.x, ri = tid & (SS_ROWS - 1), jl = tid / SS_ROWS;
    const CovBlock blk = blocks[w[0]];
    const double* bd = data + blk.doff;
    const int i = w[1] * SS_ROWS + ri, slot = w[4];
    const bool live = i < blk.dim;
    auto entry = [&](int j) {
        return s < 0 ? cov_dentry(blk, cov, rows, bd, th, i, j, r) : cov_d2entry(blk, cov, rows, bd, th, i, j, r, s);
    };
    const double* dcol = Dm + blk.matstart;
    for (int c0 = 0; c0 < P; c0 += SS_PC) {
        double acc[SS_PC];
#pragma unroll
        for (int k = 0; k < SS_PC; ++k) acc[k] = 0.0;
        if (blk.all_gr) {
            if (live && jl == 0) {
                const double f = entry(i);
#pragma unroll
                for (int k = 0; k < SS_PC; ++k)
                    if (c0 + k < P) acc[k] = f * dcol[i + (size_t)(c0 + k) * ldd];
            }
        } else {
            for (int j0 = 0; j0 < blk.dim; j0 += SS_ROWS) {
                __syncthreads();                                        // the previous rows' reads
                for (int e = tid; e < SS_ROWS * SS_PC; e += 256) {
                    const int jj = e & (SS_ROWS - 1), k = e / SS_ROWS, j = j0 + jj;
                    dt[jj][k] = (j < blk.dim && c0 + k < P) ? dcol[j + (size_t)(c0 + k) * ldd] : 0.0;
                }
                __syncthreads();
                if (live)
                    for (int jj = jl; jj < SS_ROWS && j0 + jj < blk.dim; jj += SS_JL) {
                        const double f = entry(j0 + jj);
#pragma unroll
                        for (int k = 0; k < SS_PC; ++k) acc[k] += f * dt[jj][k];
                    }
            }
        }
        __syncthreads();                                                // the previous pass's reads of red
#pragma unroll
        for (int k = 0; k < SS_PC; ++k) red[jl][ri][k] = acc[k];
        __syncthreads();
        if (live && jl == 0)
            for (int k = 0; k < SS_PC && c0 + k < P; ++k)
                W[blk.matstart + i + ((size_t)slot * P + c0 + k) * ldw] = ((red[0][ri][k] + red[1][ri][k]) + red[2][ri][k]) + red[3][ri][k];
    }
}

// ------------------------------------------------------------------ gaussian / identity: A = V (X - ZL c), V A, A2 = V (A - ZL c2)
// out[i, p] = v_i (src[i, p] - zc[i, p]) and, where out2 is not null, out2[i, p] = v_i out[i, p]
__global__ __launch_bounds__(256) void k_ss_resid(const double* src, int lds, const double* zc, int ldz, const double* v, int n, int P,
                                                  double* out, int ldo, double* out2, int ldo2)
{
    const int i = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (i >= n || p >= P) return;
    const double a = v[i] * (src[i + (size_t)p * lds] - zc[i + (size_t)p * ldz]);
    out[i + (size_t)p * ldo] = a;
    if (out2) out2[i + (size_t)p * ldo2] = v[i] * a;
}

// out[i, p] = sum_k ell_val[i, k] C[ell_col[i, k], p], k ascending: ZL C over the ELL rows of ZL (the padding holds column 0 and value 0)
__global__ __launch_bounds__(256) void k_ss_ell(const int* ell_col, const double* ell_val, int n, int W, const double* C, int ldc, int P,
                                                double* out, int ldo)
{
    const int i = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (i >= n || p >= P) return;
    double s = 0;
    for (int k = 0; k < W; ++k) s += ell_val[i + (size_t)k * n] * C[ell_col[i + (size_t)k * n] + (size_t)p * ldc];
    out[i + (size_t)p * ldo] = s;
}

// ------------------------------------------------------------------ component operator
// the component's variables into gv, S0 <- R_c and S1 <- L_c (lower triangles, as k_ti_comp stages them)
__device__ __forceinline__ void ss_stage(int nv, const int* gv, const double* Rc, const double* L, int ldl, double* S0, double* S1)
{
    for (int e = threadIdx.x; e < nv * nv; e += 256) {
        const int i = e % nv, j = e / nv;
        S0[i * SS_LS + j] = i >= j ? Rc[i + (size_t)j * nv] : 0.0;
        S1[i * SS_LS + j] = i >= j ? L[gv[i] + (size_t)gv[j] * ldl] : 0.0;
    }
}

// One workgroup per component, a thread per column: Cout[:, col] = R_c^-T Sin[:, col] (i descending, as k_comp_solve<true>; Sin may
// be Cout) and Dout[:, col] = L_c^-T Cout[:, col], over the component's variables
__global__ __launch_bounds__(256) void k_ss_comp_back(const int* var_ptr, const int* vars, const double* fac, const int* fac_ptr,
                                                      const double* L, int ldl, const double* Sin, int lds, int ncols, double* Cout,
                                                      int ldc, double* Dout, int ldd)
{
    extern __shared__ double lds_[];
    double *S0 = lds_, *S1 = S0 + TI_COMP_MAX_VARS * SS_LS, *S3 = S1 + TI_COMP_MAX_VARS * SS_LS;
    __shared__ int gv[TI_COMP_MAX_VARS];
    const int c = blockIdx.x, v0 = var_ptr[c], nv = var_ptr[c + 1] - v0, tid = threadIdx.x;
    if (nv > TI_COMP_MAX_VARS) return;                                  // the whole workgroup: the host checks the cap
    if (tid < nv) gv[tid] = vars[v0 + tid];
    __syncthreads();
    ss_stage(nv, gv, fac + fac_ptr[c], L, ldl, S0, S1);
    __syncthreads();
    if (tid < nv) lower_inverse_column(S1, S3, SS_LS, nv, tid);
    __syncthreads();
    for (int col = tid; col < ncols; col += 256) {
        const double* sc = Sin + (size_t)col * lds;
        double* cc = Cout + (size_t)col * ldc;
        double* dc = Dout + (size_t)col * ldd;
        for (int k = nv - 1; k >= 0; --k) {
            double acc = sc[gv[k]];
            for (int i = nv - 1; i > k; --i) acc -= S0[i * SS_LS + k] * cc[gv[i]];
            cc[gv[k]] = acc / S0[k * SS_LS + k];
        }
        for (int i = 0; i < nv; ++i) {
            double s = 0;
            for (int k = i; k < nv; ++k) s += S3[k * SS_LS + i] * cc[gv[k]];
            dc[gv[i]] = s;
        }
    }
}

// One workgroup per component, a thread per column: T[:, col] <- L_c^-T M_c^-1 N_c L_c^-1 U[:, col] = ((Z' Sigma^-1 Z) U)[:, col]
// over the component's variables, through Y[:, col].  N_c = ZL_c' V ZL_c from the CSR / ELL rows as k_ti_comp builds it; loc:
// the local index of every variable in its component
__global__ __launch_bounds__(256) void k_ss_comp_y(const int* var_ptr, const int* vars, const double* fac, const int* fac_ptr,
                                                   const double* L, int ldl, const int* loc, const int* csr_ptr, const int* csr_i,
                                                   const double* csr_val, const int* ell_col, const double* ell_val, int n, int W,
                                                   const double* v, const double* U, int ldu, int ncols, double* T, int ldt,
                                                   double* Y, int ldy)
{
    extern __shared__ double lds_[];
    double *S0 = lds_, *S1 = S0 + TI_COMP_MAX_VARS * SS_LS, *S2 = S1 + TI_COMP_MAX_VARS * SS_LS, *S3 = S2 + TI_COMP_MAX_VARS * SS_LS;
    __shared__ int gv[TI_COMP_MAX_VARS];
    const int c = blockIdx.x, v0 = var_ptr[c], nv = var_ptr[c + 1] - v0, tid = threadIdx.x;
    if (nv > TI_COMP_MAX_VARS) return;
    if (tid < nv) gv[tid] = vars[v0 + tid];
    __syncthreads();
    ss_stage(nv, gv, fac + fac_ptr[c], L, ldl, S0, S1);
    for (int e = tid; e < nv * nv; e += 256) S2[(e % nv) * SS_LS + e / nv] = 0.0;
    __syncthreads();
    if (tid < nv) {                                                     // S2 <- N_c, thread a its row a
        const int q = gv[tid];
        for (int t = csr_ptr[q]; t < csr_ptr[q + 1]; ++t) {
            const int i = csr_i[t];
            const double w = csr_val[t] * v[i];
            for (int k = 0; k < W; ++k) {
                const int col = ell_col[i + (size_t)k * n], l = loc[col];
                if (l < nv && gv[l] == col) S2[tid * SS_LS + l] += w * ell_val[i + (size_t)k * n];
            }
        }
    } else if (tid >= 64 && tid - 64 < nv) {
        lower_inverse_column(S1, S3, SS_LS, nv, tid - 64);              // S3 <- L_c^-1
    }
    __syncthreads();
    for (int col = tid; col < ncols; col += 256) {
        const double* uc = U + (size_t)col * ldu;
        double* tc = T + (size_t)col * ldt;
        double* yc = Y + (size_t)col * ldy;
        for (int i = 0; i < nv; ++i) {                                  // t = L_c^-1 u
            double s = 0;
            for (int k = 0; k <= i; ++k) s += S3[i * SS_LS + k] * uc[gv[k]];
            tc[gv[i]] = s;
        }
        for (int i = 0; i < nv; ++i) {                                  // y = N_c t
            double s = 0;
            for (int k = 0; k < nv; ++k) s += S2[i * SS_LS + k] * tc[gv[k]];
            yc[gv[i]] = s;
        }
        for (int k = 0; k < nv; ++k) {                                  // R_c y' = y, R_c' y'' = y'
            double acc = yc[gv[k]];
            for (int i = 0; i < k; ++i) acc -= S0[k * SS_LS + i] * yc[gv[i]];
            yc[gv[k]] = acc / S0[k * SS_LS + k];
        }
        for (int k = nv - 1; k >= 0; --k) {
            double acc = yc[gv[k]];
            for (int i = nv - 1; i > k; --i) acc -= S0[i * SS_LS + k] * yc[gv[i]];
            yc[gv[k]] = acc / S0[k * SS_LS + k];
        }
        for (int i = 0; i < nv; ++i) {                                  // t = L_c^-T y''
            double s = 0;
            for (int k = i; k < nv; ++k) s += S3[k * SS_LS + i] * yc[gv[k]];
            tc[gv[i]] = s;
        }
    }
}

// ------------------------------------------------------------------ the Gram reduction of every job
// dst[a + b P] = scale sum_i u[i, a] w[i, b] over `rows` rows.  sym: a >= b computed and mirrored, also into dstT (the same matrix
// at the transposed index pair) where dstT >= 0; else every (a, b), and dstT[b + a P] = the same value (the transposed matrix)
struct SsJob {
    const double *u, *w;
    int ldu, ldw, rows, sym;
    double scale;
    long long dst, dstT;
};

__global__ __launch_bounds__(256) void k_ss_gram(const SsJob* jobs, int P, int nch, double* part)
{
    __shared__ double sh[4];
    const int a = blockIdx.x % P, b = blockIdx.x / P, job = blockIdx.y / nch, ch = blockIdx.y % nch;
    const SsJob jb = jobs[job];
    if (jb.sym && a < b) return;                                        // the whole block
    const double *u = jb.u + (size_t)a * jb.ldu, *w = jb.w + (size_t)b * jb.ldw;
    const int r0 = ch * SS_CHUNK, r1 = r0 + SS_CHUNK < jb.rows ? r0 + SS_CHUNK : jb.rows;
    double acc = 0;
    for (int i = r0 + threadIdx.x; i < r1; i += 256) acc += u[i] * w[i];
    const double r = block_sum(acc, sh);
    if (threadIdx.x == 0) part[((size_t)job * P * P + blockIdx.x) * nch + ch] = r;
}

// the partials ascending, scaled, to their places in res; thread 0 the two flags of the call behind I_beta
__global__ __launch_bounds__(256) void k_ss_gram_final(const SsJob* jobs, int njobs, int P, int nch, const double* part,
                                                       const int* errflag, const int* bad, double* res)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, PP = (long long)P * P;
    if (t == 0) { res[PP] = (double)*errflag; res[PP + 1] = (double)*bad; }
    if (t >= PP * njobs) return;
    const int job = (int)(t / PP), ab = (int)(t % PP), a = ab % P, b = ab / P;
    const SsJob jb = jobs[job];
    if (jb.sym && a < b) return;
    const double* p = part + (size_t)t * nch;
    double sum = 0;
    for (int ch = 0; ch < nch; ++ch) sum += p[ch];
    const double val = jb.scale * sum;
    res[jb.dst + a + (size_t)b * P] = val;
    if (jb.sym) {
        res[jb.dst + b + (size_t)a * P] = val;
        if (jb.dstT >= 0) { res[jb.dstT + a + (size_t)b * P] = val; res[jb.dstT + b + (size_t)a * P] = val; }
    } else if (jb.dstT >= 0) {
        res[jb.dstT + b + (size_t)a * P] = val;
    }
}

// ------------------------------------------------------------------ host
// rows x cols, zero all over (the K padding of a GEMM that reads it); *bytes += what the matrix takes
static int ss_alloc_zero(Ctx& c, DevMat& A, int rows, int cols, long long* bytes)
{
    MCML_TRY(A.alloc(rows, cols));
    MCML_HIP(hipMemsetAsync(A.d(), 0, sizeof(double) * (size_t)A.ld * A.cols_alloc, c.stream));
    *bytes += (long long)sizeof(double) * A.ld * A.cols_alloc;
    return MCML_OK;
}

static int ss_copy(Ctx& c, DevMat& dst, const double* src, int lds, int cols)
{
    MCML_HIP(hipMemcpy2DAsync(dst.d(), sizeof(double) * (size_t)dst.ld, src, sizeof(double) * (size_t)lds,
                              sizeof(double) * (size_t)dst.rows, (size_t)cols, hipMemcpyDeviceToDevice, c.stream));
    return MCML_OK;
}

// ZC = ZL C on the operator of the call (n x P)
static int ss_zl_apply(Ctx& c, bool comp, const DevMat& C, DevMat& ZC, long long* launches)
{
    const int n = c.n, Q = c.Q, P = c.P;
    if (comp) {
        hipLaunchKernelGGL(k_ss_ell, dim3((n + 255) / 256, P), dim3(256), 0, c.stream, c.sp.ell_col.as<int>(), c.sp.ell_val.d(), n,
                           c.sp.W, C.d(), C.ld, P, ZC.d(), ZC.ld);
        MCML_HIP(hipGetLastError());
        ++*launches;
        return MCML_OK;
    }
    const EpiAxpby epi{ZC.d(), ZC.ld, 1.0, 0.0};
    return launch_gemm<false>(c.stream, n, P, Q, c.ZL.d(), c.ZL.ld, C.d(), C.ld, epi);
}

static int ss_comp_back(Ctx& c, const double* Sin, int lds, int ncols, DevMat& C, DevMat& D, long long* launches)
{
    MCML_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&k_ss_comp_back), (int)SS_BACK_LDS));
    hipLaunchKernelGGL(k_ss_comp_back, dim3(c.cp.plan.ncomp), dim3(256), SS_BACK_LDS, c.stream, c.cp.var_ptr.as<int>(),
                       c.cp.vars.as<int>(), c.info.f.fac.d(), c.info.f.fac_ptr.as<int>(), c.L.d(), c.L.ld, Sin, lds, ncols, C.d(), C.ld,
                       D.d(), D.ld);
    MCML_HIP(hipGetLastError());
    ++*launches;
    return MCML_OK;
}

int small_sample(Ctx& c, const double* beta, double var_par, const double* theta, int op, double* info, int ldi, double* tinfo,
                 int ldt, double* Pm, double* Qm, double* Rm, int* nout)
{
    const int n = c.n, Q = c.Q, P = c.P, R = c.cov.npar;
    MCML_REQUIRE(n > 0 && P > 0 && R > 0, "small_sample: the context has no model / covariance");
    MCML_REQUIRE(beta && theta && info && tinfo && Pm && Qm && Rm && nout, "small_sample: null argument");
    MCML_REQUIRE(op >= 0 && op <= 2, "small_sample: op must be 0 (auto), 1 (dense) or 2 (component)");
    MCML_REQUIRE(c.have_L && !c.l_foreign, "small_sample: the context holds no L made from theta");
    MCML_REQUIRE(std::isfinite(var_par), "small_sample: var_par is not finite");
    const int sigma_row = c.flink == 7 ? 1 : 0, no = R + sigma_row, np = ss_pair(R, 0);
    MCML_REQUIRE(ldi >= P && ldt >= no, "small_sample: ldi %d / ldt %d too small for %d / %d rows", ldi, ldt, P, no);
    MCML_REQUIRE(!sigma_row || var_par != 0.0, "small_sample: sigma is 0");
    SmallSampleState& s = c.ss;
    InfoState& x = c.info;
    ThetaInfoState& t = c.tinfo;
    ThetaInfoCall k;
    MCML_TRY(theta_info_begin(c, "small_sample", theta, op, k));
    const bool comp = k.comp;
    const ComponentPlan& p = c.cp.plan;
    const long long plan0[8] = {op, comp ? 1 : 0, p.ncomp, p.max_vars, 0, 0, R, no};
    std::copy(plan0, plan0 + 8, s.plan);
    long long launches = 0, bytes = 0;

    // ---- the work items of k_ss_apply, the pairs of parameters a block reads together
    const CovSpec& cs = c.cov;
    std::vector<int> work;
    std::vector<int> vslot((size_t)np, -1);                        // the column block of V_rs in W; -1: no block reads both
    int nslot = R;
    for (int r = 0; r < R; ++r)
        for (int q = 0; q <= r; ++q)
            for (int b = 0; b < cs.B; ++b)
                if (((k.mask[b] >> r) & 1u) && ((k.mask[b] >> q) & 1u)) { vslot[ss_pair(r, q)] = nslot++; break; }
    for (int b = 0; b < cs.B; ++b)
        for (int rt = 0; rt < (cs.blocks[b].dim + SS_ROWS - 1) / SS_ROWS; ++rt)
            for (int r = 0; r < R; ++r) {
                if (!((k.mask[b] >> r) & 1u)) continue;
                work.insert(work.end(), {b, rt, r, -1, r});
                for (int q = 0; q <= r; ++q)
                    if ((k.mask[b] >> q) & 1u) work.insert(work.end(), {b, rt, r, q, vslot[ss_pair(r, q)]});
            }
    const int nwork = (int)(work.size() / 5);
    MCML_REQUIRE(nwork > 0, "small_sample: no covariance block reads a parameter");

    // ---- I_beta, then c = R^-T S while c.chol.linv holds the inverted diagonal blocks of M's factor
    InfoDenseScope dense(c);
    MCML_TRY(info_front(c, beta, var_par, comp, true, dense));
    MCML_TRY(info_solve_gram(c, comp, dense.on));
    MCML_TRY(ss_alloc_zero(c, s.C, Q, P, &bytes));
    MCML_TRY(ss_alloc_zero(c, s.Dm, Q, P, &bytes));
    if (comp) {
        MCML_TRY(ss_comp_back(c, x.S.d(), x.S.ld, P, s.C, s.Dm, &launches));
    } else {
        MCML_TRY(ss_copy(c, s.C, x.S.d(), x.S.ld, P));
        MCML_TRY(trsm_left_lower_trans(c, x.M.d(), x.M.ld, Q, s.C.d(), s.C.ld, P));
    }
    if (sigma_row) {
        // A = V (X - ZL c), c2 = M^-1 ZL' V A, A2 = V (A - ZL c2)
        MCML_TRY(ss_alloc_zero(c, s.ZC, n, P, &bytes));
        MCML_TRY(ss_alloc_zero(c, s.A, n, P, &bytes));
        MCML_TRY(ss_alloc_zero(c, s.VA, n, P, &bytes));
        MCML_TRY(ss_alloc_zero(c, s.A2, n, P, &bytes));
        MCML_TRY(ss_alloc_zero(c, s.C2, Q, P, &bytes));
        MCML_TRY(ss_alloc_zero(c, s.D2, Q, P, &bytes));
        const dim3 g((n + 255) / 256, P);
        MCML_TRY(ss_zl_apply(c, comp, s.C, s.ZC, &launches));
        hipLaunchKernelGGL(k_ss_resid, g, dim3(256), 0, c.stream, c.X.d(), c.X.ld, s.ZC.d(), s.ZC.ld, x.v.d(), n, P, s.A.d(), s.A.ld,
                           s.VA.d(), s.VA.ld);
        MCML_HIP(hipGetLastError());
        if (comp) {
            int form = 0;
            MCML_TRY(comp_rhs_csr_launch(c, s.VA.d(), s.VA.ld, P, s.C2.d(), s.C2.ld));
            MCML_TRY(comp_solve_launch(c, x.f, s.C2.d(), s.C2.ld, P, false, &form));
            MCML_TRY(ss_comp_back(c, s.C2.d(), s.C2.ld, P, s.C2, s.D2, &launches));
        } else {
            const EpiAxpby epi{s.C2.d(), s.C2.ld, 1.0, 0.0};
            MCML_TRY(launch_gemm<false>(c.stream, Q, P, n, c.ZLT.d(), c.ZLT.ld, s.VA.d(), s.VA.ld, epi));
            MCML_TRY(trsm_left_lower(c, x.M.d(), x.M.ld, Q, s.C2.d(), s.C2.ld, P));
            MCML_TRY(trsm_left_lower_trans(c, x.M.d(), x.M.ld, Q, s.C2.d(), s.C2.ld, P));
        }
        MCML_TRY(ss_zl_apply(c, comp, s.C2, s.ZC, &launches));
        hipLaunchKernelGGL(k_ss_resid, g, dim3(256), 0, c.stream, s.A.d(), s.A.ld, s.ZC.d(), s.ZC.ld, x.v.d(), n, P, s.A2.d(), s.A2.ld,
                           (double*)nullptr, 0);
        MCML_HIP(hipGetLastError());
        launches += 2;
    }

    // ---- I_theta; the dense operator leaves B = M^-1 N and, in c.chol.linv, the inverted diagonal blocks of L
    MCML_TRY(theta_info_compute(c, k, var_par));
    if (!comp) {
        MCML_TRY(ss_copy(c, s.Dm, s.C.d(), s.C.ld, P));
        MCML_TRY(trsm_left_lower_trans(c, c.L.d(), c.L.ld, Q, s.Dm.d(), s.Dm.ld, P));
        if (sigma_row) {
            MCML_TRY(ss_copy(c, s.D2, s.C2.d(), s.C2.ld, P));
            MCML_TRY(trsm_left_lower_trans(c, c.L.d(), c.L.ld, Q, s.D2.d(), s.D2.ld, P));
        }
    }

    // ---- U_r, V_rs
    const int ucols = R * P;
    MCML_TRY(ss_alloc_zero(c, s.W, Q, nslot * P, &bytes));
    MCML_TRY(s.work.ensure(sizeof(int) * work.size()));
    MCML_TRY(copy_h2d(s.work.p, work.data(), sizeof(int) * work.size(), c.stream));
    hipLaunchKernelGGL(k_ss_apply, dim3(nwork), dim3(256), 0, c.stream, s.work.as<int>(), c.d_blocks.as<CovBlock>(),
                       c.d_cov.as<int32_t>(), cs.rows, c.d_data.d(), k.th, s.Dm.d(), s.Dm.ld, P, s.W.d(), s.W.ld);
    MCML_HIP(hipGetLastError());
    ++launches;

    // ---- Y_r = (Z' Sigma^-1 Z) U_r, all R P columns at once
    MCML_TRY(ss_alloc_zero(c, s.T, Q, ucols, &bytes));
    MCML_TRY(ss_alloc_zero(c, s.Y, Q, ucols, &bytes));
    const double* Yr;
    int ldy;
    if (comp) {
        MCML_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&k_ss_comp_y), (int)SS_Y_LDS));
        hipLaunchKernelGGL(k_ss_comp_y, dim3(p.ncomp), dim3(256), SS_Y_LDS, c.stream, c.cp.var_ptr.as<int>(), c.cp.vars.as<int>(),
                           x.f.fac.d(), x.f.fac_ptr.as<int>(), c.L.d(), c.L.ld, t.blk_of_var.as<int>() + Q, c.sp.csr_ptr.as<int>(),
                           c.sp.csr_i.as<int>(), c.sp.csr_val.d(), c.sp.ell_col.as<int>(), c.sp.ell_val.d(), n, c.sp.W, x.v.d(),
                           s.W.d(), s.W.ld, ucols, s.T.d(), s.T.ld, s.Y.d(), s.Y.ld);
        MCML_HIP(hipGetLastError());
        ++launches;
        Yr = s.T.d(); ldy = s.T.ld;
    } else {
        MCML_TRY(ss_copy(c, s.T, s.W.d(), s.W.ld, ucols));
        MCML_TRY(trsm_left_lower(c, c.L.d(), c.L.ld, Q, s.T.d(), s.T.ld, ucols));
        const EpiAxpby epi{s.Y.d(), s.Y.ld, 1.0, 0.0};
        MCML_TRY(launch_gemm<false>(c.stream, Q, ucols, Q, t.B.d(), t.B.ld, s.T.d(), s.T.ld, epi));
        MCML_TRY(trsm_left_lower_trans(c, c.L.d(), c.L.ld, Q, s.Y.d(), s.Y.ld, ucols));
        Yr = s.Y.d(); ldy = s.Y.ld;
    }

    // ---- the jobs of the Gram reduction, the result
    const size_t PP = (size_t)P * P;
    const long long off_ti = (long long)PP + 2, off_P = off_ti + (long long)no * no, off_Q = off_P + (long long)no * PP,
                    off_R = off_Q + (long long)no * no * PP, total = off_R + (long long)no * no * PP;
    auto at = [&](long long off, int r, int q) { return off + (long long)(r + no * q) * (long long)PP; };
    auto wcol = [&](int slot) { return s.W.d() + (size_t)slot * P * s.W.ld; };
    std::vector<SsJob> jobs;
    for (int r = 0; r < R; ++r) jobs.push_back({s.Dm.d(), wcol(r), s.Dm.ld, s.W.ld, Q, 1, -1.0, off_P + (long long)r * (long long)PP, -1});
    for (int r = 0; r < R; ++r)
        for (int q = 0; q <= r; ++q) {
            jobs.push_back({wcol(r), Yr + (size_t)q * P * ldy, s.W.ld, ldy, Q, r == q ? 1 : 0, 1.0, at(off_Q, r, q),
                            r == q ? -1 : at(off_Q, q, r)});
            if (vslot[ss_pair(r, q)] >= 0)
                jobs.push_back({s.Dm.d(), wcol(vslot[ss_pair(r, q)]), s.Dm.ld, s.W.ld, Q, 1, 1.0, at(off_R, r, q), r == q ? -1 : at(off_R, q, r)});
        }
    if (sigma_row) {
        const double sg = var_par;
        jobs.push_back({s.A.d(), s.A.d(), s.A.ld, s.A.ld, n, 1, -2.0 * sg, off_P + (long long)R * (long long)PP, -1});
        jobs.push_back({s.A.d(), s.A2.d(), s.A.ld, s.A2.ld, n, 1, 4.0 * sg * sg, at(off_Q, R, R), -1});
        jobs.push_back({s.A.d(), s.A.d(), s.A.ld, s.A.ld, n, 1, 2.0, at(off_R, R, R), -1});
        for (int r = 0; r < R; ++r)
            jobs.push_back({wcol(r), s.D2.d(), s.W.ld, s.D2.ld, Q, 0, 2.0 * sg, at(off_Q, r, R), at(off_Q, R, r)});
    }
    const int njobs = (int)jobs.size(), nch = (std::max(n, Q) + SS_CHUNK - 1) / SS_CHUNK;
    MCML_REQUIRE((long long)njobs * nch <= 65535 && PP * (size_t)njobs < (size_t)1 << 31, "small_sample: %d Gram jobs of %d chunks", njobs, nch);
    MCML_TRY(s.jobs.ensure(sizeof(SsJob) * jobs.size()));
    MCML_TRY(copy_h2d(s.jobs.p, jobs.data(), sizeof(SsJob) * jobs.size(), c.stream));
    MCML_TRY(s.part.ensure(sizeof(double) * PP * (size_t)njobs * nch));
    MCML_TRY(s.res.ensure(sizeof(double) * (size_t)total));
    MCML_HIP(hipMemsetAsync(s.res.d(), 0, sizeof(double) * (size_t)total, c.stream));
    MCML_HIP(hipMemcpyAsync(s.res.d(), x.res.d(), sizeof(double) * PP, hipMemcpyDeviceToDevice, c.stream));
    MCML_HIP(hipMemcpyAsync(s.res.d() + off_ti, t.res.d(), sizeof(double) * (size_t)no * no, hipMemcpyDeviceToDevice, c.stream));
    hipLaunchKernelGGL(k_ss_gram, dim3((unsigned)PP, njobs * nch), dim3(256), 0, c.stream, s.jobs.as<SsJob>(), P, nch, s.part.d());
    MCML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ss_gram_final, dim3((unsigned)((PP * njobs + 255) / 256)), dim3(256), 0, c.stream, s.jobs.as<SsJob>(), njobs, P, nch,
                       s.part.d(), c.errflag(), x.bad.as<int>(), s.res.d());
    MCML_HIP(hipGetLastError());
    launches += 2;
    s.plan[4] = launches; s.plan[5] = bytes;

    // ---- the one download (it synchronises the stream: work and jobs may leave scope)
    std::vector<double> h;
    const int rc = query_download(c, s.res, P, (size_t)(total - (long long)PP - 2), "small_sample",
                                  "a weight dhdmu(x' beta) * scale, or its reciprocal,", h);
    if (rc != MCML_OK) {
        if (rc == MCML_EHIP) (void)hipStreamSynchronize(c.stream);
        return rc;
    }
    copy_columns(info, ldi, h.data(), P, P);
    copy_columns(tinfo, ldt, h.data() + off_ti, no, no);
    memcpy(Pm, h.data() + off_P, sizeof(double) * (size_t)no * PP);
    memcpy(Qm, h.data() + off_Q, sizeof(double) * (size_t)no * no * PP);
    memcpy(Rm, h.data() + off_R, sizeof(double) * (size_t)no * no * PP);
    *nout = no;
    return MCML_OK;
}

}  // namespace mcml
