// info.hip -- the GLS information matrix of the fixed effects, X' (W^-1 + Z D Z')^-1 X, on the device (a query: DESIGN.md 5.9).
// The definition is the caller layer's (glmmrmcml_amd/model.py information_matrix): W^-1 = diag(w), w_i = dhdmu(x_i' beta)
// times the family's scale, no random-effect term in the linear predictor.  With D = L L' and V = diag(1 / w), Woodbury gives
//     X' (V^-1 + ZL ZL')^-1 X = X' V X - S' S,    M = I + ZL' V ZL = R R',    S = R^-1 (ZL' V X)
// and M is the matrix the Laplace fits and the exact draws build and factorise:
//   k_info_weights                  v = 1 / w and XV = diag(v) X (n x P)
//   dense operator                  B = ZL' XV by the MFMA GEMM on c.ZLT, build_M_dense (lower), potrf, trsm_left_lower (P columns)
//   component operator              component.h, "applying a factor": B by the CSR rows of ZL' (comp_rhs_csr_launch),
//                                   lac_factor_launch with W = v, then comp_solve_launch: R_c S_c = B_c for all P columns
//   gram_launch                     out[a, b] = sum_i X_ia v_i X_ib - sum_q S_qa S_qb, a >= b, mirrored
// Everything runs on c.stream and one download of P x P + 2 doubles ends the call.  No atomics, every sum in a fixed order:
// two calls give the same bits.  y is not read, no collective is issued, and nothing a sampler or a fit reads is changed.
// Two rules the sandwich (sandwich.hip) shares live here and are declared in entry.h: the chunked Gram reduction (gram_launch:
// its meat is the same reduction without the second sum) and the flagged tail that ends a query (query_download).
// info_matrix itself is info_front, info_solve_gram and the download; the small-sample query (small_sample.hip) calls the
// first two for its I_beta block and goes on from the S they leave.
#include "entry.h"
#include "component.h"
#include "dgemm_mfma.h"
#include "glm.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

namespace mcml {

// v_i = 1 / (dhdmu(xb_i) scale), xb_i = row_xb, and row i of XV.  A weight or a reciprocal that is not finite raises *bad
// (every thread that stores, stores 1)
__global__ __launch_bounds__(256) void k_info_weights(const double* X, int ldx, int n, int P, const double* beta, int flink,
                                                      double scale, double* v, double* XV, int ldxv, int* bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double w = glm_dhdmu(row_xb(X, ldx, i, P, beta), flink) * scale;
    const double vi = 1 / w;
    if (!__builtin_isfinite(w) || !__builtin_isfinite(vi)) *bad = 1;
    v[i] = vi;
    for (int p = 0; p < P; ++p) XV[i + (size_t)p * ldxv] = vi * X[i + (size_t)p * ldx];
}

// ---- the Gram reduction.  Block (a + b P, c), a >= b: the partial sum of chunk c -- chunks [0, cx) are INFO_CHUNK rows of
// X[:, a] XV[:, b], chunks [cx, gridDim.y) INFO_CHUNK rows of S[:, a] S[:, b] -- in the fixed order of block_sum
constexpr int INFO_CHUNK = 2048;
__global__ __launch_bounds__(256) void k_info_gram(const double* X, int ldx, const double* XV, int ldxv, int n, const double* S,
                                                   int lds, int Q, int P, int cx, double* part)
{
    __shared__ double sh[4];
    const int a = blockIdx.x % P, b = blockIdx.x / P, c = blockIdx.y;
    if (a < b) return;                               // the whole block
    const double *u, *w;
    int r0, r1;
    if (c < cx) {
        u = X + (size_t)a * ldx; w = XV + (size_t)b * ldxv;
        r0 = c * INFO_CHUNK; r1 = r0 + INFO_CHUNK < n ? r0 + INFO_CHUNK : n;
    } else {
        u = S + (size_t)a * lds; w = S + (size_t)b * lds;
        r0 = (c - cx) * INFO_CHUNK; r1 = r0 + INFO_CHUNK < Q ? r0 + INFO_CHUNK : Q;
    }
    double acc = 0;
    for (int i = r0 + threadIdx.x; i < r1; i += 256) acc += u[i] * w[i];
    const double r = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * gridDim.y + c] = r;
}

// out[a, b] = out[b, a] = (sum of the X partials, ascending) - (sum of the S partials, ascending), a >= b; the two flags of the
// call ride behind the matrix: out[P P] = the context's "not positive definite" flag, out[P P + 1] = the weights'
__global__ __launch_bounds__(256) void k_info_gram_final(const double* part, int P, int cx, int nch, const int* errflag,
                                                         const int* bad, double* out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0) { out[(size_t)P * P] = (double)*errflag; out[(size_t)P * P + 1] = (double)*bad; }
    if (t >= P * P) return;
    const int a = t % P, b = t / P;
    if (a < b) return;
    const double* p = part + (size_t)t * nch;
    double sx = 0, ss = 0;
    for (int c = 0; c < cx; ++c) sx += p[c];
    for (int c = cx; c < nch; ++c) ss += p[c];
    const double val = sx - ss;
    out[a + (size_t)b * P] = val;
    out[b + (size_t)a * P] = val;
}

int gram_launch(Ctx& c, const double* U, int ldu, const double* W, int ldw, int n, const double* S, int lds, int Q, int P,
                DevBuf& part, const int* bad, double* out)
{
    const int cx = (n + INFO_CHUNK - 1) / INFO_CHUNK, nch = cx + (Q + INFO_CHUNK - 1) / INFO_CHUNK;
    const size_t PP = (size_t)P * P;
    MCML_TRY(part.ensure(sizeof(double) * PP * (size_t)nch));
    hipLaunchKernelGGL(k_info_gram, dim3((unsigned)PP, nch), dim3(256), 0, c.stream, U, ldu, W, ldw, n, S, lds, Q, P, cx, part.d());
    MCML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_info_gram_final, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, c.stream, part.d(), P, cx, nch,
                       c.errflag(), bad, out);
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

int query_download(Ctx& c, const DevBuf& res, int P, size_t extra, const char* who, const char* bad_what, std::vector<double>& h)
{
    const size_t PP = (size_t)P * P;
    h.resize(PP + 2 + extra);
    MCML_TRY(copy_d2h(h.data(), res.p, sizeof(double) * h.size(), c.stream));
    MCML_HIP(hipStreamSynchronize(c.stream));
    if (h[PP] != 0.0) {                                               // cleared as check_errflag clears it
        MCML_HIP(hipMemsetAsync(c.errflag(), 0, sizeof(int), c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
    }
    if (h[PP + 1] != 0.0) {
        set_error("%s: %s is not finite", who, bad_what);
        return MCML_EINVAL;
    }
    if (h[PP] != 0.0) {
        set_error("%s: ZL' V ZL + I is not positive definite", who);
        return MCML_ENOTPD;
    }
    return MCML_OK;
}

// the scale of the weights (model.py information_matrix): sigma^2 gaussian, sigma Gamma, 1 + sigma beta, else 1
static double info_scale(int flink, double var_par)
{
    if (glm_is_gaussian(flink)) return var_par * var_par;
    if (flink >= 9 && flink <= 11) return var_par;
    if (flink == 12) return 1 + var_par;
    return 1.0;
}

// The front half of a query on Sigma = diag(w) + Z D Z' (info_matrix here, theta_info.hip): the weights with their flag, then the
// factor of M = I + ZL' V ZL -- the component operator's factors in x.f (comp), or the dense M factorised in x.M, its inverted
// diagonal blocks in c.chol.linv, on the dense ZL / ZL' that `dense` builds beside a sparse operator.  rhs: the right-hand
// sides ZL' V X of the information query ride along into x.S (Q x P), at the places info_matrix has always launched them
int info_front(Ctx& c, const double* beta, double var_par, bool comp, bool rhs, InfoDenseScope& dense)
{
    const int n = c.n, Q = c.Q, P = c.P;
    InfoState& x = c.info;
    const ComponentPlan& p = c.cp.plan;
    // ---- weights, XV
    MCML_TRY(x.beta.ensure(sizeof(double) * (size_t)P));
    MCML_TRY(x.bad.ensure(sizeof(int)));
    MCML_TRY(x.v.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(x.XV.alloc(n, P));
    if (rhs) MCML_TRY(x.S.alloc(Q, P));
    MCML_TRY(copy_h2d(x.beta.p, beta, sizeof(double) * (size_t)P, c.stream));
    MCML_HIP(hipMemsetAsync(x.bad.p, 0, sizeof(int), c.stream));
    MCML_HIP(hipMemsetAsync(x.XV.d(), 0, sizeof(double) * (size_t)x.XV.ld * x.XV.cols_alloc, c.stream));   // the K padding of the GEMM
    if (rhs) MCML_HIP(hipMemsetAsync(x.S.d(), 0, sizeof(double) * (size_t)x.S.ld * x.S.cols_alloc, c.stream));
    hipLaunchKernelGGL(k_info_weights, dim3((n + 255) / 256), dim3(256), 0, c.stream, c.X.d(), c.X.ld, n, P, x.beta.d(), c.flink,
                       info_scale(c.flink, var_par), x.v.d(), x.XV.d(), x.XV.ld, x.bad.as<int>());
    MCML_HIP(hipGetLastError());

    if (comp) {
        // ---- B by the CSR rows of ZL', every M_c factorised
        MCML_TRY(comp_factors_ensure(c, x.f));
        if (rhs) MCML_TRY(comp_rhs_csr_launch(c, x.XV.d(), x.XV.ld, P, x.S.d(), x.S.ld));
        x.waves = cp_waves(p, cp_forced_waves(CP_LA_WAVES_ENV));
        MCML_TRY(lac_factor_launch(c, x.v.d(), 0.0, nullptr, nullptr, x.f.logdet.d(), x.f.fac.d(), x.f.fac_ptr.as<int>(), x.waves, nullptr));
    } else {
        // ---- B = ZL' XV, M and its factor on the dense ZL / ZL'
        if (c.sp.active) MCML_TRY(dense.build());
        MCML_REQUIRE(c.ZL.d() && c.ZLT.d() && c.ZL.rows == n && c.ZL.cols == Q, "information: the dense ZL is not resident");
        if (rhs) {
            const EpiAxpby epi{x.S.d(), x.S.ld, 1.0, 0.0};
            MCML_TRY(launch_gemm<false>(c.stream, Q, P, n, c.ZLT.d(), c.ZLT.ld, x.XV.d(), x.XV.ld, epi));
        }
        MCML_TRY(build_M_dense(c, x.v.d(), 1.0, x.M, x.ZLTW, true));
        MCML_TRY(potrf_lower(c, x.M.d(), Q, x.M.ld));                 // a failed pivot raises c.errflag(): read at the end
    }
    return MCML_OK;
}

int info_solve_gram(Ctx& c, bool comp, bool dense_built)
{
    const int n = c.n, Q = c.Q, P = c.P;
    InfoState& x = c.info;
    if (comp) {
        int form = 0;
        MCML_TRY(comp_solve_launch(c, x.f, x.S.d(), x.S.ld, P, false, &form));
        x.plan[1] = form; x.plan[4] = x.waves; x.plan[5] = 2;
    } else {
        MCML_TRY(trsm_left_lower(c, x.M.d(), x.M.ld, Q, x.S.d(), x.S.ld, P));
        x.plan[6] = (long long)(x.M.buf.bytes + x.ZLTW.buf.bytes + (dense_built ? c.ZL.buf.bytes + c.ZLT.buf.bytes : 0));
    }
    // ---- the Gram reduction
    MCML_TRY(x.res.ensure(sizeof(double) * ((size_t)P * P + 2)));
    return gram_launch(c, c.X.d(), c.X.ld, x.XV.d(), x.XV.ld, n, x.S.d(), x.S.ld, Q, P, x.part, x.bad.as<int>(), x.res.d());
}

int info_matrix(Ctx& c, const double* beta, double var_par, int op, double* out, int ldo)
{
    const int n = c.n, P = c.P;
    MCML_REQUIRE(n > 0 && P > 0, "information: the context has no model");
    MCML_REQUIRE(beta && out && ldo >= P, "information: null argument / ldo too small");
    MCML_REQUIRE(op >= 0 && op <= 2, "information: op must be 0 (auto), 1 (dense) or 2 (component)");
    MCML_REQUIRE(c.have_L, "information: the context holds no L: pass theta or call update_L first");
    MCML_REQUIRE(std::isfinite(var_par), "information: var_par is not finite");
    InfoState& x = c.info;
    const ComponentPlan& p = c.cp.plan;
    const bool comp_ok = comp_operator_ready(c);
    const long long plan0[8] = {op, 0, p.ncomp, p.max_vars, 0, 0, 0, P};
    std::copy(plan0, plan0 + 8, x.plan);
    if (op == 2 && !comp_ok) {
        set_error("information: the component operator needs the sparse ZL operator and no component above %d variables",
                  CP_WIDE_MAX_VARS);
        return MCML_EUNSUPPORTED;
    }
    const bool comp = op != 1 && comp_ok;

    InfoDenseScope dense(c);
    MCML_TRY(info_front(c, beta, var_par, comp, true, dense));
    MCML_TRY(info_solve_gram(c, comp, dense.on));
    // ---- the one download
    std::vector<double> h;
    MCML_TRY(query_download(c, x.res, P, 0, "information", "a weight dhdmu(x' beta) * scale, or its reciprocal,", h));
    copy_columns(out, ldo, h.data(), P, P);
    return MCML_OK;
}

}  // namespace mcml
