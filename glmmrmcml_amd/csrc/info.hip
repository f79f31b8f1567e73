// info.hip -- the GLS information matrix of the fixed effects, X' (W^-1 + Z D Z')^-1 X, on the device (a query: DESIGN.md 5.9).
// The definition is the caller layer's (glmmrmcml_amd/model.py information_matrix): W^-1 = diag(w), w_i = dhdmu(x_i' beta)
// times the family's scale, no random-effect term in the linear predictor.  With D = L L' and V = diag(1 / w), Woodbury gives
//     X' (V^-1 + ZL ZL')^-1 X = X' V X - S' S,    M = I + ZL' V ZL = R R',    S = R^-1 (ZL' V X)
// and M is the matrix the Laplace fits and the exact draws build and factorise:
//   k_info_weights                  v = 1 / w and XV = diag(v) X (n x P)
//   dense operator                  B = ZL' XV by the MFMA GEMM on c.ZLT, build_M_dense (lower), potrf, trsm_left_lower (P columns)
//   component operator              B by the CSR rows of ZL' (k_info_rhs_csr), lac_factor_launch with W = v (component.hip), then
//                                   k_cinfo_solve: R_c S_c = B_c for all P columns, component by component in LDS
//   k_info_gram, k_info_gram_final  out[a, b] = sum_i X_ia v_i X_ib - sum_q S_qa S_qb, a >= b, mirrored
// Everything runs on c.stream and one download of P x P + 2 doubles ends the call.  No atomics, every sum in a fixed order:
// two calls give the same bits.  y is not read, no collective is issued, and nothing a sampler or a fit reads is changed.
#include "entry.h"
#include "component.h"
#include "dgemm_mfma.h"
#include "glm.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

namespace mcml {

// v_i = 1 / (dhdmu(xb_i) scale), xb = X beta (p ascending, as k_xb), and row i of XV.  A weight or a reciprocal that is not
// finite raises *bad (every thread that stores, stores 1)
__global__ __launch_bounds__(256) void k_info_weights(const double* X, int ldx, int n, int P, const double* beta, int flink,
                                                      double scale, double* v, double* XV, int ldxv, int* bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double xb = 0;
    for (int p = 0; p < P; ++p) xb += X[i + (size_t)p * ldx] * beta[p];
    const double w = glm_dhdmu(xb, flink) * scale;
    const double vi = 1 / w;
    if (!__builtin_isfinite(w) || !__builtin_isfinite(vi)) *bad = 1;
    v[i] = vi;
    for (int p = 0; p < P; ++p) XV[i + (size_t)p * ldxv] = vi * X[i + (size_t)p * ldx];
}

// B[q, a] = sum_t csr_val[t] XV[csr_i[t], a]: row q of ZL', observations ascending, for every column a
__global__ __launch_bounds__(256) void k_info_rhs_csr(const int* csr_ptr, const int* csr_i, const double* csr_val, const double* XV,
                                                      int ldxv, int Q, int P, double* B, int ldb)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    for (int a = blockIdx.y; a < P; a += gridDim.y) {
        const double* col = XV + (size_t)a * ldxv;
        B[q + (size_t)a * ldb] = csr_row_sum(csr_ptr, csr_i, csr_val, q, [&](int i) { return col[i]; });
    }
}

// ---- the component solve.  A lane owns one (component, column) pair and runs the forward substitution R_c s = b for it, its
// vector in LDS as [variable][lane] (the layout of k_exc_draw: the 32 lanes of a half read consecutive doubles).  R_c is
// staged from the factor scratch as packed rows -- entry (k, i), i <= k, at k (k + 1) / 2 + i -- so that the wave's own block
// of LDS holds the triangle and the vectors side by side at CP_WIDE_MAX_VARS (a square with an odd leading dimension as in
// k_lac_factor_wg would take 129 KB and leave the vectors 31 KB).  Two forms, picked by the plan as for k_exc_draw:
//   staged items   components up to CP_MAX_VARS variables: CINFO_WAVES waves per workgroup, a wave per work item; the item's
//                  components are staged G at a time, each at an ODD stride, and the lanes enumerate (component, column)
//                  pairs: lanes of one component read one address (a broadcast), lanes of different components different
//                  banks.  With P = 2 and components of 11 variables (config 5) 15 components keep 30 lanes busy
//   one component  up to CP_WIDE_MAX_VARS: one wave per workgroup and component, every read of R_c a broadcast
// More than 64 pairs are worked through 64 at a time (one component: the columns in chunks of 64).
constexpr int CINFO_WAVES = 4;
constexpr int CINFO_R_DOUBLES = 1024;                // a wave's room for staged triangles in the item form
constexpr int cinfo_stride(int mv) { return (mv * (mv + 1) / 2) | 1; }
constexpr int cinfo_r_doubles(int mv) { return mv <= CP_MAX_VARS && cinfo_stride(mv) < CINFO_R_DOUBLES ? CINFO_R_DOUBLES : cinfo_stride(mv); }
constexpr int cinfo_waves(int mv) { return mv <= CP_MAX_VARS ? CINFO_WAVES : 1; }
constexpr int cinfo_lds_bytes(int mv) { return 8 * cinfo_waves(mv) * (mv * 64 + cinfo_r_doubles(mv)); }
static_assert(cinfo_lds_bytes(CP_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_cinfo_solve, staged items at their cap");
static_assert(cinfo_lds_bytes(CP_WIDE_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_cinfo_solve, one wave at the cap");

struct CinfoArgs {
    CompView cv;                         // items != 0: a wave takes work item t = components [item_ptr[t], item_ptr[t + 1]); else component t
    const int* fac_ptr;                  // InfoState: the factors of lac_factor_launch, lower triangles, leading dimension nv_c
    const double* fac;
    double* S;                           // Q x P, in: B, out: S
    size_t lds;
    int P, items;
};

// grid ceil(items / waves), 64 * waves threads, cinfo_lds_bytes(max_vars) of dynamic LDS.  No workgroup barrier
__global__ __launch_bounds__(64 * CINFO_WAVES) void k_cinfo_solve(CinfoArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double cinfo_lds[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blockIdx.x * (a.items ? CINFO_WAVES : 1) + w;
    if (item >= (a.items ? a.cv.nitems : a.cv.ncomp)) return;
    const int mv = a.cv.max_vars, stride = cinfo_stride(mv), rd = cinfo_r_doubles(mv);
    double* x = cinfo_lds + (size_t)w * (mv * 64 + rd);                          // [variable][lane]
    double* R = x + mv * 64;                                                     // slot s at R + s stride
    const int G = a.items ? (rd / stride < 64 ? rd / stride : 64) : 1;           // components staged side by side, >= 1
    const int c0 = a.items ? a.cv.item_ptr[item] : item, c1 = a.items ? a.cv.item_ptr[item + 1] : item + 1;
    for (int cs = c0; cs < c1; cs += G) {
        const int g = c1 - cs < G ? c1 - cs : G;
        wave_lds_sync();                             // the previous group's reads of R
        for (int s = 0; s < g; ++s) {
            const int nv = a.cv.var_ptr[cs + s + 1] - a.cv.var_ptr[cs + s];      // 1 <= nv <= mv
            const double* F = a.fac + a.fac_ptr[cs + s];
            double* Rs = R + s * stride;
            for (int e = lane; e < nv * nv; e += 64) {
                const int i = e % nv, j = e / nv;
                if (i >= j) Rs[i * (i + 1) / 2 + j] = F[e];
            }
        }
        wave_lds_sync();
        for (int e = lane; e < g * a.P; e += 64) {
            const int s = e / a.P, col = e - s * a.P;
            const int v0 = a.cv.var_ptr[cs + s], nv = a.cv.var_ptr[cs + s + 1] - v0;
            const double* Rs = R + s * stride;
            double* Sc = a.S + (size_t)col * a.lds;
            // s_k = (b_k - sum_{i < k} R_c[k, i] s_i) / R_c[k, k], i ascending
            for (int k = 0; k < nv; ++k) {
                const int q = a.cv.vars[v0 + k];
                const double* row = Rs + k * (k + 1) / 2;
                double acc = Sc[q];
                for (int i = 0; i < k; ++i) acc -= row[i] * x[i * 64 + lane];
                acc = acc / row[k];
                x[k * 64 + lane] = acc;
                Sc[q] = acc;
            }
        }
    }
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

// the scale of the weights (model.py information_matrix): sigma^2 gaussian, sigma Gamma, 1 + sigma beta, else 1
static double info_scale(int flink, double var_par)
{
    if (glm_is_gaussian(flink)) return var_par * var_par;
    if (flink >= 9 && flink <= 11) return var_par;
    if (flink == 12) return 1 + var_par;
    return 1.0;
}

// op = 1 on a context whose operator is the sparse one: the dense ZL / ZL' beside it, built as the Laplace fits' dense operator
// builds them; the sparse pair and the records are not written, so the context's operator is the sparse one again on every exit
struct InfoDenseScope {
    Ctx& c;
    bool on = false;
    explicit InfoDenseScope(Ctx& ctx) : c(ctx) {}
    int build()
    {
        on = true;
        c.no_sparse_zl = true;
        return model_update_L(c);
    }
    ~InfoDenseScope() { if (on) { c.no_sparse_zl = false; c.sp.active = true; } }
};

bool info_component_applicable(const Ctx& c) { return c.have_L && c.sp.active && c.cp.ready && c.cp.plan.records; }

int info_matrix(Ctx& c, const double* beta, double var_par, int op, double* out, int ldo)
{
    const int n = c.n, Q = c.Q, P = c.P;
    MCML_REQUIRE(n > 0 && P > 0, "information: the context has no model");
    MCML_REQUIRE(beta && out && ldo >= P, "information: null argument / ldo too small");
    MCML_REQUIRE(op >= 0 && op <= 2, "information: op must be 0 (auto), 1 (dense) or 2 (component)");
    MCML_REQUIRE(c.have_L, "information: the context holds no L: pass theta or call update_L first");
    MCML_REQUIRE(std::isfinite(var_par), "information: var_par is not finite");
    InfoState& x = c.info;
    const ComponentPlan& p = c.cp.plan;
    const bool comp_ok = info_component_applicable(c);
    const long long plan0[8] = {op, 0, p.ncomp, p.max_vars, 0, 0, 0, P};
    std::copy(plan0, plan0 + 8, x.plan);
    if (op == 2 && !comp_ok) {
        set_error("information: the component operator needs the sparse ZL operator and no component above %d variables",
                  CP_WIDE_MAX_VARS);
        return MCML_EUNSUPPORTED;
    }
    const bool comp = op != 1 && comp_ok;

    // ---- weights, XV
    MCML_TRY(x.beta.ensure(sizeof(double) * (size_t)P));
    MCML_TRY(x.bad.ensure(sizeof(int)));
    MCML_TRY(x.v.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(x.XV.alloc(n, P));
    MCML_TRY(x.S.alloc(Q, P));
    MCML_TRY(copy_h2d(x.beta.p, beta, sizeof(double) * (size_t)P, c.stream));
    MCML_HIP(hipMemsetAsync(x.bad.p, 0, sizeof(int), c.stream));
    MCML_HIP(hipMemsetAsync(x.XV.d(), 0, sizeof(double) * (size_t)x.XV.ld * x.XV.cols_alloc, c.stream));   // the K padding of the GEMM
    MCML_HIP(hipMemsetAsync(x.S.d(), 0, sizeof(double) * (size_t)x.S.ld * x.S.cols_alloc, c.stream));
    hipLaunchKernelGGL(k_info_weights, dim3((n + 255) / 256), dim3(256), 0, c.stream, c.X.d(), c.X.ld, n, P, x.beta.d(), c.flink,
                       info_scale(c.flink, var_par), x.v.d(), x.XV.d(), x.XV.ld, x.bad.as<int>());
    MCML_HIP(hipGetLastError());

    if (comp) {
        // ---- B by the CSR rows of ZL', every M_c factorised, the forward solves
        if (!x.fac_doubles) {                                         // the pattern is fixed per model
            const std::vector<int> off = comp_factor_offsets(p);
            MCML_TRY(x.fac_ptr.ensure(sizeof(int) * off.size()));
            MCML_TRY(copy_h2d(x.fac_ptr.p, off.data(), sizeof(int) * off.size(), c.stream));
            MCML_HIP(hipStreamSynchronize(c.stream));
            MCML_TRY(x.fac.ensure(sizeof(double) * (size_t)off.back()));
            x.fac_doubles = off.back();
        }
        MCML_TRY(x.logdet.ensure(sizeof(double) * (size_t)p.ncomp));
        hipLaunchKernelGGL(k_info_rhs_csr, dim3((Q + 255) / 256, P < 1024 ? P : 1024), dim3(256), 0, c.stream, c.sp.csr_ptr.as<int>(),
                           c.sp.csr_i.as<int>(), c.sp.csr_val.d(), x.XV.d(), x.XV.ld, Q, P, x.S.d(), x.S.ld);
        MCML_HIP(hipGetLastError());
        const int waves = cp_waves(p, cp_forced_waves(CP_LA_WAVES_ENV));
        MCML_TRY(lac_factor_launch(c, x.v.d(), 0.0, nullptr, nullptr, x.logdet.d(), x.fac.d(), x.fac_ptr.as<int>(), waves, nullptr));
        const bool items = p.feasible;                                // max_vars <= CP_MAX_VARS: the plan's work items are built
        const CinfoArgs a{comp_view(c), x.fac_ptr.as<int>(), x.fac.d(), x.S.d(), (size_t)x.S.ld, P, items ? 1 : 0};
        const int nw = cinfo_waves(p.max_vars), cnt = items ? a.cv.nitems : a.cv.ncomp;
        // one kernel, both forms: the attribute is set once per kernel and device, so to the larger of the two caps
        MCML_TRY(ensure_dynamic_lds((const void*)k_cinfo_solve, std::max(cinfo_lds_bytes(CP_MAX_VARS), cinfo_lds_bytes(CP_WIDE_MAX_VARS))));
        hipLaunchKernelGGL(k_cinfo_solve, dim3((cnt + nw - 1) / nw), dim3(64 * nw), cinfo_lds_bytes(p.max_vars), c.stream, a);
        MCML_HIP(hipGetLastError());
        x.plan[1] = items ? 1 : 2; x.plan[4] = waves; x.plan[5] = 2;
    } else {
        // ---- B = ZL' XV, M, its factor, S = R^-1 B on the dense ZL / ZL'
        InfoDenseScope dense(c);
        const bool sparse_ctx = c.sp.active;
        if (sparse_ctx) MCML_TRY(dense.build());
        MCML_REQUIRE(c.ZL.d() && c.ZLT.d() && c.ZL.rows == n && c.ZL.cols == Q, "information: the dense ZL is not resident");
        const EpiAxpby epi{x.S.d(), x.S.ld, 1.0, 0.0};
        MCML_TRY(launch_gemm<false>(c.stream, Q, P, n, c.ZLT.d(), c.ZLT.ld, x.XV.d(), x.XV.ld, epi));
        MCML_TRY(build_M_dense(c, x.v.d(), 1.0, x.M, x.ZLTW, true));
        MCML_TRY(potrf_lower(c, x.M.d(), Q, x.M.ld));                 // a failed pivot raises c.errflag(): read at the end
        MCML_TRY(trsm_left_lower(c, x.M.d(), x.M.ld, Q, x.S.d(), x.S.ld, P));
        x.plan[6] = (long long)(x.M.buf.bytes + x.ZLTW.buf.bytes + (sparse_ctx ? c.ZL.buf.bytes + c.ZLT.buf.bytes : 0));
    }

    // ---- the Gram reduction and the one download
    const int cx = (n + INFO_CHUNK - 1) / INFO_CHUNK, nch = cx + (Q + INFO_CHUNK - 1) / INFO_CHUNK;
    const size_t PP = (size_t)P * P;
    MCML_TRY(x.part.ensure(sizeof(double) * PP * (size_t)nch));
    MCML_TRY(x.res.ensure(sizeof(double) * (PP + 2)));
    hipLaunchKernelGGL(k_info_gram, dim3((unsigned)PP, nch), dim3(256), 0, c.stream, c.X.d(), c.X.ld, x.XV.d(), x.XV.ld, n, x.S.d(),
                       x.S.ld, Q, P, cx, x.part.d());
    MCML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_info_gram_final, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, c.stream, x.part.d(), P, cx, nch,
                       c.errflag(), x.bad.as<int>(), x.res.d());
    MCML_HIP(hipGetLastError());
    std::vector<double> h(PP + 2);
    MCML_TRY(copy_d2h(h.data(), x.res.p, sizeof(double) * h.size(), c.stream));
    MCML_HIP(hipStreamSynchronize(c.stream));
    if (h[PP] != 0.0) {                                               // cleared as check_errflag clears it
        MCML_HIP(hipMemsetAsync(c.errflag(), 0, sizeof(int), c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
    }
    if (h[PP + 1] != 0.0) {
        set_error("information: a weight dhdmu(x' beta) * scale, or its reciprocal, is not finite");
        return MCML_EINVAL;
    }
    if (h[PP] != 0.0) {
        set_error("information: ZL' V ZL + I is not positive definite");
        return MCML_ENOTPD;
    }
    for (int b = 0; b < P; ++b) memcpy(out + (size_t)b * ldo, h.data() + (size_t)b * P, sizeof(double) * (size_t)P);
    return MCML_OK;
}

}  // namespace mcml
