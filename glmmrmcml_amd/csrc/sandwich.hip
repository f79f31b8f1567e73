// sandwich.hip -- the cluster-robust (sandwich) covariance of the fixed effects on the device (a query: DESIGN.md 5.11).
// With eta = X beta (no random-effect term), w, v = 1 / w and Sigma = diag(w) + Z D Z' exactly as the information query has them:
//     e_i = (y_i - h(eta_i)) detadmu(eta_i)        the working residual
//     a   = Sigma^-1 e = v o (e - ZL t),           t = M^-1 ZL' (v o e),   M = I + ZL' V ZL = R R'   (Woodbury, one column)
//     G[c, p] = sum_{i in cluster c} X[i, p] a_i   the cluster scores, observations ascending
//     B   = G' G                                   the meat;  the bread is info_matrix's X' Sigma^-1 X, called as it stands
// The bread comes first: info_matrix leaves v and the factor of M in InfoState (x.M + the inverted diagonal blocks of the Cholesky
// stack on the dense operator, x.f (CompFactors) on the component operator), and the residual column travels in launches of its own:
//   k_sand_resid                    e and v o e, xb_i = row_xb (glm.h) as the information query's weights have it
//   dense operator                  ZL' (v o e) by the MFMA GEMM on c.ZLT with N = 1, trsm_left_lower and trsm_left_lower_trans on
//                                   x.M with m = 1, ZL t by the GEMM on c.ZL with N = 1, k_sand_a_dense.  Every one of these entries
//                                   takes one column as it is (columns past N are neither loaded nor stored): nothing is padded
//   component operator              component.h, "applying a factor", with one column: comp_rhs_csr_launch, comp_solve_launch with
//                                   the back sweep (R_c s = b, R_c' t = s); then k_sand_a_ell (the ELL rows of ZL)
//   k_sand_scores                   G, a wave or a workgroup per (cluster, column) by the largest cluster
//   gram_launch (info.hip)          the meat B[a, b] = sum_c G[c, a] G[c, b], a >= b, mirrored, in chunks of clusters: the
//                                   information query's Gram reduction with U = W = G and no second sum; the flags behind it
// Everything runs on c.stream, no atomics, every sum in a fixed order: two calls give the same bits.  One download of
// P x P + 2 (+ ncl x P) doubles ends the call (query_download, info.hip).  No collective; nothing a sampler, a fit or another
// query reads is changed.  What is this file's own: the residual, the two epilogues a = v o (e - ZL t), the scores, the clusters.
#include "entry.h"
#include "component.h"
#include "dgemm_mfma.h"
#include "glm.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

namespace mcml {

// e_i = (y_i - h(xb_i)) detadmu(xb_i), xb_i = row_xb, and v_i e_i.  An e_i that is not finite raises *bad (every thread that
// stores, stores 1)
__global__ __launch_bounds__(256) void k_sand_resid(const double* X, int ldx, int n, int P, const double* beta, const double* y,
                                                    const double* v, int link_code, double* e, double* ve, int* bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double xb = row_xb(X, ldx, i, P, beta);
    const double ei = (y[i] - glm_mod_inv(xb, link_code)) * glm_detadmu(xb, link_code);
    if (!__builtin_isfinite(ei)) *bad = 1;
    e[i] = ei;
    ve[i] = v[i] * ei;
}

// a_i = v_i (e_i - sum_k ell_val[i + k n] t[ell_col[i + k n]]), k ascending over the W entries of the ELL row (the padding holds
// column 0 and value 0)
__global__ __launch_bounds__(256) void k_sand_a_ell(const int* ell_col, const double* ell_val, int n, int W, const double* t,
                                                    const double* v, const double* e, double* a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double zt = 0;
    for (int k = 0; k < W; ++k) zt += ell_val[i + (size_t)k * n] * t[ell_col[i + (size_t)k * n]];
    a[i] = v[i] * (e[i] - zt);
}

// the dense operator's epilogue: a_i = v_i (e_i - (ZL t)_i)
__global__ __launch_bounds__(256) void k_sand_a_dense(int n, const double* zt, const double* v, const double* e, double* a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v[i] * (e[i] - zt[i]);
}

// ---- the scores.  G[c, p] = sum over the rows of cluster c (cl_rows[cl_ptr[c] .. cl_ptr[c + 1]), ascending) of X[i, p] a_i.
// Two forms by the largest cluster, as cp_waves picks the factor kernels':
//   WG = false   a wave per (cluster, column), four waves per workgroup: lane l adds rows l, l + 64, ... in turn, then wave_sum
//   WG = true    a workgroup per (cluster, column): thread t adds rows t, t + 256, ... in turn, then block_sum
// Either tree depends on the cluster alone, not on the grid.  The workgroup form is taken from SAND_WG_ROWS rows in the largest
// cluster: a guess until measured (config 5 has 10 rows per cluster, config 4 has 400); GLMMR_MCML_SAND_SCORES = wave | wg,
// read per call, forces a form (a test runs both in one process)
constexpr int SAND_WG_ROWS = 128;
constexpr const char* SAND_SCORES_ENV = "GLMMR_MCML_SAND_SCORES";
template <bool WG>
__global__ __launch_bounds__(256) void k_sand_scores(const int* cl_ptr, const int* cl_rows, int ncl, const double* X, int ldx,
                                                     const double* a, double* G, int ldg)
{
    __shared__ double sh[4];
    const int p = blockIdx.y;
    const int c = WG ? (int)blockIdx.x : (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (c >= ncl) return;                            // WG: the whole workgroup; else the whole wave
    const double* col = X + (size_t)p * ldx;
    const int r0 = cl_ptr[c], r1 = cl_ptr[c + 1];
    double acc = 0;
    if (WG) {
        for (int t = r0 + threadIdx.x; t < r1; t += 256) { const int i = cl_rows[t]; acc += col[i] * a[i]; }
        const double r = block_sum(acc, sh);
        if (threadIdx.x == 0) G[c + (size_t)p * ldg] = r;
    } else {
        for (int t = r0 + (threadIdx.x & 63); t < r1; t += 64) { const int i = cl_rows[t]; acc += col[i] * a[i]; }
        const double r = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) G[c + (size_t)p * ldg] = r;
    }
}

// the clusters as a CSR over the observations, rows ascending inside a cluster.  cluster null: the connected components of
// ZL's coupling graph (ComponentPlan::comp_of_row), refused where the context has no plan or an observation has no entry
static int sand_clusters(const Ctx& c, const int* cluster, int ncluster, std::vector<int>& ptr, std::vector<int>& rows)
{
    const int n = c.n;
    if (!cluster) {
        const ComponentPlan& p = c.cp.plan;
        if (!(c.sp.active && c.cp.ready && p.ncomp > 0 && (int)p.comp_of_row.size() == n)) {
            set_error("sandwich: no default clusters: the context does not run the sparse ZL operator, so there is no component "
                      "plan; pass explicit cluster ids");
            return MCML_EINVAL;
        }
        for (int i = 0; i < n; ++i) {
            bool any = false;
            for (int k = 0; k < c.z_width && !any; ++k) any = c.h_zval[i + (size_t)k * n] != 0.0;
            if (!any) {
                set_error("sandwich: no default clusters: observation %d has no entry of ZL and belongs to no component; pass "
                          "explicit cluster ids", i);
                return MCML_EINVAL;
            }
        }
        ptr = p.row_ptr; rows = p.rows;
        return MCML_OK;
    }
    MCML_REQUIRE(ncluster >= 1, "sandwich: ncluster must be at least 1");
    ptr.assign((size_t)ncluster + 1, 0);
    for (int i = 0; i < n; ++i) {
        MCML_REQUIRE(cluster[i] >= 0 && cluster[i] < ncluster, "sandwich: cluster id %d of observation %d is outside [0, %d)",
                     cluster[i], i, ncluster);
        ++ptr[cluster[i] + 1];
    }
    for (int k = 0; k < ncluster; ++k) ptr[k + 1] += ptr[k];
    rows.assign((size_t)n, 0);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int i = 0; i < n; ++i) rows[fill[cluster[i]]++] = i;
    return MCML_OK;
}

int sandwich_matrices(Ctx& c, const double* beta, double var_par, int op, const int* cluster, int ncluster, double* info, int ldi,
                      double* meat, int ldm, double* scores, int lds, int* ncluster_out)
{
    const int n = c.n, Q = c.Q, P = c.P;
    MCML_REQUIRE(n > 0 && P > 0, "sandwich: the context has no model");
    MCML_REQUIRE(beta && info && meat && ldi >= P && ldm >= P, "sandwich: null argument / ldi or ldm too small");
    MCML_REQUIRE(c.have_L, "sandwich: the context holds no L: pass theta or call update_L first");
    MCML_REQUIRE(c.y.d() && (c.flink != 8 || c.y_given.d()), "sandwich: the context holds no y");
    SandwichState& s = c.sand;
    std::vector<int> ptr, rows;
    MCML_TRY(sand_clusters(c, cluster, ncluster, ptr, rows));
    const int ncl = (int)ptr.size() - 1;
    MCML_REQUIRE(!scores || lds >= ncl, "sandwich: lds %d is smaller than the %d clusters", lds, ncl);
    int max_rows = 0;
    for (int k = 0; k < ncl; ++k) max_rows = std::max(max_rows, ptr[k + 1] - ptr[k]);
    const long long plan0[8] = {op, 0, ncl, max_rows, cluster ? 0 : 1, 0, 0, P};
    std::copy(plan0, plan0 + 8, s.plan);

    // ---- the bread: the information query as it stands.  It leaves v, beta and the factor of M in c.info
    std::vector<double> hinfo((size_t)P * P);
    MCML_TRY(info_matrix(c, beta, var_par, op, hinfo.data(), P));
    InfoState& x = c.info;
    const bool comp = x.plan[1] != 0;
    s.plan[1] = x.plan[1]; s.plan[6] = x.plan[6];

    const size_t PP = (size_t)P * P, nres = PP + 2 + (size_t)ncl * P;
    MCML_TRY(s.bad.ensure(sizeof(int)));
    MCML_TRY(s.e.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(s.ve.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(s.a.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(s.t.ensure(sizeof(double) * (size_t)pad_ld(Q)));
    MCML_TRY(s.cl_ptr.ensure(sizeof(int) * ptr.size()));
    MCML_TRY(s.cl_rows.ensure(sizeof(int) * (size_t)n));
    MCML_TRY(s.res.ensure(sizeof(double) * nres));
    MCML_TRY(copy_h2d(s.cl_ptr.p, ptr.data(), sizeof(int) * ptr.size(), c.stream));
    MCML_TRY(copy_h2d(s.cl_rows.p, rows.data(), sizeof(int) * (size_t)n, c.stream));
    MCML_HIP(hipMemsetAsync(s.bad.p, 0, sizeof(int), c.stream));
    MCML_HIP(hipMemsetAsync(s.ve.p, 0, sizeof(double) * (size_t)pad_ld(n), c.stream));       // the K padding of the GEMM
    MCML_HIP(hipMemsetAsync(s.t.p, 0, sizeof(double) * (size_t)pad_ld(Q), c.stream));
    long long launches = 0;

    // ---- e, v o e
    const double* y = c.flink == 8 ? c.y_given.d() : c.y.d();       // gaussian / log: the resident y is log y (model_setup)
    hipLaunchKernelGGL(k_sand_resid, dim3((n + 255) / 256), dim3(256), 0, c.stream, c.X.d(), c.X.ld, n, P, x.beta.d(), y,
                       x.v.d(), c.link_code, s.e.d(), s.ve.d(), s.bad.as<int>());
    MCML_HIP(hipGetLastError());
    ++launches;

    if (comp) {
        // ---- t = M^-1 ZL' (v o e) component by component, a on the ELL rows
        MCML_TRY(comp_rhs_csr_launch(c, s.ve.d(), pad_ld(n), 1, s.t.d(), pad_ld(Q)));
        int form = 0;
        MCML_TRY(comp_solve_launch(c, x.f, s.t.d(), pad_ld(Q), 1, true, &form));
        hipLaunchKernelGGL(k_sand_a_ell, dim3((n + 255) / 256), dim3(256), 0, c.stream, c.sp.ell_col.as<int>(), c.sp.ell_val.d(), n,
                           c.sp.W, s.t.d(), x.v.d(), s.e.d(), s.a.d());
        MCML_HIP(hipGetLastError());
        launches += 3;
    } else {
        // ---- the same on the dense ZL / ZL' (built beside the sparse operator by the information query where the context is
        // sparse, and still resident) and the factor in x.M, whose inverted diagonal blocks the Cholesky stack still holds
        MCML_REQUIRE(c.ZL.d() && c.ZLT.d() && c.ZL.rows == n && c.ZL.cols == Q && x.M.d(), "sandwich: the dense ZL is not resident");
        MCML_TRY(s.zt.ensure(sizeof(double) * (size_t)pad_ld(n)));
        const EpiAxpby rhs{s.t.d(), pad_ld(Q), 1.0, 0.0};
        MCML_TRY(launch_gemm<false>(c.stream, Q, 1, n, c.ZLT.d(), c.ZLT.ld, s.ve.d(), pad_ld(n), rhs));
        MCML_TRY(trsm_left_lower(c, x.M.d(), x.M.ld, Q, s.t.d(), pad_ld(Q), 1));
        MCML_TRY(trsm_left_lower_trans(c, x.M.d(), x.M.ld, Q, s.t.d(), pad_ld(Q), 1));
        const EpiAxpby zt{s.zt.d(), pad_ld(n), 1.0, 0.0};
        MCML_TRY(launch_gemm<false>(c.stream, n, 1, Q, c.ZL.d(), c.ZL.ld, s.t.d(), pad_ld(Q), zt));
        hipLaunchKernelGGL(k_sand_a_dense, dim3((n + 255) / 256), dim3(256), 0, c.stream, n, s.zt.d(), x.v.d(), s.e.d(), s.a.d());
        MCML_HIP(hipGetLastError());
        ++launches;
    }

    // ---- scores, meat and the one download: res = B (P x P) | 2 flags | G (ncl x P)
    double* G = s.res.d() + PP + 2;
    bool wg = max_rows >= SAND_WG_ROWS;
    if (const char* env = getenv(SAND_SCORES_ENV)) {
        if (!strcmp(env, "wave")) wg = false;
        if (!strcmp(env, "wg")) wg = true;
    }
    if (wg) hipLaunchKernelGGL(k_sand_scores<true>, dim3(ncl, P), dim3(256), 0, c.stream, s.cl_ptr.as<int>(), s.cl_rows.as<int>(),
                               ncl, c.X.d(), c.X.ld, s.a.d(), G, ncl);
    else hipLaunchKernelGGL(k_sand_scores<false>, dim3((ncl + 3) / 4, P), dim3(256), 0, c.stream, s.cl_ptr.as<int>(),
                            s.cl_rows.as<int>(), ncl, c.X.d(), c.X.ld, s.a.d(), G, ncl);
    MCML_HIP(hipGetLastError());
    MCML_TRY(gram_launch(c, G, ncl, G, ncl, ncl, nullptr, 0, 0, P, s.part, s.bad.as<int>(), s.res.d()));
    launches += 3;
    s.plan[5] = launches;
    std::vector<double> h;
    MCML_TRY(query_download(c, s.res, P, scores ? (size_t)ncl * P : 0, "sandwich", "a working residual (y - h(x' beta)) detadmu(x' beta)", h));
    copy_columns(info, ldi, hinfo.data(), P, P);
    copy_columns(meat, ldm, h.data(), P, P);
    if (scores) copy_columns(scores, lds, h.data() + PP + 2, ncl, P);
    if (ncluster_out) *ncluster_out = ncl;
    return MCML_OK;
}

}  // namespace mcml
