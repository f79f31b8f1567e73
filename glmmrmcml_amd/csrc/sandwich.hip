// sandwich.hip -- the cluster-robust (sandwich) covariance of the fixed effects on the device (a query: DESIGN.md 5.11).
// With eta = X beta (no random-effect term), w, v = 1 / w and Sigma = diag(w) + Z D Z' exactly as the information query has them:
//     e_i = (y_i - h(eta_i)) detadmu(eta_i)        the working residual
//     a   = Sigma^-1 e = v o (e - ZL t),           t = M^-1 ZL' (v o e),   M = I + ZL' V ZL = R R'   (Woodbury, one column)
//     G[c, p] = sum_{i in cluster c} X[i, p] a_i   the cluster scores, observations ascending
//     B   = G' G                                   the meat;  the bread is info_matrix's X' Sigma^-1 X, called as it stands
// The bread comes first: info_matrix leaves v and the factor of M in InfoState (x.M + the inverted diagonal blocks of the Cholesky
// stack on the dense operator, x.fac / x.fac_ptr on the component operator), and the residual column travels in launches of its own:
//   k_sand_resid                    e and v o e, the xb sum in k_info_weights' order
//   dense operator                  ZL' (v o e) by the MFMA GEMM on c.ZLT with N = 1, trsm_left_lower and trsm_left_lower_trans on
//                                   x.M with m = 1, ZL t by the GEMM on c.ZL with N = 1, k_sand_a_dense.  Every one of these entries
//                                   takes one column as it is (columns past N are neither loaded nor stored): nothing is padded
//   component operator              k_sand_rhs_csr (the CSR rows of ZL', csr_row_sum), k_csand_solve (R_c s = b, R_c' t = s, component
//                                   by component in LDS), k_sand_a_ell (the ELL rows of ZL)
//   k_sand_scores                   G, a wave or a workgroup per (cluster, column) by the largest cluster
//   k_sand_meat, k_sand_meat_final  B[a, b] = sum_c G[c, a] G[c, b], a >= b, mirrored, in chunks of clusters; the flags behind it
// Everything runs on c.stream, no atomics, every sum in a fixed order: two calls give the same bits.  One download of
// P x P + 2 (+ ncl x P) doubles ends the call.  No collective; nothing a sampler, a fit or another query reads is changed.
#include "entry.h"
#include "component.h"
#include "dgemm_mfma.h"
#include "glm.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

namespace mcml {

// e_i = (y_i - h(xb_i)) detadmu(xb_i), xb = X beta (p ascending, as k_info_weights), and v_i e_i.  An e_i that is not finite
// raises *bad (every thread that stores, stores 1)
__global__ __launch_bounds__(256) void k_sand_resid(const double* X, int ldx, int n, int P, const double* beta, const double* y,
                                                    const double* v, int link_code, double* e, double* ve, int* bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double xb = 0;
    for (int p = 0; p < P; ++p) xb += X[i + (size_t)p * ldx] * beta[p];
    const double ei = (y[i] - glm_mod_inv(xb, link_code)) * glm_detadmu(xb, link_code);
    if (!__builtin_isfinite(ei)) *bad = 1;
    e[i] = ei;
    ve[i] = v[i] * ei;
}

// b[q] = sum_t csr_val[t] ve[csr_i[t]]: row q of ZL', observations ascending (k_info_rhs_csr's sum for the one column)
__global__ __launch_bounds__(256) void k_sand_rhs_csr(const int* csr_ptr, const int* csr_i, const double* csr_val, const double* ve,
                                                      int Q, double* b)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    b[q] = csr_row_sum(csr_ptr, csr_i, csr_val, q, [&](int i) { return ve[i]; });
}

// ---- the component solve, forward AND back: R_c s = b_c, R_c' t = s, one column.  R_c is staged from the factor scratch as
// packed rows -- entry (k, i), i <= k, at k (k + 1) / 2 + i -- exactly as k_cinfo_solve stages it.  Two forms, by the plan:
//   staged items   components up to CP_MAX_VARS variables: CSAND_WAVES waves per workgroup, a wave per work item; the item's
//                  components are staged G at a time, each at an ODD stride, and a LANE runs both substitutions of one
//                  component, its vector in LDS as [variable][lane].  In the forward substitution the lane walks a row of its
//                  triangle, in the back substitution a COLUMN (entry (i, k), i descending): either way the lanes of a group
//                  of 32 sit at the SAME offset inside their triangles (lanes whose component is smaller are masked), so their
//                  addresses differ by multiples of the odd stride and fall into 32 different pairs of banks: the odd stride that
//                  keeps the row walk free of conflicts keeps the column walk free of them as well (checked on the address
//                  formula, not measured)
//   one component  up to CP_WIDE_MAX_VARS: one wave per workgroup and component, the vector x[nv] in LDS, the wave works a
//                  step of either substitution together: lane i takes x_i -= R[i, k] x_k (forward, a column of the packed
//                  triangle: the offsets i (i + 1) / 2 of 32 consecutive i are distinct modulo 32, no conflict) or
//                  x_i -= R[k, i] x_k (back, a row: consecutive).  Every x_i receives its updates in the order the lane of the
//                  staged form applies them -- forward k ascending, back k descending -- so the two forms give the same bits
constexpr int CSAND_WAVES = 4;
constexpr int CSAND_R_DOUBLES = 1024;                // a wave's room for staged triangles in the item form
constexpr int csand_stride(int mv) { return (mv * (mv + 1) / 2) | 1; }
constexpr int csand_r_doubles(int mv) { return csand_stride(mv) < CSAND_R_DOUBLES ? CSAND_R_DOUBLES : csand_stride(mv); }
constexpr int csand_item_lds_bytes(int mv) { return 8 * CSAND_WAVES * (mv * 64 + csand_r_doubles(mv)); }
constexpr int csand_wide_lds_bytes(int mv) { return 8 * (csand_stride(mv) + mv); }
static_assert(csand_item_lds_bytes(CP_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_csand_solve, staged items at their cap");
static_assert(csand_wide_lds_bytes(CP_WIDE_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_csand_solve, one wave at the cap");

struct CsandArgs {
    CompView cv;                         // WIDE: component blockIdx.x; else a wave takes work item t = components [item_ptr[t], item_ptr[t + 1])
    const int* fac_ptr;                  // InfoState: the factors of lac_factor_launch, lower triangles, leading dimension nv_c
    const double* fac;
    double* t;                           // Q, in: b, out: t
};

// packed rows of the lower triangle of F (nv x nv, column-major) -> Rs, by the whole wave
__device__ __forceinline__ void csand_stage(const double* F, int nv, double* Rs, int lane)
{
    for (int e = lane; e < nv * nv; e += 64) {
        const int i = e % nv, j = e / nv;
        if (i >= j) Rs[i * (i + 1) / 2 + j] = F[e];
    }
}

// WIDE: grid ncomp, 64 threads, csand_wide_lds_bytes(max_vars); else grid ceil(nitems / CSAND_WAVES), 64 * CSAND_WAVES threads,
// csand_item_lds_bytes(max_vars) of dynamic LDS.  No workgroup barrier
template <bool WIDE>
__global__ __launch_bounds__(WIDE ? 64 : 64 * CSAND_WAVES) void k_csand_solve(CsandArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double csand_lds[];
    const int lane = threadIdx.x & 63;
    const int mv = a.cv.max_vars, stride = csand_stride(mv);
    if (WIDE) {
        const int comp = blockIdx.x;
        if (comp >= a.cv.ncomp) return;
        const int v0 = a.cv.var_ptr[comp], nv = a.cv.var_ptr[comp + 1] - v0;     // 1 <= nv <= mv
        double* R = csand_lds;
        double* x = csand_lds + stride;
        csand_stage(a.fac + a.fac_ptr[comp], nv, R, lane);
        for (int k = lane; k < nv; k += 64) x[k] = a.t[a.cv.vars[v0 + k]];
        wave_lds_sync();
        for (int k = 0; k < nv; ++k) {                                           // R s = b
            const double sk = x[k] / R[k * (k + 1) / 2 + k];
            wave_lds_sync();                                                     // every lane has read x[k]
            if (lane == 0) x[k] = sk;
            for (int i = k + 1 + lane; i < nv; i += 64) x[i] -= R[i * (i + 1) / 2 + k] * sk;
            wave_lds_sync();
        }
        for (int k = nv - 1; k >= 0; --k) {                                      // R' t = s
            const double* row = R + k * (k + 1) / 2;
            const double tk = x[k] / row[k];
            wave_lds_sync();
            if (lane == 0) x[k] = tk;
            for (int i = lane; i < k; i += 64) x[i] -= row[i] * tk;
            wave_lds_sync();
        }
        for (int k = lane; k < nv; k += 64) a.t[a.cv.vars[v0 + k]] = x[k];
        return;
    }
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blockIdx.x * CSAND_WAVES + w;
    if (item >= a.cv.nitems) return;
    const int rd = csand_r_doubles(mv);
    double* x = csand_lds + (size_t)w * (mv * 64 + rd);                          // [variable][lane]
    double* R = x + mv * 64;                                                     // slot s at R + s stride
    const int G = rd / stride < 64 ? rd / stride : 64;                           // components staged side by side, >= 1
    const int c0 = a.cv.item_ptr[item], c1 = a.cv.item_ptr[item + 1];
    for (int cs = c0; cs < c1; cs += G) {
        const int g = c1 - cs < G ? c1 - cs : G;
        wave_lds_sync();                             // the previous group's reads of R
        for (int s = 0; s < g; ++s)
            csand_stage(a.fac + a.fac_ptr[cs + s], a.cv.var_ptr[cs + s + 1] - a.cv.var_ptr[cs + s], R + s * stride, lane);
        wave_lds_sync();
        if (lane < g) {
            const int v0 = a.cv.var_ptr[cs + lane], nv = a.cv.var_ptr[cs + lane + 1] - v0;
            const double* Rs = R + lane * stride;
            // s_k = (b_k - sum_{i < k} R_c[k, i] s_i) / R_c[k, k], i ascending
            for (int k = 0; k < nv; ++k) {
                const double* row = Rs + k * (k + 1) / 2;
                double acc = a.t[a.cv.vars[v0 + k]];
                for (int i = 0; i < k; ++i) acc -= row[i] * x[i * 64 + lane];
                x[k * 64 + lane] = acc / row[k];
            }
            // t_k = (s_k - sum_{i > k} R_c[i, k] t_i) / R_c[k, k], i descending: column k of the packed triangle
            for (int k = nv - 1; k >= 0; --k) {
                double acc = x[k * 64 + lane];
                for (int i = nv - 1; i > k; --i) acc -= Rs[i * (i + 1) / 2 + k] * x[i * 64 + lane];
                acc = acc / Rs[k * (k + 1) / 2 + k];
                x[k * 64 + lane] = acc;
                a.t[a.cv.vars[v0 + k]] = acc;
            }
        }
    }
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

// ---- the meat, in the shape of k_info_gram / k_info_gram_final.  Block (a + b P, ch), a >= b: the partial sum of SAND_CHUNK
// clusters of G[:, a] G[:, b] in the fixed order of block_sum
constexpr int SAND_CHUNK = 2048;
__global__ __launch_bounds__(256) void k_sand_meat(const double* G, int ldg, int ncl, int P, double* part)
{
    __shared__ double sh[4];
    const int a = blockIdx.x % P, b = blockIdx.x / P, ch = blockIdx.y;
    if (a < b) return;                               // the whole block
    const double *u = G + (size_t)a * ldg, *w = G + (size_t)b * ldg;
    const int r0 = ch * SAND_CHUNK, r1 = r0 + SAND_CHUNK < ncl ? r0 + SAND_CHUNK : ncl;
    double acc = 0;
    for (int c = r0 + threadIdx.x; c < r1; c += 256) acc += u[c] * w[c];
    const double r = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * gridDim.y + ch] = r;
}

// out[a, b] = out[b, a] = the sum of the partials, ascending, a >= b; the two flags of the call ride behind the matrix:
// out[P P] = the context's "not positive definite" flag, out[P P + 1] = the residuals'
__global__ __launch_bounds__(256) void k_sand_meat_final(const double* part, int P, int nch, const int* errflag, const int* bad,
                                                         double* out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0) { out[(size_t)P * P] = (double)*errflag; out[(size_t)P * P + 1] = (double)*bad; }
    if (t >= P * P) return;
    const int a = t % P, b = t / P;
    if (a < b) return;
    const double* p = part + (size_t)t * nch;
    double s = 0;
    for (int c = 0; c < nch; ++c) s += p[c];
    out[a + (size_t)b * P] = s;
    out[b + (size_t)a * P] = s;
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
    const int nch = (ncl + SAND_CHUNK - 1) / SAND_CHUNK;
    MCML_TRY(s.bad.ensure(sizeof(int)));
    MCML_TRY(s.e.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(s.ve.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(s.a.ensure(sizeof(double) * (size_t)pad_ld(n)));
    MCML_TRY(s.t.ensure(sizeof(double) * (size_t)pad_ld(Q)));
    MCML_TRY(s.cl_ptr.ensure(sizeof(int) * ptr.size()));
    MCML_TRY(s.cl_rows.ensure(sizeof(int) * (size_t)n));
    MCML_TRY(s.part.ensure(sizeof(double) * PP * (size_t)nch));
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
        const ComponentPlan& p = c.cp.plan;
        hipLaunchKernelGGL(k_sand_rhs_csr, dim3((Q + 255) / 256), dim3(256), 0, c.stream, c.sp.csr_ptr.as<int>(),
                           c.sp.csr_i.as<int>(), c.sp.csr_val.d(), s.ve.d(), Q, s.t.d());
        MCML_HIP(hipGetLastError());
        const CsandArgs a{comp_view(c), x.fac_ptr.as<int>(), x.fac.d(), s.t.d()};
        if (p.feasible) {                                             // max_vars <= CP_MAX_VARS: the plan's work items are built
            MCML_TRY(ensure_dynamic_lds((const void*)k_csand_solve<false>, csand_item_lds_bytes(CP_MAX_VARS)));
            hipLaunchKernelGGL(k_csand_solve<false>, dim3((a.cv.nitems + CSAND_WAVES - 1) / CSAND_WAVES), dim3(64 * CSAND_WAVES),
                               csand_item_lds_bytes(p.max_vars), c.stream, a);
        } else {
            MCML_REQUIRE(p.max_vars <= CP_WIDE_MAX_VARS, "sandwich: a component of %d variables on the component operator", p.max_vars);
            MCML_TRY(ensure_dynamic_lds((const void*)k_csand_solve<true>, csand_wide_lds_bytes(CP_WIDE_MAX_VARS)));
            hipLaunchKernelGGL(k_csand_solve<true>, dim3(a.cv.ncomp), dim3(64), csand_wide_lds_bytes(p.max_vars), c.stream, a);
        }
        MCML_HIP(hipGetLastError());
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
    hipLaunchKernelGGL(k_sand_meat, dim3((unsigned)PP, nch), dim3(256), 0, c.stream, G, ncl, ncl, P, s.part.d());
    MCML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sand_meat_final, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, c.stream, s.part.d(), P, nch, c.errflag(),
                       s.bad.as<int>(), s.res.d());
    MCML_HIP(hipGetLastError());
    launches += 3;
    s.plan[5] = launches;
    std::vector<double> h(scores ? nres : PP + 2);
    MCML_TRY(copy_d2h(h.data(), s.res.p, sizeof(double) * h.size(), c.stream));
    MCML_HIP(hipStreamSynchronize(c.stream));
    if (h[PP] != 0.0) {                                               // cleared as check_errflag clears it
        MCML_HIP(hipMemsetAsync(c.errflag(), 0, sizeof(int), c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
    }
    if (h[PP + 1] != 0.0) {
        set_error("sandwich: a working residual (y - h(x' beta)) detadmu(x' beta) is not finite");
        return MCML_EINVAL;
    }
    if (h[PP] != 0.0) {
        set_error("sandwich: ZL' V ZL + I is not positive definite");
        return MCML_ENOTPD;
    }
    for (int b = 0; b < P; ++b) {
        memcpy(info + (size_t)b * ldi, hinfo.data() + (size_t)b * P, sizeof(double) * (size_t)P);
        memcpy(meat + (size_t)b * ldm, h.data() + (size_t)b * P, sizeof(double) * (size_t)P);
        if (scores) memcpy(scores + (size_t)b * lds, h.data() + PP + 2 + (size_t)b * ncl, sizeof(double) * (size_t)ncl);
    }
    if (ncluster_out) *ncluster_out = ncl;
    return MCML_OK;
}

}  // namespace mcml
