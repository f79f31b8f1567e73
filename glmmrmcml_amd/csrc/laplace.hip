// laplace.hip -- the Laplace-approximation fits mcml_la / mcml_la_nr on the device.
//   functors  LA_likelihood / LA_likelihood_cov / LA_likelihood_btheta   likelihood.h:112-230
//   steps     la_optim / la_optim_cov / la_optim_bcov / hess_la / mcnr_b mcmloptim.h:116-195,238-293
//   drivers   mcml_la / mcml_la_nr                                       src/mcml_la.cpp:28-290
//   state     mcmlModel ctor, update_W(i, useL), log_grad(v, usezl=false) mcmlmodel.h:51-134,156-168
// Every objective evaluation runs on the device (Z, X, y, L, ZL resident) and returns one
// scalar; the Q x Q x n product ZL' W ZL and its Cholesky use the same MFMA GEMM / potrf as
// the MCML path, the vector-sized pieces are plain streaming kernels.  Opt-in (glmmr_mcml_ctx_set_la_operator, DESIGN.md
// 5.5): on a block-structured design the same statements run on the sparse ZL operator and factorise M component by
// component (component.hip, lac_factor_launch: a wave per component up to CP_MAX_VARS variables under "component", a wave or a
// workgroup up to CP_WIDE_MAX_VARS under "component_wide"); nothing of size Q x n or Q x Q is then built per evaluation.
//
// Reference behaviour reproduced on purpose (also restated in oracle/la.py):
//   * v = u column 0 is the whitened effect, yet update_W(useL = false) forms Z v and
//     log_grad(v, false) forms xb + Z v and -D v (mcmlmodel.h:121,165-166);
//   * D_ is built once from the starting theta and never refreshed (src/mcml_la.cpp:247);
//   * var_par starts at 1 whatever `start` holds (src/mcml_la.cpp:45,191);
//   * at convergence L keeps the previous iteration's theta, and u = L v uses it (:76-97,:147).
// Departures: a theta with a non-positive-definite block is an infinitely bad objective
// instead of NaN; after an optimisation the model is left at the optimum (the reference
// leaves it at rminqa's last evaluated point, which is optimiser-specific); hess_la for the
// beta family is refused (its functor mis-sizes theta, likelihood.h:196-201).
#include "entry.h"
#include "dgemm_mfma.h"
#include "component.h"
#include "glm.h"
#include "optim.h"
#include "parspace.h"
#include "host_linalg.h"
#include "reduce.h"
#include "vecops.h"
#include <algorithm>
#include <cmath>

namespace mcml {

// ------------------------------------------------------------------ kernels
// out_i = sum_k val[i + k n] v[idx[i + k n]], k ascending: ZL v over the ELL rows of ZL (sp.ell_col / sp.ell_val, width
// sp.W) and Z v over the padded-CSR rows of Z (z_idx / z_val, width z_width); padding entries hold the value 0
__global__ __launch_bounds__(256) void k_lac_rows_times_v(const int* idx, const double* val, int n, int width, const double* v,
                                                          double* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0;
    for (int k = 0; k < width; ++k) s += val[i + (size_t)k * n] * v[idx[i + (size_t)k * n]];
    out[i] = s;
}

// out_q = post (ZL' score)_q - (D0 v)_q.  ZL' by its CSR rows, observations ascending.  D0 = L L' at the starting theta
// couples the variables of a COVARIANCE block, which can span several components (a variable whose observations were
// dropped is a component of its own): row q of D0 over the columns [row_start[q], row_end[q]) of its block
__global__ __launch_bounds__(256) void k_lac_vgrad(const int* csr_ptr, const int* csr_i, const double* csr_val, const double* score,
                                                   double post, const double* D0, int ldd, const int* row_start, const int* row_end,
                                                   const double* v, int Q, double* out)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const double s = csr_row_sum(csr_ptr, csr_i, csr_val, q, [&](int i) { return score[i]; });
    double d = 0;
    for (int j = row_start[q]; j < row_end[q]; ++j) d += D0[q + (size_t)j * ldd] * v[j];
    out[q] = post * s - d;
}

// partial sums of log f(y_i | xb_i + zv_i)
__global__ __launch_bounds__(256) void k_la_ll(const double* y, const double* xb, const double* zv, int n,
                                               double var_par, int flink, double* partials)
{
    __shared__ double sh[4];
    double acc = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        acc += glm_logpdf(y[i], xb[i] + zv[i], var_par, flink);
    const double r = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// W_i = 1 / (dhdmu(xb_i + zv_i) nvar)   (mcmlmodel.h:122-133)
__global__ void k_la_W(const double* xb, const double* zv, int n, int flink, double nvar, double* W)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) W[i] = 1 / (glm_dhdmu(xb[i] + zv[i], flink) * nvar);
}

// out[q + i ld] = A[q + i ld] W[i]   (columns = observations)
__global__ void k_la_scale_cols(const double* A, int lda, int rows, int cols, const double* W, double* out, int ldo)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows) return;
    for (int i = blockIdx.y; i < cols; i += gridDim.y) out[q + (size_t)i * ldo] = A[q + (size_t)i * lda] * W[i];
}

__global__ void k_la_add_identity(double* M, int ld, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) M[i + (size_t)i * ld] += 1.0;
}

// mcnr_b's per-observation pieces (mcmloptim.h:248-266): resid, Wu = W detadmu resid, score(xb + Zv)
__global__ void k_la_nr_obs(const double* y, const double* xb, const double* zlv, const double* zv, const double* W,
                            int n, int flink, int link_code, double var_par, double* resid, double* Wu, double* score)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double eta = xb[i] + zlv[i];
    const double r = y[i] - glm_mod_inv(eta, link_code);
    resid[i] = r;
    Wu[i] = W[i] * glm_detadmu(eta, link_code) * r;
    score[i] = flink == 12 ? glm_score_beta(y[i], xb[i] + zv[i], var_par) : glm_score(y[i], xb[i] + zv[i], flink);
}

// X' diag(W) X (P x P) and X' Wu (P): tiny P, one block per (a, b) pair / per a
__global__ __launch_bounds__(256) void k_la_xtwx(const double* X, int ldx, int n, int P, const double* W,
                                                 const double* Wu, double* out /* P*P + P */)
{
    __shared__ double sh[4];
    const int idx = blockIdx.x;
    double acc = 0;
    if (idx < P * P) {
        const int a = idx % P, b = idx / P;
        for (int i = threadIdx.x; i < n; i += 256) acc += X[i + (size_t)a * ldx] * W[i] * X[i + (size_t)b * ldx];
    } else {
        const int a = idx - P * P;
        for (int i = threadIdx.x; i < n; i += 256) acc += X[i + (size_t)a * ldx] * Wu[i];
    }
    const double r = block_sum(acc, sh);
    if (threadIdx.x == 0) out[idx] = r;
}

// M = ZL' diag(W) ZL + I from the current c.ZL / c.ZLT (ctx.h): the Laplace fits' M with their per-observation weights, the
// exact conditional draws' (hmc_exact.h) with the constant 1 / sigma^2, which is the product's alpha
int build_M_dense(Ctx& c, const double* W, double w0, DevMat& M, DevMat& ZLTW, bool lower_only)
{
    const int n = c.n, Q = c.Q;
    MCML_TRY(M.alloc(Q, Q));
    const double* A = c.ZLT.d(); int lda = c.ZLT.ld;
    if (W) {
        MCML_TRY(ZLTW.alloc(Q, n, 32));
        if ((size_t)ZLTW.cols_alloc > (size_t)n)
            MCML_HIP(hipMemsetAsync(ZLTW.at(0, n), 0, sizeof(double) * (size_t)ZLTW.ld * (ZLTW.cols_alloc - n), c.stream));
        int gy = n < 1024 ? n : 1024;
        hipLaunchKernelGGL(k_la_scale_cols, dim3((Q + 255) / 256, gy), dim3(256), 0, c.stream, c.ZLT.d(), c.ZLT.ld, Q, n,
                           W, ZLTW.d(), ZLTW.ld);
        MCML_HIP(hipGetLastError());
        A = ZLTW.d(); lda = ZLTW.ld;
    }
    if (lower_only) MCML_HIP(hipMemsetAsync(M.d(), 0, sizeof(double) * (size_t)M.ld * Q, c.stream));
    EpiAxpby epi{M.d(), M.ld, W ? 1.0 : w0, 0.0};
    MCML_TRY(launch_gemm<false>(c.stream, Q, Q, n, A, lda, c.ZL.d(), c.ZL.ld, epi, lower_only));
    hipLaunchKernelGGL(k_la_add_identity, dim3((Q + 255) / 256), dim3(256), 0, c.stream, M.d(), M.ld, Q);
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

// ------------------------------------------------------------------ state
struct LaFit {
    Ctx& c;
    int n, Q, P, R, flink, link_code;
    std::vector<double> beta, theta, theta_model;   // theta_model: the theta the model's L / ZL belong to
    double sigma = 0, var_par = 1.0;
    bool model_L_valid = false;                     // c.L / c.ZL / c.ZLT currently hold L(theta_model)
    int trace = 0, maxfun = 0;
    DevBuf v, W, zv, tmpn, tmpn2, tmpn3, tmpq, tmpq2, part, small;
    DevMat M, ZLTW, D0;
    std::vector<double> hv;                         // host copy of v
    bool comp = false;                              // the component operator (component.h) instead of the dense ZL / M
    int waves = 0;                                  // its form: 1 k_lac_factor, 4 k_lac_factor_wg; 0 with the dense operator
    DevBuf lac_ld;                                  // its per-component log-determinants
    size_t zl_bytes0 = 0;                           // what c.ZL + c.ZLT held when the call began

    LaFit(Ctx& ctx) : c(ctx), n(ctx.n), Q(ctx.Q), P(ctx.P), R(ctx.cov.npar), flink(ctx.flink), link_code(ctx.link_code)
    {
        zl_bytes0 = c.ZL.buf.bytes + c.ZLT.buf.bytes;
        c.la_last_op = 0; c.la_waves = 0; c.la_launches = 0; c.la_dense_bytes = 0;
    }
    // glmmr_mcml_dbg_la_plan: the dense matrices this call allocated (component) or worked on (dense)
    ~LaFit()
    {
        const size_t zl = c.ZL.buf.bytes + c.ZLT.buf.bytes;
        c.la_dense_bytes = (long long)(M.buf.bytes + ZLTW.buf.bytes + (comp ? zl - zl_bytes0 : zl));
    }

    int nblk() const { int b = (n + 255) / 256; return b > 1024 ? 1024 : (b < 1 ? 1 : b); }

    int init(const double* start)
    {
        parse_start(start, P, R, glm_is_gaussian(flink), &beta, &theta, &sigma);
        theta_model = theta;
        var_par = 1.0;
        hv.assign(Q, 0.0);
        MCML_TRY(v.ensure(sizeof(double) * (size_t)(Q + 64)));
        MCML_TRY(W.ensure(sizeof(double) * (size_t)n));
        MCML_TRY(zv.ensure(sizeof(double) * (size_t)n));
        MCML_TRY(tmpn.ensure(sizeof(double) * (size_t)n));
        MCML_TRY(tmpn2.ensure(sizeof(double) * (size_t)n));
        MCML_TRY(tmpn3.ensure(sizeof(double) * (size_t)n));
        MCML_TRY(tmpq.ensure(sizeof(double) * (size_t)(Q + 64)));
        MCML_TRY(tmpq2.ensure(sizeof(double) * (size_t)(Q + 64)));
        MCML_TRY(part.ensure(sizeof(double) * (size_t)std::max(1100, (Q + 255) / 256)));   // ll_and_vv: nblk() <= 1024 | Q / 256 partials
        MCML_TRY(small.ensure(sizeof(double) * (size_t)(P * P + P + 16)));
        MCML_HIP(hipMemsetAsync(v.p, 0, sizeof(double) * (size_t)(Q + 64), c.stream));
        // the component operator: asked for, and the model has the sparse ZL with a component plan its kernel takes (L
        // always comes from theta here: gen_L).  Otherwise, silently, the dense ZL as ever.  "component" is the one-wave
        // kernel and its cap; "component_wide" takes components up to CP_WIDE_MAX_VARS and picks the form (cp_waves)
        if (c.la_mode == 1 || c.la_mode == 2) {
            MCML_TRY(model_sparse_setup(c));
            comp = c.sp.possible && c.cp.ready && (c.la_mode == 2 ? c.cp.plan.records : c.cp.plan.feasible);
        }
        if (comp) {
            MCML_TRY(lac_ld.ensure(sizeof(double) * (size_t)c.cp.plan.ncomp));
            waves = c.la_mode == 2 ? cp_waves(c.cp.plan, cp_forced_waves(CP_LA_WAVES_ENV)) : 1;
        }
        c.la_last_op = comp ? c.la_mode : 0;
        c.la_waves = waves;
        c.no_sparse_zl = !comp;                                   // the dense path works on the dense ZL
        // D_ = L L' at the starting theta (mcmlmodel.h:71); genD(chol = false) gives it directly
        MCML_TRY(mvn_gen_L(c, theta.data(), false));
        MCML_TRY(D0.alloc(Q, Q));
        MCML_HIP(hipMemcpyAsync(D0.d(), c.L.d(), sizeof(double) * (size_t)c.L.ld * Q, hipMemcpyDeviceToDevice, c.stream));
        model_L_valid = false;
        MCML_TRY(ensure_model_L());
        MCML_TRY(model_update_beta(c, beta.data()));
        MCML_TRY(update_W(false));                                // mcmlmodel.h:94
        return MCML_OK;
    }

    int gen_L(const double* th)                                   // c.L, c.ZL, c.ZLT <- theta
    {
        MCML_TRY(mvn_gen_L(c, th, true));
        MCML_TRY(model_update_L(c));
        MCML_REQUIRE(!comp || c.sp.active, "mcml_la: the sparse ZL operator did not follow L");
        model_L_valid = false;
        return MCML_OK;
    }
    int ensure_model_L()
    {
        if (model_L_valid) return MCML_OK;
        MCML_TRY(gen_L(theta_model.data()));
        model_L_valid = true;
        return MCML_OK;
    }
    int set_v(const double* host_v)
    {
        hv.assign(host_v, host_v + Q);
        MCML_TRY(copy_h2d(v.p, hv.data(), sizeof(double) * (size_t)Q, c.stream));
        return MCML_OK;
    }
    int get_v()
    {
        MCML_TRY(copy_d2h(hv.data(), v.p, sizeof(double) * (size_t)Q, c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
        return MCML_OK;
    }
    int rows_times_v(const DevBuf& idx, const DevBuf& val, int width, double* out)   // the component operator's products with v
    {
        hipLaunchKernelGGL(k_lac_rows_times_v, dim3((n + 255) / 256), dim3(256), 0, c.stream, idx.as<int>(), val.d(), n, width,
                           v.d(), out);
        MCML_HIP(hipGetLastError());
        return MCML_OK;
    }
    // out = ZL v from the current c.ZLT (Q x n): column i of ZLT is row i of ZL
    int zl_times_v(double* out)
    {
        if (comp) return rows_times_v(c.sp.ell_col, c.sp.ell_val, c.sp.W, out);
        return dev_gemv_t(c, c.ZLT.d(), c.ZLT.ld, Q, n, v.d(), out, 1.0, 0.0);
    }
    int z_times_v(double* out)
    {
        if (comp) return rows_times_v(c.z_idx, c.z_val, c.z_width, out);
        return dev_gemv_n(c, c.Z.d(), c.Z.ld, n, Q, v.d(), out);
    }
    int scalar_from(const double* dev, double* host)
    {
        MCML_TRY(copy_d2h(host, dev, sizeof(double), c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
        return MCML_OK;
    }

    // mcmlmodel.h:120-134; useL needs the MODEL's ZL
    int update_W(bool useL)
    {
        if (useL) { MCML_TRY(ensure_model_L()); MCML_TRY(zl_times_v(zv.d())); }
        else MCML_TRY(z_times_v(zv.d()));
        double nvar = 1.0;
        if (glm_is_gaussian(flink)) nvar = var_par * var_par;
        else if (flink == 12) nvar = 1 + var_par;
        hipLaunchKernelGGL(k_la_W, dim3((n + 255) / 256), dim3(256), 0, c.stream, c.xb.d(), zv.d(), n, flink, nvar, W.d());
        MCML_HIP(hipGetLastError());
        return MCML_OK;
    }

    // sum_i log f(y_i | xb_i + (ZL v)_i) with the CURRENT c.ZLT, and v'v
    int ll_and_vv(double* ll, double* vv)
    {
        MCML_TRY(zl_times_v(tmpn.d()));
        const int nb = nblk();
        hipLaunchKernelGGL(k_la_ll, dim3(nb), dim3(256), 0, c.stream, c.y.d(), c.xb.d(), tmpn.d(), n, var_par, flink, part.d());
        MCML_HIP(hipGetLastError());
        MCML_TRY(dev_sum(c, part.d(), nb, small.d()));
        const int qb = (Q + 255) / 256;                          // v as one column: a partial per 256 entries (part: init)
        MCML_TRY(dev_sumsq_partials(c, v.d(), Q, Q, 1, qb, 1, part.d()));
        MCML_TRY(dev_sum(c, part.d(), qb, small.d() + 1));
        double h[2];
        MCML_TRY(copy_d2h(h, small.p, sizeof(double) * 2, c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
        *ll = h[0]; *vv = h[1];
        return MCML_OK;
    }

    // M = ZL' W ZL + I from the current c.ZL / c.ZLT
    int build_M() { return build_M_dense(c, W.d(), 1.0, M, ZLTW, false); }
    // every M_c built and factorised from the current record values and W (component.h); with g, x = M^-1 g as well
    int lac_factor(const double* g, double* x)
    {
        return lac_factor_launch(c, W.d(), 1.0, g, x, lac_ld.d(), nullptr, nullptr, waves, &c.la_launches);
    }
    // a non-positive pivot of some M_c, as potrf_lower_checked reports one of M; synchronises the stream
    int lac_check() { return check_errflag(c, "mcml_la: ZL' W ZL + I is not positive definite"); }
    int logdet_M(double* out)
    {
        if (comp) {
            MCML_TRY(lac_factor(nullptr, nullptr));
            MCML_TRY(dev_sum(c, lac_ld.d(), c.cp.plan.ncomp, small.d() + 2));
            MCML_TRY(copy_d2h(out, small.d() + 2, sizeof(double), c.stream));
            return lac_check();
        }
        MCML_TRY(build_M());
        int rc = potrf_lower_checked(c, M.d(), Q, M.ld);
        if (rc) return rc;
        MCML_TRY(dev_logdet_chol(c, M.d(), M.ld, Q, small.d() + 2));       // moremaths.h:105-116
        return scalar_from(small.d() + 2, out);
    }

    // LA_likelihood (likelihood.h:112-140): par = (beta, v); uses the model's ZL
    int obj_bv(const std::vector<double>& par, double* val)
    {
        MCML_TRY(ensure_model_L());
        MCML_TRY(model_update_beta(c, par.data()));
        MCML_TRY(set_v(par.data() + P));
        double ll, vv;
        MCML_TRY(ll_and_vv(&ll, &vv));
        *val = -1.0 * (ll - 0.5 * vv);
        return MCML_OK;
    }
    // shared tail of LA_likelihood_cov / _btheta: theta -> L, ZL; ll - v'v/2 - logdet/2
    int obj_theta_tail(const double* th, double* val)
    {
        int rc = gen_L(th);
        if (rc == MCML_ENOTPD) { *val = HUGE_VAL; return MCML_OK; }
        MCML_TRY(rc);
        double ll, vv, ld;
        MCML_TRY(ll_and_vv(&ll, &vv));
        rc = logdet_M(&ld);
        if (rc == MCML_ENOTPD) { *val = HUGE_VAL; return MCML_OK; }
        MCML_TRY(rc);
        *val = -1 * (ll - 0.5 * vv - 0.5 * ld);
        return MCML_OK;
    }
    // LA_likelihood_cov (likelihood.h:142-183): par = (theta[, var_par])
    int obj_cov(const std::vector<double>& par, double* val)
    {
        const int Rp = glm_has_var_par(flink) ? (int)par.size() - 1 : (int)par.size();
        if (glm_has_var_par(flink)) var_par = par[Rp];
        return obj_theta_tail(par.data(), val);
    }
    // LA_likelihood_btheta (likelihood.h:185-230): par = (beta, theta[, var_par if gaussian])
    int obj_btheta(const std::vector<double>& par, double* val)
    {
        if (glm_is_gaussian(flink)) var_par = par.back();
        MCML_TRY(model_update_beta(c, par.data()));
        MCML_TRY(update_W(false));
        return obj_theta_tail(par.data() + P, val);
    }

    // mcmloptim.h:116-129: the (beta, v) space is all free
    int la_optim()
    {
        std::vector<double> x(beta);
        x.insert(x.end(), hv.begin(), hv.end());
        std::vector<double> lo(x.size(), -HUGE_VAL), up(x.size(), HUGE_VAL);
        objective_fn f = [&](const std::vector<double>& par, double* val) { return obj_bv(par, val); };
        BobyqaResult r;
        MCML_TRY(bobyqa(f, x, lo, up, bopts(trace, maxfun), &r));
        beta.assign(r.x.begin(), r.x.begin() + P);
        MCML_TRY(set_v(r.x.data() + P));
        return MCML_OK;
    }
    // bobyqa over a space (parspace.h); the model is left at the optimum
    int minimise(const objective_fn& f, const ParSpace& sp)
    {
        MCML_TRY(sp.minimise(f, bopts(trace, maxfun), 0, &beta, &theta, &sigma));
        if (sp.has_sigma) var_par = sigma;
        return MCML_OK;
    }
    // mcmloptim.h:131-151
    int la_optim_cov()
    {
        objective_fn f = [&](const std::vector<double>& par, double* val) { return obj_cov(par, val); };
        return minimise(f, ParSpace(0, R, glm_has_var_par(flink)));
    }
    // mcmloptim.h:153-178
    int la_optim_bcov()
    {
        objective_fn f = [&](const std::vector<double>& par, double* val) { return obj_btheta(par, val); };
        return minimise(f, ParSpace(P, R, glm_is_gaussian(flink)));
    }
    // mcmloptim.h:180-195
    int hess_la(double tol, std::vector<double>* H)
    {
        if (flink == 12) { set_error("hess_la: the beta family is not built (the reference functor mis-sizes theta)"); return MCML_EUNSUPPORTED; }
        const ParSpace::Point p = ParSpace(P, R, glm_has_var_par(flink)).pack(beta, theta, sigma);
        std::vector<double> nd(p.x.size(), tol);
        objective_fn f = [&](const std::vector<double>& par, double* val) { return obj_btheta(par, val); };
        return fd_hessian(f, p.x, nd, false, p.lower, p.upper, H);      // without bounds, as the reference
    }

    // mcmloptim.h:238-293
    int mcnr_b()
    {
        MCML_TRY(ensure_model_L());
        MCML_TRY(zl_times_v(tmpn.d()));                           // zd = ZL v
        MCML_TRY(z_times_v(zv.d()));                              // Z v (log_grad with usezl = false)
        hipLaunchKernelGGL(k_la_nr_obs, dim3((n + 255) / 256), dim3(256), 0, c.stream, c.y.d(), c.xb.d(), tmpn.d(), zv.d(),
                           W.d(), n, flink, link_code, var_par, tmpn2.d(), tmpn3.d(), tmpn.d());
        MCML_HIP(hipGetLastError());
        // tmpn2 = resid, tmpn3 = Wu, tmpn = score(xb + Z v)
        hipLaunchKernelGGL(k_la_xtwx, dim3(P * P + P), dim3(256), 0, c.stream, c.X.d(), c.X.ld, n, P, W.d(), tmpn3.d(), small.d());
        MCML_HIP(hipGetLastError());
        std::vector<double> st((size_t)P * P + P), resid(n);
        MCML_TRY(copy_d2h(st.data(), small.p, sizeof(double) * st.size(), c.stream));
        MCML_TRY(copy_d2h(resid.data(), tmpn2.p, sizeof(double) * (size_t)n, c.stream));
        if (comp) {
            // vgrad = -D0 v + post * ZL' score (D0 by covariance blocks), vincr = M^-1 vgrad component by component
            hipLaunchKernelGGL(k_lac_vgrad, dim3((Q + 255) / 256), dim3(256), 0, c.stream, c.sp.csr_ptr.as<int>(),
                               c.sp.csr_i.as<int>(), c.sp.csr_val.d(), tmpn.d(), glm_score_post(var_par, flink), D0.d(), D0.ld,
                               c.sp.row_start.as<int>(), c.sp.row_end.as<int>(), v.d(), Q, tmpq2.d());
            MCML_HIP(hipGetLastError());
            MCML_TRY(lac_factor(tmpq2.d(), tmpq.d()));
            MCML_TRY(lac_check());
        } else {
            // vgrad = -D0 v + post * ZL' score
            MCML_TRY(dev_gemv_t(c, c.ZL.d(), c.ZL.ld, n, Q, tmpn.d(), tmpq.d(), glm_score_post(var_par, flink), 0.0));
            MCML_TRY(dev_gemv_t(c, D0.d(), D0.ld, Q, Q, v.d(), tmpq.d(), -1.0, 1.0));
            // vincr = (ZL' W ZL + I)^-1 vgrad
            MCML_TRY(build_M());
            MCML_TRY(potrf_lower_checked(c, M.d(), Q, M.ld));
            MCML_TRY(potrs_lower_vec(c, M.d(), M.ld, Q, tmpq.d(), tmpq2.d()));
        }
        MCML_TRY(dev_axpy(c, v.d(), tmpq.d(), 1.0, Q));
        MCML_TRY(get_v());                                        // also synchronises st / resid
        double mean = 0;
        for (int i = 0; i < n; ++i) mean += resid[i];
        mean /= n;
        double ss = 0;
        for (int i = 0; i < n; ++i) ss += (resid[i] - mean) * (resid[i] - mean);
        // beta += (X'WX)^-1 X' Wu
        std::vector<double> A(st.begin(), st.begin() + (size_t)P * P), b(st.begin() + (size_t)P * P, st.end());
        if (!ge_solve(A, b, P)) { set_error("mcnr_b: X'WX is singular"); return MCML_ESINGULAR; }
        for (int k = 0; k < P; ++k) beta[k] += b[k];
        sigma = sqrt(ss / (n - 1));
        return MCML_OK;
    }

    // src/mcml_la.cpp:62-103 / 204-243 and the tail :105-155 / 245-289
    int run(bool nr, bool usehess, double tol, int maxiter, int verbose, double* beta_out, double* theta_out,
            double* sigma_out, double* se_out, int nstart, double* u_out, int* converged_out, int* iters_out)
    {
        std::vector<double> b0 = beta, t0 = theta;
        double vp = 1.0, new_vp = 1.0;
        if (nr) MCML_TRY(update_W(true));                         // :195
        int it = 1; double maxdiff = 1; bool converged = false;
        while (maxdiff > tol && it <= maxiter) {
            if (nr) MCML_TRY(mcnr_b()); else MCML_TRY(la_optim());
            std::vector<double> nb = beta;
            MCML_TRY(model_update_beta(c, nb.data()));
            MCML_TRY(update_W(nr));
            MCML_TRY(la_optim_cov());
            std::vector<double> nt = theta;
            if (glm_is_gaussian(flink) || (nr && flink == 12)) new_vp = sigma;     // :84 vs :222
            maxdiff = fabs(vp - new_vp);
            for (int i = 0; i < P; ++i) maxdiff = fmax(maxdiff, fabs(b0[i] - nb[i]));
            for (int i = 0; i < R; ++i) maxdiff = fmax(maxdiff, fabs(t0[i] - nt[i]));
            converged = maxdiff < tol;
            b0 = nb; t0 = nt; vp = new_vp;
            if (!converged) {
                MCML_TRY(model_update_beta(c, b0.data()));
                if (nr) {
                    // update_W(0, true) runs BEFORE update_L: it still sees the previous ZL (:245-247)
                    var_par = new_vp;
                    MCML_TRY(update_W(true));
                } else {
                    MCML_TRY(update_W(false));
                    var_par = new_vp;
                }
                theta_model = t0;
                model_L_valid = false;
            } else {
                // the functor evaluations left other thetas in c.L: the model keeps theta_model
                model_L_valid = false;
            }
            if (verbose) {
                printf("\nIter %d  beta:", it);
                for (double x : b0) printf(" %g", x);
                printf("  theta:");
                for (double x : t0) printf(" %g", x);
                printf("  max diff %g%s\n", maxdiff, converged ? " CONVERGED" : "");
            }
            ++it;
        }
        MCML_TRY(la_optim_bcov());
        if (glm_is_gaussian(flink)) vp = sigma;
        for (int i = 0; i < P; ++i) beta_out[i] = beta[i];
        for (int i = 0; i < R; ++i) theta_out[i] = theta[i];
        *sigma_out = vp;
        if (se_out) {
            for (int i = 0; i < nstart; ++i) se_out[i] = 0.0;
            if (usehess) {
                std::vector<double> H;
                MCML_TRY(hess_la(1e-4, &H));
                const int nv = P + R + (glm_has_var_par(flink) ? 1 : 0);
                std::vector<double> Hi;
                // hess.llt().solve(I) (src/mcml_la.cpp:120-124)
                if (!spd_inverse(H, nv, &Hi)) { set_error("hess_la: Hessian is not positive definite"); return MCML_ENOTPD; }
                for (int i = 0; i < nv && i < nstart; ++i) se_out[i] = sqrt(Hi[i + (size_t)i * nv]);
            }
        }
        if (u_out) {                                              // u = L v with the driver's L
            model_L_valid = false;
            MCML_TRY(ensure_model_L());
            MCML_TRY(dev_gemv_n(c, c.L.d(), c.L.ld, Q, Q, v.d(), tmpq.d()));
            MCML_TRY(copy_d2h(u_out, tmpq.p, sizeof(double) * (size_t)Q, c.stream));
            MCML_HIP(hipStreamSynchronize(c.stream));
        }
        if (converged_out) *converged_out = converged ? 1 : 0;
        if (iters_out) *iters_out = it - 1;
        return MCML_OK;
    }
};

// the Laplace path forces the dense ZL (unless it runs the component operator) and leaves c.L at an arbitrary theta:
// restore / invalidate on every exit
struct LaScope {
    Ctx& c;
    explicit LaScope(Ctx& ctx) : c(ctx) {}
    ~LaScope() { c.no_sparse_zl = false; c.have_L = false; }
};

// ------------------------------------------------------------------ entry points (entry.h)
int drv_la(Ctx& c, const double* start, int nstart, int nr, int usehess, double tol, int verbose, int trace,
           int maxiter, const glmmr_mcml_ext* e, double* beta, double* theta, double* sigma, double* se, double* u,
           int* converged, int* iters)
{
    MCML_REQUIRE(c.n > 0 && c.cov.npar > 0, "mcml_la: the context has no model / covariance");
    MCML_REQUIRE(start && nstart >= c.P + c.cov.npar + (glm_is_gaussian(c.flink) ? 1 : 0), "mcml_la: start too short");
    MCML_REQUIRE(beta && theta && sigma, "mcml_la: null output");
    LaScope scope(c);
    LaFit f(c);
    f.trace = trace;
    f.maxfun = (e && e->maxfun > 0) ? e->maxfun : 0;
    MCML_TRY(f.init(start));
    return f.run(nr != 0, usehess != 0, tol, maxiter, verbose, beta, theta, sigma, se, nstart, u, converged, iters);
}

// test hook: one functor value / one mcnr_b step from a given state (see include/glmmr_mcml_c.h)
int drv_la_probe(Ctx& c, const double* start, int nstart, int kind, const double* v, double var_par,
                 const double* par, int npar, double* out, double* v_out, double* beta_out, double* sigma_out)
{
    MCML_REQUIRE(c.n > 0 && c.cov.npar > 0, "la_probe: the context has no model / covariance");
    MCML_REQUIRE(start && nstart >= c.P + c.cov.npar, "la_probe: start too short");
    LaScope scope(c);
    LaFit f(c);
    MCML_TRY(f.init(start));
    f.var_par = var_par;
    if (v) MCML_TRY(f.set_v(v));
    int rc = MCML_OK;
    if (kind <= 2) {
        std::vector<double> p(par, par + npar);
        if (kind == 1 || kind == 2) MCML_TRY(f.update_W(false));       // W as the constructor / driver leaves it
        rc = kind == 0 ? f.obj_bv(p, out) : kind == 1 ? f.obj_cov(p, out) : f.obj_btheta(p, out);
    } else {
        MCML_TRY(f.update_W(true));
        rc = f.mcnr_b();
        if (!rc) {
            for (int i = 0; i < c.Q; ++i) v_out[i] = f.hv[i];
            for (int i = 0; i < c.P; ++i) beta_out[i] = f.beta[i];
            *sigma_out = f.sigma;
        }
    }
    return rc;
}

}  // namespace mcml
