// hmc_exact.h -- exact conditional draws for gaussian / identity models (opt-in, Ctx::draws_mode = 1; included by hmc.hip).
//
// For family / link 7 the density the HMC sampler targets in the whitened variables v (mhmcmc.h:61-119 with
// mcmlmodel.h:138-153 case 7: a N(0, I) prior and data that enter quadratically) IS Gaussian:
//     v | y ~ N(mu*, M^-1),   M = I + ZL' ZL / sigma^2,   M mu* = b = ZL' (y - X beta) / sigma^2
// (sigma = var_par, a standard deviation; 1 / sigma^2 = glm_score_post).  With M = R R' (lower R) a draw is
//     v = R^-T (R^-1 b + z),   z ~ N(0, I)
// since R^-T R^-1 b = mu* and cov(R^-T z) = M^-1.  One call is therefore: one Q x Q x n product (build_M_dense, shared
// with the Laplace fits), one factorisation (potrf_lower_checked), a forward solve for one vector (trsm_left_lower, m = 1), a
// fill kernel, ONE transposed solve for all columns (trsm_left_lower_trans) and the L V product every sampler ends with --
// instead of (warmup + draws) x steps product pairs.  The draws are independent: no warm-up, no step size, no rejections.
//
// The request is honoured only where it is exact and the dense operator is resident (exact_applicable); anywhere else
// hmc_sample runs as ever.  Family / link 8 (gaussian / log) is excluded: its score and its density disagree in the
// reference, so "what HMC samples there" is not the Gaussian above.
#pragma once

namespace mcml {

static bool exact_applicable(const Ctx& c)
{
    return c.flink == 7 && !c.sp.active && c.have_L && c.ZL.d() && c.ZLT.d();
}

// b[j] = post * sum_i ZL[i, j] (y_i - xb_i): one wave per column of ZL
__global__ __launch_bounds__(256) void k_exact_rhs(const double* ZL, int ld, int n, int Q, const double* y, const double* xb,
                                                   double post, double* b)
{
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= Q) return;
    double s = 0;
    for (int i = lane; i < n; i += 64) s += ZL[i + (size_t)j * ld] * (y[i] - xb[i]);
    s = wave_sum(s);
    if (lane == 0) b[j] = post * s;
}

// T[q, j] = z(q, j) + w[q]: column j is a draw of a chain as in the HMC draws' layout (draw_of_column, hmc_chain.h); z is
// injected (Q x ncols, no padding) or the standard normal of rng.h, tag 8
__global__ __launch_bounds__(256) void k_exact_fill(double* T, int ldt, int Q, int ncols, const double* w, const double* inj_z,
                                                    uint64_t seed, uint32_t chain_offset, uint32_t iter_idx, int C, int d)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const double wq = w[q];
    for (int j = blockIdx.y; j < ncols; j += gridDim.y) {
        uint32_t chain, draw;
        draw_of_column(j, C, d, &chain, &draw);
        const double z = inj_z ? inj_z[q + (size_t)j * Q]
                               : rng_normal(seed, (uint32_t)q, chain_offset + chain, draw, 16u * iter_idx + 8u);
        T[q + (size_t)j * ldt] = z + wq;
    }
}

// HIP events around the phases of one call (ExactState::prof), read after the final synchronisation
struct ExactProf {
    bool on; hipStream_t s; hipEvent_t ev[6] = {}; int n = 0;
    ExactProf(bool on_, hipStream_t s_) : on(on_), s(s_) {}
    void mark() { if (on && n < 6 && hipEventCreate(&ev[n]) == hipSuccess) { (void)hipEventRecord(ev[n], s); ++n; } }
    void collect(double* ms) {
        for (int i = 0; i < 5; ++i) {
            float t = 0;
            ms[i] = (on && i + 1 < n && hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) ? t : 0.0;
        }
    }
    ~ExactProf() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
};

// ---- what the two exact samplers (here and hmc_exact_comp.h) share: hmc_sample's signature and side effects (c.U = L * draws,
// c.mcols, c.niter); o->warmup, lambda, max_steps, target_accept and adapt only size the flags / probs extents
struct ExactCall : ExactProf {
    using ExactProf::ExactProf;
    SampleShape sh; double post;                 // post = 1 / sigma^2
    DevBuf d_z;                                  // inj_z on the device, or null
};

// the argument checks, then `applicable` (false: MCML_EUNSUPPORTED with the message the caller has set); the shape (column 0 of
// one chain is just another draw), xb = X beta, T (Q x ncols) with finite padding rows, inj_z (host, Q x ncols, or null) uploaded
static int exact_begin(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, const double* inj_z,
                       bool applicable, DevMat& T, ExactCall& k)
{
    MCML_REQUIRE(o && o->nsamp > 0 && o->warmup >= 0, "exact draws: bad options");
    MCML_REQUIRE(beta, "exact draws: beta is null");
    MCML_REQUIRE(var_par > 0, "exact draws: var_par (sigma) must be positive");
    if (!applicable) return MCML_EUNSUPPORTED;
    k.sh = sample_shape(o->nsamp, o->warmup, o->chains);
    k.post = glm_score_post(var_par, c.flink);
    MCML_TRY(model_update_beta(c, beta));
    MCML_TRY(T.alloc(c.Q, k.sh.ncols));
    MCML_HIP(hipMemsetAsync(T.d(), 0, sizeof(double) * (size_t)T.ld * k.sh.ncols, c.stream));
    if (inj_z) {
        MCML_TRY(k.d_z.ensure(sizeof(double) * (size_t)c.Q * k.sh.ncols));
        MCML_TRY(copy_h2d(k.d_z.p, inj_z, sizeof(double) * (size_t)c.Q * k.sh.ncols, c.stream));
    }
    return MCML_OK;
}

// T holds the draws: U = L T as every sampler ends, the context's record of the call, the final synchronisation (notpd: the
// message if a pivot failed on the way, or null where nothing raises the flag), the phases' times, the caller's outputs
static int exact_end(Ctx& c, ExactCall& k, DevMat& T, int kernel, const char* notpd, double* ms, uint8_t* flags_out,
                     double* probs_out, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    MCML_TRY(samples_to_U(c, T, k.sh.ncols));                     // return (L * samples)  (mhmcmc.h:155)
    k.mark();
    c.niter = k.sh.niter; c.last_kernel[0] = c.last_kernel[1] = kernel;
    const int rc = notpd ? check_errflag(c, notpd) : c.sync();
    k.collect(ms);
    MCML_TRY(rc);
    exact_finish(k.sh, flags_out, probs_out, diag, ncols_out);
    return MCML_OK;
}

// inj_z: host, Q x ncols, or null
static int exact_gaussian_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed,
                                 uint32_t iter_idx, const double* inj_z, uint8_t* flags_out, double* probs_out,
                                 glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    const bool ok = exact_applicable(c);
    if (!ok) set_error("exact draws need a gaussian / identity model on the dense ZL operator with L set");
    const int Q = c.Q, n = c.n;
    ExactState& x = c.exact;
    ExactCall k(x.prof, c.stream);
    MCML_TRY(exact_begin(c, beta, var_par, o, inj_z, ok, x.T, k));
    const int ncols = k.sh.ncols;
    k.mark();
    DevMat unused;
    MCML_TRY(build_M_dense(c, nullptr, k.post, x.M, unused, true));
    k.mark();
    MCML_TRY(potrf_lower_checked(c, x.M.d(), Q, x.M.ld));
    k.mark();

    MCML_TRY(x.b.ensure(sizeof(double) * (size_t)(pad_ld(Q) + 64)));
    MCML_HIP(hipMemsetAsync(x.b.p, 0, sizeof(double) * (size_t)(pad_ld(Q) + 64), c.stream));
    hipLaunchKernelGGL(k_exact_rhs, dim3((Q + 3) / 4), dim3(256), 0, c.stream, c.ZL.d(), c.ZL.ld, n, Q, c.y.d(), c.xb.d(), k.post,
                       x.b.d());
    MCML_HIP(hipGetLastError());
    MCML_TRY(trsm_left_lower(c, x.M.d(), x.M.ld, Q, x.b.d(), pad_ld(Q), 1));      // w = R^-1 b
    hipLaunchKernelGGL(k_exact_fill, dim3((Q + 255) / 256, ncols < 1024 ? ncols : 1024), dim3(256), 0, c.stream, x.T.d(), x.T.ld,
                       Q, ncols, x.b.d(), k.d_z.d(), seed, (uint32_t)o->chain_offset, iter_idx, k.sh.C, k.sh.d);
    MCML_HIP(hipGetLastError());
    k.mark();
    MCML_TRY(trsm_left_lower_trans(c, x.M.d(), x.M.ld, Q, x.T.d(), x.T.ld, ncols));
    k.mark();
    return exact_end(c, k, x.T, KERNEL_EXACT, nullptr, x.ms, flags_out, probs_out, diag, ncols_out);
}

}  // namespace mcml
