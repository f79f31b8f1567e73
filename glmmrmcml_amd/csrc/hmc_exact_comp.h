// hmc_exact_comp.h -- exact conditional draws, component by component, on the sparse chain-major operator (opt-in,
// Ctx::draws_mode = 2; included by hmc.hip after hmc_exact.h).
//
// The Gaussian of hmc_exact.h, v | y ~ N(mu*, M^-1) with M = I + ZL' ZL / sigma^2, on a block-structured design: M is block
// diagonal over the connected components of ZL's coupling graph (component_plan.h), and a component's variables are kept in
// ascending order, so the Cholesky factor of M restricted to a component IS the factor R_c of M_c.  The draw
//     v_c = mu*_c + R_c^-T z_c,   M_c mu*_c = b_c
// is the dense draw R^-T (R^-1 b + z) up to rounding.  One call:
//   k_exc_rhs                       b = ZL' (y - X beta) / sigma^2 over the CSR rows of ZL', observations ascending
//   k_lac_factor / k_lac_factor_wg  the Laplace fits' kernels (la_comp.h) with W = 1 / sigma^2 and g = b: they build and
//                                   factorise every M_c in LDS, solve for mu*_c, and leave R_c in the factor scratch
//                                   (LacArgs::fac); the form, a wave or a workgroup per component, is lac_waves' choice
//   k_exc_draw                      lane = sample column: z, the backward solve R_c' s = z, v = mu* + s, stored chain-major
//   k_cm_transpose, samples_to_U    to the Q x ncols sample matrix and U = L V, as every sampler ends
// No atomics, every sum in a fixed order: two calls with one seed give the same bits, and a column's arithmetic does not
// depend on the block of 64 it sits in.
#pragma once

namespace mcml {

static bool exact_component_applicable(const Ctx& c)
{
    return c.flink == 7 && c.have_L && c.sp.active && c.cp.ready && c.cp.plan.records;
}

// b[q] = post * sum_t csr_val[t] (y - xb)[csr_i[t]]: row q of ZL', observations ascending
__global__ __launch_bounds__(256) void k_exc_rhs(const int* csr_ptr, const int* csr_i, const double* csr_val, const double* y,
                                                 const double* xb, double post, int Q, double* b)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    double s = 0;
    for (int t = csr_ptr[q]; t < csr_ptr[q + 1]; ++t) { const int i = csr_i[t]; s += csr_val[t] * (y[i] - xb[i]); }
    b[q] = post * s;
}

__global__ __launch_bounds__(256) void k_exc_fill(double* W, int n, double v)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) W[i] = v;
}

// ---- the draw kernel.  A wave is 64 sample columns of one work item (consecutive components), lane = column.  The lane's
// vector lives in LDS as [variable][lane]: 512 B per variable, the lanes read consecutive doubles (two passes over the 64
// banks, no conflict).  An entry of R_c is the same for every lane: an LDS broadcast where R_c is staged (components up to
// CP_MAX_VARS variables: EXC_WAVES waves per workgroup, each with its own R_c -- leading dimension odd as LAC_LD -- and
// vector block), a uniform load from the factor scratch above (one wave per workgroup, the vector block alone: 64 KB at
// CP_WIDE_MAX_VARS).
constexpr int EXC_WAVES = 4;
inline int exc_ldr(int max_vars) { return max_vars | 1; }
inline int exc_wave_doubles(int max_vars) { return max_vars <= CP_MAX_VARS ? max_vars * 64 + max_vars * exc_ldr(max_vars) : max_vars * 64; }
inline int exc_waves(int max_vars) { return max_vars <= CP_MAX_VARS ? EXC_WAVES : 1; }
inline int exc_lds_bytes(int max_vars) { return 8 * exc_waves(max_vars) * exc_wave_doubles(max_vars); }
static_assert(8 * EXC_WAVES * (CP_MAX_VARS * 64 + CP_MAX_VARS * (CP_MAX_VARS | 1)) <= CP_LDS_BYTES_PER_CU, "k_exc_draw, staged form at its cap");
static_assert(8 * CP_WIDE_MAX_VARS * 64 <= CP_LDS_BYTES_PER_CU, "k_exc_draw, one wave at the cap");

struct ExcArgs {
    const int *item_ptr;                 // nullable: work item t = components [item_ptr[t], item_ptr[t + 1]); null: item t = component t
    const int *var_ptr, *vars, *fac_ptr; // ComponentDev, ExactCompState
    const double *fac, *mu;              // the factors (k_lac_factor*), mu* (Q)
    const double* inj_z;                 // nullable: Q x ncols, no padding
    double* out;                         // chain-major: element (column j, variable q) at j + q * ld
    size_t ld;
    int nitems, Q, ncols, mv;            // mv: the plan's max_vars (sizes the LDS)
    int C, d;                            // draw_of_column
    uint64_t seed; uint32_t chain_offset, tag;
};

// grid (ceil(nitems / waves), ceil(ncols / 64)), 64 * waves threads, exc_lds_bytes(mv) of dynamic LDS.  No workgroup barrier:
// the waves are independent
template <bool STAGE>
__global__ __launch_bounds__(64 * EXC_WAVES) void k_exc_draw(ExcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double exc_lds[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blockIdx.x * (STAGE ? EXC_WAVES : 1) + w;
    if (item >= a.nitems) return;
    const int ldr = a.mv | 1;
    double* x = exc_lds + (size_t)w * (a.mv * 64 + (STAGE ? a.mv * ldr : 0));    // [variable][lane]
    double* R = x + a.mv * 64;                                                   // column-major, ldr (STAGE)
    const int col = blockIdx.y * 64 + lane;
    const bool live = col < a.ncols;
    uint32_t chain, draw;
    draw_of_column(col, a.C, a.d, &chain, &draw);
    chain += a.chain_offset;
    const int c0 = a.item_ptr ? a.item_ptr[item] : item, c1 = a.item_ptr ? a.item_ptr[item + 1] : item + 1;
    for (int comp = c0; comp < c1; ++comp) {
        const int v0 = a.var_ptr[comp], nv = a.var_ptr[comp + 1] - v0;           // 1 <= nv <= mv
        const double* F = a.fac + a.fac_ptr[comp];                               // lower triangle, leading dimension nv
        if (STAGE) {
            wave_lds_sync();                         // the previous component's reads of R
            for (int e = lane; e < nv * nv; e += 64) {
                const int i = e % nv, j = e / nv;
                if (i >= j) R[i + j * ldr] = F[e];
            }
            wave_lds_sync();
        }
        for (int i = 0; i < nv; ++i) {
            const int q = a.vars[v0 + i];
            double z = 0.0;
            if (live) z = a.inj_z ? a.inj_z[q + (size_t)col * a.Q] : rng_normal(a.seed, (uint32_t)q, chain, draw, a.tag);
            x[i * 64 + lane] = z;
        }
        // R_c' s = z backward: s_k = (z_k - sum_{i > k} R_c[i, k] s_i) / R_c[k, k], i ascending
        for (int k = nv - 1; k >= 0; --k) {
            double acc = x[k * 64 + lane];
            if (STAGE) {
                for (int i = k + 1; i < nv; ++i) acc -= R[i + k * ldr] * x[i * 64 + lane];
                acc = acc / R[k + k * ldr];
            } else {
                const double* Fk = F + (size_t)k * nv;
                for (int i = k + 1; i < nv; ++i) acc -= Fk[i] * x[i * 64 + lane];
                acc = acc / Fk[k];
            }
            x[k * 64 + lane] = acc;
            const int q = a.vars[v0 + k];
            if (live) a.out[col + (size_t)q * a.ld] = a.mu[q] + acc;             // 512 B per variable per wave
        }
    }
}

// hmc_sample's signature and side effects, as exact_gaussian_sample.  inj_z: host, Q x ncols, or null
static int exact_component_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed,
                                  uint32_t iter_idx, const double* inj_z, uint8_t* flags_out, double* probs_out,
                                  glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    MCML_REQUIRE(o && o->nsamp > 0 && o->warmup >= 0, "exact draws: bad options");
    MCML_REQUIRE(beta, "exact draws: beta is null");
    MCML_REQUIRE(var_par > 0, "exact draws: var_par (sigma) must be positive");
    if (!exact_component_applicable(c)) {
        set_error("component-wise exact draws need a gaussian / identity model on the sparse ZL operator with L set and no "
                  "component above %d variables", CP_WIDE_MAX_VARS);
        return MCML_EUNSUPPORTED;
    }
    const SampleShape sh = sample_shape(o->nsamp, o->warmup, o->chains);
    const int ncols = sh.ncols;
    const int Q = c.Q, n = c.n;
    const double post = glm_score_post(var_par, c.flink);
    const ComponentDev& cp = c.cp;
    const ComponentPlan& p = cp.plan;
    ExactCompState& x = c.exact_comp;
    ExactProf prof(x.prof, c.stream);

    MCML_TRY(model_update_beta(c, beta));
    if (!x.fac_doubles) {                                         // the pattern is fixed per model
        std::vector<int> off(p.ncomp + 1, 0);
        for (int k = 0; k < p.ncomp; ++k) { const int nv = p.var_ptr[k + 1] - p.var_ptr[k]; off[k + 1] = off[k] + nv * nv; }
        MCML_TRY(x.fac_ptr.ensure(sizeof(int) * off.size()));
        MCML_TRY(copy_h2d(x.fac_ptr.p, off.data(), sizeof(int) * off.size(), c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
        MCML_TRY(x.fac.ensure(sizeof(double) * (size_t)off[p.ncomp]));
        x.fac_doubles = off[p.ncomp];
    }
    MCML_TRY(x.W.ensure(sizeof(double) * (size_t)n));
    MCML_TRY(x.b.ensure(sizeof(double) * (size_t)Q));
    MCML_TRY(x.mu.ensure(sizeof(double) * (size_t)Q));
    MCML_TRY(x.logdet.ensure(sizeof(double) * (size_t)p.ncomp));
    const size_t ldc = (size_t)round_up(ncols, 64);
    MCML_TRY(x.CM.ensure(sizeof(double) * ldc * (size_t)Q));
    MCML_TRY(x.T.alloc(Q, ncols));
    DevBuf d_z;
    if (inj_z) {
        MCML_TRY(d_z.ensure(sizeof(double) * (size_t)Q * ncols));
        MCML_TRY(copy_h2d(d_z.p, inj_z, sizeof(double) * (size_t)Q * ncols, c.stream));
    }
    prof.mark();
    // ---- factor and mean
    hipLaunchKernelGGL(k_exc_fill, dim3((n + 255) / 256), dim3(256), 0, c.stream, x.W.d(), n, post);
    hipLaunchKernelGGL(k_exc_rhs, dim3((Q + 255) / 256), dim3(256), 0, c.stream, c.sp.csr_ptr.as<int>(), c.sp.csr_i.as<int>(),
                       c.sp.csr_val.d(), c.y.d(), c.xb.d(), post, Q, x.b.d());
    MCML_HIP(hipGetLastError());
    MCML_TRY(lac_factor_launch(c, x.W.d(), x.b.d(), x.mu.d(), x.logdet.d(), x.fac.d(), x.fac_ptr.as<int>(), lac_waves_now(p)));
    prof.mark();
    // ---- the draws, chain-major
    const bool stage = p.max_vars <= CP_MAX_VARS;                 // then the plan is feasible: its work items are built
    ExcArgs a{stage ? cp.item_ptr.as<int>() : nullptr, cp.var_ptr.as<int>(), cp.vars.as<int>(), x.fac_ptr.as<int>(), x.fac.d(),
              x.mu.d(), d_z.d(), x.CM.d(), ldc, stage ? p.nitems() : p.ncomp, Q, ncols, p.max_vars, sh.C, sh.d, seed,
              (uint32_t)o->chain_offset, 16u * iter_idx + 8u};
    const int lds = exc_lds_bytes(p.max_vars);
    const dim3 grid((a.nitems + exc_waves(p.max_vars) - 1) / exc_waves(p.max_vars), (ncols + 63) / 64);
    if (stage) {
        MCML_TRY(ensure_dynamic_lds((const void*)k_exc_draw<true>, exc_lds_bytes(CP_MAX_VARS)));
        hipLaunchKernelGGL(k_exc_draw<true>, grid, dim3(64 * EXC_WAVES), lds, c.stream, a);
    } else {
        MCML_TRY(ensure_dynamic_lds((const void*)k_exc_draw<false>, exc_lds_bytes(CP_WIDE_MAX_VARS)));
        hipLaunchKernelGGL(k_exc_draw<false>, grid, dim3(64), lds, c.stream, a);
    }
    MCML_HIP(hipGetLastError());
    prof.mark();
    // ---- T[q + j ld] = CM[j + q ldc]
    MCML_HIP(hipMemsetAsync(x.T.d(), 0, sizeof(double) * (size_t)x.T.ld * ncols, c.stream));   // finite padding rows
    hipLaunchKernelGGL(k_cm_transpose, dim3((Q + 31) / 32, (ncols + 31) / 32), dim3(256), 0, c.stream, x.CM.d(), (int)ldc, Q, ncols,
                       x.T.d(), (size_t)x.T.ld, (size_t)1, 0);
    MCML_HIP(hipGetLastError());
    prof.mark();
    MCML_TRY(samples_to_U(c, x.T, ncols));                        // return (L * samples)  (mhmcmc.h:155)
    prof.mark();
    c.niter = sh.niter;
    c.last_kernel[0] = c.last_kernel[1] = KERNEL_EXACT_COMPONENT;
    const int rc = check_errflag(c, "exact draws: I + ZL' ZL / sigma^2 is not positive definite");   // a pivot of some M_c
    prof.collect(x.ms);
    MCML_TRY(rc);
    exact_finish(sh, flags_out, probs_out, diag, ncols_out);
    return MCML_OK;
}

}  // namespace mcml
