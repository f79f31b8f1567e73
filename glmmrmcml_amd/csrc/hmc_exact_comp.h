// hmc_exact_comp.h -- exact conditional draws, component by component, on the sparse chain-major operator (opt-in,
// Ctx::draws_mode = 2; included by hmc.hip after hmc_exact.h).
//
// The Gaussian of hmc_exact.h, v | y ~ N(mu*, M^-1) with M = I + ZL' ZL / sigma^2, on a block-structured design: M is block
// diagonal over the connected components of ZL's coupling graph (component_plan.h), and a component's variables are kept in
// ascending order, so the Cholesky factor of M restricted to a component IS the factor R_c of M_c.  The draw
//     v_c = mu*_c + R_c^-T z_c,   M_c mu*_c = b_c
// is the dense draw R^-T (R^-1 b + z) up to rounding.  One call:
//   k_exc_rhs                       b = ZL' (y - X beta) / sigma^2 over the CSR rows of ZL', observations ascending
//   k_lac_factor / k_lac_factor_wg  the component operator (component.hip, lac_factor_launch) with the constant weight 1 / sigma^2
//                                   and g = b: they build and factorise every M_c in LDS, solve for mu*_c, and leave R_c in the
//                                   factor scratch (CompFactors, comp_factors_ensure: shared with the queries); a wave or a
//                                   workgroup per component: cp_waves under GLMMR_MCML_LA_WAVES
//   k_exc_draw                      lane = sample column: z, the backward solve R_c' s = z, v = mu* + s, stored chain-major
//   k_cm_transpose, samples_to_U    to the Q x ncols sample matrix and U = L V, as every sampler ends
// No atomics, every sum in a fixed order: two calls with one seed give the same bits, and a column's arithmetic does not
// depend on the block of 64 it sits in.  k_exc_rhs and k_exc_draw are this file's own and do not go through the shared
// right-hand side and substitution kernels of component.hip: component.h says why.
#pragma once
#include "component.h"

namespace mcml {

static bool exact_component_applicable(const Ctx& c) { return c.flink == 7 && comp_operator_ready(c); }

// b[q] = post * sum_t csr_val[t] (y - xb)[csr_i[t]]: row q of ZL', observations ascending
__global__ __launch_bounds__(256) void k_exc_rhs(const int* csr_ptr, const int* csr_i, const double* csr_val, const double* y,
                                                 const double* xb, double post, int Q, double* b)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    b[q] = post * csr_row_sum(csr_ptr, csr_i, csr_val, q, [&](int i) { return y[i] - xb[i]; });
}

// ---- the draw kernel.  A wave is 64 sample columns of one work item (consecutive components), lane = column.  The lane's
// vector lives in LDS as [variable][lane]: 512 B per variable, the lanes read consecutive doubles (two passes over the 64
// banks, no conflict).  An entry of R_c is the same for every lane: an LDS broadcast where R_c is staged (components up to
// CP_MAX_VARS variables: EXC_WAVES waves per workgroup, each with its own R_c -- leading dimension odd as LAC_LD -- and
// vector block), a uniform load from the factor scratch above (one wave per workgroup, the vector block alone: 64 KB at
// CP_WIDE_MAX_VARS).
constexpr int EXC_WAVES = 4;
constexpr int exc_wave_doubles(int mv) { return mv <= CP_MAX_VARS ? mv * 64 + mv * (mv | 1) : mv * 64; }
constexpr int exc_waves(int mv) { return mv <= CP_MAX_VARS ? EXC_WAVES : 1; }
constexpr int exc_lds_bytes(int mv) { return 8 * exc_waves(mv) * exc_wave_doubles(mv); }
static_assert(exc_lds_bytes(CP_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_exc_draw, staged form at its cap");
static_assert(exc_lds_bytes(CP_WIDE_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_exc_draw, one wave at the cap");

struct ExcArgs {
    CompView cv;                         // STAGE: a wave takes work item t = components [item_ptr[t], item_ptr[t + 1]); else component t
    const int* fac_ptr;                  // CompFactors
    const double *fac, *mu;              // the factors (k_lac_factor*), mu* (Q)
    const double* inj_z;                 // nullable: Q x ncols, no padding
    double* out;                         // chain-major: element (column j, variable q) at j + q * ld
    size_t ld;
    int Q, ncols;
    int C, d;                            // draw_of_column
    uint64_t seed; uint32_t chain_offset, tag;
};

// grid (ceil(items / waves), ceil(ncols / 64)), 64 * waves threads, exc_lds_bytes(max_vars) of dynamic LDS.  No workgroup
// barrier: the waves are independent
template <bool STAGE>
__global__ __launch_bounds__(64 * EXC_WAVES) void k_exc_draw(ExcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double exc_lds[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blockIdx.x * (STAGE ? EXC_WAVES : 1) + w;
    if (item >= (STAGE ? a.cv.nitems : a.cv.ncomp)) return;
    const int mv = a.cv.max_vars, ldr = mv | 1;
    double* x = exc_lds + (size_t)w * (mv * 64 + (STAGE ? mv * ldr : 0));        // [variable][lane]
    double* R = x + mv * 64;                                                     // column-major, ldr (STAGE)
    const int col = blockIdx.y * 64 + lane;
    const bool live = col < a.ncols;
    uint32_t chain, draw;
    draw_of_column(col, a.C, a.d, &chain, &draw);
    chain += a.chain_offset;
    const int c0 = STAGE ? a.cv.item_ptr[item] : item, c1 = STAGE ? a.cv.item_ptr[item + 1] : item + 1;
    for (int comp = c0; comp < c1; ++comp) {
        const int v0 = a.cv.var_ptr[comp], nv = a.cv.var_ptr[comp + 1] - v0;     // 1 <= nv <= mv
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
            const int q = a.cv.vars[v0 + i];
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
            const int q = a.cv.vars[v0 + k];
            if (live) a.out[col + (size_t)q * a.ld] = a.mu[q] + acc;             // 512 B per variable per wave
        }
    }
}

// as exact_gaussian_sample.  inj_z: host, Q x ncols, or null
static int exact_component_sample(Ctx& c, const double* beta, double var_par, const glmmr_mcml_hmc_opts* o, uint64_t seed,
                                  uint32_t iter_idx, const double* inj_z, uint8_t* flags_out, double* probs_out,
                                  glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    const bool ok = exact_component_applicable(c);
    if (!ok) set_error("component-wise exact draws need a gaussian / identity model on the sparse ZL operator with L set and no "
                       "component above %d variables", CP_WIDE_MAX_VARS);
    const int Q = c.Q;
    const ComponentPlan& p = c.cp.plan;
    ExactCompState& x = c.exact_comp;
    ExactCall k(x.prof, c.stream);
    MCML_TRY(exact_begin(c, beta, var_par, o, inj_z, ok, x.T, k));
    const int ncols = k.sh.ncols;
    MCML_TRY(comp_factors_ensure(c, x.f));
    MCML_TRY(x.b.ensure(sizeof(double) * (size_t)Q)); MCML_TRY(x.mu.ensure(sizeof(double) * (size_t)Q));
    const size_t ldc = (size_t)round_up(ncols, 64);
    MCML_TRY(x.CM.ensure(sizeof(double) * ldc * (size_t)Q));
    k.mark();
    // ---- factor and mean
    hipLaunchKernelGGL(k_exc_rhs, dim3((Q + 255) / 256), dim3(256), 0, c.stream, c.sp.csr_ptr.as<int>(), c.sp.csr_i.as<int>(),
                       c.sp.csr_val.d(), c.y.d(), c.xb.d(), k.post, Q, x.b.d());
    MCML_HIP(hipGetLastError());
    MCML_TRY(lac_factor_launch(c, nullptr, k.post, x.b.d(), x.mu.d(), x.f.logdet.d(), x.f.fac.d(), x.f.fac_ptr.as<int>(),
                               cp_waves(p, cp_forced_waves(CP_LA_WAVES_ENV)), nullptr));
    k.mark();
    // ---- the draws, chain-major
    const bool stage = p.max_vars <= CP_MAX_VARS;                 // then the plan is feasible: its work items are built
    const ExcArgs a{comp_view(c), x.f.fac_ptr.as<int>(), x.f.fac.d(), x.mu.d(), k.d_z.d(), x.CM.d(), ldc, Q, ncols, k.sh.C, k.sh.d,
                    seed, (uint32_t)o->chain_offset, 16u * iter_idx + 8u};
    const int lds = exc_lds_bytes(p.max_vars), items = stage ? a.cv.nitems : a.cv.ncomp;
    const dim3 grid((items + exc_waves(p.max_vars) - 1) / exc_waves(p.max_vars), (ncols + 63) / 64);
    if (stage) {
        MCML_TRY(ensure_dynamic_lds((const void*)k_exc_draw<true>, exc_lds_bytes(CP_MAX_VARS)));
        hipLaunchKernelGGL(k_exc_draw<true>, grid, dim3(64 * EXC_WAVES), lds, c.stream, a);
    } else {
        MCML_TRY(ensure_dynamic_lds((const void*)k_exc_draw<false>, exc_lds_bytes(CP_WIDE_MAX_VARS)));
        hipLaunchKernelGGL(k_exc_draw<false>, grid, dim3(64), lds, c.stream, a);
    }
    MCML_HIP(hipGetLastError());
    k.mark();
    // ---- T[q + j ld] = CM[j + q ldc]
    hipLaunchKernelGGL(k_cm_transpose, dim3((Q + 31) / 32, (ncols + 31) / 32), dim3(256), 0, c.stream, x.CM.d(), (int)ldc, Q, ncols,
                       x.T.d(), (size_t)x.T.ld, (size_t)1, 0);
    MCML_HIP(hipGetLastError());
    k.mark();
    return exact_end(c, k, x.T, KERNEL_EXACT_COMPONENT, "exact draws: I + ZL' ZL / sigma^2 is not positive definite", x.ms,
                     flags_out, probs_out, diag, ncols_out);
}

}  // namespace mcml
