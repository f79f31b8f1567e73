// la_comp.h -- the component operator of the Laplace fits (opt-in; included by laplace.hip only).
//
// M = ZL' W ZL + I couples two variables only through an observation whose row of ZL touches both, so it is block
// diagonal over the connected components of component_plan.h: logdet M = sum_c logdet M_c and M^-1 g is solved
// component by component.  k_lac_factor builds, factorises and (optionally) solves every M_c in LDS, one wave per
// component; k_lac_factor_wg gives a component a workgroup of four waves and M_c a dynamically sized piece of LDS (up to
// CP_WIDE_MAX_VARS variables; the observations are staged in batches that the waves share).  The vector-sized products run
// over the ELL / CSR arrays of the sparse ZL operator and over the covariance blocks of D0.  Every sum has a fixed order: no
// atomics, two runs are bit-identical.
#pragma once
#include "ctx.h"
#include "reduce.h"
#include <cstdlib>
#include <cstring>

namespace mcml {

constexpr int LAC_WAVES = 4;                         // components per workgroup (one wave each)
constexpr int LAC_LD = CP_MAX_VARS + 1;              // odd leading dimension: a row of M_c (stride LAC_LD doubles) hits distinct banks
constexpr int LAC_WAVE_DOUBLES = CP_MAX_VARS * LAC_LD + 2 * CP_MAX_VARS;   // M_c, the row r, the right-hand side
static_assert(LAC_WAVES * LAC_WAVE_DOUBLES * 8 <= 64 * 1024, "k_lac_factor keeps its LDS static");

struct LacArgs {
    const int *var_ptr, *vars, *slot_ptr;            // ComponentDev
    const int* slot_i;                               // the records, 8 ints and 8 doubles each (ComponentDev); xb and y are not
    const double* slot_d;                            // read here
    const double* W;                                 // n
    int ncomp;
    const double* g;                                 // nullable: right-hand side (Q); x = M^-1 g is written to x
    double* x;
    double* logdet;                                  // ncomp: 2 sum log diag chol(M_c)
    int* errflag;                                    // raised on a non-positive pivot (Ctx::errflag)
    double* fac = nullptr;                           // nullable: the lower triangle of chol(M_c), diagonal included, is stored
    const int* fac_ptr = nullptr;                    // column-major (leading dimension nv) at fac + fac_ptr[comp] (hmc_exact_comp.h)
};

// grid ceil(ncomp / LAC_WAVES), 64 * LAC_WAVES threads.  No workgroup barrier: the waves are independent
__global__ __launch_bounds__(64 * LAC_WAVES) void k_lac_factor(LacArgs a)
{
    __shared__ double lds[LAC_WAVES * LAC_WAVE_DOUBLES];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int comp = blockIdx.x * LAC_WAVES + w;
    if (comp >= a.ncomp) return;
    double* M = lds + (size_t)w * LAC_WAVE_DOUBLES;  // column-major, LAC_LD
    double* r = M + CP_MAX_VARS * LAC_LD;
    double* xs = r + CP_MAX_VARS;
    const int v0 = a.var_ptr[comp], nv = a.var_ptr[comp + 1] - v0;           // 1 <= nv <= CP_MAX_VARS
    const int s0 = a.slot_ptr[comp], s1 = a.slot_ptr[comp + 1];
    // entry e = lane + 64 t of the nv x nv square is (e % nv, e / nv): advanced without a division per step
    const int q64 = 64 / nv, r64 = 64 % nv, i0 = lane % nv, j0 = lane / nv;
    for (int i = i0, j = j0; j < nv;) {
        M[i + j * LAC_LD] = i == j ? 1.0 : 0.0;
        i += r64; j += q64;
        if (i >= nv) { i -= nv; ++j; }
    }
    // ---- M_c = I + sum_i W_i r_i r_i', observations ascending.  Lane j sums entry j of the row in ELL order (a local
    // column can come twice), then every entry of the square has one owner lane
    int s = s0;
    while (s < s1) {
        double rj = 0.0;
        int obs;
        for (;;) {
            const int* ip = a.slot_i + 8 * (size_t)s;
            const double* dp = a.slot_d + 8 * (size_t)s;
            const int ne = ip[4], last = ip[5];
            obs = ip[6];
#pragma unroll
            for (int u = 0; u < CP_SLOT; ++u) if (u < ne && ip[u] == lane) rj += dp[u];
            ++s;
            if (last || s >= s1) break;
        }
        const double wi = a.W[obs];
        wave_lds_sync();                             // the previous observation's reads of r
        if (lane < nv) r[lane] = rj;
        wave_lds_sync();
        for (int i = i0, j = j0; j < nv;) {
            M[i + j * LAC_LD] += wi * r[i] * r[j];
            i += r64; j += q64;
            if (i >= nv) { i -= nv; ++j; }
        }
    }
    wave_lds_sync();
    // ---- right-looking Cholesky of the lower triangle; lane & 31 = row, two columns of the trailing update at a time
    bool bad = false;
    const int ti = lane & 31, tj = lane >> 5;
    for (int k = 0; k < nv; ++k) {
        const double d = M[k + k * LAC_LD];
        if (!(d > 0.0)) { bad = true; break; }       // the same value in every lane
        const double sd = sqrt(d);
        wave_lds_sync();
        if (lane == k) M[k + k * LAC_LD] = sd;
        else if (lane > k && lane < nv) M[lane + k * LAC_LD] = M[lane + k * LAC_LD] / sd;
        wave_lds_sync();
        for (int j = k + 1 + tj; j < nv; j += 2)
            if (ti >= j && ti < nv) M[ti + j * LAC_LD] -= M[ti + k * LAC_LD] * M[j + k * LAC_LD];
        wave_lds_sync();
    }
    double lg = (!bad && lane < nv) ? log(M[lane + lane * LAC_LD]) : 0.0;
    lg = wave_sum(lg);
    if (lane == 0) {
        a.logdet[comp] = 2 * lg;                     // moremaths.h:105-116
        if (bad) *a.errflag = 1;
    }
    if (a.fac && !bad) {                             // a copy: nothing below reads it
        double* F = a.fac + a.fac_ptr[comp];
        for (int i = i0, j = j0; j < nv;) {
            if (i >= j) F[i + j * nv] = M[i + j * LAC_LD];
            i += r64; j += q64;
            if (i >= nv) { i -= nv; ++j; }
        }
    }
    if (!a.g || bad) return;
    // ---- x = L'^-1 L^-1 g: column sweeps forward, row sweeps backward (stride LAC_LD: conflict-free)
    if (lane < nv) xs[lane] = a.g[a.vars[v0 + lane]];
    wave_lds_sync();
    for (int k = 0; k < nv; ++k) {
        const double yk = xs[k] / M[k + k * LAC_LD];
        wave_lds_sync();
        if (lane == k) xs[k] = yk;
        else if (lane > k && lane < nv) xs[lane] -= M[lane + k * LAC_LD] * yk;
        wave_lds_sync();
    }
    for (int k = nv - 1; k >= 0; --k) {
        const double xk = xs[k] / M[k + k * LAC_LD];
        wave_lds_sync();
        if (lane == k) xs[k] = xk;
        else if (lane < k) xs[lane] -= M[k + lane * LAC_LD] * xk;
        wave_lds_sync();
    }
    if (lane < nv) a.x[a.vars[v0 + lane]] = xs[lane];
}

// ------------------------------------------------------------------ a workgroup per component
constexpr int LACW_B = 16;                           // observations per staged batch: two workgroup barriers per LACW_B of them
constexpr int LACW_THREADS = 256;
// doubles of LDS: M_c (leading dimension max_vars | 1, odd as LAC_LD), LACW_B staged rows, their weights, the right-hand
// side, the waves' partial log-determinants.  146 KB at max_vars = 128 (one workgroup per CU), under 2 KB at 8
inline int lacw_ld(int max_vars) { return max_vars | 1; }
inline int lacw_lds_bytes(int max_vars)
{
    return 8 * (max_vars * lacw_ld(max_vars) + LACW_B * max_vars + LACW_B + max_vars + 4);
}
static_assert(8 * (CP_WIDE_MAX_VARS * (CP_WIDE_MAX_VARS | 1) + LACW_B * CP_WIDE_MAX_VARS + LACW_B + CP_WIDE_MAX_VARS + 4) <= CP_LDS_BYTES_PER_CU,
              "k_lac_factor_wg at the cap fits a CU");
// GLMMR_MCML_LA_WAVES=1|4: the A/B switch of the two kernel forms under "component_wide", read per call
inline int lac_forced_waves()
{
    const char* e = getenv("GLMMR_MCML_LA_WAVES");
    if (e && !strcmp(e, "1")) return 1;
    if (e && !strcmp(e, "4")) return 4;
    return -1;
}
// waves per component under "component_wide".  One wave up to CP_MAX_VARS variables and below CP_WAVES4_ROWS observations
// in the largest component (config 5: 11 and 10) -- the trajectory kernel's threshold, a guess there as here: config 4
// (400 observations) is the one measured point above it (profiles/la_component_wide_timing.json).  Forcing one wave
// above CP_MAX_VARS is ignored
inline int lac_waves(const ComponentPlan& p, int forced = -1)
{
    if (p.max_vars > CP_MAX_VARS) return 4;
    if (forced == 1 || forced == 4) return forced;
    return p.max_rows >= CP_WAVES4_ROWS ? 4 : 1;
}

// grid ncomp, LACW_THREADS threads, lacw_lds_bytes(mv) of dynamic LDS; mv = the plan's max_vars.  Every entry of M_c and of
// its factor is summed in the order of k_lac_factor: the identity, then the observations ascending, then the columns k
// ascending
__global__ __launch_bounds__(LACW_THREADS) void k_lac_factor_wg(LacArgs a, int mv)
{
    extern __shared__ __attribute__((aligned(16))) double lacw_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int comp = blockIdx.x, ld = mv | 1;
    double* M = lacw_lds;                            // column-major, ld
    double* st = M + mv * ld;                        // row b of the batch at st + b nv
    double* wb = st + LACW_B * mv;                   // its weight W_obs
    double* xs = wb + LACW_B;                        // the solves' published entries
    double* red = xs + mv;
    const int v0 = a.var_ptr[comp], nv = a.var_ptr[comp + 1] - v0;           // 1 <= nv <= mv
    const int s0 = a.slot_ptr[comp], s1 = a.slot_ptr[comp + 1];
    // entry e = tid + 256 t of the nv x nv square is (e % nv, e / nv); the lower triangle is all the factor reads
    const int q256 = LACW_THREADS / nv, r256 = LACW_THREADS % nv, i0 = tid % nv, j0 = tid / nv;
    for (int i = i0, j = j0; j < nv;) {
        M[i + j * ld] = i == j ? 1.0 : 0.0;
        i += r256; j += q256;
        if (i >= nv) { i -= nv; ++j; }
    }
    // ---- M_c = I + sum_i W_i r_i r_i'.  Every wave reads the headers of the next 64 records, one per lane: the observations
    // that end among them, LACW_B at the most, are the batch (an observation has at most 64 / CP_SLOT = 16 records)
    bool bad = false;
    int s = s0;
    while (s < s1) {
        const int t = s + lane;
        int last = 0, obs = 0;
        if (t < s1) {
            const int* ip = a.slot_i + 8 * (size_t)t;
            last = ip[5] | (t == s1 - 1);
            obs = ip[6];
        }
        const unsigned long long ends = __ballot(last);
        const int ob = __popcll(ends & ((1ull << lane) - 1));               // the observation of the batch record t belongs to
        const int total = __popcll(ends), nb = total < LACW_B ? total : LACW_B;
        if (nb == 0) { bad = true; break; }          // cannot happen with rows of ZL of at most 64 entries; uniform
        if (w == 0 && last && ob < nb) wb[ob] = a.W[obs];
        for (int b = w; b < nb; b += 4) {            // wave w sums the rows b = w, w + 4, ...: lane j entry j (and j + 64), ELL order
            const unsigned long long mine = __ballot(ob == b && t < s1);
            const int f = s + (int)__builtin_ctzll(mine), c = __popcll(mine);
            double rj = 0.0, rj2 = 0.0;
            for (int u0 = 0; u0 < c; ++u0) {
                const int* ip = a.slot_i + 8 * (size_t)(f + u0);
                const double* dp = a.slot_d + 8 * (size_t)(f + u0);
                const int ne = ip[4];
#pragma unroll
                for (int u = 0; u < CP_SLOT; ++u)
                    if (u < ne) {
                        if (ip[u] == lane) rj += dp[u];
                        if (ip[u] == lane + 64) rj2 += dp[u];
                    }
            }
            if (lane < nv) st[b * nv + lane] = rj;
            if (lane + 64 < nv) st[b * nv + lane + 64] = rj2;
        }
        lds_barrier();
        for (int i = i0, j = j0; j < nv;) {
            if (i >= j) {
                double m = M[i + j * ld];
                for (int b = 0; b < nb; ++b) m += wb[b] * st[b * nv + i] * st[b * nv + j];
                M[i + j * ld] = m;
            }
            i += r256; j += q256;
            if (i >= nv) { i -= nv; ++j; }
        }
        lds_barrier();                                 // the batch is read: the staging area is free again
        s += __popcll(__ballot(ob < nb && t < s1));
    }
    lds_barrier();
    // ---- right-looking Cholesky of the lower triangle: the column is scaled by its rows' threads, the trailing columns
    // are dealt over the waves, their rows over the lanes.  Two barriers per column: d is read by everyone before the
    // first, and overwritten by sqrt(d) after it
    for (int k = 0; k < nv && !bad; ++k) {
        const double d = M[k + k * ld];
        if (!(d > 0.0)) { bad = true; break; }       // the same value in every thread
        const double sd = sqrt(d);
        if (tid > k && tid < nv) M[tid + k * ld] = M[tid + k * ld] / sd;
        lds_barrier();
        if (tid == 0) M[k + k * ld] = sd;
        for (int j = k + 1 + w; j < nv; j += 4) {
            const double mjk = M[j + k * ld];
            for (int i = j + lane; i < nv; i += 64) M[i + j * ld] -= M[i + k * ld] * mjk;
        }
        lds_barrier();
    }
    double lg = (!bad && tid < nv) ? log(M[tid + tid * ld]) : 0.0;
    lg = wave_sum(lg);
    if (lane == 0) red[w] = lg;
    lds_barrier();
    if (tid == 0) {
        a.logdet[comp] = 2 * (((red[0] + red[1]) + red[2]) + red[3]);       // moremaths.h:105-116
        if (bad) *a.errflag = 1;
    }
    if (a.fac && !bad) {                             // a copy: nothing below reads it
        double* F = a.fac + a.fac_ptr[comp];
        for (int i = i0, j = j0; j < nv;) {
            if (i >= j) F[i + j * nv] = M[i + j * ld];
            i += r256; j += q256;
            if (i >= nv) { i -= nv; ++j; }
        }
    }
    if (!a.g || bad) return;
    // ---- x = L'^-1 L^-1 g.  Thread i keeps entry i in a register and publishes it once it is final: one barrier per column
    // (forward) and per row (backward, stride ld: conflict-free)
    double xv = tid < nv ? a.g[a.vars[v0 + tid]] : 0.0;
    for (int k = 0; k < nv; ++k) {
        if (tid == k) { xv = xv / M[k + k * ld]; xs[k] = xv; }
        lds_barrier();
        if (tid > k && tid < nv) xv -= M[tid + k * ld] * xs[k];
    }
    for (int k = nv - 1; k >= 0; --k) {
        if (tid == k) { xv = xv / M[k + k * ld]; xs[k] = xv; }
        lds_barrier();
        if (tid < k) xv -= M[k + tid * ld] * xs[k];
    }
    if (tid < nv) a.x[a.vars[v0 + tid]] = xv;
}

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
    double s = 0;
    for (int t = csr_ptr[q]; t < csr_ptr[q + 1]; ++t) s += csr_val[t] * score[csr_i[t]];
    double d = 0;
    for (int j = row_start[q]; j < row_end[q]; ++j) d += D0[q + (size_t)j * ldd] * v[j];
    out[q] = post * s - d;
}

}  // namespace mcml
