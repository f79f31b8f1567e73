// la_comp.h -- the component operator of the Laplace fits (opt-in; included by laplace.hip only).
//
// M = ZL' W ZL + I couples two variables only through an observation whose row of ZL touches both, so it is block
// diagonal over the connected components of component_plan.h: logdet M = sum_c logdet M_c and M^-1 g is solved
// component by component.  k_lac_factor builds, factorises and (optionally) solves every M_c in LDS, one wave per
// component; the vector-sized products run over the ELL / CSR arrays of the sparse ZL operator and over the
// covariance blocks of D0.  Every sum has a fixed order: no atomics, two runs are bit-identical.
#pragma once
#include "ctx.h"
#include "reduce.h"

namespace mcml {

constexpr int LAC_WAVES = 4;                         // components per workgroup (one wave each)
constexpr int LAC_LD = CP_MAX_VARS + 1;              // odd leading dimension: a row of M_c (stride LAC_LD doubles) hits distinct banks
constexpr int LAC_WAVE_DOUBLES = CP_MAX_VARS * LAC_LD + 2 * CP_MAX_VARS;   // M_c, the row r, the right-hand side
static_assert(LAC_WAVES * LAC_WAVE_DOUBLES * 8 <= 64 * 1024, "k_lac_factor keeps its LDS static");

struct LacArgs {
    const int *var_ptr, *vars, *slot_ptr;            // ComponentDev
    const int* slot_i;                               // 8 per record: local columns [4], entries, last record of its observation, observation, 0
    const double* slot_d;                            // 8 per record: values [4], (xb, y, 0, 0: not read here)
    const double* W;                                 // n
    int ncomp;
    const double* g;                                 // nullable: right-hand side (Q); x = M^-1 g is written to x
    double* x;
    double* logdet;                                  // ncomp: 2 sum log diag chol(M_c)
    int* errflag;                                    // raised on a non-positive pivot (Ctx::errflag)
};

// the lanes of ONE wave exchange data through LDS: LDS operations of a wave complete in issue order, so only the
// compiler has to be kept from moving them across
__device__ __forceinline__ void lac_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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
        lac_wave_sync();                             // the previous observation's reads of r
        if (lane < nv) r[lane] = rj;
        lac_wave_sync();
        for (int i = i0, j = j0; j < nv;) {
            M[i + j * LAC_LD] += wi * r[i] * r[j];
            i += r64; j += q64;
            if (i >= nv) { i -= nv; ++j; }
        }
    }
    lac_wave_sync();
    // ---- right-looking Cholesky of the lower triangle; lane & 31 = row, two columns of the trailing update at a time
    bool bad = false;
    const int ti = lane & 31, tj = lane >> 5;
    for (int k = 0; k < nv; ++k) {
        const double d = M[k + k * LAC_LD];
        if (!(d > 0.0)) { bad = true; break; }       // the same value in every lane
        const double sd = sqrt(d);
        lac_wave_sync();
        if (lane == k) M[k + k * LAC_LD] = sd;
        else if (lane > k && lane < nv) M[lane + k * LAC_LD] = M[lane + k * LAC_LD] / sd;
        lac_wave_sync();
        for (int j = k + 1 + tj; j < nv; j += 2)
            if (ti >= j && ti < nv) M[ti + j * LAC_LD] -= M[ti + k * LAC_LD] * M[j + k * LAC_LD];
        lac_wave_sync();
    }
    double lg = (!bad && lane < nv) ? log(M[lane + lane * LAC_LD]) : 0.0;
    lg = wave_sum(lg);
    if (lane == 0) {
        a.logdet[comp] = 2 * lg;                     // moremaths.h:105-116
        if (bad) *a.errflag = 1;
    }
    if (!a.g || bad) return;
    // ---- x = L'^-1 L^-1 g: column sweeps forward, row sweeps backward (stride LAC_LD: conflict-free)
    if (lane < nv) xs[lane] = a.g[a.vars[v0 + lane]];
    lac_wave_sync();
    for (int k = 0; k < nv; ++k) {
        const double yk = xs[k] / M[k + k * LAC_LD];
        lac_wave_sync();
        if (lane == k) xs[k] = yk;
        else if (lane > k && lane < nv) xs[lane] -= M[lane + k * LAC_LD] * yk;
        lac_wave_sync();
    }
    for (int k = nv - 1; k >= 0; --k) {
        const double xk = xs[k] / M[k + k * LAC_LD];
        lac_wave_sync();
        if (lane == k) xs[k] = xk;
        else if (lane < k) xs[lane] -= M[k + lane * LAC_LD] * xk;
        lac_wave_sync();
    }
    if (lane < nv) a.x[a.vars[v0 + lane]] = xs[lane];
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
