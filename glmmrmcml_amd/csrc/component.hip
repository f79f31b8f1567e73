// component.hip -- the device side of the component plan (component.h): the upload of a ComponentPlan, the two kernels that fill
// the records, the component operator M = ZL' W ZL + I of the Laplace fits, the exact draws (5.8) and the two
// queries (5.9, 5.11), and what applies its factors afterwards: the scratch, the CSR right-hand side, the substitutions.
// M couples two variables only through an observation whose row of ZL touches both, so it is block diagonal over the
// connected components of component_plan.h: logdet M = sum_c logdet M_c and M^-1 g is solved component by component.
// k_lac_factor builds, factorises and (optionally) solves every M_c in LDS, one wave per component; k_lac_factor_wg gives a
// component a workgroup of four waves and M_c a dynamically sized piece of LDS (up to CP_WIDE_MAX_VARS variables; the
// observations are staged in batches that the waves share).  Every sum has a fixed order -- the identity, then the
// observations ascending, then the columns ascending: no atomics, two runs are bit-identical.
#include "component.h"
#include "entry.h"
#include "reduce.h"
#include <atomic>

namespace mcml {

// ------------------------------------------------------------------ the plan on the device, the records' values
int comp_setup(Ctx& c, int W, const std::vector<int>& col, const std::vector<int>& width)
{
    ComponentDev& cp = c.cp;
    component_plan_build(c.n, c.Q, W, col, width, cp.plan);
    cp.ready = false;
    const ComponentPlan& p = cp.plan;
    if (!p.records) return MCML_OK;
    auto up = [&](DevBuf& b, const std::vector<int>& v) -> int {   // item_ptr stays empty above CP_MAX_VARS
        MCML_TRY(b.ensure(sizeof(int) * (v.size() + 8)));
        return copy_h2d(b.p, v.data(), sizeof(int) * v.size(), c.stream);
    };
    MCML_TRY(up(cp.item_ptr, p.item_ptr)); MCML_TRY(up(cp.var_ptr, p.var_ptr)); MCML_TRY(up(cp.vars, p.vars));
    MCML_TRY(up(cp.slot_ptr, p.slot_ptr)); MCML_TRY(up(cp.slot_quarter, p.slot_quarter));
    MCML_TRY(up(cp.slot_i, p.slot_i)); MCML_TRY(up(cp.slot_src, p.slot_src));
    MCML_TRY(cp.slot_d.ensure(sizeof(double) * 8 * (size_t)(p.nslots + 1)));
    MCML_HIP(hipMemsetAsync(cp.slot_d.p, 0, sizeof(double) * 8 * (size_t)(p.nslots + 1), c.stream));
    cp.ready = true;
    return MCML_OK;
}

// entry t of the records' 4 nslots values: ell_val permuted (slot_src: index into ell_val, -1 for padding)
__global__ __launch_bounds__(256) void k_cp_fill_val(long tot, const int* slot_src, const double* ell_val, double* slot_d)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= tot) return;
    const int src = slot_src[t];
    slot_d[8 * (t >> 2) + (t & 3)] = src >= 0 ? ell_val[src] : 0.0;
}
int comp_fill_val(Ctx& c)
{
    const long te = 4L * c.cp.plan.nslots;
    hipLaunchKernelGGL(k_cp_fill_val, dim3((unsigned)((te + 255) / 256)), dim3(256), 0, c.stream, te, c.cp.slot_src.as<int>(),
                       c.sp.ell_val.d(), c.cp.slot_d.d());
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

// xb_i and y_i of a record's observation (xb changes with beta)
__global__ __launch_bounds__(256) void k_cp_fill_xy(int nslots, const int* slot_i, const double* xb, const double* y, double* slot_d)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nslots) return;
    const int i = slot_i[8 * (size_t)s + 6];
    slot_d[8 * (size_t)s + 4] = xb[i]; slot_d[8 * (size_t)s + 5] = y[i];
}
int comp_fill_xy(Ctx& c)
{
    const int ns = c.cp.plan.nslots;
    hipLaunchKernelGGL(k_cp_fill_xy, dim3((ns + 255) / 256), dim3(256), 0, c.stream, ns, c.cp.slot_i.as<int>(), c.xb.d(), c.y.d(),
                       c.cp.slot_d.d());
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

// ------------------------------------------------------------------ a wave per component
constexpr int LAC_WAVES = 4;                         // components per workgroup (one wave each)
constexpr int LAC_LD = CP_MAX_VARS + 1;              // odd leading dimension: a row of M_c (stride LAC_LD doubles) hits distinct banks
constexpr int LAC_WAVE_DOUBLES = CP_MAX_VARS * LAC_LD + 2 * CP_MAX_VARS;   // M_c, the row r, the right-hand side
static_assert(LAC_WAVES * LAC_WAVE_DOUBLES * 8 <= 64 * 1024, "k_lac_factor keeps its LDS static");

struct LacArgs {
    CompView cv;                                     // xb and y of the records are not read here
    const double* W; double w0;                      // W: n, or null: w0 for every observation
    const double* g; double* x;                      // g nullable: right-hand side (Q); x = M^-1 g is written to x
    double* logdet;                                  // ncomp: 2 sum log diag chol(M_c)
    int* errflag;                                    // raised on a non-positive pivot (Ctx::errflag)
    double* fac;                                     // nullable: the lower triangle of chol(M_c), diagonal included, is stored
    const int* fac_ptr;                              // column-major (leading dimension nv) at fac + fac_ptr[comp] (hmc_exact_comp.h)
};

// grid ceil(ncomp / LAC_WAVES), 64 * LAC_WAVES threads.  No workgroup barrier: the waves are independent
__global__ __launch_bounds__(64 * LAC_WAVES) void k_lac_factor(LacArgs a)
{
    __shared__ double lds[LAC_WAVES * LAC_WAVE_DOUBLES];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int comp = blockIdx.x * LAC_WAVES + w;
    if (comp >= a.cv.ncomp) return;
    double* M = lds + (size_t)w * LAC_WAVE_DOUBLES;  // column-major, LAC_LD
    double* r = M + CP_MAX_VARS * LAC_LD;
    double* xs = r + CP_MAX_VARS;
    const int v0 = a.cv.var_ptr[comp], nv = a.cv.var_ptr[comp + 1] - v0;     // 1 <= nv <= CP_MAX_VARS
    const int s0 = a.cv.slot_ptr[comp], s1 = a.cv.slot_ptr[comp + 1];
    const SquareWalk<64> sq(lane, nv);
    sq.for_each([&](int i, int j) { M[i + j * LAC_LD] = i == j ? 1.0 : 0.0; });
    // ---- M_c = I + sum_i W_i r_i r_i', observations ascending.  Lane j sums entry j of the row over the observation's
    // records, then every entry of the square has one owner lane
    int s = s0;
    while (s < s1) {
        double rj = 0.0;
        int obs;
        for (;;) {
            const int* ip = a.cv.slot_i + 8 * (size_t)s;
            const double* dp = a.cv.slot_d + 8 * (size_t)s;
            const int ne = ip[4], last = ip[5]; obs = ip[6];
#pragma unroll
            for (int u = 0; u < CP_SLOT; ++u) if (u < ne) rj = cp_entry_of(ip, dp, u, lane, rj);
            ++s;
            if (last || s >= s1) break;
        }
        const double wi = a.W ? a.W[obs] : a.w0;
        wave_lds_sync();                             // the previous observation's reads of r
        if (lane < nv) r[lane] = rj;
        wave_lds_sync();
        sq.for_each([&](int i, int j) { M[i + j * LAC_LD] += wi * r[i] * r[j]; });
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
        sq.for_each([&](int i, int j) { if (i >= j) F[i + j * nv] = M[i + j * LAC_LD]; });
    }
    if (!a.g || bad) return;
    // ---- x = L'^-1 L^-1 g: column sweeps forward, row sweeps backward (stride LAC_LD: conflict-free)
    if (lane < nv) xs[lane] = a.g[a.cv.vars[v0 + lane]];
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
    if (lane < nv) a.x[a.cv.vars[v0 + lane]] = xs[lane];
}

// ------------------------------------------------------------------ a workgroup per component
constexpr int LACW_B = 16;                           // observations per staged batch: two workgroup barriers per LACW_B of them
constexpr int LACW_THREADS = 256;
// bytes of LDS: M_c (leading dimension max_vars | 1, odd as LAC_LD), LACW_B staged rows, their weights, the right-hand
// side, the waves' partial log-determinants.  146 KB at max_vars = 128 (one workgroup per CU), under 2 KB at 8
constexpr int lacw_lds_bytes(int mv) { return 8 * (mv * (mv | 1) + LACW_B * mv + LACW_B + mv + 4); }
static_assert(lacw_lds_bytes(CP_WIDE_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_lac_factor_wg at the cap fits a CU");

// grid ncomp, LACW_THREADS threads, lacw_lds_bytes(max_vars) of dynamic LDS.  Every entry of M_c and of its factor is summed
// in the order of k_lac_factor: the identity, then the observations ascending, then the columns k ascending
__global__ __launch_bounds__(LACW_THREADS) void k_lac_factor_wg(LacArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lacw_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int comp = blockIdx.x, mv = a.cv.max_vars, ld = mv | 1;
    double* M = lacw_lds;                            // column-major, ld
    double* st = M + mv * ld;                        // row b of the batch at st + b nv
    double* wb = st + LACW_B * mv;                   // its weight W_obs
    double* xs = wb + LACW_B;                        // the solves' published entries
    double* red = xs + mv;
    const int v0 = a.cv.var_ptr[comp], nv = a.cv.var_ptr[comp + 1] - v0;     // 1 <= nv <= mv
    const int s0 = a.cv.slot_ptr[comp], s1 = a.cv.slot_ptr[comp + 1];
    const SquareWalk<LACW_THREADS> sq(tid, nv);      // the lower triangle is all the factor reads
    sq.for_each([&](int i, int j) { M[i + j * ld] = i == j ? 1.0 : 0.0; });
    // ---- M_c = I + sum_i W_i r_i r_i'.  Every wave reads the headers of the next 64 records, one per lane: the observations
    // that end among them, LACW_B at the most, are the batch (an observation has at most 64 / CP_SLOT = 16 records)
    bool bad = false;
    int s = s0;
    while (s < s1) {
        const int t = s + lane;
        int last = 0, obs = 0;
        if (t < s1) {
            const int* ip = a.cv.slot_i + 8 * (size_t)t;
            last = ip[5] | (t == s1 - 1);
            obs = ip[6];
        }
        const unsigned long long ends = __ballot(last);
        const int ob = __popcll(ends & ((1ull << lane) - 1));               // the observation of the batch record t belongs to
        const int total = __popcll(ends), nb = total < LACW_B ? total : LACW_B;
        if (nb == 0) { bad = true; break; }          // cannot happen with rows of ZL of at most 64 entries; uniform
        if (w == 0 && last && ob < nb) wb[ob] = a.W ? a.W[obs] : a.w0;
        for (int b = w; b < nb; b += 4) {            // wave w sums the rows b = w, w + 4, ...: lane j entry j (and j + 64), ELL order
            const unsigned long long mine = __ballot(ob == b && t < s1);
            const int f = s + (int)__builtin_ctzll(mine), c = __popcll(mine);
            double rj = 0.0, rj2 = 0.0;
            for (int u0 = 0; u0 < c; ++u0) {
                const int* ip = a.cv.slot_i + 8 * (size_t)(f + u0);
                const double* dp = a.cv.slot_d + 8 * (size_t)(f + u0);
                const int ne = ip[4];
#pragma unroll
                for (int u = 0; u < CP_SLOT; ++u)
                    if (u < ne) { rj = cp_entry_of(ip, dp, u, lane, rj); rj2 = cp_entry_of(ip, dp, u, lane + 64, rj2); }
            }
            if (lane < nv) st[b * nv + lane] = rj;
            if (lane + 64 < nv) st[b * nv + lane + 64] = rj2;
        }
        lds_barrier();
        sq.for_each([&](int i, int j) {
            if (i >= j) {
                double m = M[i + j * ld];
                for (int b = 0; b < nb; ++b) m += wb[b] * st[b * nv + i] * st[b * nv + j];
                M[i + j * ld] = m;
            }
        });
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
        sq.for_each([&](int i, int j) { if (i >= j) F[i + j * nv] = M[i + j * ld]; });
    }
    if (!a.g || bad) return;
    // ---- x = L'^-1 L^-1 g.  Thread i keeps entry i in a register and publishes it once it is final: one barrier per column
    // (forward) and per row (backward, stride ld: conflict-free)
    double xv = tid < nv ? a.g[a.cv.vars[v0 + tid]] : 0.0;
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
    if (tid < nv) a.x[a.cv.vars[v0 + tid]] = xv;
}

// the Laplace fits' k_lac_factor / k_lac_factor_wg launches of this process, over all contexts (glmmr_mcml_dbg_la_component_launches)
static std::atomic<long long> g_lac_launches{0};
long long la_component_launch_count() { return g_lac_launches.load(); }

int lac_factor_launch(Ctx& c, const double* W, double w0, const double* g, double* x, double* logdet, double* fac,
                      const int* fac_ptr, int waves, long long* launches)
{
    const LacArgs a{comp_view(c), W, w0, g, x, logdet, c.errflag(), fac, fac_ptr};
    if (waves == 4) {
        MCML_TRY(ensure_dynamic_lds((const void*)k_lac_factor_wg, lacw_lds_bytes(CP_WIDE_MAX_VARS)));
        hipLaunchKernelGGL(k_lac_factor_wg, dim3(a.cv.ncomp), dim3(LACW_THREADS), lacw_lds_bytes(a.cv.max_vars), c.stream, a);
    } else {
        hipLaunchKernelGGL(k_lac_factor, dim3((a.cv.ncomp + LAC_WAVES - 1) / LAC_WAVES), dim3(64 * LAC_WAVES), 0, c.stream, a);
    }
    MCML_HIP(hipGetLastError());
    if (launches) { ++*launches; ++g_lac_launches; }
    return MCML_OK;
}

// ------------------------------------------------------------------ applying the factors: scratch, right-hand side, solves
long long comp_factor_doubles(const Ctx& c) { return comp_factor_offsets(c.cp.plan).back(); }

int comp_factors_ensure(Ctx& c, CompFactors& f)
{
    if (!f.doubles) {                                             // the pattern is fixed per model
        const std::vector<int> off = comp_factor_offsets(c.cp.plan);
        MCML_TRY(f.fac_ptr.ensure(sizeof(int) * off.size()));
        MCML_TRY(copy_h2d(f.fac_ptr.p, off.data(), sizeof(int) * off.size(), c.stream));
        MCML_HIP(hipStreamSynchronize(c.stream));
        MCML_TRY(f.fac.ensure(sizeof(double) * (size_t)off.back()));
        f.doubles = off.back();
    }
    return f.logdet.ensure(sizeof(double) * (size_t)c.cp.plan.ncomp);
}

__global__ __launch_bounds__(256) void k_comp_rhs_csr(const int* csr_ptr, const int* csr_i, const double* csr_val, const double* V,
                                                      int ldv, int Q, int ncols, double* B, int ldb)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    for (int a = blockIdx.y; a < ncols; a += gridDim.y) {
        const double* col = V + (size_t)a * ldv;
        B[q + (size_t)a * ldb] = csr_row_sum(csr_ptr, csr_i, csr_val, q, [&](int i) { return col[i]; });
    }
}
int comp_rhs_csr_launch(Ctx& c, const double* V, int ldv, int ncols, double* B, int ldb)
{
    hipLaunchKernelGGL(k_comp_rhs_csr, dim3((c.Q + 255) / 256, ncols < 1024 ? ncols : 1024), dim3(256), 0, c.stream,
                       c.sp.csr_ptr.as<int>(), c.sp.csr_i.as<int>(), c.sp.csr_val.d(), V, ldv, c.Q, ncols, B, ldb);
    MCML_HIP(hipGetLastError());
    return MCML_OK;
}

// ---- the substitutions.  R_c is staged from the factor scratch as PACKED ROWS -- entry (k, i), i <= k, at k (k + 1) / 2 + i --
// so that a wave's own block of LDS holds the triangle and the vectors side by side at CP_WIDE_MAX_VARS (a square with an odd
// leading dimension as in k_lac_factor_wg would take 129 KB and leave the vectors 31 KB).  Components staged side by side sit
// at an ODD stride.  A lane that solves for its own component walks a row of its triangle in the forward substitution and a
// COLUMN (entry (i, k), i descending) in the back substitution: either way the lanes of a group of 32 sit at the SAME offset
// inside their triangles (lanes whose component is smaller are masked), so their addresses differ by multiples of the odd
// stride and fall into 32 different pairs of banks; lanes of one component read one address, a broadcast.  The odd stride
// that keeps the row walk free of conflicts keeps the column walk free of them as well (checked on the address formula, not
// measured).
constexpr int CSOLVE_WAVES = 4;
constexpr int CSOLVE_R_DOUBLES = 1024;               // a wave's room for staged triangles in the item form
constexpr int csolve_stride(int mv) { return (mv * (mv + 1) / 2) | 1; }
constexpr int csolve_r_doubles(int mv) { return mv <= CP_MAX_VARS && csolve_stride(mv) < CSOLVE_R_DOUBLES ? CSOLVE_R_DOUBLES : csolve_stride(mv); }
constexpr int csolve_waves(int mv) { return mv <= CP_MAX_VARS ? CSOLVE_WAVES : 1; }
constexpr int csolve_lds_bytes(int mv) { return 8 * csolve_waves(mv) * (mv * 64 + csolve_r_doubles(mv)); }   // k_comp_solve
constexpr int csolve_wave_lds_bytes(int mv) { return 8 * (csolve_stride(mv) + mv); }                         // k_comp_solve_wave
constexpr int CSOLVE_LDS_CAP = csolve_lds_bytes(CP_MAX_VARS) > csolve_lds_bytes(CP_WIDE_MAX_VARS) ? csolve_lds_bytes(CP_MAX_VARS)
                                                                                                    : csolve_lds_bytes(CP_WIDE_MAX_VARS);
static_assert(CSOLVE_LDS_CAP <= CP_LDS_BYTES_PER_CU, "k_comp_solve, staged items and one wave at their caps");
static_assert(csolve_wave_lds_bytes(CP_WIDE_MAX_VARS) <= CP_LDS_BYTES_PER_CU, "k_comp_solve_wave at the cap");

struct CompSolveArgs {
    CompView cv;                         // items != 0: a wave takes work item t = components [item_ptr[t], item_ptr[t + 1]); else component t
    const int* fac_ptr;                  // CompFactors: the factors of lac_factor_launch, lower triangles, leading dimension nv_c
    const double* fac;
    double* X;                           // Q x ncols, in: b, out: s or t
    size_t ldx;
    int ncols, items;
};

// packed rows of the lower triangle of F (nv x nv, column-major) -> Rs, by the whole wave
__device__ __forceinline__ void comp_stage_packed(const double* F, int nv, double* Rs, int lane)
{
    for (int e = lane; e < nv * nv; e += 64) {
        const int i = e % nv, j = e / nv;
        if (i >= j) Rs[i * (i + 1) / 2 + j] = F[e];
    }
}

// A lane owns one (component, column) pair and runs the substitutions for it, its vector in LDS as [variable][lane] (the layout
// of k_exc_draw: the 32 lanes of a half read consecutive doubles).  Two forms, picked by the plan as for k_exc_draw:
//   staged items   components up to CP_MAX_VARS variables: CSOLVE_WAVES waves per workgroup, a wave per work item; the item's
//                  components are staged G at a time and the lanes enumerate (component, column) pairs.  With 2 columns and
//                  components of 11 variables (config 5) 15 components keep 30 lanes busy
//   one component  up to CP_WIDE_MAX_VARS: one wave per workgroup and component, every read of R_c a broadcast
// More than 64 pairs are worked through 64 at a time (one component: the columns in chunks of 64).  BACK = false stores s,
// BACK = true only t.  grid ceil(items / waves), 64 * waves threads, csolve_lds_bytes(max_vars) of dynamic LDS.  No workgroup barrier
template <bool BACK>
__global__ __launch_bounds__(64 * CSOLVE_WAVES) void k_comp_solve(CompSolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double csolve_lds[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blockIdx.x * (a.items ? CSOLVE_WAVES : 1) + w;
    if (item >= (a.items ? a.cv.nitems : a.cv.ncomp)) return;
    const int mv = a.cv.max_vars, stride = csolve_stride(mv), rd = csolve_r_doubles(mv);
    double* x = csolve_lds + (size_t)w * (mv * 64 + rd);                         // [variable][lane]
    double* R = x + mv * 64;                                                     // slot s at R + s stride
    const int G = a.items ? (rd / stride < 64 ? rd / stride : 64) : 1;           // components staged side by side, >= 1
    const int c0 = a.items ? a.cv.item_ptr[item] : item, c1 = a.items ? a.cv.item_ptr[item + 1] : item + 1;
    for (int cs = c0; cs < c1; cs += G) {
        const int g = c1 - cs < G ? c1 - cs : G;
        wave_lds_sync();                             // the previous group's reads of R
        for (int s = 0; s < g; ++s)
            comp_stage_packed(a.fac + a.fac_ptr[cs + s], a.cv.var_ptr[cs + s + 1] - a.cv.var_ptr[cs + s], R + s * stride, lane);
        wave_lds_sync();
        for (int e = lane; e < g * a.ncols; e += 64) {
            const int s = e / a.ncols, col = e - s * a.ncols;
            const int v0 = a.cv.var_ptr[cs + s], nv = a.cv.var_ptr[cs + s + 1] - v0;     // 1 <= nv <= mv
            const double* Rs = R + s * stride;
            double* Xc = a.X + (size_t)col * a.ldx;
            // s_k = (b_k - sum_{i < k} R_c[k, i] s_i) / R_c[k, k], i ascending
            for (int k = 0; k < nv; ++k) {
                const int q = a.cv.vars[v0 + k];
                const double* row = Rs + k * (k + 1) / 2;
                double acc = Xc[q];
                for (int i = 0; i < k; ++i) acc -= row[i] * x[i * 64 + lane];
                acc = acc / row[k];
                x[k * 64 + lane] = acc;
                if (!BACK) Xc[q] = acc;
            }
            if (!BACK) continue;
            // t_k = (s_k - sum_{i > k} R_c[i, k] t_i) / R_c[k, k], i descending: column k of the packed triangle
            for (int k = nv - 1; k >= 0; --k) {
                double acc = x[k * 64 + lane];
                for (int i = nv - 1; i > k; --i) acc -= Rs[i * (i + 1) / 2 + k] * x[i * 64 + lane];
                acc = acc / Rs[k * (k + 1) / 2 + k];
                x[k * 64 + lane] = acc;
                Xc[a.cv.vars[v0 + k]] = acc;
            }
        }
    }
}

// R_c s = b, R_c' t = s for ONE column of a component of up to CP_WIDE_MAX_VARS variables, the whole wave on it (a lane-serial
// solve would idle 63 lanes): the vector x[nv] in LDS, lane i takes x_i -= R[i, k] x_k (forward, a column of the packed
// triangle: the offsets i (i + 1) / 2 of 32 consecutive i are distinct modulo 32, no conflict) or x_i -= R[k, i] x_k (back,
// a row: consecutive).  Every x_i receives its updates in the order the lane of k_comp_solve<true> applies them -- forward k
// ascending, back k descending -- so the two give the same bits.  grid ncomp, 64 threads, csolve_wave_lds_bytes(max_vars)
__global__ __launch_bounds__(64) void k_comp_solve_wave(CompSolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double csolve_lds[];
    const int lane = threadIdx.x & 63, comp = blockIdx.x;
    if (comp >= a.cv.ncomp) return;
    const int v0 = a.cv.var_ptr[comp], nv = a.cv.var_ptr[comp + 1] - v0;         // 1 <= nv <= max_vars
    double* R = csolve_lds;
    double* x = csolve_lds + csolve_stride(a.cv.max_vars);
    comp_stage_packed(a.fac + a.fac_ptr[comp], nv, R, lane);
    for (int k = lane; k < nv; k += 64) x[k] = a.X[a.cv.vars[v0 + k]];
    wave_lds_sync();
    for (int k = 0; k < nv; ++k) {                                               // R s = b
        const double sk = x[k] / R[k * (k + 1) / 2 + k];
        wave_lds_sync();                                                         // every lane has read x[k]
        if (lane == 0) x[k] = sk;
        for (int i = k + 1 + lane; i < nv; i += 64) x[i] -= R[i * (i + 1) / 2 + k] * sk;
        wave_lds_sync();
    }
    for (int k = nv - 1; k >= 0; --k) {                                          // R' t = s
        const double* row = R + k * (k + 1) / 2;
        const double tk = x[k] / row[k];
        wave_lds_sync();
        if (lane == 0) x[k] = tk;
        for (int i = lane; i < k; i += 64) x[i] -= row[i] * tk;
        wave_lds_sync();
    }
    for (int k = lane; k < nv; k += 64) a.X[a.cv.vars[v0 + k]] = x[k];
}

int comp_solve_launch(Ctx& c, const CompFactors& f, double* X, int ldx, int ncols, bool back, int* form)
{
    const ComponentPlan& p = c.cp.plan;
    const bool items = p.feasible;                                // max_vars <= CP_MAX_VARS: the plan's work items are built
    MCML_REQUIRE(p.records && ncols >= 1 && (!back || items || ncols == 1), "component solve: %d columns, %d variables, back %d",
                 ncols, p.max_vars, (int)back);
    const CompSolveArgs a{comp_view(c), f.fac_ptr.as<int>(), f.fac.d(), X, (size_t)ldx, ncols, items ? 1 : 0};
    const int nw = csolve_waves(p.max_vars), cnt = items ? a.cv.nitems : a.cv.ncomp;
    const dim3 grid((cnt + nw - 1) / nw), block(64 * nw);
    // the attribute is set once per kernel and device, so to the larger of the caps of its forms
    if (!back) {
        MCML_TRY(ensure_dynamic_lds((const void*)k_comp_solve<false>, CSOLVE_LDS_CAP));
        hipLaunchKernelGGL(k_comp_solve<false>, grid, block, csolve_lds_bytes(p.max_vars), c.stream, a);
    } else if (items) {
        MCML_TRY(ensure_dynamic_lds((const void*)k_comp_solve<true>, CSOLVE_LDS_CAP));
        hipLaunchKernelGGL(k_comp_solve<true>, grid, block, csolve_lds_bytes(p.max_vars), c.stream, a);
    } else {
        MCML_TRY(ensure_dynamic_lds((const void*)k_comp_solve_wave, csolve_wave_lds_bytes(CP_WIDE_MAX_VARS)));
        hipLaunchKernelGGL(k_comp_solve_wave, dim3(a.cv.ncomp), dim3(64), csolve_wave_lds_bytes(p.max_vars), c.stream, a);
    }
    MCML_HIP(hipGetLastError());
    *form = items ? 1 : 2;
    return MCML_OK;
}

}  // namespace mcml
