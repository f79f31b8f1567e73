// component.h -- the device side of the component plan (component_plan.h), in one place: the view a kernel takes of the
// resident records, the idioms every kernel on the components shares, and the launchers of component.hip.
//
// Six opt-in paths run on the components: the HMC trajectories of hmc_traj.h, the component operator of the
// Laplace fits (laplace.hip, 5.5), the exact draws of hmc_exact_comp.h (5.8), the information query (info.hip, 5.9), the
// sandwich (sandwich.hip, 5.11) and the covariance parameters' information (theta_info.hip, 5.12: its k_ti_comp reads the
// factors and the plan's variable lists); the last five factorise through lac_factor_launch.
// k_cm_traj and k_exc_draw stay in the sampler's translation unit (glm.h, rng.h, hmc_chain.h) and take the CompView.
//
// APPLYING A FACTOR.  Whoever needs M^-1 or R^-1 on a few columns after the factor kernels calls, in this order,
//   comp_operator_ready    the one predicate: L set, the sparse operator active, records built
//   comp_factors_ensure    the factor scratch (CompFactors, ctx.h): offsets uploaded once per model, fac and logdet sized
//   comp_rhs_csr_launch    B = ZL' V over the CSR rows of ZL', observations ascending, for ncols columns
//   lac_factor_launch      with fac / fac_ptr of the CompFactors
//   comp_solve_launch      R_c s = b (and R_c' t = s) in place, component by component in LDS
// The packed-triangle layout, its LDS budget and the two substitution kernels live in component.hip and nowhere else.  Three
// solves stay where they are, on purpose:
//   k_exc_draw (hmc_exact_comp.h)   its back substitution sums i ASCENDING over a square triangle with an odd leading dimension
//                                   and is fused with the RNG fill and the mu* add: sharing the arithmetic would change its bits
//   k_exc_rhs (hmc_exact_comp.h)    the right-hand side post * ZL' (y - xb): scaled, and a difference of two vectors per entry
//   k_lac_factor / k_lac_factor_wg  their own solves run on the M_c they have just factorised in LDS, before it is stored
//
// A RECORD is CP_SLOT = 4 entries of one row of ZL, 8 ints in slot_i and 8 doubles in slot_d:
//   slot_i  local columns [4] | entries in the record | 1 if the observation ends here | observation | 0
//   slot_d  values [4] (comp_fill_val: whenever L changes) | xb_i | y_i (comp_fill_xy: once per sampler call) | 0 | 0
// in component order, observations ascending inside a component; an observation of w entries takes ceil(w / 4) consecutive
// records, at least one.  The pattern is fixed per model (comp_setup).
#pragma once
#include "ctx.h"

namespace mcml {

// what a kernel takes of ComponentDev; built by comp_view alone
struct CompView {
    const int *item_ptr, *var_ptr, *vars, *slot_ptr, *slot_quarter, *slot_i;
    const double* slot_d;
    int ncomp, nitems, max_vars;         // nitems: 0 unless the plan is feasible
};
inline CompView comp_view(const Ctx& c)
{
    const ComponentDev& d = c.cp;
    return CompView{d.item_ptr.as<int>(), d.var_ptr.as<int>(), d.vars.as<int>(), d.slot_ptr.as<int>(), d.slot_quarter.as<int>(),
                    d.slot_i.as<int>(), d.slot_d.d(), d.plan.ncomp, d.plan.feasible ? d.plan.nitems() : 0, d.plan.max_vars};
}

// the nv x nv square dealt over T threads: entry e = tid + T t is (e % nv, e / nv), advanced without a division per step.
// Thread tid owns the same entries in every walk
template <int T>
struct SquareWalk {
    int nv, q, r, i0, j0;
    __device__ __forceinline__ SquareWalk(int tid, int nv_) : nv(nv_), q(T / nv_), r(T % nv_), i0(tid % nv_), j0(tid / nv_) {}
    template <class F> __device__ __forceinline__ void for_each(F f) const
    {
        for (int i = i0, j = j0; j < nv;) { f(i, j); i += r; j += q; if (i >= nv) { i -= nv; ++j; } }
    }
};

// acc + entry u of a record (ip, dp: its 8 ints and 8 doubles; u < ip[4]) if it lies in local column col.  Called for u ascending: a
// column can come twice in a row of ZL, and the sum keeps the ELL order.  The value is loaded whatever the lane's column
__device__ __forceinline__ double cp_entry_of(const int* ip, const double* dp, int u, int col, double acc)
{
    const double d = dp[u];
    return ip[u] == col ? acc + d : acc;
}

// sum_t val[t] rhs(idx[t]) over row q of a CSR matrix, t ascending (ZL': observations ascending)
template <class F> __device__ __forceinline__ double csr_row_sum(const int* ptr, const int* idx, const double* val, int q, F rhs)
{
    double s = 0;
    for (int t = ptr[q]; t < ptr[q + 1]; ++t) s += val[t] * rhs(idx[t]);
    return s;
}

// ---- component.hip ----
// the plan of the ELL rows of ZL (col, width: as sparse_zl_setup builds them) and its device copies: c.cp
int comp_setup(Ctx& c, int W, const std::vector<int>& col, const std::vector<int>& width);
int comp_fill_val(Ctx& c);                                   // the records' values <- c.sp.ell_val
int comp_fill_xy(Ctx& c);                                    // the records' xb_i, y_i <- c.xb, c.y
// every M_c = I + ZL_c' diag(W) ZL_c of the resident records built and factorised in one launch: waves = 1 a wave
// (k_lac_factor), 4 a workgroup (k_lac_factor_wg) per component.  W null: W = w0 for every observation (as build_M_dense).
// logdet: ncomp.  g / x nullable: x = M^-1 g (Q).  fac / fac_ptr nullable: the factors' lower triangles, component c column-major
// (leading dimension nv_c) at fac + fac_ptr[c].  A failed pivot raises c.errflag().  launches nullable: the Laplace fits' count
// of their launches, which are the ones la_component_launch_count reports
int lac_factor_launch(Ctx& c, const double* W, double w0, const double* g, double* x, double* logdet, double* fac,
                      const int* fac_ptr, int waves, long long* launches);

// the component operator can be applied: L is set, the sparse ZL operator runs and the plan has records (no component above
// CP_WIDE_MAX_VARS variables)
inline bool comp_operator_ready(const Ctx& c) { return c.have_L && c.sp.active && c.cp.ready && c.cp.plan.records; }
// f sized for the plan of c: fac_ptr uploaded once per model (the pattern is fixed), fac = comp_factor_doubles(c) doubles,
// logdet = ncomp
int comp_factors_ensure(Ctx& c, CompFactors& f);
long long comp_factor_doubles(const Ctx& c);
// B[q, a] = sum_t csr_val[t] V[csr_i[t], a], a < ncols: row q of ZL', observations ascending (csr_row_sum).  One launch
int comp_rhs_csr_launch(Ctx& c, const double* V, int ldv, int ncols, double* B, int ldb);
// R_c s = b_c for the ncols columns of X (Q x ncols) in place, every component; back: then R_c' t = s, and only t is stored.
// One launch.  *form: 1 the plan's work items (a lane per (component, column) pair), 2 a wave per component -- the lanes take
// the columns, or, for the forward-then-back solve of ONE column, work the column together.  back with more than one column
// off the work items has no caller and no kernel
int comp_solve_launch(Ctx& c, const CompFactors& f, double* X, int ldx, int ncols, bool back, int* form);

}  // namespace mcml
