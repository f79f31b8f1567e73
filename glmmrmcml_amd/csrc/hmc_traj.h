// hmc_traj.h -- component-local HMC trajectories on the sparse chain-major operator (opt-in).
//
// The coupling graph of ZL falls into small connected components (component_plan.h), and a whole leapfrog trajectory of
// one (component, chain) pair needs no data of any other component.  k_cm_traj runs it in ONE launch per proposal: a
// wave is 64 chains of one component (lane = chain), the component's x, r and gradient accumulator live in LDS as
// [local variable][64 lanes] doubles (local indices are wave-uniform but known only at run time, and a register array
// indexed at run time goes to scratch; lane * 8 + var * 512 is conflict-free), every chain takes its own number of steps
// (lanes that have finished are masked), and V / GRAD are read once, UP / GRADP written once.  Only the accept decision is
// joint: the kernel leaves one partial per (work item, chain) of K0 = sum r0^2, sum log f(y | mu), sum log N(x; 0, 1) and
// sum r^2 at the end point, and k_cm_accept_fin<true> (hmc_cm.h) adds them in item order.  No step ring, no k_max_steps,
// no host synchronisation, and S / MU / LX / ZS are not touched.
//
// Per step the arithmetic is that of k_cm_forward + k_cm_backward + cm_leapfrog on the product form (mhmcmc.h:61-119,
// mcmlmodel.h:138-279): eta_i = xb_i + sum val x[col] over the ELL entries in order, the score of glm.h,
// acc[col] += val * s_i in ascending observation order, g = -x + post * acc, the half / full momentum updates.
// WAVES = 4 (components with many observations, config 4): the four waves of a workgroup share x and r and split the
// observations into contiguous quarters; their accumulators are added in wave order through LDS.
#pragma once
#include "hmc_cm.h"
#include "component.h"

namespace mcml {

struct TrajArgs {
    double *V, *GRAD, *UP, *GRADP;
    int ld, C, Q;
    ChainArrays ca;
    uint64_t seed; uint32_t chain_offset, iter_idx; int it;
    const double* inj_mom;
    const int* accflag;              // nullable: the previous proposal's decisions, not yet applied to V / GRAD (k_cm_propose)
    double lambda; int max_steps;
    int flink; double var_par, post;
    double *part_k0, *part_ll, *part_lp, *part_kin; int ldp;
};

// the observations of records [s0, s1) (whole observations): eta, score, accumulate.  xs / gs: this lane's column of the
// LDS arrays (element j at [j * 64])
template <int FL>
__device__ __forceinline__ void cp_rows(const CompView& m, int s0, int s1, const double* xs, double* gs, int flink,
                                        double var_par, bool want_ll, double& ll)
{
    const int fl = FL ? FL : flink;
    int s = s0;
    while (s < s1) {
        cp_i8 iv, jv; cp_d8 dv, ev;
        sload_slot(m.slot_i + 8 * (size_t)s, m.slot_d + 8 * (size_t)s, iv, dv);
        jv = iv; ev = dv;
        double acc = 0.0;
        int sa = s;
        for (;;) {
#pragma unroll
            for (int u = 0; u < CP_SLOT; ++u) if (u < jv[4]) acc += ev[u] * xs[jv[u] * 64];
            ++sa;
            if (jv[5] || sa >= s1) break;
            sload_slot(m.slot_i + 8 * (size_t)sa, m.slot_d + 8 * (size_t)sa, jv, ev);
        }
        const double yi = ev[5];
        const double mu = ev[4] + acc;
        double sc;
        if constexpr (FL == 12) sc = glm_score_beta(yi, mu, var_par);
        else sc = glm_score(yi, mu, fl);
        if (want_ll) ll += glm_logpdf(yi, mu, var_par, fl);
        if (sa == s + 1) {                                  // the usual case: the record is still in registers
#pragma unroll
            for (int u = 0; u < CP_SLOT; ++u) if (u < iv[4]) gs[iv[u] * 64] += dv[u] * sc;
        } else
            for (int sb = s; sb < sa; ++sb) {
                sload_slot(m.slot_i + 8 * (size_t)sb, m.slot_d + 8 * (size_t)sb, jv, ev);
#pragma unroll
                for (int u = 0; u < CP_SLOT; ++u) if (u < jv[4]) gs[jv[u] * 64] += ev[u] * sc;
            }
        s = sa;
    }
}

// grid (work items, chain blocks of 64), 64 * WAVES threads, dynamic LDS of cp_lds_bytes(m.max_vars, WAVES)
template <int FL, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_cm_traj(CompView m, TrajArgs a)
{
    extern __shared__ double cp_lds[];
    const int lane = threadIdx.x & 63, w = WAVES == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int MV = m.max_vars;
    double* xs = cp_lds + lane;                              // x  [var][64]
    double* rs = xs + (size_t)MV * 64;                       // r
    double* g0 = rs + (size_t)MV * 64;                       // accumulator of wave 0; afterwards the gradient
    double* gs = g0 + (size_t)w * MV * 64;                   // this wave's accumulator
    const int c = blockIdx.y * 64 + lane;
    const bool cin = c < a.C;
    const int cc = cin ? c : 0;
    const uint32_t gid = a.chain_offset + (uint32_t)cc;
    const double e = a.ca.e[cc];
    const int st = chain_step_count(a.lambda, e, a.max_steps);
    const bool accp = a.accflag && a.accflag[cc];
    const double* Vin = accp ? a.UP : a.V;
    const double* Gin = accp ? a.GRADP : a.GRAD;
    double k0 = 0.0, ll = 0.0, lp = 0.0, kin = 0.0;
    int c0, c1;
    sload_i32x2(m.item_ptr + blockIdx.x, c0, c1);
    for (int comp = c0; comp < c1; ++comp) {
        int v0, v1, s0, s1;
        sload_i32x2(m.var_ptr + comp, v0, v1);
        if constexpr (WAVES == 1) sload_i32x2(m.slot_ptr + comp, s0, s1);
        else sload_i32x2(m.slot_quarter + 5 * (size_t)comp + w, s0, s1);
        const int nv = v1 - v0;
        // ---- new_proposal, first part (k_cm_propose): momentum, first half step, position.  Four variables' loads in flight
        for (int j0 = w * 4; j0 < nv; j0 += 4 * WAVES) {
            int q[4]; double gv[4], vv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = sload_i32(m.vars + v0 + (j0 + u < nv ? j0 + u : nv - 1));
#pragma unroll
            for (int u = 0; u < 4; ++u) { const size_t off = cc + (size_t)q[u] * a.ld; gv[u] = Gin[off]; vv[u] = Vin[off]; }
            double rr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                double r = a.inj_mom ? a.inj_mom[q[u] + ((size_t)a.it * a.C + cc) * a.Q]
                                     : rng_normal(a.seed, (uint32_t)q[u], gid, (uint32_t)a.it, 16u * a.iter_idx + 2u);
                if (j0 + u < nv) k0 += r * r;
                r = r + (e / 2) * gv[u];
                rr[u] = r;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j0 + u < nv) {
                    xs[(j0 + u) * 64] = vv[u] + e * rr[u];
                    rs[(j0 + u) * 64] = rr[u];
                    if (accp && cin) { const size_t off = c + (size_t)q[u] * a.ld; a.GRAD[off] = gv[u]; a.V[off] = vv[u]; }
                }
        }
        if constexpr (WAVES > 1) __syncthreads();
        // ---- the trajectory: every lane its own st steps; the wave runs until its last lane has finished
        for (int s = 0; s < a.max_steps; ++s) {
            if (__ballot(cin && s < st) == 0ull) break;                    // the same lanes in every wave of the workgroup
            const bool wave_last = __ballot(cin && s + 1 < st) == 0ull;    // nobody moves after this step: x is the end point
            for (int j = 0; j < nv; ++j) gs[j * 64] = 0.0;
            cp_rows<FL>(m, s0, s1, xs, gs, a.flink, a.var_par, wave_last, ll);
            if constexpr (WAVES > 1) __syncthreads();
            // a lane that has finished keeps x and r: its gradient comes out the same again
            for (int j = w; j < nv; j += WAVES) {
                double acc = g0[j * 64];
                if constexpr (WAVES == 4)
                    acc = ((acc + g0[(size_t)(MV + j) * 64]) + g0[(size_t)(2 * MV + j) * 64]) + g0[(size_t)(3 * MV + j) * 64];
                const double x = xs[j * 64];
                double g = -1.0 * x;
                g = g + a.post * acc;
                g0[j * 64] = g;
                if (s < st) {                                              // cm_leapfrog, mode 1
                    double r = rs[j * 64];
                    r = r + (e / 2) * g;
                    if (s + 1 < st) { r = r + (e / 2) * g; xs[j * 64] = x + e * r; }
                    rs[j * 64] = r;
                }
            }
            if constexpr (WAVES > 1) __syncthreads();
        }
        // ---- end point: UP, GRADP, log N(x; 0, 1), r^2
        for (int j = w; j < nv; j += WAVES) {
            const int q = sload_i32(m.vars + v0 + j);
            const double x = xs[j * 64], r = rs[j * 64], g = g0[j * 64];
            lp += glm_logpdf(x, 0, 1, 7);
            kin += r * r;
            if (cin) { const size_t off = c + (size_t)q * a.ld; a.UP[off] = x; a.GRADP[off] = g; }
        }
        if constexpr (WAVES > 1) __syncthreads();                          // before the next component reuses the arrays
    }
    const size_t po = (size_t)blockIdx.x * a.ldp + c;
    if constexpr (WAVES == 1) {
        if (cin) { a.part_k0[po] = k0; a.part_ll[po] = ll; a.part_lp[po] = lp; a.part_kin[po] = kin; }
    } else {
        double* red = cp_lds + (size_t)6 * MV * 64;                        // [4 sums][4 waves][64], behind the arrays
        red[(0 * 4 + w) * 64 + lane] = k0; red[(1 * 4 + w) * 64 + lane] = ll;
        red[(2 * 4 + w) * 64 + lane] = lp; red[(3 * 4 + w) * 64 + lane] = kin;
        __syncthreads();
        if (w == 0 && cin) {
            double* out[4] = {a.part_k0, a.part_ll, a.part_lp, a.part_kin};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                out[k][po] = ((red[(k * 4 + 0) * 64 + lane] + red[(k * 4 + 1) * 64 + lane]) + red[(k * 4 + 2) * 64 + lane]) + red[(k * 4 + 3) * 64 + lane];
        }
    }
}

}  // namespace mcml
