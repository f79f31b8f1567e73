// hmc_chain.h -- what every HMC back end shares per chain and per call: the per-chain arrays, the scalar rules of
// mcmcRunHMC (mhmcmc.h:47-117) and the shape of the sample matrix.  The kernels of hmc.hip (column-major state),
// hmc_cm.h (chain-major) and hmc_traj.h (component trajectories) call the rules; each rule is written here once, as the
// plain IEEE sequence the CPU oracle evaluates (-ffp-contract=off), so a chain decides the same in every back end.
// NUTS keeps its own NutsChain and Stan's rules (nuts.h).
#pragma once
#include "../../include/glmmr_mcml_c.h"
#include "ctx.h"
#include "rng.h"

namespace mcml {

struct ChainArrays {
    double *e, *ebar, *H, *lpcur, *K0;
    int *steps, *acc;
    uint32_t* gen;
    long long* leap;
};

inline ChainArrays chain_arrays(const HmcState& h)
{
    ChainArrays a;
    const size_t C = (size_t)round_up(h.C, 16);
    double* d = h.chain.d();
    a.e = d; a.ebar = d + C; a.H = d + 2 * C; a.lpcur = d + 3 * C; a.K0 = d + 4 * C;
    a.leap = reinterpret_cast<long long*>(d + 5 * C);
    a.steps = reinterpret_cast<int*>(d + 6 * C);
    a.acc = a.steps + C;
    a.gen = reinterpret_cast<uint32_t*>(a.acc + C);
    return a;
}

// ---- the rules of one chain c ----------------------------------------------------------------------------------------
// initialise_u, mhmcmc.h:47-59; gid: the chain's global number (its minstd seed, rng.h)
__device__ __forceinline__ void chain_reset(const ChainArrays& ca, int c, uint64_t seed, uint32_t gid, uint32_t iter_idx)
{
    ca.e[c] = 0.001; ca.ebar[c] = 1.0; ca.H[c] = 0.0; ca.acc[c] = 0; ca.leap[c] = 0;
    ca.gen[c] = chain_minstd_seed(seed, gid, iter_idx);
    ca.steps[c] = 1;
}

// leapfrog steps of a proposal with step size e, mhmcmc.h:69-70.  Stores nothing
__device__ __forceinline__ int chain_step_count(double lambda, double e, int max_steps)
{
    double st = round(lambda / e);
    if (!(st >= 1.0)) st = 1.0;
    if (st > (double)max_steps) st = (double)max_steps;
    return (int)st;
}

// new_proposal, first part (mhmcmc.h:62-75), once the momentum is drawn: sum_r2 = sum of its squares
__device__ __forceinline__ void chain_begin_proposal(const ChainArrays& ca, int c, double sum_r2, double lambda, int max_steps)
{
    ca.K0[c] = 0.5 * sum_r2;
    const int st = chain_step_count(lambda, ca.e[c], max_steps);
    ca.steps[c] = st;
    ca.leap[c] += (long long)st;
}

// new_proposal, second part (mhmcmc.h:80-117): the Metropolis decision with the chain's minstd draw, then dual averaging
// (:107-114) or e = ebar (:116).  l2: log_prob at the end point, kin: sum of the end point's squared momenta.  flags / probs
// (nullable, C per proposal) get the decision and its probability.  Returns 1 if the proposal is accepted
__device__ __forceinline__ int chain_decide(const ChainArrays& ca, int c, double l2, double kin, double target_accept, int adapt,
                                            int it, int C, uint8_t* flags, double* probs)
{
    const double lprt = 0.5 * kin, lpr = ca.K0[c], l1 = ca.lpcur[c];
    const double prob = fmin(1.0, exp(-l1 + lpr + l2 - lprt));
    uint32_t g = ca.gen[c];
    const double runif = minstd_canonical(g);
    ca.gen[c] = g;
    const int acc = runif < prob;
    if (acc) { ca.lpcur[c] = l2; ca.acc[c] += 1; }
    if (flags) flags[c + (size_t)it * C] = (uint8_t)acc;
    if (probs) probs[c + (size_t)it * C] = prob;
    if (adapt) {
        const int iter = it + 1;
        const double f1 = 1.0 / (iter + 10);
        const double H = (1 - f1) * ca.H[c] + f1 * (target_accept - prob);
        ca.H[c] = H;
        const double loge = -4.60517 - (sqrt((double)iter / 0.05)) * H;
        const double powm = pow((double)iter, -0.75);
        const double logbare = powm * loge + (1 - powm) * log(ca.ebar[c]);
        ca.e[c] = exp(loge);
        ca.ebar[c] = exp(logbare);
    } else {
        ca.e[c] = ca.ebar[c];
    }
    return acc;
}

// ---- the sample matrix of one sampler call -----------------------------------------------------------------------------
// C chains draw d times each after `warmup` proposals: `total` proposals, Q x ncols samples.  Chain c's draw k is column
// c * d + k.  One HMC chain keeps the reference's layout instead (mhmcmc.h:126,142,147): nsamp + 1 columns, column 0 the state
// after the warm-up.  D5: the reference's beta-step then reads niter = nsamp columns (mcmlmodel.h:73) while the theta-step
// reads all mcols = nsamp + 1 (mcmldmatrix.h:24); everywhere else niter = ncols.
struct SampleShape {
    int C, d, total, ncols, niter, warmup;
    bool single_chain_layout;
    // the proposal `it`'s draw: its column for chain 0 and the distance to the next chain's (*stride), or -1: not stored
    int column_of(int it, int* stride) const
    {
        *stride = single_chain_layout ? 0 : d;
        if (single_chain_layout) return it >= warmup - 1 ? it - warmup + 1 : -1;      // samples.col(0) = u_, :142; col(i + 1), :147
        return it >= warmup ? it - warmup : -1;
    }
};
inline SampleShape sample_shape(int nsamp, int warmup, int chains, bool nuts = false)
{
    SampleShape s;
    s.C = chains > 0 ? chains : 1;
    s.single_chain_layout = s.C == 1 && !nuts;                    // NUTS (gen_u_samples.R) has no column 0
    s.d = (nsamp + s.C - 1) / s.C;
    s.warmup = warmup; s.total = warmup + s.d;
    s.ncols = s.single_chain_layout ? s.d + 1 : s.C * s.d;
    s.niter = s.single_chain_layout ? s.d : s.ncols;
    return s;
}
// the inverse for the samplers that fill whole columns (exact draws): column j is draw *draw of chain *chain
__host__ __device__ __forceinline__ void draw_of_column(int j, int C, int d, uint32_t* chain, uint32_t* draw)
{
    *chain = C > 1 ? (uint32_t)(j / d) : 0u;
    *draw = C > 1 ? (uint32_t)(j % d) : (uint32_t)j;
}

// the tail of a call whose draws are exact: every proposal counts as accepted, no step size, no leapfrog steps
inline void exact_finish(const SampleShape& s, uint8_t* flags_out, double* probs_out, glmmr_mcml_hmc_diag* diag, int* ncols_out)
{
    const size_t np = (size_t)s.C * s.total;
    if (flags_out) memset(flags_out, 1, np);
    if (probs_out) for (size_t i = 0; i < np; ++i) probs_out[i] = 1.0;
    if (diag) {
        diag->accept_rate = 1.0;
        diag->mean_e = 0.0; diag->min_e = 0.0; diag->max_e = 0.0;
        diag->max_steps_used = 0; diag->leapfrog_total = 0;
    }
    if (ncols_out) *ncols_out = s.ncols;
}

}  // namespace mcml
