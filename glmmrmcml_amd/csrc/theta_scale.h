// theta_scale.h -- candidates of a theta-step that differ in a pure SCALE parameter share one factorisation.
//
// If D(theta) = s(theta) R(theta_rest) with s = prod_i theta_i^{p_i} (the p_i proved from the covariance specification,
// never inferred numerically), then for two candidates with the same theta_rest and log ratio lr = log s' - log s
//     logdet D' = logdet D + dim lr          || inv(L') U ||^2 = || inv(L) U ||^2 exp(-lr)
// -- the two scalars the MVN log-likelihood is made of (mvn.hip k_finish_large).  One member of such a group (its
// representative: the first in candidate order) is built, factorised and solved; the others get their value on the
// host from the representative's two scalars.  Host code only: no HIP calls here (tests/host_theta_scale_driver.cpp
// builds it alone).
#pragma once
#include "covspec.h"
#include <cmath>
#include <cstring>
#include <map>

namespace mcml {

// Exponents p_i >= 0, one per covariance parameter: D(theta) = (prod theta_i^{p_i}) R(theta_j : p_j = 0) for the WHOLE
// D.  Every entry of a block is the product of its rows' terms (cov_term), so a block is homogeneous of degree
// sum(rows' exponents at i) in theta_i, provided no row of the block reads theta_i as anything but a scale.  A
// coordinate qualifies when that degree is the same, and positive, in every block and nothing anywhere reads it
// otherwise; all others get 0 (several formulas with parameters of their own: each scales its own blocks only).
inline std::vector<int> theta_scale_exponents(const CovSpec& cs)
{
    std::vector<int> p(cs.npar > 0 ? cs.npar : 0, 0);
    if (cs.blocks.empty() || p.empty()) return p;
    std::vector<char> other(p.size(), 0);          // read as a range / correlation parameter somewhere
    std::vector<int> deg;
    for (size_t b = 0; b < cs.blocks.size(); ++b) {
        deg.assign(p.size(), 0);
        for (int r = cs.blocks[b].r0; r < cs.blocks[b].r1; ++r) {
            const int fn = cs.c(r, 2), pi = cs.c(r, 4), np = CovSpec::fn_npar(fn), e = CovSpec::fn_scale_exp(fn);
            for (int q = 0; q < np; ++q) {
                if (pi + q < 0 || pi + q >= (int)p.size()) return std::vector<int>(p.size(), 0);
                if (q == 0 && e > 0) deg[pi] += e; else other[pi + q] = 1;
            }
        }
        for (size_t i = 0; i < p.size(); ++i) {
            if (b == 0) p[i] = deg[i];
            else if (p[i] != deg[i]) p[i] = -1;     // degrees differ between blocks: not a scale of the whole D
        }
    }
    for (size_t i = 0; i < p.size(); ++i) if (p[i] < 0 || other[i]) p[i] = 0;
    return p;
}

inline bool theta_scale_any(const std::vector<int>& p)
{
    for (int e : p) if (e > 0) return true;
    return false;
}

// the MVN sum of m columns from the two scalars: the formula of k_finish_large
inline double theta_scale_value(int dim, int m, double logdet, double sumsq)
{
    return (double)m * (-0.5 * dim * 1.8378770664093454835606594728112 - 0.5 * logdet) - 0.5 * sumsq;
}

// what a factorised candidate leaves for the others of its group: the two scalars, its own log-scale coordinates and
// whether it had a value at all (rc: MCML_OK or MCML_ENOTPD)
struct ThetaScaleEntry { double logdet = 0, sumsq = 0; std::vector<double> zref; int rc = MCML_OK; };

// One theta-step's groups.  Key: the exact bit pattern of the non-scale coordinates, in the optimiser's own
// coordinates.  The samples are fixed during a theta-step and nowhere longer, so an object of this type lives inside
// one theta-step (clear() at its start).
struct ThetaScaleMemo {
    typedef std::vector<uint64_t> Key;
    std::vector<int> p;                   // exponents; all zero: every candidate is its own group
    bool logcoords = true;                // the candidates' coordinates are log(theta) (else theta itself)
    std::map<Key, ThetaScaleEntry> known;
    long long factorised = 0;

    void reset(const std::vector<int>& p_, bool logcoords_) { p = p_; logcoords = logcoords_; clear(); }
    void clear() { known.clear(); }

    Key key(const double* x) const
    {
        Key k;
        for (size_t i = 0; i < p.size(); ++i)
            if (p[i] == 0) { uint64_t u; memcpy(&u, x + i, sizeof u); k.push_back(u); }
        return k;
    }
    // the scale coordinates in log form (0 elsewhere)
    std::vector<double> zscale(const double* x) const
    {
        std::vector<double> z(p.size(), 0.0);
        for (size_t i = 0; i < p.size(); ++i) if (p[i] > 0) z[i] = logcoords ? x[i] : std::log(x[i]);
        return z;
    }

    // A round of k candidates X (candidate j = x[j * stride .. + p.size())) -> the candidates to factorise, in
    // candidate order: the first member of every group this theta-step has not seen yet.
    std::vector<int> plan(const double* X, int stride, int k) const
    {
        std::vector<int> reps;
        if (!theta_scale_any(p)) { for (int j = 0; j < k; ++j) reps.push_back(j); return reps; }
        std::map<Key, int> seen;
        for (int j = 0; j < k; ++j) {
            const Key kj = key(X + (size_t)j * stride);
            if (known.count(kj) || seen.count(kj)) continue;
            seen[kj] = j;
            reps.push_back(j);
        }
        return reps;
    }

    // The round's values from its representatives' (reps = plan(...): sums, parts = logdet and sum of squares, rcs).
    // A representative keeps the value it was evaluated to; every other member is rescaled from its group's entry, and
    // has no value (same status) where the representative had none.  dim: total dimension of D, m: sample columns.
    void finish(const double* X, int stride, int k, const std::vector<int>& reps, const double* rep_sums,
                const double* rep_parts, const int* rep_rcs, int dim, int m, double* sums, int* rcs)
    {
        factorised += (long long)reps.size();
        if (!theta_scale_any(p)) {
            for (size_t q = 0; q < reps.size(); ++q) { sums[reps[q]] = rep_sums[q]; rcs[reps[q]] = rep_rcs[q]; }
            return;
        }
        std::vector<int> pos(k, -1);
        for (size_t q = 0; q < reps.size(); ++q) {
            const double* x = X + (size_t)reps[q] * stride;
            pos[reps[q]] = (int)q;
            ThetaScaleEntry e;
            e.logdet = rep_parts[2 * q]; e.sumsq = rep_parts[2 * q + 1]; e.zref = zscale(x); e.rc = rep_rcs[q];
            known[key(x)] = e;
        }
        for (int j = 0; j < k; ++j) {
            if (pos[j] >= 0) { sums[j] = rep_sums[pos[j]]; rcs[j] = rep_rcs[pos[j]]; continue; }
            const double* x = X + (size_t)j * stride;
            const ThetaScaleEntry& e = known.find(key(x))->second;
            rcs[j] = e.rc; sums[j] = 0.0;
            if (e.rc != MCML_OK) continue;
            const std::vector<double> z = zscale(x);
            double lr = 0.0;
            for (size_t i = 0; i < p.size(); ++i) if (p[i] > 0) lr += p[i] * (z[i] - e.zref[i]);
            sums[j] = theta_scale_value(dim, m, e.logdet + dim * lr, e.sumsq * std::exp(-lr));
        }
    }
};

// GLMMR_MCML_THETA_SCALE=0: one factorisation per candidate (A/B, tests).  Read at every theta-step, not cached.
inline bool theta_scale_enabled()
{
    const char* e = getenv("GLMMR_MCML_THETA_SCALE");
    return !(e && !strcmp(e, "0"));
}

}  // namespace mcml
