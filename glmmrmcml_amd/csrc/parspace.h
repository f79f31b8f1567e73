// parspace.h -- the search spaces of the host optimisers and finite differences (host only, no HIP): which of beta, theta
// and sigma a step of McmlOptim (drivers.hip) or LaFit (laplace.hip) searches over, in that order, and their bounds
// (mcmloptim.h:35-38,76-79,98-105): beta free; theta >= 1e-6, on the batch schedules searched as log theta; sigma >= 0,
// present for some families.  Also what the two are built from: the `start` vector and the optimiser's options.
#pragma once
#include "optim.h"
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace mcml {

struct ParSpace {
    int nbeta, ntheta;          // coordinates of beta / theta in the space (0: not searched)
    bool has_sigma, log_theta;
    ParSpace(int nbeta_, int ntheta_, bool has_sigma_, bool log_theta_ = false)
        : nbeta(nbeta_), ntheta(ntheta_), has_sigma(has_sigma_), log_theta(log_theta_) {}

    static constexpr double theta_min = 1e-6;
    double theta_at(double coord) const { return log_theta ? std::exp(coord) : coord; }     // theta of its coordinate

    struct Point { std::vector<double> x, lower, upper; };
    Point pack(const std::vector<double>& beta, const std::vector<double>& theta, double sigma) const
    {
        Point p;
        p.x.assign(beta.begin(), beta.begin() + nbeta);
        p.lower.assign(nbeta, -HUGE_VAL);
        for (int i = 0; i < ntheta; ++i) {
            p.x.push_back(log_theta ? std::log(std::max(theta[i], theta_min)) : theta[i]);
            p.lower.push_back(log_theta ? std::log(theta_min) : theta_min);
        }
        if (has_sigma) { p.x.push_back(sigma); p.lower.push_back(0.0); }
        p.upper.assign(p.x.size(), HUGE_VAL);
        return p;
    }
    // the parts the space holds; the others are left as they are
    void unpack(const std::vector<double>& x, std::vector<double>* beta, std::vector<double>* theta, double* sigma) const
    {
        if (nbeta) beta->assign(x.begin(), x.begin() + nbeta);
        for (int i = 0; i < ntheta; ++i) (*theta)[i] = theta_at(x[nbeta + i]);
        if (has_sigma) *sigma = x[nbeta + ntheta];
    }
    // bobyqa (an objective_fn) or bobyqa_batch at `width` (a batch_objective_fn) from (beta, theta, sigma), which take the result
    template <class Objective>
    int minimise(const Objective& f, const BobyqaOpts& o, int width, std::vector<double>* beta, std::vector<double>* theta, double* sigma) const
    {
        const Point p = pack(*beta, *theta, *sigma);
        BobyqaResult r;
        int rc;
        if constexpr (std::is_same<Objective, batch_objective_fn>::value) rc = bobyqa_batch(f, p.x, p.lower, p.upper, o, width, &r);
        else rc = bobyqa(f, p.x, p.lower, p.upper, o, &r);
        if (!rc) unpack(r.x, beta, theta, sigma);
        return rc;
    }
};

// start = c(beta, theta[, sigma]): sigma is read for the gaussian family only (mcmloptim.h:30)
inline void parse_start(const double* start, int P, int R, bool gaussian, std::vector<double>* beta, std::vector<double>* theta, double* sigma)
{
    beta->assign(start, start + P);
    theta->assign(start + P, start + P + R);
    *sigma = gaussian ? start[P + R] : 0;
}

inline BobyqaOpts bopts(int trace, int maxfun) { BobyqaOpts o; o.iprint = trace; if (maxfun > 0) o.maxfun = maxfun; return o; }

}  // namespace mcml
