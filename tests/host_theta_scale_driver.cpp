// Host logic of the theta-step's scale grouping (glmmrmcml_amd/csrc/theta_scale.h) under AddressSanitizer + UBSan:
// the scale exponents proved from a covariance specification, the grouping of a round by the bit pattern of the
// non-scale coordinates, representative order, the rescaled values, "no value" propagation and the memo's life.
// Built and run by tests/test_theta_scale_cpu.py.
#include "theta_scale.h"
#include <cstdio>
using namespace mcml;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

// rows of (block id, block dim, function id, n variables, parameter index), every block's data zero
static std::vector<int> exps_of(const std::vector<std::vector<int>>& rows, const char* what)
{
    const int nr = (int)rows.size();
    std::vector<int32_t> cov((size_t)nr * 5);
    size_t nd = 0;
    for (int r = 0; r < nr; ++r) { for (int q = 0; q < 5; ++q) cov[r + (size_t)q * nr] = rows[r][q]; nd += (size_t)rows[r][1] * rows[r][3]; }
    std::vector<double> data(nd + 1, 0.0), eff(1, 0.0);
    CovSpec cs;
    const int rc = cs.parse(cov.data(), nr, data.data(), (int)data.size(), eff.data(), 0);
    CHECK(rc == MCML_OK, "%s: parse failed: %s", what, last_error());
    return theta_scale_exponents(cs);
}
static void expect(const std::vector<std::vector<int>>& rows, const std::vector<int>& want, const char* what)
{
    const std::vector<int> got = exps_of(rows, what);
    CHECK(got == want, "%s: exponents differ (got %zu values, first %d)", what, got.size(), got.empty() ? -1 : got[0]);
}

// a stand-in for the factorisation with the exact structure D = t0 R(t1), over (log t0, log t1)
static const int DIM = 37, M = 5;
static double ld_of(double z0, double z1) { return DIM * z0 + 3.0 * std::sin(z1) - 40.0; }
static double ss_of(double z0, double z1) { return std::exp(-z0) * (100.0 + 7.0 * std::cos(3 * z1)); }
static bool pd_of(double z1) { return z1 < 0.9; }

static void eval_reps(const std::vector<double>& X, const std::vector<int>& reps, bool logc, std::vector<double>& sums,
                      std::vector<double>& parts, std::vector<int>& rcs)
{
    sums.assign(reps.size(), 0.0); parts.assign(2 * reps.size() + 2, 0.0); rcs.assign(reps.size(), 0);
    for (size_t q = 0; q < reps.size(); ++q) {
        const double a = X[2 * reps[q]], b = X[2 * reps[q] + 1];
        const double z0 = logc ? a : std::log(a), z1 = logc ? b : std::log(b);
        parts[2 * q] = ld_of(z0, z1); parts[2 * q + 1] = ss_of(z0, z1);
        rcs[q] = pd_of(z1) ? MCML_OK : MCML_ENOTPD;
        sums[q] = theta_scale_value(DIM, M, parts[2 * q], parts[2 * q + 1]);
    }
}

static void grouping(bool logc)
{
    const double r1 = -2.25, r2 = -2.0, r3 = 1.5;                 // r3: not positive definite
    const double r1u = std::nextafter(r1, 0.0);                   // one ulp away from r1
    std::vector<double> Z = {-1.0, r1,  -0.75, r1,  -1.0, r2,  -1.25, r1,  -1.0, r1u,  -0.5, r2,  -1.0, r3,  -0.8, r3};
    std::vector<double> X = Z;
    if (!logc) for (double& v : X) v = std::exp(v);
    if (!logc) {                                                   // exp may merge r1 and r1u: restore a one-ulp gap
        X[9] = std::nextafter(X[1], 1.0);
        for (int j : {1, 3}) X[2 * j + 1] = X[1];
        X[11] = X[5]; X[15] = X[13];
    }
    const int k = 8;
    ThetaScaleMemo ts;
    ts.reset({1, 0}, logc);
    std::vector<int> reps = ts.plan(X.data(), 2, k);
    CHECK((reps == std::vector<int>{0, 2, 4, 6}), "plan: representatives are not 0 2 4 6 (%zu of them)", reps.size());
    std::vector<double> rs, parts, sums(k, -1.0); std::vector<int> rr, rcs(k, -7);
    eval_reps(X, reps, logc, rs, parts, rr);
    ts.finish(X.data(), 2, k, reps, rs.data(), parts.data(), rr.data(), DIM, M, sums.data(), rcs.data());
    CHECK(ts.factorised == 4, "factorised %lld, not 4", ts.factorised);
    for (int j = 0; j < k; ++j) {
        const double z0 = logc ? X[2 * j] : std::log(X[2 * j]), z1 = logc ? X[2 * j + 1] : std::log(X[2 * j + 1]);
        if (!pd_of(z1)) { CHECK(rcs[j] == MCML_ENOTPD, "candidate %d: status %d, not 'no value'", j, rcs[j]); continue; }
        const double want = theta_scale_value(DIM, M, ld_of(z0, z1), ss_of(z0, z1));
        CHECK(rcs[j] == MCML_OK && std::fabs(sums[j] - want) <= 1e-13 * std::fabs(want), "candidate %d: %.17g vs %.17g", j, sums[j], want);
    }
    for (size_t q = 0; q < reps.size(); ++q)
        CHECK(memcmp(&sums[reps[q]], &rs[q], sizeof(double)) == 0, "representative %d did not keep its own value", reps[q]);
    // a later round of the same theta-step: known groups are not factorised again, a new one is
    std::vector<double> X2 = {logc ? -3.0 : std::exp(-3.0), X[1], logc ? 0.1 : std::exp(0.1), X[13], X[0], logc ? -1.75 : std::exp(-1.75)};
    std::vector<int> reps2 = ts.plan(X2.data(), 2, 3);
    CHECK((reps2 == std::vector<int>{2}), "second round: representatives are not {2}");
    std::vector<double> s2(3, 0.0); std::vector<int> c2(3, 0);
    eval_reps(X2, reps2, logc, rs, parts, rr);
    ts.finish(X2.data(), 2, 3, reps2, rs.data(), parts.data(), rr.data(), DIM, M, s2.data(), c2.data());
    {
        const double z0 = logc ? X2[0] : std::log(X2[0]), z1 = logc ? X2[1] : std::log(X2[1]);
        const double want = theta_scale_value(DIM, M, ld_of(z0, z1), ss_of(z0, z1));
        CHECK(c2[0] == MCML_OK && std::fabs(s2[0] - want) <= 1e-13 * std::fabs(want), "memo value %.17g vs %.17g", s2[0], want);
        CHECK(c2[1] == MCML_ENOTPD, "memo: 'no value' was not kept across rounds");
        CHECK(ts.factorised == 5, "factorised %lld, not 5", ts.factorised);
    }
    // the next theta-step: nothing is known
    ts.clear();
    CHECK(ts.plan(X.data(), 2, k) == (std::vector<int>{0, 2, 4, 6}), "clear(): the memo survived a theta-step");
    CHECK(ts.plan(X2.data(), 2, 3) == (std::vector<int>{0, 1, 2}), "clear(): the memo survived a theta-step (second round)");
    // no scale: every candidate is its own group, nothing is remembered
    ThetaScaleMemo none;
    none.reset({0, 0}, logc);
    CHECK(none.plan(X.data(), 2, k).size() == (size_t)k, "no scale: candidates were grouped");
}

int main()
{
    const int d = 6;
    expect({{0, d, 7, 2, 0}}, {1, 0}, "fexp");
    expect({{0, d, 4, 2, 0}}, {1, 0}, "sqexp");
    expect({{0, d, 1, 1, 0}}, {2}, "gr");
    expect({{0, d, 2, 2, 0}}, {0}, "fexp0");
    expect({{0, d, 3, 1, 0}}, {0}, "ar1");
    expect({{0, d, 14, 2, 0}}, {0}, "sqexp0");
    expect({{0, d, 1, 1, 0}, {0, d, 3, 1, 1}}, {2, 0}, "gr*ar1");
    expect({{0, d, 7, 2, 0}, {1, d, 7, 2, 2}}, {0, 0, 0, 0}, "two formulas, separate parameters");
    expect({{0, d, 7, 2, 0}, {1, d + 1, 7, 2, 0}}, {1, 0}, "two blocks of one formula");
    expect({{0, d, 7, 2, 0}, {0, d, 1, 1, 2}}, {1, 0, 2}, "fexp*gr");
    expect({{0, d, 7, 2, 0}, {0, d, 2, 2, 0}}, {0, 0}, "fexp*fexp0 sharing a parameter");
    expect({{0, d, 7, 2, 0}, {1, d, 1, 1, 0}}, {0, 0}, "a scale of one block only (different degrees)");
    grouping(true);
    grouping(false);
    printf("fails=%d\n", fails);
    return fails ? 1 : 0;
}
