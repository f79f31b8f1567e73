"""The step exports on dense-block models and at theta without a value (csrc/drivers.hip: f_optim_batch, the pre-pass of
f_hess, aic, the loop of mcml_full) against the oracle's results on the cases of driver_cases.py, stored in
golden/driver_golden.json and checked without a GPU by test_driver_cases_cpu.py.

Bounds.  Optima: F(got) <= F(oracle) + 1e-9 |F|, beta and theta within 1e-6 relative (test_mcml_optim's figures) unless
the case's CPU twin needed a bound of its own.  Every logged objective value: 1e-10 relative, the project's mvn_ll
tolerance.  Hessians: at step 1e-4 the existing 1e-4 of the largest entry; at step h = 1e-2
max |H - Ho| <= RTOL (|ll| + |logl|) / h^2, RTOL = 1e-10 -- an entry is four objective values over 4 h^2 and fd_hessian is
optimhess to the bit, so values that agree to RTOL move an entry by at most 4 RTOL (|ll| + |logl|) / (4 h^2).  AIC 1e-9.
The loop: beta and theta 2e-6 (test_mcml_full_iteration_by_iteration), u within twice the response of the oracle's
second iteration to a 2e-6 relative change of what the first hands it.

Measured on an MI355X (worst ratio to each bound).  mcml_simlik on the batch schedule (theta_batch 0 and 3): F gap at most
1.2e-15 (1e-6 of the bound), beta / theta at most 1.4e-7 (0.14).  Logged values against the oracle's mvn_ll: at most
1.2e-14 (1.2e-4).  mcml_optim on SW80 / SW95: theta 2.1e-7 absolute of 4.7e-6 (0.05), D gap 2.4e-13 (2.4e-4).  mcml_hess:
step 1e-4 at most 2.8e-5 of the bound, step 1e-2 at most 1.8e-5 (2.3e-8 absolute on TWO_LARGE_A); switch on and off gave
equal matrices, 5 against 19 (DG, DP) and 13 against 25 (AR) factorised.  aic_mcml: 8.7e-16 (1e-6).  mcml_full: beta /
theta 6e-9 (0.003), u 2.7e-8 of 4.4e-6 (0.006).

mcml_simlik at theta_batch 1, the sequential optimiser on 2n + 1 interpolation points: F gap at most 1.1e-15, beta / theta
at most 8.3e-8 (0.08).  On minqa's n + 2 points, which f_optim ran before, DP ended 4.31e-6 from the optimum in beta_1 (F
gap 7e-13) and DG 1.4e-6, with every logged value within 2e-15 of the oracle's: the run crept along beta_1 (curvature 26
against 4352) in steps of its final radius and stopped early, where depending on the rounding of the objective."""
import numpy as np
import pytest

import driver_cases as dc

pytestmark = pytest.mark.gpu


def _context(name):
    from glmmrmcml_amd import api
    d = dc.case(name)
    ctx = api.Context(*dc.args(d), d["family"], d["link"])
    ctx.set_u(d["u"], d["niter"])
    return ctx


def _fact(ctx):
    return ctx.shard_stats()["theta_factorised"]


def _logged_simlik(ctx, d, tb):
    """mcml_simlik with the log on -> (result, logged rows, matrices factorised)"""
    ctx.theta_log(enable=True)
    f0 = _fact(ctx)
    got = ctx.mcml_simlik(d["start"], theta_batch=tb)
    fact = _fact(ctx) - f0
    return got, ctx.theta_log(enable=False), fact


def _meets_the_optimum(name, got, tb, label=""):
    g = dc.golden()["simlik"][name]
    bound = dc.par_bound(name, tb or 8)
    label = "theta_batch %d %s" % (tb, label)
    d = dc.case(name)
    x = np.r_[got["beta"], got["theta"]]
    F = dc.F_obj(name)
    eb, et = dc.par_err(x, g["x"], d["P"])
    print("%s %s: F gap %.2e of %.0e, beta %.2e theta %.2e of %.1e" % (name, label, (F(x) - g["F"]) / abs(g["F"]), dc.F_BOUND,
                                                                       eb, et, bound))
    assert F(x) <= g["F"] + dc.F_BOUND * abs(g["F"])
    assert max(eb, et) <= bound


def _log_matches_the_oracle(orc, d, log):
    R = d["start"].size - d["P"] - 1
    assert log.shape[0] > 0
    worst = 0.0
    for row in log:
        want = orc.mvn_ll(d["cov"], d["data"], d["eff_range"], row[:R], d["u"])
        worst = max(worst, abs(row[R] - want) / abs(want))
    print("   %d logged values, worst %.2e of 1e-10" % (log.shape[0], worst))
    assert worst <= 1e-10


# ------------------------------------------------------------------------------------------------ mcml_simlik
@pytest.mark.parametrize("tb", [0, 3, 1])
@pytest.mark.parametrize("name", dc.SIMLIK)
def test_mcml_simlik(orc, name, tb):
    """theta_batch 0 (the default: 8 candidates a round), 3 and 1 (the sequential optimiser over theta)"""
    from glmmrmcml_amd import _lib
    d = dc.case(name)
    with _context(name) as ctx:
        if name == "AR":                                       # the first round steps to rho = 1.156: no value there
            with pytest.raises(_lib.McmlError) as e:
                ctx.mvn_ll(dc.ar_first_round_point())
            assert e.value.code == -3
        got, log, _ = _logged_simlik(ctx, d, tb)
    _meets_the_optimum(name, got, tb)
    if tb != 1:                                                # the batch schedule leaves sigma where it started
        assert got["sigma"] == dc.fix_sigma(d)
    _log_matches_the_oracle(orc, d, log)


def test_mcml_simlik_scale_memo(orc, monkeypatch):
    """DG's candidates repeat a range under several scales: with the switch on fewer matrices are factorised than values
    logged, with it off as many (one more row: the denominator's single evaluation at the start, which is no candidate)"""
    d = dc.case("DG")
    for sw in ("1", "0"):
        monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", sw)
        with _context("DG") as ctx:
            got, log, fact = _logged_simlik(ctx, d, 0)
        print("switch %s: %d rows, %d factorised" % (sw, log.shape[0], fact))
        _meets_the_optimum("DG", got, 0, "scale switch " + sw)
        assert np.array_equal(log[0, :2], d["start"][2:4])
        if sw == "1":
            assert 0 < fact < log.shape[0] - 1
        else:
            assert fact == log.shape[0] - 1
            _log_matches_the_oracle(orc, d, log)


# ------------------------------------------------------------------------------------------------ mcml_optim, sequential
@pytest.mark.parametrize("name", dc.OPTIM)
def test_mcml_optim_where_the_sequential_step_meets_rho_above_one(orc, name):
    """test_mcml_optim's assertions on the two stepped-wedge cases whose theta-step evaluates a rho > 1"""
    from glmmrmcml_amd import api
    d = dc.case(name); mod = dc.model(name)
    want = dc.golden()["optim"][name]
    got = api.mcml_optim(*dc.args(d), d["u"], d["family"], d["link"], d["start"], trace=0, mcnr=True)
    wb, wt = np.array(want["beta"]), np.array(want["theta"])
    f = mod.D_obj(d["u"])
    print("%s: beta %.2e, theta %.2e, D gap %.2e" % (name, np.abs(got["beta"] - wb).max(), np.abs(got["theta"] - wt).max(),
                                                     (f(got["theta"]) - want["D"]) / abs(want["D"])))
    assert np.abs(got["beta"] - wb).max() < 1e-6 * max(1.0, np.abs(wb).max())
    assert np.abs(got["theta"] - wt).max() < 1e-6 * max(1e-2, np.abs(wt).max()) * 5
    assert f(got["theta"]) <= want["D"] + 1e-9 * abs(want["D"])


# ------------------------------------------------------------------------------------------------ mcml_hess
@pytest.mark.parametrize("name", dc.HESS)
def test_mcml_hess(orc, name, monkeypatch):
    d = dc.case(name); mod = dc.model(name)
    g = dc.golden()["hess"][name]
    x = np.array(g["x"]); P = d["P"]
    start = np.r_[x, d["start"][-1]]
    ll = orc.model_loglik(mod.Z, mod.X @ x[:P], mod.y, d["u"], dc.fix_sigma(d), mod.fl)
    logl = orc.mvn_ll(d["cov"], d["data"], d["eff_range"], x[P:], d["u"])
    assert abs(-(ll + logl) - g["F"]) <= 1e-12 * abs(g["F"])
    grouped = name in ("DG", "DP", "AR")                       # one dense block with a scale: the pre-pass groups
    with _context(name) as ctx:
        for h in dc.HESS_STEPS:
            Ho = np.array(g["H"]["%g" % h])
            bound = 1e-4 * np.abs(Ho).max() if h == 1e-4 else dc.HESS_RTOL * (abs(ll) + abs(logl)) / (h * h)
            res = {}
            for sw in ("1", "0"):
                monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", sw)
                ctx.theta_log(enable=True)
                f0 = _fact(ctx)
                H = ctx.mcml_hess(start, tol=h)
                res[sw] = (H, _fact(ctx) - f0, ctx.theta_log(enable=False))
                err = np.abs(H - Ho).max()
                print("%s h %g switch %s: |H - Ho| %.3e of %.3e (ratio %.3f), max|Ho| %.4g, %d factorised, %d logged"
                      % (name, h, sw, err, bound, err / bound, np.abs(Ho).max(), res[sw][1], res[sw][2].shape[0]))
                assert err <= bound
                assert np.array_equal(H, H.T)
            (Hon, fon, logon), (Hoff, foff, logoff) = res["1"], res["0"]
            assert np.abs(Hon - Hoff).max() <= bound
            assert logon.shape == logoff.shape and foff == logoff.shape[0]
            assert (0 < fon < foff) if grouped else fon == foff
        if name == "MIXED":                                    # not dense only: the round falls back to single evaluations
            R = x.size - P
            for row in logoff:
                assert ctx.mvn_ll(row[:R]) == row[R]


# ------------------------------------------------------------------------------------------------ aic_mcml
@pytest.mark.parametrize("name", dc.AIC)
def test_aic_mcml(name):
    g = dc.golden()["aic"][name]
    with _context(name) as ctx:
        a = ctx.aic_mcml(g["beta_par"], g["cov_par"])
    print("%s: aic %.12g, relative difference %.2e of 1e-9" % (name, a, abs(a - g["aic"]) / abs(g["aic"])))
    assert abs(a - g["aic"]) < 1e-9 * abs(g["aic"])


# ------------------------------------------------------------------------------------------------ mcml_full
@pytest.mark.parametrize("key", list(dc.LOOP_CASES))
def test_mcml_full_two_iterations(orc, key):
    from glmmrmcml_amd import api
    name, chains, seed = dc.LOOP_CASES[key]
    d = dc.case(name)
    g = dc.golden()["loop"][key]
    got = api.mcml_full(*dc.args(d), d["family"], d["link"], np.r_[d["beta"], d["theta"], 1.0], mcnr=True, maxiter=2,
                        tol=1e-12, verbose=False, seed=seed, chains=chains, **dc.LOOP)
    a1, a2 = g["after"]
    beta, theta = np.array(a2["beta"]), np.array(a2["theta"])
    u, _ = dc.loop_sample(name, np.array(a1["beta"]), np.array(a1["theta"]), a1["sigma"], 2, chains, seed)
    eb = np.abs(got["beta"] - beta).max() / max(1.0, np.abs(beta).max())
    et, eu = np.abs(got["theta"] - theta).max(), np.abs(got["u"] - u).max()
    print("%s: beta %.2e theta %.2e of 2e-6, u %.2e of %.2e" % (key, eb, et, eu, 2 * g["u_response"]))
    assert not got["converged"]
    assert eb < 2e-6 and et < 2e-6
    if d["family"] == "gaussian":
        assert abs(got["sigma"] - a2["sigma"]) < 2e-6 * a2["sigma"]
    assert got["u"].shape == u.shape and eu <= 2 * g["u_response"]
