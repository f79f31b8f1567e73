"""Candidates of a theta-step round that differ in a pure scale parameter share one factorisation (csrc/theta_scale.h,
mvn.hip mvn_loglik_batch_parts over chol.hip potrf_blocked): the grouped round against single evaluations of every candidate, against the ungrouped
round (GLMMR_MCML_THETA_SCALE=0), the number of matrices factorised, "no value" propagation, models without a scale,
and whole mcml_full / mcml_hess calls with the switch on and off.

Tolerance 1e-12 relative between a rescaled value and the single evaluation of that theta: what the project accepts
between the regrouped sums of a batch and a single evaluation; the identity itself holds to ~1e-14."""
import ctypes as C

import numpy as np
import pytest

from glmmrmcml_amd import synth

pytestmark = pytest.mark.gpu

FEXP, FEXP0, AR1 = synth.FN_FEXP, synth.FN_FEXP0, synth.FN_AR1


def _round(ctx, thetas):
    from glmmrmcml_amd import _lib
    th = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))     # row j = candidate j
    out = np.zeros(th.shape[0])
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.lib().glmmr_mcml_dbg_theta_round(ctx._h, th.ctypes.data_as(dp), th.shape[0], out.ctypes.data_as(dp)))
    return out


def _fact(ctx):
    return ctx.shard_stats()["theta_factorised"]


# 8 candidates, 5 of which share their range in two groups: {0, 1, 3} and {2, 4}; 5, 6, 7 are groups of one
CANDS = np.array([[0.25, 0.10], [0.30, 0.10], [0.25, 0.12], [0.20, 0.10], [0.28, 0.12], [0.25, 0.09], [0.31, 0.11],
                  [0.22, 0.13]])


@pytest.mark.parametrize("n", [200, 1300])
def test_grouped_round_equals_single_evaluations(n, monkeypatch):
    """n = 200: two panels, single-level blocking; n = 1300: above 1152, the K = 1024 regrouping runs"""
    from glmmrmcml_amd import api
    m = 16
    d = synth.geospatial(n, seed=3)
    rng = np.random.default_rng(n)
    u = np.asfortranarray(np.linalg.cholesky(synth._fexp_D(d["data"].reshape(2, n).T, d["theta"])) @ rng.standard_normal((n, m)))
    with api.Context(d["cov"], d["data"], d["eff_range"]) as ctx:
        ctx.set_u(u)
        monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", "1")
        f0 = _fact(ctx)
        on = _round(ctx, CANDS)
        assert _fact(ctx) - f0 == 5
        monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", "0")
        f0 = _fact(ctx)
        off = _round(ctx, CANDS)
        assert _fact(ctx) - f0 == 8
        single = np.array([ctx.mvn_ll(t) for t in CANDS])
    rel = np.abs(on - single) / np.abs(single)
    print("n=%d: grouped vs single %s; grouped vs ungrouped %s" % (n, rel, np.abs(on - off) / np.abs(off)))
    assert np.all(np.isfinite(on)) and rel.max() <= 1e-12, rel
    assert np.array_equal(on[5:], off[5:]), (on[5:], off[5:])          # a group of one: the same bits as without the grouping


def test_no_value_propagates_and_blocks_add_up(monkeypatch):
    """fexp x ar1 in one block: an AR1 parameter of 1.5 is outside the positive definite region -- the representative has
    no value and neither has the member of its group; two blocks of ONE formula: the two scalars are summed over blocks"""
    from glmmrmcml_amd import api
    monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", "1")
    n, m = 160, 16
    rng = np.random.default_rng(1)
    xy = rng.random((n, 2)); t = rng.integers(0, 4, n).astype(float)
    cov = np.array([[0, n, FEXP, 2, 0], [0, n, AR1, 1, 2]], dtype=np.int32, order="F")
    data = np.concatenate([xy[:, 0], xy[:, 1], t])
    u = np.asfortranarray(0.5 * rng.standard_normal((n, m)))
    th = np.array([[0.25, 5.0, 1.5], [0.40, 5.0, 1.5], [0.25, 0.1, 0.5], [0.30, 0.1, 0.5]])
    with api.Context(cov, data, np.zeros(2)) as ctx:
        ctx.set_u(u)
        f0 = _fact(ctx)
        got = _round(ctx, th)
        assert _fact(ctx) - f0 == 2
        assert np.isnan(got[0]) and np.isnan(got[1]) and np.all(np.isfinite(got[2:]))
        want = np.array([ctx.mvn_ll(x) for x in th[2:]])
        assert np.abs(got[2:] - want).max() <= 1e-12 * np.abs(want).max()
    n1, n2 = 150, 70
    xy = rng.random((n1 + n2, 2))
    cov = np.array([[0, n1, FEXP, 2, 0], [1, n2, FEXP, 2, 0]], dtype=np.int32, order="F")
    data = np.concatenate([xy[:n1, 0], xy[:n1, 1], xy[n1:, 0], xy[n1:, 1]])
    u = np.asfortranarray(0.5 * rng.standard_normal((n1 + n2, m)))
    with api.Context(cov, data, np.zeros(2)) as ctx:
        ctx.set_u(u)
        f0 = _fact(ctx)
        got = _round(ctx, CANDS)
        assert _fact(ctx) - f0 == 5
        want = np.array([ctx.mvn_ll(x) for x in CANDS])
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), np.abs(got - want) / np.abs(want)


def test_models_without_a_scale_factorise_every_candidate(monkeypatch):
    from glmmrmcml_amd import api
    monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", "1")
    n, m = 140, 16
    rng = np.random.default_rng(2)
    xy = rng.random((n, 2))
    u = np.asfortranarray(0.5 * rng.standard_normal((n, m)))
    cov = np.array([[0, n, FEXP0, 2, 0]], dtype=np.int32, order="F")
    th0 = np.array([[0.1], [0.1], [0.12], [0.09], [0.1], [0.11], [0.13], [0.08]])          # even equal thetas: no grouping
    with api.Context(cov, np.concatenate([xy[:, 0], xy[:, 1]]), np.zeros(1)) as ctx:
        ctx.set_u(u)
        f0 = _fact(ctx)
        got = _round(ctx, th0)
        assert _fact(ctx) - f0 == 8 and np.array_equal(got, ctx.mvn_ll_batch(th0))
    n1 = 70
    cov = np.array([[0, n1, FEXP, 2, 0], [1, n - n1, FEXP, 2, 2]], dtype=np.int32, order="F")       # two formulas, own parameters
    data = np.concatenate([xy[:n1, 0], xy[:n1, 1], xy[n1:, 0], xy[n1:, 1]])
    th2 = np.hstack([CANDS, CANDS[::-1]])
    th2[:, 3] = 0.1                                                                           # candidates 0, 1, 3 differ in the two scales only
    with api.Context(cov, data, np.zeros(2)) as ctx:
        ctx.set_u(u)
        f0 = _fact(ctx)
        got = _round(ctx, th2)
        assert _fact(ctx) - f0 == 8 and np.array_equal(got, ctx.mvn_ll_batch(th2))


def test_mcml_full_and_hess_with_the_switch_on_and_off(monkeypatch):
    """two mcml_full iterations at n = 333, m = 64: the first theta-step's first round is the same candidates, its logged
    values agree to 1e-12, both fits are finite and inside the band of test_gpu_fullsize.py; mcml_hess on the same samples
    agrees to the Hessian tolerance of test_gpu_drivers.py (1e-4 of the largest entry) with fewer matrices factorised"""
    from glmmrmcml_amd import api
    n, m = 333, 64
    d = synth.geospatial(n, seed=20240601)
    kw = dict(mcnr=True, m=m, warmup=100, tol=0.0, lambda_=5.0, maxsteps=10, target_accept=0.9, seed=20240601, chains=m,
              maxfun=40)
    out = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", sw)
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.theta_log(enable=True)
            ctx.mcml_full(d["start"], maxiter=1, **kw)
            log1 = ctx.theta_log(enable=True)
            s0 = ctx.shard_stats()
            r = ctx.mcml_full(d["start"], maxiter=2, **kw)
            s1 = ctx.shard_stats()
            out[sw] = dict(log1=log1, r=r, fact=s1["theta_factorised"] - s0["theta_factorised"],
                           evals=s1["theta_evals_all"] - s0["theta_evals_all"])
            if sw == "1":                   # the Hessian on ONE set of samples at one point, switch on then off
                for hs in ("1", "0"):
                    monkeypatch.setenv("GLMMR_MCML_THETA_SCALE", hs)
                    f0 = _fact(ctx)
                    out["H" + hs] = (ctx.mcml_hess(d["start"], tol=1e-4), _fact(ctx) - f0)
    on, off = out["1"], out["0"]
    (Hon, hon), (Hoff, hoff) = out["H1"], out["H0"]
    print("factorised %d of %d evaluations (off: %d of %d); hess %d vs %d" % (on["fact"], on["evals"], off["fact"], off["evals"],
                                                                             hon, hoff))
    assert off["fact"] == off["evals"] and on["fact"] < on["evals"] <= 80
    # the first round at two parameters: the 6 points of the initial quadratic design and one opposite diagonal
    # (csrc/optim.hip bobyqa_batch), none of which depends on a value; the 8th logged candidate opens the second round
    assert on["log1"].shape == off["log1"].shape and on["log1"].shape[0] >= 8
    assert np.array_equal(on["log1"][:7, :2], off["log1"][:7, :2])
    assert np.allclose(on["log1"][:, 2], off["log1"][:, 2], rtol=1e-12, atol=0), np.abs(on["log1"][:, 2] - off["log1"][:, 2]).max()
    for o in (on, off):
        r = o["r"]
        assert np.all(np.isfinite(r["beta"])) and np.all(np.isfinite(r["theta"])) and np.isfinite(r["sigma"])
        assert 0.1 < r["theta"][0] < 0.6 and 0.03 < r["theta"][1] < 0.3 and 0.7 < r["sigma"] < 1.3 and 0.0 < r["beta"][0] < 2.0
    assert 0 < hon < hoff
    assert np.all(np.isfinite(Hon)) and np.abs(Hon - Hoff).max() < 1e-4 * np.abs(Hoff).max()
