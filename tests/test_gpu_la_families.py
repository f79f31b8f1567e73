"""The Laplace path (csrc/laplace.hip) for every family / link case of the reference's switch, on the device against
the oracle restatement (oracle/la.py): the three functors LA_likelihood / LA_likelihood_cov / LA_likelihood_btheta
(la_probe kinds 0, 1, 2) and one mcnr_b Newton step (kind 3).

k_la_ll, k_la_W and k_la_nr_obs take the family at run time; tests/test_gpu_la.py runs three of the twelve.  Here all
twelve run with var_par != 1 wherever the family reads it (the `vp` column of family_designs.CASES): the beta family's
weight 1 + var_par and its own score (glm_score_beta), the gaussian var_par^2, gamma's factor after the score
(glm_score_post), and the parameter vectors follow oracle/la.py -- kind 1 takes (theta, var_par) for flink 7, 8 and 12,
kind 2 appends var_par for 7 and 8 only.  Two shapes (family_designs.LA_CASES): n = 144, Q = 24 of tests/test_gpu_la.py,
and n = 420, Q = 280 -- a second 256-row block in every row-indexed kernel, Q > 256 and no multiple of 4 * 64 for
k_la_scale_cols, k_la_gemv_t and k_la_logdet.

Tolerances are those of tests/test_gpu_la.py: functor values 1e-9 relative; the step rtol 1e-8 / atol 1e-10, sigma
1e-10.  v is drawn as there (0.3 N(0, 1) for the functors, 0.2 N(0, 1) for the step) except for binomial / log (0.2) and
binomial / identity (0.03), whose bounded domain xb + Z v would leave otherwise (family_designs.LA_V_SCALE;
tests/test_family_designs_cpu.py checks domain, finiteness and the conditioning of both solves of the step on the oracle:
cond(M) < 1e3, cond(X'WX) < 1e4 for every case, so no case needed a smaller v for conditioning's sake)."""
import numpy as np
import pytest

import family_designs as fd
from glmmrmcml_amd import _lib, api

pytestmark = pytest.mark.gpu


def _ctx(d):
    return api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])


def _functors(ctx, d, kinds=(0, 1, 2)):
    v, _, beta, theta, vp = fd.la_points(d)
    par = {0: np.r_[beta, v], 1: fd.la_cov_par(d, theta, vp), 2: fd.la_btheta_par(d, beta, theta, vp)}
    name = {0: "bv", 1: "cov", 2: "btheta"}
    return {name[k]: ctx.la_probe(d["start"], k, v=None if k == 0 else v, var_par=vp, par=par[k]) for k in kinds}


def _step(ctx, d):
    _, vs, _, _, vp = fd.la_points(d)
    return ctx.la_probe(d["start"], 3, v=vs, var_par=vp)


def _check_step(got, want, tag):
    print(tag, "v %.3g beta %.3g sigma %.3g" % (np.abs(got["v"] - want["v"]).max(), np.abs(got["beta"] - want["beta"]).max(),
                                                abs(got["sigma"] / want["sigma"] - 1)))
    assert np.allclose(got["v"], want["v"], rtol=1e-8, atol=1e-10), tag
    assert np.allclose(got["beta"], want["beta"], rtol=1e-8, atol=1e-10), tag
    assert got["sigma"] == pytest.approx(want["sigma"], rel=1e-10), tag


@pytest.mark.parametrize("key,family,link", fd.LA_POINTS, ids=fd.LA_IDS)
def test_functors_and_newton_step_match_oracle(key, family, link):
    d = fd.la_design(key, family, link)
    want = fd.la_reference(key, family, link)
    with _ctx(d) as ctx:
        got = _functors(ctx, d)
        p = ctx.la_plan()
        assert p["requested"] == "dense" and p["operator"] == "dense" and p["launches"] == 0, p
        st = _step(ctx, d)
    for k in ("bv", "cov", "btheta"):
        print(key, family, link, k, "%.3g" % abs(got[k] / want[k] - 1))
    for k in ("bv", "cov", "btheta"):
        assert got[k] == pytest.approx(want[k], rel=1e-9), k
    _check_step(st, want["step"], "%s %s-%s" % (key, family, link))


@pytest.mark.parametrize("family,link,vp", fd.CASES, ids=fd.IDS)
def test_component_operator_runs_every_family(family, link, vp, monkeypatch):
    """the component operator (csrc/component.hip) shares k_la_ll / k_la_W / k_la_nr_obs with the dense one: the same twelve
    families at the block-structured shape, one functor (kind 2: W, the log density and the log-determinant) and the
    step, where la_plan() reports that it ran"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = fd.la_design(fd.LA_COMPONENT_KEY, family, link)
    want = fd.la_reference(fd.LA_COMPONENT_KEY, family, link)
    with _ctx(d) as ctx:
        ctx.set_la_operator("component")
        got = _functors(ctx, d, kinds=(2,))
        p = ctx.la_plan()
        assert p["requested"] == "component" and p["operator"] == "component", p
        assert (p["ncomp"], p["max_vars"], p["max_rows"]) == fd.LA_COMPONENT_COUNTS and p["launches"] == 1, p
        st = _step(ctx, d)
        assert ctx.la_plan()["operator"] == "component"
    assert got["btheta"] == pytest.approx(want["btheta"], rel=1e-9)
    _check_step(st, want["step"], "component %s-%s" % (family, link))


def test_hess_la_still_refuses_the_beta_family():
    """mcml_la(usehess = True) on beta / logit: the fit runs, hess_la returns MCML_EUNSUPPORTED (-2) -- the reference's
    functor mis-sizes theta there -- and the context stays usable"""
    d = fd.la_design("small_144x24", "beta", "logit")
    with _ctx(d) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            ctx.mcml_la(d["start"], usehess=True, nr=True, maxiter=1, maxfun=40)
        assert e.value.code == -2 and "hess_la" in str(e.value), e.value
        r = ctx.mcml_la(d["start"], usehess=False, nr=True, maxiter=1, maxfun=40)     # the context stays usable
        assert np.isfinite(r["beta"]).all() and np.isfinite(r["theta"]).all()
