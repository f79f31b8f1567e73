"""ModelMCML's `information=` keyword (glmmrmcml_amd/model.py) with a recording backend in place of the GPU exports: where
the GLS information matrix behind the standard errors comes from.  No GPU."""
import numpy as np
import pytest

from glmmrmcml_amd import synth
from glmmrmcml_amd.model import ModelMCML
from test_model_caller import FakeBackend, FakeCtx


class RecordingCtx(FakeCtx):
    def gen_D(self, theta, chol=False):
        self.be._rec("gen_D", (np.array(theta, float),), dict(chol=chol))
        return super().gen_D(theta, chol)


class InfoBackend(FakeBackend):
    """the recording backend of tests/test_model_caller.py with the `information_matrix` export: it returns diag(2, 3, ...)"""

    def Context(self, cov, data, eff):
        return RecordingCtx(self, cov, data, eff)

    def information_matrix(self, *a, **k):
        self._rec("information_matrix", a, k)
        return np.diag(np.arange(2.0, 2.0 + self.P))


def _model(family):
    d = synth.cluster_rct(ncl=4, nt=3, nind=3, seed=1, family=family)
    be = InfoBackend(d["P"], 2, d["Z"].shape[1])
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                  var_par=1.3, backend=be)
    return d, be, m


def _names(be):
    return [c[0] for c in be.calls]


def _check_device_call(be, m, fit, sigma):
    P = m.X.shape[1]
    calls = [c for c in be.calls if c[0] == "information_matrix"]
    assert len(calls) == 1 and "gen_D" not in _names(be)
    a, k = calls[0][1], calls[0][2]
    # (cov, data, eff_range, Z, X, family, link, beta, theta) + var_par: the FINAL estimates of the fake fit
    assert a[3] is m.Z and a[4] is m.X and a[5] == m.family and a[6] == m.link
    assert np.array_equal(a[7], np.full(P, 0.5)) and np.array_equal(a[8], np.full(2, 0.2))
    assert k["var_par"] == sigma
    assert np.allclose(fit["coefficients"]["SE"][:P], 1 / np.sqrt(np.arange(2.0, 2.0 + P)))
    assert np.all(np.isnan(fit["coefficients"]["SE"][P:P + 2]))


def test_mcml_approx_se_from_the_device_export():
    d, be, m = _model("binomial")
    fit = m.MCML(d["y"], verbose=False, se_method="approx", information="device")
    _check_device_call(be, m, fit, 1.0)                                # binomial: the start vector's trailing one
    assert m._information == "host"                                    # restored after the call


def test_la_se_from_the_device_export():
    d, be, m = _model("poisson")
    fit = m.LA(d["y"], information="device")
    _check_device_call(be, m, fit, 1.0)
    assert m._information == "host"
    be.calls.clear()
    m.LA(d["y"], use_hess=True, information="device")                   # with the Hessian no information matrix at all
    assert "information_matrix" not in _names(be) and "gen_D" not in _names(be)


def test_hessian_fallback_takes_the_chosen_route():
    d, be, m = _model("binomial")
    be.mcml_hess = lambda *a, **k: np.full((m.X.shape[1] + 2,) * 2, np.nan)      # an unusable Hessian: SE[:P] is NaN
    fit = m.MCML(d["y"], verbose=False, se_method="lik", information="device")
    _check_device_call(be, m, fit, 1.0)
    assert fit["hessian"] is False


@pytest.mark.parametrize("information", [None, "host"])
def test_default_and_host_call_gen_D_as_before(information):
    d, be, m = _model("binomial")
    fit = m.MCML(d["y"], verbose=False, information=information)
    assert "gen_D" in _names(be) and "information_matrix" not in _names(be)
    d2, be2, m2 = _model("binomial")
    want = m2.MCML(d2["y"], verbose=False)                              # no keyword at all
    assert np.array_equal(fit["coefficients"]["SE"], want["coefficients"]["SE"], equal_nan=True)
    d3, be3, m3 = _model("poisson")
    m3.LA(d3["y"], information=information)
    assert "gen_D" in _names(be3) and "information_matrix" not in _names(be3)


def test_information_matrix_on_device_and_bad_values():
    d, be, m = _model("binomial")
    M = m.information_matrix(d["theta"], d["beta"], 1.0, on="device")
    assert np.array_equal(M, np.diag(np.arange(2.0, 2.0 + m.X.shape[1]))) and "gen_D" not in _names(be)
    with pytest.raises(ValueError, match="information"):
        m.MCML(d["y"], verbose=False, information="gpu")
    with pytest.raises(ValueError, match="information"):
        m.LA(d["y"], information="gpu")
    with pytest.raises(ValueError, match="information"):
        m.information_matrix(d["theta"], d["beta"], 1.0, on="gpu")
    assert m._information == "host"


def test_gamma_reaches_the_export_in_lower_case():
    """ModelMCML spells the family "Gamma" (R6ModelExtMCML.R); the exports' table is lower-case"""
    d = synth.cluster_rct(ncl=4, nt=3, nind=3, seed=1, family="poisson")
    be = InfoBackend(d["P"], 2, d["Z"].shape[1])
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], "Gamma", "log", d["beta"], d["theta"], var_par=2.0,
                  backend=be)
    m.information_matrix(d["theta"], d["beta"], 2.0, on="device")
    assert be.calls[-1][1][5] == "gamma" and be.calls[-1][2]["var_par"] == 2.0
