"""ModelMCML.theta_information and the `theta_se=` keyword of MCML() / LA() (glmmrmcml_amd/model.py) with a recording backend
in place of the GPU exports: the host formula against the long-double definition, where the device export is called and with
what, argument validation, and that the defaults are unchanged.  No GPU."""
import numpy as np
import pytest

import theta_information_reference as tr
from glmmrmcml_amd import synth
from glmmrmcml_amd.model import ModelMCML
from test_model_caller import FakeBackend

INFO = np.array([[4.0, 1.0], [1.0, 9.0]])


class ThetaBackend(FakeBackend):
    """the recording backend of tests/test_model_caller.py with the `theta_information` export"""
    info = INFO

    def theta_information(self, *a, **k):
        self._rec("theta_information", a, k)
        n = self.info.shape[0]
        return dict(information=self.info.copy(), names=["theta%d" % r for r in range(n)])


def _model(family, info=INFO):
    d = synth.cluster_rct(ncl=4, nt=3, nind=3, seed=1, family=family)
    be = ThetaBackend(d["P"], 2, d["Z"].shape[1])
    be.info = info
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                  var_par=1.3, backend=be)
    return d, be, m


def _names(be):
    return [c[0] for c in be.calls]


@pytest.mark.parametrize("key", ["family-poisson-log", "family-gaussian-identity", "family-gamma-log", "stepped_wedge_7x8x3",
                                 "weak", "geo150", "mixed"])
def test_host_path_against_the_long_double_definition(key):
    """on="host": numpy on the n x n matrices with model.py's own d D, held to the device's bound.  The reference takes the
    float64 D the model itself builds, so the two share D and nothing else"""
    c = tr.case(key)
    m = ModelMCML(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], "Gamma" if c["family"] == "gamma" else c["family"],
                  c["link"], c["beta"], c["theta"], var_par=c["var_par"], backend=FakeBackend(c["X"].shape[1], 2, 1))
    got = m.theta_information(c["theta"], c["beta"], c["var_par"], on="host")
    D = m._dD_host(c["theta"])[0]
    r = tr.ratio(got["information"], tr.reference(c, D))
    print("%s host path: ratio %.3f of C_TI %.1f" % (key, r, tr.C_TI))
    assert r <= tr.C_TI
    assert len(got["names"]) == tr.rows(c) and (got["names"][-1] == "sigma") == tr.sigma_row(c)
    assert np.array_equal(got["information"], got["information"].T)


@pytest.mark.parametrize("fit", ["MCML", "LA"])
def test_theta_se_from_the_device_export(fit):
    d, be, m = _model("poisson")
    P = m.X.shape[1]
    f = m.MCML(d["y"], verbose=False, theta_se="device") if fit == "MCML" else m.LA(d["y"], theta_se="device")
    calls = [c for c in be.calls if c[0] == "theta_information"]
    assert len(calls) == 1
    a, k = calls[0][1], calls[0][2]
    # (cov, data, eff_range, Z, X, family, link, beta, theta) + var_par: the FINAL estimates of the fake fit
    assert a[3] is m.Z and a[4] is m.X and a[5] == "poisson" and a[6] == "log"
    assert np.array_equal(a[7], np.full(P, 0.5)) and np.array_equal(a[8], np.full(2, 0.2)) and k["var_par"] == 1.0
    assert np.allclose(f["coefficients"]["SE"][P:P + 2], np.sqrt(np.diag(np.linalg.inv(INFO))), rtol=1e-15)
    assert np.array_equal(f["theta_information"]["information"], INFO)
    assert f["theta_information"]["names"] == m._cov_par_names()
    # the beta column and everything else are what the fit without the keyword gives
    d0, be0, m0 = _model("poisson")
    f0 = m0.MCML(d0["y"], verbose=False) if fit == "MCML" else m0.LA(d0["y"])
    assert "theta_information" not in _names(be0) and "theta_information" not in f0
    assert np.all(np.isnan(f0["coefficients"]["SE"][P:P + 2]))          # the default: NaN, as before
    keep = np.r_[0:P, P + 2:f0["coefficients"]["SE"].size]
    assert np.array_equal(f["coefficients"]["SE"][keep], f0["coefficients"]["SE"][keep], equal_nan=True)
    assert np.array_equal(f["coefficients"]["est"], f0["coefficients"]["est"])
    co = f["coefficients"]
    assert np.allclose(co["upper"] - co["lower"], 2 * 1.959963984540054 * co["SE"], equal_nan=True)


def test_gaussian_identity_fills_sigma_too():
    d = synth.geospatial(12, seed=2)
    be = ThetaBackend(1, 2, 12)
    be.info = np.diag([4.0, 9.0, 16.0])
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], "gaussian", "identity", d["beta"], d["theta"],
                  var_par=1.3, backend=be)
    f = m.LA(d["y"], theta_se="device")
    assert f["coefficients"]["par"][1:4] == m._cov_par_names() + ["sigma"]
    assert np.allclose(f["coefficients"]["SE"][1:4], [0.5, 1 / 3, 0.25], rtol=1e-15)
    assert f["theta_information"]["names"][-1] == "sigma"


def test_gamma_reaches_the_export_in_lower_case_and_sigma_stays_nan():
    d = synth.cluster_rct(ncl=4, nt=3, nind=3, seed=1, family="poisson")
    be = ThetaBackend(d["P"], 2, d["Z"].shape[1])
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], "Gamma", "log", d["beta"], d["theta"], var_par=2.0,
                  backend=be)
    r = m.theta_information(d["theta"], d["beta"], 2.0, on="device")
    assert be.calls[-1][1][5] == "gamma" and be.calls[-1][2]["var_par"] == 2.0 and "sigma" not in r["names"]
    P = d["P"]
    f = m.LA(np.abs(d["y"]) + 0.5, theta_se="device")
    assert np.all(np.isfinite(f["coefficients"]["SE"][P:P + 2])) and np.isnan(f["coefficients"]["SE"][P + 2])


def test_a_singular_information_gives_nan_and_a_warning():
    d, be, m = _model("poisson", info=np.array([[1.0, 1.0], [1.0, 1.0]]))
    P = m.X.shape[1]
    f = m.LA(d["y"], theta_se="device")
    assert np.all(np.isnan(f["coefficients"]["SE"][P:P + 2]))
    assert any("not invertible" in w for w in f["warnings"])
    d, be, m = _model("poisson", info=np.array([[1.0, 2.0], [2.0, 1.0]]))        # invertible, a negative variance
    f = m.LA(d["y"], theta_se="device")
    assert np.all(np.isnan(f["coefficients"]["SE"][P:P + 2])) and any("not invertible" in w for w in f["warnings"])


def test_argument_validation():
    d, be, m = _model("binomial")
    with pytest.raises(ValueError, match="theta_se"):
        m.MCML(d["y"], verbose=False, theta_se="gpu")
    with pytest.raises(ValueError, match="theta_se"):
        m.LA(d["y"], theta_se="gpu")
    with pytest.raises(ValueError, match="theta_information"):
        m.theta_information(d["theta"], d["beta"], 1.0, on="gpu")
    assert "theta_information" not in _names(be)
