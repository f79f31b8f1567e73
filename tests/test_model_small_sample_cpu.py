"""ModelMCML.small_sample and the `small_sample=` keyword of MCML() / LA() (glmmrmcml_amd/model.py) with a recording backend in
place of the GPU exports: the host path against the long-double definition and the host algebra of
tests/small_sample_reference.py, where the device export is called and with what, the fit's record and its print, argument
validation, and that the defaults are unchanged.  No GPU."""
import warnings

import numpy as np
import pytest
from scipy import stats

import information_reference as ir
import small_sample_reference as sr
import theta_information_reference as tr
from glmmrmcml_amd import synth
from glmmrmcml_amd.model import ModelMCML
from test_model_caller import FakeBackend


def _blocks(P, no, seed=5):
    """a well-conditioned fake result of the device export: I_beta, I_theta, P_r, Q_rs, R_rs"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((P, P))
    info = a @ a.T + P * np.eye(P)
    b = rng.standard_normal((no, no))
    tinfo = b @ b.T + no * np.eye(no)
    Pm = 0.1 * rng.standard_normal((no, P, P))
    Pm = Pm + Pm.transpose(0, 2, 1)
    Qm = 0.01 * rng.standard_normal((no, no, P, P))
    Qm = Qm + Qm.transpose(1, 0, 3, 2)
    Rm = 0.01 * rng.standard_normal((no, no, P, P))
    Rm = Rm + Rm.transpose(1, 0, 3, 2)
    return dict(information=info, theta_information=tinfo, P=Pm, Q=Qm, R=Rm, names=["theta%d" % r for r in range(no)])


class SmallSampleBackend(FakeBackend):
    """the recording backend of tests/test_model_caller.py with the `small_sample` export"""
    blocks = None

    def small_sample(self, *a, **k):
        self._rec("small_sample", a, k)
        return {key: (v.copy() if isinstance(v, np.ndarray) else list(v)) for key, v in self.blocks.items()}


def _model(family, blocks=None):
    d = synth.cluster_rct(ncl=4, nt=3, nind=3, seed=1, family=family)
    be = SmallSampleBackend(d["P"], 2, d["Z"].shape[1])
    be.blocks = _blocks(d["P"], 2) if blocks is None else blocks
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                  var_par=1.3, backend=be)
    return d, be, m


def _names(be):
    return [c[0] for c in be.calls]


@pytest.mark.parametrize("key", ["family-poisson-log", "family-gaussian-identity", "stepped_wedge_7x8x3", "geo150", "mixed"])
def test_host_path_against_the_long_double_definition_and_the_host_algebra(key):
    """on="host": numpy on the n x n matrices with model.py's own d D and d2 D.  Its blocks (_small_sample_blocks) are held to
    HOST_RATIO of the long-double reference; vcov, se and dof equal kr(...) of the reference module on the same blocks to
    rounding"""
    c = sr.case(key)
    m = ModelMCML(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], "Gamma" if c["family"] == "gamma" else c["family"],
                  c["link"], c["beta"], c["theta"], var_par=c["var_par"], backend=FakeBackend(c["X"].shape[1], 2, 1))
    D, dD, d2D = m._dD_host(c["theta"], second=True)
    # model.py's derivatives against the reference module's, which come from the log-derivative tables
    want2 = sr.d2D(c, D, np.float64)
    size2 = sr.d2D(c, D, np.float64, absolute=True)
    assert set(d2D) == set(want2)
    for k in want2:
        assert np.max(np.abs(d2D[k] - want2[k])) <= 1e-12 * np.max(size2[k]), (key, k)
    for a, b in zip(dD, tr.dD(c, D, np.float64)):
        assert np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b)), key
    got = {t: m.small_sample(c["theta"], c["beta"], c["var_par"], on="host", type=t) for t in sr.TYPES}
    ref, sc = sr.reference(c, D), sr.scales(c, D)
    blocks = m._small_sample_blocks(c["theta"], c["beta"], c["var_par"], "host")     # the model's own host path
    r = sr.ratio(blocks, ref, sc)
    print("%s model host path: ratio %.3f of HOST_RATIO %.1f" % (key, r, sr.HOST_RATIO))
    assert r <= sr.HOST_RATIO
    assert np.array_equal(blocks["information"], got["KR"]["information"])
    info, tinfo = got["KR"]["information"], got["KR"]["theta_information"]
    assert ir.ratio(info, ir.reference(c, D), c) <= ir.C_INFO and tr.ratio(tinfo, tr.reference(c, D)) <= tr.C_TI
    for t in sr.TYPES:
        want = sr.kr(info, tinfo, blocks["P"], blocks["Q"], blocks["R"], t)
        g = got[t]
        assert g["type"] == t and len(g["names"]) == sr.rows(c) and (g["names"][-1] == "sigma") == sr.sigma_row(c)
        for k in ("vcov", "se", "dof", "vcov_unadjusted"):
            atol = 1e-10 * np.nanmax(np.abs(want[k])) if np.any(np.isfinite(want[k])) else 0.0   # an entry that cancels to 0
            assert np.allclose(g[k], want[k], rtol=1e-7, atol=atol, equal_nan=True), (key, t, k)
        # (KR2's -R_rs / 4 can take a variance below 0 where theta is as small as the family designs': se is then NaN)
        assert np.all(g["dof"] > 0) and (t == "KR2" or np.all(np.isfinite(g["se"])))
    assert np.array_equal(got["sat"]["vcov"], got["sat"]["vcov_unadjusted"])
    assert np.array_equal(got["KR"]["dof"], got["sat"]["dof"])


def test_device_path_calls_the_export_and_does_the_host_algebra():
    d, be, m = _model("poisson")
    for t in sr.TYPES:
        r = m.small_sample(d["theta"], d["beta"], 1.0, on="device", type=t)
        a, k = be.calls[-1][1], be.calls[-1][2]
        assert be.calls[-1][0] == "small_sample" and a[3] is m.Z and a[4] is m.X and a[5] == "poisson" and a[6] == "log"
        assert np.array_equal(a[7], d["beta"]) and np.array_equal(a[8], d["theta"]) and k["var_par"] == 1.0
        b = be.blocks
        want = sr.kr(b["information"], b["theta_information"], b["P"], b["Q"], b["R"], t)
        for key in ("vcov", "se", "dof", "vcov_unadjusted"):
            assert np.allclose(r[key], want[key], rtol=1e-13, atol=0), (t, key)
        assert r["names"] == m._cov_par_names() and r["type"] == t
        assert np.array_equal(r["information"], b["information"]) and np.array_equal(r["theta_information"], b["theta_information"])
    assert _names(be).count("small_sample") == 3


@pytest.mark.parametrize("fit", ["MCML", "LA"])
@pytest.mark.parametrize("type_", ["KR", "KR2", "sat"])
def test_the_keyword_attaches_a_record_and_leaves_the_table(fit, type_):
    d, be, m = _model("poisson")
    P = m.X.shape[1]
    f = m.MCML(d["y"], verbose=False, small_sample=type_) if fit == "MCML" else m.LA(d["y"], small_sample=type_)
    calls = [c for c in be.calls if c[0] == "small_sample"]
    assert len(calls) == 1
    a, k = calls[0][1], calls[0][2]
    # the FINAL estimates of the fake fit
    assert np.array_equal(a[7], np.full(P, 0.5)) and np.array_equal(a[8], np.full(2, 0.2)) and k["var_par"] == 1.0
    b = be.blocks
    want = sr.kr(b["information"], b["theta_information"], b["P"], b["Q"], b["R"], type_)
    rec = f["small_sample"]
    assert rec["type"] == type_ and set(rec) == {"type", "vcov", "se", "dof", "lower", "upper"}
    assert np.allclose(rec["vcov"], want["vcov"], rtol=1e-13) and np.allclose(rec["dof"], want["dof"], rtol=1e-13)
    q = stats.t.ppf(0.975, want["dof"])
    est = f["coefficients"]["est"][:P]
    assert np.allclose(rec["lower"], est - q * want["se"], rtol=1e-12) and np.allclose(rec["upper"], est + q * want["se"], rtol=1e-12)
    assert np.all(q > 1.959963984540054)                                # wider than the normal interval
    text = str(f)
    assert "Small-sample correction of the fixed effects (%s)" % type_ in text and "d.f." in text
    # the default: no call, no record, the same table and the same print without the record's lines
    d0, be0, m0 = _model("poisson")
    f0 = m0.MCML(d0["y"], verbose=False) if fit == "MCML" else m0.LA(d0["y"])
    assert "small_sample" not in _names(be0) and "small_sample" not in f0
    for key in ("est", "SE", "lower", "upper"):
        assert np.array_equal(f["coefficients"][key], f0["coefficients"][key], equal_nan=True), key
    assert "Small-sample" not in str(f0) and all(line in text.split("\n") for line in str(f0).split("\n"))
    assert _names(be0) == [n for n in _names(be) if n != "small_sample"]


def test_a_singular_information_gives_nan_and_a_warning():
    d, be, m = _model("poisson")
    blocks = _blocks(m.X.shape[1], 2)
    blocks["theta_information"] = np.array([[1.0, 1.0], [1.0, 1.0]])
    be.blocks = blocks
    with pytest.warns(UserWarning, match="not invertible"):
        r = m.small_sample(d["theta"], d["beta"], 1.0, on="device")
    assert np.all(np.isnan(r["dof"])) and np.all(np.isnan(r["se"])) and np.all(np.isnan(r["vcov"]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # the fit records the warning instead of raising it
        f = m.LA(d["y"], small_sample="KR")
    assert any("not invertible" in w for w in f["warnings"])
    assert np.all(np.isnan(f["small_sample"]["dof"])) and np.all(np.isnan(f["small_sample"]["lower"]))


def test_argument_validation():
    d, be, m = _model("binomial")
    with pytest.raises(ValueError, match="small_sample"):
        m.MCML(d["y"], verbose=False, small_sample="kr")
    with pytest.raises(ValueError, match="small_sample"):
        m.LA(d["y"], small_sample="satterthwaite")
    with pytest.raises(ValueError, match="type"):
        m.small_sample(d["theta"], d["beta"], 1.0, type="KR3")
    with pytest.raises(ValueError, match="on should be"):
        m.small_sample(d["theta"], d["beta"], 1.0, on="gpu")
    assert "small_sample" not in _names(be)
