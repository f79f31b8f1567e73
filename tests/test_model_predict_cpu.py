"""ModelMCML.predict(on="host"): shapes, the law of total variance, the one-column convention, the linear predictor with and
without Z, argument errors.  No GPU: the host path is numpy."""
import numpy as np
import pytest

import cov_layouts as cl
import kriging_reference as kr
from glmmrmcml_amd import model


def _setup(m):
    c = kr.case("EDGE32")
    cov, data = cl.layout(c["blocks"])
    Q = cl.total_dim(c["blocks"])
    rng = np.random.default_rng(3)
    X = np.column_stack([np.ones(Q), rng.standard_normal(Q)])
    mod = model.ModelMCML(cov, data, np.zeros(1), np.eye(Q), X, "gaussian", "identity", [0.5, -0.2], c["theta"])
    fit = dict(theta=np.r_[0.5, -0.2, c["theta"], 1.0], re_samps=cl.sample_matrix("EDGE32")[:, :m])
    return c, mod, fit


def test_shapes_and_the_law_of_total_variance():
    c, mod, fit = _setup(4)
    p = mod.predict(fit, c["newdata"], on="host")
    assert set(p) == {"re_mean", "re_var", "cond_var", "sample_var"}
    assert all(p[k].shape == (c["K"],) for k in p)
    assert np.array_equal(p["re_var"], p["cond_var"] + p["sample_var"])
    assert np.all(p["cond_var"] >= 0) and np.all(p["sample_var"] >= 0)
    ref = kr.reference("EDGE32")
    assert np.allclose(p["re_mean"], ref["mean"].astype(float), rtol=0, atol=1e-12)
    assert p["cond_var"][0] <= 1e-12 * ref["prior"][0]                       # the coincident point


def test_one_sample_column_has_no_between_sample_variance():
    c, mod, fit = _setup(1)
    p = mod.predict(fit, c["newdata"], on="host")
    assert np.all(np.isnan(p["sample_var"])) and np.array_equal(p["re_var"], p["cond_var"])
    fit["re_samps"] = fit["re_samps"][:, 0]                                   # a vector is one column
    q = mod.predict(fit, c["newdata"], on="host")
    assert np.array_equal(q["re_mean"], p["re_mean"])


def test_the_linear_predictor_with_and_without_z():
    c, mod, fit = _setup(4)
    K = c["K"]
    rng = np.random.default_rng(4)
    X = np.column_stack([np.ones(K), rng.standard_normal(K)])
    p = mod.predict(fit, c["newdata"], X=X, on="host")
    assert np.array_equal(p["linear_predictor"], X @ np.array([0.5, -0.2]) + p["re_mean"])
    Z = rng.standard_normal((5, K))
    q = mod.predict(fit, c["newdata"], X=X[:5], Z=Z, on="host")
    assert q["linear_predictor"].shape == (5,)
    assert np.array_equal(q["linear_predictor"], X[:5] @ np.array([0.5, -0.2]) + Z @ q["re_mean"])


def test_argument_errors():
    c, mod, fit = _setup(4)
    K = c["K"]
    with pytest.raises(ValueError, match="on should be"):
        mod.predict(fit, c["newdata"], on="gpu")
    with pytest.raises(ValueError, match="blocks"):
        mod.predict(fit, c["newdata"][:1], on="host")
    with pytest.raises(ValueError, match="columns"):
        mod.predict(fit, [np.zeros((2, 3)), None], on="host")
    with pytest.raises(ValueError, match="no new points"):
        mod.predict(fit, [None, None], on="host")
    with pytest.raises(ValueError, match="pass Z"):
        mod.predict(fit, c["newdata"], X=np.ones((K + 1, 2)), on="host")
    with pytest.raises(ValueError, match="Z must be"):
        mod.predict(fit, c["newdata"], X=np.ones((3, 2)), Z=np.ones((3, K + 1)), on="host")
    with pytest.raises(ValueError, match="X must have"):
        mod.predict(fit, c["newdata"], X=np.ones((K, 3)), on="host")
    with pytest.raises(ValueError, match="Z without X"):
        mod.predict(fit, c["newdata"], Z=np.eye(K), on="host")
    bad = dict(fit, re_samps=fit["re_samps"][:-1])
    with pytest.raises(ValueError, match="re_samps"):
        mod.predict(bad, c["newdata"], on="host")
