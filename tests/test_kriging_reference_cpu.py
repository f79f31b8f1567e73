"""tests/kriging_reference.py on its own: the float64 twins against the long-double reference (the calibration of C_KRIGE),
the power of the bound, the identities of a coincident point and the conditioning of the cases.  No GPU, no library call.

Measured on these cases (the twins' worst ratios against 2^-52 S): means 0.0406 (MIXED_m70, the module's float64 pass),
cvar 0.0643 (MIXED_m3, the same pass); ModelMCML.predict(on="host") 0.0299 and 0.0296.  TWIN_RATIO = 0.07 is the larger
rounded up and C_KRIGE = 8 * TWIN_RATIO = 0.56.  The smallest move of a dense block under theta * (1 + 1e-6): 5.4e3 units
of 2^-52 S (TWO_LARGE_A), against 100 * C_KRIGE = 56."""
import numpy as np
import pytest

import cov_layouts as cl
import kriging_reference as kr
from glmmrmcml_amd import model

CASES = [k for k in kr.KEYS if kr.case(k)["chunk"] is None]          # the chunked case is MIXED_m3 with an environment variable


def _fit(c):
    """a fit record as ModelMCML.predict reads it: P = 1, theta = (beta, covariance parameters, sigma)"""
    return dict(theta=np.r_[0.5, c["theta"], 1.0], re_samps=c["u"])


def _model(c):
    cov, data = cl.layout(c["blocks"])
    Q = cl.total_dim(c["blocks"])
    return model.ModelMCML(cov, data, np.zeros(1), np.eye(Q), np.ones((Q, 1)), "gaussian", "identity", [0.5], c["theta"])


@pytest.mark.parametrize("key", CASES)
def test_the_float64_twins_stay_within_an_eighth_of_the_bound(key):
    c, ref = kr.case(key), kr.reference(key)
    tw = kr.evaluate(c, np.float64, scales=False)
    own = kr.ratios(dict(means=tw["means"], mean=tw["mean"], cond_var=tw["cvar"]), ref, c["m"])
    host = model.predict_host(*cl.layout(c["blocks"]), c["theta"], c["u"], c["newdata"], means=True)
    hr = kr.ratios(host, ref, c["m"])
    print(key, "own pass", own, "host", hr)
    for r in (own, hr):
        assert r[0] <= kr.TWIN_RATIO and r[2] <= kr.TWIN_RATIO and r[1] <= 1.0 / 8, (key, r)
    assert kr.C_KRIGE == 8 * kr.TWIN_RATIO
    # the caller layer hands the same numbers on
    p = _model(c).predict(_fit(c), c["newdata"], on="host")
    assert np.array_equal(p["re_mean"], host["mean"]) and np.array_equal(p["cond_var"], host["cond_var"])
    assert kr.sample_var_check(host, c["m"])[0] <= 1.0


@pytest.mark.parametrize("key", CASES)
def test_a_relative_change_of_1e_6_in_theta_is_far_outside_the_bound(key):
    """on every dense block that has a moved point (the one new point of EDGE32's 32 block is the coincident one, whose
    mean is the observed sample whatever theta is)"""
    c, ref = kr.case(key), kr.reference(key)
    pert = kr.evaluate(c, kr.LD, theta=c["theta"] * (1 + 1e-6), scales=False)
    seen = 0
    for sl in ref["block"]:
        if not ref["dense"][sl][0] or sl.stop - sl.start < 2:
            continue
        move = float(np.max(np.abs(pert["means"][sl] - ref["means"][sl]) / (kr.EPS * ref["S_mean"][sl])))
        assert move > 100 * kr.C_KRIGE, (key, sl, move)
        seen += 1
    assert seen >= 1


@pytest.mark.parametrize("key", CASES)
def test_a_coincident_point_returns_the_sample_and_no_variance(key):
    c, ref = kr.case(key), kr.reference(key)
    s = r = 0
    for block, xn in zip(c["blocks"], c["newdata"]):
        dim = block[0]
        if xn is not None:
            if cl.kind(block) != "diag":
                X = kr._block_columns(block)[0]
                row = int(np.flatnonzero((X == xn[0]).all(1))[0])
                d = np.abs(ref["means"][r] - c["u"][s + row].astype(kr.LD))
                assert np.all(d <= kr.C_KRIGE * kr.EPS * ref["S_mean"][r]), (key, r)
                assert ref["cvar"][r] <= 1e-15 * ref["prior"][r]
            else:                                               # a matched level: the sample itself; an unmatched one: 0 and p
                row = int(np.flatnonzero((kr._block_columns(block)[0] == xn[0]).all(1))[0])
                assert np.array_equal(ref["means"][r].astype(float), c["u"][s + row]) and ref["cvar"][r] == 0
                if len(xn) > 1:
                    assert np.all(ref["means"][r + 1] == 0) and ref["cvar"][r + 1] == ref["prior"][r + 1]
            r += len(xn)
        s += dim


def test_every_block_is_well_conditioned():
    for key in CASES:
        c = kr.case(key)
        for block in c["blocks"]:
            assert np.linalg.cond(cl.block_matrix(block, c["theta"])[0]) < 1e4, key


def test_the_cases_reach_the_branches_they_name():
    c = kr.case("MIXED_m3")
    assert c["served"] == dict(diag=3, small=2, large=3) and c["K"] == sum(kr.MIXED_COUNTS) == 266
    assert kr.chunks_expected(c) == 8 and kr.chunks_expected(kr.case("MIXED_chunk64")) == 1 + 1 + 3 + 1 + 1 + 2 + 1 + 1
    assert kr.case("MIXED_m70")["m"] == 70 and kr.case("EDGE32")["served"] == dict(diag=0, small=1, large=1)
    assert [b[0] for b in kr.case("TWO_LARGE_B")["blocks"]] == [161, 300]
    assert all(kr.case(k)["why"] for k in kr.KEYS)
