"""ModelMCML.sandwich and the `sandwich=` keyword of MCML() / LA() (glmmrmcml_amd/model.py) without a GPU: the host formula
against the long-double reference of tests/sandwich_reference.py (D from the CPU oracle), the CR1 factor, the host union-find
against the rule of csrc/component_plan.h, and the keyword's bookkeeping with a recording backend."""
import numpy as np
import pytest

import information_reference as ir
import sandwich_reference as sr
from glmmrmcml_amd import synth
from glmmrmcml_amd.model import ModelMCML, components_of_rows
from test_model_caller import FakeBackend


class OracleBackend:
    """Context(...).gen_D from the CPU oracle: all that sandwich(on="host") asks of a backend"""

    def __init__(self, orc):
        self.orc = orc

    def Context(self, cov, data, eff):
        be = self

        class Ctx:
            def __enter__(self):
                return self

            def __exit__(self, *a):
                return False

            def gen_D(self, theta, chol=False):
                return np.asarray(be.orc.gen_D(cov, data, eff, np.asarray(theta, float), chol=chol))

        return Ctx()


def _model(c, be):
    return ModelMCML(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], ir.model_family(c["family"]), c["link"], c["beta"],
                     c["theta"], var_par=c["var_par"], backend=be)


@pytest.mark.parametrize("name", ["family-poisson-log", "family-gamma-inverse", "family-binomial-probit", "geo150_p1",
                                  "stepped_wedge_7x8x3+unions", "longitudinal_70x3+across"])
def test_host_sandwich_against_the_reference(name, orc):
    c = sr.case(name)
    D = np.asarray(orc.gen_D(c["cov"], c["data"], c["eff_range"], c["theta"], chol=False))
    a, G, B = sr.reference(c, D)
    r = _model(c, OracleBackend(orc)).sandwich(c["y"], c["theta"], c["beta"], c["var_par"], cluster=c["cluster"], on="host")
    assert r["ncluster"] == G.shape[0] and r["adjust"] == "CR0"
    ratio = sr.ratio(r["scores"], G, sr.score_scale(c, D))
    print("%s host ratio %.3f of C_SAND %.1f" % (name, ratio, sr.C_SAND))
    assert ratio <= sr.C_SAND
    assert sr.meat_excess(r["meat"], r["scores"]) <= 1.0
    assert ir.ratio(r["information"], ir.reference(c, D), c) <= ir.C_INFO
    want = np.linalg.solve(r["information"], np.linalg.solve(r["information"], r["meat"]).T)
    assert np.array_equal(r["vcov"], want) and np.array_equal(r["se"], np.sqrt(np.diag(want)))


def test_cr1_factor(orc):
    c = sr.case("stepped_wedge_7x8x3+unions")
    m = _model(c, OracleBackend(orc))
    r0 = m.sandwich(c["y"], c["theta"], c["beta"], 1.0, cluster=c["cluster"], on="host")
    r1 = m.sandwich(c["y"], c["theta"], c["beta"], 1.0, cluster=c["cluster"], on="host", adjust="CR1")
    n, P, G = c["X"].shape[0], c["X"].shape[1], 3
    assert (n, P) == (168, 9) and r1["ncluster"] == G and r1["adjust"] == "CR1"
    assert np.array_equal(r1["vcov"], r0["vcov"] * (G / (G - 1.0) * (n - 1.0) / (n - P)))
    assert np.array_equal(r1["meat"], r0["meat"]) and np.array_equal(r1["information"], r0["information"])
    with pytest.raises(ValueError, match="adjust"):
        m.sandwich(c["y"], c["theta"], c["beta"], 1.0, on="host", adjust="CR2")
    with pytest.raises(ValueError, match="on should"):
        m.sandwich(c["y"], c["theta"], c["beta"], 1.0, on="gpu")
    with pytest.raises(ValueError, match="cluster"):
        m.sandwich(c["y"], c["theta"], c["beta"], 1.0, cluster=np.zeros(5, int), on="host")


def plan_rule(d):
    """comp_of_row of csrc/component_plan.h, restated: the ELL row of observation i holds, for every nonzero (i, j) of Z,
    the columns from the start of j's covariance block to j (csrc/model.hip sparse_zl_setup); a union-find over the rows whose
    root is the smallest variable; components numbered by it; a row belongs to the component of its first column"""
    cov = np.asarray(d["cov"])
    start_of, at, r = [], 0, 0
    while r < cov.shape[0]:
        dim = int(cov[r, 1])
        start_of += [at] * dim
        at += dim
        bid = cov[r, 0]
        while r < cov.shape[0] and cov[r, 0] == bid:
            r += 1
    Q = at
    parent = list(range(Q))

    def find(q):
        while parent[q] != q:
            parent[q] = parent[parent[q]]
            q = parent[q]
        return q

    first = []
    for row in np.asarray(d["Z"]):
        cols = [t for j in np.nonzero(row)[0] for t in range(start_of[j], j + 1)]
        first.append(cols[0])
        for t in cols[1:]:
            a, b = find(cols[0]), find(t)
            if a != b:
                parent[max(a, b)] = min(a, b)
    comp, ncomp = {}, 0
    for q in range(Q):
        rt = find(q)
        if rt not in comp:
            comp[rt] = ncomp
            ncomp += 1
    return np.array([comp[find(q)] for q in first]), ncomp


@pytest.mark.parametrize("design,ncomp", [(lambda: synth.stepped_wedge(7, 8, 3), 7), (lambda: synth.longitudinal(70, 3), 70)])
def test_host_union_find_equals_the_component_plan_rule(design, ncomp, orc):
    d = design()
    L = np.asarray(orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True))
    got, n_got = components_of_rows(d["Z"] @ L)
    want, n_want = plan_rule(d)
    assert n_got == n_want == ncomp and np.array_equal(got, want)
    with pytest.raises(ValueError, match="no entry"):
        components_of_rows(np.vstack([d["Z"] @ L, np.zeros((1, d["Q"]))]))


class SandwichBackend(FakeBackend):
    """the recording backend of tests/test_model_caller.py with the `sandwich` export: bread diag(2, 3, ...), meat the identity"""

    def sandwich(self, *a, **k):
        self._rec("sandwich", a, k)
        info = np.diag(np.arange(2.0, 2.0 + self.P))
        return dict(information=info, meat=np.eye(self.P), scores=np.eye(4, self.P), ncluster=4,
                    vcov=np.linalg.inv(info) @ np.linalg.inv(info))


def _fake(family):
    d = synth.cluster_rct(ncl=4, nt=3, nind=3, seed=1, family=family)
    be = SandwichBackend(d["P"], 2, d["Z"].shape[1])
    return d, be, ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                            var_par=1.3, backend=be)


@pytest.mark.parametrize("fit_with", ["MCML", "LA"])
def test_the_keyword_adds_a_record_and_nothing_else(fit_with):
    d, be, m = _fake("binomial" if fit_with == "MCML" else "poisson")
    kw = dict(verbose=False) if fit_with == "MCML" else {}
    cluster = np.arange(d["n"]) % 4
    fit = getattr(m, fit_with)(d["y"], sandwich="CR1", cluster=cluster, **kw)
    calls = [c for c in be.calls if c[0] == "sandwich"]
    assert len(calls) == 1
    a, k = calls[0][1], calls[0][2]
    P, n = d["P"], d["n"]
    # (cov, data, eff_range, Z, X, y, family, link, beta, theta): the FINAL estimates of the fake fit
    assert a[3] is m.Z and a[4] is m.X and np.array_equal(a[5], d["y"]) and a[6] == m.family and a[7] == m.link
    assert np.array_equal(a[8], fit["theta"][:P]) and np.array_equal(a[9], fit["theta"][P:P + 2])
    assert k["var_par"] == 1.0 and np.array_equal(k["cluster"], cluster) and k["scores"] is True
    rb = fit["robust"]
    factor = 4 / 3.0 * (n - 1.0) / (n - P)
    assert rb["adjust"] == "CR1" and rb["ncluster"] == 4
    assert np.allclose(rb["vcov"], np.diag(1 / np.arange(2.0, 2.0 + P) ** 2) * factor, rtol=1e-14, atol=0)
    assert np.array_equal(rb["se"], np.sqrt(np.diag(rb["vcov"])))
    d2, be2, m2 = _fake(d["family"])
    plain = getattr(m2, fit_with)(d2["y"], **kw)
    assert "robust" not in plain and "sandwich" not in [c[0] for c in be2.calls]
    for key in ("par", "est", "SE", "lower", "upper"):
        assert np.array_equal(np.asarray(fit["coefficients"][key]), np.asarray(plain["coefficients"][key]), equal_nan=(key != "par"))
    assert str(fit) == str(plain)
    with pytest.raises(ValueError, match="sandwich"):
        getattr(m, fit_with)(d["y"], sandwich="CR2", **kw)
