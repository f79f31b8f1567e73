"""Calibration of the bound tests/test_gpu_sandwich.py holds the device to (tests/sandwich_reference.py): the float64 twin of
the Woodbury route and the host formula against the long-double definition, on every case the GPU test runs.  No GPU: D comes
from the CPU oracle."""
import numpy as np
import pytest

import sandwich_reference as sr


@pytest.fixture(scope="module")
def refs(orc):
    """name -> (D, (a, G, B) in long double, S_G), computed once"""
    out = {}
    for name in sr.NAMES:
        c = sr.case(name)
        D = np.asarray(orc.gen_D(c["cov"], c["data"], c["eff_range"], c["theta"], chol=False))
        out[name] = (D, sr.reference(c, D), sr.score_scale(c, D))
    return out


def test_cases_are_usable(refs):
    """e is finite, Sigma is positive definite (the reference factorised it), at least two clusters, and a default-cluster case
    has no observation without an entry of ZL"""
    for name in sr.NAMES:
        c = sr.case(name)
        D, (a, G, B), scale = refs[name]
        assert np.all(np.isfinite(sr.residual(c))), name
        assert np.all(np.isfinite(a.astype(np.float64))) and np.isfinite(scale) and scale > 0, name
        S = np.diag(sr.ir.weights(c)) + c["Z"] @ D @ c["Z"].T
        assert np.all(np.linalg.eigvalsh(S) > 0), name
        assert G.shape[0] >= 2 and G.shape[1] == c["X"].shape[1], name
        ids = sr.clusters(c, D)
        assert ids.shape == (c["X"].shape[0],) and ids.min() == 0 and np.all(np.bincount(ids) > 0), name
        if c["cluster"] is None:
            ZL = c["Z"] @ np.linalg.cholesky(D)
            assert np.all((ZL != 0).any(axis=1)), name
    assert set(sr.DEFAULT_NAMES) == set(sr.ir.FAMILY_KEYS + sr.ir.COMPONENT_KEYS + sr.ir.WIDE_KEYS)


def test_the_cluster_rules_are_what_they_claim(refs):
    c = sr.case("stepped_wedge_7x8x3+unions")
    comp = sr.components(c["Z"] @ np.linalg.cholesky(refs[c["name"]][0]))
    assert comp.max() == 6
    for k in range(7):                                               # every component lies inside one cluster
        assert len(set(c["cluster"][comp == k])) == 1
    assert [sorted(set(comp[c["cluster"] == g])) for g in range(3)] == [[0, 1], [2, 3], [4, 5, 6]]
    c = sr.case("longitudinal_70x3+across")
    comp = sr.components(c["Z"] @ np.linalg.cholesky(refs[c["name"]][0]))
    assert comp.max() == 69 and all(len(set(c["cluster"][comp == k])) > 1 for k in range(70))      # cut across
    c = sr.case("comp129")
    assert np.array_equal(c["cluster"], sr.components(c["Z"] @ np.linalg.cholesky(refs["comp129"][0])))


def test_twin_against_long_double_gives_the_constant(refs):
    worst, where = 0.0, None
    for name in sr.NAMES:
        c = sr.case(name)
        D, (a, G, B), scale = refs[name]
        r = sr.ratio(sr.twin(c, D)[1], G, scale)
        print("%-32s twin ratio %.3f  S_G %.3g  max|G| %.3g  clusters %d" % (name, r, scale, float(np.max(np.abs(G))), G.shape[0]))
        if r > worst:
            worst, where = r, name
    print("worst twin ratio %.3f at %s; TWIN_RATIO %.2f, C_SAND %.1f" % (worst, where, sr.TWIN_RATIO, sr.C_SAND))
    assert worst <= sr.TWIN_RATIO, (worst, where)
    assert worst >= sr.TWIN_RATIO / 4, "TWIN_RATIO is no longer the measured value rounded up: %.3f at %s" % (worst, where)
    assert sr.C_SAND == 8 * sr.TWIN_RATIO


def test_host_formula_against_long_double(refs):
    for name in sr.NAMES:
        c = sr.case(name)
        D, (a, G, B), scale = refs[name]
        r = sr.ratio(sr.host_formula(c, D)[1], G, scale)
        print("%-32s host formula ratio %.3f" % (name, r))
        assert r <= sr.C_SAND, (name, r)


def test_meat_bound_holds_for_a_float64_product(refs):
    """the derived bound of the meat on numpy's own G' G: any order of the sum stays inside it"""
    for name in sr.NAMES:
        G = refs[name][1][1].astype(np.float64)
        assert sr.meat_excess(G.T @ G, G) <= 1.0, name
