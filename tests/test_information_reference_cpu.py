"""Calibration of the bound tests/test_gpu_information.py holds the device to (tests/information_reference.py): the float64
twin of the Woodbury form and the host formula against the long-double definition, on every case the GPU test runs.  No GPU:
D comes from the CPU oracle."""
import numpy as np
import pytest

import family_designs as fd
import information_reference as ir


@pytest.fixture(scope="module")
def refs(orc):
    """key -> (D, long-double reference), computed once"""
    out = {}
    for key in ir.KEYS:
        c = ir.case(key)
        D = np.asarray(orc.gen_D(c["cov"], c["data"], c["eff_range"], c["theta"], chol=False))
        out[key] = (D, ir.reference(c, D))
    return out


def test_twin_against_long_double_gives_the_constant(refs):
    worst, where = 0.0, None
    for key in ir.KEYS:
        c = ir.case(key)
        D, ref = refs[key]
        r = ir.ratio(ir.twin(c, D), ref, c)
        print("%-28s twin ratio %.3f  max|X'VX| %.3g  max|info| %.3g" % (key, r, ir.xtvx_max(c), float(np.max(np.abs(ref)))))
        if r > worst:
            worst, where = r, key
    print("worst twin ratio %.3f at %s; TWIN_RATIO %.1f, C_INFO %.1f" % (worst, where, ir.TWIN_RATIO, ir.C_INFO))
    assert worst <= ir.TWIN_RATIO, (worst, where)
    assert worst >= ir.TWIN_RATIO / 4, "TWIN_RATIO is no longer the measured value rounded up: %.3f at %s" % (worst, where)
    assert ir.C_INFO == 8 * ir.TWIN_RATIO


def test_host_formula_against_long_double(refs):
    for key in ir.KEYS:
        c = ir.case(key)
        D, ref = refs[key]
        r = ir.ratio(ir.host_formula(c, D), ref, c)
        assert r <= ir.C_INFO, (key, r)


def test_reference_is_symmetric_and_positive_definite(refs):
    for key in ir.KEYS:
        ref = refs[key][1].astype(np.float64)
        assert np.allclose(ref, ref.T, rtol=1e-13, atol=0)
        assert np.all(np.linalg.eigvalsh((ref + ref.T) / 2) > 0), key


def test_weights_are_finite_and_positive_inside_the_domain():
    for key in ir.KEYS:
        c = ir.case(key)
        assert fd.in_domain(c["family"], c["link"], c["X"] @ c["beta"]), key
        w = ir.weights(c)
        assert np.all(np.isfinite(w)) and np.all(w > 0), key
        assert np.all(np.isfinite(1 / w)), key


def test_cases_are_what_the_gpu_test_says_they_are():
    """the shapes behind the GPU test's claims: components, their sizes, P"""
    from glmmrmcml_amd import synth  # noqa: F401
    c = ir.case("family-poisson-log")
    assert c["X"].shape[0] == 144 and c["Z"].shape[1] == 24
    assert ir.case("longitudinal_70x3")["X"].shape[1] == 2 and ir.case("stepped_wedge_7x8x3")["X"].shape[1] == 9
    assert ir.case("wide_41")["X"].shape[1] == 41 and ir.case("wide_41_p71")["X"].shape[1] == 71      # 64 + a chunk of 7
    assert ir.case("geo300_p3")["Z"].shape == (300, 300) and ir.case("geo300_p3")["X"].shape[1] == 3
    assert ir.case("geo150_p1")["X"].shape[1] == 1
    assert ir.case("densez_poisson_log")["Z"].shape == (297, 36)
    assert ir.case("comp129")["Z"].shape == (256, 258) and ir.case("comp129")["X"].shape[1] == 129
    for key in ir.KEYS:                                              # full column rank: the information is invertible
        X = ir.case(key)["X"]
        assert np.linalg.matrix_rank(X) == X.shape[1], key
