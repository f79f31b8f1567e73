"""Calibration of the bound tests/test_gpu_theta_information.py holds the device to (tests/theta_information_reference.py):
the analytic d D of the reference against central differences, the float64 twin of the Q x Q form and the host formula against
the long-double n x n definition, on every case the GPU test runs.  No GPU: D comes from the CPU oracle."""
import numpy as np
import pytest

import cov_layouts as cl
import theta_information_reference as tr

LD = tr.LD


@pytest.fixture(scope="module")
def refs(orc):
    """key -> (D, long-double reference), computed once"""
    out = {}
    for key in tr.KEYS:
        c = tr.case(key)
        D = np.asarray(orc.gen_D(c["cov"], c["data"], c["eff_range"], c["theta"], chol=False))
        out[key] = (D, tr.reference(c, D))
    return out


@pytest.mark.parametrize("key", ["stepped_wedge_7x8x3", "wide_41", "geo150", "mixed"])
def test_analytic_dD_against_central_differences(key):
    """every function of the table, a product of two terms, a shared parameter and the all-gr blocks: long-double central
    differences of cov_layouts.block_matrix with a relative step of 1e-6 (truncation 1e-12 relative, rounding 1e-19 / 1e-6);
    1e-9 guards formulas, not rounding"""
    c = tr.case(key)
    theta = c["theta"]
    blocks = cl.from_wire(c["cov"], c["data"])

    def dense(th):
        mats = []
        for b in blocks:
            D = cl.block_matrix(b, th, LD)[0]
            mats.append(D * np.eye(b[0], dtype=LD) if cl.kind(b) == "diag" else D)
        return cl.block_diag(mats)

    D = dense(theta)
    got = tr.dD(c, D.astype(np.float64))
    assert len(got) == theta.size
    for r in range(theta.size):
        h = LD(theta[r]) * LD(1e-6)
        up, dn = theta.astype(LD), theta.astype(LD)
        up[r] += h; dn[r] -= h
        # block_matrix takes float64 parameters: the step is made of the float64 values actually used
        up64, dn64 = up.astype(np.float64), dn.astype(np.float64)
        fd_ = (dense(up64) - dense(dn64)) / (up64.astype(LD)[r] - dn64.astype(LD)[r])
        scale = np.max(np.abs(fd_))
        assert scale > 0, (key, r)
        err = float(np.max(np.abs(got[r] - fd_)) / scale)
        print("%s d/dtheta%d: relative difference %.2e" % (key, r, err))
        assert err <= 1e-9, (key, r, err)


def test_twin_against_long_double_gives_the_constant(refs):
    worst, where = 0.0, None
    for key in tr.KEYS:
        c = tr.case(key)
        D, ref = refs[key]
        r = tr.ratio(tr.twin(c, D), ref)
        print("%-24s twin ratio %10.3f   max|I| %.3g   (%d x %d)" % (key, r, float(np.max(np.abs(ref))), *ref.shape))
        if r > worst:
            worst, where = r, key
    D, ref = refs["weak"]
    print("weak, B = I - M^-1 instead (not used): ratio %.3g" % tr.ratio(tr.twin_cancelling(tr.case("weak"), D), ref))
    print("worst twin ratio %.3f at %s; TWIN_RATIO %.1f, C_TI %.1f" % (worst, where, tr.TWIN_RATIO, tr.C_TI))
    assert worst <= tr.TWIN_RATIO, (worst, where)
    assert worst >= tr.TWIN_RATIO / 4, "TWIN_RATIO is no longer the measured value rounded up: %.3f at %s" % (worst, where)
    assert tr.C_TI == 8 * tr.TWIN_RATIO


def test_host_formula_against_long_double(refs):
    for key in tr.KEYS:
        c = tr.case(key)
        D, ref = refs[key]
        r = tr.ratio(tr.host_formula(c, D), ref)
        print("%-24s host formula ratio %.3f" % (key, r))
        assert r <= tr.C_TI, (key, r)


def test_reference_is_symmetric_and_positive_definite(refs):
    for key in tr.KEYS:
        ref = refs[key][1].astype(np.float64)
        assert ref.shape == (tr.rows(tr.case(key)),) * 2
        assert np.allclose(ref, ref.T, rtol=1e-13, atol=0)
        assert np.all(np.linalg.eigvalsh((ref + ref.T) / 2) > 0), key


def test_cases_are_what_the_gpu_test_says_they_are():
    assert tr.case("family-poisson-log")["Z"].shape == (144, 24)
    assert tr.rows(tr.case("family-gaussian-identity")) == 3 and tr.rows(tr.case("family-gamma-log")) == 2
    assert np.array_equal(tr.case("weak")["theta"], tr.case("family-poisson-log")["theta"] * 0.02)
    assert tr.case("wide_41")["Z"].shape[1] == 3 * 41 and tr.case("comp65")["Z"].shape[1] == 2 * 65
    c = tr.case("split_block")
    assert c["Z"].shape == (7 * 8 * 3 - 3, 56) and not np.any(c["Z"][:, 7]) and np.all(np.any(c["Z"][:, :7], axis=0))
    assert tr.case("geo300")["Z"].shape == (300, 300) and tr.rows(tr.case("geo300")) == 3
    assert tr.case("densez_poisson_log")["Z"].shape == (297, 36)
    m = tr.case("mixed")
    assert m["theta"].size == 10 and m["Z"].shape == (522, 522)
    assert sorted(tr.COMPONENT_KEYS + tr.DENSE_KEYS) == sorted(tr.KEYS)
    for key in tr.KEYS:
        assert tr.case(key)["op"] == (1 if key in tr.COMPONENT_KEYS else 0), key
