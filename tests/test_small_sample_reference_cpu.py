"""Calibration of the bound tests/test_gpu_small_sample.py holds the device to (tests/small_sample_reference.py): the
reference's second derivatives of D against second central differences, -Phi P_r Phi against central differences of Phi(theta)
(which pins what P_r means), the float64 twin of the Q x Q form and the host formula against the long-double n x n definition on
every case the GPU test runs, and the one-row Kenward-Roger degrees of freedom against Satterthwaite's.  No GPU: D comes from the
CPU oracle.

Measured here, in units of 2^-52 S per output block: the twin's worst ratio 16.626 (longitudinal_70x3, P_1; next
family-gamma-log 4.403, wide_41 4.351, the dense cases 0.04 .. 2.8), the host formula's 11.574 (family-poisson-log; next
family-gaussian-identity 8.78, weak 7.70).  TWIN_RATIO = 17 and HOST_RATIO = 12 of the reference module are these rounded up to
the next integer."""
import numpy as np
import pytest

import cov_layouts as cl
import small_sample_reference as sr
import theta_information_reference as tr

LD = sr.LD


@pytest.fixture(scope="module")
def refs(orc):
    """key -> (D, long-double reference, scales), computed once"""
    out = {}
    for key in sr.KEYS:
        c = sr.case(key)
        D = np.asarray(orc.gen_D(c["cov"], c["data"], c["eff_range"], c["theta"], chol=False))
        out[key] = (D, sr.reference(c, D), sr.scales(c, D))
    return out


def _dense(c, th):
    mats = []
    for b in cl.from_wire(c["cov"], c["data"]):
        D = cl.block_matrix(b, th, LD)[0]
        mats.append(D * np.eye(b[0], dtype=LD) if cl.kind(b) == "diag" else D)
    return cl.block_diag(mats)


@pytest.mark.parametrize("key", ["stepped_wedge_7x8x3", "wide_41", "geo150", "mixed"])
def test_analytic_d2D_against_second_central_differences(key):
    """every function of the table, the r != s cross term of a product of two terms, a shared parameter and the all-gr blocks:
    long-double central differences of cov_layouts.block_matrix with a relative step of 1e-4 (truncation 1e-8 relative, rounding
    1e-19 / 1e-8); 1e-6 guards formulas, not rounding, against the uncancelled size of the entry, |D| (|dl_r| |dl_s| + |d2l_r|): the
    second derivative in a pure scale parameter (sqexp, fexp t0) is 0.  A pair no block reads together has no entry and a zero
    difference"""
    c = sr.case(key)
    theta = c["theta"]
    got = sr.d2D(c, _dense(c, theta).astype(np.float64))
    size = sr.d2D(c, _dense(c, theta).astype(np.float64), absolute=True)
    R = theta.size

    def at(shift):
        th = theta.astype(LD).copy()
        for r, h in shift:
            th[r] += h
        return _dense(c, th.astype(np.float64)), th.astype(np.float64).astype(LD)

    for r in range(R):
        for s in range(r + 1):
            hr, hs = LD(theta[r]) * LD(1e-4), LD(theta[s]) * LD(1e-4)
            if r == s:
                (up, tu), (md, tm), (dn, td) = at([(r, hr)]), at([]), at([(r, -hr)])
                h1, h2 = tu[r] - tm[r], tm[r] - td[r]
                fd_ = 2 * (h2 * up - (h1 + h2) * md + h1 * dn) / (h1 * h2 * (h1 + h2))
            else:
                pp, pm, mp, mm = at([(r, hr), (s, hs)]), at([(r, hr), (s, -hs)]), at([(r, -hr), (s, hs)]), at([(r, -hr), (s, -hs)])
                fd_ = (pp[0] - pm[0] - mp[0] + mm[0]) / ((pp[1][r] - mm[1][r]) * (pp[1][s] - mm[1][s]))
            if (r, s) not in got:
                assert not np.any(fd_), (key, r, s)
                continue
            scale = float(np.max(size[(r, s)]))
            assert scale > 0, (key, r, s)
            err = float(np.max(np.abs(got[(r, s)] - fd_)) / scale)
            print("%s d2/dtheta%d dtheta%d: relative difference %.2e" % (key, r, s, err))
            assert err <= 1e-6, (key, r, s, err)


@pytest.mark.parametrize("key", ["stepped_wedge_7x8x3", "family-gaussian-identity", "geo150"])
def test_P_is_the_derivative_of_the_information(key, refs, orc):
    """d Phi / d theta_r = -Phi P_r Phi, Phi = (X' Sigma^-1 X)^-1: central differences of Phi(theta) (and of Phi(sigma)) in
    long double, relative step 1e-6; 1e-8 guards the meaning and the sign, not rounding"""
    import information_reference as ir
    c = sr.case(key)
    D, ref, _ = refs[key]
    inv = lambda a: np.linalg.inv(a.astype(np.float64)).astype(LD)     # P <= 9: float64 inverse, error 1e-13

    def phi(theta, var_par):
        cc = dict(c, theta=theta, var_par=var_par)
        Dt = np.asarray(orc.gen_D(c["cov"], c["data"], c["eff_range"], theta, chol=False))
        return inv(ir.reference(cc, Dt))

    Phi = phi(c["theta"], c["var_par"])
    for r in range(sr.rows(c)):
        th_u, th_d, sg_u, sg_d = c["theta"].copy(), c["theta"].copy(), c["var_par"], c["var_par"]
        if r < c["theta"].size:
            h = c["theta"][r] * 1e-6
            th_u[r] += h; th_d[r] -= h
            step = LD(th_u[r]) - LD(th_d[r])
        else:
            sg_u, sg_d = c["var_par"] * (1 + 1e-6), c["var_par"] * (1 - 1e-6)
            step = LD(sg_u) - LD(sg_d)
        fd_ = (phi(th_u, sg_u) - phi(th_d, sg_d)) / step
        want = -(Phi @ ref["P"][r] @ Phi)
        err = float(np.max(np.abs(want - fd_)) / np.max(np.abs(fd_)))
        print("%s dPhi/d%s: relative difference %.2e" % (key, sr.names(c)[r], err))
        assert err <= 1e-6, (key, r, err)


def test_twin_against_long_double_gives_the_constant(refs):
    worst, where = 0.0, None
    for key in sr.KEYS:
        D, ref, sc = refs[key]
        br = sr.block_ratios(sr.twin(sr.case(key), D), ref, sc)
        at = max(br, key=br.get)
        print("%-26s twin ratio %8.3f at %s   (P = %d, %d parameters)" % (key, br[at], at, ref["P"].shape[1], ref["P"].shape[0]))
        if br[at] > worst:
            worst, where = br[at], key
    print("worst twin ratio %.3f at %s; TWIN_RATIO %.1f, C_SS %.1f" % (worst, where, sr.TWIN_RATIO, sr.C_SS))
    assert worst <= sr.TWIN_RATIO, (worst, where)
    assert np.ceil(worst) == sr.TWIN_RATIO, "TWIN_RATIO is not the measured value rounded up: %.3f at %s" % (worst, where)
    assert sr.C_SS == 8 * sr.TWIN_RATIO


def test_host_formula_against_long_double(refs):
    worst, where = 0.0, None
    for key in sr.KEYS:
        D, ref, sc = refs[key]
        r = sr.ratio(sr.host_formula(sr.case(key), D), ref, sc)
        print("%-26s host formula ratio %.3f" % (key, r))
        if r > worst:
            worst, where = r, key
    print("worst host ratio %.3f at %s; HOST_RATIO %.1f" % (worst, where, sr.HOST_RATIO))
    assert worst <= sr.HOST_RATIO and np.ceil(worst) == sr.HOST_RATIO, (worst, where)


def test_reference_symmetries_and_structural_zeros(refs):
    for key in sr.KEYS:
        c = sr.case(key)
        _, ref, sc = refs[key]
        no, R = sr.rows(c), c["theta"].size
        assert ref["P"].shape[0] == no and ref["Q"].shape[:2] == (no, no) and ref["R"].shape[:2] == (no, no)
        tol = lambda m: 1e-15 * float(np.max(np.abs(m))) + 1e-300
        for r in range(no):
            assert np.max(np.abs(ref["P"][r] - ref["P"][r].T)) <= tol(ref["P"][r])
            for s in range(no):
                assert np.max(np.abs(ref["Q"][r, s] - ref["Q"][s, r].T)) <= tol(ref["Q"][r, s])
                assert np.array_equal(ref["R"][r, s], ref["R"][s, r])
                if sc["R"][r, s] == 0:                                 # (a pure scale parameter has R_rr = 0 with S > 0: geo, t0)
                    assert not np.any(ref["R"][r, s]), (key, r, s)
        if sr.sigma_row(c):
            assert not np.any(ref["R"][:R, R]) and np.any(ref["R"][R, R])


@pytest.mark.parametrize("key", ["stepped_wedge_7x8x3", "family-gaussian-identity", "wide_41"])
def test_one_row_kenward_roger_is_satterthwaite(key, refs):
    """m of Kenward & Roger for the contrast e_k equals 2 Phi_kk^2 / (g_k' W g_k) and lambda equals 1"""
    import information_reference as ir
    c = sr.case(key)
    D, ref, _ = refs[key]
    info = ir.reference(c, D).astype(np.float64)
    tinfo = tr.reference(c, D).astype(np.float64)
    Pm, Qm, Rm = (ref[k].astype(np.float64) for k in ("P", "Q", "R"))
    out = {t: sr.kr(info, tinfo, Pm, Qm, Rm, t) for t in sr.TYPES}
    for k in range(min(info.shape[0], 5)):
        m, lam = sr.kr_one_row(info, tinfo, Pm, k)
        assert abs(m - out["sat"]["dof"][k]) <= 1e-8 * m and abs(lam - 1) <= 1e-8, (key, k, m, lam)
    assert np.array_equal(out["KR"]["dof"], out["sat"]["dof"]) and np.array_equal(out["KR2"]["dof"], out["sat"]["dof"])
    assert np.array_equal(out["sat"]["vcov"], out["sat"]["vcov_unadjusted"])
    assert np.all(out["sat"]["dof"] > 0) and np.all(np.diag(out["KR"]["vcov"]) > 0)
    assert not np.array_equal(out["KR"]["vcov"], out["KR2"]["vcov"])
    with pytest.raises(ValueError):
        sr.kr(info, tinfo, Pm, Qm, Rm, "kr")


def test_cases_are_what_the_gpu_test_says_they_are():
    assert len(sr.KEYS) == 15 and sr.KEYS[:14] == tr.KEYS
    for key in sr.KEYS:
        P = sr.case(key)["X"].shape[1]
        assert (P == 1) if key == "mixed" else (P >= 2), (key, P)
    assert sr.case("wide_41_p71")["X"].shape[1] == 71 and sr.case("wide_41_p71")["Z"].shape[1] == 123
    assert sr.case("geo300")["X"].shape == (300, 3) and sr.rows(sr.case("geo300")) == 3
    assert sorted(sr.COMPONENT_KEYS + sr.DENSE_KEYS) == sorted(sr.KEYS)
