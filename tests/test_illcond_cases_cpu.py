"""tests/illcond_cases.py checked on the CPU (no GPU, no library call): the condition bands, the adequacy of the long-double
reference, the restated leaf against the textbook one where the answer is known, every twin within a quarter of the
bound the GPU tests use, the constants' derivation, and the power of the checks against two mutations of the leaf."""
import numpy as np
import pytest

import chol_reference as cr
import cov_layouts as cl
import illcond_cases as ic

LD = np.longdouble
HIGH = ("E9", "E11", "E12")


def test_condition_bands():
    """every case on every rung, and every candidate of the batches the GPU test spreads inside a rung"""
    for name, rung in ic.CASE_RUNGS:
        lo, hi = ic.BANDS[rung]
        k = ic.kappa_of(name, ic.theta(name, rung))
        print("%s %s kappa %.3g" % (name, rung, k))
        assert lo <= k <= hi, (name, rung, k)
        assert abs(k - ic.TWIN[(name, rung)][0]) <= 0.01 * k, (name, rung, k)
    for name in ("SQ300", "FE300", "MIX"):
        for rung in ic.RUNGS[name]:
            lo, hi = ic.BANDS[rung]
            for th in ic.candidates(name, rung, 8):
                assert lo <= ic.kappa_of(name, th) <= hi, (name, rung, th)
    assert ic.BANDS["E12"][1] <= 2e12
    for bi, rung in ic.MIX_BLOCK_RUNG.items():
        lo, hi = ic.BANDS[rung]
        assert lo <= np.linalg.cond(cl.block_matrix(ic.CASES["MIX"][bi], ic.theta("MIX", "E12"))[0], 2) <= hi


def test_constants_follow_the_recorded_twin_ratios():
    """C = max(floor, 4 x worst recorded ratio of the rung, two digits, rounded up); the docstring carries the tables"""
    for rung in ic.BANDS:
        C = ic.constants(rung)
        for i, kind in enumerate(ic.KINDS):
            worst = max([row[1 + i] for (n, r), row in ic.TWIN.items() if r == rung and row[1 + i] is not None] + [0.0])
            assert C[kind] >= ic.FLOORS[kind] and C[kind] >= 4 * worst
            assert C[kind] == ic.FLOORS[kind] or C[kind] <= 4 * worst * 1.1
    assert set(ic.TWIN) == set(ic.CASE_RUNGS)
    for (name, rung) in ic.TWIN:
        assert "%-6s %-4s" % (name, rung) in ic.__doc__
    print(ic._constants_table())


@pytest.mark.parametrize("name,rung", ic.CASE_RUNGS)
def test_reference_agrees_with_its_second_evaluation(name, rung):
    """value and gradient through the factor of D as it stands, and through D scaled to unit diagonal with its rows and
    columns reversed: the two agree to 1e-3 of the C = 1 bounds (no wider than any bound in use), so the reference's own
    error, kappa 2^-64, does not count"""
    m = max(ic.MS[name])
    for w in (None, ic.weights(m)):
        a, b = ic.ref_score(name, rung, m, w), ic.ref_score(name, rung, m, w, variant=1)
        rv = ic.value_ratio(b["value"], a)
        rg = ic.grad_ratios(b["grad"], a)[1]
        print("%s %s: second evaluation at %.2e (value), %.2e (gradient) of the bound" % (name, rung, rv, rg.max()))
        assert rv <= 1e-3 and rg.max() <= 1e-3, (name, rung, rv, rg)


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 127, 128])
@pytest.mark.parametrize("family", ["W", "S"])
def test_twin_leaf16_reproduces_the_textbook_leaf(family, n):
    """families W and S (kappa_2(A) <= 9, kappa_2(L) <= 3): two backward-stable factorisations differ by at most twice the
    forward error kappa_2 (n + 1) u max|L| (the bound test_gpu_chol_solve.py holds the closed form of S to), the inverses
    by twice that again, and on S the restated leaf meets the closed form"""
    A = cr.family_W(n) if family == "W" else cr.family_S(n)
    L0, X0 = cr._leaf(A)
    L1, X1 = cr.twin_leaf16(A)
    tol = 2 * 9 * (n + 1) * 2.0 ** -53
    assert not np.any(np.triu(L1, 1)) and not np.any(np.triu(X1, 1))
    assert np.abs(L1 - L0).max() <= tol * np.abs(L0).max()
    assert np.abs(X1 - X0).max() <= 2 * tol * np.abs(X0).max()
    if family == "S":
        assert np.abs(L1 - cr.closed_S(n)).max() <= tol * np.abs(L0).max()
    assert cr.factor_ratio(A, L1)[0] <= (0.25 if n >= 15 else 1.0) * cr.C_WS
    assert cr.linv_ratio(L1, X1)[0] <= 0.25 * 2.0 or n < 15


def test_existing_twin_keeps_its_bits():
    """twin_potrf without a leaf argument is the twin the existing constants were calibrated with"""
    A = cr.family_W(300)
    L, _, invs = cr.twin_potrf(A)
    L2, _, invs2 = cr.twin_potrf(A, leaf=cr._leaf)
    assert np.array_equal(L, L2) and all(np.array_equal(a, b) for a, b in zip(invs, invs2))


@pytest.mark.parametrize("name,rung", ic.CASE_RUNGS)
def test_twins_within_a_quarter_of_every_bound(name, rung):
    """each measured twin ratio is at most the recorded one, hence a quarter of the rung's constant; no |ref grad_k| is a
    cancellation residue (>= 1e3 x the twin's absolute error); and on E9 and above the relative gradient bound is at least
    1e6 times tighter than 2^-52 kappa mag_k (MIX: for the parameters of its E9 and E12 blocks; its other parameters belong
    to the gr terms and the E6 block)"""
    row, residue, tighter = ic.measure(name, rung)
    C = ic.constants(rung)
    print('    ("%s", "%s"): (%.2e, %s),' % (name, rung, row[0], ", ".join("None" if x is None else "%.3g" % x for x in row[1:])))
    print("    smallest |ref| / twin error %s, mag / |ref| %s" % (np.array2string(residue, precision=3), np.array2string(tighter, precision=3)))
    for kind, x, rec in zip(ic.KINDS, row[1:], ic.TWIN[(name, rung)][1:]):
        assert (x is None) == (rec is None), (name, rung, kind)
        if x is not None:
            assert x <= rec, (name, rung, kind, x, rec)
            assert x <= 0.25 * C[kind], (name, rung, kind, x, C[kind])
    assert residue.min() >= 1e3, (name, rung, residue)
    if rung in HIGH:
        t = tighter[[1, 4]] if name == "MIX" else tighter
        assert (t / C["grad"]).min() >= 1e6, (name, rung, tighter, C["grad"])


def test_mix_blocks_factor_twin():
    """gen_D(chol=True) on MIX: each dense block's twin factor within a quarter of the constant of the rung it sits on"""
    th = ic.theta("MIX", "E12")
    for bi, rung in ic.MIX_BLOCK_RUNG.items():
        D, bound = cr.build_D(ic.CASES["MIX"][bi], th)
        for A in (D, ic.perturbed(D, bound)):
            L, _, _ = ic.twin_factor(A)
            w, at = cr.factor_ratio(A, L)
            print("MIX block %d (%s): factor %.3g" % (bi, rung, w))
            assert w <= 0.25 * ic.constants(rung)["factor"], (bi, rung, w, at)


# ---------------------------------------------------------------------------------------------- power
def test_dropped_inverse_term_breaks_the_linv_bound():
    """SQ128 at E9: block row 5 of the inverse without the K = 3 term of its column tile 2"""
    A = ic.matrix("SQ128", "E9")
    C = ic.constants("E9")["linv"]
    L, X = cr.twin_leaf16(A)
    assert cr.linv_ratio(L, X)[0] <= 0.25 * C
    Lb, Xb = cr.twin_leaf16(A, drop_term=(5, 2, 3))
    assert np.array_equal(L, Lb)
    w, at = cr.linv_ratio(Lb, Xb)
    print("dropped term: linv ratio %.3g at %s" % (w, at))
    assert w > C and 80 <= at[0] < 96 and 32 <= at[1] < 48, (w, at)


def test_wrong_inverse_tile_breaks_the_factor_bound():
    """SQ128 at E9: the panel rows of step t multiplied by the inverse tile of step t - 1, for every step that has panel rows
    beyond the 32 that ride along.  A trailing matrix that is no longer positive definite counts as caught: the device
    would report -3 where the test expects a factor"""
    A = ic.matrix("SQ128", "E9")
    C = ic.constants("E9")["factor"]
    assert cr.factor_ratio(A, cr.twin_leaf16(A)[0])[0] <= 0.25 * C
    for t in (1, 2, 3, 4):
        try:
            w, at = cr.factor_ratio(A, cr.twin_leaf16(A, wrong_tile=t)[0])
        except np.linalg.LinAlgError:
            w, at = np.inf, None
        print("wrong tile at step %d: factor ratio %.3g at %s" % (t, w, at))
        assert w > C, (t, w, at)
