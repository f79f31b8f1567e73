"""The reference of the GPU Cholesky / solve tests, checked on the CPU (no GPU, no library call): the closed form of family
S, the float64 twin of the library's algorithm against the componentwise bounds on every matrix the GPU tests use, the
measured constant of family F, and the power of the checks against two structural mutations of the twin."""
import numpy as np
import pytest

import chol_reference as cr
import cov_layouts as cl

LD = np.longdouble


@pytest.mark.parametrize("n", [1, 2, 17, 129, 300])
def test_closed_form_of_S_is_the_long_double_factor(n):
    """L_ij = s_i s_j rho^(i - j) c_j against cov_layouts.cholesky in long double: the entries of A are exact powers of two, so
    the two differ by the rounding of the long-double factorisation alone, 2^-64 kappa_2 (n + 1) max|L| (kappa_2 <= 9)"""
    A = cr.family_S(n)
    L = cl.cholesky(A.astype(LD))
    Lc = cr.closed_S(n, dtype=LD)
    assert np.abs(L - Lc).max() <= LD(2.0) ** -64 * 9 * (n + 1) * np.abs(Lc).max()
    assert np.array_equal(cr.closed_S(n), Lc.astype(np.float64))
    assert np.linalg.cond(A) <= 9.0


def test_check_rows():
    assert np.array_equal(cr.check_rows(520), np.arange(520))
    r = set(cr.check_rows(2200).tolist())
    assert {127, 128, 1023, 1024, 2047, 2048, 2175, 2176, 2199} <= r and len(r) <= 2 * 17 + 1 + 32
    assert np.array_equal(cr.check_rows(2200), cr.check_rows(2200))


# ---------------------------------------------------------------------------------------------- the twin on the GPU tests' matrices
def _direct_cases():
    for n in cr.DIRECT_SIZES:
        yield n, max(cr.DIRECT_M + (cr.DIRECT_MORE_M if n in cr.DIRECT_MORE_N else ()))


@pytest.mark.parametrize("family", ["W", "S"])
def test_twin_within_a_quarter_of_the_bound_direct(family):
    """families W and S at every size of tests/test_gpu_chol_solve.py, the widest right-hand side of each size (its leading
    columns are the narrower ones' shapes; every column is solved on its own): each ratio to the C = 1 bound is at most
    0.25 C = 0.5.  Measured, worst over n >= 15 (each at n = 15 .. 17 and falling with n; at n = 520: 0.007 / 0.005 / 0.021 / 0.003):
    W factor 0.116, forward 0.146, transposed 0.200, potrs 0.106; S 0.049, 0.090, 0.127, 0.052.

    n = 1 and n = 2 are held to C itself: there the bound counts one or two roundings and the algorithm commits exactly
    those -- l = fl(sqrt(a)) gives |a - l^2| up to 2 u l^2 = the whole (n + 1) u |L||L'| at C = 1 (0.60 measured), and
    x = fl(fl(1 / l) b) gives |l x - b| up to 2 u |l||x| = the whole n u |L||X| at C = 2 (1.11 measured at C = 1) -- so there
    is no sum of many roundings whose typical size could stay a factor four under its worst case."""
    worst = {}
    for n, m in _direct_cases():
        A = cr.family_W(n) if family == "W" else cr.family_S(n)
        B = cr.rhs(n, m)
        t = cr.twin_all(A, B)
        for key, (w, at) in cr.all_ratios(A, B, t["L"], t["X"], t["Y"], t["Z"]).items():
            assert w <= (0.25 if n >= 15 else 1.0) * cr.C_WS, (family, n, m, key, w, at)
            worst[key] = max(worst.get(key, 0.0), w)
    print(family, worst)


def _ws_cases():
    for d in cr.WS_EAGER_D:
        yield d, max(cr.WS_EAGER_M), cr.thetas_S(1)
    for d in cr.WS_GRAPH_D:
        yield d, cr.WS_M, cr.thetas_S(2)
    for k, d in cr.WS_BATCH:
        yield d, cr.WS_M, cr.thetas_S(k)


def test_twin_within_a_quarter_of_the_bound_workspace_S():
    """the gr x ar1 blocks of tests/test_gpu_mvn_workspace.py at every (sigma, rho) those tests evaluate, with the sample rows
    carried below the matrix as the library carries them (measured at d = 33, the worst size: 0.023 for the factor, 0.044 for the rows)"""
    seen = set()
    for d, m, thetas in _ws_cases():
        for th in thetas:
            if (d, m, tuple(th)) in seen:
                continue
            seen.add((d, m, tuple(th)))
            D, bb = cr.build_D(cr.block_S(d), th)
            u = cr.samples(d, m)
            L, X, _ = cr.twin_potrf(D, extra=u.T)
            wf, at = cr.factor_ratio(D, L)
            assert wf <= 0.25 * cr.C_WS, (d, th, wf, at)
            wr, at = cr.rows_ratio(L, X, u.T)
            assert wr <= 0.25 * cr.C_WS, (d, th, wr, at)


def test_family_F_constant():
    """the twin's worst ratio on the fexp0 block over every range the GPU tests evaluate is the number chol_reference states,
    and C_F follows from it as max(2, 4 x ratio) and stays below 16"""
    worst = 0.0
    for th in cr.F_THETAS:
        D, _ = cr.build_D(cr.block_F(), th)
        assert np.linalg.cond(D) < 1e4
        u = cr.samples(300, cr.WS_M)
        L, X, _ = cr.twin_potrf(D, extra=u.T)
        worst = max(worst, cr.factor_ratio(D, L)[0], cr.rows_ratio(L, X, u.T)[0])
    print("family F: worst twin ratio", worst)
    assert 0.5 * cr.F_TWIN_RATIO <= worst <= cr.F_TWIN_RATIO
    assert cr.C_F == max(2.0, 4 * cr.F_TWIN_RATIO) and cr.C_F <= 16


# ---------------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("n,step,slice_", [(300, 0, 3), (520, 2, 7), (1300, 8, 0)])
def test_dropped_k_slice_breaks_the_factor_bound(n, step, slice_):
    """one 16-wide K slice left out of ONE trailing update: the residual exceeds the C = 2 bound at least 100 times"""
    A = cr.family_W(n)
    good, _, _ = cr.twin_potrf(A)
    bad, _, _ = cr.twin_potrf(A, drop=(step, slice_))
    assert cr.factor_ratio(A, good)[0] <= 0.25 * cr.C_WS
    w, at = cr.factor_ratio(A, bad)
    assert w >= 100 * cr.C_WS, (w, at)
    assert at[0] >= (step + 1) * cr.NB                  # the element named lies in the trailing matrix of that step


@pytest.mark.parametrize("n,k", [(300, 128), (520, 384)])
def test_skipped_panel_update_breaks_the_transposed_solve_bound(n, k):
    """the transposed solve without the rows-above update of one panel"""
    A = cr.family_W(n)
    B = cr.rhs(n, 3)
    L, _, invs = cr.twin_potrf(A)
    assert cr.trans_ratio(L, cr.twin_trans(L, invs, B), B)[0] <= 0.25 * cr.C_WS
    w, at = cr.trans_ratio(L, cr.twin_trans(L, invs, B, skip=k), B)
    assert w >= 100 * cr.C_WS, (w, at)
    assert at[0] < k                                    # ... in a row that update should have reached
