"""The blocked Cholesky factorisation, its inverted diagonal blocks and the three triangular solves, element by element on
matrices of the test's choosing (glmmr_mcml_dbg_chol), and the transposed-A operand form of the GEMM the transposed solve
runs on (glmmr_mcml_dbg_dgemm_at).  Bounds, families and the float64 twin that calibrates them: tests/chol_reference.py.

What the sizes reach (128-wide panels, 16-wide tiles inside the leaf):
    1, 2, 15, 16, 17, 33, 127   the leaf alone, ragged in every way: one tile, a tile edge, several tiles with a ragged last one
    128                         the leaf alone, full
    129, 130                    one panel and a last panel of 1 or 2: the panel product and the update have K = 128, the last
                                diagonal solve K = 1 / 2 (register-staged kernel; K = 1 reads a pad row in the transposed solve)
    144, 145                    a last panel of K = 16 (the smallest the LDS-DMA kernel takes) and of 17 (odd, not a multiple of 16)
    255, 256, 257               the look-ahead threshold: 256 is the last size on one stream, 257 the first with the leaf forked
                                to the side stream, three panels
    300, 385, 520               three, four and five panels, ragged last ones (44, 1, 8)
Right-hand sides: m = 1 (what potrs and the exact draws' forward solve use) and 65 (one column past a 64-wide tile); 129, 257
and 300 also with 3, 64 and 130 columns (130: more than one 128-wide column tile).
"""
import numpy as np
import pytest

import chol_reference as cr
import cov_layouts as cl

pytestmark = pytest.mark.gpu

CASES = [(n, m) for n in cr.DIRECT_SIZES for m in cr.DIRECT_M] + [(n, m) for n in cr.DIRECT_MORE_N for m in cr.DIRECT_MORE_M]
_factor_cache = {}


@pytest.fixture(scope="module")
def ctx():
    """a context made from a covariance alone"""
    from glmmrmcml_amd import api
    cov, data = cl.layout([cr.block_S(40)])
    with api.Context(cov, data, np.zeros(cov.shape[0])) as c:
        yield c


def _matrix(family, n):
    return cr.family_W(n) if family == "W" else cr.family_S(n)


def _factor_ratio(A, L):
    """the factor residual, computed once per distinct factor (the same bits have the same residual)"""
    key = (A.shape[0], A.tobytes(), np.tril(L).tobytes())
    if key not in _factor_cache:
        _factor_cache.clear()
        _factor_cache[key] = cr.factor_ratio(A, L)
    return _factor_cache[key]


def _check_all(family, n, A, B, got, C=cr.C_WS):
    L = np.tril(got["A"])
    w, at = _factor_ratio(A, L)
    print("%s n=%d m=%d factor %.4f at %s" % (family, n, B.shape[1], w, at))
    assert w <= C, ("factor", family, n, w, at)
    for kind, fn in (("fwd", cr.forward_ratio), ("trans", cr.trans_ratio), ("potrs", lambda l, z, b: cr.potrs_ratio(l, z, b, C))):
        w, at = fn(L, got[kind], B)
        print("  %s %.4f at %s" % (kind, w, at))
        assert w <= C, (kind, family, n, B.shape[1], w, at)
    # the inverted diagonal blocks
    for k in range((n + cr.NB - 1) // cr.NB):
        nb = min(cr.NB, n - k * cr.NB)
        X = got["linv"][k]
        assert not np.any(np.triu(X, 1)), ("linv above the diagonal", family, n, k)
        assert not np.any(X[nb:]) and not np.any(X[:, nb:]), ("linv beyond n", family, n, k)
        w, at = cr.linv_ratio(L[k * cr.NB:k * cr.NB + nb, k * cr.NB:k * cr.NB + nb], X[:nb, :nb])
        print("  linv[%d] %.4f" % (k, w))
        assert w <= 2.0, ("linv", family, n, k, w, at)
    if family == "S":     # known answer: forward error <= kappa_2 x the backward error, kappa_2 <= 9
        Lc = cr.closed_S(n)
        err = np.abs(L - Lc)
        at = np.unravel_index(err.argmax(), err.shape)
        assert err[at] <= 2 * 9 * (n + 1) * 2.0 ** -53 * np.abs(Lc).max(), ("closed form", n, err[at], at)


@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("family", ["W", "S"])
def test_factor_and_solves(ctx, family, n, m):
    """factor residual, forward / transposed / potrs residuals, inverse blocks, the closed form of S; then the same input with
    the strict upper triangle NaN: the factorisation and both solves never read above the diagonal (the exact draws build
    the lower tiles of their matrix only), so every result keeps its bits"""
    A = _matrix(family, n)
    B = cr.rhs(n, m)
    got = ctx.dbg_chol(np.tril(A), B)
    _check_all(family, n, A, B, got)
    poisoned = np.tril(A)
    poisoned[np.triu_indices(n, 1)] = np.nan
    again = ctx.dbg_chol(poisoned, B)
    assert np.array_equal(np.tril(again["A"]), np.tril(got["A"])), "the factor changed with the upper triangle"
    for kind in ("fwd", "trans", "potrs", "linv"):
        assert np.array_equal(again[kind], got[kind]), (kind, "changed with the upper triangle")


def test_symmetric_input_gives_the_same_factor(ctx):
    """the full symmetric array, as gen_D's blocks are built, against the lower triangle alone"""
    for n in (129, 300):
        A = cr.family_W(n)
        B = cr.rhs(n, 3)
        a, b = ctx.dbg_chol(A, B), ctx.dbg_chol(np.tril(A), B)
        assert np.array_equal(np.tril(a["A"]), np.tril(b["A"]))
        for kind in ("fwd", "trans", "potrs"):
            assert np.array_equal(a[kind], b[kind])


def test_not_positive_definite_is_reported_and_the_context_survives(ctx):
    from glmmrmcml_amd import _lib
    n = 300
    A = cr.family_W(n)
    B = cr.rhs(n, 3)
    bad = A.copy()
    bad[200, 200] = -1.0
    with pytest.raises(_lib.McmlError) as e:
        ctx.dbg_chol(bad, B)
    assert e.value.code == -3
    _check_all("W", n, A, B, ctx.dbg_chol(np.tril(A), B))


# ------------------------------------------------------------------------------------------------ C = alpha A' B + beta C
AT_SHAPES = [(16, 16, 4), (5, 3, 1), (5, 3, 2), (161, 129, 17), (128, 65, 128), (333, 77, 127), (300, 130, 44), (640, 300, 128)]


def _operands(M, N, K, seed):
    """A (K2 x M), B (K2 x N) with the pad row of an odd K poisoned, and their clean K-row parts"""
    rng = np.random.default_rng(seed)
    K2 = K + (K & 1)
    A = rng.normal(size=(K2, M)); B = rng.normal(size=(K2, N))
    if K & 1:
        A[K] = np.nan; B[K] = np.nan
    return A, B, A[:K], B[:K]


@pytest.mark.parametrize("M,N,K", AT_SHAPES)
@pytest.mark.parametrize("tile", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0)])
def test_dgemm_at_matches_numpy(M, N, K, tile, alpha, beta):
    """every tile of launch_gemm_at; K = 1 and odd K with the pad row k = K of both operands NaN (dgemm_mfma.h: it is zeroed on
    the way to LDS); ragged M and N; the bound of test_gpu_dgemm.py"""
    from glmmrmcml_amd import api
    A, B, Ak, Bk = _operands(M, N, K, M * 7 + N * 3 + K)
    C0 = np.random.default_rng(K).normal(size=(M, N))
    got = api.dbg_dgemm_at(A, B, C0, K, alpha, beta, tile)
    want = alpha * (Ak.T @ Bk) + beta * C0
    bound = 1e-12 * (np.abs(Ak.T) @ np.abs(Bk) + np.abs(C0))
    err = np.abs(got - want)
    assert np.all(err <= bound), (np.unravel_index(np.nanargmax(np.where(np.isnan(err), np.inf, err)), err.shape), err.max())


@pytest.mark.parametrize("n", [48, 47])
@pytest.mark.parametrize("tile", [-1, 0, 1, 2, 3])
def test_dgemm_at_identity_catches_a_transposed_store(n, tile):
    from glmmrmcml_amd import api
    K2 = n + (n & 1)
    A = np.zeros((K2, n)); A[:n] = np.eye(n)
    B = np.zeros((K2, 40)); B[:n] = np.arange(n * 40, dtype=float).reshape(n, 40)
    if n & 1:
        A[n] = np.nan; B[n] = np.nan
    got = api.dbg_dgemm_at(A, B, np.zeros((n, 40)), n, 1.0, 0.0, tile)
    assert np.array_equal(got, B[:n])


@pytest.mark.parametrize("K", [128, 100, 37, 1])
@pytest.mark.parametrize("N", [1, 65, 130])
def test_dgemm_at_in_place_diagonal_block(K, N):
    """the diagonal-block product of trsm_left_lower_trans: C aliases B, M = K <= 128, tile 2 (one 128-row tile holds every
    row of B, so each workgroup has read its columns before it writes them)"""
    from glmmrmcml_amd import api
    A, B, Ak, Bk = _operands(K, N, K, 31 * K + N)
    Ak[:] = np.tril(Ak)                      # a transposed lower-triangular inverse, as in the solve
    want = Ak.T @ Bk
    bound = 1e-12 * (np.abs(Ak.T) @ np.abs(Bk))
    got = api.dbg_dgemm_at(A, B.copy(order="F"), None, K, 1.0, 0.0, 2)
    assert np.all(np.abs(got - want) <= bound)
