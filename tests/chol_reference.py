"""Element-by-element reference for the blocked Cholesky factorisation and its triangular solves (csrc/chol.hip
potrf_blocked / potrf_graphed, trsm_left_lower, trsm_left_lower_trans, potrs_lower_vec).

Nothing here calls the library.  A computed factor or solution is judged by its COMPONENTWISE BACKWARD ERROR, evaluated in
long double (u = 2^-53 is the unit roundoff of the float64 under test):

    factor             |A - L L'|_ij   <= C (n + 1) u (|L| |L'|)_ij          i >= j    (Higham, Accuracy and Stability, Thm 10.3)
    forward solve      |L X - B|       <= C n u |L| |X|                                (Thm 8.5)
    transposed solve   |L' Y - B|      <= C n u |L'| |Y|                               (Thm 8.5)
    potrs              |L L' Z - B|    <= C n u (2 + C n u) |L| |L'| |Z|               (two-sided, derived at potrs_ratio)

C = 1 is the textbook constant of the substitution algorithms for any order of summation.  The library multiplies panels by
explicitly inverted 128-wide diagonal blocks, which adds a term proportional to kappa_2(L_kk) <= sqrt(kappa_2(A)) -- measured
on sqexp blocks (tests/illcond_cases.py, the twin with the kernel's own leaf, twin_leaf16): the factor's ratio to the C = 1 bound
is 0.42 at kappa_2(A) = 3e6, 2.0 at 2e9 and 15 at 1e12 (device: 0.33, 1.2, 17.6), a transposed solve's 1.2, 19 and 120
(device: 0.7, 13.6, 55); the bounds up there carry a constant per rung of kappa --;
families W and S (kappa_2(A) <= 9, kappa_2(L_kk) <= 3) are held to C = 2; `twin_potrf` and the twin solves below restate the library's
algorithm in float64 numpy, and tests/test_chol_reference_cpu.py asserts that the twin stays at or below a quarter of every
bound on every matrix the GPU tests use.  Every ratio function returns (worst ratio to the C = 1 bound, where), so a failure
names the element.

Every bound also carries n * 2^-1074 absolute: the standard model fl(x op y) = (x op y)(1 + delta) holds barring underflow,
and the AR1 blocks with rho = 0.5 have entries 2^-|i - j| that leave the normal range of float64 at |i - j| > 1022; with
gradual underflow each operation adds at most half the smallest subnormal.

Families (all seeded):
    W   B B'/n + I, B standard normal                           kappa_2 = 4.7 .. 5.1 for n = 17 .. 1300
    S   s_i s_j rho^|i - j|, rho = 0.5, random signs s          kappa_2 <= 9; factor known in closed form (closed_S)
    F   one fexp0 block, range 0.1, 300 uniform points in the unit square, built through cov_layouts
        measured (test_chol_reference_cpu.py): the twin's worst ratio to the C = 1 bound over the parameter values F_THETAS
        is 0.080 (factor or solved sample rows, whichever is worse), so C_F = max(2, 4 x 0.08) = 2
"""
import functools

import numpy as np

import cov_layouts as cl

LD = np.longdouble
U = LD(2.0) ** -53
TINY = LD(2.0) ** -1074
NB = 128             # panel width of the library (CHOL_NB)
SPW = 1024           # super-panel width of a batch
FULL_MAX = 520       # above this the factor residual is evaluated on check_rows only

C_WS = 2.0           # families W and S
F_TWIN_RATIO = 0.08  # measured, asserted by test_chol_reference_cpu.py (worst of factor / solved rows over F_THETAS, rounded up)
C_F = max(2.0, 4 * F_TWIN_RATIO)

RHO = 0.5

# what the GPU tests run (tests/test_gpu_chol_solve.py, tests/test_gpu_mvn_workspace.py); the CPU test walks the same lists
DIRECT_SIZES = (1, 2, 15, 16, 17, 33, 127, 128, 129, 130, 144, 145, 255, 256, 257, 300, 385, 520)
DIRECT_M = (1, 65)
DIRECT_MORE_N = (129, 257, 300)
DIRECT_MORE_M = (3, 64, 130)
WS_EAGER_D = (33, 48, 129, 255)
WS_EAGER_M = (1, 17, 130)
WS_GRAPH_D = (300, 1153)
WS_BATCH = ((2, 129), (8, 129), (2, 300), (8, 300), (3, 1153), (3, 2200))      # (candidates, d)
WS_M = 17


# ------------------------------------------------------------------------------------------------ families
def family_W(n, seed=None):
    rng = np.random.default_rng(7000 + n if seed is None else seed)
    B = rng.standard_normal((n, n))
    A = B @ B.T / n + np.eye(n)
    return (A + A.T) / 2


def signs_S(n, seed=None):
    return np.random.default_rng(8000 + n if seed is None else seed).choice([-1.0, 1.0], size=n)


def family_S(n, seed=None, rho=RHO):
    s = signs_S(n, seed)
    k = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    return s[:, None] * s[None, :] * np.power(rho, k)


def closed_S(n, seed=None, rho=RHO, dtype=np.float64):
    """the factor of family_S: L_ij = s_i s_j rho^(i - j) c_j, c_0 = 1, c_j = sqrt(1 - rho^2)"""
    s = signs_S(n, seed).astype(dtype)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    c = np.full(n, np.sqrt(1 - dtype(rho) ** 2), dtype=dtype)
    c[0] = 1
    return np.where(i >= j, s[:, None] * s[None, :] * np.power(dtype(rho), np.maximum(i - j, 0).astype(dtype)) * c[None, :], 0)


def rhs(n, m, seed=None):
    return np.asfortranarray(np.random.default_rng(9000 + 131 * n + m if seed is None else seed).standard_normal((n, m)))


# ---- single-block layouts for the workspace tests
def block_S(d):
    """gr x ar1 on times 0 .. d-1: D = theta_0^2 theta_1^|i - j|"""
    return (d, [(cl.GR, np.ones((d, 1)), 0), (cl.AR1, np.arange(float(d))[:, None], 1)])


def thetas_S(k):
    """k candidate (sigma, rho), the first at rho = 0.5, the others better conditioned (kappa_2 = ((1 + rho) / (1 - rho))^2 <= 9)"""
    return np.array([[1.0 + 0.1 * j, RHO - 0.03 * j] for j in range(k)])


@functools.lru_cache(maxsize=None)
def block_F():
    return (300, [(cl.FEXP0, np.random.default_rng(20250401).random((300, 2)), 0)])


F_THETAS = np.array([[0.1 * (1 - 0.03 * j)] for j in range(8)])      # shorter ranges: no worse conditioned than the first


def build_D(block, theta):
    """(D, bound): the block's matrix from cov_layouts.block_matrix in float64, and that module's entrywise bound on another
    float64 evaluation of the same table, 2^-52 (8 + 2 sum_k |a_k|) |D_ij| (cov_layouts.dense_definition)"""
    D, A, _ = cl.block_matrix(block, theta)
    return D, (2.0 ** -52 * (8 + 2 * A.astype(LD)) * np.abs(D.astype(LD)))


def samples(d, m, seed=None):
    return np.asfortranarray(np.random.default_rng(6000 + 17 * d + m if seed is None else seed).standard_normal((d, m)))


# ------------------------------------------------------------------------------------------------ the checks
def check_rows(n):
    """all rows up to FULL_MAX; above it the rows on either side of every 128-panel and 1024-super-panel edge, the last row
    and 32 seeded random rows"""
    if n <= FULL_MAX:
        return np.arange(n)
    r = {n - 1}
    for w in (NB, SPW):
        for e in range(w, n, w):
            r.update((e - 1, e))
    r.update(int(i) for i in np.random.default_rng(5000 + n).choice(n, 32, replace=False))
    return np.array(sorted(r))


def _absprod(a, b):
    """the product of two nonnegative long-double matrices that scales a BOUND.  Up to FULL_MAX in long double; above it in
    float64 (BLAS), whose result is within (n + 2) u < 1e-12 of the exact product in relative terms and is scaled down by
    that much, so the bound is never wider than the long-double one (products that underflow in float64 only lower it)"""
    if a.shape[-1] <= FULL_MAX:
        return a @ b
    return ((a.astype(np.float64) @ b.astype(np.float64)) * (1 - 1e-12)).astype(LD)


def _worst(ratio):
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def factor_ratio(A, L, build_bound=None):
    """worst |A - L L'|_ij / ((n + 1) u (|L| |L'|)_ij + build_bound_ij + n 2^-1074) over the checked rows i and all j <= i,
    and (i, j); only the lower triangle of L is read.  A NaN anywhere in it gives inf."""
    n = A.shape[0]
    Lq = np.tril(np.asarray(L)[:n, :n]).astype(LD)
    if not np.all(np.isfinite(Lq)):
        return np.inf, tuple(int(i) for i in np.argwhere(~np.isfinite(Lq))[0])
    aL = np.abs(Lq)
    Aq = np.asarray(A).astype(LD)
    rows = check_rows(n)
    if len(rows) == n:
        P, Q = Lq @ Lq.T, aL @ aL.T
    else:
        P = np.zeros((len(rows), n), dtype=LD)
        for r, i in enumerate(rows):                     # (L L')_ij, j <= i, reads columns 0 .. i only
            P[r, :i + 1] = Lq[:i + 1, :i + 1] @ Lq[i, :i + 1]
        Q = _absprod(aL[rows], aL.T)
    bound = (n + 1) * U * Q + n * TINY
    if build_bound is not None:
        bound = bound + np.asarray(build_bound)[rows]
    ratio = np.abs(Aq[rows] - P) / bound
    ratio[np.arange(n)[None, :] > rows[:, None]] = 0
    w, (r, j) = _worst(ratio)
    return w, (int(rows[r]), j)


def forward_ratio(L, X, B):
    """worst |L X - B| / (n u |L| |X| + n 2^-1074)"""
    n = L.shape[0]
    Lq, Xq = np.tril(L).astype(LD), np.asarray(X).astype(LD).reshape(n, -1)
    if not np.all(np.isfinite(Xq)):
        return np.inf, tuple(int(i) for i in np.argwhere(~np.isfinite(Xq))[0])
    R = np.abs(Lq @ Xq - np.asarray(B).astype(LD).reshape(n, -1))
    return _worst(R / (n * U * _absprod(np.abs(Lq), np.abs(Xq)) + n * TINY))


def trans_ratio(L, Y, B):
    """worst |L' Y - B| / (n u |L'| |Y| + n 2^-1074)"""
    n = L.shape[0]
    Lq, Yq = np.tril(L).astype(LD).T, np.asarray(Y).astype(LD).reshape(n, -1)
    if not np.all(np.isfinite(Yq)):
        return np.inf, tuple(int(i) for i in np.argwhere(~np.isfinite(Yq))[0])
    R = np.abs(Lq @ Yq - np.asarray(B).astype(LD).reshape(n, -1))
    return _worst(R / (n * U * _absprod(np.abs(Lq), np.abs(Yq)) + n * TINY))


def potrs_ratio(L, Z, B, C=1.0):
    """worst |L L' Z - B| / (n u (2 + C n u) |L| |L'| |Z| + n 2^-1074), the two-sided form.

    potrs computes x from L x = b, then z from L' z = x.  With the one-sided bounds, for the computed x and z,
        |L x - b| <= g |L| |x|,    |L' z - x| <= g |L'| |z|,    g = C n u.
    L L' z - b = L (L' z - x) + (L x - b), so |L L' z - b| <= g |L| |L'| |z| + g |L| |x|; the intermediate x is not
    returned, but x = L' z - (L' z - x) gives |x| <= (1 + g) |L'| |z|, hence
        |L L' z - b| <= g (2 + g) |L| |L'| |z|.
    The ratio returned is to that bound at the C given in the g of (2 + g) and C = 1 in the leading g, so that the caller
    compares it with C like every other ratio."""
    n = L.shape[0]
    Lq, Zq = np.tril(L).astype(LD), np.asarray(Z).astype(LD).reshape(n, -1)
    if not np.all(np.isfinite(Zq)):
        return np.inf, tuple(int(i) for i in np.argwhere(~np.isfinite(Zq))[0])
    R = np.abs(Lq @ (Lq.T @ Zq) - np.asarray(B).astype(LD).reshape(n, -1))
    g = n * U
    return _worst(R / (g * (2 + C * g) * (np.abs(Lq) @ (np.abs(Lq.T) @ np.abs(Zq))) + n * TINY))


def rows_ratio(L, X, Ut):
    """the solved sample rows of the mvn workspace, X (m x d) = U' inv(L)': worst |X L' - U'| / (d u |X| |L'| + d 2^-1074)"""
    w, (i, j) = forward_ratio(L, np.asarray(X).T, np.asarray(Ut).T)
    return w, (j, i)


def linv_ratio(Lkk, Xkk):
    """worst |L_kk X_kk - I| / (128 u |L_kk| |X_kk|) on the lower triangle"""
    nb = Lkk.shape[0]
    Lq, Xq = np.tril(Lkk).astype(LD), np.tril(Xkk).astype(LD)
    R = np.abs(Lq @ Xq - np.eye(nb, dtype=LD))
    bound = NB * U * (np.abs(Lq) @ np.abs(Xq))
    low = np.tril(np.ones((nb, nb), dtype=bool))
    return _worst(np.where(low, R, 0) / np.where(low, bound, 1))


# ------------------------------------------------------------------------------------------------ the float64 twin
def _leaf(Akk):
    """(L_kk, inv(L_kk)) in float64: unblocked factorisation, inverse by forward substitution on the identity"""
    Lkk = cl.cholesky(np.tril(Akk) + np.tril(Akk, -1).T)
    return Lkk, np.tril(cl.forward_sub(Lkk, np.eye(len(Lkk))))


def twin_leaf16(Akk, drop_term=None, wrong_tile=None):
    """(L_kk, inv(L_kk)) in float64 as k_potrf_leaf (csrc/chol.hip) computes them: right-looking steps 16 columns wide.
    Step t: the 16 x 16 diagonal tile is eliminated column by column, every row scaled by the RECIPROCAL pivot
    y = 1 / sqrt(pivot); the 16 rows of the identity ride along (their solution is X_tt, the diagonal tile of the
    inverse, whose diagonal is the reciprocal pivots) and so do the first 32 rows of the panel below -- these by
    substitution; the remaining panel rows are PRODUCTS with X_tt'; the trailing matrix is updated with K = 16.  Block
    row I of the inverse: X_IJ = -X_II (sum_{K = J}^{I - 1} L_IK X_KJ), J < I.  A ragged last tile is the kernel's
    identity-padded one (the padding meets zeros only).  Raises LinAlgError at a pivot that is not > 0, as the kernel
    flags it.

    Mutations for the power checks: drop_term = (I, J, K) leaves the term K out of that sum; wrong_tile = t multiplies
    the panel rows of step t (t >= 1) by the inverse tile of step t - 1."""
    n = len(Akk)
    S = np.tril(np.asarray(Akk, dtype=np.float64))
    X = np.zeros((n, n))
    nt = (n + 15) // 16
    for t in range(nt):
        kb, ke = 16 * t, min(16 * t + 16, n)
        w, pe = ke - kb, min(kb + 48, n)
        R = np.vstack([S[kb:pe, kb:ke], np.eye(w)])          # tile rows, ride-along panel rows, identity rows
        for c in range(w):
            if not R[c, c] > 0:
                raise np.linalg.LinAlgError("leaf: pivot %d is not positive" % (kb + c))
            l = R[:, c] * (1.0 / np.sqrt(R[c, c]))
            R[:, c] = l
            if c + 1 < w:
                R[:, c + 1:] -= l[:, None] * l[None, c + 1:w]
        S[kb:ke, kb:ke] = np.tril(R[:w])
        S[ke:pe, kb:ke] = R[w:pe - kb]
        Xtt = np.tril(R[pe - kb:].T)
        X[kb:ke, kb:ke] = Xtt
        if pe < n:
            Xp = X[kb - 16:kb, kb - 16:kb] if wrong_tile == t else Xtt
            S[pe:, kb:ke] = S[pe:, kb:ke] @ Xp.T
        if ke < n:
            P = S[ke:, kb:ke]
            S[ke:, ke:] -= P @ P.T
            S[ke:, ke:] = np.tril(S[ke:, ke:])
        for J in range(t):                                   # block row t of the inverse
            T = np.zeros((w, 16))
            for K in range(J, t):
                if drop_term != (t, J, K):
                    T += S[kb:ke, 16 * K:16 * K + 16] @ X[16 * K:16 * K + 16, 16 * J:16 * J + 16]
            X[kb:ke, 16 * J:16 * J + 16] = -(Xtt @ T)
    return S, X


def twin_potrf(A, extra=None, drop=None, leaf=None):
    """(L, X, invs): the library's algorithm in float64 numpy -- 128-wide panels; each diagonal block factorised and its
    factor inverted; the panel below (and the `extra` rows carried under the matrix, m x n) as a PRODUCT with that
    inverse; a SYRK update of the trailing matrix.  drop = (t, s): the trailing update of step t leaves out the
    16-wide slice s of its K = 128 (the mutation of the power check).  leaf: what factorises and inverts a diagonal
    block (default _leaf, textbook substitution; twin_leaf16 restates the kernel's own leaf)."""
    leaf = _leaf if leaf is None else leaf
    n = A.shape[0]
    m = 0 if extra is None else extra.shape[0]
    W = np.zeros((n + m, n))
    W[:n] = np.tril(A)
    if m:
        W[n:] = extra
    invs = []
    for t, k in enumerate(range(0, n, NB)):
        nb = min(NB, n - k)
        Lkk, inv = leaf(W[k:k + nb, k:k + nb])
        W[k:k + nb, k:k + nb] = Lkk
        invs.append(inv)
        if k + nb < n + m:
            P = W[k + nb:, k:k + nb] @ inv.T
            W[k + nb:, k:k + nb] = P
            if k + nb < n:
                keep = np.ones(nb, dtype=bool)
                if drop is not None and drop[0] == t:
                    keep[16 * drop[1]:16 * drop[1] + 16] = False
                W[k + nb:, k + nb:n] -= P[:, keep] @ P[:n - k - nb, keep].T
    return np.tril(W[:n]), W[n:].copy(), invs


def twin_forward(L, invs, B):
    """trsm_left_lower: panel by panel, the diagonal block against its inverse, then the rows below -= L21 X_k"""
    n = L.shape[0]
    X = np.array(B, dtype=np.float64).reshape(n, -1)
    for t, k in enumerate(range(0, n, NB)):
        nb = min(NB, n - k)
        X[k:k + nb] = invs[t] @ X[k:k + nb]
        if k + nb < n:
            X[k + nb:] -= L[k + nb:, k:k + nb] @ X[k:k + nb]
    return X


def twin_trans(L, invs, B, skip=None):
    """trsm_left_lower_trans: panels from the last to the first, the diagonal block against its inverse transposed, then the
    rows above -= R21' Y_k.  skip = k: the panel at row k leaves out that update (the mutation of the power check)."""
    n = L.shape[0]
    Y = np.array(B, dtype=np.float64).reshape(n, -1)
    for k in range((n - 1) // NB * NB, -1, -NB):
        nb = min(NB, n - k)
        Y[k:k + nb] = invs[k // NB].T @ Y[k:k + nb]
        if k > 0 and k != skip:
            Y[:k] -= L[k:k + nb, :k].T @ Y[k:k + nb]
    return Y


def twin_all(A, B):
    """factor and the three solves of the twin: dict(L, X, Y, Z, invs)"""
    L, _, invs = twin_potrf(A)
    X = twin_forward(L, invs, B)
    return dict(L=L, invs=invs, X=X, Y=twin_trans(L, invs, B), Z=twin_trans(L, invs, X))


def all_ratios(A, B, L, X, Y, Z, build_bound=None):
    """the four ratios (to the C = 1 bounds) with their places, keyed factor / forward / trans / potrs"""
    return dict(factor=factor_ratio(A, L, build_bound), forward=forward_ratio(L, X, B), trans=trans_ratio(L, Y, B),
                potrs=potrs_ratio(L, Z, B, C_WS))
