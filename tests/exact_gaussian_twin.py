"""numpy float64 restatement of the exact conditional draws for gaussian / identity models (csrc/hmc_exact.h) -- a helper
module, not a test.

    v | y ~ N(mu*, M^-1),  M = I + (ZL)' ZL / sigma^2,  M mu* = b = (ZL)' (y - X beta) / sigma^2
    U = L R^-T (R^-1 b 1' + z),  R = chol(M) (lower),  z the Q x ncols standard normals

z for a given (seed, chain_offset, iter_idx, C, d) comes from the oracle's normal() with tag 16 iter_idx + 8, addressed
(element q, chain_offset + chain(j), draw(j)) with the column layout the HMC draws have: C > 1: column j = chain * d + draw;
C = 1: chain 0, draw j (d + 1 columns).

SHAPES are the designs the GPU test runs (the panel logic of the blocked solves is 128 wide); COLUMNS the (chains, nsamp)
pairs.  test_exact_gaussian_cpu.py pins this module against an extended-precision evaluation at every one of them."""
import numpy as np

from glmmrmcml_amd import synth


def dense_z_design(n=330, Q=200, seed=33):
    """a dense non-identity Z the way test_gpu_hmc.py builds its dense-Z cases (the columns of a Householder reflector),
    here n x Q with n > Q"""
    d = synth.geospatial(Q, seed=seed)
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n); v /= np.linalg.norm(v)
    H = np.eye(n) - 2.0 * np.outer(v, v)
    d["Z"] = np.asfortranarray(H[:, :Q])
    d["X"] = np.ones((n, 1), order="F")
    D = synth._fexp_D(np.c_[d["data"][:Q], d["data"][Q:]], d["theta"])
    d["y"] = d["beta"][0] + d["Z"] @ (np.linalg.cholesky(D) @ rng.standard_normal(Q)) + d["sigma"] * rng.standard_normal(n)
    d["n"] = n
    return d


SHAPES = {
    "one partial panel (40)": lambda: synth.geospatial(40),
    "exactly one panel (128)": lambda: synth.geospatial(128),
    "one panel plus one row (129)": lambda: synth.geospatial(129, sigma=0.5),
    "three panels, ragged last (300)": lambda: synth.geospatial(300),
    "three panels, sigma 0.2 (300)": lambda: synth.geospatial(300, sigma=0.2),
    "dense Z 330 x 200": dense_z_design,
}
COLUMNS = ((1, 3), (40, 80), (130, 130))      # (chains, nsamp): 4 columns, 80, 130 (past one 128-column tile)


def layout(chains, nsamp):
    """(C, draws per chain, columns) of a sampler call"""
    C = max(int(chains), 1)
    d = nsamp if C == 1 else -(-nsamp // C)
    return C, d, (d + 1 if C == 1 else C * d)


def normals(orc, Q, seed, chains, nsamp, chain_offset=0, iter_idx=0):
    C, d, ncols = layout(chains, nsamp)
    z = np.empty((Q, ncols), order="F")
    tag = 16 * iter_idx + 8
    for j in range(ncols):
        chain, draw = (j // d, j % d) if C > 1 else (0, j)
        for q in range(Q):
            z[q, j] = orc.normal(seed, q, chain_offset + chain, draw, tag)
    return z


def system(Z, L, X, y, beta, sigma, dtype=np.float64):
    """(M, b, ZL) in the given precision"""
    Z, L, X, y, beta = (np.asarray(a, dtype=dtype) for a in (Z, L, X, y, beta))
    s2 = dtype(sigma) * dtype(sigma)
    ZL = Z @ L
    M = np.eye(L.shape[0], dtype=dtype) + (ZL.T @ ZL) / s2
    b = ZL.T @ (y - X @ beta) / s2
    return M, b, ZL


def twin(Z, L, X, y, beta, sigma, z):
    """-> (U, mu*) in float64"""
    M, b, _ = system(Z, L, X, y, beta, sigma)
    R = np.linalg.cholesky(M)
    w = np.linalg.solve(R, b)
    V = np.linalg.solve(R.T, w[:, None] + np.asarray(z, dtype=np.float64))
    mu = np.linalg.solve(R.T, w)
    return np.asarray(L, dtype=np.float64) @ V, mu


# ---- the same in extended precision: hand-rolled factor and solves (numpy has no LAPACK for longdouble) ----
def _chol_ld(M):
    n = M.shape[0]
    R = np.zeros_like(M)
    for j in range(n):
        dj = M[j, j] - R[j, :j] @ R[j, :j]
        R[j, j] = np.sqrt(dj)
        if j + 1 < n:
            R[j + 1:, j] = (M[j + 1:, j] - R[j + 1:, :j] @ R[j, :j]) / R[j, j]
    return R


def _fwd_ld(R, B):
    X = np.array(B, dtype=R.dtype)
    for i in range(R.shape[0]):
        X[i] = (X[i] - R[i, :i] @ X[:i]) / R[i, i]
    return X


def _bwd_t_ld(R, B):
    """R' X = B"""
    X = np.array(B, dtype=R.dtype)
    for i in range(R.shape[0] - 1, -1, -1):
        X[i] = (X[i] - R[i + 1:, i] @ X[i + 1:]) / R[i, i]
    return X


def twin_extended(Z, L, X, y, beta, sigma, z):
    ld = np.longdouble
    M, b, _ = system(Z, L, X, y, beta, sigma, dtype=ld)
    R = _chol_ld(M)
    w = _fwd_ld(R, b)
    V = _bwd_t_ld(R, w[:, None] + np.asarray(z, dtype=ld))
    mu = _bwd_t_ld(R, w)
    return np.asarray(L, dtype=ld) @ V, mu
