"""The score of mvn_ll on the named covariance layouts (tests/cov_layouts.py), from the definition: no call into the
oracle's C code or the library.

    value(theta) = sum_j w_j sum_b log N(u_bj; 0, D_b(theta))            (w_j = 1 / m without weights)
    d value / d theta_k = sum_b 1/2 sum_ij (d_k D_b)_ij H_b,ij
    H_b = A diag(w) A' - (sum w) inv(D_b),   A = inv(D_b) U_b

Every covariance function is a product of terms, and d(term)/dt = term * dlog with

    fn        d/dt[0]                 d/dt[1]
    1 gr      2/t0 (where d == 0; the term is 0 elsewhere)
    2 fexp0   d/t0^2
    3 ar1     d/t0
    4 sqexp   1/t0                    2 d^2/t1^3
    7 fexp    1/t0                    d/t1^2
    14 sqexp0 2 d^2/t0^3

so (d_k D)_ij = D_ij * dlog.  A parameter index shared by several terms and blocks collects all their contributions.

``reference`` evaluates this in ``np.longdouble`` (D itself built in float64 and then widened, exactly as
cov_layouts.definition_columns does, so that its central differences differentiate the same function); ``twin`` is the
same algorithm in float64.  Besides value and gradient both return

    mag_k = 1/2 sum_b sum_ij |d_k D_b|_ij (|A| diag(w) |A|' + (sum w) |inv(D_b)|)_ij

-- the gradient with every cancellation removed, the scale its rounding errors live on -- and kappa, the largest 2-norm
condition number of the blocks.  A float64 evaluation through a Cholesky factor is expected within
bound_k = 2^-52 * kappa * mag_k of the reference.

Measured (test_mvn_grad_reference_cpu.py, all four layouts x three thetas x m in {1, 17, 65}, with and without weights):
the float64 twin's largest error is 0.0101 bound_k and 2.22 units of 2^-52 mag_k without kappa, both on MIXED (EDGE32:
0.0014 and 0.56, TWO_LARGE_A: 0.0020 and 0.33, TWO_LARGE_B: 0.0011 and 0.28).
"""
import functools

import numpy as np

import cov_layouts as cl

LD = np.longdouble
MAX_COLUMNS = 130


def weights(m, seed=5):
    """m sample weights >= 0 with exact zeros among them (every third, where m > 1) that do not sum to 1"""
    w = np.random.default_rng(seed + m).uniform(0.2, 1.8, size=m)
    if m > 1:
        w[::3] = 0.0
    return w


def dlog_terms(block, theta, dtype):
    """[(parameter index, dlog matrix)] for every parameter of every term of the block, in `dtype`"""
    dim, terms = block
    th = np.asarray(theta, dtype=np.float64).astype(dtype)
    out = []
    for fn, x, pi in terms:
        d = cl._distance(np.asarray(x, dtype=np.float64).reshape(dim, -1), dtype)
        t = th[pi:]
        one = np.ones_like(d)
        if fn == cl.GR:
            out.append((pi, np.where(d == 0, 2 / t[0], 0 * t[0]) * one))
        elif fn == cl.FEXP0:
            out.append((pi, d / (t[0] * t[0])))
        elif fn == cl.AR1:
            out.append((pi, d / t[0]))
        elif fn == cl.SQEXP:
            out.append((pi, one / t[0]))
            out.append((pi + 1, 2 * d * d / (t[1] * t[1] * t[1])))
        elif fn == cl.FEXP:
            out.append((pi, one / t[0]))
            out.append((pi + 1, d / (t[1] * t[1])))
        elif fn == cl.SQEXP0:
            out.append((pi, 2 * d * d / (t[0] * t[0] * t[0])))
        else:
            raise ValueError("covariance function id %d is not in the table" % fn)
    return out


def back_sub(L, Y):
    """inv(L)' Y, row by row from the last"""
    A = np.zeros_like(Y)
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        A[i] = (Y[i] - (L[i + 1:, i, None] * A[i + 1:]).sum(0)) / L[i, i]
    return A


def block_parts(block, theta, U, dtype):
    """what one block contributes that does not depend on the weights: (D, log-determinant term, Y = inv(L) U, A = inv(D) U,
    inv(D), [(parameter, d_k D)]), all in `dtype`"""
    dim = block[0]
    D = cl.block_matrix(block, theta)[0].astype(dtype)              # built in float64, as the definition builds it
    L = cl.cholesky(D)
    Y = cl.forward_sub(L, U.astype(dtype))
    A = back_sub(L, Y)
    Dinv = back_sub(L, cl.forward_sub(L, np.eye(dim, dtype=dtype)))
    dD = [(p, D * dl) for p, dl in dlog_terms(block, theta, dtype)]
    const = -dtype(0.5) * dim * cl.LOG_2PI.astype(dtype) - np.log(np.diag(L)).sum()
    return D, const, Y, A, Dinv, dD


def score(blocks, theta, u, w=None, dtype=LD, parts=None):
    """(value, grad, mag, kappa) of the layout at theta on the columns of u (Q x m); w = None: 1 / m each"""
    u = np.asarray(u, dtype=np.float64)
    if u.ndim == 1:
        u = u[:, None]
    m = u.shape[1]
    w = (np.full(m, 1.0, dtype=dtype) / dtype(m)) if w is None else np.asarray(w, dtype=np.float64).astype(dtype)
    assert w.shape == (m,)
    sw = w.sum()
    npar = len(theta)
    value = dtype(0)
    grad = np.zeros(npar, dtype=dtype)
    mag = np.zeros(npar, dtype=dtype)
    kappa = 0.0
    s = 0
    for bi, block in enumerate(blocks):
        dim = block[0]
        D, const, Y, A, Dinv, dD = parts[bi] if parts is not None else block_parts(block, theta, u[s:s + dim], dtype)
        Y, A = Y[:, :m], A[:, :m]
        value += (w * (const - dtype(0.5) * (Y * Y).sum(0))).sum()
        H = (A * w) @ A.T - sw * Dinv
        Habs = (np.abs(A) * w) @ np.abs(A).T + sw * np.abs(Dinv)
        for p, d in dD:
            grad[p] += dtype(0.5) * (d * H).sum()
            mag[p] += dtype(0.5) * (np.abs(d) * Habs).sum()
        kappa = max(kappa, float(np.linalg.cond(D.astype(np.float64), 2)))
        s += dim
    assert s == u.shape[0], "u has %d rows, the blocks %d" % (u.shape[0], s)
    return value, grad, mag, kappa


@functools.lru_cache(maxsize=None)
def _parts(name, ti, long_double):
    """block_parts of every block of a named layout at thetas(name)[ti] on the first MAX_COLUMNS sample columns"""
    blocks, theta = cl.LAYOUTS[name][0], cl.thetas(name)[ti]
    u = cl.sample_matrix(name)[:, :min(MAX_COLUMNS, cl.COLUMNS[name])]
    out, s = [], 0
    for block in blocks:
        out.append(block_parts(block, theta, u[s:s + block[0]], LD if long_double else np.float64))
        s += block[0]
    return out


def _named(name, ti, m, w, long_double):
    blocks, theta = cl.LAYOUTS[name][0], cl.thetas(name)[ti]
    assert m <= min(MAX_COLUMNS, cl.COLUMNS[name])
    return score(blocks, theta, cl.sample_matrix(name)[:, :m], w, LD if long_double else np.float64,
                 parts=_parts(name, ti, long_double))


def reference(name, ti, m, weights=None):
    """(value, grad, mag, kappa) in np.longdouble on the first m sample columns of the named layout"""
    return _named(name, ti, m, weights, True)


def twin(name, ti, m, weights=None):
    """the same algorithm in float64 numpy"""
    return _named(name, ti, m, weights, False)
