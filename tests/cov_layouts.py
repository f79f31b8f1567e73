"""Covariance layouts with more than one kind of block, and the definition of mvn_ll / genD on them.

A layout is a list of blocks ``(dim, [(fn, data, par_index), ...])``: the block's covariance is the product of its
terms, term k being function ``fn`` of the Euclidean distance between the rows of ``data`` (dim x nv), with its
parameters at ``theta[par_index:]``.  ``layout`` turns that into the (cov, data) wire format of csrc/covspec.h;
``definition`` evaluates it from the formula table in that header's comment -- every block built in numpy (float64),
factorised and solved in ``np.longdouble`` -- with no call into the oracle's C code or the library:

    1 gr     d==0 ? v*t^2 : 0        2 fexp0  v*exp(-d/t)
    3 ar1    v*t^d                   4 sqexp  v*t0*exp(-d^2/t1^2)
    7 fexp   v*t0*exp(-d/t1)        14 sqexp0 v*exp(-d^2/t^2)

Every distance is chosen so that each block's 2-norm condition number stays below 1e4 (test_cov_layouts_cpu.py
asserts it): sqexp / sqexp0 on jittered grids of spacing 0.1 with ranges about the spacing, AR1 parameters <= 0.8,
fexp / fexp0 with range 0.1 on uniform random points.
"""
import functools

import numpy as np

GR, FEXP0, AR1, SQEXP, FEXP, SQEXP0 = 1, 2, 3, 4, 7, 14
LD = np.longdouble
LOG_2PI = np.log(2 * np.arccos(LD(-1)))


# ---------------------------------------------------------------------------------------------- wire format
def layout(blocks):
    """(cov, data): cov int32 rows x 5 Fortran order = (block id, dim, function id, n variables, parameter index),
    data = every block's dim x (all its variables) matrix flattened column-major, concatenated"""
    rows, data = [], []
    for b, (dim, terms) in enumerate(blocks):
        for fn, x, pi in terms:
            x = np.asarray(x, dtype=np.float64).reshape(dim, -1)
            rows.append([b, dim, fn, x.shape[1], pi])
            data.append(x.ravel(order="F"))
    return np.array(rows, dtype=np.int32, order="F"), np.concatenate(data)


def from_wire(cov, data):
    """the inverse of `layout`: the (cov, data) wire format back as a list of blocks (dim, [(fn, x, par_index), ...])"""
    cov = np.asarray(cov)
    data = np.asarray(data, dtype=np.float64).ravel()
    blocks, r, off = [], 0, 0
    while r < cov.shape[0]:
        bid, dim, terms = cov[r, 0], int(cov[r, 1]), []
        while r < cov.shape[0] and cov[r, 0] == bid:
            nv = int(cov[r, 3])
            terms.append((int(cov[r, 2]), data[off:off + dim * nv].reshape(dim, nv, order="F"), int(cov[r, 4])))
            off += dim * nv
            r += 1
        blocks.append((dim, terms))
    return blocks


def starts(blocks):
    """first random-effect index of every block"""
    return [int(s) for s in np.cumsum([0] + [b[0] for b in blocks])[:-1]]


def total_dim(blocks):
    return int(sum(b[0] for b in blocks))


def kind(block):
    """the path mvn_setup sends a block down: "diag" (every term gr), "small" (dim <= 32), "large\""""
    dim, terms = block
    if all(fn == GR for fn, _, _ in terms):
        return "diag"
    return "small" if dim <= 32 else "large"


# ---------------------------------------------------------------------------------------------- the definition
def _distance(x, dtype):
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1).astype(dtype)
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))


def _term(fn, d, t):
    """(factor, |exponent argument|, whether the argument is a square) of one term of the product; t = theta[par_index:]"""
    if fn == GR:
        return np.where(d == 0, t[0] * t[0], 0 * t[0]), np.zeros_like(d), False
    if fn == FEXP0:
        return np.exp(-d / t[0]), d / t[0], False
    if fn == AR1:
        return np.power(t[0], d), d * np.abs(np.log(t[0])), False
    if fn == SQEXP:
        return t[0] * np.exp(-d * d / (t[1] * t[1])), d * d / (t[1] * t[1]), True
    if fn == FEXP:
        return t[0] * np.exp(-d / t[1]), d / t[1], False
    if fn == SQEXP0:
        return np.exp(-d * d / (t[0] * t[0])), d * d / (t[0] * t[0]), True
    raise ValueError("covariance function id %d is not in the table" % fn)


def block_matrix(block, theta, dtype=np.float64):
    """(D, A, A2) in `dtype` (float64: the definition; long double: its exact value to 64 bits): the block's covariance matrix; entry by entry, the sum over its terms of the
    magnitude of the exponent argument (d/t, d^2/t^2 or d |log rho|; 0 for gr); and the part of that sum that
    comes from the squared arguments d^2/t^2"""
    dim, terms = block
    theta = np.asarray(theta, dtype=np.float64).astype(dtype)
    D = np.ones((dim, dim), dtype=dtype)
    A = np.zeros((dim, dim), dtype=dtype)
    A2 = np.zeros((dim, dim), dtype=dtype)
    for fn, x, pi in terms:
        f, a, squared = _term(fn, _distance(np.asarray(x, dtype=np.float64).reshape(dim, -1), dtype), theta[pi:])
        D = D * f
        A = A + a
        if squared:
            A2 = A2 + a
    return D, A, A2


def cholesky(D):
    """lower Cholesky factor, column by column, in the precision of D"""
    n = D.shape[0]
    L = np.zeros_like(D)
    for j in range(n):
        d = D[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            raise np.linalg.LinAlgError("block is not positive definite at column %d" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (D[j + 1:, j] - (L[j + 1:, :j] * L[j, :j]).sum(1)) / L[j, j]
    return L


def forward_sub(L, U):
    """inv(L) U, row by row"""
    Y = np.zeros_like(U)
    for i in range(L.shape[0]):
        Y[i] = (U[i] - (L[i, :i, None] * Y[:i]).sum(0)) / L[i, i]
    return Y


def definition_columns(blocks, theta, u):
    """(Ds, Ls, ll): the blocks' covariance matrices (built in float64), their Cholesky factors (float64 roundings of
    the long-double ones) and ll[j] = sum_b log N(u_bj; 0, D_b) for every column j of u, in long double"""
    u = np.asarray(u, dtype=np.float64)
    if u.ndim == 1:
        u = u[:, None]
    u = u.astype(LD)
    ll = np.zeros(u.shape[1], dtype=LD)
    Ds, Ls, s = [], [], 0
    for block in blocks:
        dim = block[0]
        D = block_matrix(block, theta)[0]
        L = cholesky(D.astype(LD))
        Y = forward_sub(L, u[s:s + dim])
        ll += -LD(0.5) * dim * LOG_2PI - np.log(np.diag(L)).sum() - LD(0.5) * (Y * Y).sum(0)
        Ds.append(D); Ls.append(L.astype(np.float64))
        s += dim
    assert s == u.shape[0], "u has %d rows, the blocks %d" % (u.shape[0], s)
    return Ds, Ls, ll


def definition(blocks, theta, u):
    """(per-block dense matrices, (1/m) sum_b sum_j log N(u_bj; 0, D_b))"""
    Ds, _, ll = definition_columns(blocks, theta, u)
    return Ds, float(ll.sum() / len(ll))


def block_diag(mats):
    Q = sum(m.shape[0] for m in mats)
    out = np.zeros((Q, Q), dtype=mats[0].dtype)
    s = 0
    for m in mats:
        out[s:s + m.shape[0], s:s + m.shape[0]] = m
        s += m.shape[0]
    return out


def dense_definition(blocks, theta):
    """(D, bound, exact, derived) Q x Q: the definition's D (float64 numpy) with the entrywise bound on another
    float64 evaluation of the same table, and the long-double value of D with a bound on any float64 evaluation.

    bound = 2^-52 (8 + 2 sum_k |a_k|) |D_ij|: the rounding of each exponent argument magnified by exp / pow, plus a
    few ulps for the functions themselves and the products.

    derived = 2^-52 (8 + 2 sum_k |a_k| + 2.5 sum_{squared k} |a_k|) |D_ij|, against `exact`.  The table's expression
    for sqexp / sqexp0 squares the ROUNDED distance: x_i - x_j (u = 2^-53), its square (3u), the sum of two (4u),
    the square root (3u), dist * dist (7u), t * t (u), the quotient (9u) -- 4.5 units of 2^-52 on d^2/t^2 in the
    worst case against the exact value, where d/t and d |log rho| collect at most 2; 2.7 is the most seen on the
    named layouts, on far-apart points whose covariance is below 1e-30"""
    D = block_diag([block_matrix(b, theta)[0] for b in blocks])
    Dm, Am, A2m = zip(*(block_matrix(b, theta, LD) for b in blocks))
    E, A, A2 = block_diag(Dm), block_diag(Am), block_diag(A2m)
    scale = 2.0 ** -52 * np.abs(E)
    return D, ((8 + 2 * A) * scale).astype(np.float64), E.astype(np.float64), ((8 + 2 * A + 2.5 * A2) * scale).astype(np.float64)


# ---------------------------------------------------------------------------------------------- named layouts
def _grid(nx, ny, rng, spacing=0.1, jitter=0.02):
    """nx * ny points of a grid of the given spacing, each moved by up to +-jitter in both coordinates"""
    gx, gy = np.meshgrid(np.arange(nx) * spacing, np.arange(ny) * spacing, indexing="ij")
    xy = np.column_stack([gx.ravel(), gy.ravel()])
    return xy + rng.uniform(-jitter, jitter, size=xy.shape)


def _mixed():
    rng = np.random.default_rng(20250301)
    ones = lambda n, v=1.0: np.full((n, 1), v)
    blocks = [(1, [(GR, [[float(k + 1)]], 0)]) for k in range(3)]                         # 0, 1, 2: diagonal
    blocks.append((150, [(SQEXP, _grid(15, 10, rng), 3)]))                                # 3 (odd), > 128
    blocks.append((5, [(GR, ones(5, 2.0), 1), (AR1, np.arange(1.0, 6.0)[:, None], 2)]))   # 153
    blocks.append((33, [(FEXP0, rng.random((33, 2)), 5)]))                                # 158: the first large size
    blocks.append((32, [(GR, ones(32, 3.0), 1), (SQEXP0, _grid(8, 4, rng), 6)]))          # 191: the last small size
    blocks.append((3, [(GR, ones(3, 4.0), 0),                                             # 223: all gr, dim > 1
                       (GR, np.column_stack([np.full(3, 4.0), np.arange(1.0, 4.0)]), 1)]))
    blocks.append((7, [(FEXP0, np.sort(rng.random(7))[:, None] + 0.05 * np.arange(7)[:, None], 5)]))   # 226
    blocks.append((289, [(GR, ones(289, 5.0), 1), (FEXP, rng.random((289, 2)), 7),        # 233 (odd), > 2 * 128
                         (AR1, rng.uniform(0.0, 3.0, size=(289, 1)), 9)]))
    #                  gr    gr    rho   sqexp       fexp0 sqexp0 fexp       rho (289 block)
    theta = np.array([0.30, 0.45, 0.60, 0.25, 0.115, 0.10, 0.13, 0.35, 0.10, 0.70])
    return blocks, theta


def _two_large(order):
    rng = np.random.default_rng(20250302)
    sq = (300, [(SQEXP, _grid(20, 15, rng), 0)])
    ar = (161, [(GR, np.full((161, 1), 1.0), 2), (AR1, np.arange(1.0, 162.0)[:, None], 3)])
    theta = np.array([0.25, 0.115, 0.50, 0.75])
    return ([sq, ar] if order == "A" else [ar, sq]), theta


def _edge32():
    rng = np.random.default_rng(20250303)
    blocks = [(32, [(SQEXP0, _grid(8, 4, rng), 0)]), (33, [(FEXP0, rng.random((33, 2)), 1)])]
    return blocks, np.array([0.13, 0.10])


def _ten_slots():
    """a small and a large block with ten parameter slots each (five fexp terms, two parameters a term, on the same ten
    parameters): more than the eight slots one pass of the score's reductions carries (GRAD_SLOTS, csrc/mvn_grad.h).  The
    product of the terms is an exponential covariance on five coordinates with ranges about 1: condition numbers 4.0 and 24.4"""
    rng = np.random.default_rng(20261021)
    blocks = [(dim, [(FEXP, rng.random((dim, 1)), 2 * k) for k in range(5)]) for dim in (6, 40)]
    return blocks, np.array([1.1, 0.9, 0.8, 1.3, 1.2, 0.7, 0.9, 1.1, 1.05, 0.6])


MIXED, MIXED_THETA = _mixed()
TWO_LARGE_A, TWO_LARGE_THETA = _two_large("A")
TWO_LARGE_B, _ = _two_large("B")
EDGE32, EDGE32_THETA = _edge32()

MIXED_RHO = 2            # the AR1 parameter of MIXED's 5-dim block only
TWO_LARGE_RHO = 3        # the AR1 parameter of the 161-dim block

# NOT an entry of LAYOUTS: at condition numbers this small the float64 numpy twin of the score uses up to 0.035 of the gradient
# bound 2^-52 kappa mag_k (m in {1, 7, 64, 70}, three thetas, weighted and not), above the 0.0101 that
# test_mvn_grad_reference_cpu.py asserts over LAYOUTS.  Its samples: samples(TEN_SLOTS, 70, TEN_SLOTS_SEED)
TEN_SLOTS, TEN_SLOTS_THETA = _ten_slots()
TEN_SLOTS_SEED = 1021

LAYOUTS = {"MIXED": (MIXED, MIXED_THETA), "TWO_LARGE_A": (TWO_LARGE_A, TWO_LARGE_THETA),
           "TWO_LARGE_B": (TWO_LARGE_B, TWO_LARGE_THETA), "EDGE32": (EDGE32, EDGE32_THETA)}


def further_thetas(name):
    """two more parameter vectors of a named layout, inside the ranges the condition bound was checked for"""
    th = LAYOUTS[name][1]
    if name == "MIXED":
        a = th * np.array([1.2, 0.8, 1.25, 1.3, 0.96, 1.1, 0.9, 0.7, 1.2, 1.1])
        b = th * np.array([0.7, 1.3, 0.5, 0.6, 1.04, 0.8, 1.1, 1.4, 0.9, 0.6])
        return [a, b]
    if name.startswith("TWO_LARGE"):
        return [th * np.array([1.3, 0.96, 0.8, 1.05]), th * np.array([0.7, 1.04, 1.2, 0.6])]
    return [th * np.array([0.9, 1.2]), th * np.array([1.1, 0.8])]


def samples(blocks, m, seed):
    """Q x m sample columns, Fortran order"""
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((total_dim(blocks), m)) * 0.4)


# ---------------------------------------------------------------------------------------------- shared references
COLUMNS = {"MIXED": 1100, "TWO_LARGE_A": 40, "TWO_LARGE_B": 40, "EDGE32": 70}


def thetas(name):
    return [LAYOUTS[name][1]] + further_thetas(name)


@functools.lru_cache(maxsize=None)
def sample_matrix(name):
    """the layout's sample columns (tests take the first m of them); read-only"""
    u = samples(LAYOUTS[name][0], COLUMNS[name], seed=sum(map(ord, name)))
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def reference(name, ti=0):
    """the definition of a named layout at thetas(name)[ti], computed once per process and read-only:
    D, bound, exact, derived (dense_definition), L (the dense Cholesky factor) and ll (one value per column of sample_matrix(name):
    mvn_ll of the first m columns is ll[:m].mean())"""
    blocks, theta = LAYOUTS[name][0], thetas(name)[ti]
    _, Ls, ll = definition_columns(blocks, theta, sample_matrix(name))
    D, bound, exact, derived = dense_definition(blocks, theta)
    out = dict(D=D, bound=bound, exact=exact, derived=derived, L=block_diag(Ls), ll=ll)
    for a in out.values():
        a.setflags(write=False)
    return out


def reference_ll(name, ti, m):
    return float(reference(name, ti)["ll"][:m].sum() / m)
