"""Ill-conditioned covariance blocks: seeded cases, a long-double reference of mvn_ll and its score on them, the scales
their rounding errors live on, and float64 twins of the library's own algorithm (tests/chol_reference.py, leaf included)
that calibrate every bound tests/test_gpu_illcond.py uses.  Nothing here calls the library; there is no test in here.

Cases (wire format of cov_layouts; kappa = the largest 2-norm condition number of the blocks, bands asserted by
tests/test_illcond_cases_cpu.py):  E6 in [1e5, 1e7], E7 in [5e6, 1e8], E9 in [1e8, 1e10], E11 in [1e11, 1e12],
E12 in [1e11, 2e12].  Above 2e12 the long-double reference's own error (kappa 2^-64) is no longer below 1/1000 of the
bounds, and nothing is claimed but the breakdown contract (LADDERS).

    SQ128   sqexp0, jittered 16 x 8 grid, d = 128: the leaf alone, all eight tiles of the inverse recursion
    SQ127   the same minus one point: the ragged leaf's store path
    SQ130   sqexp0, 13 x 10 grid: one panel and a last panel of 2
    SQ300   sqexp (scale, range), 20 x 15 grid: three panels, look-ahead, graph capture
    FE300   fexp (scale, range), 300 uniform points: the bench family at long ranges
    AR300   gr x ar1 on times 0 .. 299, rho -> 1
    SQ32    sqexp0, 8 x 4 grid: the last one-wave size;  SQ33 one more point: the first blocked size
    MIX     SQ32 at E9, three diagonal rows, FE300 at E6, SQ130 at E12, one gr parameter shared by all

Scales.  value_mag = (sum w) (d/2 log 2 pi + sum |log L_ii|) + 1/2 sum_j w_j y_j'y_j, the value with every cancellation
removed; the value is held to C_V 2^-52 kappa value_mag.  The gradient is held to the existing 2^-52 kappa mag_k
(mvn_grad_reference) AND to C_G 2^-52 kappa |ref grad_k|: mag_k carries |inv(D)|, which makes the first bound loose by
about kappa up here (the CPU test asserts a factor >= 1e6 on E9 and above).

Twins.  chol_reference.twin_potrf(leaf=twin_leaf16) is the factorisation; twin_value / twin_score add what
csrc/mvn.hip and csrc/mvn_grad.h do with it: the sample columns ride below the matrix as extra rows X = U' inv(L)';
S = X' diag(w) X - (sum w) I; H = inv(L)' S inv(L) by two transposed solves against the inverted diagonal blocks with a
transposition between them (inv(D) is never formed for a large block); the lower triangle of H contracted with
D o dlog, except a pure scale (sqexp / fexp's first parameter, a gr term), whose dlog is constant: coef trace(S).  Blocks of d <= 32 run textbook substitution in one wave (inverse of L by columns, inv(D) = inv(L)' inv(L)).
Every twin runs twice -- on the float64 D of cov_layouts and on D with each entry moved by +- that module's entrywise
build bound, fixed random signs -- because the device builds D with its own exp / pow; the deviation recorded is the
worse of the two.

Measured (test_illcond_cases_cpu.py prints them and asserts they do not exceed what is recorded; TWIN below holds them
rounded up to two digits; every ratio is to the C = 1 bound).  Per case and rung: kappa; factor = the worse of |A - L L'| and the solved sample rows;
solve = the worst of forward / transposed / potrs at m = 65; linv; value; grad (relative to |ref grad_k|):

%(table)s

Constants: C = max(floor, 4 x the rung's worst twin ratio, rounded up to two digits); the floors are the existing
constants -- 2 for factor, solves and linv (chol_reference.C_WS, the flat 2.0 of test_gpu_chol_solve.py), 1 for value and
gradient (the C = 1 of 2^-52 kappa mag_k):

%(constants)s

Device, measured on an MI355X (worst ratio to the C = 1 bound per rung; test_gpu_illcond.py prints them):

%(device)s
"""
import functools

import numpy as np

import chol_reference as cr
import cov_layouts as cl
import mvn_grad_reference as gr

LD = np.longdouble
EPS = 2.0 ** -52
BANDS = {"E6": (1e5, 1e7), "E7": (5e6, 1e8), "E9": (1e8, 1e10), "E11": (1e11, 1e12), "E12": (1e11, 2e12)}
MAX_COLUMNS = 130
SAMPLE_SCALE = 0.4


# ------------------------------------------------------------------------------------------------ the cases
def _points():
    rng = np.random.default_rng(20251001)
    g128 = cl._grid(16, 8, rng)
    g130 = cl._grid(13, 10, rng)
    g32 = cl._grid(8, 4, rng)
    x33 = np.vstack([g32, [[0.35, 0.45]]])
    fe = rng.random((300, 2))
    g300 = cl._grid(20, 15, np.random.default_rng(3))
    return g128, g130, g32, x33, fe, g300


def _cases():
    g128, g130, g32, x33, fe, g300 = _points()
    ones = lambda n: np.ones((n, 1))
    one = lambda th: np.array([th])
    c = {}
    # name: (blocks, {rung: theta}, sample counts m, index of the range-like parameter, index of a pure scale or None)
    c["SQ128"] = ([(128, [(cl.SQEXP0, g128, 0)])], {"E6": one(0.20), "E9": one(0.27), "E12": one(0.34)}, (1, 17), 0, None)
    c["SQ127"] = ([(127, [(cl.SQEXP0, g128[:127], 0)])], {"E9": one(0.27)}, (1, 17), 0, None)
    c["SQ130"] = ([(130, [(cl.SQEXP0, g130, 0)])], {"E9": one(0.26), "E12": one(0.32)}, (1, 17), 0, None)
    c["SQ300"] = ([(300, [(cl.SQEXP, g300, 0)])], {"E6": np.array([1.7, 0.20]), "E9": np.array([1.7, 0.25]),
                                                   "E12": np.array([1.7, 0.30])}, (1, 17, 130), 1, 0)
    c["FE300"] = ([(300, [(cl.FEXP, fe, 0)])], {"E6": np.array([0.8, 1.0]), "E7": np.array([0.8, 10.0])}, (1, 17), 1, 0)
    c["AR300"] = ([(300, [(cl.GR, ones(300), 0), (cl.AR1, np.arange(300.0)[:, None], 1)])],
                  {"E6": np.array([1.3, 0.999]), "E7": np.array([1.3, 0.99999])}, (1, 17), 1, 0)
    c["SQ32"] = ([(32, [(cl.SQEXP0, g32, 0)])], {"E6": one(0.25), "E9": one(0.41), "E11": one(0.60)}, (1, 17), 0, None)
    c["SQ33"] = ([(33, [(cl.SQEXP0, x33, 0)])], {"E6": one(0.25), "E9": one(0.41), "E11": one(0.60)}, (1, 17), 0, None)
    mix = [(32, [(cl.GR, ones(32), 0), (cl.SQEXP0, g32, 1)])]
    mix += [(1, [(cl.GR, [[float(k + 1)]], 0)]) for k in range(3)]
    mix += [(300, [(cl.GR, ones(300), 0), (cl.FEXP, fe, 2)]), (130, [(cl.GR, ones(130), 0), (cl.SQEXP0, g130, 4)])]
    #                                     gr   SQ32  fexp scale, range  SQ130
    c["MIX"] = (mix, {"E12": np.array([0.9, 0.41, 0.8, 1.0, 0.32])}, (1, 17), 4, 0)
    return c


_C = _cases()
CASES = {k: v[0] for k, v in _C.items()}
RUNGS = {k: v[1] for k, v in _C.items()}
MS = {k: v[2] for k, v in _C.items()}
CASE_RUNGS = [(name, rung) for name in _C for rung in RUNGS[name]]
DIRECT = [(n, r) for n, r in CASE_RUNGS if n in ("SQ127", "SQ128", "SQ130", "SQ300")]     # handed to dbg_chol as matrices
DIRECT_M = (1, 65)
MIX_BLOCK_RUNG = {0: "E9", 4: "E6", 5: "E12"}      # MIX's dense blocks and the rung each sits on


def theta(name, rung):
    return RUNGS[name][rung]


def candidates(name, rung, k):
    """k parameter vectors spread inside one rung: the range-like parameter shortened by 0.3 % per pair (kappa falls,
    and stays in the band), the pure scale, where the case has one, alternating between 1 and 1.1 times its value"""
    _, rungs, _, vary, scale = _C[name]
    out = np.repeat(rungs[rung][None, :], k, axis=0)
    for j in range(k):
        out[j, vary] *= 1 - 0.003 * (j // 2 if scale is not None else j)
        if scale is not None and j % 2:
            out[j, scale] *= 1.1
    return out


def wire(name):
    cov, data = cl.layout(CASES[name])
    return cov, data, np.zeros(cov.shape[0])


@functools.lru_cache(maxsize=None)
def sample_matrix(name):
    """Q x MAX_COLUMNS sample columns 0.4 N(0, 1), read-only; tests take the first m"""
    Q = cl.total_dim(CASES[name])
    u = np.asfortranarray(np.random.default_rng(sum(map(ord, name)) + 77).standard_normal((Q, MAX_COLUMNS)) * SAMPLE_SCALE)
    u.setflags(write=False)
    return u


def kappa_of(name, th):
    return max(float(np.linalg.cond(cl.block_matrix(b, th)[0], 2)) for b in CASES[name] if cl.kind(b) != "diag")


def matrix(name, rung):
    """the single block's D in float64 (the cases of DIRECT)"""
    assert len(CASES[name]) == 1
    return cl.block_matrix(CASES[name][0], theta(name, rung))[0]


# ------------------------------------------------------------------------------------------------ the long-double reference
def _block_parts_ld(block, th, U, variant):
    """what gr.score needs of one block, in long double, and sum |log L_ii|.  variant 0: the factorisation of D as it
    stands (gr.block_parts).  variant 1: the SAME quantities through another computation -- D scaled symmetrically to unit
    diagonal, its rows and columns in reverse order -- whose rounding errors are unrelated"""
    dim = block[0]
    D = cl.block_matrix(block, th)[0].astype(LD)
    Uq = U.astype(LD)
    dD = [(p, D * dl) for p, dl in gr.dlog_terms(block, th, LD)]
    eye = np.eye(dim, dtype=LD)
    if variant == 0:
        L = cl.cholesky(D)
        Y = cl.forward_sub(L, Uq)
        A = gr.back_sub(L, Y)
        Dinv = gr.back_sub(L, cl.forward_sub(L, eye))
        logs = np.log(np.diag(L))
        const = -LD(0.5) * dim * cl.LOG_2PI - logs.sum()
        return (D, const, Y, A, Dinv, dD), np.abs(logs).sum()
    s = 1 / np.sqrt(np.diag(D))
    p = np.arange(dim)[::-1]
    D2 = (D * s[:, None] * s[None, :])[np.ix_(p, p)]
    L2 = cl.cholesky(D2)
    Y = cl.forward_sub(L2, (Uq * s[:, None])[p])
    A = np.empty_like(Y)
    A[p] = gr.back_sub(L2, Y)
    A *= s[:, None]
    Di2 = gr.back_sub(L2, cl.forward_sub(L2, eye))
    Dinv = np.empty_like(Di2)
    Dinv[np.ix_(p, p)] = Di2
    Dinv *= s[:, None] * s[None, :]
    const = -LD(0.5) * dim * cl.LOG_2PI - np.log(np.diag(L2)).sum() + np.log(s).sum()
    return (D, const, Y, A, Dinv, dD), None


@functools.lru_cache(maxsize=None)
def _ref_parts(name, rung, variant=0):
    th = theta(name, rung)
    u = sample_matrix(name)[:, :max(MS[name])]
    parts, logs, s = [], LD(0), 0
    for block in CASES[name]:
        pt, la = _block_parts_ld(block, th, u[s:s + block[0]], variant)
        parts.append(pt)
        logs = logs + (la if la is not None else 0)
        s += block[0]
    return parts, logs


def weights(m):
    return gr.weights(m)


def ref_score(name, rung, m, w=None, variant=0):
    """dict(value, grad, mag, kappa, value_mag, ll) in long double on the first m sample columns; ll = the per-column
    pieces sum_b log N(u_bj; 0, D_b), value = sum_j w_j ll_j (w = None: 1 / m each)"""
    parts, logs = _ref_parts(name, rung, variant)
    u = sample_matrix(name)[:, :m]
    value, grad, mag, kappa = gr.score(CASES[name], theta(name, rung), u, w, LD, parts=parts)
    wq = np.full(m, LD(1) / m) if w is None else np.asarray(w).astype(LD)
    quad = sum((pt[2][:, :m] ** 2).sum(0) for pt in parts)
    const = sum(pt[1] for pt in parts)
    Q = cl.total_dim(CASES[name])
    value_mag = wq.sum() * (LD(0.5) * Q * cl.LOG_2PI + logs) + LD(0.5) * (wq * quad).sum()
    return dict(value=value, grad=grad, mag=mag, kappa=kappa, value_mag=value_mag, ll=const - LD(0.5) * quad)


# ------------------------------------------------------------------------------------------------ the float64 twins
def perturbed(D, bound, seed=11):
    """D with every entry moved by + or - its build bound, symmetric, signs fixed by the seed"""
    s = np.random.default_rng(seed).choice([-1.0, 1.0], size=D.shape)
    s = np.triu(s) + np.triu(s, 1).T
    return D + s * np.asarray(bound, dtype=np.float64)


def _block_D(block, th, run):
    D, bound = cr.build_D(block, th)
    return D if run == 0 else perturbed(D, bound)


def twin_factor(D, Ut=None):
    """(L, X, invs) of chol_reference.twin_potrf with the kernel's own leaf"""
    return cr.twin_potrf(D, extra=Ut, leaf=cr.twin_leaf16)


def _twin_block(block, th, U, w, run, want_grad):
    """(weighted value, [(parameter, gradient term)]) of one block as the device's path for its kind computes them"""
    dim = block[0]
    sw = w.sum()
    if cl.kind(block) == "diag":
        v, g, _, _ = gr.score([block], th, U, w, np.float64)
        return v, [(k, g[k]) for k in range(len(th)) if g[k] != 0]
    D = _block_D(block, th, run)
    dls = gr.dlog_terms(block, th, np.float64) if want_grad else []
    mult = np.tril(np.full((dim, dim), 2.0), -1) + np.eye(dim)
    if cl.kind(block) == "small":
        L = cl.cholesky(D)
        Z = cl.forward_sub(L, U)
        value = (w * (-0.5 * dim * float(cl.LOG_2PI) - np.log(np.diag(L)).sum() - 0.5 * (Z * Z).sum(0))).sum()
        if not want_grad:
            return value, []
        Li = cl.forward_sub(L, np.eye(dim))
        A = gr.back_sub(L, Z)
        H = (A * w) @ A.T - sw * (Li.T @ Li)
    else:
        L, X, invs = twin_factor(D, U.T)
        value = (w * (-0.5 * dim * float(cl.LOG_2PI) - np.log(np.diag(L)).sum() - 0.5 * (X * X).sum(1))).sum()
        if not want_grad:
            return value, []
        S = X.T @ (w[:, None] * X) - sw * np.eye(dim)
        T1 = cr.twin_trans(L, invs, S)
        H = cr.twin_trans(L, invs, T1.T.copy())
        # a slot whose dlog is constant over the block is coef trace(S), the trace taken before the solves (k_grad_scale_slot)
        scale = [c for fn, _, _ in block[1] for c in ((2,) if fn == cl.GR else (1, 0) if fn in (cl.SQEXP, cl.FEXP) else (0,))]
        trs = np.trace(S)
        return value, [(p, 0.5 * (c / th[p] * trs if c else (mult * H * D * dl).sum())) for c, (p, dl) in zip(scale, dls)]
    return value, [(p, 0.5 * (mult * H * D * dl).sum()) for p, dl in dls]


def _twin(name, rung, m, w, want_grad):
    th = theta(name, rung)
    u = np.array(sample_matrix(name)[:, :m])
    wv = np.full(m, 1.0 / m) if w is None else np.asarray(w, dtype=np.float64)
    out = []
    for run in (0, 1):
        value, grad, s = 0.0, np.zeros(len(th)), 0
        for block in CASES[name]:
            v, terms = _twin_block(block, th, u[s:s + block[0]], wv, run, want_grad)
            value += v
            for p, g in terms:
                grad[p] += g
            s += block[0]
        out.append((value, grad))
    return out


def twin_value(name, rung, m, w=None):
    """the two runs' values (on D, and on D moved by its build bound)"""
    return [v for v, _ in _twin(name, rung, m, w, False)]


def twin_score(name, rung, m, w=None):
    """the two runs' (value, grad)"""
    return _twin(name, rung, m, w, True)


# ------------------------------------------------------------------------------------------------ the ratios
def value_ratio(value, ref):
    """|value - ref| / (2^-52 kappa value_mag)"""
    return float(abs(LD(value) - ref["value"]) / (EPS * ref["kappa"] * ref["value_mag"]))


def grad_ratios(grad, ref):
    """(|g - ref| / (2^-52 kappa mag), |g - ref| / (2^-52 kappa |ref|)), entry by entry"""
    err = np.abs(np.asarray(grad).astype(LD) - ref["grad"])
    return (err / (EPS * ref["kappa"] * ref["mag"])).astype(float), (err / (EPS * ref["kappa"] * np.abs(ref["grad"]))).astype(float)


def linv_worst(L, invs):
    n = L.shape[0]
    return max(cr.linv_ratio(L[k:k + min(cr.NB, n - k), k:k + min(cr.NB, n - k)], np.asarray(X)[:min(cr.NB, n - k), :min(cr.NB, n - k)])[0]
               for X, k in zip(invs, range(0, n, cr.NB)))


# ------------------------------------------------------------------------------------------------ measured twin ratios, constants
# (case, rung): (kappa, factor, solve, linv, value, grad); None where the case does not run that check
TWIN = {
    ("SQ128", "E6"): (1.04e+06, 0.19, 0.63, 0.061, 0.23, 0.5),
    ("SQ128", "E9"): (1.03e+09, 0.31, 17.0, 0.079, 0.19, 0.4),
    ("SQ128", "E12"): (5.57e+11, 0.4, 120.0, 0.096, 0.21, 0.43),
    ("SQ127", "E9"): (1.03e+09, 0.33, 19.0, 0.079, 0.57, 1.2),
    ("SQ130", "E9"): (1.37e+09, 1.4, 7.7, 0.12, 0.084, 0.17),
    ("SQ130", "E12"): (5.27e+11, 9.3, 20.0, 0.16, 0.064, 0.13),
    ("SQ300", "E6"): (2.60e+06, 0.42, 1.2, 0.17, 0.062, 0.13),
    ("SQ300", "E9"): (1.57e+09, 2.0, 5.8, 0.14, 0.16, 0.38),
    ("SQ300", "E12"): (1.08e+12, 15.0, 29.0, 0.12, 0.55, 2.3),
    ("FE300", "E6"): (5.88e+05, 0.08, None, None, 0.017, 0.042),
    ("FE300", "E7"): (9.01e+06, 0.065, None, None, 0.0079, 0.017),
    ("AR300", "E6"): (5.44e+05, 0.074, None, None, 0.0089, 0.021),
    ("AR300", "E7"): (5.99e+07, 0.089, None, None, 0.0098, 0.02),
    ("SQ32", "E6"): (1.09e+06, 0.48, None, None, 0.24, 0.51),
    ("SQ32", "E9"): (1.09e+09, 0.89, None, None, 0.28, 0.61),
    ("SQ32", "E11"): (2.43e+11, 0.57, None, None, 0.27, 0.54),
    ("SQ33", "E6"): (1.09e+06, 0.23, None, None, 0.17, 0.3),
    ("SQ33", "E9"): (1.40e+09, 0.56, None, None, 0.11, 0.23),
    ("SQ33", "E11"): (3.19e+11, 0.28, None, None, 0.15, 0.3),
    ("MIX", "E12"): (5.27e+11, None, None, None, 0.074, 0.15),
}
FLOORS = dict(factor=2.0, solve=2.0, linv=2.0, value=1.0, grad=1.0)
KINDS = ("factor", "solve", "linv", "value", "grad")


def _up2(x):
    """x rounded up to two significant digits"""
    if x <= 0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 1
    return float(np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e)


def measure(name, rung):
    """the row of TWIN for one case and rung, measured now, and two more figures of the gradient check: the smallest
    |ref grad_k| / (twin's absolute error) and the smallest mag_k / |ref grad_k| over every m and weighting, per parameter"""
    th = theta(name, rung)
    factor = solve = linv = None
    blocks = CASES[name]
    if len(blocks) == 1:
        D, bound = cr.build_D(blocks[0], th)
        u = np.array(sample_matrix(name)[:, :17])
        factor = 0.0
        for run in (0, 1):
            A = D if run == 0 else perturbed(D, bound)
            L, X, invs = twin_factor(A, u.T)
            factor = max(factor, cr.factor_ratio(A, L)[0], cr.rows_ratio(L, X, u.T)[0])
        if (name, rung) in DIRECT:
            L, _, invs = twin_factor(D)
            B = cr.rhs(D.shape[0], max(DIRECT_M))
            Xf = cr.twin_forward(L, invs, B)
            solve = max(cr.forward_ratio(L, Xf, B)[0], cr.trans_ratio(L, cr.twin_trans(L, invs, B), B)[0],
                        cr.potrs_ratio(L, cr.twin_trans(L, invs, Xf), B, FLOORS["solve"])[0])
            linv = linv_worst(L, invs)
    value = grad = 0.0
    residue = tighter = np.full(len(th), np.inf)
    for m in MS[name]:
        for w in (None, weights(m)):
            ref = ref_score(name, rung, m, w)
            for v, g in twin_score(name, rung, m, w):
                value = max(value, value_ratio(v, ref))
                err = np.abs(g.astype(LD) - ref["grad"])
                grad = max(grad, float(grad_ratios(g, ref)[1].max()))
                residue = np.minimum(residue, (np.abs(ref["grad"]) / np.maximum(err, LD(1e-300))).astype(float))
            tighter = np.minimum(tighter, (ref["mag"] / np.abs(ref["grad"])).astype(float))
    return (ref["kappa"], factor, solve, linv, value, grad), residue, tighter


def constants(rung):
    """dict kind -> C for a rung: max(floor, 4 x the worst recorded twin ratio of the cases on that rung, rounded up to two
    digits).  MIX's blocks sit on three rungs; its value and gradient are recorded under its own (worst) rung"""
    out = {}
    for i, kind in enumerate(KINDS):
        worst = max([row[1 + i] for (n, r), row in TWIN.items() if r == rung and row[1 + i] is not None] + [0.0])
        out[kind] = max(FLOORS[kind], _up2(4 * worst))
    return out


def _table():
    head = "    %-6s %-4s %9s %8s %8s %8s %8s %8s" % (("case", "rung", "kappa") + KINDS)
    fmt = lambda x: "       -" if x is None else "%8.3g" % x
    rows = ["    %-6s %-4s %9.2e %s" % (n, r, row[0], " ".join(fmt(x) for x in row[1:])) for (n, r), row in TWIN.items()]
    return "\n".join([head] + rows)


def _constants_table():
    rows = ["    %-4s %s" % (r, "  ".join("%s %.3g" % (k, v) for k, v in constants(r).items())) for r in BANDS]
    return "\n".join(rows)


# ------------------------------------------------------------------------------------------------ the breakdown ladders
def _coincident():
    x = np.random.default_rng(20251002).random((33, 2))
    x[20] = x[5]
    return [(33, [(cl.FEXP0, x, 0)])]


def _ladders():
    """name -> (blocks, parameter vectors from the case's last rung on to the far side of numerical singularity, a
    well-conditioned parameter vector or None, whether the vectors are ordered towards singularity).  COIN: a fexp0 block
    with two coincident points, as real coordinates have them: exactly singular at every range, so the pivot that decides
    is rounding noise of either sign and its three ranges are three such matrices, not steps of a ladder"""
    far = np.array([1.0, 1.1, 1.2, 1.35, 1.5, 1.75, 2.0, 2.5, 3.0])
    return {
        "SQ300": (CASES["SQ300"], [np.array([1.7, 0.30 * f]) for f in far], np.array([1.7, 0.15]), True),
        "SQ32": (CASES["SQ32"], [np.array([0.60 * f]) for f in far], np.array([0.15]), True),
        "AR300": (CASES["AR300"], [np.array([1.3, r]) for r in (0.99999, 1 - 1e-7, 1 - 1e-8, 1 - 1e-9, 1 - 1e-10, 1 - 1e-11,
                                                                 1 - 1e-13, 1 - 1e-16, 1.0)], np.array([1.3, 0.5]), True),
        "FE300": (CASES["FE300"], [np.array([0.8, r]) for r in (10.0, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10)],
                  np.array([0.8, 0.1]), True),
        "COIN": (_coincident(), [np.array([r]) for r in (0.1, 1.0, 10.0)], None, False),
    }


LADDERS = _ladders()


def must_succeed(blocks, th):
    """whether the contract requires success at th: every dense block has kappa_2 <= 2e12 and a long-double factor"""
    for b in blocks:
        if cl.kind(b) == "diag":
            continue
        D = cl.block_matrix(b, th)[0]
        if not np.all(np.isfinite(D)) or not np.linalg.cond(D, 2) <= 2e12:
            return False
        try:
            cl.cholesky(D.astype(LD))
        except np.linalg.LinAlgError:
            return False
    return True


# device ratios per rung, copied from a run of tests/test_gpu_illcond.py on an MI355X
DEVICE = """    rung  factor   solve    linv   value    grad   grad / (2^-52 kappa mag_k)
    E6     0.33     0.7    0.16   0.043   0.079   2.1e-06
    E7    0.065       -       -  0.0059   0.005   3.9e-07
    E9     1.22    13.6   0.074   0.069     0.2   5.6e-09
    E11    0.05       -       -   0.013   0.027   1.4e-11
    E12    17.6    54.9    0.15     0.4    1.31   9.3e-11
    batched and single values: the same bits on every candidate.  First -3 on the ladders: SQ300 at range 0.36 on every path
    (0.33, kappa = 5e13, factorises); AR300 at rho = 1 - 1e-16 on every path; FE300 never, up to range 1e10; SQ32: mvn_ll,
    mvn_ll_grad and mvn_ll_batch (one wave, substitution) never, up to range 1.8, gen_D and update_L (the leaf) at 1.8; COIN:
    -3 at range 0.1, a finite value at range 1"""

__doc__ = __doc__ % dict(table=_table(), constants=_constants_table(), device=DEVICE)
