"""Cases and long-double reference for the conditional (kriging) prediction of the random effects at new points
(csrc/predict.hip, Context.predict_re, ModelMCML.predict).  Nothing here calls the library or needs a GPU.

THE QUANTITY.  Block b with covariance D (built by the table of csrc/covspec.h), new points with cross-covariance C
(the same table between a new point and an observed row) and prior variance p (the table at distance 0); u the block's
rows of the sample matrix:

    means = C D^-1 u,        cvar_i = max(p - C_i D^-1 C_i', 0),        summary = (mean_j means, cvar, var_j means)

`evaluate(case, LD)` is the reference: D and C are built in float64 by the table (cov_layouts.block_matrix and
`cross_matrix` below, which rests on cov_layouts._term), then factorised and solved in np.longdouble by the hand-written
cov_layouts.cholesky / forward_sub.  `evaluate(case, np.float64)` is the same pass in float64: one of the two float64 twins
the bound is calibrated with (the other is ModelMCML.predict(on="host")).  All-gr blocks are diagonal: means = (C / p) u.

THE SCALE.  C D^-1 u cancels, so an entry is held against a scale, not against itself.  With a = D^-1 u,
E_M = (8 + 2 sum_k |arg_k|) |M| entrywise (the `bound` of cov_layouts.dense_definition: what another float64 evaluation
of the table may differ by, in units of 2^-52) and L the factor:

    S_mean = |C| |D^-1| (|L| |L'|) |a|  +  E_C |a|  +  |C| |D^-1| E_D |a|

-- the backward error of a Cholesky solve (|L||L'| per unit roundoff) carried to the result, the cross-covariance's own
rounding, and the block's.  S_var_i is the same with g_i = D^-1 C_i' in place of a and E_C counted twice (C_i enters
p - C_i D^-1 C_i' on both sides), plus p_i for the subtraction.  For a diagonal block S_mean = 3 |C / p| |u| and
S_var = p + 3 C^2 / p: a quotient, a product and a sum.  The summary's mean over m columns is held to
C_KRIGE mean_j S_mean + (m - 1) mean_j |means|: the entries' bound plus the worst case of a serial sum of m terms.

THE BOUND.  max |dev - ref| <= C_KRIGE 2^-52 S.  C_KRIGE = 8 * TWIN_RATIO, where TWIN_RATIO is the worst ratio of the
float64 twins over every case below, rounded up (tests/test_kriging_reference_cpu.py measures it and asserts it); the
margin of 8 stands for the device's other orders of summation (MFMA accumulation, the blocked solves against inverted
diagonal blocks, the wave sums), the rule C_INFO of information_reference.py was set by.
"""
import functools

import numpy as np

import cov_layouts as cl

LD = np.longdouble
EPS = 2.0 ** -52
TWIN_RATIO = 0.07           # the twins' worst ratio over the cases below, measured 0.0643 (cvar, MIXED_m3; means 0.0406,
                            # MIXED_m70), rounded up: the scale is a worst-case one (condition numbers up to 3.1e2)
C_KRIGE = 8 * TWIN_RATIO    # = 0.56
MOVE = 0.03                 # a new point is an observed row whose non-gr columns moved by up to +-MOVE


# ---------------------------------------------------------------------------------------------- new points
def _block_columns(block):
    """(the block's dim x ncol data matrix, a mask of its columns that belong to gr terms)"""
    dim, terms = block
    cols, gr = [], []
    for fn, x, _ in terms:
        x = np.asarray(x, dtype=np.float64).reshape(dim, -1)
        cols.append(x)
        gr += [fn == cl.GR] * x.shape[1]
    return np.column_stack(cols), np.array(gr)


def new_points(block, k, rng):
    """k new points of a block (k x ncol).  Dense block: rows of its own data matrix with the non-gr columns moved by up to
    +-MOVE, the gr columns kept (the point stays in its group); point 0 is exactly coincident with an observed row.
    Diagonal block: point 0 matches a level, point 1 (if any) matches none, the rest match levels"""
    X, gr = _block_columns(block)
    if k == 0:
        return None
    rows = rng.integers(0, block[0], size=k)
    P = X[rows].copy()
    if cl.kind(block) == "diag":
        if k > 1:
            P[1, -1] += 1000.5
        return P
    move = rng.uniform(-MOVE, MOVE, size=P.shape)
    move[:, gr] = 0.0
    move[0] = 0.0
    return P + move


def cross_matrix(block, xn, theta, dtype=np.float64):
    """(C, A) in `dtype`: the k x dim cross-covariance of the new points xn and the block's rows by the table, and the sum
    over the terms of the magnitude of the exponent argument (cov_layouts.block_matrix's A)"""
    dim, terms = block
    theta = np.asarray(theta, dtype=np.float64).astype(dtype)
    xn = np.asarray(xn, dtype=np.float64).reshape(len(xn), -1).astype(dtype)
    Cm = np.ones((xn.shape[0], dim), dtype=dtype)
    A = np.zeros((xn.shape[0], dim), dtype=dtype)
    col = 0
    for fn, x, pi in terms:
        x = np.asarray(x, dtype=np.float64).reshape(dim, -1).astype(dtype)
        nv = x.shape[1]
        d = np.sqrt(((xn[:, None, col:col + nv] - x[None, :, :]) ** 2).sum(-1))
        f, a, _ = cl._term(fn, d, theta[pi:])
        Cm = Cm * f
        A = A + a
        col += nv
    return Cm, A


# ---------------------------------------------------------------------------------------------- cases
def make_case(blocks, theta, counts, u, seed, why, chunk=None):
    rng = np.random.default_rng(seed)
    newdata = [new_points(b, int(k), rng) for b, k in zip(blocks, counts)]
    kinds = [cl.kind(b) for b in blocks]
    served = {kd: sum(1 for b, k in zip(kinds, counts) if b == kd and k > 0) for kd in ("diag", "small", "large")}
    return dict(blocks=blocks, theta=np.asarray(theta, float), counts=[int(k) for k in counts], newdata=newdata,
                u=np.asfortranarray(u), m=u.shape[1], K=int(sum(counts)), served=served, why=why, chunk=chunk)


def _named(name, counts, m, why, chunk=None):
    blocks, theta = cl.LAYOUTS[name]
    return make_case(blocks, theta, counts, cl.sample_matrix(name)[:, :m], sum(map(ord, name)) + m, why, chunk)


#                 diag, diag, diag, 150, 5, 33, 32, 3 gr, 7, 289
MIXED_COUNTS = [2, 0, 1, 130, 17, 9, 65, 2, 0, 40]
BUILDERS = {
    "MIXED_m3": lambda: _named("MIXED", MIXED_COUNTS, 3, "k = 0 on a diagonal block and on the 7 block; 17 and 65 new points on "
                               "small blocks (65: past one wave of new points); 130 on the 150 block (past one 128 panel of the "
                               "solve's columns); 9 on the 33 block (48 with its border); 40 on the 289 block (three leaves); a "
                               "level that matches and one that does not on the diagonal rows and on the 3-dim all-gr block"),
    "MIXED_m70": lambda: _named("MIXED", MIXED_COUNTS, 70, "the same with 70 sample columns: past one 64-column pass of the small "
                                "kernel, a second tile of the product"),
    "TWO_LARGE_A": lambda: _named("TWO_LARGE_A", [20, 12], 5, "300 then 161: the query's workspace reused by a smaller block"),
    "TWO_LARGE_B": lambda: _named("TWO_LARGE_B", [12, 20], 5, "161 then 300: the workspace reused by a larger block"),
    "EDGE32": lambda: _named("EDGE32", [1, 7], 4, "32 | 33: the last small and the first large size; one new point on a block"),
    "MIXED_chunk64": lambda: _named("MIXED", MIXED_COUNTS, 3, "GLMMR_MCML_PREDICT_CHUNK=64: the 130 new points of the 150 block run "
                                    "in three chunks, the 65 of the 32 block in two", chunk=64),
}
KEYS = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(key):
    return BUILDERS[key]()


def chunks_expected(c, kc=None):
    kc = kc or c["chunk"]
    return sum(1 if not kc else -(-k // kc) for k in c["counts"] if k > 0)


# ---------------------------------------------------------------------------------------------- the definition
def evaluate(c, dtype=LD, theta=None, scales=True):
    """dict(means K x m, cvar K, mean K, prior K[, S_mean K x m, S_var K, S_sum K]) in `dtype`; block (list of row slices),
    dense (mask of the rows that belong to dense blocks)"""
    theta = c["theta"] if theta is None else np.asarray(theta, float)
    u = c["u"].astype(dtype)
    means, cvar, prior, Sm, Sv, rows, dense = [], [], [], [], [], [], []
    s = r = 0
    for block, xn in zip(c["blocks"], c["newdata"]):
        dim = block[0]
        ub = u[s:s + dim]
        s += dim
        if xn is None:
            continue
        k = len(xn)
        C64, AC = cross_matrix(block, xn, theta)
        D64, AD, _ = cl.block_matrix(block, theta)
        p = cross_matrix(block, _block_columns(block)[0][:1], theta)[0][0, 0]          # distance 0
        Cm = C64.astype(dtype)
        pd = dtype(p)
        if cl.kind(block) == "diag":
            W = Cm / pd
            means.append(W @ ub)
            cvar.append(np.maximum(pd - (Cm * W).sum(1), 0))
            if scales:
                Sm.append(3 * np.abs(W) @ np.abs(ub))
                Sv.append(pd + 3 * (Cm * W).sum(1))
        else:
            L = cl.cholesky(D64.astype(dtype))
            WT = cl.forward_sub(L, Cm.T.copy())
            Y = cl.forward_sub(L, ub.copy())
            means.append(WT.T @ Y)
            cvar.append(np.maximum(pd - (WT * WT).sum(0), 0))
            if scales:
                Li = cl.forward_sub(L, np.eye(dim, dtype=dtype))
                Dinv = Li.T @ Li
                a = Dinv @ ub                                   # dim x m
                G = Dinv @ Cm.T                                 # dim x k
                aC, aDi = np.abs(Cm), np.abs(Dinv)
                LLt = np.abs(L) @ np.abs(L).T
                EC = (8 + 2 * AC.astype(dtype)) * aC
                ED = (8 + 2 * AD.astype(dtype)) * np.abs(D64.astype(dtype))
                CDi = aC @ aDi                                  # k x dim
                Sm.append(CDi @ (LLt @ np.abs(a)) + EC @ np.abs(a) + CDi @ (ED @ np.abs(a)))
                aG = np.abs(G)
                Sv.append(((CDi @ LLt) * aG.T).sum(1) + 2 * (EC * aG.T).sum(1) + ((CDi @ ED) * aG.T).sum(1) + pd)
        prior.append(np.full(k, pd))
        rows.append(slice(r, r + k))
        dense += [cl.kind(block) != "diag"] * k
        r += k
    out = dict(means=np.vstack(means), cvar=np.concatenate(cvar), prior=np.concatenate(prior), block=rows,
               dense=np.array(dense))
    out["mean"] = out["means"].sum(1) / dtype(c["m"])
    if scales:
        out["S_mean"], out["S_var"] = np.vstack(Sm), np.concatenate(Sv)
        out["S_sum"] = C_KRIGE * out["S_mean"].sum(1) / c["m"] + (c["m"] - 1) * np.abs(out["means"]).sum(1) / c["m"]
    return out


@functools.lru_cache(maxsize=None)
def reference(key):
    """evaluate(case(key), LD), computed once per process and read-only"""
    out = evaluate(case(key))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def ratios(got, ref, m):
    """(means, summary mean, cvar): max |got - ref| / (2^-52 S); the first and the last are held to C_KRIGE, the middle one
    to 1 (S_sum carries C_KRIGE itself).  got: the dict of api.predict_re (means may be missing)"""
    def worst(g, r, S):
        g = np.asarray(g)
        if not np.all(np.isfinite(g)):
            return np.inf
        d = np.abs(g.astype(LD) - r)
        return float(np.max(np.where(d == 0, 0, d / (LD(EPS) * np.where(S > 0, S, LD(1e-300))))))   # an exact zero on a zero scale
    return (worst(got["means"], ref["means"], ref["S_mean"]) if "means" in got else 0.0,
            worst(got["mean"], ref["mean"], ref["S_sum"]), worst(got["cond_var"], ref["cvar"], ref["S_var"]))


def sample_var_check(got, m):
    """(worst |sample_var - v| / tol, v): v the variance across the samples (divisor m - 1) recomputed in long double from the
    device's own means; tol = 2^-52 (m + 8) v + 2 (m 2^-52 max |x|)^2 -- a few ulps of each of its m + 1 terms and the square
    of the rounding of the mean, which is all a shifted mean adds (the deviations sum to zero)"""
    x = np.asarray(got["means"]).astype(LD)
    mu = x.sum(1) / LD(m)
    v = ((x - mu[:, None]) ** 2).sum(1) / LD(m - 1)
    tol = LD(EPS) * (m + 8) * v + 2 * (m * LD(EPS) * np.abs(x).max(1)) ** 2
    d = np.abs(np.asarray(got["sample_var"]).astype(LD) - v)
    return float(np.max(np.where(d == 0, 0, d / np.where(tol > 0, tol, 1)))), v
