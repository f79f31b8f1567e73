"""Cases, long-double reference, float64 twin and host algebra for the small-sample query (csrc/small_sample.hip,
Context.small_sample, ModelMCML.small_sample).  Nothing here calls the library or needs a GPU.

The definition (include/glmmr_mcml_small_sample.h): with Sigma = diag(w) + Z D(theta) Z', d_r Sigma = Z (d_r D) Z' and, for
gaussian / identity, one more parameter sigma last with d_sigma Sigma = 2 sigma I, d2_sigma,sigma Sigma = 2 I,

    P_r = -X' Sigma^-1 d_r Sigma Sigma^-1 X,   Q_rs = X' Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma Sigma^-1 X,
    R_rs = X' Sigma^-1 d2_rs Sigma Sigma^-1 X.

`reference` evaluates them as written in np.longdouble from the float64 w and D: Sigma = G G' (cov_layouts.cholesky),
A = Sigma^-1 X by the two substitutions, B_r = G^-1 d_r Sigma A, P_r = -A' d_r Sigma A, Q_rs = B_r' B_s, R_rs = A' d2_rs Sigma A.
d_r D is theta_information_reference.dD; d2_rs D = D o (dl_r dl_s + [r = s] d2l_r) with the second log-derivatives of `d2log`
below, a table of this module's own.  `twin` restates what the device computes, in float64 numpy: the Q x Q form of the module
comment of csrc/small_sample.hip.  `kr` is the host algebra of ModelMCML.small_sample.

THE BOUND is per output block (each P_r, Q_rs, R_rs) against the block's uncancelled scale,

    max |dev - ref|  <=  C_SS * EPS * S,        EPS = 2^-52,        C_SS = 8 * TWIN_RATIO,

S = the largest entry of the same expression with every factor replaced by its absolute value (`scales`): |d| = |L^-T| |c|,
|U_r| = |d_r D| |d|, |Y_r| = |L^-T| |M^-1| |N| |L^-1| |U_r|, |V_rs| = |D| o (|dl_r| |dl_s| + |d2l|) |d|, and for the sigma entries
|A| = |V| (|X| + |ZL| |c|), the form in which the device builds Sigma^-1 X, |c2| = |M^-1| |ZL'| |V| |A|, |A2| = |V| (|A| + |ZL| |c2|).
A block that is zero by structure (R_r,sigma; R_rs where no block reads both parameters) has S = 0 and must be 0.
TWIN_RATIO is the twin's worst ratio over the cases below -- the very cases tests/test_gpu_small_sample.py runs -- rounded up to
the next integer and asserted by tests/test_small_sample_reference_cpu.py; the 8 stands for the device's other summation order,
as in theta_information_reference.py.  No case is left out."""
import functools

import numpy as np

import cov_layouts as cl
import information_reference as ir
import theta_information_reference as tr

LD = np.longdouble
EPS = 2.0 ** -52
TWIN_RATIO = 17.0            # the twin's worst ratio over the cases, measured 16.626 (longitudinal_70x3, P_1: the slope's variance,
                             # where d = L^-T c cancels; next family-gamma-log 4.40, wide_41 4.35), rounded up to the next
                             # integer; asserted by test_small_sample_reference_cpu.py
C_SS = 8 * TWIN_RATIO        # = 136; the device's measured worst is 30.4 (family-poisson-log, test_gpu_small_sample.py)
HOST_RATIO = 12.0            # the host formula's (ModelMCML.small_sample(on="host")) worst ratio against the long-double
                             # reference in the same measure, measured 11.574 (family-poisson-log), rounded up; asserted there


def _with_x(c, X, beta):
    c = dict(c)
    c["X"], c["beta"] = np.asfortranarray(X), np.asarray(beta, float)
    return c


def _build(key):
    if key == "wide_41_p71":
        w = ir.case("wide_41_p71")
        return _with_x(tr.case("wide_41"), w["X"], w["beta"])
    c = tr.case(key)
    if c["X"].shape[1] >= 2 or key == "mixed":
        return c
    assert key.startswith("geo"), key                                  # P = 1: the coordinates as two more columns
    n = c["X"].shape[0]
    xy = np.asarray(c["data"], float).reshape(2, n).T
    return _with_x(c, np.column_stack([np.ones(n), xy]), [1.0, 0.2, -0.3])


KEYS = list(tr.KEYS) + ["wide_41_p71"]
COMPONENT_KEYS = list(tr.COMPONENT_KEYS) + ["wide_41_p71"]
DENSE_KEYS = list(tr.DENSE_KEYS)


@functools.lru_cache(maxsize=None)
def case(key):
    return _build(key)


rows, names, sigma_row, weights = tr.rows, tr.names, tr.sigma_row, tr.weights


# ---------------------------------------------------------------------------------------------- derivatives of D
def d2log(block, theta, dtype=LD):
    """{parameter: sum over the block's terms that read it of d^2 log(term) / d parameter^2}, dim x dim each:
    gr t^2 -> -2 / t^2;  fexp0 exp(-d/t) -> -2 d / t^3;  ar1 t^d -> -d / t^2;  sqexp t0 exp(-d^2/t1^2) -> -1 / t0^2,
    -6 d^2 / t1^4;  fexp t0 exp(-d/t1) -> -1 / t0^2, -2 d / t1^3;  sqexp0 exp(-d^2/t^2) -> -6 d^2 / t^4.  The log of every term is
    a sum of functions of one parameter each: every cross second log-derivative is 0"""
    dim, terms = block
    theta = np.asarray(theta, dtype=np.float64).astype(dtype)
    out = {}

    def add(p, v):
        out[p] = out.get(p, np.zeros((dim, dim), dtype=dtype)) + v

    one = np.ones((dim, dim), dtype=dtype)
    for fn, x, pi in terms:
        d = cl._distance(np.asarray(x, dtype=np.float64).reshape(dim, -1), dtype)
        t = theta[pi:]
        if fn == cl.GR:
            add(pi, -2 * one / t[0] ** 2)
        elif fn == cl.FEXP0:
            add(pi, -2 * d / t[0] ** 3)
        elif fn == cl.AR1:
            add(pi, -d / t[0] ** 2)
        elif fn == cl.SQEXP:
            add(pi, -one / t[0] ** 2); add(pi + 1, -6 * d * d / t[1] ** 4)
        elif fn == cl.FEXP:
            add(pi, -one / t[0] ** 2); add(pi + 1, -2 * d / t[1] ** 3)
        elif fn == cl.SQEXP0:
            add(pi, -6 * d * d / t[0] ** 4)
        else:
            raise ValueError(fn)
    return out


def d2D(c, D, dtype=LD, absolute=False):
    """{(r, s), r >= s: d^2 D / d theta_r d theta_s} for the pairs some block reads together, Q x Q in `dtype`: D o (dl_r dl_s +
    [r = s] d2l_r) block by block (D as given: diagonal on a block of gr terms alone).  absolute: |D| o (|dl_r| |dl_s| + |d2l_r|)"""
    D = np.asarray(D, dtype=np.float64).astype(dtype)
    out = {}
    s0 = 0
    for block in cl.from_wire(c["cov"], c["data"]):
        sl = slice(s0, s0 + block[0])
        dl, d2 = tr.dlog(block, c["theta"], dtype), d2log(block, c["theta"], dtype)
        for r in dl:
            for s in dl:
                if s > r:
                    continue
                f = np.abs(dl[r]) * np.abs(dl[s]) if absolute else dl[r] * dl[s]
                if r == s:
                    f = f + (np.abs(d2[r]) if absolute else d2[r])
                m = out.setdefault((r, s), np.zeros(D.shape, dtype=dtype))
                m[sl, sl] += (np.abs(D[sl, sl]) if absolute else D[sl, sl]) * f
        s0 += block[0]
    return out


# ---------------------------------------------------------------------------------------------- the definition
def _back_sub(G, Y):
    """inv(G') Y by cov_layouts.forward_sub on the reversed triangle"""
    return cl.forward_sub(G.T[::-1, ::-1], Y[::-1])[::-1]


def _pack(c, Pl, Ql, Rl, dtype):
    no, P = rows(c), c["X"].shape[1]
    out = dict(P=np.zeros((no, P, P), dtype=dtype), Q=np.zeros((no, no, P, P), dtype=dtype), R=np.zeros((no, no, P, P), dtype=dtype))
    for r in range(no):
        out["P"][r] = Pl[r]
        for s in range(no):
            out["Q"][r, s] = Ql[r][s]
            if (max(r, s), min(r, s)) in Rl:
                out["R"][r, s] = Rl[(max(r, s), min(r, s))]
    return out


def reference(c, D):
    """dict(P, Q, R) -- P (no, P, P), Q and R (no, no, P, P) -- by the definition in long double (module docstring)"""
    Z, X = c["Z"].astype(LD), c["X"].astype(LD)
    Dl = np.asarray(D, dtype=np.float64).astype(LD)
    S = tr._zmz(c["Z"], Dl)
    S[np.diag_indices_from(S)] += weights(c).astype(LD)
    G = cl.cholesky(S)
    A = _back_sub(G, cl.forward_sub(G, X))                             # Sigma^-1 X
    ZA = Z.T @ A
    R_ = c["theta"].size
    dSA = [Z @ (d @ ZA) for d in tr.dD(c, D)]                          # d_r Sigma A
    Rl = {k: ZA.T @ (m @ ZA) for k, m in d2D(c, D).items()}
    if sigma_row(c):
        sg = LD(c["var_par"])
        dSA.append(2 * sg * A)
        Rl[(R_, R_)] = 2 * (A.T @ A)
    B = [cl.forward_sub(G, m) for m in dSA]
    Pl = [-(A.T @ m) for m in dSA]
    Ql = [[a.T @ b for b in B] for a in B]
    return _pack(c, Pl, Ql, Rl, LD)


def host_formula(c, D):
    """ModelMCML.small_sample(on="host")'s ingredients without a backend: the n x n definition in float64 numpy"""
    Z, X = c["Z"], c["X"]
    S = np.diag(weights(c)) + Z @ D @ Z.T
    A = np.linalg.solve(S, X)
    dS = [Z @ d @ Z.T for d in tr.dD(c, D, np.float64)]
    Rl = {k: A.T @ (Z @ m @ Z.T) @ A for k, m in d2D(c, D, np.float64).items()}
    if sigma_row(c):
        dS.append(2 * c["var_par"] * np.eye(S.shape[0]))
        Rl[(c["theta"].size,) * 2] = 2 * (A.T @ A)
    Pl = [-(A.T @ d @ A) for d in dS]
    SdA = [np.linalg.solve(S, d @ A) for d in dS]
    Ql = [[(dr @ A).T @ sa for sa in SdA] for dr in dS]
    return _pack(c, Pl, Ql, Rl, np.float64)


# ---------------------------------------------------------------------------------------------- the Q x Q form
def _q_parts(c, D):
    Z, X = c["Z"], c["X"]
    v = 1 / weights(c)
    L = np.linalg.cholesky(D)
    ZL = Z @ L
    N = ZL.T @ (ZL * v[:, None])
    M = np.eye(N.shape[0]) + N
    Rf = np.linalg.cholesky(M)
    b = ZL.T @ (X * v[:, None])
    return v, L, ZL, N, M, Rf, b


def twin(c, D):
    """the device's computation in float64 numpy (module comment of csrc/small_sample.hip): c = R^-T R^-1 b, d = L^-T c,
    U_r = d_r D d, Y_r = L^-T R^-T R^-1 N L^-1 U_r, V_rs = d2_rs D d; the sigma entries from A = V (X - ZL c)"""
    X = c["X"]
    v, L, ZL, N, M, Rf, b = _q_parts(c, D)
    minv = lambda m: _back_sub(Rf, cl.forward_sub(Rf, m))              # the two substitutions, as the device solves
    cc = minv(b)
    d = _back_sub(L, cc)
    U = [m @ d for m in tr.dD(c, D, np.float64)]
    Y = [_back_sub(L, minv(N @ cl.forward_sub(L, u))) for u in U]
    Rl = {k: d.T @ (m @ d) for k, m in d2D(c, D, np.float64).items()}
    Pl = [-(d.T @ u) for u in U]
    Ql = [[u.T @ y for y in Y] for u in U]
    if sigma_row(c):
        sg, R_ = c["var_par"], c["theta"].size
        A = v[:, None] * (X - ZL @ cc)
        c2 = minv(ZL.T @ (v[:, None] * A))
        A2 = v[:, None] * (A - ZL @ c2)
        d2 = _back_sub(L, c2)
        Pl.append(-2 * sg * (A.T @ A))
        for r in range(R_):
            Ql[r].append(2 * sg * (U[r].T @ d2))
        Ql.append([Ql[r][R_].T for r in range(R_)] + [4 * sg * sg * (A.T @ A2)])
        Rl[(R_, R_)] = 2 * (A.T @ A)
    return _pack(c, Pl, Ql, Rl, np.float64)


def scales(c, D):
    """dict(P, Q, R): S of every output block, shapes (no,), (no, no), (no, no) (module docstring, THE BOUND)"""
    X = np.abs(c["X"])
    v, L, ZL, N, M, Rf, b = _q_parts(c, D)
    Li, Mi = np.abs(np.linalg.inv(L)), np.abs(np.linalg.inv(M))
    aZL, aN, av = np.abs(ZL), np.abs(N), np.abs(v)[:, None]
    cc = np.abs(np.linalg.solve(Rf.T, np.linalg.solve(Rf, b)))
    d = Li.T @ cc
    U = [np.abs(m) @ d for m in tr.dD(c, D, np.float64)]
    Y = [Li.T @ (Mi @ (aN @ (Li @ u))) for u in U]
    no, R_ = rows(c), c["theta"].size
    out = dict(P=np.zeros(no), Q=np.zeros((no, no)), R=np.zeros((no, no)))
    for r in range(R_):
        out["P"][r] = np.max(d.T @ U[r])
        for s in range(R_):
            out["Q"][r, s] = np.max(U[r].T @ Y[s])
    for (r, s), m in d2D(c, D, np.float64, absolute=True).items():
        out["R"][r, s] = out["R"][s, r] = np.max(d.T @ (m @ d))
    if sigma_row(c):
        sg = abs(c["var_par"])
        A = av * (X + aZL @ cc)
        c2 = Mi @ (aZL.T @ (av * A))
        A2 = av * (A + aZL @ c2)
        d2 = Li.T @ c2
        out["P"][R_] = 2 * sg * np.max(A.T @ A)
        out["Q"][R_, R_] = 4 * sg * sg * np.max(A.T @ A2)
        for r in range(R_):
            out["Q"][r, R_] = out["Q"][R_, r] = 2 * sg * np.max(U[r].T @ d2)
        out["R"][R_, R_] = 2 * np.max(A.T @ A)
    return out


def block_ratios(got, ref, sc):
    """{(name, index): max |got - ref| / (EPS S)} of every output block; 0 where S = 0 and the block is 0, inf where it is not"""
    out = {}
    for name in ("P", "Q", "R"):
        g, r = np.asarray(got[name]), ref[name]
        if g.shape != r.shape or not np.all(np.isfinite(g)):
            return {(name, ()): np.inf}
        for idx in np.ndindex(*sc[name].shape):
            err = float(np.max(np.abs(g[idx].astype(LD) - r[idx])))
            s = float(sc[name][idx])
            out[(name, idx)] = err / (EPS * s) if s > 0 else (0.0 if err == 0 else np.inf)
    return out


def ratio(got, ref, sc):
    """the worst block ratio: compared with C_SS (device), TWIN_RATIO (twin) or HOST_RATIO (host formula)"""
    return max(block_ratios(got, ref, sc).values())


# ---------------------------------------------------------------------------------------------- the host algebra
TYPES = ("KR", "KR2", "sat")


def kr(info, tinfo, Pm, Qm, Rm, type="KR"):
    """dict(vcov, se, dof, vcov_unadjusted) from the query's blocks: Phi = I_beta^-1, W = I_theta^-1,
    Phi_A = Phi + 2 Phi [sum_rs W_rs (Q_rs - P_r Phi P_s - kappa R_rs / 4)] Phi, kappa = 0 ("KR", Kenward & Roger 1997) or 1
    ("KR2"); "sat" keeps Phi.  dof[k] = 2 Phi_kk^2 / (g_k' W g_k), g_k[r] = (Phi P_r Phi)_kk, for all three"""
    if type not in TYPES:
        raise ValueError("type should be one of %s" % (TYPES,))
    info, tinfo, Pm, Qm, Rm = (np.asarray(a, float) for a in (info, tinfo, Pm, Qm, Rm))
    Phi, W = np.linalg.inv(info), np.linalg.inv(tinfo)
    no = W.shape[0]
    vcov = Phi
    if type != "sat":
        kappa = 1.0 if type == "KR2" else 0.0
        mid = sum(W[r, s] * (Qm[r, s] - Pm[r] @ Phi @ Pm[s] - kappa * 0.25 * Rm[r, s]) for r in range(no) for s in range(no))
        vcov = Phi + 2 * Phi @ mid @ Phi
        vcov = (vcov + vcov.T) / 2
    g = np.array([np.diag(Phi @ Pm[r] @ Phi) for r in range(no)])       # no x P
    with np.errstate(divide="ignore", invalid="ignore"):
        dof = 2 * np.diag(Phi) ** 2 / np.einsum("rk,rs,sk->k", g, W, g)
        se = np.sqrt(np.diag(vcov))
    return dict(vcov=vcov, se=se, dof=dof, vcov_unadjusted=Phi)


def kr_one_row(info, tinfo, Pm, k):
    """(m, lambda) of Kenward & Roger (1997, section 3) for the one-row contrast e_k, as the paper writes them for l = 1"""
    Phi, W = np.linalg.inv(np.asarray(info, float)), np.linalg.inv(np.asarray(tinfo, float))
    no, l = W.shape[0], 1
    e = np.zeros(Phi.shape[0]); e[k] = 1.0
    Theta = np.outer(e, e) / (e @ Phi @ e)
    T = [Theta @ Phi @ Pm[r] @ Phi for r in range(no)]
    A1 = sum(W[r, s] * np.trace(T[r]) * np.trace(T[s]) for r in range(no) for s in range(no))
    A2 = sum(W[r, s] * np.trace(T[r] @ T[s]) for r in range(no) for s in range(no))
    B = (A1 + 6 * A2) / (2 * l)
    g = ((l + 1) * A1 - (l + 4) * A2) / ((l + 2) * A2)
    den = 3 * l + 2 * (1 - g)
    c1, c2, c3 = g / den, (l - g) / den, (l + 2 - g) / den
    Es = 1 / (1 - A2 / l)
    Vs = (2 / l) * (1 + c1 * B) / ((1 - c2 * B) ** 2 * (1 - c3 * B))
    rho = Vs / (2 * Es * Es)
    m = 4 + (l + 2) / (l * rho - 1)
    return m, m / (Es * (m - 2))
