"""Cases, long-double reference and float64 twin for the GLS information of the covariance parameters on the device
(csrc/theta_info.hip, Context.theta_information).  Nothing here calls the library or needs a GPU.

The definition (include/glmmr_mcml_theta_info.h): with the weights w of the information query of the fixed effects,

    Sigma = diag(w) + Z D(theta) Z',    I[r, s] = 1/2 tr(Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma),    d_r Sigma = Z (d_r D) Z',

and for gaussian / identity (w = sigma^2) one more row and column for sigma, d_sigma Sigma = 2 sigma I.

`reference` evaluates it as written in np.longdouble from the float64 D it is given: Sigma = G G' by cov_layouts.cholesky,
Y_r = G^-1 d_r Sigma G^-T by cov_layouts.forward_sub, I[r, s] = 1/2 sum Y_r o Y_s.  d_r D is analytic: D o (the sum over the
terms of the block that read theta_r of d log(term) / d theta_r), the terms' arguments from the table of cov_layouts._term.
`twin` restates what the device computes, in float64 numpy: the Q x Q form with B = M^-1 N (module comment of
csrc/theta_info.hip).

THE BOUND is normwise against the result,

    max |dev - ref|  <=  C_TI * EPS * max |ref|,        EPS = 2^-52,        C_TI = 8 * TWIN_RATIO.

TWIN_RATIO is the twin's worst ratio max |twin - ref| / (EPS max |ref|) over the cases below -- the very cases
tests/test_gpu_theta_information.py runs -- rounded up and asserted by tests/test_theta_information_reference_cpu.py; the 8
stands, as in information_reference.py, for the device's other summation order (MFMA accumulation, the blocked solves against
inverted diagonal blocks, the tile and wave tree sums).

WHICH FORM OF B.  Both operators of the device form B = M^-1 N from N = ZL' V ZL itself (the dense operator by a GEMM of its
own, the component kernel from the rows of ZL), not B = I - M^-1: in the `weak` case N is of the order 1e-6 and the difference
loses that many digits of B, and with it of the result (twin_cancelling below restates that form: its ratio on `weak`, printed
by the calibration test, is 6.9e4, against 0.57 for the form kept).  The weak case therefore does not drive TWIN_RATIO: the
largest ratios are those of the family designs, whose theta = (0.05, 0.03) puts 2 / theta = 40 .. 67 into every E_r."""
import functools

import numpy as np

import cov_layouts as cl
import family_designs as fd
import information_reference as ir
from glmmrmcml_amd import synth

LD = np.longdouble
EPS = 2.0 ** -52
TWIN_RATIO = 5.0             # the twin's worst ratio over the cases, measured 4.452 (family-binomial-logit; next family-gamma-log
                             # 3.72, densez_poisson_log 3.02), rounded up to the next integer: the twin runs on numpy's BLAS, whose
                             # rounding moves by several per cent from one machine to the next; asserted by
                             # test_theta_information_reference_cpu.py
C_TI = 8 * TWIN_RATIO        # = 40


def _case(d, family, link, var_par, op, comps=None, theta=None, why=""):
    """op: the operator Context.theta_information must report under operator=None (0 dense, 1 component); comps: (ncomp,
    max_vars) of the component plan where the context has one"""
    return dict(cov=d["cov"], data=d["data"], eff_range=d["eff_range"], Z=np.asfortranarray(d["Z"]), X=np.asfortranarray(d["X"]),
                family=family, link=link, beta=np.asarray(d["beta"], float),
                theta=np.asarray(d["theta"] if theta is None else theta, float), var_par=float(var_par), op=op, comps=comps,
                why=why, y=np.asarray(d["y"], float), start=np.asarray(d["start"], float))


def _family_case(f, l):
    d = fd.design(f, l, ncl=6, nt=3, nind=8)
    return _case(d, f, l, fd.VAR_PAR[(f, l)], 1, (6, 4), why="n = 144, Q = 24, six components of 4 variables")


def _weak():
    d = fd.design("poisson", "log", ncl=6, nt=3, nind=8)
    return _case(d, "poisson", "log", 1.0, 1, (6, 4), theta=np.asarray(d["theta"]) * 0.02,
                 why="theta x 0.02: N of the order 1e-6, I - M^-1 would cancel")


def _plain(d, op, comps, why):
    return _case(d, d["family"], d["link"], 1.0, op, comps, why=why)


def _split_block():
    d = dict(synth.stepped_wedge(7, 8, 3))
    cl_, t = np.repeat(np.arange(7), 8 * 3), np.tile(np.repeat(np.arange(8), 3), 7)
    keep = ~((cl_ == 0) & (t == 7))
    d["X"], d["Z"], d["y"] = np.asfortranarray(d["X"][keep]), np.asfortranarray(d["Z"][keep]), d["y"][keep]
    return _plain(d, 0, (8, 8), "variable 7 has no observation: a component of its own, block 0 straddles two components")


def _geo(n):
    d = synth.geospatial(n)
    return _case(d, "gaussian", "identity", d["sigma"], 0,
                 why="Z = I, Q = %d, 3 x 3 with the sigma row: %s" % (n, "below two 128 panels" if n < 256 else
                                                                       "two full 128 panels and a ragged 44"))


def _dense_z():
    d = fd.design("poisson", "log", z="dense", **fd.BETA_SIZES)
    return _case(d, "poisson", "log", 1.0, 0, why="n = 297, Q = 36, a dense non-identity Z")


def _mixed():
    cov, data = cl.layout(cl.MIXED)
    Q = cl.total_dim(cl.MIXED)
    d = dict(cov=cov, data=data, eff_range=np.zeros(cov.shape[0]), Z=np.eye(Q, order="F"), X=np.ones((Q, 1), order="F"),
             beta=np.array([0.3]), theta=cl.MIXED_THETA, y=np.zeros(Q), start=np.r_[0.3, cl.MIXED_THETA])
    return _case(d, "poisson", "log", 1.0, 0, why="Q = 522, ten parameters (more than GRAD_SLOTS = 8), every block kind")


FAMILIES = [("poisson", "log"), ("binomial", "logit"), ("gamma", "log"), ("gaussian", "identity")]
BUILDERS = {("family-%s-%s" % (f, l)): functools.partial(_family_case, f, l) for f, l in FAMILIES}
BUILDERS.update({
    "weak": _weak,
    "longitudinal_70x3": lambda: _plain(synth.longitudinal(70, 3), 1, (70, 4), "70 components of 4 variables"),
    "stepped_wedge_7x8x3": lambda: _plain(synth.stepped_wedge(7, 8, 3), 1, (7, 8),
                                          "7 blocks of 8 with a gr * ar1 product: two slots in one block"),
    "wide_41": lambda: _plain(synth.cluster_rct(3, 40, 2), 1, (3, 41), "three components of 41 variables"),
    "comp65": lambda: _plain(synth.cluster_rct(2, 64, 1), 0, (2, 65), "two components of 65 variables: above the cap, dense"),
    "split_block": _split_block,
    "geo150": lambda: _geo(150),
    "geo300": lambda: _geo(300),
    "densez_poisson_log": _dense_z,
    "mixed": _mixed,
})
KEYS = list(BUILDERS)
COMPONENT_KEYS = [k for k in KEYS if k.startswith("family-")] + ["weak", "longitudinal_70x3", "stepped_wedge_7x8x3", "wide_41"]
DENSE_KEYS = ["comp65", "split_block", "geo150", "geo300", "densez_poisson_log", "mixed"]


@functools.lru_cache(maxsize=None)
def case(key):
    return BUILDERS[key]()


def sigma_row(c):
    return c["family"] == "gaussian" and c["link"] == "identity"


def rows(c):
    return c["theta"].size + (1 if sigma_row(c) else 0)


def names(c):
    return ["theta%d" % r for r in range(c["theta"].size)] + (["sigma"] if sigma_row(c) else [])


def dlog(block, theta, dtype=LD):
    """{parameter: sum over the block's terms that read it of d log(term) / d parameter}, dim x dim each.  From the table of
    cov_layouts._term: a term's second return value is |its exponent argument| a, so
    gr t^2 -> 2 / t;  fexp0 exp(-d/t) -> a / t;  ar1 t^d -> d / t;  sqexp t0 exp(-d^2/t1^2) -> 1 / t0, 2 a / t1;
    fexp t0 exp(-d/t1) -> 1 / t0, a / t1;  sqexp0 exp(-d^2/t^2) -> 2 a / t"""
    dim, terms = block
    theta = np.asarray(theta, dtype=np.float64).astype(dtype)
    out = {}

    def add(p, v):
        out[p] = out.get(p, np.zeros((dim, dim), dtype=dtype)) + v

    one = np.ones((dim, dim), dtype=dtype)
    for fn, x, pi in terms:
        d = cl._distance(np.asarray(x, dtype=np.float64).reshape(dim, -1), dtype)
        t = theta[pi:]
        a = cl._term(fn, d, t)[1]
        if fn == cl.GR:
            add(pi, 2 * one / t[0])
        elif fn == cl.FEXP0:
            add(pi, a / t[0])
        elif fn == cl.AR1:
            add(pi, d / t[0])
        elif fn == cl.SQEXP:
            add(pi, one / t[0]); add(pi + 1, 2 * a / t[1])
        elif fn == cl.FEXP:
            add(pi, one / t[0]); add(pi + 1, a / t[1])
        elif fn == cl.SQEXP0:
            add(pi, 2 * a / t[0])
        else:
            raise ValueError(fn)
    return out


def dD(c, D, dtype=LD):
    """[d D / d theta_r, r < R], Q x Q in `dtype`: D (the matrix given, diagonal on a block of gr terms alone, as the device
    builds it) times dlog, block by block"""
    R = c["theta"].size
    D = np.asarray(D, dtype=np.float64).astype(dtype)
    out = [np.zeros(D.shape, dtype=dtype) for _ in range(R)]
    s = 0
    for block in cl.from_wire(c["cov"], c["data"]):
        sl = slice(s, s + block[0])
        for p, f in dlog(block, c["theta"], dtype).items():
            out[p][sl, sl] += D[sl, sl] * f
        s += block[0]
    assert s == D.shape[0]
    return out


def weights(c, dtype=np.float64):
    return ir.weights(c, dtype)


def _zmz(Z, M):
    """Z M Z' in long double; Z = I (geo, mixed) is not multiplied out: the products with exact zeros and ones change nothing"""
    if Z.shape[0] == Z.shape[1] and np.array_equal(Z, np.eye(Z.shape[0])):
        return M.copy()
    Z = Z.astype(LD)
    return Z @ M @ Z.T


def reference(c, D):
    """the definition in long double from the float64 w and D (module docstring)"""
    S = _zmz(c["Z"], np.asarray(D, dtype=np.float64).astype(LD))
    S[np.diag_indices_from(S)] += weights(c).astype(LD)
    G = cl.cholesky(S)
    dS = [_zmz(c["Z"], d) for d in dD(c, D)]
    if sigma_row(c):
        dS.append(2 * LD(c["var_par"]) * np.eye(S.shape[0], dtype=LD))
    Y = [cl.forward_sub(G, cl.forward_sub(G, d).T) for d in dS]
    return np.array([[(a * b).sum() / 2 for b in Y] for a in Y], dtype=LD)


def host_formula(c, D):
    """ModelMCML.theta_information(on="host") without a backend: the n x n definition in float64 numpy, d D of this module"""
    S = np.diag(weights(c)) + c["Z"] @ D @ c["Z"].T
    dS = [c["Z"] @ d @ c["Z"].T for d in dD(c, D, np.float64)]
    if sigma_row(c):
        dS.append(2 * c["var_par"] * np.eye(S.shape[0]))
    A = [np.linalg.solve(S, d) for d in dS]
    info = np.array([[0.5 * np.sum(a * b.T) for b in A] for a in A])
    return (info + info.T) / 2


def _q_form(c, D, B_of):
    Z, n = c["Z"], c["Z"].shape[0]
    v = 1 / weights(c)
    L = np.linalg.cholesky(D)
    ZL = Z @ L
    N = ZL.T @ (ZL * v[:, None])
    M = np.eye(N.shape[0]) + N
    B = B_of(M, N)
    G = []
    for d in dD(c, D, np.float64):
        E = np.linalg.solve(L, np.linalg.solve(L, d).T)
        G.append(B @ E)
    R = len(G)
    no = rows(c)
    out = np.zeros((no, no))
    for r in range(R):
        for s in range(r + 1):
            out[r, s] = out[s, r] = 0.5 * np.sum(G[r] * G[s].T)
    if sigma_row(c):
        sg = c["var_par"]
        for r in range(R):
            out[R, r] = out[r, R] = (np.trace(G[r]) - np.sum(G[r] * B.T)) / sg
        out[R, R] = 2 * (n - 2 * np.trace(B) + np.sum(B * B.T)) / (sg * sg)
    return out


def twin(c, D):
    """the device's computation in float64 numpy: B = M^-1 N by the two substitutions with R, E_r = L^-1 d_r D L^-T,
    G_r = B E_r, I[r, s] = 1/2 sum G_r o G_s', the sigma row from tr G_r, tr(B G_r), tr B, tr(B B)"""
    def B_of(M, N):
        R = np.linalg.cholesky(M)
        return np.linalg.solve(R.T, np.linalg.solve(R, N))
    return _q_form(c, D, B_of)


def twin_cancelling(c, D):
    """the same with B = I - M^-1: the form the device does NOT use (module docstring)"""
    return _q_form(c, D, lambda M, N: np.eye(M.shape[0]) - np.linalg.inv(M))


def ratio(got, ref):
    """max |got - ref| / (EPS max |ref|): compared with C_TI (device, host formula) or TWIN_RATIO (twin)"""
    got = np.asarray(got)
    if got.shape != ref.shape or not np.all(np.isfinite(got)):
        return np.inf
    return float(np.max(np.abs(got.astype(LD) - ref)) / (LD(EPS) * np.max(np.abs(ref))))
