"""Cases, long-double reference and float64 twin for the GLS information matrix on the device (csrc/info.hip,
Context.information_matrix).  Nothing here calls the library or needs a GPU.

The definition is the caller layer's (glmmrmcml_amd/model.py ModelMCML.information_matrix):

    info = X' (diag(w) + Z D Z')^-1 X,    w_i = dhdmu(x_i' beta) * scale,    scale = sigma^2 | sigma | 1 + sigma | 1

`reference` evaluates it as written, by a hand-written Cholesky solve in np.longdouble (cov_layouts.cholesky / forward_sub, the
routines chol_reference.py rests on) from the float64 D it is given.  `twin` restates what the device computes, in float64
numpy: the Woodbury form X'VX - S'S with V = diag(1 / w), S = R^-1 ZL' V X, R R' = I + ZL' V ZL, the two Gram sums in the
device's shape (chunks of 2048 rows; inside a chunk 256 strided partial sums, then their sum).

THE BOUND.  X'VX - S'S cancels where the random effects dominate, so the error of the Woodbury form is a few roundings of
X'VX, not of the result: the device is held to

    max |dev - ref|  <=  C_INFO * EPS * max |X' V X|,        EPS = 2^-52

normwise.  C_INFO is calibrated the way chol_reference.py calibrates C_F: tests/test_information_reference_cpu.py measures
the twin's worst ratio max |twin - ref| / (EPS max |X'VX|) over every case below -- the cases tests/test_gpu_information.py
runs -- and asserts it stays at or below TWIN_RATIO, the measured value rounded up; C_INFO = 8 * TWIN_RATIO, the margin of
8 standing for the device's other summation order (MFMA accumulation, the blocked solve against inverted diagonal blocks,
the wave tree sums).  The host formula itself (float64 numpy, np.linalg.solve) is held to the same bound there."""
import functools

import numpy as np

import cov_layouts as cl
import family_designs as fd
from glmmrmcml_amd import synth
from glmmrmcml_amd.model import _dhdmu

LD = np.longdouble
EPS = 2.0 ** -52
CHUNK = 2048                 # INFO_CHUNK of csrc/info.hip
TWIN_RATIO = 2.5             # the twin's worst ratio over the cases, measured 2.417 (comp129; next densez_poisson_log 1.77,
                             # family-gaussian-log 1.53), rounded up; asserted by test_information_reference_cpu.py
C_INFO = 8 * TWIN_RATIO      # = 20


def _case(d, family, link, var_par, beta=None, X=None, op=None, why=""):
    X = np.asfortranarray(d["X"] if X is None else X)
    beta = np.asarray(d["beta"] if beta is None else beta, float)
    assert beta.size == X.shape[1]
    return dict(cov=d["cov"], data=d["data"], eff_range=d["eff_range"], Z=np.asfortranarray(d["Z"]), X=X, family=family,
                link=link, beta=beta, theta=np.asarray(d["theta"], float), var_par=float(var_par), op=op, why=why,
                y=np.asarray(d["y"], float), start=np.asarray(d["start"], float))      # y, start: the design's own (fits only)


def _family_case(f, l):
    d = fd.design(f, l, ncl=6, nt=3, nind=8)
    return _case(d, f, l, fd.VAR_PAR[(f, l)], op=1, why="n = 144, Q = 24, six components of 4 variables")


def _geo(n, full):
    d = synth.geospatial(n)
    if not full:
        return _case(d, "gaussian", "identity", d["sigma"], op=0, why="P = 1, Q = %d: below two 128 panels" % n)
    xy = d["data"].reshape(2, n).T
    X = np.column_stack([np.ones(n), xy])
    return _case(d, "gaussian", "identity", d["sigma"], beta=[1.0, 0.2, -0.3], X=X, op=0,
                 why="P = 3, Z = I, Q = 300: two full 128 panels and a ragged 44")


def _wide(extra):
    d = synth.cluster_rct(3, 40, 2)
    X, beta = d["X"], d["beta"]
    if extra:
        rng = np.random.default_rng(20250611)
        X = np.column_stack([X, rng.standard_normal((d["n"], extra))])
        beta = np.r_[beta, 0.05 * rng.standard_normal(extra)]
    return _case(d, d["family"], d["link"], 1.0, beta=beta, X=X, op=2,
                 why="three components of 41 variables, P = %d" % X.shape[1])


def _dense_z(f, l):
    d = fd.design(f, l, z="dense", **fd.BETA_SIZES)
    return _case(d, f, l, fd.VAR_PAR[(f, l)], op=0, why="n = 297, Q = 36, a dense non-identity Z")


def _plain(d, op, why):
    return _case(d, d["family"], d["link"], 1.0, op=op, why=why)


# key -> builder; `op` is the operator Context.information_matrix must report under operator=None
BUILDERS = {("family-%s-%s" % (f, l)): functools.partial(_family_case, f, l) for f, l, _ in fd.CASES}
BUILDERS.update({
    "longitudinal_70x3": lambda: _plain(synth.longitudinal(70, 3), 1, "70 components of 4 variables, P = 2: several per wave"),
    "stepped_wedge_7x8x3": lambda: _plain(synth.stepped_wedge(7, 8, 3), 1, "7 components of 8 variables, P = 9: a ragged last item"),
    "wide_41": lambda: _wide(0),
    "wide_41_p71": lambda: _wide(30),
    "geo300_p3": lambda: _geo(300, True),
    "geo150_p1": lambda: _geo(150, False),
    "densez_poisson_log": lambda: _dense_z("poisson", "log"),
    "densez_gamma_inverse": lambda: _dense_z("gamma", "inverse"),
    "comp129": lambda: _plain(synth.cluster_rct(2, 128, 1), 0, "two components of 129 variables: above the cap, dense; P = 129"),
})
KEYS = list(BUILDERS)
FAMILY_KEYS = [k for k in KEYS if k.startswith("family-")]
COMPONENT_KEYS = ["longitudinal_70x3", "stepped_wedge_7x8x3"]
WIDE_KEYS = ["wide_41", "wide_41_p71"]
DENSE_KEYS = ["geo300_p3", "geo150_p1", "densez_poisson_log", "densez_gamma_inverse"]


@functools.lru_cache(maxsize=None)
def case(key):
    return BUILDERS[key]()


def model_family(family):
    """the family as ModelMCML spells it (R6ModelExtMCML.R: "Gamma")"""
    return "Gamma" if family == "gamma" else family


def weights(c, dtype=np.float64):
    """w of the definition, as ModelMCML.information_matrix forms it"""
    w = _dhdmu(c["X"] @ c["beta"], c["family"], c["link"]).astype(dtype)
    s = dtype(c["var_par"])
    if c["family"] == "gaussian":
        w = w * s * s
    elif c["family"] == "gamma":
        w = w * s
    elif c["family"] == "beta":
        w = w * (1 + s)
    return w


def xtvx_max(c):
    w = weights(c)
    return float(np.max(np.abs(c["X"].T @ (c["X"] / w[:, None]))))


def bound(c):
    return C_INFO * EPS * xtvx_max(c)


def reference(c, D):
    """X' (diag(w) + Z D Z')^-1 X in long double from the float64 w and D: S = G G', Y = G^-1 X, info = Y' Y"""
    Z, X = c["Z"].astype(LD), c["X"].astype(LD)
    S = Z @ np.asarray(D, dtype=np.float64).astype(LD) @ Z.T
    S[np.diag_indices_from(S)] += weights(c).astype(LD)
    G = cl.cholesky(S)
    Y = cl.forward_sub(G, X)
    return Y.T @ Y


def host_formula(c, D):
    """ModelMCML.information_matrix(on="host") without a backend: float64 numpy"""
    S = np.diag(weights(c)) + c["Z"] @ D @ c["Z"].T
    return c["X"].T @ np.linalg.solve(S, c["X"])


def _dot_device_shape(u, w):
    """sum_i u_i w_i the way k_info_gram adds it: chunks of CHUNK rows, inside a chunk thread t adds rows t, t + 256, ...
    in turn, the 256 sums are added, then the chunks' partials in ascending order"""
    tot = 0.0
    for r0 in range(0, len(u), CHUNK):
        p = u[r0:r0 + CHUNK] * w[r0:r0 + CHUNK]
        p = np.r_[p, np.zeros(-len(p) % 256)].reshape(-1, 256)
        lanes = np.zeros(256)
        for row in p:
            lanes = lanes + row
        tot = tot + lanes.sum()
    return tot


def twin(c, D):
    """the device's computation in float64 numpy: X'VX - S'S (module docstring)"""
    X, Z = c["X"], c["Z"]
    P = X.shape[1]
    v = 1 / weights(c)
    XV = X * v[:, None]
    L = np.linalg.cholesky(D)
    ZL = Z @ L
    B = ZL.T @ XV
    M = np.eye(ZL.shape[1]) + ZL.T @ (ZL * v[:, None])
    R = cl.cholesky(M)
    S = cl.forward_sub(R, B)
    out = np.zeros((P, P))
    for a in range(P):
        for b in range(a + 1):
            out[a, b] = out[b, a] = _dot_device_shape(X[:, a], XV[:, b]) - _dot_device_shape(S[:, a], S[:, b])
    return out


def ratio(got, ref, c):
    """max |got - ref| / (EPS max |X'VX|): compared with C_INFO (device, host formula) or TWIN_RATIO (twin)"""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float(np.max(np.abs(got.astype(LD) - ref)) / (LD(EPS) * LD(xtvx_max(c))))
