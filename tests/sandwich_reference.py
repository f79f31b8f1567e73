"""Cases, long-double reference and float64 twin for the cluster-robust sandwich query on the device (csrc/sandwich.hip,
Context.sandwich).  Nothing here calls the library or needs a GPU.

The cases are information_reference.case(key), unchanged (they carry y), each with a cluster rule:

    None (the connected components of ZL's coupling graph)   the sparse designs
    arange(n) % 12                                            geo300_p3, geo150_p1
    arange(n) % 9                                             the two dense-Z cases
    the two true clusters, explicitly                         comp129 (above the cap: the dense operator with explicit ids)
    unions of components {0,1},{2,3},{4,5,6}                  stepped_wedge_7x8x3+unions
    arange(n) % 5, which cuts across the components           longitudinal_70x3+across

The definition (include/glmmr_mcml_sandwich.h): with eta = X beta and the weights w of the information query,

    e = (y - h(eta)) d eta / d mu,   a = Sigma^-1 e,   Sigma = diag(w) + Z D Z',   G[c, p] = sum_{i in c} X_ip a_i,   B = G' G.

`reference` evaluates it as written, by a Cholesky solve in np.longdouble (cov_layouts.cholesky / forward_sub and the back
substitution below) from the float64 e, w and D.  `twin` restates what the device computes, in float64 numpy: the Woodbury
route a = v o (e - ZL t), t = M^-1 ZL' (v o e), R R' = M = I + ZL' V ZL, the back substitution with its sum descending, the
score sums in the shape of k_sand_scores (64 or 256 strided partial sums, then the tree of reduce.h).

THE BOUND.  a = v o (e - ZL t) cancels where the random effects dominate, so the scores are held to their uncancelled scale

    max |G_dev - G_ref|  <=  C_SAND * EPS * S_G,    S_G = max_{c, p} sum_{i in c} |X_ip| v_i (|e_i| + sum_k |ZL_ik| |t_k|)

C_SAND is calibrated as C_INFO is: tests/test_sandwich_reference_cpu.py measures the twin's worst ratio
max |G_twin - G_ref| / (EPS S_G) over every case below, asserts it stays at or below TWIN_RATIO, the measured value rounded up,
and C_SAND = 8 * TWIN_RATIO, the project's margin of 8 for the device's other summation order.  The numpy host formula
(np.linalg.solve(Sigma, e)) is held to the same bound there.

The meat is held to the worst case of ANY order of ncl products and their sum, so derived, not measured:

    |B_dev - G_dev' G_dev (long double)|  <=  (ncl + 2) * EPS * sum_c |G_ca G_cb|    entrywise."""
import functools

import numpy as np

import cov_layouts as cl
import information_reference as ir
from glmmrmcml_amd.model import _working_residual

LD = np.longdouble
EPS = 2.0 ** -52
WG_ROWS = 128                # SAND_WG_ROWS of csrc/sandwich.hip: the workgroup form of k_sand_scores from this many rows
TWIN_RATIO = 0.5             # the twin's worst ratio over the cases, measured 0.419 (family-poisson-identity; next
                             # family-binomial-log 0.385, densez_poisson_log 0.364), rounded up; asserted by test_sandwich_reference_cpu.py
C_SAND = 8 * TWIN_RATIO      # = 4


def _unions(c):
    comp = np.arange(c["X"].shape[0]) // (8 * 3)                     # stepped_wedge(7, 8, 3): cluster-major rows, 24 per component
    return np.array([0, 0, 1, 1, 2, 2, 2])[comp]


# name -> (key of information_reference, cluster rule: None or case -> ids)
RULES = {k: (k, None) for k in ir.FAMILY_KEYS + ir.COMPONENT_KEYS + ir.WIDE_KEYS}
RULES.update({
    "geo300_p3": ("geo300_p3", lambda c: np.arange(300) % 12),
    "geo150_p1": ("geo150_p1", lambda c: np.arange(150) % 12),
    "densez_poisson_log": ("densez_poisson_log", lambda c: np.arange(c["X"].shape[0]) % 9),
    "densez_gamma_inverse": ("densez_gamma_inverse", lambda c: np.arange(c["X"].shape[0]) % 9),
    "comp129": ("comp129", lambda c: np.repeat(np.arange(2), 128)),
    "stepped_wedge_7x8x3+unions": ("stepped_wedge_7x8x3", _unions),
    "longitudinal_70x3+across": ("longitudinal_70x3", lambda c: np.arange(c["X"].shape[0]) % 5),
})
NAMES = list(RULES)
DEFAULT_NAMES = [k for k, (_, rule) in RULES.items() if rule is None]
DENSE_NAMES = ir.DENSE_KEYS + ["comp129"]


@functools.lru_cache(maxsize=None)
def case(name):
    """the information case with `cluster` (ids as int32, or None for the default clusters) and `name`"""
    key, rule = RULES[name]
    c = dict(ir.case(key))
    c["name"], c["key"] = name, key
    c["cluster"] = None if rule is None else np.asarray(rule(c), dtype=np.int32)
    return c


def residual(c):
    """e of the definition in float64, the expressions of csrc/glm.h"""
    return _working_residual(c["y"], c["X"] @ c["beta"], c["link"])


def components(ZL):
    """the default clusters: the connected components of the coupling graph of ZL's rows, numbered by their smallest column
    (csrc/component_plan.h) -> ids per row; a row without an entry raises"""
    from glmmrmcml_amd.model import components_of_rows
    return components_of_rows(ZL)[0]


def clusters(c, D):
    """the ids the query uses for the case: its rule, or the components of Z chol(D)"""
    if c["cluster"] is not None:
        return c["cluster"]
    return components(c["Z"] @ np.linalg.cholesky(D))


def back_sub(G, Y):
    """inv(G') Y for a lower G, row by row from the last, in the precision of the operands"""
    n = G.shape[0]
    T = np.zeros_like(Y)
    for i in range(n - 1, -1, -1):
        T[i] = (Y[i] - (G[i + 1:, i, None] * T[i + 1:]).sum(0)) / G[i, i]
    return T


def scores_of(X, a, ids):
    G = np.zeros((int(ids.max()) + 1, X.shape[1]), dtype=a.dtype)
    np.add.at(G, ids, X.astype(a.dtype) * a[:, None])
    return G


def reference(c, D):
    """(a, G, B) in long double from the float64 e, w and D"""
    Z = c["Z"].astype(LD)
    S = Z @ np.asarray(D, dtype=np.float64).astype(LD) @ Z.T
    S[np.diag_indices_from(S)] += ir.weights(c).astype(LD)
    Gc = cl.cholesky(S)
    a = back_sub(Gc, cl.forward_sub(Gc, residual(c).astype(LD)[:, None]))[:, 0]
    G = scores_of(c["X"], a, clusters(c, D))
    return a, G, G.T @ G


def host_formula(c, D):
    """ModelMCML.sandwich(on="host") without a backend: float64 numpy -> (a, G, B)"""
    S = np.diag(ir.weights(c)) + c["Z"] @ D @ c["Z"].T
    a = np.linalg.solve(S, residual(c))
    G = scores_of(c["X"], a, clusters(c, D))
    return a, G, G.T @ G


def _tree(v):
    """wave_sum of reduce.h over 64 lane values: v[l] += v[l + o], o = 32 .. 1; lane 0"""
    v = np.array(v, dtype=np.float64)
    o = 32
    while o:
        v[:o] = v[:o] + v[o:2 * o]
        o //= 2
    return v[0]


def _score_sum(vals, wg):
    """the sum of a cluster's products the way k_sand_scores adds them: thread t adds entries t, t + T, ... in turn (T = 64,
    or 256 in the workgroup form), a wave tree per 64 threads, then the waves' sums in ascending order"""
    T = 256 if wg else 64
    p = np.r_[vals, np.zeros(-len(vals) % T)].reshape(-1, T)
    lanes = np.zeros(T)
    for row in p:
        lanes = lanes + row
    if not wg:
        return _tree(lanes)
    tot = 0.0
    for w in range(4):
        tot = tot + _tree(lanes[64 * w:64 * w + 64])
    return tot


def twin_parts(c, D):
    """the device's route in float64 -> dict(v, e, ZL, t, a)"""
    Z = c["Z"]
    v = 1 / ir.weights(c)
    e = residual(c)
    ZL = Z @ np.linalg.cholesky(D)
    M = np.eye(ZL.shape[1]) + ZL.T @ (ZL * v[:, None])
    R = cl.cholesky(M)
    s = cl.forward_sub(R, (ZL.T @ (v * e))[:, None])
    Q = R.shape[0]
    t = np.zeros(Q)
    for k in range(Q - 1, -1, -1):                                    # the sum descending, as k_comp_solve's
        acc = s[k, 0]
        for i in range(Q - 1, k, -1):
            if R[i, k] != 0.0:
                acc -= R[i, k] * t[i]
        t[k] = acc / R[k, k]
    return dict(v=v, e=e, ZL=ZL, t=t, a=v * (e - ZL @ t))


def twin(c, D):
    """(a, G) as the device computes them, in float64 numpy"""
    p = twin_parts(c, D)
    ids = clusters(c, D)
    ncl = int(ids.max()) + 1
    wg = max(np.bincount(ids, minlength=ncl)) >= WG_ROWS
    X = c["X"]
    G = np.zeros((ncl, X.shape[1]))
    for k in range(ncl):
        rows = np.nonzero(ids == k)[0]
        for q in range(X.shape[1]):
            G[k, q] = _score_sum(X[rows, q] * p["a"][rows], wg)
    return p["a"], G


def score_scale(c, D):
    """S_G of the module docstring, from the twin's t"""
    p = twin_parts(c, D)
    per_row = p["v"] * (np.abs(p["e"]) + np.abs(p["ZL"]) @ np.abs(p["t"]))
    ids = clusters(c, D)
    S = np.zeros((int(ids.max()) + 1, c["X"].shape[1]))
    np.add.at(S, ids, np.abs(c["X"]) * per_row[:, None])
    return float(S.max())


def ratio(G, G_ref, scale):
    """max |G - G_ref| / (EPS S_G): compared with C_SAND (device, host formula) or TWIN_RATIO (twin)"""
    G = np.asarray(G)
    if G.shape != G_ref.shape or not np.all(np.isfinite(G)):
        return np.inf
    return float(np.max(np.abs(G.astype(LD) - G_ref)) / (LD(EPS) * LD(scale)))


def meat_excess(B, G):
    """max over the entries of |B - G' G (long double)| / ((ncl + 2) EPS sum_c |G_ca G_cb|): at most 1 for any order of the sum"""
    Gl = np.asarray(G).astype(LD)
    want, room = Gl.T @ Gl, (np.abs(Gl).T @ np.abs(Gl)) * LD(EPS) * (G.shape[0] + 2)
    err = np.abs(np.asarray(B).astype(LD) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, LD(0), err / room)
    return float(np.max(r))
