"""Designs and shape lists for the family / link tests of the beta-step and the Laplace path (no test in here, no GPU,
no import of the library).

`design` is the builder tests/test_gpu_families.py has always used -- a cluster design (synth.cluster_rct) whose linear
predictor stays inside the link's domain, for each of the twelve family / link cases of the reference's switch -- with
its sizes as arguments and a choice of the form of Z:

  indicator  the cluster design's own Z: two ones per row.  model_setup (csrc/model.hip) keeps such a Z as padded sparse
             rows (z_width = 2) and z_times runs k_zgather.
  dense      the same cov / data / eff_range, Z replaced by a seeded matrix in which every row has between 9 and Q
             non-zeros of size 0.05 .. 0.5.  model_setup keeps sparse rows only while no row has more than 8 non-zeros
             (maxrow <= 8), so z_width = 0 and z_times takes its GEMM branch (launch_gemm<false> with EpiAxpby into ZU,
             M = n, N = m, K = Q).  No hook reports which branch ran; the condition is restated in z_branch() and
             tests/test_family_designs_cpu.py asserts it on every design.

The shape lists name, entry by entry, the boundary of csrc/model.hip / csrc/laplace.hip they cross;
tests/test_family_designs_cpu.py recomputes every claim from n and m, and checks on the oracle alone that every case is
finite, inside the link's domain and inside the family's support, so that no GPU case needs a skip.
tests/test_gpu_beta_step_shapes.py and tests/test_gpu_la_families.py run them on the device."""
import functools
import math

import numpy as np

from glmmrmcml_amd import synth

# (family, link, var_par): flink = index + 1 (moremaths.h:26-102); var_par != 1 wherever the family reads it
CASES = [("poisson", "log", 1.0), ("poisson", "identity", 1.0), ("binomial", "logit", 1.0), ("binomial", "log", 1.0),
         ("binomial", "identity", 1.0), ("binomial", "probit", 1.0), ("gaussian", "identity", 0.7),
         ("gaussian", "log", 0.6), ("gamma", "log", 2.0), ("gamma", "inverse", 2.0), ("gamma", "identity", 2.0),
         ("beta", "logit", 4.0)]
VAR_PAR = {(f, l): vp for f, l, vp in CASES}
FLINK = {(f, l): i + 1 for i, (f, l, _) in enumerate(CASES)}
IDS = ["%s-%s" % (f, l) for f, l, _ in CASES]
THETA = (0.05, 0.03)                                    # tiny random effects: eta stays near X beta

# constants of csrc/model.hip the shape lists are written against (restated, with their lines, in
# tests/test_family_designs_cpu.py)
ROW_BLOCK, MCNR_CHUNK, ROWSUM_UNROLL, LOGLIK_GRID_Y, ZGATHER_GRID_Y, Z_WIDTH_MAX = 256, 16, 8, 64, 1024, 8


def centre(family, link):
    """the value of eta the design is centred on"""
    c = {"log": 0.3, "identity": 0.5, "logit": 0.2, "probit": 0.1, "inverse": 1.5}[link]
    if family == "binomial" and link == "log":
        c = -1.0                                        # exp(eta) must stay below 1
    if family == "poisson" and link == "identity":
        c = 3.0
    if family == "gamma" and link == "identity":
        c = 2.0
    if family == "gaussian" and link == "log":
        c = 1.5             # the reference logs y twice (mcmlmodel.h:90 and moremaths.h:81): keep log(y) > 0
    return c


def dense_Z(n, Q, seed):
    """n x Q, every row with at least 9 non-zeros (a random half of the columns and nine chosen ones), each of size
    0.05 .. 0.5 with a random sign: with u = L V of size ~0.03, Z u stays a few hundredths"""
    assert Q >= 9
    rng = np.random.default_rng(seed + 7000)
    mask = rng.random((n, Q)) < 0.5
    for i in range(n):
        mask[i, rng.permutation(Q)[:9]] = True
    val = rng.uniform(0.05, 0.5, size=(n, Q)) * rng.choice([-1.0, 1.0], size=(n, Q))
    return np.asfortranarray(np.where(mask, val, 0.0))


def design(family, link, ncl=6, nt=3, nind=6, seed=5, z="indicator", nrows=None, intercept_only=False):
    """small cluster design whose linear predictor stays inside the link's domain.
    z: "indicator" (the gather path of z_times) or "dense" (its GEMM branch: model_setup takes it when some row of Z has
    more than 8 non-zeros, maxrow > 8).  nrows: keep the first nrows observations (rows of X, Z, y) only.
    intercept_only: X is one column of ones (P = 1)."""
    d = synth.cluster_rct(ncl=ncl, nt=nt, nind=nind, seed=seed, family="poisson")
    rng = np.random.default_rng(seed + 100)
    n, P = d["n"], d["P"]
    X = d["X"]
    beta = np.zeros(P)
    theta = np.array(THETA)
    c = centre(family, link)
    beta[1:] = c                                        # the period columns partition the rows
    beta[0] = 0.05
    if intercept_only:
        X, beta, P = np.ones((n, 1), order="F"), np.array([c]), 1
    eta = X @ beta
    if family == "poisson":
        mu = np.exp(eta) if link == "log" else eta
        y = rng.poisson(mu).astype(float)
    elif family == "binomial":
        p = {"logit": 1 / (1 + np.exp(-eta)), "log": np.exp(eta), "identity": eta,
             "probit": 0.5 * (1 + np.vectorize(math.erf)(eta / np.sqrt(2)))}[link]
        y = (rng.random(n) < p).astype(float)
    elif family == "gaussian":
        y = eta + 0.3 * rng.normal(size=n) if link == "identity" else np.exp(eta + 0.1 * rng.normal(size=n))
    elif family == "gamma":
        mu = {"log": np.exp(eta), "inverse": 1 / eta, "identity": eta}[link]
        y = rng.gamma(shape=2.0, scale=mu / 2.0)
    else:                                               # beta
        mu = 1 / (1 + np.exp(-eta))
        y = np.clip(rng.beta(mu * 5, (1 - mu) * 5), 1e-3, 1 - 1e-3)
    Z = d["Z"]
    if z == "dense":
        Z = dense_Z(n, d["Q"], seed)
    else:
        assert z == "indicator", z
    if nrows is not None:
        assert 0 < nrows <= n
        X, Z, y, n = np.asfortranarray(X[:nrows]), np.asfortranarray(Z[:nrows]), y[:nrows].copy(), nrows
    start = np.r_[beta, theta, VAR_PAR[(family, link)]] if family == "gaussian" else np.r_[beta, theta]
    return dict(d, family=family, link=link, y=y, beta=beta, theta=theta, X=X, Z=Z, n=n, P=P, start=start)


def z_branch(Z):
    """the branch of z_times model_setup picks for this Z (csrc/model.hip: z_width > 0 <=> 0 < maxrow <= 8 and
    nnz <= 0.02 n Q + 8 n)"""
    n, Q = Z.shape
    cnt = np.count_nonzero(Z, axis=1)
    sparse = 0 < cnt.max() <= Z_WIDTH_MAX and cnt.sum() <= 0.02 * n * Q + 8.0 * n
    return "gather" if sparse else "gemm"


def in_domain(family, link, eta):
    """every element of eta where the family's log density, mean and weight are defined"""
    eta = np.asarray(eta)
    if link == "identity" and family in ("poisson", "gamma"):
        return bool((eta > 0).all())
    if link == "identity" and family == "binomial":
        return bool(((eta > 0) & (eta < 1)).all())
    if link == "log" and family == "binomial":
        return bool((eta < 0).all())
    if link == "inverse":
        return bool((eta > 0).all())
    return bool(np.isfinite(eta).all())


def in_support(family, link, y):
    y = np.asarray(y)
    if family == "poisson":
        return bool(((y >= 0) & (y == np.round(y))).all())
    if family == "binomial":
        return bool(((y == 0) | (y == 1)).all())
    if family == "gaussian":
        return bool((y > 1).all()) if link == "log" else bool(np.isfinite(y).all())   # log(y) > 0, see centre()
    if family == "gamma":
        return bool((y > 0).all())
    return bool(((y > 0) & (y < 1)).all())              # beta


def reach(n, m):
    """what a beta-step over m sample columns of n observations reaches in csrc/model.hip, from n and m alone"""
    nchunks = -(-m // MCNR_CHUNK)
    return dict(row_blocks=-(-n // ROW_BLOCK),                              # grid x of k_zgather / k_loglik / k_mcnr_row
                chunks=nchunks,                                             # grid y of k_mcnr_row
                last_chunk=m - (nchunks - 1) * MCNR_CHUNK,                  # columns in the last chunk (16: full)
                unrolled=nchunks // ROWSUM_UNROLL,                          # passes of k_mcnr_rowsum's eight-at-a-time loop
                tail=nchunks % ROWSUM_UNROLL,                               # chunks left to its tail loop
                loglik_stride=m > LOGLIK_GRID_Y,                            # k_loglik: j += gridDim.y taken
                zgather_stride=m > ZGATHER_GRID_Y,                          # k_zgather: j += gridDim.y taken
                ragged_rows=n % ROW_BLOCK != 0)                             # j += 256 loops of k_mcnr_col / _fin end ragged


# ------------------------------------------------------------------------------------------ beta-step shapes
BETA_SIZES = dict(ncl=9, nt=3, nind=11)                 # n = 297 = 256 + 41, Q = 36, P = 4
ALL_FAMILIES_M = 150
SWEEP_FAMILIES = [("poisson", "log"), ("gamma", "inverse")]             # one compile-time instance (FL = 1), one FL = 0
ROW_FAMILIES = [("poisson", "log"), ("binomial", "probit")]

# every beta-step case: key -> dict(sizes, nrows, m, niter, z, intercept_only, families, why, reach = the claims)
BETA_CASES = {
    "all_297x150": dict(
        sizes=BETA_SIZES, m=150, families=[(f, l) for f, l, _ in CASES],
        why="second row block of 41 rows; 10 chunks = 8 unrolled + 2 tail, last chunk of 6 columns; k_loglik strides",
        reach=dict(row_blocks=2, chunks=10, last_chunk=6, unrolled=1, tail=2, loglik_stride=True, zgather_stride=False,
                   ragged_rows=True)),
    "m128": dict(
        sizes=BETA_SIZES, m=128, families=SWEEP_FAMILIES,
        why="16 * 8 columns exactly: one unrolled pass of k_mcnr_rowsum, empty tail, full last chunk",
        reach=dict(row_blocks=2, chunks=8, last_chunk=16, unrolled=1, tail=0, loglik_stride=True, zgather_stride=False,
                   ragged_rows=True)),
    "m129": dict(
        sizes=BETA_SIZES, m=129, families=SWEEP_FAMILIES,
        why="last chunk of one column (fifteen clamped loads), one tail chunk after the unrolled pass",
        reach=dict(row_blocks=2, chunks=9, last_chunk=1, unrolled=1, tail=1, loglik_stride=True, zgather_stride=False,
                   ragged_rows=True)),
    "m1": dict(
        sizes=BETA_SIZES, m=1, families=SWEEP_FAMILIES,
        why="a single column: the first chunk is the partial one, grid y of 1 everywhere",
        reach=dict(row_blocks=2, chunks=1, last_chunk=1, unrolled=0, tail=1, loglik_stride=False, zgather_stride=False,
                   ragged_rows=True)),
    "m17": dict(
        sizes=BETA_SIZES, m=17, families=SWEEP_FAMILIES,
        why="one column past a full chunk: the smallest partial chunk that is not the first",
        reach=dict(row_blocks=2, chunks=2, last_chunk=1, unrolled=0, tail=2, loglik_stride=False, zgather_stride=False,
                   ragged_rows=True)),
    "m65": dict(
        sizes=BETA_SIZES, m=65, families=SWEEP_FAMILIES,
        why="one column past k_loglik's 64 column groups: only group 0 strides",
        reach=dict(row_blocks=2, chunks=5, last_chunk=1, unrolled=0, tail=5, loglik_stride=True, zgather_stride=False,
                   ragged_rows=True)),
    "m150_niter149": dict(
        sizes=BETA_SIZES, m=150, niter=149, families=SWEEP_FAMILIES,
        why="set_u(u, niter = m - 1): ZU has 150 columns, the beta-step reads 149 (last chunk of 5)",
        reach=dict(row_blocks=2, chunks=10, last_chunk=5, unrolled=1, tail=2, loglik_stride=True, zgather_stride=False,
                   ragged_rows=True)),
    "m1030": dict(
        sizes=BETA_SIZES, m=1030, families=SWEEP_FAMILIES,
        why="more columns than k_zgather's 1024 column groups: groups 0..5 stride; 65 chunks = 8 passes + 1 tail",
        reach=dict(row_blocks=2, chunks=65, last_chunk=6, unrolled=8, tail=1, loglik_stride=True, zgather_stride=True,
                   ragged_rows=True)),
    "n255": dict(
        sizes=dict(ncl=5, nt=3, nind=17), m=33, families=ROW_FAMILIES,
        why="one row short of a full row block; 3 chunks, last of one column",
        reach=dict(row_blocks=1, chunks=3, last_chunk=1, unrolled=0, tail=3, loglik_stride=False, zgather_stride=False,
                   ragged_rows=True)),
    "n256": dict(
        sizes=dict(ncl=6, nt=3, nind=15), nrows=256, m=33, families=ROW_FAMILIES,
        why="exactly one full row block (270 rows trimmed to 256)",
        reach=dict(row_blocks=1, chunks=3, last_chunk=1, unrolled=0, tail=3, loglik_stride=False, zgather_stride=False,
                   ragged_rows=False)),
    "n257": dict(
        sizes=dict(ncl=6, nt=3, nind=15), nrows=257, m=33, families=ROW_FAMILIES,
        why="a second row block of a single row (270 rows trimmed to 257)",
        reach=dict(row_blocks=2, chunks=3, last_chunk=1, unrolled=0, tail=3, loglik_stride=False, zgather_stride=False,
                   ragged_rows=True)),
    "n513": dict(
        sizes=dict(ncl=9, nt=3, nind=19), m=33, families=ROW_FAMILIES,
        why="a third row block of a single row; the j += 256 loops of k_mcnr_col / k_mcnr_fin run three times",
        reach=dict(row_blocks=3, chunks=3, last_chunk=1, unrolled=0, tail=3, loglik_stride=False, zgather_stride=False,
                   ragged_rows=True)),
    "dense_297x150": dict(
        sizes=BETA_SIZES, m=150, z="dense", families=SWEEP_FAMILIES,
        why="every row of Z has 9 non-zeros or more: z_times takes its GEMM branch into ZU (M = 297, N = 150, K = 36)",
        reach=dict(row_blocks=2, chunks=10, last_chunk=6, unrolled=1, tail=2, loglik_stride=True, zgather_stride=False,
                   ragged_rows=True)),
    "p1_297x150": dict(
        sizes=BETA_SIZES, m=150, intercept_only=True, families=[("gaussian", "identity")],
        why="P = 1: k_xb, k_mcnr_fin and the host solve with a single fixed effect (4 outputs instead of 22)",
        reach=dict(row_blocks=2, chunks=10, last_chunk=6, unrolled=1, tail=2, loglik_stride=True, zgather_stride=False,
                   ragged_rows=True)),
}
BETA_POINTS = [(key, f, l) for key, c in BETA_CASES.items() for f, l in c["families"]]
BETA_IDS = ["%s-%s-%s" % p for p in BETA_POINTS]
CACHE_FAMILIES = SWEEP_FAMILIES                         # the cache tests: set_u(u150), set_u(u20), set_u(u150, 149)
CACHE_M = (150, 20)


@functools.lru_cache(maxsize=None)
def beta_design(key, family, link):
    c = BETA_CASES[key]
    return design(family, link, seed=5, z=c.get("z", "indicator"), nrows=c.get("nrows"),
                  intercept_only=c.get("intercept_only", False), **c["sizes"])


def samples(orc, d, m, seed=1):
    """u = L V with V = 0.5 N(0, 1), Q x m, as tests/test_gpu_families.py draws it"""
    Lo = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    V = np.random.default_rng(seed).normal(size=(d["Q"], m)) * 0.5
    return np.asfortranarray(Lo @ V)


def model_y(d):
    """what the model keeps as y: log(y) for gaussian / log (mcmlmodel.h:89-91)"""
    return np.log(d["y"]) if (d["family"], d["link"]) == ("gaussian", "log") else d["y"]


def beta_oracle(orc, d, u, niter=None, beta=None):
    """(model_loglik, mcnr dict) of the oracle over the first niter columns of u"""
    fam, link = d["family"], d["link"]
    vp, fl = VAR_PAR[(fam, link)], FLINK[(fam, link)]
    beta = d["beta"] if beta is None else beta
    yo = model_y(d)
    ll = orc.model_loglik(d["Z"], d["X"] @ beta, yo, u, vp, fl, ncols=niter)
    return ll, orc.mcnr(d["X"], d["Z"], yo, u, beta, vp, fam, link, ncols=niter)


def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def beta_reference(key, family, link):
    """(u, niter, model_loglik, mcnr dict) of a beta-step case on the oracle: computed once, shared, read-only"""
    c = BETA_CASES[key]
    orc, d = _oracle(), beta_design(key, family, link)
    u = samples(orc, d, c["m"])
    u.setflags(write=False)
    niter = c.get("niter", c["m"])
    ll, r = beta_oracle(orc, d, u, niter)
    return u, niter, ll, r


# ------------------------------------------------------------------------------------------ Laplace shapes
# key -> dict(sizes, why, reach); every family of CASES runs at both
LA_CASES = {
    "small_144x24": dict(
        sizes=dict(ncl=6, nt=3, nind=8),
        why="the small shape of tests/test_gpu_la.py: one row block, Q below one wave",
        reach=dict(n=144, Q=24, row_blocks=1, q_blocks=1, q_mod_256=24)),
    "wide_420x280": dict(
        sizes=dict(ncl=70, nt=3, nind=2),
        why="a second 256-row block in every row-indexed kernel; Q > 256 (k_la_scale_cols' second block, k_la_logdet's "
            "and k_la_gemv_t's strided loops) and no multiple of 4 * 64",
        reach=dict(n=420, Q=280, row_blocks=2, q_blocks=2, q_mod_256=24)),
}
LA_POINTS = [(key, f, l) for key in LA_CASES for f, l, _ in CASES]
LA_IDS = ["%s-%s-%s" % p for p in LA_POINTS]
LA_COMPONENT_KEY = "small_144x24"                       # block-structured: 6 components of 4 variables and 24 observations
LA_COMPONENT_COUNTS = (6, 4, 24)

# v = scale * N(0, 1), functors / Newton step.  The recipe of tests/test_gpu_la.py is 0.3 / 0.2.  The Laplace path
# evaluates W and the score at xb + Z v with the WHITENED v (mcmlmodel.h:121,165: no L in between), so there eta moves by
# the sum of two entries of v -- up to about 1.5 at 0.3 over 280 effects.  Links whose domain is bounded on the side the
# design is centred near get the largest scale of 0.3, 0.2, 0.1, 0.03 at which xb + Z v and xb + ZL v stay inside the
# domain at both shapes (tests/test_family_designs_cpu.py asserts it): binomial / log (eta < 0, centre -1) reaches 0.17 at
# 0.3, binomial / identity (0 < eta < 1, centre 0.5) reaches 1.0 at 0.1.  That is a statement about the inputs, measured
# on the oracle alone, not about the device.
LA_V_SCALE = {("binomial", "log"): (0.2, 0.2), ("binomial", "identity"): (0.03, 0.03)}


def la_v_scale(family, link):
    return LA_V_SCALE.get((family, link), (0.3, 0.2))


@functools.lru_cache(maxsize=None)
def la_design(key, family, link):
    return design(family, link, seed=5, **LA_CASES[key]["sizes"])


def la_reach(n, Q):
    return dict(n=n, Q=Q, row_blocks=-(-n // ROW_BLOCK), q_blocks=-(-Q // 256), q_mod_256=Q % 256)


def la_points(d, trial=0):
    """(v for the functors, v for the Newton step, beta, theta, var_par) of a Laplace case, drawn as
    tests/test_gpu_la.py draws them (generators 11 and 5)"""
    fam, link = d["family"], d["link"]
    sf, ss = la_v_scale(fam, link)
    rng = np.random.default_rng(11 + trial)
    v = rng.normal(size=d["Q"]) * sf
    beta = d["beta"] + rng.normal(size=d["P"]) * 0.1
    theta = d["theta"] * (1 + 0.3 * rng.random(d["theta"].size))
    vs = np.random.default_rng(5 + trial).normal(size=d["Q"]) * ss
    return v, vs, beta, theta, VAR_PAR[(fam, link)]


def la_model(d):
    from oracle import la as ola
    return ola.LaModel(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"], d["start"])


def la_cov_par(d, theta, vp):
    """kind 1, LA_likelihood_cov: (theta, var_par) for the families that have one (flink 7, 8, 12)"""
    return np.r_[theta, vp] if FLINK[(d["family"], d["link"])] in (7, 8, 12) else np.asarray(theta)


def la_btheta_par(d, beta, theta, vp):
    """kind 2, LA_likelihood_btheta: var_par appended for the gaussian family only (flink 7, 8)"""
    return np.r_[beta, theta, vp] if FLINK[(d["family"], d["link"])] in (7, 8) else np.r_[beta, theta]


@functools.lru_cache(maxsize=None)
def la_reference(key, family, link):
    _oracle()
    return la_oracle(la_design(key, family, link))


def la_oracle(d, trial=0):
    """the three functors and the mcnr_b step on the oracle, following tests/test_gpu_la.py"""
    v, vs, beta, theta, vp = la_points(d, trial)
    m = la_model(d); m.var_par = vp
    f_bv = m.la_objective(np.r_[beta, v])
    m = la_model(d); m.var_par = vp; m.v = v.copy(); m.update_W(False)
    f_cov = m.la_cov_objective(la_cov_par(d, theta, vp))
    m = la_model(d); m.var_par = vp; m.v = v.copy()
    f_bt = m.la_btheta_objective(la_btheta_par(d, beta, theta, vp))
    m = la_model(d); m.var_par = vp; m.v = vs.copy()
    m.update_W(True)
    m.mcnr_b()
    return dict(bv=f_bv, cov=f_cov, btheta=f_bt, step=dict(v=m.v.copy(), beta=m.beta.copy(), sigma=float(m.sigma)))
