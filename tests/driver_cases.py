"""Designs, starts and sample matrices for the step exports on dense-block models (test_gpu_drivers_dense.py), and their
oracle side (test_driver_cases_cpu.py, golden/make_driver_golden.py).

Every dense design has Z = I and X = (1, x - 1/2); the samples are L(theta0) N(0, I) from a seeded generator and are
regenerated here, never stored.

    DG     gaussian / identity, one fexp block, n = Q = 130, m = 40, theta0 = (0.25, 0.1), start theta0 * (1.2, 0.85)
    DP     DG's design with poisson / log
    DP5    DP with 41 columns set and niter = 40: the beta term reads 40 columns, the MVN term 41 (defect D5)
    AR     poisson / log, one block fexp x ar1, n = 120, m = 32, three covariance parameters; on the log-theta schedule
           (rhobeg 0.25) the first round's point rho = 0.9 e^0.25 = 1.156 has no value
    SW80   stepped_wedge(10, 6, 5), gr x ar1 blocks of 6: the theta-step is the sequential optimiser, which evaluates a
    SW95   rho > 1 on its way (true rho 0.80 from (0.3, 0.9); true rho 0.95 from (0.3, 0.8))
    MIXED, TWO_LARGE_A   cov_layouts.py's, Z = I, X = 1, poisson / log, m = 24: for mcml_hess and aic_mcml only

The golden file holds what the oracle makes of them (optima, Hessians, AIC values, loop results) and what the CPU twins
of the drivers -- the library's bobyqa / bobyqa_batch over the oracle's objective -- measured against those optima."""
import ctypes as C
import functools
import json
import os

import numpy as np

import cov_layouts as cl
from glmmrmcml_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_golden.json")
WIDTHS = (1, 3, 8)                 # theta_batch 1, 3 and the default
PAR_BOUND = 1e-6                   # beta / theta against the stored optimum, unless the case records a bound of its own
F_BOUND = 1e-9                     # objective at the product's optimum against the oracle's
HESS_STEPS = (1e-4, 1e-2)
HESS_RTOL = 1e-10                  # the project's mvn_ll tolerance (test_gpu_mvn_model.py)
LOOP = dict(m=24, warmup=20, lambda_=0.3, maxsteps=8, target_accept=0.9)
LOOP_CASES = {"DP_c8": ("DP", 8, 4242), "DP_c24": ("DP", 24, 7), "DG_c8": ("DG", 8, 4242)}
LOOP_PERT = 2e-6


def _finish(d, u, start, niter=None):
    d.update(u=np.asfortranarray(u), start=np.asarray(start, float), niter=u.shape[1] if niter is None else niter)
    for k in ("u", "start", "y"):
        d[k].setflags(write=False)
    return d


def _dense(family, m, niter=None):
    n = 130
    d = synth.geospatial(n, seed=7, theta=(0.25, 0.1))
    rng = np.random.default_rng(8)
    xy = d["data"].reshape(2, n).T
    X = np.asfortranarray(np.c_[np.ones(n), xy[:, 0] - 0.5])
    beta = np.array([0.6, 0.4])
    L = np.linalg.cholesky(synth._fexp_D(xy, d["theta"]))
    eta = X @ beta + L @ rng.standard_normal(n)
    if family == "poisson":
        y, link = rng.poisson(np.exp(eta)).astype(float), "log"
    else:
        y, link = eta + rng.standard_normal(n), "identity"
    d.update(X=X, y=y, family=family, link=link, beta=beta, P=2)
    u = L @ np.random.default_rng(3).normal(size=(n, m))
    return _finish(d, u, np.r_[beta, d["theta"] * [1.2, 0.85], 1.0], niter)


def _ar():
    n, m = 120, 32
    rng = np.random.default_rng(11)
    xy = rng.random((n, 2)); t = rng.integers(0, 4, n).astype(float)
    cov = np.array([[0, n, synth.FN_FEXP, 2, 0], [0, n, synth.FN_AR1, 1, 2]], dtype=np.int32, order="F")
    data = np.concatenate([xy[:, 0], xy[:, 1], t])
    theta = np.array([0.25, 0.5, 0.6])
    dist = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    L = np.linalg.cholesky(theta[0] * np.exp(-dist / theta[1]) * theta[2] ** np.abs(t[:, None] - t[None, :]))
    X = np.asfortranarray(np.c_[np.ones(n), xy[:, 0] - 0.5]); beta = np.array([0.6, 0.4])
    y = rng.poisson(np.exp(X @ beta + L @ rng.standard_normal(n))).astype(float)
    u = L @ rng.standard_normal((n, m))
    d = dict(cov=cov, data=data, eff_range=np.zeros(2), Z=np.eye(n, order="F"), X=X, y=y, family="poisson", link="log",
             theta=theta, beta=beta, sigma=1.0, n=n, Q=n, P=2)
    return _finish(d, u, np.r_[beta, 0.3, 0.45, 0.9, 1.0])


def _sw(true_rho, start_rho):
    d = synth.stepped_wedge(ncl=10, nt=6, nind=5, seed=3, theta=(0.25, true_rho))
    nt = 6
    dt = np.abs(np.arange(nt)[:, None] - np.arange(nt)[None, :])
    Lb = np.linalg.cholesky(0.25 ** 2 * true_rho ** dt)
    z = np.random.default_rng(5).standard_normal((d["Q"], 40))
    u = np.concatenate([Lb @ z[c * nt:(c + 1) * nt] for c in range(10)])
    return _finish(d, u, np.r_[d["beta"], 0.3, start_rho, 1.0])


def _layout(name):
    blocks, theta = cl.LAYOUTS[name]
    cov, data = cl.layout(blocks)
    Q = cl.total_dim(blocks)
    rng = np.random.default_rng(12)
    beta = np.array([0.2])
    L = cl.reference(name)["L"]
    y = rng.poisson(np.exp(0.2 + L @ (0.5 * rng.normal(size=Q)))).astype(float)
    d = dict(cov=cov, data=data, eff_range=np.zeros(cov.shape[0]), Z=np.eye(Q, order="F"), X=np.ones((Q, 1), order="F"),
             y=y, family="poisson", link="log", theta=np.array(theta), beta=beta, sigma=1.0, n=Q, Q=Q, P=1)
    return _finish(d, cl.sample_matrix(name)[:, :24], np.r_[beta, theta, 1.0])


_MAKE = {"DG": lambda: _dense("gaussian", 40), "DP": lambda: _dense("poisson", 40),
         "DP5": lambda: _dense("poisson", 41, niter=40), "AR": _ar, "SW80": lambda: _sw(0.80, 0.9),
         "SW95": lambda: _sw(0.95, 0.8), "MIXED": lambda: _layout("MIXED"), "TWO_LARGE_A": lambda: _layout("TWO_LARGE_A")}
SIMLIK = ("DG", "DP", "DP5", "AR")
OPTIM = ("SW80", "SW95")
HESS = ("DG", "DP", "AR", "MIXED", "TWO_LARGE_A")
AIC = ("DG", "DP", "AR", "MIXED")


@functools.lru_cache(maxsize=None)
def case(name):
    """the design of a named case with its samples u (Q x m), start = (beta, theta, sigma | 1) and niter; read-only"""
    return _MAKE[name]()


def args(d):
    return (d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"])


def model(name):
    from oracle import drivers
    d = case(name)
    return drivers.Model(*args(d), d["family"], d["link"])


def fix_sigma(d):
    """what F_likelihood holds the variance parameter at (mcmloptim.h:30): the start's sigma for gaussian, else 0"""
    return float(d["start"][-1]) if d["family"] == "gaussian" else 0.0


def F_obj(name):
    """the oracle's simulated-likelihood objective of a case over (beta, theta)"""
    d = case(name)
    return model(name).F_obj(d["u"], d["niter"], fix_sigma(d))


def ar_first_round_point():
    """theta of AR's first-round point on the log-theta schedule that has no value"""
    th = case("AR")["start"][2:5].copy()
    th[2] *= np.exp(0.25)
    return th


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def par_err(got, want, P):
    """(beta error relative to max(1, |beta|), largest relative error of a covariance parameter)"""
    got = np.asarray(got, float); want = np.asarray(want, float)
    eb = np.abs(got[:P] - want[:P]).max() / max(1.0, np.abs(want[:P]).max()) if P else 0.0
    return float(eb), float((np.abs(got[P:] - want[P:]) / np.abs(want[P:])).max())


def par_bound(name, width):
    """the bound on beta / theta of mcml_simlik for a case at a width: 1e-6, or three times what its CPU twin measured"""
    return golden()["simlik"][name]["twin"][str(width)]["par_bound"]


# ------------------------------------------------------------------------------------------ the drivers' CPU twins
_dp = C.POINTER(C.c_double)
_OBJ = C.CFUNCTYPE(C.c_double, _dp, C.c_int, C.c_void_p)


def bobyqa(fun, x0, lower, width=1, batch=False, rhobeg=0.0, rhoend=0.0, npt=0):
    """the library's bobyqa (batch False; npt interpolation points, 0 its default) or bobyqa_batch at `width` on a Python
    objective -> (x, f, nf, calls)"""
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    n = len(x0)
    calls = []

    def cb(xp, nn, user):
        x = np.array([xp[i] for i in range(nn)])
        v = float(fun(x))
        calls.append((x, v))
        return v
    cbk = _OBJ(cb)
    x0 = np.asarray(x0, float); out = np.zeros(n); f = C.c_double(); nf = C.c_int(); rd = C.c_int()
    lo = np.maximum(np.asarray(lower, float), -1e300); up = np.full(n, 1e300)
    head = (cbk, None, n, x0.ctypes.data_as(_dp), lo.ctypes.data_as(_dp), up.ctypes.data_as(_dp), C.c_double(rhobeg),
            C.c_double(rhoend), 0)
    if batch:
        rc = L.glmmr_mcml_dbg_bobyqa_batch(*head, int(width), out.ctypes.data_as(_dp), C.byref(f), C.byref(nf), C.byref(rd))
    else:
        rc = L.glmmr_mcml_dbg_bobyqa_npt(*head, int(npt), out.ctypes.data_as(_dp), C.byref(f), C.byref(nf))
    _lib.check(rc)
    return out, f.value, nf.value, calls


def simlik_twin(name, width):
    """f_optim as drivers.hip runs it at theta_batch = width, over the oracle's pieces: the objective is the importance
    form -(ll + logl - logl(start theta)) in the driver's order of operations (the constant changes no optimum, but it
    changes every rounding, and the sequential run's end point moves with those); width > 1 the batch schedule over (beta,
    log theta) with rhobeg 0.25 / rhoend 1e-7, width 1 the sequential optimiser over (beta, theta[, sigma]) on 2n + 1
    interpolation points -> (x = (beta, theta), F(x), nf, calls)"""
    from oracle import oracle as orc
    d = case(name); P = d["P"]; R = d["start"].size - P - 1
    mod = model(name)
    denom = mod._mvn(d["start"][P:P + R], d["u"])

    def imp(x):
        ll = orc.model_loglik(mod.Z, mod.X @ x[:P], mod.y, d["u"], fix_sigma(d), mod.fl, ncols=d["niter"])
        return -1.0 * (ll + mod._mvn(x[P:P + R], d["u"]) - denom)
    if width > 1:
        z, _, nf, calls = bobyqa(lambda z: imp(np.r_[z[:P], np.exp(z[P:])]), np.r_[d["start"][:P], np.log(d["start"][P:P + R])],
                                 np.r_[np.full(P, -np.inf), np.full(R, np.log(1e-6))], width, True, 0.25, 1e-7)
        x = np.r_[z[:P], np.exp(z[P:])]
    else:
        gauss = d["family"] == "gaussian"
        x0 = d["start"] if gauss else d["start"][:P + R]
        lo = np.r_[np.full(P, -np.inf), np.full(R, 1e-6), [0.0] if gauss else []]
        x, _, nf, calls = bobyqa(imp, x0, lo, npt=2 * x0.size + 1)
        x = x[:P + R]
    return x, F_obj(name)(x), nf, calls


def optim_twin(name):
    """d_optim's sequential form (mcmloptim.h:56-68) over the oracle's D objective -> (theta, D(theta), nf, calls)"""
    d = case(name); P = d["P"]
    return bobyqa(model(name).D_obj(d["u"]), d["start"][P:-1], np.full(d["start"].size - P - 1, 1e-6))


# ------------------------------------------------------------------------------------------ the loop, oracle side
def loop_sample(name, beta, theta, sigma, it, chains, seed):
    """iteration `it`'s samples as the oracle draws them -> (u, accept flags of every chain)"""
    from oracle import oracle as orc
    d = case(name); mod = model(name)
    L = orc.gen_D(mod.cov, mod.data, mod.eff, theta, chol=True)
    per = -(-LOOP["m"] // chains)
    cols, flags = [], []
    for c in range(chains):
        s, fl, _, _ = orc.hmc_chain(mod.X @ beta, mod.Z @ L, mod.y, sigma, mod.fl, LOOP["warmup"], per, LOOP["lambda_"],
                                    LOOP["maxsteps"], LOOP["target_accept"], seed, chain_id=c, iter_idx=it)
        cols.append(s[:, 1:]); flags.append(fl)
    return L @ np.concatenate(cols, axis=1), np.array(flags)


def loop_oracle(key):
    """two iterations of the oracle's loop (sampler + mcml_optim(mcnr=True)) -> the state after each"""
    from oracle import drivers
    name, chains, seed = LOOP_CASES[key]
    d = case(name); mod = model(name); P = d["P"]
    beta, theta, sig = d["beta"].copy(), d["theta"].copy(), 1.0
    out = []
    for it in (1, 2):
        u, _ = loop_sample(name, beta, theta, sig, it, chains, seed)
        r = drivers.mcml_optim(mod, u, np.r_[beta, theta, 1.0], mcnr=True, niter=u.shape[1], var_par=sig)
        beta, theta = r["beta"], r["theta"]
        if d["family"] == "gaussian":
            sig = r["sigma"]
        out.append(dict(beta=beta.tolist(), theta=theta.tolist(), sigma=float(sig)))
    return out


def loop_response(key, after1):
    """(largest change of iteration 2's u under a +-LOOP_PERT relative change of (beta, theta) after iteration 1, whether
    every accept decision stayed)"""
    name, chains, seed = LOOP_CASES[key]
    b, t, s = np.array(after1["beta"]), np.array(after1["theta"]), after1["sigma"]
    u0, f0 = loop_sample(name, b, t, s, 2, chains, seed)
    worst, same = 0.0, True
    for p in (LOOP_PERT, -LOOP_PERT):
        u, f = loop_sample(name, b * (1 + p), t * (1 + p), s, 2, chains, seed)
        worst = max(worst, float(np.abs(u - u0).max()))
        same = same and np.array_equal(f, f0)
    return worst, same
