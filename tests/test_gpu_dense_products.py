"""The sampler's two products per leapfrog step on the dense operator (geospatial designs), with their real fused
epilogues (hmc.hip EpiForwardT / EpiBackward, and k_band_reduce in the streamed decomposition), against the CPU
oracle: log_prob / log_grad of all 12 family / link cases and chains compared one by one, on every dense kernel --
the few-column stream (dgemm_skinny.h), the banded MFMA kernel in both decompositions (dgemm_band.h), the dense
direct-to-LDS kernel (dgemm_dlds.h) and the register-staged one (dgemm_mfma.h).  Every case asserts the kernel it
means through ctx.last_kernels(), and the banded cases their decomposition through ctx.band_plan().

Tolerances as in test_gpu_families / test_gpu_hmc: log_prob / log_grad 1e-10 relative; chains: identical accept
flags, probabilities within 1e-9, samples within 1e-8 relative.  A chain's draws depend on (seed, global chain id)
only, so at large chain counts a subset of chains is compared: the first of the second 16-wide group, the edges of
the first column tile and the last chain of every column tile."""
import os
import subprocess
import sys

import numpy as np
import pytest

from glmmrmcml_amd import api, synth

pytestmark = pytest.mark.gpu

CASES = [("poisson", "log", 1.0), ("poisson", "identity", 1.0), ("binomial", "logit", 1.0), ("binomial", "log", 1.0),
         ("binomial", "identity", 1.0), ("binomial", "probit", 1.0), ("gaussian", "identity", 0.7),
         ("gaussian", "log", 0.6), ("gamma", "log", 2.0), ("gamma", "inverse", 2.0), ("gamma", "identity", 2.0),
         ("beta", "logit", 4.0)]
# one family per epilogue instance (EpiForwardT<1>, <3>, <7>, <12>, the run-time <0>) and per glm_score_post factor
# (1, 1/vp^2 for flinks 7-8, vp for flinks 9-11)
CHAIN_CASES = [CASES[i] for i in (0, 2, 5, 6, 7, 8, 11)]
THETA = (0.05, 0.1)                    # small spatial variance: eta stays inside the link's domain
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _y(family, link, eta, rng):
    if family == "poisson":
        return rng.poisson(np.exp(eta) if link == "log" else eta).astype(float)
    if family == "binomial":
        p = {"logit": 1 / (1 + np.exp(-eta)), "log": np.exp(eta), "identity": eta,
             "probit": 0.5 * (1 + np.vectorize(__import__("math").erf)(eta / np.sqrt(2)))}[link]
        return (rng.random(eta.size) < p).astype(float)
    if family == "gaussian":
        return eta + 0.3 * rng.normal(size=eta.size) if link == "identity" else np.exp(eta + 0.1 * rng.normal(size=eta.size))
    if family == "gamma":
        mu = {"log": np.exp(eta), "inverse": 1 / eta, "identity": eta}[link]
        return rng.gamma(shape=2.0, scale=mu / 2.0)
    mu = 1 / (1 + np.exp(-eta))
    return np.clip(rng.beta(mu * 5, (1 - mu) * 5), 1e-3, 1 - 1e-3)


def design(family, link, Q, zkind="eye", seed=5, theta=THETA):
    """geospatial design (one fexp block over Q locations, X = 1) with any family / link.  zkind:
    eye        Z = I (n = Q; ZL triangular);
    replicated n = 3Q, observation i at location i // 3 (both operands banded, M != K);
    predict    Q - 240 observed locations and 240 trailing unobserved ones, Z = [I 0] (whole empty bands of ZL');
    gap        240 observations without a spatial effect after the first 100 (whole empty bands of ZL)"""
    rng = np.random.default_rng(seed)
    xy = rng.random((Q, 2))
    cov = np.array([[0, Q, synth.FN_FEXP, 2, 0]], dtype=np.int32, order="F")
    if zkind == "eye":
        Z = np.eye(Q, order="F")
    elif zkind == "replicated":
        Z = np.zeros((3 * Q, Q), order="F")
        Z[np.arange(3 * Q), np.arange(3 * Q) // 3] = 1.0
    elif zkind == "predict":
        Z = np.asfortranarray(np.eye(Q)[:Q - 240])
    elif zkind == "gap":
        Z = np.zeros((Q + 240, Q), order="F")
        rows = np.r_[np.arange(100), np.arange(340, Q + 240)]
        Z[rows, np.arange(Q)] = 1.0
    else:
        raise ValueError(zkind)
    n = Z.shape[0]
    centre = {"log": 0.3, "identity": 0.5, "logit": 0.2, "probit": 0.1, "inverse": 1.5}[link]
    if family == "binomial" and link == "log":
        centre = -1.0
    if family == "poisson" and link == "identity":
        centre = 3.0
    if family == "gamma" and link == "identity":
        centre = 2.0
    if family == "gaussian" and link == "log":
        centre = 1.5
    beta = np.array([centre])
    yrng = np.random.default_rng(seed + 1000 + 17 * CASES.index(next(c for c in CASES if c[:2] == (family, link))))
    y = _y(family, link, np.full(n, centre), yrng)
    return dict(cov=cov, data=np.concatenate([xy[:, 0], xy[:, 1]]), eff_range=np.zeros(1), Z=Z,
                X=np.ones((n, 1), order="F"), y=y, family=family, link=link, beta=beta, theta=np.array(theta),
                n=n, Q=Q, seed=seed, zkind=zkind)


_LO = {}


def oracle_L(orc, d):
    """the oracle's Cholesky factor of D, shared by every design on the same locations and theta"""
    key = (d["Q"], d["seed"], tuple(d["theta"]))
    if key not in _LO:
        _LO[key] = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    return _LO[key]


def context(d):
    ctx = api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])
    ctx.update_L(d["theta"])
    return ctx


def _oracle_model(orc, d, Lo):
    fl = orc.flink(d["family"], d["link"])
    yo = np.log(d["y"]) if fl == 8 else d["y"]            # the model keeps log(y) for gaussian-log
    ZL = Lo if d.get("zkind", "eye") == "eye" else np.asfortranarray(d["Z"] @ Lo)
    return ZL, d["X"] @ d["beta"], yo, fl


def tile_columns(C):
    """columns compared at large counts: 0, 15, 16, the first and last of every column tile, the last column"""
    cols = {0, 15, 16, C - 1}
    for t in range(-(-C // 128)):
        cols |= {128 * t, min(128 * t + 127, C - 1)}
    return sorted(c for c in cols if c < C)


def check_log_prob_grad(orc, d, lp, G, V, cols=None, L=None):
    Lo = oracle_L(orc, d) if L is None else L
    ZL, xb, yo, fl = _oracle_model(orc, d, Lo)
    vp = next(c[2] for c in CASES if c[:2] == (d["family"], d["link"]))
    for c in (range(V.shape[1]) if cols is None else cols):
        lo = orc.log_prob(xb, ZL, yo, vp, fl, V[:, c])
        go = orc.log_grad(xb, ZL, yo, vp, fl, V[:, c])
        assert np.isfinite(lo) and np.all(np.isfinite(go)), (d["family"], d["link"], c)
        assert abs(lp[c] - lo) <= 1e-10 * abs(lo), (d["family"], d["link"], c, lp[c], lo)
        assert np.abs(G[:, c] - go).max() <= 1e-10 * max(1.0, np.abs(go).max()), (d["family"], d["link"], c)


def run_log_prob_grad(d, ncols, seed=3):
    vp = next(c[2] for c in CASES if c[:2] == (d["family"], d["link"]))
    V = np.asfortranarray(np.random.default_rng(seed).normal(size=(d["Q"], ncols)) * 0.3)
    with context(d) as ctx:
        lp, G = ctx.log_prob_grad(d["beta"], vp, V)
        kinds = ctx.last_kernels()
        plans = (ctx.band_plan(ncols, "fwd"), ctx.band_plan(ncols, "bwd"))
    return V, lp, G, kinds, plans


# sampler settings of the chain-by-chain checks: a short adaptive warm-up, so the step sizes differ per chain
WARM, LAM, MS, TA, SEED, IT, ADAPT = 6, 0.5, 6, 0.9, 8675309, 1, 6


def run_chains(ctx, d, C, seed=SEED):
    vp = next(c[2] for c in CASES if c[:2] == (d["family"], d["link"]))
    diag, flags, probs = ctx.hmc_sample(d["beta"], vp, WARM, C, LAM, MS, TA, seed, chains=C, iter_idx=IT,
                                        adapt=ADAPT, want_trace=True)
    return ctx.get_u(), flags.copy(), probs.copy()


def check_chains(orc, d, u, flags, probs, chains, L=None, seed=SEED, nsamp=None):
    """chain c of the run against orc.hmc_chain; u holds one draw per chain (C > 1) or the single chain's Q x (nsamp+1)"""
    Lo = oracle_L(orc, d) if L is None else L
    ZL, xb, yo, fl = _oracle_model(orc, d, Lo)
    vp = next(c[2] for c in CASES if c[:2] == (d["family"], d["link"]))
    for c in chains:
        so, fo, po, _ = orc.hmc_chain(xb, ZL, yo, vp, fl, WARM, nsamp or 1, LAM, MS, TA, seed, chain_id=c,
                                      iter_idx=IT, adapt=ADAPT)
        assert np.array_equal(flags[c], fo), (d["family"], d["link"], c, flags[c], fo, probs[c], po)
        assert np.abs(probs[c] - po).max() < 1e-9, (d["family"], d["link"], c)
        uo = Lo @ (so if nsamp else so[:, 1:])
        got = u if nsamp else u[:, c:c + 1]
        assert np.abs(got - uo).max() < 1e-8 * max(1.0, np.abs(uo).max()), (d["family"], d["link"], c)


def _assert_band(ctx, C, paired, split=None):
    for which in ("fwd", "bwd"):
        p = ctx.band_plan(C, which)
        assert p["used"] and p["built"] and p["paired"] == paired, (which, p)
        if split is not None:
            assert (p["nred"] > 0) == split, (which, p)
    return ctx.band_plan(C, "fwd"), ctx.band_plan(C, "bwd")


# ---------------------------------------------------------------- a) log_prob / log_grad, all 12 cases
@pytest.mark.parametrize("family,link,vp", CASES)
def test_log_prob_grad_skinny(orc, family, link, vp, monkeypatch):
    monkeypatch.delenv("GLMMR_MCML_SKINNY", raising=False)
    d = design(family, link, 333)
    for ncols in (3, 16):
        V, lp, G, kinds, _ = run_log_prob_grad(d, ncols)
        assert kinds == ("skinny", "skinny"), (ncols, kinds)
        check_log_prob_grad(orc, d, lp, G, V)


@pytest.mark.parametrize("family,link,vp", CASES)
def test_log_prob_grad_band_streamed_split(orc, family, link, vp):
    """n = Q = 333, 130 columns: two column tiles, the second ragged; every band split (k_band_reduce applies both
    epilogues)"""
    d = design(family, link, 333)
    V, lp, G, kinds, (pf, pb) = run_log_prob_grad(d, 130)
    assert kinds == ("band", "band")
    for p in (pf, pb):
        assert p["used"] and p["built"] and not p["paired"] and p["gn"] == 2 and p["nred"] > 0, p
    check_log_prob_grad(orc, d, lp, G, V)


@pytest.mark.parametrize("family,link,vp", CASES)
def test_log_prob_grad_band_paired(orc, family, link, vp):
    """n = Q = 2000, 1921 columns: the first count that pairs there, 16 column tiles, the last one a single column"""
    d = design(family, link, 2000)
    V, lp, G, kinds, (pf, pb) = run_log_prob_grad(d, 1921)
    assert kinds == ("band", "band")
    for p in (pf, pb):
        assert p["used"] and p["built"] and p["paired"] and p["gn"] == 16 and p["nred"] == 0, p
    check_log_prob_grad(orc, d, lp, G, V, cols=tile_columns(1921))


@pytest.mark.parametrize("family,link,vp", CASES)
def test_log_prob_grad_dlds(orc, family, link, vp, monkeypatch):
    monkeypatch.setenv("GLMMR_MCML_GEMM", "dlds")            # read by update_L: the banded kernel is not set up
    d = design(family, link, 333)
    V, lp, G, kinds, _ = run_log_prob_grad(d, 40)
    assert kinds == ("dlds", "dlds")
    check_log_prob_grad(orc, d, lp, G, V)


def test_log_prob_grad_register_staged_kernel(orc, tmp_path):
    """GLMMR_MCML_GEMM=reg is read once per process (hmc.hip use_dlds): all 12 cases in one child process"""
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_dense_products as T
out = {}
for i, (fam, link, vp) in enumerate(T.CASES):
    d = T.design(fam, link, 333)
    V, lp, G, kinds, _ = T.run_log_prob_grad(d, 20)
    out["V%%d" %% i], out["lp%%d" %% i], out["G%%d" %% i] = V, lp, G
    out["k%%d" %% i] = np.array([k == "reg" for k in kinds])
np.savez(sys.argv[1], **out)
""" % (ROOT, os.path.join(ROOT, "tests"))
    f = str(tmp_path / "reg.npz")
    subprocess.run([sys.executable, "-c", code, f], check=True, env=dict(os.environ, GLMMR_MCML_GEMM="reg"), timeout=300)
    with np.load(f) as z:
        for i, (fam, link, vp) in enumerate(CASES):
            assert z["k%d" % i].all(), (fam, link)
            check_log_prob_grad(orc, design(fam, link, 333), z["lp%d" % i], z["G%d" % i], z["V%d" % i])


# ---------------------------------------------------------------- b) chain by chain
@pytest.mark.parametrize("family,link,vp", CHAIN_CASES)
def test_chains_band_streamed(orc, family, link, vp):
    d = design(family, link, 333)
    with context(d) as ctx:
        u, flags, probs = run_chains(ctx, d, 130)
        assert ctx.last_kernels() == ("band", "band")
        _assert_band(ctx, 130, paired=False, split=True)
    check_chains(orc, d, u, flags, probs, tile_columns(130))


@pytest.mark.parametrize("family,link,vp", CHAIN_CASES)
def test_chains_band_paired(orc, family, link, vp):
    d = design(family, link, 2000)
    with context(d) as ctx:
        u, flags, probs = run_chains(ctx, d, 1921)
        assert ctx.last_kernels() == ("band", "band")
        _assert_band(ctx, 1921, paired=True, split=False)
    check_chains(orc, d, u, flags, probs, tile_columns(1921))


@pytest.mark.parametrize("family,link,vp", CHAIN_CASES)
def test_chains_dlds(orc, family, link, vp, monkeypatch):
    monkeypatch.setenv("GLMMR_MCML_GEMM", "dlds")
    d = design(family, link, 333)
    with context(d) as ctx:
        u, flags, probs = run_chains(ctx, d, 40)
        assert ctx.last_kernels() == ("dlds", "dlds")
    check_chains(orc, d, u, flags, probs, [0, 15, 16, 31, 32, 39])


@pytest.mark.parametrize("family,link,vp", CHAIN_CASES)
def test_chains_skinny(orc, family, link, vp, monkeypatch):
    monkeypatch.delenv("GLMMR_MCML_SKINNY", raising=False)
    d = design(family, link, 333)
    with context(d) as ctx:
        u, flags, probs = run_chains(ctx, d, 16)
        assert ctx.last_kernels() == ("skinny", "skinny")
    check_chains(orc, d, u, flags, probs, range(16))


@pytest.mark.parametrize("family,link,vp", CHAIN_CASES)
def test_single_chain_on_the_band_kernel(orc, family, link, vp, monkeypatch):
    """chains = 1 (the reference's Q x (nsamp+1) layout) with GLMMR_MCML_SKINNY=0: one column on the banded kernel"""
    monkeypatch.setenv("GLMMR_MCML_SKINNY", "0")
    d = design(family, link, 333)
    nsamp = 3
    with context(d) as ctx:
        diag, flags, probs = ctx.hmc_sample(d["beta"], vp, WARM, nsamp, LAM, MS, TA, SEED, chains=1, iter_idx=IT,
                                            adapt=ADAPT, want_trace=True)
        u = ctx.get_u()
        assert ctx.last_kernels() == ("band", "band")
        _assert_band(ctx, 1, paired=False)
    assert u.shape == (d["Q"], nsamp + 1)
    check_chains(orc, d, u, flags, probs, [0], nsamp=nsamp)


# ---------------------------------------------------------------- c) the decomposition boundary
def test_streamed_to_paired_boundary(orc):
    """n = Q = 2000: 1920 chains (15 column tiles) run streamed, 1921 and 1930 (16) paired.  Within one decomposition
    the shared chains are the same draws bit for bit (1921 / 1930).  Across the boundary the split-K pieces of the
    streamed form are summed in another order than the paired form's single K loop (dgemm_band.h: bit-reproducible
    per operand and chain count), so every shared chain of 1920 / 1921 is held to the oracle contract instead; a
    subset of each run, chain 1920 of the paired one included, against the oracle"""
    d = design("poisson", "log", 2000)
    runs = {}
    for C, paired in ((1920, False), (1921, True), (1930, True)):
        with context(d) as ctx:
            runs[C] = run_chains(ctx, d, C)
            assert ctx.last_kernels() == ("band", "band")
            pf, pb = _assert_band(ctx, C, paired=paired)
            assert pf["gn"] == pb["gn"] == -(-C // 128)
    (u0, f0, p0), (u1, f1, p1), (u2, f2, p2) = runs[1920], runs[1921], runs[1930]
    assert np.array_equal(u1, u2[:, :1921])
    assert np.array_equal(f1, f2[:1921]) and np.array_equal(p1, p2[:1921])
    assert np.array_equal(f0, f1[:1920])
    assert np.abs(p0 - p1[:1920]).max() < 1e-9
    assert np.abs(u0 - u1[:, :1920]).max() < 1e-8 * max(1.0, np.abs(u1).max())
    check_chains(orc, d, u1, f1, p1, [0, 127, 1919, 1920])
    check_chains(orc, d, u0, f0, p0, [0, 1792, 1919])


# ---------------------------------------------------------------- d) band-structure edges
@pytest.mark.parametrize("zkind,Q,family,link", [("eye", 333, "binomial", "logit"), ("replicated", 150, "poisson", "log"),
                                                 ("predict", 573, "gamma", "log"), ("gap", 333, "binomial", "probit")])
def test_band_structure_edges(orc, zkind, Q, family, link):
    """Z = I at sizes off the tile grid; n = 3Q replicated observations (M != K in both products); trailing prediction
    locations (whole empty bands of ZL': G = -x and the leapfrog update with no product); observations without a
    spatial effect (whole empty bands of ZL: S = score(y, xb))"""
    d = design(family, link, Q, zkind)
    V, lp, G, kinds, (pf, pb) = run_log_prob_grad(d, 130)
    assert kinds == ("band", "band")
    assert pf["used"] and pb["used"]
    empty = {"eye": (0, 0), "replicated": (0, 0), "predict": (0, 3), "gap": (2, 0)}[zkind]
    assert (pf["nempty"], pb["nempty"]) == empty, (pf, pb)
    check_log_prob_grad(orc, d, lp, G, V)
    C = 144
    with context(d) as ctx:
        u, flags, probs = run_chains(ctx, d, C)
        assert ctx.last_kernels() == ("band", "band")
        _assert_band(ctx, C, paired=False)
    check_chains(orc, d, u, flags, probs, tile_columns(C))


# ---------------------------------------------------------------- e) the bench's shapes
def test_bench_shapes_chain_by_chain(orc):
    """n = Q = 5000 gaussian-identity: 1024 chains paired (the benchmark's configuration) and 128 streamed (one rank of
    the 8-GPU job).  ZL for the oracle is the device's own factor (ctx.gen_D(chol=True)): the oracle's Cholesky at
    this size takes tens of seconds, and the device factor is pinned against it elsewhere (test_gpu_fullsize)"""
    d = synth.geospatial(5000)
    d["seed"] = 0
    vp = d["sigma"]
    ctx = context(d)
    try:
        L = ctx.gen_D(d["theta"], chol=True)
        for C, paired, chains in ((1024, True, [0, 511, 1023]), (128, False, [0, 127])):
            diag, flags, probs = ctx.hmc_sample(d["beta"], vp, WARM, C, LAM, MS, TA, SEED, chains=C, iter_idx=IT,
                                                adapt=ADAPT, want_trace=True)
            assert ctx.last_kernels() == ("band", "band")
            _assert_band(ctx, C, paired=paired)
            u = ctx.get_u()
            xb = d["X"] @ d["beta"]
            for c in chains:
                so, fo, po, _ = orc.hmc_chain(xb, L, d["y"], vp, 7, WARM, 1, LAM, MS, TA, SEED, chain_id=c,
                                              iter_idx=IT, adapt=ADAPT)
                assert np.array_equal(flags[c], fo), (C, c)
                assert np.abs(probs[c] - po).max() < 1e-9, (C, c)
                uo = L @ so[:, 1:]
                assert np.abs(u[:, c:c + 1] - uo).max() < 1e-8 * max(1.0, np.abs(uo).max()), (C, c)
    finally:
        ctx.close()


# ---------------------------------------------------------------- f) one context, several chain counts
def test_context_reuse_across_chain_counts(monkeypatch):
    """plans are cached per column-tile count (BandPlan::by_gn) and the sampler state is re-allocated per chain count:
    one context sampling 1921, 130, 5, 1 and 1930 chains in turn, then again after update_L at a second theta, gives
    the same bits as a fresh context for every call"""
    monkeypatch.delenv("GLMMR_MCML_SKINNY", raising=False)
    d = design("binomial", "logit", 2000)
    theta2 = np.array([0.08, 0.15])
    counts = (1921, 130, 5, 1, 1930)
    seq = []
    with context(d) as ctx:
        for C in counts:
            seq.append(run_chains(ctx, d, C))
        ctx.update_L(theta2)
        for C in (130, 1921):
            seq.append(run_chains(ctx, d, C))
    fresh = []
    for C in counts:
        with context(d) as ctx:
            fresh.append(run_chains(ctx, d, C))
    d2 = dict(d, theta=theta2)
    for C in (130, 1921):
        with context(d2) as ctx:
            fresh.append(run_chains(ctx, d2, C))
    for k, (a, b) in enumerate(zip(seq, fresh)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), k
