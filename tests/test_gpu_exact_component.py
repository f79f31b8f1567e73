"""Component-wise exact conditional draws on the sparse operator (csrc/hmc_exact_comp.h, Context.set_draws("exact_component") /
Context.exact_sample(operator="component")) on the GPU.

The reference is the dense float64 twin tests/exact_gaussian_twin.py (pinned to extended precision on these designs by
test_exact_component_designs_cpu.py, which also shows that M is block diagonal over the components and that a per-component
evaluation equals the twin to rounding).  Every positive case first asserts that the sparse operator is active, that the plan
hook reports the path applicable with the design's (components, most variables, most observations), and afterwards that
last_kernels() names the path.

1. parity with the twin at 1e-10 max|want| (the bound of test_gpu_exact_gaussian.py) at 4, 80 and 130 columns -- below one
   block of 64, past one, past two with a ragged last -- on the smallest designs at which each branch of the two factor
   kernels and of the draw kernel can go wrong (DESIGNS);
2. the mean is the stationary point of the density the device's own log_prob_grad evaluates;
3. the dispatch of hmc_sample under the third mode, where it is honoured and where it is ignored;
4. the RNG addressing;
5. the full driver and the caller's keyword."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_gaussian_twin as tw
from glmmrmcml_amd import _lib, api, synth
from test_gpu_exact_gaussian import EXACT_DIAG, _gaussian_cluster_design, _hmc
from test_gpu_la_component_wide import rct_wide, wide_design
from test_gpu_sparse_products import context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240601
G = ("gaussian", "identity")
COMP = ("exact_component", "exact_component")

# design -> what it exercises; all gaussian / identity.  (wide_design falls through to la_design for the first eight)
DESIGNS = {
    "tiny": "3 variables",
    "rct": "the one-wave factor form",
    "sw_long_ragged": "200 observations per component: the four-wave form by rule",
    "sw_blk16": "a non-diagonal L",
    "dup": "a local column twice in a row",
    "empty_row": "an observation without entries",
    "sw_short_drop": "an empty component",
    "cap32": "32 variables, the narrow cap",
    "rct32": "33 variables",
    "rct63": "64 variables",
    "rct64": "65 variables",
    "rct127": "128 variables, the cap",
    "paired_ar1": "48 variables, two covariance blocks in one component",
}
SIGMAS = {name: (0.8, 0.2) if name in ("rct", "cap32", "rct127") else (0.8,) for name in DESIGNS}
MEAN_DESIGNS = ("rct", "sw_blk16", "rct41")
RULE_WAVES = {"rct": 1, "sw_long_ragged": 4}        # the form cp_waves picks; the test also forces the other one


def make(name):
    """-> (design, (components, most variables, most observations))"""
    return wide_design(name, *G)


def open_ctx(d, monkeypatch, waves=None):
    if waves is None:
        monkeypatch.delenv("GLMMR_MCML_LA_WAVES", raising=False)
    else:
        monkeypatch.setenv("GLMMR_MCML_LA_WAVES", str(waves))
    return context(d, monkeypatch, None)


def assert_applicable(ctx, counts, cols, waves=None):
    assert ctx.sparse_plan(cols)["active"]
    p = ctx.exact_component_plan()
    assert p["applicable"], p
    assert (p["ncomp"], p["max_vars"], p["max_rows"]) == tuple(counts), p
    assert p["factor_waves"] == (waves if waves is not None else (4 if counts[1] > 32 or counts[2] >= 128 else 1)), p
    assert 0 < p["draw_lds_bytes"] <= 160 * 1024 and 0 < p["factor_bytes"] <= 8 * 128 * ctx.Q, p
    return p


@pytest.fixture(scope="module")
def normals(orc):
    """tw.normals for (Q, chains, nsamp) at SEED, chain_offset 3, iter_idx 2: computed once, returned read-only"""
    cache = {}

    def get(Q, chains, nsamp):
        key = (Q, chains, nsamp)
        if key not in cache:
            z = tw.normals(orc, Q, SEED, chains, nsamp, chain_offset=3, iter_idx=2)
            z.setflags(write=False)
            cache[key] = z
        return cache[key]
    return get


def check_parity(orc, normals, monkeypatch, name, sigma, waves=None):
    d, counts = make(name)
    Q = d["Q"]
    L = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    with open_ctx(d, monkeypatch, waves) as ctx:
        for chains, nsamp in tw.COLUMNS:
            ncols = tw.layout(chains, nsamp)[2]
            assert_applicable(ctx, counts, ncols, waves)
            diag = ctx.exact_sample(d["beta"], sigma, nsamp, SEED, chains=chains, chain_offset=3, iter_idx=2,
                                    operator="component")
            assert ctx.last_kernels() == COMP
            got = ctx.get_u()
            want, _ = tw.twin(d["Z"], L, d["X"], d["y"], d["beta"], sigma, normals(Q, chains, nsamp))
            assert got.shape == want.shape == (Q, ncols)
            err = np.abs(got - want).max() / np.abs(want).max()
            print("%s sigma %.1f, %d columns: |got - want| / |want| = %.2e" % (name, sigma, ncols, err))
            assert err <= 1e-10
            assert diag == EXACT_DIAG


# ---------------------------------------------------------------- 1. parity with the twin
@pytest.mark.parametrize("name,sigma", [(n, s) for n in DESIGNS for s in SIGMAS[n]])
def test_component_draws_match_the_twin(orc, normals, monkeypatch, name, sigma):
    check_parity(orc, normals, monkeypatch, name, sigma)


@pytest.mark.parametrize("name", list(RULE_WAVES))
def test_the_other_factor_form_matches_the_twin(orc, normals, monkeypatch, name):
    check_parity(orc, normals, monkeypatch, name, 0.8, waves=5 - RULE_WAVES[name])


# ---------------------------------------------------------------- 2. same target as the HMC path
@pytest.mark.parametrize("name", MEAN_DESIGNS)
def test_mean_is_the_stationary_point_of_the_sampled_density(orc, monkeypatch, name):
    """inj_z = 0: every column is L mu*; the device's own log_grad (what the HMC path integrates) vanishes there"""
    d, counts = make(name)
    Q, sigma = d["Q"], 0.8
    L = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    b = (d["Z"] @ L).T @ (d["y"] - d["X"] @ d["beta"]) / sigma ** 2
    with open_ctx(d, monkeypatch) as ctx:
        assert_applicable(ctx, counts, 4)
        ctx.exact_sample(d["beta"], sigma, 3, SEED, inj_z=np.zeros((Q, 4)), operator="component")
        assert ctx.last_kernels() == COMP
        u = ctx.get_u()
        assert u.shape == (Q, 4) and np.abs(u - u[:, :1]).max() <= 1e-12 * np.abs(u).max()
        v = np.linalg.solve(L, u)
        _, grad = ctx.log_prob_grad(d["beta"], sigma, v)
    print("%s: |grad| / |b| = %.2e" % (name, np.abs(grad).max() / np.abs(b).max()))
    assert np.abs(grad).max() <= 1e-10 * np.abs(b).max()


# ---------------------------------------------------------------- 3. dispatch
def test_hmc_sample_dispatches_to_the_component_path_and_back(monkeypatch):
    d, counts = make("rct")
    with open_ctx(d, monkeypatch) as plain:                # a context that never heard of the switch
        diag0, flags0, probs0 = _hmc(plain, d, sigma=0.8)
        u0 = plain.get_u()
        assert "exact_component" not in plain.last_kernels() and plain.exact_component_plan()["requested"] == "hmc"
    with open_ctx(d, monkeypatch) as ctx:
        assert_applicable(ctx, counts, 40)
        ctx.exact_sample(d["beta"], 0.8, 40, 5, chains=20, iter_idx=1, operator="component")
        assert ctx.last_kernels() == COMP
        ue = ctx.get_u()
        ctx.set_draws("exact_component")
        assert ctx.exact_component_plan()["requested"] == "exact_component"
        assert ctx.draws_plan() == dict(requested="exact_component", applicable=False, Q=d["Q"],
                                        m_bytes=8 * 32 * -(-d["Q"] // 32) * d["Q"])
        diag, flags, probs = _hmc(ctx, d, sigma=0.8)
        assert ctx.last_kernels() == COMP
        assert np.array_equal(ctx.get_u(), ue)
        assert flags.shape == (20, 12 + 2) and np.all(flags == 1) and np.all(probs == 1.0)
        assert diag == EXACT_DIAG
        assert not np.array_equal(ue, u0)
        ctx.set_draws("hmc")
        diag1, flags1, probs1 = _hmc(ctx, d, sigma=0.8)
        assert np.array_equal(ctx.get_u(), u0) and np.array_equal(flags1, flags0) and np.array_equal(probs1, probs0)
        assert diag1 == diag0 and "exact_component" not in ctx.last_kernels()


def test_on_the_dense_operator_the_mode_is_the_dense_exact_path():
    d = synth.geospatial(150)
    out = []
    for mode in ("exact", "exact_component"):
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            ctx.set_draws(mode)
            assert not ctx.exact_component_plan()["applicable"] and ctx.draws_plan()["applicable"]
            diag, flags, probs = _hmc(ctx, d)
            assert ctx.last_kernels() == ("exact", "exact") and diag == EXACT_DIAG
            out.append((ctx.get_u(), flags, probs))
    assert all(np.array_equal(a, b) for a, b in zip(*out))


@pytest.mark.parametrize("which", ["binomial", "gaussian, components of 129 variables"])
def test_request_is_ignored_where_the_path_does_not_apply(which, monkeypatch):
    if which == "binomial":
        d, sigma = synth.cluster_rct(ncl=6, nt=4, nind=5), 1.0
    else:
        d, sigma = rct_wide(128, *G)[0], 0.8
    out = []
    for mode in ("hmc", "exact_component"):
        with open_ctx(d, monkeypatch) as ctx:
            ctx.set_draws(mode)
            assert ctx.sparse_plan(20)["active"]
            p = ctx.exact_component_plan()
            assert not p["applicable"] and p["requested"] == mode and not ctx.draws_plan()["applicable"]
            diag, flags, probs = _hmc(ctx, d, sigma=sigma)
            assert not set(ctx.last_kernels()) & {"exact", "exact_component"}
            out.append((ctx.get_u(), flags, probs, diag))
            if mode == "exact_component":
                with pytest.raises(_lib.McmlError):
                    ctx.exact_sample(d["beta"], sigma, 40, 5, chains=20, operator="component")
                assert np.array_equal(ctx.get_u(), out[-1][0])          # the refused call left the samples alone
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]


def test_environment_default_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from glmmrmcml_amd import api\n"
            "from test_gpu_exact_gaussian import _gaussian_cluster_design\n"
            "d = _gaussian_cluster_design()\n"
            "print(api.get_default_draws())\n"
            "with api.Context(d['cov'], d['data'], d['eff_range'], d['Z'], d['X'], d['y'], d['family'], d['link']) as ctx:\n"
            "    ctx.update_L(d['theta'])\n"
            "    ctx.hmc_sample(d['beta'], d['sigma'], 5, 8, 0.4, 4, 0.9, 3, chains=8)\n"
            "    print(ctx.exact_component_plan()['requested'], *ctx.last_kernels())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, GLMMR_MCML_DRAWS="exact_component"),
                       capture_output=True, text=True, timeout=120)
    assert r.stdout.strip().splitlines()[-2:] == ["exact_component", "exact_component exact_component exact_component"], r.stdout


# ---------------------------------------------------------------- 4. RNG addressing
def test_rng_addressing(monkeypatch):
    d, counts = make("rct")
    Q = d["Q"]

    def draw(ctx, nsamp, **kw):
        ctx.exact_sample(d["beta"], 0.8, nsamp, 11, operator="component", **kw)
        assert ctx.last_kernels() == COMP
        return ctx.get_u()
    with open_ctx(d, monkeypatch) as ctx:
        assert_applicable(ctx, counts, 40)
        a = draw(ctx, 40, chains=40, iter_idx=1)
        assert np.array_equal(draw(ctx, 40, chains=40, iter_idx=1), a)           # the same seed reproduces bits
        b = draw(ctx, 40, chains=40, iter_idx=2)
        assert a.shape == b.shape == (Q, 40)
        assert all(not np.array_equal(a[:, j], b[:, j]) for j in range(40))      # another iteration: every column
        assert len({a[:, j].tobytes() for j in range(40)}) == 40                 # no two columns equal
        one = draw(ctx, 6)                                                       # one chain: column 0 is a draw too
        assert one.shape == (Q, 7) and len({one[:, j].tobytes() for j in range(7)}) == 7
    halves = []
    for off in (0, 20):
        with open_ctx(d, monkeypatch) as ctx:
            halves.append(draw(ctx, 20, chains=20, chain_offset=off, iter_idx=1))
    assert np.abs(np.hstack(halves) - a).max() <= 1e-12 * np.abs(a).max()


# ---------------------------------------------------------------- 5. driver and caller
def _driver_design():
    d = _gaussian_cluster_design()
    return dict(d, start=np.r_[d["beta"], d["theta"], d["sigma"]])


def test_mcml_full_in_component_mode_equals_the_hand_run_loop(monkeypatch):
    d = _driver_design()
    start, P = d["start"], d["X"].shape[1]
    with open_ctx(d, monkeypatch) as ctx:
        ctx.set_draws("exact_component")
        assert ctx.sparse_plan(64)["active"] and ctx.exact_component_plan()["applicable"]
        got = ctx.mcml_full(start, mcnr=True, m=64, maxiter=2, chains=64, seed=7)
        gu = ctx.get_u()
        assert ctx.last_kernels() == COMP
    with open_ctx(d, monkeypatch) as ctx:
        ctx.set_draws("exact_component")
        beta, theta, sigma = start[:P].copy(), start[P:P + 2].copy(), float(start[P + 2])
        for it in (1, 2):
            ctx.update_L(theta)
            ctx.hmc_sample(beta, sigma, 500, 64, 0.05, 100, 0.9, seed=7, chains=64, iter_idx=it)
            assert ctx.last_kernels() == COMP
            u = ctx.get_u()
            r = ctx.mcml_optim(np.r_[beta, theta, sigma], mcnr=True)
            beta, theta, sigma = r["beta"], r["theta"], r["sigma"]

    def rel(a, b):
        return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())
    print("beta %.2e theta %.2e sigma %.2e u %.2e" % (rel(got["beta"], beta), rel(got["theta"], theta),
                                                      rel(got["sigma"], sigma), rel(gu, u)))
    assert got["iters"] == 2
    assert rel(got["beta"], beta) <= 1e-9 and rel(got["theta"], theta) <= 1e-9 and rel(got["sigma"], sigma) <= 1e-9
    assert rel(gu, u) <= 1e-9


def test_caller_keyword_sets_and_restores_the_process_default(monkeypatch):
    from glmmrmcml_amd.model import ModelMCML
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = _driver_design()
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                  var_par=d["sigma"])
    m.mcmc_options.update(warmup=20, samps=64, lambda_=0.5, maxsteps=8)
    assert api.get_default_draws() == "hmc"
    kw = dict(verbose=False, max_iter=2, seed=7, chains=64, se_method="none", options=dict(maxfun=40))
    fit = m.MCML(d["y"], draws="exact_component", **kw)
    assert api.get_default_draws() == "hmc"
    api.set_default_draws("exact_component")
    try:
        same = m.MCML(d["y"], **kw)                       # the default itself set: the same fit
        assert api.get_default_draws() == "exact_component"
        other = m.MCML(d["y"], draws="hmc", **kw)
        assert api.get_default_draws() == "exact_component"
    finally:
        api.set_default_draws("hmc")
    assert np.array_equal(fit["theta"], same["theta"]) and np.array_equal(fit["re_samps"], same["re_samps"])
    assert not np.array_equal(fit["re_samps"], other["re_samps"])
    with pytest.raises(KeyError):
        m.MCML(d["y"], draws="gibbs", **kw)
    assert api.get_default_draws() == "hmc"
